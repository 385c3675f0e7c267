"""GPU parity of batched decoding (qeft_amd/batch.py, csrc/decode_batch.hip): the batched attention against an fp64 reference
per row and against one-row launches on the same slot, batched token begin / end against their one-sequence forms, the engine
against the single-sequence engine on each sequence alone, and continuous batching against decoding each prompt alone."""
import dataclasses

import pytest
import torch

from util import REL_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 128


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from qeft_amd import _lib
    return _lib.lib(), _lib.check


def _rot(x, c, s):          # x [..., 128], c / s [..., 64]: neox-style rotary, as the kernels
    a, b = x[..., :64], x[..., 64:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


# ragged positions of one launch: 0, 1, 15, 16, 255, max_seq - 1, a done row, and 100
MAX_SEQ = 272
POSITIONS = [0, 1, 15, 16, 255, MAX_SEQ - 1, 37, 100]
DONE_ROW = 6
SLOTS = [7, 2, 9, 0, 5, 3, 8, 1]                 # permuted, non-contiguous (slots 4 and 6 unused) of 10


@pytest.mark.parametrize("heads,kv", [(32, 32), (40, 40), (64, 8)])
def test_batched_attention_vs_fp64_and_one_row(heads, kv):
    lib, ck = _lib()
    n_slots = 10
    g = torch.Generator().manual_seed(heads + kv)
    ang = torch.randn(MAX_SEQ, 64, generator=g)
    cos, sin = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()
    ws = torch.zeros(max(lib.qeft_attn_batch_workspace_bytes(heads, 8, 8), 16) // 4, device=DEV)
    ws1 = torch.zeros(max(lib.qeft_attn_workspace_bytes(heads, 8), 16) // 4, device=DEV)
    nq = (heads + 2 * kv) * HD
    kc0 = (torch.randn(n_slots, kv, MAX_SEQ, HD, generator=g) * 0.5).half().to(DEV)
    vc0 = (torch.randn(n_slots, kv, MAX_SEQ, HD, generator=g) * 0.5).half().to(DEV)
    pos_tab = torch.full((n_slots,), 3, dtype=torch.int32)
    done = torch.zeros(n_slots, dtype=torch.int32)
    for r, s in enumerate(SLOTS):
        pos_tab[s] = POSITIONS[r]
    done[SLOTS[DONE_ROW]] = 1
    pos_d, done_d = pos_tab.to(DEV), done.to(DEV)
    slots_d = torch.tensor(SLOTS, dtype=torch.int32, device=DEV)
    for m in range(1, 9):
        qkv = torch.randn(m, nq, generator=g).half().to(DEV)
        qp = qkv.data_ptr()
        for split in (1, 2, 4, 8):
            runs = []
            for _ in range(2):                       # two runs from the same caches: bitwise equal
                kc, vc = kc0.clone(), vc0.clone()
                out = torch.full((m, heads * HD), 7.0, dtype=torch.float16, device=DEV)
                ck(lib.qeft_rope_attn_decode_batch(qp, qp + heads * HD * 2, qp + (heads + kv) * HD * 2, nq, cos.data_ptr(),
                                                   sin.data_ptr(), 64, MAX_SEQ, kc.data_ptr(), vc.data_ptr(), slots_d.data_ptr(),
                                                   pos_d.data_ptr(), done_d.data_ptr(), None, out.data_ptr(), heads * HD, ws.data_ptr(),
                                                   split, n_slots, heads, kv, MAX_SEQ, m, _st()))
                runs.append((out, kc, vc))
            torch.cuda.synchronize()
            (out, kc, vc), (out2, kc2, vc2) = runs
            assert torch.equal(out, out2) and torch.equal(kc, kc2) and torch.equal(vc, vc2), (m, split)
            # slots no row of this launch serves: every byte unchanged
            for s in range(n_slots):
                if s not in SLOTS[:m] or (DONE_ROW < m and s == SLOTS[DONE_ROW]):
                    assert torch.equal(kc[s], kc0[s]) and torch.equal(vc[s], vc0[s]), (m, split, s)
            qf, K, V = qkv.double().cpu(), kc.double().cpu(), vc.double().cpu()
            for r in range(m):
                s, p = SLOTS[r], POSITIONS[r]
                if r == DONE_ROW:
                    assert (out[r] == 0).all(), (m, split)
                    continue
                # one-row launch on a copy of the same slot: V rows exactly, K rows within one fp16 ulp
                k1, v1 = kc0[s].clone(), vc0[s].clone()
                o1 = torch.zeros(heads * HD, dtype=torch.float16, device=DEV)
                p1 = torch.tensor([p], dtype=torch.int32, device=DEV)
                q1 = qkv[r].contiguous()
                ws1.zero_()                              # (the one-row workspace keeps its counters behind records sized by the split)
                ck(lib.qeft_rope_attn_decode(q1.data_ptr(), q1.data_ptr() + heads * HD * 2, q1.data_ptr() + (heads + kv) * HD * 2,
                                             cos.data_ptr(), sin.data_ptr(), MAX_SEQ, k1.data_ptr(), v1.data_ptr(), p1.data_ptr(), None,
                                             o1.data_ptr(), ws1.data_ptr(), split, heads, kv, MAX_SEQ, _st()))
                torch.cuda.synchronize()
                assert torch.equal(vc[s], v1), (m, split, r)
                assert torch.equal(kc[s][:, :p], k1[:, :p]) and torch.equal(kc[s][:, p + 1:], k1[:, p + 1:]), (m, split, r)
                dk = (kc[s][:, p].float() - k1[:, p].float()).abs()
                assert (dk <= k1[:, p].float().abs() * 2.0 ** -10 + 2.0 ** -24).all(), (m, split, r, dk.max().item())
                # fp64 reference over keys [0, p] of the slot (the kernel's roundings: q rotated, scaled to fp16; k rotated to fp16)
                c, sn = cos.double().cpu()[p], sin.double().cpu()[p]
                q = _rot(qf[r, :heads * HD].view(heads, HD), c, sn)
                q = (q * HD ** -0.5).half().double()
                grp = heads // kv
                Kh = K[s, :, :p + 1].repeat_interleave(grp, 0)          # [heads, p + 1, 128]
                Vh = V[s, :, :p + 1].repeat_interleave(grp, 0)
                pr = torch.softmax(torch.einsum("hd,hpd->hp", q, Kh), -1)
                ref = torch.einsum("hp,hpd->hd", pr, Vh).reshape(-1)
                got = out[r].double().cpu()
                assert (got - ref).abs().max().item() < 2e-3 + 2e-3 * ref.abs().max().item(), (heads, m, split, r)
                assert (out[r].float() - o1.float()).abs().max().item() < 4e-3, (m, split, r)


def test_batched_token_begin_equals_token_begin_m():
    lib, ck = _lib()
    g = torch.Generator().manual_seed(2)
    hidden, vocab, max_seq, n_slots = 4096, 1000, 64, 10
    embed = torch.randn(vocab, hidden, generator=g).half().to(DEV)
    gamma = (torch.rand(hidden, generator=g) + 0.5).half().to(DEV)
    rope_tab = torch.randn(max_seq, 128, generator=g).to(DEV)
    nb = lib.qeft_token_begin_norm_blocks(hidden)
    m = 8
    toks = torch.randint(0, vocab, (m,), generator=g).to(DEV)
    pos = torch.randint(0, max_seq, (n_slots,), generator=g).int().to(DEV)
    slots = torch.tensor(SLOTS, dtype=torch.int32, device=DEV)
    h, xn = torch.zeros(m, hidden, device=DEV), torch.zeros(m, hidden, dtype=torch.float16, device=DEV)
    ssq, rope = torch.zeros(m, nb, device=DEV), torch.zeros(m, 128, device=DEV)
    ck(lib.qeft_token_begin_norm_batch(embed.data_ptr(), toks.data_ptr(), rope_tab.data_ptr(), slots.data_ptr(), pos.data_ptr(),
                                       h.data_ptr(), rope.data_ptr(), gamma.data_ptr(), xn.data_ptr(), ssq.data_ptr(), hidden, vocab,
                                       max_seq, n_slots, m, _st()))
    for r in range(m):
        h1, xn1 = torch.zeros(1, hidden, device=DEV), torch.zeros(1, hidden, dtype=torch.float16, device=DEV)
        ssq1, rope1 = torch.zeros(1, nb, device=DEV), torch.zeros(1, 128, device=DEV)
        t1, p1 = toks[r:r + 1].clone(), pos[SLOTS[r]:SLOTS[r] + 1].clone()
        ck(lib.qeft_token_begin_norm_m(embed.data_ptr(), t1.data_ptr(), rope_tab.data_ptr(), p1.data_ptr(), h1.data_ptr(),
                                       rope1.data_ptr(), gamma.data_ptr(), xn1.data_ptr(), ssq1.data_ptr(), hidden, vocab, max_seq, 1, _st()))
        torch.cuda.synchronize()
        for a, b in ((h, h1), (xn, xn1), (ssq, ssq1), (rope, rope1)):
            assert torch.equal(a[r], b[0]), r


def test_batched_token_end_argmax_and_stops():
    lib, ck = _lib()
    g = torch.Generator().manual_seed(5)
    n_slots, cap = 10, 4
    for vocab in (1000, 32000, 1003):
        m = 8
        lg = torch.randn(m, vocab, generator=g).half()
        lg[:3, 17] = 30.0                              # a tie between 17 and 900 in rows 0..2: the lower index wins
        lg[:3, 900] = 30.0
        am = torch.argmax(lg.float(), -1).tolist()
        assert am[:3] == [17] * 3
        slots = torch.tensor(SLOTS, dtype=torch.int32, device=DEV)
        pos = torch.full((n_slots,), 5, dtype=torch.int32)
        limit = torch.full((n_slots,), 100, dtype=torch.int32)
        eos = torch.full((n_slots,), -1, dtype=torch.int32)
        done = torch.zeros(n_slots, dtype=torch.int32)
        eos[SLOTS[1]] = am[1]                          # row 1 emits its EOS
        limit[SLOTS[2]] = 6                            # row 2 reaches its limit
        done[SLOTS[3]] = 2                             # row 3 already stopped
        st = [t.to(DEV) for t in (pos, limit, eos, done)]
        tok = torch.full((m,), -5, dtype=torch.long, device=DEV)
        out = torch.full((m, cap), -9, dtype=torch.long, device=DEV)
        ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
        lgd = lg.to(DEV)
        for _ in range(2):
            ck(lib.qeft_token_end_batch(lgd.data_ptr(), slots.data_ptr(), tok.data_ptr(), st[0].data_ptr(), st[1].data_ptr(),
                                        st[2].data_ptr(), st[3].data_ptr(), out.data_ptr(), ctr.data_ptr(), vocab, cap, n_slots, m, _st()))
        torch.cuda.synchronize()
        pos2, done2 = st[0].cpu(), st[3].cpu()
        assert ctr.tolist() == [2, 0]
        for r in range(m):
            s = SLOTS[r]
            if r == 3:
                assert out[r, :2].tolist() == [-1, -1] and tok[r].item() == -5 and pos2[s] == 5
            elif r in (1, 2):                          # stopped after the first call
                assert out[r, :2].tolist() == [am[r], -1] and tok[r].item() == am[r] and pos2[s] == 6
                assert done2[s] == (1 if r == 1 else 2)
            else:
                assert out[r, :2].tolist() == [am[r], am[r]] and tok[r].item() == am[r] and pos2[s] == 7 and done2[s] == 0
        assert out[:, 2:].eq(-9).all()


# ---- the engine --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["7b", "70b"])
def model2(request):
    from qeft_amd.llama import LLAMA2_7B, LLAMA2_70B, QuantLlama
    base = {"7b": LLAMA2_7B, "70b": LLAMA2_70B}[request.param]
    shape = dataclasses.replace(base, n_layers=2, max_seq=256, name=base.name + "-2layers")
    model = QuantLlama(shape, DEV, seed=3, fast_init=True)
    yield request.param, model
    del model
    torch.cuda.empty_cache()


def _prompts(vocab, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g) for n in lengths]


_SINGLE = {}


def _single(model, prompt, feed=None, n=0):
    """prefill + DecodeEngine on one sequence alone: (tokens, fp32 logits per step).  feed: teacher-forced tokens instead."""
    key = (id(model), tuple(prompt.tolist()), tuple(feed.tolist()) if feed is not None else None, n)
    if key not in _SINGLE:
        _SINGLE[key] = _single_run(model, prompt, feed, n)
    return _SINGLE[key]


def _single_run(model, prompt, feed, n):
    from qeft_amd.llama import DecodeEngine, prefill
    eng = DecodeEngine(model, use_graph=True)
    logits = prefill(model, prompt.to(DEV), engine=eng)
    toks, rows = [int(torch.argmax(logits[-1]).item())], []
    eng.greedy = feed is None
    eng.tok.fill_(toks[0])
    for i in range(len(feed) if feed is not None else n):
        if feed is not None:
            eng.tok.fill_(int(feed[i]))
        eng.step()
        rows.append(eng.logits[0].float().clone())
        toks.append(int(eng.tok.item()))
    return toks, rows


def _near_tie(row, tol=REL_TOL):
    top2 = row.topk(2).values
    return (top2[0] - top2[1]).item() <= tol * row.abs().max().item() + 2.0 ** -10 * top2[0].abs().item()


def _same_or_near_tie(got, ref, ref_rows, first_ok=True):
    """Greedy tokens must equal the single-sequence ones; at the first mismatch the reference's top-2 margin must be a near-tie
    (comparison stops there).  ref_rows[j] are the logits that produced ref[j + 1]."""
    assert got[0] == ref[0] or not first_ok
    for j in range(1, min(len(got), len(ref))):
        if got[j] != ref[j]:
            assert _near_tie(ref_rows[j - 1]), f"token {j}: {got[j]} vs {ref[j]}, not a near-tie"
            return j
    assert len(got) == len(ref), (len(got), len(ref))
    return None


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_teacher_forced_rows_match_single_sequence(model2, use_graph):
    from qeft_amd.batch import BatchDecodeEngine
    from qeft_amd.llama import DecodeEngine
    name, model = model2
    vocab = model.shape.vocab
    prompts = _prompts(vocab, [5, 17, 9, 30], seed=1)
    feeds = _prompts(vocab, [12, 12, 12, 12], seed=2)
    eng = DecodeEngine(model, use_graph=True)
    snap = ([k.clone() for k in eng.kc], [v.clone() for v in eng.vc], eng.pos.clone(), eng.host_pos)
    be = BatchDecodeEngine(eng, max_batch=4, use_graph=use_graph)
    start = [0, 0, 3, 7]                             # admitted at different times (passes already run)
    slots, got, i = {}, {j: [] for j in range(4)}, 0
    for step in range(20):
        for j in range(4):
            if start[j] == step:
                slots[j] = be.admit(prompts[j], 100)
        live = [j for j in slots if len(got[j]) < 12]
        if not live:
            break
        be.step({slots[j]: int(feeds[j][len(got[j])]) for j in live})
        for j in live:
            got[j].append(be.logits(slots[j]).float().clone())
    torch.cuda.synchronize()
    worst = 0.0
    for j in range(4):
        _, ref = _single(model, prompts[j], feed=feeds[j])
        ref, g = torch.stack(ref), torch.stack(got[j])
        worst = max(worst, (g - ref).abs().max().item() / ref.abs().max().item())
    print(f"[batch {name} graph={use_graph}] teacher-forced max|d|/max|ref| = {worst:.3e}")
    assert worst < REL_TOL, worst
    # isolation: the engine's own caches and position are untouched
    assert all(torch.equal(a, b) for a, b in zip(eng.kc, snap[0])) and all(torch.equal(a, b) for a, b in zip(eng.vc, snap[1]))
    assert torch.equal(eng.pos, snap[2]) and eng.host_pos == snap[3]


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_greedy_tokens_match_single_sequence(model2, use_graph):
    from qeft_amd.batch import BatchDecodeEngine
    from qeft_amd.llama import DecodeEngine
    name, model = model2
    prompts = _prompts(model.shape.vocab, [3, 40, 11, 25, 7], seed=3)
    be = BatchDecodeEngine(DecodeEngine(model, use_graph=True), max_batch=5, use_graph=use_graph)
    slots = [be.admit(p, 64) for p in prompts]
    be.run(63)
    assert be.finished() == {s: "length" for s in slots}
    for j, s in enumerate(slots):
        ref, rows = _single(model, prompts[j], n=63)
        got = be.tokens(s)
        assert len(got) == 64
        _same_or_near_tie(got, ref, rows)
        assert be.table.get(s).pos == len(prompts[j]) + 63


def test_engine_batch_invariance_and_eager_equals_graph(model2):
    """For a fixed m, a row's logits are bitwise independent of the other rows and of its slot / row; eager == graph."""
    from qeft_amd.batch import BatchDecodeEngine
    from qeft_amd.llama import DecodeEngine
    name, model = model2
    vocab = model.shape.vocab
    target = _prompts(vocab, [21], seed=4)[0]
    feed = _prompts(vocab, [6], seed=5)[0]
    results = []
    for case, (others, graph) in enumerate([(_prompts(vocab, [4, 9, 30], seed=6), True), (_prompts(vocab, [33, 2, 15], seed=7), True),
                                           (_prompts(vocab, [4, 9, 30], seed=6), False)]):
        be = BatchDecodeEngine(DecodeEngine(model, use_graph=True), max_batch=4, use_graph=graph)
        order = [others[0], target, others[1], others[2]] if case != 1 else [others[0], others[1], others[2], target]
        slots = [be.admit(p, 50) for p in order]
        ts = slots[1] if case != 1 else slots[3]
        rows = []
        for t in feed.tolist():
            be.step({s: (t if s == ts else 5) for s in slots})
            rows.append(be.logits(ts).clone())
        torch.cuda.synchronize()
        results.append(torch.stack(rows))
    assert torch.equal(results[0], results[1]), "a row's logits depend on the other rows or its slot"
    assert torch.equal(results[0], results[2]), "eager and graph passes differ"


def test_engine_stops_inside_a_multi_token_graph(model2):
    """EOS and length stops inside one 8-token graph replay: position, cache and output stay frozen after the stop."""
    from qeft_amd.batch import BatchDecodeEngine
    from qeft_amd.llama import DecodeEngine
    name, model = model2
    prompts = _prompts(model.shape.vocab, [6, 13, 9], seed=8)
    eng = DecodeEngine(model, use_graph=True)
    ref = BatchDecodeEngine(eng, max_batch=3)
    slots = [ref.admit(p, 100) for p in prompts]
    ref.run(8)
    full = [ref.tokens(s) for s in slots]
    # the EOS: the first token of sequence 0 that differs from its first token (emitted at token k_eos >= 1)
    k_eos = next((k for k in range(1, 8) if full[0][k] != full[0][0]), None)
    assert k_eos is not None, f"sequence 0 repeats one token: {full[0]}"
    eos = full[0][k_eos]
    be = BatchDecodeEngine(eng, max_batch=3)
    a = be.admit(prompts[0], 100, eos_id=eos)         # EOS at token k_eos
    b = be.admit(prompts[1], 4)                       # length: 4 tokens
    c = be.admit(prompts[2], 100)
    be.run(8)
    assert list(be.graphs) == [(3, 1, be.MULTI)]      # one multi-token graph, one replay
    assert be.tokens(a) == full[0][:k_eos + 1] and be.tokens(b) == full[1][:4] and be.tokens(c) == full[2][:9]
    assert be.finished() == {a: "eos", b: "length"}
    for s, n_gen, T in ((a, k_eos, 6), (b, 3, 13)):
        p = T + n_gen
        assert int(be.pos[s].item()) == p and be.table.get(s).pos == p
        for li in range(model.shape.n_layers):       # nothing written at or past the stop position
            assert be.kc[li][s][:, p:].eq(0).all() and be.vc[li][s][:, p:].eq(0).all()
    assert be.out[0, :8].tolist()[k_eos:] == [-1] * (8 - k_eos)


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_rows_cross_the_split_switches_and_reuse_a_long_slot(use_graph):
    """Long, ragged rows on a 2048-row cache: prompts of 5, 250, 1530 and 1000 tokens teacher-forced for 12 passes, so that one
    row crosses position 256 and one 1536 inside the run (the pass's split is the longest row's: 4, then 8, which leaves the
    5-token row's splits without keys).  Then the 1530-token slot is released and a 3-token prompt admitted into it, with the old
    sequence's K/V still behind it, for 8 more passes.  Every row against the single-sequence engine on that sequence alone."""
    from qeft_amd.batch import BatchDecodeEngine
    from qeft_amd.llama import DecodeEngine, QuantLlama, tiny_shape
    shape = tiny_shape(n_layers=2, hidden=256, inter=512, n_heads=2, vocab=384, max_seq=2048)
    model = QuantLlama(shape, DEV, seed=11)
    lengths = [5, 250, 1530, 1000]
    prompts = _prompts(shape.vocab, lengths, seed=12)
    feeds = _prompts(shape.vocab, [20, 20, 12, 20], seed=13)
    be = BatchDecodeEngine(DecodeEngine(model, use_graph=True), max_batch=4, use_graph=use_graph)
    slots = [be.admit(p, 100) for p in prompts]
    got = {j: [] for j in range(5)}

    def passes(n, live):
        for _ in range(n):
            be.step({slots[j]: int(feeds[j][len(got[j])]) for j in live})
            for j in live:
                got[j].append(be.logits(slots[j]).float().clone())
    passes(12, [0, 1, 2, 3])
    if use_graph:
        assert {k[:2] for k in be.graphs} == {(4, 4), (4, 8)}, sorted(be.graphs)      # (rows, split): 1530..1535, then 1536..1541
    long_slot = slots[2]
    stale = be.kc[0][long_slot][:, 3:1542].abs().sum().item()
    be.release(long_slot)
    prompts.append(_prompts(shape.vocab, [3], seed=14)[0])
    feeds.append(_prompts(shape.vocab, [8], seed=15)[0])
    slots.append(be.admit(prompts[4], 100))
    assert slots[4] == long_slot and stale > 0
    assert be.kc[0][long_slot][:, 3:1542].abs().sum().item() == stale               # the old sequence's keys are still there
    passes(8, [0, 1, 3, 4])
    if use_graph:
        assert {k[:2] for k in be.graphs} == {(4, 4), (4, 8)}, sorted(be.graphs)      # now the longest row is at 1012..1019: split 4
    torch.cuda.synchronize()
    worst = {}
    for j in range(5):
        _, ref = _single(model, prompts[j], feed=feeds[j][:len(got[j])])
        ref, g = torch.stack(ref), torch.stack(got[j])
        assert torch.isfinite(g).all(), j
        worst[j] = (g - ref).abs().max().item() / ref.abs().max().item()
    print(f"[batch long graph={use_graph}] prompts {lengths} + [3 into the released slot]: teacher-forced max|d|/max|ref| = "
          + ", ".join(f"{worst[j]:.3e}" for j in range(5)))
    assert max(worst.values()) < REL_TOL, worst
    for key in [key for key in _SINGLE if key[0] == id(model)]:      # this model goes away: so do its cached single-sequence runs
        del _SINGLE[key]
    del be, model
    torch.cuda.empty_cache()


def test_generate_batch_continuous():
    from qeft_amd.batch import generate_batch
    from qeft_amd.llama import DecodeEngine, QuantLlama, tiny_shape
    model = QuantLlama(tiny_shape(n_layers=2, hidden=256, inter=512, n_heads=2, vocab=384, max_seq=96), DEV, seed=9)
    lengths = [3, 17, 5, 40, 8, 1, 22, 12, 9, 30, 2, 60]
    prompts = _prompts(384, lengths, seed=10)
    N = 24
    refs = [_single(model, p, n=N - 1) for p in prompts]
    # an EOS that some sequences emit
    counts = {}
    for toks, _ in refs:
        for t in toks[1:]:
            counts[t] = counts.get(t, 0) + 1
    eos = max(counts, key=counts.get)
    got = generate_batch(DecodeEngine(model, use_graph=True), prompts, N, eos_id=eos, max_batch=4)
    n_eos = 0
    for j, (toks, rows) in enumerate(refs):
        ref = toks[:toks.index(eos) + 1] if eos in toks else toks
        n_eos += eos in toks
        _same_or_near_tie(got[j], ref, rows)
    assert n_eos >= 1
