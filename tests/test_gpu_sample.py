"""GPU checks of sampled decoding (csrc/decode_sample.hip, qeft_amd/sampling.py): the kernel against the fp64 filter and the
numpy Philox draw, the distribution of 20 000 draws, invariance (rows, m, replays; temperature 0 equals the argmax token ends
bit for bit), and the engines: DecodeEngine.set_sampling and sampled rows of BatchDecodeEngine."""
import dataclasses

import numpy as np
import pytest
import torch

from sampling_ref import cdf_interval, draw_u, filter_probs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOTS = [7, 2, 9, 0, 5, 3, 8, 1]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from qeft_amd import _lib
    return _lib.lib(), _lib.check


def _f32(x):
    return float(np.float32(x))


def _rec(T, k, p, seed):
    from qeft_amd.sampling import SamplingParams
    return SamplingParams(T, k, p, seed).record()


def _run_sample(lg, recs, positions):
    """qeft_sample over fp16 rows lg [m][vocab] (host), records [m][8], positions [m] -> tokens (host list)."""
    lib, ck = _lib()
    m, vocab = lg.shape
    x = lg.to(DEV)
    rec = torch.tensor(recs, dtype=torch.int32, device=DEV)
    pos = torch.tensor(positions, dtype=torch.int32, device=DEV)
    out = torch.full((m,), -7, dtype=torch.long, device=DEV)
    ck(lib.qeft_sample(x.data_ptr(), vocab, m, rec.data_ptr(), pos.data_ptr(), out.data_ptr(), _st()))
    torch.cuda.synchronize()
    return out.cpu().tolist()


def _rows(vocab, g):
    """random and adversarial fp16 rows"""
    rows = [torch.randn(vocab, generator=g) * 2,                                      # random
            torch.randint(0, 3, (vocab,), generator=g).float() * -0.5,                # mass ties on 3 values
            torch.randn(vocab, generator=g) * 0.5,                                    # one dominant logit
            torch.full((vocab,), 0.25)]                                               # all equal
    rows[2][vocab // 3] = 12.0
    r = torch.randn(vocab, generator=g) * 1.5                                         # NaN / -inf / -0 entries
    r[torch.randint(0, vocab, (max(1, vocab // 50),), generator=g)] = float("nan")
    r[torch.randint(0, vocab, (max(1, vocab // 50),), generator=g)] = float("-inf")
    r[torch.randint(0, vocab, (max(1, vocab // 100),), generator=g)] = -0.0
    rows.append(r)
    return torch.stack(rows).half()


GRID = [(T, k, p) for T in (0, 0.3, 1, 1.7) for k in (0, 1, 40, "V+5") for p in (1, 0.95, 0.5, 1e-6)]


@pytest.mark.parametrize("vocab", [32000, 32001, 511, 128256])
def test_kernel_against_fp64_reference(vocab):
    g = torch.Generator().manual_seed(vocab)
    base = _rows(vocab, g)
    n_pos = 3
    lg, recs, pos, meta = [], [], [], []
    for ri in range(base.shape[0]):
        for (T, k, p) in GRID:
            kk = vocab + 5 if k == "V+5" else k
            seed = (ri * 1000003 + len(meta) * 7919) & (2 ** 64 - 1) | (ri << 40)
            for j in range(n_pos):
                lg.append(base[ri])
                recs.append(_rec(T, kk, p, seed))
                pos.append(17 + 1000 * j + len(meta))
            meta.append((ri, T, kk, p, seed))
    toks = _run_sample(torch.stack(lg), recs, pos)
    bad = []
    for i, (ri, T, kk, p, seed) in enumerate(meta):
        l = base[ri].double().numpy()
        kept, pr, margin = filter_probs(l, _f32(T), kk, _f32(p))
        u, _ = draw_u(seed, pos[i * n_pos:(i + 1) * n_pos])
        for j in range(n_pos):
            t = toks[i * n_pos + j]
            if not 0 <= t < vocab:
                bad.append((ri, T, kk, p, "range", t))
                continue
            if T == 0:
                if not kept[t]:
                    bad.append((ri, T, kk, p, "argmax", t, int(np.nonzero(kept)[0][0])))
                continue
            if not kept[t]:
                if margin[t] > 1e-6:
                    bad.append((ri, T, kk, p, "not kept", t))
                continue
            lo, hi = cdf_interval(pr, t)
            if not lo - 1e-6 <= u[j] <= hi + 1e-6:
                if margin.min() > 1e-6:                # (a kept-set boundary within 1e-6 Z shifts the CDF)
                    bad.append((ri, T, kk, p, "cdf", t, lo, hi, u[j]))
    assert not bad, bad[:8]


def test_equal_logits_draw_floor_16u():
    n = 4096
    lg = torch.full((n, 16), 1.5).half()
    seed = 0x5eed_0000_1234_abcd
    toks = _run_sample(lg, [_rec(1.0, 0, 1.0, seed)] * n, list(range(n)))
    u, _ = draw_u(seed, range(n))
    assert toks == np.floor(16 * u).astype(int).tolist()


# The smallest shapes with every operand in an exact-size allocation of its own (a child process with
# PYTORCH_NO_CUDA_MEMORY_CACHING=1, as tests/test_gpu_zz_alloc_guard.py): a read past the row, the record, the positions or the
# slot state would reach the end of its mapping instead of landing inside a pooled segment.  vocab 1 and 7 (register-held keys,
# the scalar tail path) and 32769 (the re-reading instantiation, odd length), m = 1, greedy and sampled records.
ALLOC_CHILD = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np, torch
from qeft_amd import _lib
from qeft_amd.sampling import SamplingParams
from sampling_ref import filter_probs
lib, ck = _lib.lib(), _lib.check
DEV = "cuda:0"
st = lambda: torch.cuda.current_stream().cuda_stream
i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
g = torch.Generator().manual_seed(77)
for vocab in (1, 7, 32769):
    for T, k, p in ((0.0, 0, 1.0), (1.0, 3, 0.8), (0.5, 0, 1.0)):
        lg = (torch.randn(vocab, generator=g) * 2).half().to(DEV)
        rec = i32(SamplingParams(T, k, p, seed=99).record())
        kept, _, _ = filter_probs(lg.cpu().double().numpy(), float(np.float32(T)), k, float(np.float32(p)))
        out, pos = torch.full((1,), -7, dtype=torch.long, device=DEV), i32([5])
        ck(lib.qeft_sample(lg.data_ptr(), vocab, 1, rec.data_ptr(), pos.data_ptr(), out.data_ptr(), st()))
        tok, p1 = torch.full((1,), -7, dtype=torch.long, device=DEV), i32([4])
        ck(lib.qeft_token_end_sample(lg.data_ptr(), tok.data_ptr(), p1.data_ptr(), vocab, rec.data_ptr(), st()))
        # batch entry, m = 1, one slot: token drawn at pos[0] + 1 = 5 as well
        slots, bpos, limit, eos, done = i32([0]), i32([4]), i32([100]), i32([-1]), i32([0])
        btok, bout, ctr = torch.full((1,), -7, dtype=torch.long, device=DEV), torch.full((1,), -9, dtype=torch.long, device=DEV), i32([0, 0])
        ck(lib.qeft_token_end_sample_batch(lg.data_ptr(), slots.data_ptr(), btok.data_ptr(), bpos.data_ptr(), limit.data_ptr(),
                                           eos.data_ptr(), done.data_ptr(), bout.data_ptr(), ctr.data_ptr(), rec.data_ptr(), vocab, 1,
                                           1, 1, st()))
        torch.cuda.synchronize()
        t = out.item()
        assert 0 <= t < vocab and kept[t], (vocab, T, k, p, t)
        assert tok.item() == t and p1.item() == 5, (vocab, T, tok.item(), p1.item())
        assert btok.item() == t and bout.item() == t and bpos.item() == 5 and ctr.tolist() == [1, 0] and done.item() == 0
print("SAMPLE-GUARD-OK")
'''


def test_smallest_shapes_in_own_allocations():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTORCH_NO_CUDA_MEMORY_CACHING="1")
    out = subprocess.run([sys.executable, "-c", ALLOC_CHILD % {"root": root}], cwd=root, env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SAMPLE-GUARD-OK" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])


def test_distribution_chi_square():
    from scipy.stats import chi2
    g = torch.Generator().manual_seed(11)
    row = (torch.randn(64, generator=g) * 1.5).half()
    n = 20000
    for (T, k, p) in [(1.0, 0, 1.0), (0.7, 20, 1.0), (1.3, 0, 0.9)]:
        toks = _run_sample(row.expand(n, 64).contiguous(), [_rec(T, k, p, 424242)] * n, list(range(n)))
        kept, pr, _ = filter_probs(row.double().numpy(), _f32(T), k, _f32(p))
        counts = np.bincount(toks, minlength=64)
        assert counts[~kept].sum() == 0
        e = pr[kept] * n
        stat = ((counts[kept] - e) ** 2 / e).sum()
        assert stat < chi2.ppf(1 - 1e-4, kept.sum() - 1), (T, k, p, stat)


def test_invariance_rows_m_and_replay():
    g = torch.Generator().manual_seed(12)
    vocab = 32000
    base = (torch.randn(8, vocab, generator=g) * 2).half()
    recs = [_rec(0.8 + 0.1 * r, [0, 40, 0, 5, 0, 1, 100, 0][r], [1, 1, 0.9, 0.95, 0.5, 1, 0.8, 1e-6][r], 1000 + r) for r in range(8)]
    pos = [100 + 3 * r for r in range(8)]
    ref = _run_sample(base, recs, pos)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    got = _run_sample(base[perm], [recs[i] for i in perm], [pos[i] for i in perm])
    assert [got[perm.index(r)] for r in range(8)] == ref
    for m in (1, 3):
        assert _run_sample(base[:m], recs[:m], pos[:m]) == ref[:m]
    assert _run_sample(base, recs, pos) == ref
    # a graph replay of the launch
    lib, ck = _lib()
    x, rec = base.to(DEV), torch.tensor(recs, dtype=torch.int32, device=DEV)
    pd, out = torch.tensor(pos, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.long, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ck(lib.qeft_sample(x.data_ptr(), vocab, 8, rec.data_ptr(), pd.data_ptr(), out.data_ptr(), _st()))
    for _ in range(2):
        out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().tolist() == ref


@pytest.mark.parametrize("vocab", [1000, 32000, 1003])
def test_zero_temperature_token_ends_equal_argmax_ends(vocab):
    """T = 0: qeft_token_end_sample == qeft_token_end and qeft_token_end_sample_batch == qeft_token_end_batch, bit for bit,
    over 8 launches captured in one graph with an EOS and a length stop inside it."""
    lib, ck = _lib()
    g = torch.Generator().manual_seed(vocab)
    lg = (torch.randn(8, vocab, generator=g) * 2).half()
    lg[:3, 17] = 30.0
    lg[:3, 900 % vocab] = 30.0
    lg[4, 5] = float("nan")
    am = [int(a) for a in torch.argmax(torch.nan_to_num(lg.float(), nan=-1e9), -1)]
    lgd = lg.to(DEV)
    # one sequence (each row in an aligned buffer of its own)
    tok_a, pos_a = torch.zeros(1, dtype=torch.long, device=DEV), torch.tensor([3], dtype=torch.int32, device=DEV)
    tok_b, pos_b = tok_a.clone(), pos_a.clone()
    rec1 = torch.tensor(_rec(0, 40, 0.5, 77), dtype=torch.int32, device=DEV)
    for r in range(8):
        row = lgd[r].clone()
        ck(lib.qeft_token_end(row.data_ptr(), tok_a.data_ptr(), pos_a.data_ptr(), vocab, 1, _st()))
        ck(lib.qeft_token_end_sample(row.data_ptr(), tok_b.data_ptr(), pos_b.data_ptr(), vocab, rec1.data_ptr(), _st()))
        torch.cuda.synchronize()
        assert tok_a.item() == tok_b.item() == am[r] and pos_a.item() == pos_b.item() == 4 + r
    # batch: slot state of 10 slots, rows in SLOTS; two runs of 8 token ends, the sampled one captured in one graph
    n_slots, cap = 10, 16
    pos = torch.full((n_slots,), 5, dtype=torch.int32)
    limit = torch.full((n_slots,), 100, dtype=torch.int32)
    eos = torch.full((n_slots,), -1, dtype=torch.int32)
    done = torch.zeros(n_slots, dtype=torch.int32)
    eos[SLOTS[1]] = am[1]
    limit[SLOTS[2]] = 9                                 # stops after 4 tokens, inside the graph
    done[SLOTS[3]] = 2
    params = torch.tensor([_rec(0, 3, 0.7, s) for s in range(n_slots)], dtype=torch.int32, device=DEV)
    slots = torch.tensor(SLOTS, dtype=torch.int32, device=DEV)

    def fresh():
        return ([t.to(DEV) for t in (pos, limit, eos, done)], torch.full((8,), -5, dtype=torch.long, device=DEV),
                torch.full((8, cap), -9, dtype=torch.long, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    (sa, toka, outa, ctra), (sb, tokb, outb, ctrb) = fresh(), fresh()
    for _ in range(8):
        ck(lib.qeft_token_end_batch(lgd.data_ptr(), slots.data_ptr(), toka.data_ptr(), sa[0].data_ptr(), sa[1].data_ptr(),
                                    sa[2].data_ptr(), sa[3].data_ptr(), outa.data_ptr(), ctra.data_ptr(), vocab, cap, n_slots, 8, _st()))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(8):
            ck(lib.qeft_token_end_sample_batch(lgd.data_ptr(), slots.data_ptr(), tokb.data_ptr(), sb[0].data_ptr(), sb[1].data_ptr(),
                                               sb[2].data_ptr(), sb[3].data_ptr(), outb.data_ptr(), ctrb.data_ptr(), params.data_ptr(),
                                               vocab, cap, n_slots, 8, _st()))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(sa + [toka, outa, ctra], sb + [tokb, outb, ctrb]):
        assert torch.equal(a, b)
    assert ctra.tolist() == [8, 0] and sa[3][SLOTS[1]].item() == 1 and sa[3][SLOTS[2]].item() == 2


def test_sampled_batch_token_end_is_row_and_slot_invariant():
    lib, ck = _lib()
    g = torch.Generator().manual_seed(13)
    vocab, n_slots, cap = 32000, 10, 8
    lg = (torch.randn(8, vocab, generator=g) * 2).half()
    recs = [_rec(0.9, 50, 0.9, 5000 + r) for r in range(8)]

    def run(order, slot_of):
        params = torch.zeros(n_slots, 8, dtype=torch.int32)
        pos = torch.zeros(n_slots, dtype=torch.int32)
        for r in order:
            params[slot_of[r]] = torch.tensor(recs[r], dtype=torch.int32)
            pos[slot_of[r]] = 40 + r
        st = [pos.to(DEV), torch.full((n_slots,), 1000, dtype=torch.int32, device=DEV),
              torch.full((n_slots,), -1, dtype=torch.int32, device=DEV), torch.zeros(n_slots, dtype=torch.int32, device=DEV)]
        x = lg[order].to(DEV)
        sl = torch.tensor([slot_of[r] for r in order], dtype=torch.int32, device=DEV)
        tok = torch.zeros(len(order), dtype=torch.long, device=DEV)
        out = torch.zeros(len(order), cap, dtype=torch.long, device=DEV)
        ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
        pd = params.to(DEV)
        for _ in range(3):
            ck(lib.qeft_token_end_sample_batch(x.data_ptr(), sl.data_ptr(), tok.data_ptr(), st[0].data_ptr(), st[1].data_ptr(),
                                               st[2].data_ptr(), st[3].data_ptr(), out.data_ptr(), ctr.data_ptr(), pd.data_ptr(),
                                               vocab, cap, n_slots, len(order), _st()))
        torch.cuda.synchronize()
        o = out.cpu()
        return {r: o[i, :3].tolist() for i, r in enumerate(order)}
    a = run(list(range(8)), SLOTS)
    b = run([3, 1, 6, 0, 7, 2, 5, 4], [9, 8, 7, 6, 5, 4, 3, 2])
    c = run([6, 2], SLOTS)
    assert a == b and all(a[r] == c[r] for r in c)
    # each draw is the standalone kernel's at the same position
    for r in range(8):
        assert a[r] == _run_sample(lg[r:r + 1].expand(3, vocab).contiguous(), [recs[r]] * 3, [41 + r, 42 + r, 43 + r])


# ---- the engines -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["7b", "70b"])
def model2(request):
    from qeft_amd.llama import LLAMA2_7B, LLAMA2_70B, QuantLlama
    base = {"7b": LLAMA2_7B, "70b": LLAMA2_70B}[request.param]
    shape = dataclasses.replace(base, n_layers=2, max_seq=256, name=base.name + "-2layers")
    model = QuantLlama(shape, DEV, seed=3, fast_init=True)
    yield request.param, model
    del model
    torch.cuda.empty_cache()


def _greedy_run(eng, first, p0, n):
    eng.set_sampling(None)
    eng.greedy = True
    eng.set_position(p0)
    eng.tok.fill_(first)
    eng.run(n)
    torch.cuda.synchronize()
    return eng.logits.clone(), int(eng.tok.item())


def test_decode_engine_sampled_run(model2):
    from qeft_amd.llama import DecodeEngine, prefill
    from qeft_amd.sampling import SamplingParams
    name, model = model2
    prompt = torch.randint(0, model.shape.vocab, (9,), generator=torch.Generator().manual_seed(21))
    eng = DecodeEngine(model, use_graph=True)
    logits = prefill(model, prompt.to(DEV), engine=eng)
    T = 9
    first = int(torch.argmax(logits[-1]))
    snap_k = [k.clone() for k in eng.kc]
    snap_v = [v.clone() for v in eng.vc]
    g_before = _greedy_run(eng, first, T, 16)
    sp = SamplingParams(0.8, 40, 0.95, seed=123456789)

    def sampled(params, use_graph, multi, steps=16):
        for k, v, a, b in zip(eng.kc, eng.vc, snap_k, snap_v):
            k.copy_(a)
            v.copy_(b)
        eng.use_graph = use_graph
        eng.greedy = False
        eng.set_sampling(params)
        eng.set_position(T)
        eng.tok.fill_(first)
        toks, rows = [], []
        if multi:
            eng.run(steps)
            torch.cuda.synchronize()
            return None, None
        for _ in range(steps):
            eng.step()
            rows.append(eng.logits[0].clone())
            toks.append(int(eng.tok.item()))
        return toks, rows
    eager, rows = sampled(sp, False, False)
    graph, _ = sampled(sp, True, False)
    assert eager == graph
    sampled(sp, True, True)
    assert int(eng.tok.item()) == eager[-1] and eng.host_pos == T + 16 and int(eng.pos.item()) == T + 16
    assert (eng._split_for(T), "sample", eng.MULTI) in eng.graphs
    again, _ = sampled(sp, True, False)
    other, _ = sampled(SamplingParams(0.8, 40, 0.95, seed=987654321), True, False)
    assert again == eager and other != eager
    # every step's token is the kernel's draw on that step's logits at its position
    for i, (t, row) in enumerate(zip(eager, rows)):
        got = _run_sample(row.cpu().unsqueeze(0), [sp.record()], [T + i + 1])[0]
        assert got == t, i
        kept, pr, margin = filter_probs(row.cpu().double().numpy(), _f32(0.8), 40, _f32(0.95))
        u, _ = draw_u(sp.seed, [T + i + 1])
        lo, hi = cdf_interval(pr, t)
        assert kept[t] and lo - 1e-6 <= u[0] <= hi + 1e-6
    # greedy after a sampled run: bit-identical to before
    eng.use_graph = True
    for k, v, a, b in zip(eng.kc, eng.vc, snap_k, snap_v):
        k.copy_(a)
        v.copy_(b)
    g_after = _greedy_run(eng, first, T, 16)
    assert torch.equal(g_before[0], g_after[0]) and g_before[1] == g_after[1]
    # assisted decoding stays greedy: it refuses an engine with sampling set
    from qeft_amd.assisted import PromptLookupDraft, assisted_generate
    eng.set_sampling(sp)
    with pytest.raises(ValueError):
        assisted_generate(eng, PromptLookupDraft(), first, 4, 3)
    eng.set_sampling(None)


def test_batch_engine_sampled_rows(model2):
    from qeft_amd.batch import BatchDecodeEngine, generate_batch
    from qeft_amd.llama import DecodeEngine
    from qeft_amd.sampling import SamplingParams
    name, model = model2
    vocab = model.shape.vocab
    gen = torch.Generator().manual_seed(31)
    prompts = [torch.randint(0, vocab, (n,), generator=gen) for n in (5, 12, 8, 20)]
    eng = DecodeEngine(model, use_graph=True)
    sp = [SamplingParams(1.0, 0, 1.0, seed=11), None, SamplingParams(0.7, 30, 0.9, seed=12), SamplingParams(0.0, seed=13)]
    N = 20

    def run(order, graph, others=None):
        be = BatchDecodeEngine(eng, max_batch=4, use_graph=graph)
        slots = {}
        for j in order:
            slots[j] = be.admit(prompts[j] if others is None or j == 0 else others[j], N, sampling=sp[j])
        be.run(N - 1)
        return {j: be.tokens(s) for j, s in slots.items()}, be
    a, be = run([0, 1, 2, 3], True)
    assert any(len(k) == 4 and k[3] == "sample" for k in be.graphs)
    assert all(len(a[j]) == N for j in a)
    b, _ = run([3, 2, 1, 0], True)              # other slots
    c, _ = run([0, 1, 2, 3], False)             # eager
    assert a == b == c
    # the sampled row 0 does not depend on the other rows (fixed m = 4)
    others = [None] + [torch.randint(0, vocab, (n,), generator=gen) for n in (7, 3, 15)]
    d, _ = run([0, 1, 2, 3], True, others)
    assert d[0] == a[0]
    # greedy rows (None and T = 0) of a mixed batch equal an all-greedy batch's
    g = generate_batch(eng, prompts, N, max_batch=4)
    assert a[1] == g[1] and a[3] == g[3]
    # generate_batch: all-T=0 sampling == greedy; equal seeds reproduce
    assert generate_batch(eng, prompts, N, max_batch=4, sampling=SamplingParams(0.0)) == g
    s1 = generate_batch(eng, prompts, N, max_batch=2, sampling=sp)
    s2 = generate_batch(eng, prompts, N, max_batch=2, sampling=sp)
    assert s1 == s2 and all(len(t) == N for t in s1)
    # a sampled EOS stops the row (same m = 4 as `a`): its own 5th token as EOS
    eos = a[0][4]
    k = a[0].index(eos)
    be = BatchDecodeEngine(eng, max_batch=4)
    s = [be.admit(prompts[j], N, eos_id=eos if j == 0 else None, sampling=sp[j]) for j in range(4)]
    be.run(N - 1)
    assert be.tokens(s[0]) == a[0][:k + 1] and be.finished()[s[0]] == "eos"
    assert [be.tokens(s[j]) for j in (1, 2, 3)] == [a[j] for j in (1, 2, 3)]
