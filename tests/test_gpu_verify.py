"""GPU parity of the verify pass: the m-row launches against m one-row launches and fp32 torch references, the engine's
verify() against teacher-forced step() rows, and greedy assisted generation against plain greedy decoding."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import qeft_oracle as O
from util import REL_TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from qeft_amd import _lib
    return _lib.lib(), _lib.check


def _packed_layer(n, k, seed):
    from qeft_amd import qeft_cuda
    bufs = O.make_layer(n, k, 128, 128, seed=seed)
    t = {kk: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for kk, v in bufs.items() if kk != "fake_weight"}
    return bufs, t["qweight"], qeft_cuda.pack_scales(t["scales"], t["scaled_zeros"], n, k, 128), t["oweight"]


def _linear(lib, ck, qw, sz, ow, n, k, m, x, y, mode=0, residual=None, ssq_in=None, n_ssq=0, gamma=None, ynorm=None, ssq_out=None):
    p = lambda t: t.data_ptr() if t is not None else None       # noqa: E731
    if m == 0:      # the one-row entry
        return ck(lib.qeft_decode_linear(p(x), p(qw), p(sz), p(ow), None, p(y), n, k, 128, 128, mode, p(residual), p(ssq_in), n_ssq,
                                         1e-5, p(gamma), p(ynorm), p(ssq_out), _st()))
    return ck(lib.qeft_decode_linear_m(p(x), p(qw), p(sz), p(ow), None, p(y), n, k, 128, 128, mode, p(residual), p(ssq_in), n_ssq,
                                       1e-5, p(gamma), p(ynorm), p(ssq_out), m, _st()))


# (n, k): the one-row launch uses 8 waves here (bit-equality expected), and K = 11008 (the x-from-global form at m >= 5; the
# one-row launch takes 12 waves there, so the sums are ordered differently: within REL_TOL)
@pytest.mark.parametrize("n,k", [(256, 512), (1024, 256), (256, 11008), (12288, 4096), (22016, 4096)])
@pytest.mark.parametrize("mode", ["ssq_in", "residual", "pair"])
def test_decode_linear_m_equals_separate_launches(n, k, mode):
    lib, ck = _lib()
    bufs, qw, sz, ow = _packed_layer(n, k, seed=n + k)
    # bit-equality where the one-row launch also runs 8-wave blocks (gemv_v3_plan: 12 waves for one-set launches of >= 64 steps,
    # 4 waves for launches of > 256 blocks)
    exact = k != 11008 and n <= 16 * 256
    g = torch.Generator().manual_seed(7)
    nb = lib.qeft_decode_linear_blocks(n)
    for m in range(2, 9):
        x = (torch.randn(m, k, generator=g) * 0.5).half().to(DEV)
        if mode == "pair":
            n_ssq = 37
            ssq = (torch.rand(m, n_ssq, generator=g) * 10 + 1).to(DEV)
            y = torch.zeros(m, n // 2, dtype=torch.float16, device=DEV)
            _linear(lib, ck, qw, sz, ow, n, k, m, x, y, mode=1, ssq_in=ssq, n_ssq=n_ssq)
            ref = torch.zeros_like(y)
            for i in range(m):
                _linear(lib, ck, qw, sz, ow, n, k, 0, x[i].clone(), ref[i], mode=1, ssq_in=ssq[i].clone(), n_ssq=n_ssq)
            outs = [(y, ref)]
        elif mode == "ssq_in":
            n_ssq = 300
            ssq = (torch.rand(m, n_ssq, generator=g) * 10 + 1).to(DEV)
            y = torch.zeros(m, n, dtype=torch.float16, device=DEV)
            _linear(lib, ck, qw, sz, ow, n, k, m, x, y, ssq_in=ssq, n_ssq=n_ssq)
            ref = torch.zeros_like(y)
            for i in range(m):
                _linear(lib, ck, qw, sz, ow, n, k, 0, x[i].clone(), ref[i], ssq_in=ssq[i].clone(), n_ssq=n_ssq)
            outs = [(y, ref)]
            # the oracle on the raw product (rows scaled by rsqrt(sum / K + eps))
            yo = O.quant_linear(x.cpu().numpy(), bufs["qweight"], bufs["scales"], bufs["scaled_zeros"], bufs["oweight"], None, 128)
            rs = 1.0 / np.sqrt(ssq.double().sum(1).cpu().numpy() / k + 1e-5)
            assert rel_err(y.float().cpu().numpy(), yo * rs[:, None]) < REL_TOL
        else:
            h0 = torch.randn(m, n, generator=g).to(DEV)
            gamma = (torch.rand(n, generator=g) + 0.5).half().to(DEV)
            h = h0.clone()
            yn = torch.zeros(m, n, dtype=torch.float16, device=DEV)
            so = torch.zeros(m, nb, device=DEV)
            _linear(lib, ck, qw, sz, ow, n, k, m, x, h, residual=h, gamma=gamma, ynorm=yn, ssq_out=so)
            hr, ynr, sor = h0.clone(), torch.zeros_like(yn), torch.zeros_like(so)
            for i in range(m):
                _linear(lib, ck, qw, sz, ow, n, k, 0, x[i].clone(), hr[i], residual=hr[i], gamma=gamma, ynorm=ynr[i], ssq_out=sor[i])
            outs = [(h, hr), (yn, ynr), (so, sor)]
            yo = O.quant_linear(x.cpu().numpy(), bufs["qweight"], bufs["scales"], bufs["scaled_zeros"], bufs["oweight"], None, 128)
            assert rel_err((h - h0).cpu().numpy(), yo) < REL_TOL
        torch.cuda.synchronize()
        for got, ref in outs:
            assert torch.isfinite(got.float()).all()
            if exact:
                assert torch.equal(got, ref), (m, mode, (got.float() - ref.float()).abs().max().item())
            else:
                assert rel_err(got.float().cpu().numpy(), ref.float().cpu().numpy()) < REL_TOL, (m, mode)


def _rot(x, c, s):          # x [..., 128] fp32, c / s [..., 64]: neox-style rotary, as the kernels
    a, b = x[..., :64], x[..., 64:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


@pytest.mark.parametrize("heads,kv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("split", [1, 2, 4, 8])
@pytest.mark.parametrize("where", ["start", "end"])
def test_multi_query_attention_vs_torch(heads, kv, split, where):
    lib, ck = _lib()
    max_seq, HD = 320, 128
    g = torch.Generator().manual_seed(heads * 100 + split)
    ang = torch.randn(max_seq, 64, generator=g)
    cos, sin = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()
    ws = torch.zeros(max(lib.qeft_attn_m_workspace_bytes(heads, 8, 8), 16) // 4, device=DEV)
    ws1 = torch.zeros(max(lib.qeft_attn_workspace_bytes(heads, 8), 16) // 4, device=DEV)
    nq = (heads + 2 * kv) * HD
    for m in range(1, 9):
        pos = 3 if where == "start" else max_seq - m
        kc = (torch.randn(kv, max_seq, HD, generator=g) * 0.5).half().to(DEV)
        vc = (torch.randn(kv, max_seq, HD, generator=g) * 0.5).half().to(DEV)
        kc1, vc1 = kc.clone(), vc.clone()
        qkv = (torch.randn(m, nq, generator=g)).half().to(DEV)
        out = torch.zeros(m, heads * HD, dtype=torch.float16, device=DEV)
        pos_t = torch.tensor([pos], dtype=torch.int32, device=DEV)
        qp = qkv.data_ptr()
        ck(lib.qeft_rope_attn_decode_m(qp, qp + heads * HD * 2, qp + (heads + kv) * HD * 2, nq, cos.data_ptr(), sin.data_ptr(), 64,
                                       max_seq, kc.data_ptr(), vc.data_ptr(), pos_t.data_ptr(), None, out.data_ptr(), heads * HD,
                                       ws.data_ptr(), split, heads, kv, max_seq, m, _st()))
        # m single-query launches on copies of the caches: the same K/V rows
        out1 = torch.zeros_like(out)
        for i in range(m):
            p1 = torch.tensor([pos + i], dtype=torch.int32, device=DEV)
            q1 = qkv[i].contiguous()
            ck(lib.qeft_rope_attn_decode(q1.data_ptr(), q1.data_ptr() + heads * HD * 2, q1.data_ptr() + (heads + kv) * HD * 2,
                                         cos.data_ptr(), sin.data_ptr(), max_seq, kc1.data_ptr(), vc1.data_ptr(), p1.data_ptr(), None,
                                         out1[i].data_ptr(), ws1.data_ptr(), split, heads, kv, max_seq, _st()))
        torch.cuda.synchronize()
        # the appended rows: v verbatim; k rotated by the same fp32 formula (the two kernels' FMA contraction may differ: one
        # fp16 unit in the last place at most)
        assert torch.equal(vc[:, :pos + m], vc1[:, :pos + m]) and torch.equal(kc[:, :pos], kc1[:, :pos]), m
        dk = (kc[:, pos:pos + m].float() - kc1[:, pos:pos + m].float()).abs()
        assert (dk <= kc1[:, pos:pos + m].float().abs() * 2.0 ** -10 + 2.0 ** -24).all(), (m, dk.max().item())
        # fp32 reference, causal within the block (the kernels' roundings: q scaled and k rotated to fp16)
        qf = qkv.float().cpu()
        c, s = cos.cpu()[pos:pos + m], sin.cpu()[pos:pos + m]
        K, V = kc.float().cpu(), vc.float().cpu()
        grp = heads // kv
        for i in range(m):
            for h in range(heads):
                q = _rot(qf[i, h * HD:(h + 1) * HD], c[i], s[i])
                q = (q * HD ** -0.5).half().float()
                L = pos + i + 1
                sc = K[h // grp, :L] @ q
                pr = torch.softmax(sc, 0)
                ref = pr @ V[h // grp, :L]
                got = out[i, h * HD:(h + 1) * HD].float().cpu()
                assert (got - ref).abs().max().item() < 2e-3 + 2e-3 * ref.abs().max().item(), (m, i, h)
        assert (out.float() - out1.float()).abs().max().item() < 4e-3


def test_lm_head_m_equals_one_row_head():
    lib, ck = _lib()
    g = torch.Generator().manual_seed(3)
    for H, vocab in ((512, 1000), (4096, 4100)):
        W = (torch.randn(vocab, H, generator=g) * 0.02).half().to(DEV)
        gamma = (torch.rand(H, generator=g) + 0.5).half().to(DEV)
        for m in (1, 3, 8):
            h = torch.randn(m, H, generator=g).to(DEV)
            lg = torch.zeros(m, vocab, dtype=torch.float16, device=DEV)
            ck(lib.qeft_lm_head_f16_m(h.data_ptr(), gamma.data_ptr(), W.data_ptr(), lg.data_ptr(), H, vocab, 1e-5, m, _st()))
            ref = torch.zeros(1, vocab, dtype=torch.float16, device=DEV)
            for i in range(m):
                hi = h[i].contiguous()
                ck(lib.qeft_lm_head_f16(hi.data_ptr(), gamma.data_ptr(), W.data_ptr(), ref.data_ptr(), H, vocab, 1e-5, _st()))
                torch.cuda.synchronize()
                assert torch.equal(lg[i], ref[0]), (H, m, i)
            xn = (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + 1e-5) * gamma.float()).half().float()
            assert rel_err(lg.float().cpu().numpy(), (xn @ W.float().t()).cpu().numpy()) < 2e-3


def _verify(lib, ck, logits, tokens, greedy=1):
    m, vocab = logits.shape
    toks = torch.tensor(tokens, dtype=torch.long, device=DEV)
    out = torch.full((8,), -1, dtype=torch.long, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    tok = torch.zeros(1, dtype=torch.long, device=DEV)
    pos = torch.tensor([10], dtype=torch.int32, device=DEV)
    ck(lib.qeft_verify_greedy(logits.data_ptr(), toks.data_ptr(), m, vocab, greedy, out.data_ptr(), n.data_ptr(), tok.data_ptr(),
                              pos.data_ptr(), _st()))
    torch.cuda.synchronize()
    return int(n.item()), out.tolist(), int(tok.item()), int(pos.item())


def test_verify_greedy_cases():
    from qeft_amd.assisted import accepted_prefix
    lib, ck = _lib()
    g = torch.Generator().manual_seed(5)
    for vocab in (1000, 32000, 1003):
        for m in range(1, 9):
            lg = torch.randn(m, vocab, generator=g).half()
            lg[:, 17] = 30.0                          # a tie between 17 and 900 in every row: the lower index wins
            lg[:, 900] = 30.0
            am = torch.argmax(lg.float(), -1).tolist()
            assert am == [17] * m
            for case in ("all", "none", "partial"):
                if case == "all":
                    toks = [3] + am[:m - 1]
                elif case == "none":
                    toks = [3] + [am[0] + 1] * (m - 1)
                else:
                    toks = [3] + am[:m - 1]
                    if m > 2:
                        toks[m // 2 + 1] = 5
                n, out, tok, pos = _verify(lib, ck, lg.to(DEV), toks)
                rn, racc = accepted_prefix(am, toks)
                assert (n, out[:n + 1], tok, pos) == (rn, racc, racc[-1], 10 + rn + 1), (vocab, m, case)
                if case == "all":
                    assert n == m - 1
    n, out, tok, pos = _verify(lib, ck, torch.zeros(4, 100, dtype=torch.float16, device=DEV), [1, 2, 3, 4], greedy=0)
    assert pos == 14 and tok == 0


def _tiny(seed, n_layers=2, max_seq=64, **kw):
    from qeft_amd.llama import QuantLlama, tiny_shape
    shape = tiny_shape(n_layers=n_layers, hidden=256, inter=512, n_heads=2, vocab=384, max_seq=max_seq, **kw)
    return QuantLlama(shape, DEV, seed=seed)


def _verify_rows(eng, tokens, chunks):
    """Teacher-forced verify passes over `tokens` in chunks of the given sizes: fp32 logits rows."""
    eng.reset()
    eng.greedy = False
    rows, i = [], 0
    for c in chunks:
        assert eng.verify(tokens[i:i + c]) is None
        rows.append(eng.logits_m[:c].float().clone())
        i += c
    assert eng.host_pos == i
    return torch.cat(rows)


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_verify_rows_equal_teacher_forced(use_graph):
    from qeft_amd.llama import DecodeEngine
    model = _tiny(seed=11, n_layers=3)
    tokens = torch.randint(0, model.shape.vocab, (40,), generator=torch.Generator().manual_seed(0))
    ref = DecodeEngine(model, use_graph=use_graph).teacher_forced_logits(tokens.to(DEV))
    eng = DecodeEngine(model, use_graph=use_graph)
    chunks = [1, 3, 8, 8, 5, 2, 7, 6]
    got = _verify_rows(eng, tokens, chunks)
    torch.cuda.synchronize()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item() / scale
    print(f"[verify tiny] max|d|/max|ref| = {err:.3e}")
    assert err < 1e-2, err
    if use_graph:
        assert any(kk[0] == "verify" for kk in eng.graphs)
        eager = _verify_rows(DecodeEngine(model, use_graph=False), tokens, chunks)
        assert torch.equal(eager, got)


@pytest.fixture(scope="module")
def model7b():
    from qeft_amd.llama import LLAMA2_7B, QuantLlama
    model = QuantLlama(dataclasses.replace(LLAMA2_7B, max_seq=512), DEV, seed=0, fast_init=True)
    yield model
    del model
    torch.cuda.empty_cache()


def test_engine_verify_7b_across_position_256(model7b):
    """m = 8 and m = 4 verify passes around position 256 (where the attention split changes from 1 to 4) against the
    teacher-forced one-token rows of the same positions."""
    from qeft_amd.llama import DecodeEngine
    model = model7b
    tokens = torch.randint(0, model.shape.vocab, (272,), generator=torch.Generator().manual_seed(4))
    ref = DecodeEngine(model, use_graph=True).teacher_forced_logits(tokens.to(DEV))
    eng = DecodeEngine(model, use_graph=True)
    eng.greedy = False
    for t in tokens[:240].tolist():                   # fill the cache up to 240 with one-token passes
        eng.tok.fill_(t)
        eng.step()
    got = []
    for c in (8, 4, 8, 8, 4):                         # 240..247 | 248..251 | 252..259 (across 256: split 4) | 260..267 | 268..271
        i = eng.host_pos
        eng.verify(tokens[i:i + c])
        got.append(eng.logits_m[:c].float().clone())
    got = torch.cat(got)
    torch.cuda.synchronize()
    assert {kk[2] for kk in eng.graphs if kk[0] == "verify"} == {1, 4}
    r = ref[240:272]
    err = (got - r).abs().max().item() / r.abs().max().item()
    print(f"[verify 7b] max|d|/max|ref| = {err:.3e}; per row", [round(v, 4) for v in ((got - r).abs().amax(-1) / r.abs().max()).tolist()])
    assert err < 1e-2, err


def _greedy_reference(model, first, n):
    from qeft_amd.llama import DecodeEngine
    eng = DecodeEngine(model, use_graph=True)
    eng.reset()
    eng.greedy = True
    eng.tok.fill_(first)
    toks, logits = [], []
    for _ in range(n):
        eng.step()
        toks.append(int(eng.tok.item()))
        logits.append(eng.logits[0].float().clone())
    return toks, logits


def _check_same_or_near_tie(model, first, got, ref, ref_logits):
    """Assisted tokens must equal plain greedy run; where they do not, the one-token logits at the first divergence must be a
    near-tie: a top-2 gap below the measured m-row vs one-row logit difference at that position."""
    if got == ref:
        return
    j = next(i for i in range(len(ref)) if got[i] != ref[i])
    from qeft_amd.llama import DecodeEngine
    ctx = [first] + ref[:j]
    eng = DecodeEngine(model, use_graph=False)
    eng.greedy = False
    rows = _verify_rows(eng, ctx, [min(8, len(ctx) - i) for i in range(0, len(ctx), 8)])
    diff = (rows[j] - ref_logits[j]).abs().max().item()
    top2 = ref_logits[j].topk(2).values
    gap = (top2[0] - top2[1]).item()
    assert gap <= diff, f"divergence at {j}: top-2 gap {gap:.4g} > m-row vs one-row difference {diff:.4g}"


def test_assisted_generate_with_engine_drafts():
    from qeft_amd.assisted import EngineDraft, assisted_generate
    from qeft_amd.llama import DecodeEngine
    model = _tiny(seed=21, n_layers=2, max_seq=128)
    first, N = 7, 60
    ref, ref_logits = _greedy_reference(model, first, N)

    # the same model as draft: every draft is the target's own choice
    eng = DecodeEngine(model, use_graph=True)
    eng.reset()
    out, acc = assisted_generate(eng, EngineDraft(DecodeEngine(model, use_graph=True)), first, N, k=7)
    _check_same_or_near_tie(model, first, out, ref, ref_logits)
    if out == ref:
        assert all(a == min(7, N - sum(acc[:i]) - i - 1) for i, a in enumerate(acc)), acc

    # always wrong: each pass accepts nothing and yields the target's own token
    class Wrong:
        def propose(self, ctx, k):
            j = len(ctx) - 1                  # index into ref of the token after ctx[-1]
            return [(ref[j] + 1) % model.shape.vocab] * k if j < len(ref) else []
    eng.reset()
    out, acc = assisted_generate(eng, Wrong(), first, N, k=4)
    assert acc == [0] * N
    _check_same_or_near_tie(model, first, out, ref, ref_logits)

    # a 1-layer model as draft: whatever it accepts, the tokens are the target's
    draft = DecodeEngine(_tiny(seed=21, n_layers=1, max_seq=128), use_graph=True)
    eng.reset()
    out, acc = assisted_generate(eng, EngineDraft(draft), first, N, k=4)
    assert sum(acc) + len(acc) >= N
    _check_same_or_near_tie(model, first, out, ref, ref_logits)
    print(f"[assisted] 1-layer draft: {len(acc)} passes for {N} tokens, accepted {acc}")


def test_assisted_generate_prompt_lookup():
    from qeft_amd.assisted import PromptLookupDraft, assisted_generate
    from qeft_amd.llama import DecodeEngine
    model = _tiny(seed=22, n_layers=2, max_seq=128)
    first, N = 3, 40
    ref, ref_logits = _greedy_reference(model, first, N)
    eng = DecodeEngine(model, use_graph=True)
    eng.reset()
    out, acc = assisted_generate(eng, PromptLookupDraft(), first, N, k=4)
    _check_same_or_near_tie(model, first, out, ref, ref_logits)


def test_verify_refuses():
    from qeft_amd.llama import DecodeEngine, QuantLlama
    model = _tiny(seed=3, n_layers=1, max_seq=32)
    eng = DecodeEngine(model, use_graph=False)
    eng.set_position(28)
    with pytest.raises(RuntimeError, match="max_seq"):
        eng.verify([1, 2, 3, 4, 5])
    eng.verify([1, 2, 3, 4])                          # 28 .. 31: the last rows of the cache
    assert eng.host_pos == 32

    class One:                                        # a one-rank tensor-parallel group (the engine's simulated-group form)
        world, rank = 1, 0

        def all_gather(self, out, inp):
            out.copy_(inp)

        def all_reduce(self, t):
            pass
    tp = DecodeEngine(model, use_graph=False, tp_group=One())
    with pytest.raises(RuntimeError, match="tensor-parallel"):
        tp.verify([1, 2])
    w3 = DecodeEngine(QuantLlama(dataclasses.replace(model.shape, bits=3), DEV, seed=4), use_graph=False)
    with pytest.raises(RuntimeError, match="4-bit"):
        w3.verify([1, 2])
