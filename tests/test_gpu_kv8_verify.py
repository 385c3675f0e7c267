"""The verify pass over the e4m3 KV cache on the GPU (csrc/decode_verify_kv8.hip; DecodeEngine(kv_dtype="fp8", kv8_verify=True);
DESIGN.md §4.11), through the C ABI and through the engine.

Kernel tests: the cache of ONE sequence sits inside guarded allocations with canary bands, and every row >= pos holds code 0x7F (e4m3
NaN) and scale NaN before the launch, the m rows the launch is about to write included: a row read from the cache where the launch's
own must stand in, or read past the causal bound, makes the output NaN.  The reference is tests/kv8_ref.py: row i against
attention_fp64 over the dequantised cache as the launch left it, keys [0, pos + i]; acceptance per head
|got - ref| <= 2e-3 + 2e-3 max|ref| (tests/test_gpu_attn_long.py, _attn_close).  Each test prints the worst |got - ref| / bound."""
import os

import pytest
import torch

import kv8_ref
from kv8_ref import HD, NAN8
from util import REL_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPLITS = (1, 2, 4, 8)
BAND = 4096                 # canary bytes / floats in front of and behind every cache array
CANARY8, CANARYF = 0xA5, 12345.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ckpt_llama2l.pth")
# tests/test_gpu_kv8.py, MEASURED_DLOGIT: the fp8 engine against the fp16 engine, teacher-forced over 48 tokens of the golden
# checkpoint, max|dlogit| as measured on an MI355X.  The m-row against one-row difference on an fp8 engine (rounding, amplified by
# code flips in the new rows) is a subset of that difference; the assertion is 4x it, as there.
MEASURED_DLOGIT = 6.365967e-02


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from qeft_amd import _lib
    return _lib.lib(), _lib.check


def _attn_close(got, ref, what):
    """tests/test_gpu_attn_long.py::_attn_close: the bound, and the worst error in units of it."""
    got = got.double().view(-1, HD)
    ref = ref.view(got.shape)
    assert torch.isfinite(got).all(), what
    tol = 2e-3 + 2e-3 * ref.abs().amax(-1, keepdim=True)
    bad = (got - ref).abs() > tol
    assert not bad.any(), (what, (got - ref).abs().max().item(), bad.nonzero()[:4].tolist())
    return ((got - ref).abs() / tol).max().item()


class _Guarded:
    """A tensor of `shape` inside a larger allocation, canary bands on both sides."""

    def __init__(self, shape, dtype):
        n = 1
        for d in shape:
            n *= d
        self.fill = CANARY8 if dtype == torch.uint8 else CANARYF
        self.raw = torch.full((n + 2 * BAND,), self.fill, dtype=dtype, device=DEV)
        self.t = self.raw[BAND:BAND + n].view(*shape)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.raw[:BAND] == self.fill).all() and (self.raw[-BAND:] == self.fill).all())


class _Cache:
    """The e4m3 cache of one sequence and one head layout inside guarded allocations, rotary tables by position and ONE workspace
    sized for (m 8, split 8).  k0 / v0 are the fp16 content; poison(pos) restores quant(k0 / v0) and poisons every row >= pos."""

    def __init__(self, heads, kv, max_seq, seed):
        self.lib, self.ck = _lib()
        self.heads, self.kv, self.max_seq = heads, kv, max_seq
        self.g = torch.Generator(device=DEV).manual_seed(seed)
        self.nq = (heads + 2 * kv) * HD
        self.k0 = (torch.randn(kv, max_seq, HD, generator=self.g, device=DEV) * 0.5).half()
        self.v0 = (torch.randn(kv, max_seq, HD, generator=self.g, device=DEV) * 0.5).half()
        self.G = [_Guarded((kv, max_seq, HD), torch.uint8), _Guarded((kv, max_seq, HD), torch.uint8),
                  _Guarded((kv, max_seq), torch.float32), _Guarded((kv, max_seq), torch.float32)]
        self.kc, self.vc, self.ks, self.vs = (g.t for g in self.G)
        self.ws = torch.zeros(max(self.lib.qeft_attn_m_kv8_workspace_bytes(heads, 8, 8), 16) // 4, device=DEV)
        self.tables(torch.randn(max_seq, 64, generator=self.g, device=DEV))
        self.requant()

    def tables(self, ang):
        self.cos, self.sin = ang.cos().contiguous(), ang.sin().contiguous()

    def requant(self):
        self.q0 = [kv8_ref.quant_rows(self.k0), kv8_ref.quant_rows(self.v0)]

    def qkv(self, m):
        return torch.randn(m, self.nq, generator=self.g, device=DEV).half()

    def poison(self, pos):
        for (codes, scales), c, s in zip(self.q0, (self.kc, self.vc), (self.ks, self.vs)):
            c.copy_(codes)
            s.copy_(scales)
            c[:, pos:] = NAN8
            s[:, pos:] = float("nan")

    def snapshot(self):
        return [t.clone() for t in (self.kc, self.vc, self.ks, self.vs)]

    def out(self, m):
        return torch.full((m, self.heads * HD), float("nan"), dtype=torch.float16, device=DEV)

    def launch(self, qkv, m, pos, split, out, out_pos=None, tab_rows_m=False, ws=None):
        """tab_rows_m: the rotary tables as the m rows of positions pos .. pos + m - 1 (the engine's form)."""
        qp = qkv.data_ptr()
        pos_d = torch.tensor([pos], dtype=torch.int32, device=DEV)
        cos, sin, tab_rows = self.cos, self.sin, self.max_seq
        if tab_rows_m:
            cos, sin, tab_rows = self.cos[pos:pos + m].clone(), self.sin[pos:pos + m].clone(), m
        ws = self.ws if ws is None else ws
        self.ck(self.lib.qeft_rope_attn_decode_m_kv8(qp, qp + self.heads * HD * 2, qp + (self.heads + self.kv) * HD * 2, self.nq,
                                                     cos.data_ptr(), sin.data_ptr(), 64, tab_rows, self.kc.data_ptr(),
                                                     self.vc.data_ptr(), self.ks.data_ptr(), self.vs.data_ptr(), pos_d.data_ptr(),
                                                     out_pos.data_ptr() if out_pos is not None else None, out.data_ptr(),
                                                     self.heads * HD, ws.data_ptr(), split, self.heads, self.kv, self.max_seq, m,
                                                     _st()))
        torch.cuda.synchronize()
        assert all(g.intact() for g in self.G), "a canary band changed"

    def reference(self, qkv, m, pos):
        """fp64, causal: row i over keys [0, pos + i] of the dequantised cache as it is now -> [m, heads * 128]."""
        rows = []
        for i in range(m):
            q = kv8_ref.rot(qkv[i, :self.heads * HD].float().view(self.heads, HD), self.cos[pos + i][None], self.sin[pos + i][None])
            q = (q * HD ** -0.5).half()
            rows.append(kv8_ref.attention_fp64(q, self.kc, self.vc, self.ks, self.vs, pos + i))
        return torch.stack(rows)

    def check_rest_untouched(self, before, pos, m):
        """Every row outside [pos, pos + m) of every cache array as in `before`, bit for bit (NaN codes and scales included)."""
        for a, b in zip(self.snapshot(), before):
            a, b = (a, b) if a.dtype == torch.uint8 else (a.view(torch.int32), b.view(torch.int32))
            same = (a == b) if a.dim() == 2 else (a == b).all(-1)
            same[:, pos:pos + m] = True
            assert same.all(), same.logical_not().nonzero()[:4].tolist()

    def run_and_check(self, m, pos, split, what, **kw):
        """poison, launch, nothing else written, finite out, fp64 parity of every row: the worst err / bound."""
        self.poison(pos)
        before = self.snapshot()
        qkv, out = self.qkv(m), self.out(m)
        self.launch(qkv, m, pos, split, out, **kw)
        self.check_rest_untouched(before, pos, m)
        got = out
        if kw.get("out_pos") is not None:
            got = out[:, kw["out_pos"].long()]                # element e was stored at out_pos[e]
        assert torch.isfinite(got.float()).all(), what
        return _attn_close(got, self.reference(qkv, m, pos), what), qkv, got


LAYOUTS = [(4, 4), (8, 2), (8, 1), (5, 1)]
_caches = {}


def _cache320(heads, kv):
    """One guarded cache of 320 rows per layout, shared by the kernel tests (every test poisons it afresh)."""
    if (heads, kv) not in _caches:
        _caches[heads, kv] = _Cache(heads, kv, 320, seed=heads * 31 + kv)
    return _caches[heads, kv]


def _positions(m, max_seq):
    return sorted({0, 3, 27, 16 - m, max_seq - m})


# ---------------------------------------------------------------------------------------------------------------------
# a. parity, nothing else written
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,kv", LAYOUTS)
@pytest.mark.parametrize("split", SPLITS)
def test_parity_sweep_fp64(split, heads, kv):
    A = _cache320(heads, kv)
    worst = 0.0
    for m in range(1, 9):
        for pos in _positions(m, A.max_seq):
            worst = max(worst, A.run_and_check(m, pos, split, (heads, kv, split, m, pos))[0])
    print(f"[kv8-verify parity] heads={heads} kv={kv} split={split} max_seq=320 m=1..8 worst err/bound={worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# b. the appended rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_appended_rows_bit_equal(heads, kv):
    """V codes and scales: kv8_ref of the v rows.  K codes and scales: kv8_ref of the rows qeft_rope_attn_decode_m appends to an
    fp16 cache from the same inputs (one rotary expression)."""
    A = _cache320(heads, kv)
    ws16 = torch.zeros(max(A.lib.qeft_attn_m_workspace_bytes(heads, 8, 8), 16) // 4, device=DEV)
    for m in range(1, 9):
        for pos, split in ((0, 1), (27, 4), (A.max_seq - m, 8)):
            A.poison(pos)
            qkv, out, out16 = A.qkv(m), A.out(m), A.out(m)
            kc16, vc16 = A.k0.clone(), A.v0.clone()
            qp = qkv.data_ptr()
            pos_d = torch.tensor([pos], dtype=torch.int32, device=DEV)
            A.ck(A.lib.qeft_rope_attn_decode_m(qp, qp + heads * HD * 2, qp + (heads + kv) * HD * 2, A.nq, A.cos.data_ptr(),
                                               A.sin.data_ptr(), 64, A.max_seq, kc16.data_ptr(), vc16.data_ptr(), pos_d.data_ptr(),
                                               None, out16.data_ptr(), heads * HD, ws16.data_ptr(), split, heads, kv, A.max_seq, m,
                                               _st()))
            A.launch(qkv, m, pos, split, out)
            v = qkv[:, (heads + kv) * HD:].view(m, kv, HD).transpose(0, 1)
            assert torch.equal(vc16[:, pos:pos + m], v)
            for src, c, s in ((kc16[:, pos:pos + m], A.kc, A.ks), (v, A.vc, A.vs)):
                codes, scales = kv8_ref.quant_rows(src)
                assert torch.equal(c[:, pos:pos + m], codes), (m, pos, split)
                assert torch.equal(s[:, pos:pos + m].contiguous().view(torch.int32), scales.contiguous().view(torch.int32)), (m, pos)


# ---------------------------------------------------------------------------------------------------------------------
# c. the same as m one-row launches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,kv", LAYOUTS)
@pytest.mark.parametrize("split", [1, 8])
def test_same_as_m_one_row_launches(split, heads, kv):
    """m calls of qeft_rope_attn_decode_kv8 (one row, slot 0) at pos + i on a copy of the cache agree with the m-row output within
    the 4e-3 of tests/test_gpu_verify.py::test_multi_query_attention_vs_torch."""
    A = _cache320(heads, kv)
    ws1 = torch.zeros(max(A.lib.qeft_attn_kv8_workspace_bytes(heads, 8, 1), 16) // 4, device=DEV)
    slot0 = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    for m in (1, 3, 8):
        for pos in (3, 27, A.max_seq - m):
            A.poison(pos)
            c1 = A.snapshot()
            qkv, out, out1 = A.qkv(m), A.out(m), A.out(m)
            A.launch(qkv, m, pos, split, out)
            for i in range(m):
                q1 = qkv[i].contiguous()
                p1 = torch.tensor([pos + i], dtype=torch.int32, device=DEV)
                A.ck(A.lib.qeft_rope_attn_decode_kv8(q1.data_ptr(), q1.data_ptr() + heads * HD * 2,
                                                     q1.data_ptr() + (heads + kv) * HD * 2, A.nq, A.cos.data_ptr(), A.sin.data_ptr(), 64,
                                                     A.max_seq, c1[0].data_ptr(), c1[1].data_ptr(), c1[2].data_ptr(), c1[3].data_ptr(),
                                                     slot0.data_ptr(), p1.data_ptr(), None, None, out1[i].data_ptr(), heads * HD,
                                                     ws1.data_ptr(), split, 1, heads, kv, A.max_seq, 1, _st()))
            torch.cuda.synchronize()
            d = (out.float() - out1.float()).abs().max().item()
            assert d < 4e-3, (m, pos, d)
            worst = max(worst, d)
    print(f"[kv8-verify one-row] heads={heads} kv={kv} split={split} max|m-row - one-row| = {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# d. workspace reuse, depth, out of range
# ---------------------------------------------------------------------------------------------------------------------
def test_workspace_reuse():
    """ONE workspace sized for (8, 8) through (m 8, split 8) -> (m 3, split 4) -> (m 1, split 1) -> (m 8, split 8): a smaller
    configuration after a larger one must find its counters armed and no counter on another configuration's records."""
    A = _cache320(8, 2)
    ws = torch.zeros(A.lib.qeft_attn_m_kv8_workspace_bytes(8, 8, 8) // 4, device=DEV)
    worst = 0.0
    for m, split in ((8, 8), (3, 4), (1, 1), (8, 8)):
        worst = max(worst, A.run_and_check(m, 200, split, ("reuse", m, split), ws=ws)[0])
    print(f"[kv8-verify reuse] heads=8 kv=2 (8,8)->(3,4)->(1,1)->(8,8) worst err/bound={worst:.3f}")


@pytest.mark.parametrize("split", [1, 8])
def test_depth_4096_out_pos_and_row_tables(split):
    """4096 rows: a wave's two-runs-in-flight loop runs many rounds; out_pos a random permutation; rotary tables as m rows."""
    A = _Cache(4, 4, 4096, seed=41 + split)
    out_pos = torch.randperm(4 * HD, generator=torch.Generator().manual_seed(split)).to(torch.int32).to(DEV)
    worst, _, _ = A.run_and_check(8, 4088 - 3, split, ("depth", split), out_pos=out_pos, tab_rows_m=True)
    print(f"[kv8-verify depth] heads=4 kv=4 split={split} max_seq=4096 pos=4085 m=8 worst err/bound={worst:.3f}")


@pytest.mark.parametrize("heads,kv", [(4, 4), (8, 1)])
def test_out_of_range_touches_nothing(heads, kv):
    A = _cache320(heads, kv)
    for m, split in ((1, 1), (5, 4), (8, 8)):
        for pos in (A.max_seq - m + 1, -1):
            A.poison(100)
            A.ws.fill_(7.0)
            before = A.snapshot()
            qkv, out = A.qkv(m), A.out(m)
            A.launch(qkv, m, pos, split, out)
            A.check_rest_untouched(before, 0, 0)
            assert torch.isnan(out).all() and (A.ws == 7.0).all(), (m, split, pos)
    A.ws.zero_()


# ---------------------------------------------------------------------------------------------------------------------
# e. causality under adversarial scores
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,kv", [(4, 4), (8, 1)])
@pytest.mark.parametrize("split", [1, 8])
@pytest.mark.parametrize("case", ["sink", "equal"])
def test_causality_under_adversarial_scores(case, split, heads, kv):
    """"sink": new K row i = 2 scores about 60 nats above everything else for every query: rows 0 and 1 must match the reference
    that cannot see it (a leak of 1e-26 of its weight is invisible, a missing mask is not), rows 2..7 the reference it dominates.
    "equal": K = 0 everywhere (scale 0, codes 0, the new rows too): every score equal, row i the plain mean of values [0, pos + i]."""
    m = 8
    A = _Cache(heads, kv, 320, seed=13 * heads + kv + split)
    ramp = (torch.arange(A.max_seq, device=DEV, dtype=torch.float32) / 64)[None, :, None]
    A.v0 = (A.v0.float() + ramp).half()                     # a ramp over the positions: a dropped or leaked row moves the result
    ang = torch.randn(A.max_seq, 64, generator=A.g, device=DEV)
    ang[:, 0] = 0.0                                          # pair (0, 64) unrotated: dimension 0 lines q and k up
    A.tables(ang)
    if case == "equal":
        A.k0.zero_()
    A.requant()
    worst = 0.0
    for pos in (27, 100):                                    # new rows across the run boundary at 32; inside one run
        qkv = A.qkv(m)
        kq = qkv[:, heads * HD:(heads + kv) * HD].view(m, kv, HD)
        if case == "equal":
            kq.zero_()
        else:
            qkv[:, :heads * HD].view(m, heads, HD)[:, :, 0] = 8.0
            kq[2, :, 0] = 85.0                               # 8 * 128^-0.5 * 85 = 60.1
        A.poison(pos)
        before = A.snapshot()
        out = A.out(m)
        A.launch(qkv, m, pos, split, out)
        A.check_rest_untouched(before, pos, m)
        ref = A.reference(qkv, m, pos)
        grp = heads // kv
        if case == "equal":
            assert A.ks[:, pos:pos + m].eq(0).all() and A.kc[:, pos:pos + m].eq(0).all()
            for i in range(m):                               # the reference itself against the closed form
                mean = kv8_ref.dequant_rows(A.vc[:, :pos + i + 1], A.vs[:, :pos + i + 1], torch.float64).mean(1)
                assert (ref[i].view(heads, HD) - mean.repeat_interleave(grp, 0)).abs().max().item() < 1e-9
        else:
            v2 = kv8_ref.dequant_rows(A.vc[:, pos + 2], A.vs[:, pos + 2], torch.float64).repeat_interleave(grp, 0)
            for i in range(m):                               # the reference: rows 2.. ARE row 2's value, rows 0, 1 are far from it
                d = (ref[i].view(heads, HD) - v2).abs().max().item()
                assert (d < 1e-6) if i >= 2 else (d > 0.1), (i, d)
        worst = max(worst, _attn_close(out, ref, (case, heads, kv, split, pos)))
    print(f"[kv8-verify adv] {case:<5} heads={heads} kv={kv} split={split} worst err/bound={worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# f. the engine
# ---------------------------------------------------------------------------------------------------------------------
def _tiny(seed, n_layers=2, max_seq=64, **kw):
    from qeft_amd.llama import QuantLlama, tiny_shape
    return QuantLlama(tiny_shape(n_layers=n_layers, hidden=256, inter=512, n_heads=2, vocab=384, max_seq=max_seq, **kw), DEV, seed=seed)


def _eng(model, use_graph=True, **kw):
    from qeft_amd.llama import DecodeEngine
    return DecodeEngine(model, use_graph=use_graph, kv_dtype="fp8", kv8_verify=True, **kw)


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


def _cache_state(eng):
    return [t.clone() for group in (eng.kc, eng.vc, eng.ks, eng.vs) for t in group]


def _same_state(a, b, upto):
    """Bit-equal cache arrays over positions [0, upto)."""
    return all(torch.equal(x[:, :upto].contiguous().view(torch.uint8), y[:, :upto].contiguous().view(torch.uint8)) for x, y in zip(a, b))


def test_refusal_stays_and_the_flag_lifts_it():
    from qeft_amd.llama import DecodeEngine
    model = _tiny(seed=4)
    eng = DecodeEngine(model, use_graph=False, kv_dtype="fp8")
    assert eng.kv8_verify is False
    with pytest.raises(RuntimeError, match="fp8"):
        eng.verify([1, 2, 3])
    on = _eng(model, use_graph=False)
    assert on.verify([1, 2, 3]) is None and on.host_pos == 3
    assert torch.isfinite(on.logits_m[:3].float()).all()
    assert DecodeEngine(model, use_graph=False, kv8_verify=True).verify([1, 2, 3]) is None      # fp16: the flag has no effect


CHUNKS = [1, 3, 8, 8, 5, 2, 7, 6]


@pytest.mark.parametrize("which", ["tiny", "golden"])
def test_engine_rows_equal_teacher_forced(which):
    """Verify rows in chunks against teacher_forced_logits of an fp8 engine (the one-row path).  golden: max|dlogit| <=
    4 x MEASURED_DLOGIT; tiny: the relative 1e-2 of tests/test_gpu_verify.py::test_engine_verify_rows_equal_teacher_forced.
    Graph and eager give bit-equal logits and bit-equal cache arrays."""
    from qeft_amd.llama import DecodeEngine, QuantLlama
    model = _tiny(seed=11, n_layers=3) if which == "tiny" else QuantLlama.from_packed(GOLDEN, device=DEV, max_seq=64)
    tokens = torch.randint(0, model.shape.vocab, (40,), generator=torch.Generator().manual_seed(0))
    ref = DecodeEngine(model, use_graph=True, kv_dtype="fp8").teacher_forced_logits(tokens.to(DEV))
    eng = _eng(model, use_graph=True)
    got = _verify_rows(eng, tokens, CHUNKS)
    torch.cuda.synchronize()
    dl = (got - ref).abs().max().item()
    rel = dl / ref.abs().max().item()
    print(f"[kv8-verify rows {which}] max|dlogit| = {dl:.6e} (max|logit| {ref.abs().max().item():.3f}), relative {rel:.3e}")
    if which == "golden":
        assert dl <= 4 * MEASURED_DLOGIT, dl
    else:
        assert rel < 1e-2, rel
    assert any(kk[0] == "verify" for kk in eng.graphs)
    eager = _eng(model, use_graph=False)
    rows_e = _verify_rows(eager, tokens, CHUNKS)
    assert torch.equal(rows_e, got)
    assert _same_state(_cache_state(eager), _cache_state(eng), 40)


def test_engine_across_a_split_change():
    """max_seq 320, filled to 240 by steps; chunks 8, 4, 8, 8, 4 cross position 256, where the split goes from 1 to 4."""
    from qeft_amd.llama import DecodeEngine
    model = _tiny(seed=12, n_layers=2, max_seq=320)
    tokens = torch.randint(0, model.shape.vocab, (272,), generator=torch.Generator().manual_seed(4))
    ref = DecodeEngine(model, use_graph=True, kv_dtype="fp8").teacher_forced_logits(tokens.to(DEV))
    eng = _eng(model)
    eng.greedy = False
    for t in tokens[:240].tolist():
        eng.tok.fill_(t)
        eng.step()
    got = []
    for c in (8, 4, 8, 8, 4):
        i = eng.host_pos
        eng.verify(tokens[i:i + c])
        got.append(eng.logits_m[:c].float().clone())
    got = torch.cat(got)
    torch.cuda.synchronize()
    assert {kk[2] for kk in eng.graphs if kk[0] == "verify"} == {1, 4}
    r = ref[240:272]
    rel = (got - r).abs().max().item() / r.abs().max().item()
    print(f"[kv8-verify split change] max|d|/max|ref| = {rel:.3e}")
    assert rel < 1e-2, rel


def _greedy_steps(model, first, n):
    """The one-row fp8 engine's own greedy step loop: (tokens, fp32 logits per step)."""
    from qeft_amd.llama import DecodeEngine
    eng = DecodeEngine(model, use_graph=True, kv_dtype="fp8")
    eng.greedy = True
    eng.tok.fill_(first)
    toks, rows = [], []
    for _ in range(n):
        eng.step()
        toks.append(int(eng.tok.item()))
        rows.append(eng.logits[0].float().clone())
    return toks, rows


def _first_mismatch_is_near_tie(got, ref, ref_rows):
    """tests/test_gpu_kv8.py::_same_or_near_tie on streams that start after the first token: equal, or at the first mismatch the
    reference's top-2 margin is a near-tie (the comparison stops there).  Returns the mismatch index or None."""
    for j in range(min(len(got), len(ref))):
        if got[j] != ref[j]:
            top2 = ref_rows[j].topk(2).values
            assert (top2[0] - top2[1]).item() <= REL_TOL * ref_rows[j].abs().max().item() + 2.0 ** -10 * top2[0].abs().item(), \
                f"token {j}: {got[j]} vs {ref[j]}, not a near-tie"
            return j
    assert len(got) == len(ref), (len(got), len(ref))
    return None


def test_greedy_assisted_generate():
    from qeft_amd.assisted import EngineDraft, PromptLookupDraft, assisted_generate
    from qeft_amd.llama import DecodeEngine
    model = _tiny(seed=21, n_layers=2, max_seq=128)
    first, N = 7, 24
    ref, ref_rows = _greedy_steps(model, first, N)
    assert _greedy_steps(model, first, N)[0] == ref         # the one-row fp8 engine agrees with itself throughout
    eng = _eng(model)
    # the same model on an fp8 cache as the draft: every draft is the target's own one-row choice
    out, acc = assisted_generate(eng, EngineDraft(DecodeEngine(model, use_graph=True, kv_dtype="fp8")), first, N, k=7)
    j = _first_mismatch_is_near_tie(out, ref, ref_rows)
    assert j is None or j > 8, j
    if j is None:
        assert all(a == min(7, N - sum(acc[:i]) - i - 1) for i, a in enumerate(acc)), acc      # m - 1 on every full pass
    print(f"[kv8-verify assisted] engine draft: first mismatch {j}, accepted {acc}")
    eng.reset()
    out, acc = assisted_generate(eng, PromptLookupDraft(), first, N, k=4)
    j = _first_mismatch_is_near_tie(out, ref, ref_rows)
    assert j is None or j > 8, j
    print(f"[kv8-verify assisted] prompt lookup: first mismatch {j}, accepted {acc}")


def test_sampled_verify_stream():
    """verify_sample passes emit the token stream of the sampled one-row fp8 engine with the same SamplingParams, by the rule of
    tests/test_gpu_verify_sample.py: the one-row engine is teacher-forced along the emitted stream with the record set; where its
    draw differs from the emitted token, u must lie within TV(P1, Pm) + 1e-6 of an edge of that draw's CDF interval (P1, Pm: the
    fp64 reference distributions of the one-row and the m-row logits of the position).  Two runs with one seed are identical."""
    import numpy as np
    from qeft_amd.assisted import PromptLookupDraft, assisted_generate
    from qeft_amd.llama import DecodeEngine
    from qeft_amd.sampling import SamplingParams
    from sampling_ref import cdf_interval, draw_u, filter_probs
    model = _tiny(seed=23, n_layers=2, max_seq=128)
    sp = SamplingParams(temperature=0.7, top_k=12, top_p=0.9, seed=20261016)
    first, N = 5, 40
    eng = _eng(model)
    rows_m, inner = [], eng.verify_sample

    def recording(tokens):
        n, acc = inner(tokens)
        rows_m.extend(eng.logits_m[:n + 1].clone())
        return n, acc
    eng.verify_sample = recording
    runs = []
    for _ in range(2):
        del rows_m[:]
        eng.set_position(0)
        runs.append(assisted_generate(eng, PromptLookupDraft(), first, N, 4, sampling=sp))
    assert runs[0] == runs[1] and len(runs[0][0]) == N
    out = runs[0][0]
    e1 = DecodeEngine(model, use_graph=True, kv_dtype="fp8")      # the one-row engine along the emitted stream
    e1.set_sampling(sp)
    draws, rows_1 = [], []
    for x in [first] + out[:-1]:
        e1.tok.fill_(x)
        e1.step()
        draws.append(int(e1.tok.item()))
        rows_1.append(e1.logits[0].clone())
    T, k, p = float(np.float32(sp.temperature)), sp.top_k, float(np.float32(sp.top_p))
    u, _ = draw_u(sp.seed, [j + 1 for j in range(N)])
    mism = []
    for j in range(N):
        if draws[j] != out[j]:
            _, p1, _ = filter_probs(rows_1[j].cpu().double().numpy(), T, k, p)
            _, pm, _ = filter_probs(rows_m[j].cpu().double().numpy(), T, k, p)
            tol = 0.5 * np.abs(p1 - pm).sum() + 1e-6
            lo, hi = cdf_interval(p1, draws[j])
            assert min(abs(u[j] - lo), abs(u[j] - hi)) <= tol, (j, out[j], draws[j], float(u[j]), float(lo), float(hi), float(tol))
            mism.append(j)
    print(f"[kv8-verify sampled] {N} tokens, mismatches with the one-row draws (all within the rounding rule) at {mism}; "
          f"accepted {runs[0][1]}")


def test_cache_full_and_roll_back():
    from qeft_amd.llama import DecodeEngine, QuantLlama
    model = _tiny(seed=3, n_layers=1, max_seq=32)
    eng = _eng(model, use_graph=False)
    eng.set_position(28)
    with pytest.raises(RuntimeError, match="max_seq"):
        eng.verify([1, 2, 3, 4, 5])
    eng.verify([1, 2, 3, 4])                                # 28 .. 31: the last rows of the cache
    assert eng.host_pos == 32
    # a greedy pass that rejects drafts leaves stale rows behind host_pos; a step() from there never reads them
    golden = QuantLlama.from_packed(GOLDEN, device=DEV, max_seq=64)
    hist = torch.randint(0, golden.shape.vocab, (9,), generator=torch.Generator().manual_seed(5)).tolist()
    ref = DecodeEngine(golden, use_graph=True, kv_dtype="fp8")
    ref.greedy = True
    for t in hist:
        ref.tok.fill_(t)
        ref.step()
    own = int(ref.tok.item())                               # the target's own token after hist
    eng = _eng(golden)
    eng.greedy = True
    for t in hist[:-1]:
        eng.tok.fill_(t)
        eng.step()
    wrong = [(own + 1 + i) % golden.shape.vocab for i in range(5)]
    n, acc = eng.verify([hist[-1]] + wrong)                 # every draft rejected: rows 9 .. 13 stale, poisoned below
    assert n == 0 and len(acc) == 1 and eng.host_pos == 9 and int(eng.tok.item()) == acc[0]
    for li in range(golden.shape.n_layers):
        for c, s in ((eng.kc[li], eng.ks[li]), (eng.vc[li], eng.vs[li])):
            c[:, 9:] = NAN8
            s[:, 9:] = float("nan")
    ref.tok.fill_(acc[0])
    ref.step()
    eng.step()
    dl = (eng.logits.float() - ref.logits.float()).abs().max().item()
    print(f"[kv8-verify roll-back] accepted {acc[0]} (one-row engine's own {own}); max|dlogit| after the pass = {dl:.6e}")
    assert torch.isfinite(eng.logits.float()).all() and dl <= 4 * MEASURED_DLOGIT, dl
