"""fp64 parity of the verify pass at the shapes the engine serves (Llama-2-7B / 13B / 70B) and in every launch geometry its
m-row kernels take there: the m-row GEMV per row-set count and x source (LDS / global), in each engine mode; the m-row
attention with the GQA group split into chunks, split 1..8, long contexts, an out_pos scatter, both rotary-table forms and
adversarial score patterns; the m-row head at H = 5120 / 8192; DecodeEngine.verify on 2-layer 13B and 70B models across
positions 256 and 1536.  Each m-row launch is compared with a plain high-precision reference of the same operation, not
only with one-row launches."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import qeft_oracle as O
from util import REL_TOL, elem_err_ok, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 128


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from qeft_amd import _lib
    return _lib.lib(), _lib.check


def _cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------
# 1. m-row GEMV on every engine linear
# ---------------------------------------------------------------------------------------------------------------------
# (n, k) of q|k|v, o_proj, gate|up (PAIR), down_proj -- as tests/test_verify_cpu.py::SHAPES
SHAPES = {
    "7b": [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)],
    "13b": [(15360, 5120), (5120, 5120), (27648, 5120), (5120, 13824)],
    "70b": [(10240, 8192), (8192, 8192), (57344, 8192), (8192, 28672)],
}
KINDS = ["qkv", "o", "gu", "down"]
# the launch geometry gemv_v3_plan (its engine-m clause) picks for m = 2..8: row sets per block (rs_cap), "X" = x
# read from global memory (m K does not fit LDS next to the block's scale / outlier slabs).  Read from qeft_gemv_v3_last_plan
# launch by launch: a planner change fails here.
GEOMETRY = {
    ("7b", "qkv"): ["3"] * 7, ("7b", "o"): ["1"] * 7, ("7b", "gu"): ["3"] * 7, ("7b", "down"): ["1"] * 5 + ["X1"] * 2,
    ("13b", "qkv"): ["4"] * 7, ("13b", "o"): ["2"] * 7, ("13b", "gu"): ["4"] * 7, ("13b", "down"): ["2"] * 3 + ["X2"] * 4,
    ("70b", "qkv"): ["3"] * 6 + ["X3"], ("70b", "o"): ["2"] * 7, ("70b", "gu"): ["3"] * 6 + ["X3"],
    ("70b", "down"): ["2"] + ["X2"] * 6,
}
GEOMETRY_NO_OUTLIERS = {("13b", "down"): GEOMETRY[("13b", "down")], ("70b", "down"): GEOMETRY[("70b", "down")]}
GEMV_CASES = [(s, kd, 128) for s in SHAPES for kd in KINDS] + [(s, kd, 0) for s, kd in GEOMETRY_NO_OUTLIERS]


def test_gemv_geometry_table_reaches_every_branch():
    """The table above (each entry checked against the launches below) covers rs_cap 1..4 with x in LDS and the XG form
    with rs_cap 1..3."""
    codes = {c for v in GEOMETRY.values() for c in v}
    assert {"1", "2", "3", "4"} <= codes and {"X1", "X2", "X3"} <= codes, sorted(codes)


def _modules(kind, n, k, n_out, seed):
    from qeft_amd import fuse
    from qeft_amd.llama import synthetic_quantlinear

    def ql(name, out_f, sd):
        return synthetic_quantlinear(name, k, out_f, n_out, 128, sd, DEV, fast_init=True)
    if kind == "qkv":
        kvd = (n - k) // 2
        mods = [ql("q", k, seed), ql("k", kvd, seed + 1), ql("v", kvd, seed + 2)]
        return mods, fuse.concat_linears(mods)
    if kind == "gu":
        mods = [ql("gate", n // 2, seed), ql("up", n // 2, seed + 1)]
        return mods, fuse.pair_interleave(*mods)
    mods = [ql(kind, n, seed)]
    return mods, fuse.single(mods[0])


def _dense(ql):
    """The module's dense weights in fp64 as the GEMV multiplies by them: every 4-bit weight the unrounded q * scale +
    scaled_zero (the kernel applies scale and zero to its sums, it never rounds a weight to fp16), outlier columns from
    oweight.  Rounded to fp16 they are qeft_dequant_w4's weights (bit-exact vs the oracle): asserted to the half unit."""
    from qeft_amd import qeft_cuda
    from qeft_amd.qlinear import unpack_intweight
    k, r = ql.infeatures, ql.outlierfeatures
    w = unpack_intweight(ql.qweight).double()
    w.mul_(ql.scales.double().t().repeat_interleave(128, 1)[:, :k]).add_(ql.scaled_zeros.double().t().repeat_interleave(128, 1)[:, :k])
    if r:
        w[:, k - r:] = ql.oweight[:, -r:].double()
    d = qeft_cuda.dequantize_weight_4bit_qeft(ql.qweight, ql.scales, ql.scaled_zeros, ql.oweight if r else None).double()
    assert ((w - d).abs() <= d.abs() * 2.0 ** -11 + 2.0 ** -25).all()
    return w


def _oracle_rows(ql, x, r0, r1):
    """The numpy oracle on output rows [r0, r1) of one module: its unrounded dense weights, x @ W^T accumulated in fp64."""
    qw = ql.qweight[r0 // 4:r1 // 4].cpu().numpy()
    sc, sz = ql.scales[:, r0:r1].cpu().numpy(), ql.scaled_zeros[:, r0:r1].cpu().numpy()
    ow = ql.oweight[r0:r1, -ql.outlierfeatures:].half().cpu().numpy() if ql.outlierfeatures else None
    return O.linear_f64(x.cpu().numpy(), O.dequant_dense(qw, sc, sz, ow, 128, round_fp16=False))


def _silu(t):
    return t / (1 + torch.exp(-t))


def _f16_around(t, slack):
    """The fp16 neighbours below and above every element of t (fp64) widened by `slack`: what an fp16 rounding of a value
    within `slack` of t can be."""
    lo, hi = t - slack, t + slack
    lo16, hi16 = lo.half(), hi.half()
    lo16 = torch.where(lo16.double() > lo, torch.nextafter(lo16, torch.full_like(lo16, float("-inf"))), lo16)
    hi16 = torch.where(hi16.double() < hi, torch.nextafter(hi16, torch.full_like(hi16, float("inf"))), hi16)
    return lo16.double(), hi16.double()


def _pair_bounds(gate, up):
    """Interval of the PAIR epilogue's fp16(silu(fp16 gate) * fp16 up) for the fp64 products gate / up: the fp32 sums may sit
    1e-5 (relative, plus 1e-4 of the rms) away from fp64 and round to either fp16 neighbour; silu and the product carry fp32
    rounding; the result is rounded to nearest (half a unit, 2^-11 relative)."""
    cands = []
    gl, gh = _f16_around(gate, 1e-5 * gate.abs() + 1e-4 * gate.pow(2).mean().sqrt())
    ul, uh = _f16_around(up, 1e-5 * up.abs() + 1e-4 * up.pow(2).mean().sqrt())
    for a in (gl, gh):
        for b in (ul, uh):
            cands.append(_silu(a) * b)
    c = torch.stack(cands)
    vmin, vmax = c.amin(0), c.amax(0)
    r = 2.0 ** -11 + 1e-5
    return vmin - r * vmin.abs() - 2.0 ** -24, vmax + r * vmax.abs() + 2.0 ** -24


def _gemv_launch(lib, ck, op, m, x, y, mode=0, residual=None, ssq_in=None, gamma=None, ynorm=None, ssq_out=None):
    p = lambda t: t.data_ptr() if t is not None else None       # noqa: E731
    ck(lib.qeft_decode_linear_m(p(x), op.qweight.data_ptr(), op.sz_packed.data_ptr(), p(op.oweight) if op.outlierfeatures else None,
                                None, p(y), op.outfeatures, op.infeatures, 128, op.outlierfeatures, mode, p(residual), p(ssq_in),
                                ssq_in.shape[1] if ssq_in is not None else 0, 1e-5, p(gamma), p(ynorm), p(ssq_out), m, _st()))


def _last_plan(lib):
    """qeft_gemv_v3_last_plan as a dict of the fields this file asserts."""
    import ctypes
    out = (ctypes.c_int * 13)()
    assert lib.qeft_gemv_v3_last_plan(out) == 0
    return dict(nblk=out[0], rs_cap=out[1], nw=out[4], D=out[5], fl=out[9], mb=out[10], xg=out[11])


def _close(got, ref, what):
    got, ref = got.double().cpu().numpy(), ref.double().cpu().numpy()
    assert np.isfinite(got).all(), what
    e = rel_err(got, ref)
    assert e < REL_TOL and elem_err_ok(got, ref), (what, e)
    return e


@pytest.mark.parametrize("shape,kind,n_out", GEMV_CASES)
def test_decode_linear_m_fp64(shape, kind, n_out):
    """Every engine linear of the shape, m = 2..8, in the engine's mode for it, against x @ W in fp64 over the dense weights
    of the same modules and, for a few row sets, against the numpy oracle."""
    from qeft_amd import _lib as L
    lib, ck = _lib()
    n, k = SHAPES[shape][KINDS.index(kind)]
    mods, op = _modules(kind, n, k, n_out, seed=100 * KINDS.index(kind) + len(shape))
    assert (op.outfeatures, op.infeatures, op.outlierfeatures) == (n, k, n_out)
    g = torch.Generator(device=DEV).manual_seed(n + k)
    x = (torch.randn(8, k, generator=g, device=DEV) * 0.5).half()
    nb = lib.qeft_decode_linear_blocks(n)
    # the raw products x W^T in fp64, per module (all 8 rows at once: m rows are a prefix), one dense weight alive at a time
    raw = []
    for ql in mods:
        w = _dense(ql)
        raw.append(x.double() @ w.t())
        del w
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    table = GEOMETRY_NO_OUTLIERS if n_out == 0 else GEOMETRY
    seen = []
    for m in range(2, 9):
        xm = x[:m].contiguous()
        if kind in ("qkv", "gu"):
            # q|k|v: > 256 sums (both 256-float pieces of the producer sums); gate|up: the engine's count, o_proj's blocks
            n_ssq = 300 if kind == "qkv" else lib.qeft_decode_linear_blocks(k)
            ssq = (torch.rand(m, n_ssq, generator=g, device=DEV) * 10 + 1)
            rs = 1.0 / torch.sqrt(ssq.double().sum(1, keepdim=True) / k + 1e-5)
            if kind == "qkv":
                y = torch.zeros(m, n, dtype=torch.float16, device=DEV)
                _gemv_launch(lib, ck, op, m, xm, y, ssq_in=ssq)
                variant, plan = L.last_variant(), _last_plan(lib)
                ref = torch.cat([r[:m] for r in raw], 1) * rs
                torch.cuda.synchronize()
                _close(y, ref, (shape, kind, m))
                # the oracle on the first row set of q and the last of v (deferred 1/rms applied to it)
                for j, r0 in ((0, 0), (2, mods[2].outfeatures - 16)):
                    yo = _oracle_rows(mods[j], xm, r0, r0 + 16) * rs.cpu().numpy()
                    c0 = sum(mm.outfeatures for mm in mods[:j]) + r0
                    assert rel_err(y[:, c0:c0 + 16].float().cpu().numpy(), yo) < REL_TOL, (shape, kind, m, j)
            else:
                y = torch.zeros(m, n // 2, dtype=torch.float16, device=DEV)
                _gemv_launch(lib, ck, op, m, xm, y, mode=1, ssq_in=ssq)
                variant, plan = L.last_variant(), _last_plan(lib)
                gt, up = raw[0][:m] * rs, raw[1][:m] * rs
                torch.cuda.synchronize()
                # per tensor: the one-row PAIR launch's bound against fp64 (tests/test_gpu_gemv_v3.py::test_gate_up_pair_silu:
                # gate, up and the product each rounded to fp16, so an element may move by 1-2 fp16 units)
                e = rel_err(y.float().cpu().numpy(), (_silu(gt) * up).cpu().numpy())
                assert e < 2e-3, (shape, kind, m, e)
                # per element: y must be what those three roundings can make of the fp64 gate and up
                lo, hi = _pair_bounds(gt, up)
                yd = y.double()
                bad = (yd < lo) | (yd > hi)
                assert not bad.any(), (shape, kind, m, int(bad.sum()), bad.nonzero()[:4].tolist())
                for r0 in (0, n // 2 - 16):
                    go, uo = (_oracle_rows(mods[j], xm, r0, r0 + 16) * rs.cpu().numpy() for j in (0, 1))
                    ro = go / (1 + np.exp(-go)) * uo
                    assert rel_err(y[:, r0:r0 + 16].float().cpu().numpy(), ro) < 2 * REL_TOL, (shape, kind, m, r0)
        else:
            h0 = torch.randn(m, n, generator=g, device=DEV)
            gamma = (torch.rand(n, generator=g, device=DEV) + 0.5).half()
            h = h0.clone()
            yn = torch.zeros(m, n, dtype=torch.float16, device=DEV)
            so = torch.full((m, nb), float("nan"), device=DEV)
            _gemv_launch(lib, ck, op, m, xm, h, residual=h, gamma=gamma, ynorm=yn, ssq_out=so)
            variant, plan = L.last_variant(), _last_plan(lib)
            prod = raw[0][:m]
            href = h0.double() + prod
            torch.cuda.synchronize()
            _close(h - h0, prod, (shape, kind, m, "W x"))
            _close(h, href, (shape, kind, m, "h_new"))
            _close(yn, href * gamma.double(), (shape, kind, m, "ynorm"))
            assert torch.isfinite(so).all(), (shape, kind, m)
            sref = href.pow(2).sum(-1)
            assert ((so.double().sum(-1) - sref).abs() / sref).max().item() < REL_TOL, (shape, kind, m, "ssq_out")
            assert ((so.double().sum(-1) - h.double().pow(2).sum(-1)).abs() / sref).max().item() < 1e-5, (shape, kind, m)
            for r0 in (0, n - 16):
                yo = _oracle_rows(mods[0], xm, r0, r0 + 16)
                assert rel_err((h - h0)[:, r0:r0 + 16].cpu().numpy(), yo) < REL_TOL, (shape, kind, m, r0)
        xg, rs_cap = bool(plan["xg"]), plan["rs_cap"]
        assert xg == variant.endswith("_xg") and rs_cap == _cdiv(n // 16, nb) and plan["nblk"] == nb, (plan, variant)
        want = "gemv_v3_multi_xg" if xg else ("gemv_v3_multi_pair" if kind == "gu" else "gemv_v3_multi")
        assert variant == want, (variant, want)
        # the ring: deep (4 loads, 6 with three or four row sets) for every xg launch and where a CU holds one block whose waves
        # have 8 loads or more to make; 8 waves, MB = 2 on the flag-free half
        deep = xg or (nb <= 256 and _cdiv((k - n_out) // 128, 8) * rs_cap >= 8)
        assert plan["D"] == ((6 if rs_cap >= 3 else 4) if deep else 2) and (plan["nw"], plan["fl"], plan["mb"]) == (8, 0, 2), (plan, m)
        code = ("X" if xg else "") + str(rs_cap)
        seen.append(code)
        print(f"[gemv-m] {shape:>3} {kind:>4} n_out={n_out:<3} m={m} variant={variant:<18} rs_cap={rs_cap} D={plan['D']} blocks={nb}")
    assert seen == table[(shape, kind)], (shape, kind, n_out, seen)
    del mods, op, raw
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 2. m-row attention against fp64 causal attention
# ---------------------------------------------------------------------------------------------------------------------
def _chunk(grp, m):
    """attn_m_chunk (decode_verify.hip): query heads per block, the largest divisor of the group with hc * m <= 32."""
    hc = max(d for d in range(1, grp + 1) if grp % d == 0 and d * m <= 32)
    rows = hc * m
    return hc, grp // hc, 8 if rows <= 8 else 16 if rows <= 16 else 32


def _rot(x, c, s):          # x [..., 128] fp32, c / s [..., 64]: neox-style rotary, as the kernels
    a, b = x[..., :64], x[..., 64:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


class _Attn:
    """One head layout on one max_seq: caches, rotary tables and one workspace shared by every launch."""

    def __init__(self, heads, kv, max_seq, seed):
        self.lib, self.ck = _lib()
        self.heads, self.kv, self.max_seq = heads, kv, max_seq
        self.g = torch.Generator(device=DEV).manual_seed(seed)
        self.nq = (heads + 2 * kv) * HD
        self.kc = (torch.randn(kv, max_seq, HD, generator=self.g, device=DEV) * 0.5).half()
        self.vc = (torch.randn(kv, max_seq, HD, generator=self.g, device=DEV) * 0.5).half()
        self.ws = torch.zeros(max(self.lib.qeft_attn_m_workspace_bytes(heads, 8, 8), 16) // 4, device=DEV)
        self.tables(torch.randn(max_seq, 64, generator=self.g, device=DEV))

    def tables(self, ang):
        self.cos, self.sin = ang.cos().contiguous(), ang.sin().contiguous()

    def launch(self, qkv, m, pos, split, out, form="pos", out_pos=None):
        qp, pos_t = qkv.data_ptr(), torch.tensor([pos], dtype=torch.int32, device=DEV)
        if form == "pos":           # tables indexed by position
            cs, sn, stride, rows = self.cos.data_ptr(), self.sin.data_ptr(), 64, self.max_seq
        else:                       # the engine's form: m rows of [cos | sin], 128 floats apart
            self._rows = torch.cat([self.cos[pos:pos + m], self.sin[pos:pos + m]], 1).contiguous()
            cs, sn, stride, rows = self._rows.data_ptr(), self._rows.data_ptr() + 64 * 4, 128, m
        self.ck(self.lib.qeft_rope_attn_decode_m(qp, qp + self.heads * HD * 2, qp + (self.heads + self.kv) * HD * 2, self.nq, cs, sn,
                                                 stride, rows, self.kc.data_ptr(), self.vc.data_ptr(), pos_t.data_ptr(),
                                                 out_pos.data_ptr() if out_pos is not None else None, out.data_ptr(),
                                                 self.heads * HD, self.ws.data_ptr(), split, self.heads, self.kv, self.max_seq, m,
                                                 _st()))
        self._keep = pos_t          # alive until the launch has run

    def out(self, m):
        return torch.full((m, self.heads * HD), float("nan"), dtype=torch.float16, device=DEV)

    def reference(self, qkv, m, pos):
        """fp64 causal attention over the caches as the launch left them (rows < pos + m): q rotated in fp32, scaled and
        rounded to fp16 as the kernel does; query i sees keys 0 .. pos + i."""
        heads, grp = self.heads, self.heads // self.kv
        q = _rot(qkv[:, :heads * HD].float().view(m, heads, HD), self.cos[pos:pos + m, None], self.sin[pos:pos + m, None])
        q = (q * HD ** -0.5).half().double()
        Lk = pos + m
        K = self.kc[:, :Lk].double().repeat_interleave(grp, 0)
        V = self.vc[:, :Lk].double().repeat_interleave(grp, 0)
        sc = torch.einsum("mhd,hld->hml", q, K)
        mask = torch.arange(Lk, device=DEV)[None, :] > (pos + torch.arange(m, device=DEV))[:, None]
        sc = sc.masked_fill(mask[None], float("-inf"))
        return torch.einsum("hml,hld->mhd", sc.softmax(-1), V).reshape(m, heads * HD)

    def check_append(self, qkv, m, pos, k_before, v_before):
        """The launch's m K/V rows: v verbatim, k rotated (one fp16 unit at most from the fp32 formula); no other row moved."""
        heads, kv = self.heads, self.kv
        kn = qkv[:, heads * HD:(heads + kv) * HD].float().view(m, kv, HD)
        kr = _rot(kn, self.cos[pos:pos + m, None], self.sin[pos:pos + m, None]).transpose(0, 1)
        vn = qkv[:, (heads + kv) * HD:].view(m, kv, HD).transpose(0, 1)
        assert torch.equal(self.vc[:, pos:pos + m], vn)
        dk = (self.kc[:, pos:pos + m].float() - kr).abs()
        assert (dk <= kr.abs() * 2.0 ** -10 + 2.0 ** -24).all(), dk.max().item()
        assert torch.equal(self.kc[:, :pos], k_before[:, :pos]) and torch.equal(self.kc[:, pos + m:], k_before[:, pos + m:])
        assert torch.equal(self.vc[:, :pos], v_before[:, :pos]) and torch.equal(self.vc[:, pos + m:], v_before[:, pos + m:])


def _attn_close(got, ref, what):
    got = got.double().view(got.shape[0], -1, HD)
    ref = ref.view(got.shape)
    assert torch.isfinite(got).all(), what
    tol = 2e-3 + 2e-3 * ref.abs().amax(-1, keepdim=True)
    bad = (got - ref).abs() > tol
    assert not bad.any(), (what, (got - ref).abs().max().item(), bad.nonzero()[:4].tolist())


LAYOUTS = [(40, 40), (64, 8), (32, 1), (40, 8)]


@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_attention_m_fp64(heads, kv):
    """m = 1..8 x split 1/2/4/8 x positions 0, 1000 and max_seq - m on a 4096-row cache, against fp64 causal attention;
    both rotary-table forms (bit-identical), an out_pos scatter (bit-identical to the plain rows), repeated launches of
    one configuration (bit-identical) and launches of other (m, split) on the same workspace in between."""
    A = _Attn(heads, kv, 4096, seed=heads * 10 + kv)
    grp = heads // kv
    for m in range(1, 9):
        hc, n_chunk, R = _chunk(grp, m)
        print(f"[attn-m] heads={heads:<2} kv={kv:<2} m={m} hc={hc:<2} n_chunk={n_chunk} R={R}")
        for pos in (0, 1000, A.max_seq - m):
            qkv = torch.randn(m, A.nq, generator=A.g, device=DEV).half()
            k_before, v_before = A.kc.clone(), A.vc.clone()
            outs = {}
            for split in (1, 2, 4, 8):
                for form in ("pos", "rows"):
                    o = A.out(m)
                    A.launch(qkv, m, pos, split, o, form)
                    outs[split, form] = o
            torch.cuda.synchronize()
            A.check_append(qkv, m, pos, k_before, v_before)
            ref = A.reference(qkv, m, pos)
            for split in (1, 2, 4, 8):
                _attn_close(outs[split, "pos"], ref, (heads, kv, m, pos, split))
                assert torch.equal(outs[split, "pos"], outs[split, "rows"]), (heads, kv, m, pos, split)
            # out_pos: a permutation of the output columns (the engine passes o_proj's column order)
            perm = torch.randperm(heads * HD, generator=A.g, device=DEV).to(torch.int32)
            op = torch.zeros(m, heads * HD, dtype=torch.float16, device=DEV)
            A.launch(qkv, m, pos, 4, op, "rows", out_pos=perm)
            torch.cuda.synchronize()
            assert torch.equal(op[:, perm.long()], outs[4, "rows"]), (heads, kv, m, pos)
        # determinism: S > 1 launches back to back without a host sync; other (m, split) on the same workspace in between
        pos = 1000
        qkv = torch.randn(m, A.nq, generator=A.g, device=DEV).half()
        m2 = max(1, m - 3)
        rep = [A.out(m) for _ in range(3)]
        for o in rep:
            A.launch(qkv, m, pos, 8, o)
        o2, o4, last = A.out(m2), A.out(m), A.out(m)
        A.launch(qkv[:m2].contiguous(), m2, pos, 2, o2)
        A.launch(qkv, m, pos, 4, o4)
        A.launch(qkv, m, pos, 8, last)
        torch.cuda.synchronize()
        for o in rep[1:] + [last]:
            assert torch.equal(o, rep[0]), (heads, kv, m)
        ref = A.reference(qkv, m, pos)
        _attn_close(rep[0], ref, (heads, kv, m, "rep"))
        _attn_close(o4, ref, (heads, kv, m, "interleaved"))
        _attn_close(o2, ref[:m2], (heads, kv, m2, "interleaved"))
    del A
    torch.cuda.empty_cache()


@pytest.mark.parametrize("heads,kv", LAYOUTS)
@pytest.mark.parametrize("case", ["sink", "new_max", "equal"])
def test_attention_m_adversarial(heads, kv, case):
    """Score patterns where a wrong rescale or merge shows: a key ~35 nats above the rest in a later run of a wave of a split
    other than the one of the queries' own rows ("sink"); the maximum among this launch's appended keys ("new_max"); all
    visible keys equal ("equal": the plain mean of the values).  The values carry a ramp over the positions, so that a
    dropped or double-counted run moves the result."""
    A = _Attn(heads, kv, 2048, seed=7 * heads + kv)
    pos = 1000
    ramp = (torch.arange(A.max_seq, device=DEV, dtype=torch.float32) / 1024)[None, :, None]
    A.vc = (A.vc.float() + ramp).half()
    ang = torch.randn(A.max_seq, 64, generator=A.g, device=DEV)
    ang[:, 0] = 0.0                                  # rotary pair (0, 64) left as it is: dimension 0 lines q and k up
    if case == "equal":
        ang.zero_()
        A.kc.copy_(A.kc[:, :1].clone().expand_as(A.kc))
    A.tables(ang)
    for m in range(1, 9):
        for split in (1, 2, 4, 8):
            qkv = torch.randn(m, A.nq, generator=A.g, device=DEV).half()
            kq = qkv[:, heads * HD:(heads + kv) * HD].view(m, kv, HD)
            if case == "equal":
                kq.copy_(A.kc[:, 0][None].expand(m, kv, HD))
            else:
                qkv[:, :heads * HD].view(m, heads, HD)[:, :, 0] = 8.0
                if case == "sink":
                    # the queries' own run and its split; the sink in the next split's wave 1, in that wave's second run
                    last = (pos + m - 1) // 16
                    own = (last % (4 * split)) // 4
                    js = 4 * split + 4 * ((own + 1) % split) + 1
                    assert js < last and (js % (4 * split)) // 4 != own or split == 1
                    A.kc[:, 16 * js + 7, 0] = 50.0
                else:
                    kq[m // 2, :, 0] = 50.0               # visible to queries i >= m // 2 only
            out = A.out(m)
            A.launch(qkv, m, pos, split, out, "rows" if split % 4 else "pos")
            torch.cuda.synchronize()
            ref = A.reference(qkv, m, pos)
            _attn_close(out, ref, (heads, kv, case, m, split))
            if case == "sink":
                A.kc[:, 16 * js + 7, 0] = 0.0
    del A
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 3. m-row head at the 13B / 70B widths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [5120, 8192])
def test_lm_head_m_wide(H):
    """H = 5120 (10 loads per row and lane) and 8192 (16; 128 KB of LDS at m = 8): bit-equal to the one-row head, and within
    2e-3 of an fp64 RMSNorm + matmul (normalised rows rounded to fp16 as the kernels do)."""
    lib, ck = _lib()
    g = torch.Generator(device=DEV).manual_seed(H)
    gamma = (torch.rand(H, generator=g, device=DEV) + 0.5).half()
    for vocab in (32000, 4095, 4097, 7):
        W = (torch.randn(vocab, H, generator=g, device=DEV) * 0.02).half()
        for m in (1, 3, 8):
            h = torch.randn(m, H, generator=g, device=DEV) * 3
            lg = torch.full((m, vocab), float("nan"), dtype=torch.float16, device=DEV)
            ck(lib.qeft_lm_head_f16_m(h.data_ptr(), gamma.data_ptr(), W.data_ptr(), lg.data_ptr(), H, vocab, 1e-5, m, _st()))
            one = torch.full((m, vocab), float("nan"), dtype=torch.float16, device=DEV)
            for i in range(m):
                hi = h[i].contiguous()
                ck(lib.qeft_lm_head_f16(hi.data_ptr(), gamma.data_ptr(), W.data_ptr(), one[i].data_ptr(), H, vocab, 1e-5, _st()))
                torch.cuda.synchronize()
            assert torch.equal(lg, one), (H, vocab, m)
            hd = h.double()
            xn = (hd * torch.rsqrt(hd.pow(2).mean(-1, keepdim=True) + 1e-5) * gamma.double()).half().double()
            ref = xn @ W.double().t()
            assert rel_err(lg.float().cpu().numpy(), ref.cpu().numpy()) < 2e-3, (H, vocab, m)
        print(f"[head-m] H={H} LPR={H // 512} vocab={vocab} m=1,3,8 ok")


# ---------------------------------------------------------------------------------------------------------------------
# 4. DecodeEngine.verify on 2-layer 13B and 70B shapes
# ---------------------------------------------------------------------------------------------------------------------
P0, T_END = 248, 1560          # the cache is filled to P0, then positions P0 .. T_END - 1 run as verify chunks (across 256, 1536)
CHUNKS = [8, 5, 3, 7, 1, 8, 6, 2, 4, 8, 8]


def _chunks():
    out, p = [], P0
    while p < T_END:
        c = min(CHUNKS[len(out) % len(CHUNKS)], T_END - p)
        out.append(c)
        p += c
    return out


@pytest.fixture(scope="module", params=["13b", "70b"])
def engine_case(request):
    """A 2-layer model of the shape, its token sequence, the teacher-forced one-token rows over P0 .. T_END - 1 (from a cache
    filled by prefill) and the rows of the first 8 positions."""
    from qeft_amd.llama import LLAMA2_13B, LLAMA2_70B, DecodeEngine, QuantLlama, prefill
    base = {"13b": LLAMA2_13B, "70b": LLAMA2_70B}[request.param]
    shape = dataclasses.replace(base, n_layers=2, max_seq=2048, name=base.name + "-2layers")
    model = QuantLlama(shape, DEV, seed=5, fast_init=True)
    tokens = torch.randint(0, shape.vocab, (T_END + 8,), generator=torch.Generator().manual_seed(9))
    ref_eng = DecodeEngine(model, use_graph=True)
    prefill(model, tokens[:P0].to(DEV), engine=ref_eng)
    caches = ([k.clone() for k in ref_eng.kc], [v.clone() for v in ref_eng.vc])
    ref_eng.greedy = False
    rows = []
    for t in tokens[P0:T_END].tolist():
        ref_eng.tok.fill_(t)
        ref_eng.step()
        rows.append(ref_eng.logits[0].float().clone())
    first = ref_eng.teacher_forced_logits(tokens[:8].to(DEV))
    torch.cuda.synchronize()
    del ref_eng
    yield request.param, model, tokens, caches, torch.stack(rows), first
    del model, caches, rows, first
    torch.cuda.empty_cache()


def _load_cache(eng, caches):
    for li in range(len(eng.kc)):
        eng.kc[li].copy_(caches[0][li])
        eng.vc[li].copy_(caches[1][li])
    eng.set_position(P0)


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_verify_large_shapes(engine_case, use_graph):
    """verify() chunks of 1..8 tokens over positions 248 .. 1559 (split 1 -> 4 -> 8; on 70B the attention splits its GQA
    group into chunks at m >= 5) against the teacher-forced step() rows of the same positions, and a first chunk of 8 at
    position 0; the graph run equals the eager run."""
    from qeft_amd.llama import DecodeEngine
    name, model, tokens, caches, ref, first = engine_case
    eng = DecodeEngine(model, use_graph=use_graph)
    eng.greedy = False
    _load_cache(eng, caches)
    got = []
    for c in _chunks():
        i = eng.host_pos
        assert eng.verify(tokens[i:i + c]) is None
        got.append(eng.logits_m[:c].float().clone())
    got = torch.cat(got)
    assert eng.host_pos == T_END
    eng.reset()
    eng.verify(tokens[:8])
    got0 = eng.logits_m[:8].float().clone()
    torch.cuda.synchronize()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item() / scale
    err0 = (got0 - first).abs().max().item() / first.abs().max().item()
    print(f"[verify {name} graph={use_graph}] max|d|/max|ref| = {err:.3e} (positions {P0}..{T_END - 1}), {err0:.3e} (0..7)")
    assert torch.isfinite(got).all() and err < 1e-2 and err0 < 1e-2, (err, err0)
    if use_graph:
        assert {kk[2] for kk in eng.graphs if kk[0] == "verify"} == {1, 4, 8}
        eager = DecodeEngine(model, use_graph=False)
        eager.greedy = False
        _load_cache(eager, caches)
        rows = []
        for c in _chunks():
            i = eager.host_pos
            eager.verify(tokens[i:i + c])
            rows.append(eager.logits_m[:c].float().clone())
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(rows), got)


def test_engine_verify_large_shapes_dense_reference(engine_case):
    """The same verify rows against the plain fp32 model over the dense weights (positions 0 .. T_END - 1 fed at once):
    within the tolerance of the 70B-shape engine test, and the same argmax wherever the reference's top-2 gap is clear."""
    from qeft_amd.llama import DecodeEngine, prefill
    name, model, tokens, caches, ref, first = engine_case
    dense = model.dense_weights()
    dref = model.forward_dense_reference(tokens[:T_END].to(DEV), dense)
    del dense
    eng = DecodeEngine(model, use_graph=True)
    eng.greedy = False
    prefill(model, tokens[:P0].to(DEV), engine=eng)
    got = []
    for c in _chunks():
        i = eng.host_pos
        eng.verify(tokens[i:i + c])
        got.append(eng.logits_m[:c].float().clone())
    got = torch.cat(got)
    torch.cuda.synchronize()
    r = dref[P0:T_END]
    scale = r.abs().max().item()
    err = (got - r).abs().max().item() / scale
    top2 = r.topk(2, dim=-1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * 6e-3 * scale
    print(f"[verify {name} vs dense fp32] max|d|/max|ref| = {err:.3e}; {int(sure.sum())} of {sure.numel()} rows with a clear top-2 gap")
    assert err < 6e-3, err
    assert torch.equal(got.argmax(-1)[sure], r.argmax(-1)[sure])

    # one greedy pass whose drafts are the target's own one-token greedy choices: every draft up to the first unclear gap
    # is accepted
    p = 1530
    eng.greedy = True
    eng.set_position(p)
    eng.tok.fill_(int(tokens[p]))
    drafts, gaps = [], []
    for _ in range(7):
        eng.step()
        lg = eng.logits[0].float()
        t2 = lg.topk(2).values
        drafts.append(int(eng.tok.item()))
        gaps.append((t2[0] - t2[1]).item())
    clear = next((j for j, gp in enumerate(gaps) if gp <= 2e-2 * scale), 7)
    eng.set_position(p)
    n, acc = eng.verify([int(tokens[p])] + drafts)
    print(f"[verify {name} greedy] drafts {drafts}, gaps {[round(x, 3) for x in gaps]}: accepted {n}")
    assert n >= clear and acc[:n] == drafts[:n], (n, clear, acc, drafts)
    assert eng.host_pos == p + n + 1
