"""The training glue (csrc/train_glue.hip: qeft_add_rmsnorm_fwd / _bwd, qeft_swiglu_fwd / _bwd) through the C ABI,
through qeft_amd.glue and through finetune.causal_lm_loss(glue="fused")  (DESIGN.md section 4.16).

Every operand of every launch is a view in the middle of a larger buffer of fp16 / fp32 NaN (8192 elements on either side, NaN
gaps between padded rows); outputs start as NaN, and after a launch everything around the views is still NaN.  The fp64
references are formed from the kernel's own fp16 / fp32 inputs, never from another kernel's output.

Forwards: bit for bit qeft_rmsnorm and qeft_silu_mul.

Backwards against fp64, element-wise:  |got - ref| <= ulp16(ref) + 1.001 c u sum|terms|,  u = 2^-24 (the unit roundoff of fp32).
ulp16(ref) is the final rounding (1/2 ulp) and room for a tie that flips, as B1 of tests/test_gpu_rowwise.py; 1.001 covers the
second-order terms; `terms` are the summands whose cancellation the result can suffer, and c counts, to first order, the fp32
roundings that reach the largest of them.  Every fp32 add, multiply, FMA and division is <= 1 u relative; rsqrtf, __expf's
exponential and the hardware reciprocal are 1 ulp = 2 u (HIP's documented accuracy of the three).

  norm.   dsum = dres + r (gamma dy - s cc),  r = rsqrt(ss / H + eps),  cc = dot r^2 (1 / H),  ss = sum s^2,  dot = sum gamma dy s.
          terms  T1 = |dres|,  T2 = |r gamma dy|,  T3 = |r xhat| (1 / H) sum_k |gamma dy xhat|  (xhat = s r).
          Both sums have depth D = P + 12, P = ceil(H / 2048) passes: 4 for a chunk of 8 (product, tree of 3), 1 per pass, 6 for
          the wave (4 DPP steps, 2 adds of read lanes), 2 across the 4 waves; ss has positive terms only.
            r:   (D + 2) / 2 + 2 = D / 2 + 3        (ss, the division, + eps; halved by the root; rsqrtf)
            cc:  (D + 2) + (D + 7) + 1 + 2 = 2 D + 12   (dot with two products per term; r r; the product; 1 / H and its product)
            T1:  1 (the last add);   T2:  1 + 1 + 1 + (D / 2 + 3) + 1 = D / 2 + 7   (gamma dy, the subtraction, r ., r, the last add)
            T3:  (2 D + 12) + 1 + 1 + 1 + (D / 2 + 3) + 1 = 2.5 D + 19              (cc, s cc, the subtraction, r ., r, the last add)
          c = 2.5 D + 19: 51.5 for H <= 2048, 59 at H = 8192 (asserted <= 64 for every width below).
  SwiGLU. z = __expf(-|g|): the argument's product with log2(e) moves the result by <= 2 |g| u, the exponential by 2 u.
          p = rcp(1 + z) = sigma(|g|): 1 + 2 u and z's error scaled by z / (1 + z), (2 |g| + 2) z / (1 + z) <= 2 -> 5 u.
          z p = sigma(-|g|) = 1 - p:  (2 |g| + 2) + 5 + 1 = 2 |g| + 8.   g >= 0: sigma = p, 1 - sigma = z p;  g < 0: swapped.
          dup = dact g sigma, term |dact g sigma|:  sigma + 2 products <= 2 |g| + 10.
          dgate = A (1 + g (1 - sigma)),  A = dact u sigma;  terms  |A|,  |A g (1 - sigma)|:
            on |A|:  sigma + 2 (its products) + 1 (1 + .) + 1 (the last product) <= 2 |g| + 12
            on |A g (1 - sigma)|:  sigma + 2 + (1 - sigma) + 1 (g .) + 1 + 1;  sigma and 1 - sigma together 2 |g| + 13 -> 2 |g| + 18
          c(g) = min(64, 2 |g| + 18).  The cap binds for |g| > 23 only, where it loses nothing: for g > 23 the term that carries
          2 |g| + 18 is |A| g e^-g < 2^-28 |A| and |A| itself carries 9; for g < -23 both terms are below 2^-28 |dact u|, so the
          uncounted (2 |g| - 46) u of them is under 2^-40 |dact u| -- inside the 1/2 ulp of room in ulp16(ref) >= 2^-24 while
          |dact u| < 2^15, which the test asserts of its data.
Every case prints its largest error / bound ([train_glue] ...); DESIGN.md section 4.16 records them."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
BAND = 8192
U = 2.0 ** -24
EPS = 1e-5
EPS64 = float(torch.tensor(EPS, dtype=F32))         # what the entry receives
IGNORE = -100
NORM_H = [8, 128, 2048, 2056, 4096, 5120, 8192]
ROWS = [1, 3, 65]
SWIGLU_N = [8, 512, 2056, 11008, 28672]
GRAD_SCALES = [2.0 ** -4, 2.0 ** -16]               # a loss-scaled step's gradients; the same in fp16's subnormal range


def _st():
    return torch.cuda.current_stream().cuda_stream


def _L():
    from qeft_amd import _lib
    return _lib, _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Banded:
    """rows x width elements, rows `stride` apart, in the middle of a NaN buffer: .v is the view, intact() says that everything
    around it still is NaN."""

    def __init__(self, rows, width, stride=None, dtype=F16, init=None):
        self.rows, self.width, self.stride = rows, width, stride or width
        self.raw = torch.full((2 * BAND + rows * self.stride,), float("nan"), dtype=dtype, device=DEV)
        self.v = self.raw[BAND:BAND + rows * self.stride].view(rows, self.stride)[:, :width]
        assert self.v.data_ptr() % 16 == 0
        if init is not None:
            self.v[:] = init

    def intact(self):
        tmp = self.raw.clone()
        tmp[BAND:BAND + self.rows * self.stride].view(self.rows, self.stride)[:, :self.width] = float("nan")
        return bool(torch.isnan(tmp).all())

    def ptr(self, row=0):
        return self.v[row].data_ptr()


def _ulp16(ref):
    a = ref.abs()
    _, e = torch.frexp(a)
    u = torch.ldexp(torch.ones_like(a), e - 11)
    return torch.where(a > 0, u, torch.zeros_like(a)).clamp_min(2.0 ** -24)


WORST = {}


def _check(kernel, case, got, ref, bound):
    assert torch.isfinite(got).all(), f"{kernel} {case}: non-finite output"
    ratio = (got.double() - ref).abs() / bound
    worst = ratio.max().item()
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    print(f"[train_glue] {kernel} {case}: largest err / bound = {worst:.4f}")
    assert worst <= 1.0, f"{kernel} {case}: err / bound {worst:.3f} at {divmod(int(ratio.argmax()), ratio.shape[-1])}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\n[train_glue] {k}: largest err / bound over all cases = {WORST[k]:.4f}", end="")
    print()


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator(device=DEV).manual_seed(seed % (2 ** 31))


def _outlier_rows(m, n, g, zero_row=True):
    """x ~ N(0, 1) with a few columns x 50 (outlier channels are this project's subject) and, from 3 rows on, one all-zero row."""
    x = torch.randn(m, n, generator=g, device=DEV)
    cols = torch.randperm(n, generator=g, device=DEV)[:max(1, min(4, n // 4))]
    x[:, cols] *= 50.0
    if zero_row and m >= 3:
        x[m // 2] = 0.0
    return x


# ================================================================================================ RMSNorm + residual add
def _norm_c(H):
    D = (H + 2047) // 2048 + 12
    return 2.5 * D + 19


def _norm_ops(m, H, scale):
    g = _gen(1, m, H, int(-math.log2(scale)))
    h, add = _outlier_rows(m, H, g).half(), _outlier_rows(m, H, g).half()
    gamma = (1 + 0.1 * torch.randn(H, generator=g, device=DEV)).half()
    dy = (torch.randn(m, H, generator=g, device=DEV) * scale).half()
    dres = (torch.randn(m, H, generator=g, device=DEV) * scale).half()
    return h, add, gamma, dy, dres


def _norm_bwd64(s, gamma, dy, dres):
    """(ref, sum of the terms) of the module docstring in fp64; dy / dres may be None."""
    S, G = s.double(), gamma.double()
    H = S.shape[1]
    r = 1.0 / torch.sqrt((S * S).mean(-1, keepdim=True) + EPS64)
    xh = S * r
    ref = torch.zeros_like(S)
    terms = torch.zeros_like(S)
    if dres is not None:
        ref = ref + dres.double()
        terms = terms + dres.double().abs()
    if dy is not None:
        gd = G * dy.double()
        c = (gd * xh).sum(-1, keepdim=True) / H
        ref = ref + r * (gd - xh * c)
        terms = terms + (r * gd).abs() + (r * xh).abs() * (gd * xh).abs().sum(-1, keepdim=True) / H
    return ref, terms


def _run_norm_fwd(h, add, gamma):
    _lib, lib = _L()
    m, H = h.shape
    hb, gb = _Banded(m, H, init=h), _Banded(1, H, init=gamma)
    ab = _Banded(m, H, init=add) if add is not None else None
    sb = _Banded(m, H) if add is not None else None
    yb = _Banded(m, H)
    _lib.check(lib.qeft_add_rmsnorm_fwd(hb.ptr(), ab.ptr() if ab else None, gb.ptr(), sb.ptr() if sb else None, yb.ptr(), m, H, EPS, _st()))
    torch.cuda.synchronize()
    for b in (hb, gb, ab, sb, yb):
        assert b is None or b.intact()
    assert _same(hb.v, h) and (ab is None or _same(ab.v, add))
    return (sb.v if sb else None), yb.v


def _run_norm_bwd(s, gamma, dy, dres, rows=None):
    """rows = (first, count): that slice of the operands alone, through pointers into the same buffers."""
    _lib, lib = _L()
    m, H = s.shape
    first, count = rows or (0, m)
    sb, gb = _Banded(m, H, init=s), _Banded(1, H, init=gamma)
    yb = _Banded(m, H, init=dy) if dy is not None else None
    rb = _Banded(m, H, init=dres) if dres is not None else None
    ob = _Banded(count, H)
    _lib.check(lib.qeft_add_rmsnorm_bwd(sb.ptr(first), gb.ptr(), yb.ptr(first) if yb else None, rb.ptr(first) if rb else None, ob.ptr(),
                                        count, H, EPS, _st()))
    torch.cuda.synchronize()
    for b in (sb, gb, yb, rb, ob):
        assert b is None or b.intact()
    return ob.v


@pytest.mark.parametrize("H", NORM_H)
def test_add_rmsnorm_forward_has_the_bits_of_qeft_rmsnorm(H):
    _lib, lib = _L()
    for m in ROWS:
        h, add, gamma, _, _ = _norm_ops(m, H, 2.0 ** -4)
        for with_add in (True, False):
            s, y = _run_norm_fwd(h, add if with_add else None, gamma)
            want_s, want_y = torch.full_like(h, float("nan")), torch.full_like(h, float("nan"))
            _lib.check(lib.qeft_rmsnorm(h.data_ptr(), add.data_ptr() if with_add else None, gamma.data_ptr(),
                                        want_s.data_ptr() if with_add else None, want_y.data_ptr(), m, H, EPS, _st()))
            torch.cuda.synchronize()
            assert _same(y, want_y), (H, m, with_add)
            assert torch.isfinite(y).all()
            if with_add:
                assert _same(s, want_s) and _same(s, (h.float() + add.float()).half()), (H, m)
            if m >= 3:
                assert (y[m // 2] == 0).all()
    print(f"[train_glue] add_rmsnorm_fwd H={H}: sum_out and y bit-equal to qeft_rmsnorm, m in {ROWS}, with and without add")


@pytest.mark.parametrize("H", NORM_H)
def test_add_rmsnorm_backward_against_fp64(H):
    c = _norm_c(H)
    assert c <= 64
    for m in ROWS:
        for scale in GRAD_SCALES:
            h, add, gamma, dy, dres = _norm_ops(m, H, scale)
            for with_add in (True, False):
                s = (h.float() + add.float()).half() if with_add else h
                for with_dy, with_dres in ((True, True), (True, False), (False, True)):
                    got = _run_norm_bwd(s, gamma, dy if with_dy else None, dres if with_dres else None)
                    case = f"H={H} m={m} add={int(with_add)} dy={int(with_dy)} dres={int(with_dres)} grads 2^{int(math.log2(scale))}"
                    if not with_dy:
                        assert _same(got, dres), case                  # nothing to add: the residual gradient itself
                        continue
                    ref, terms = _norm_bwd64(s, gamma, dy, dres if with_dres else None)
                    _check("add_rmsnorm_bwd", case, got, ref, _ulp16(ref) + 1.001 * c * U * terms)
                    assert got.abs().max() > 0


@pytest.mark.parametrize("H", [8, 2056, 8192])
def test_add_rmsnorm_rows_do_not_depend_on_the_launch(H):
    """Rows 0, 32 (the zero row) and 64 of the m = 65 launches equal the same rows launched alone, bit for bit."""
    m = 65
    h, add, gamma, dy, dres = _norm_ops(m, H, 2.0 ** -4)
    s, y = _run_norm_fwd(h, add, gamma)
    d = _run_norm_bwd(s, gamma, dy, dres)
    for row in (0, 32, 64):
        s1, y1 = _run_norm_fwd(h[row:row + 1], add[row:row + 1], gamma)
        assert _same(s1, s[row:row + 1]) and _same(y1, y[row:row + 1]), (H, row)
        assert _same(_run_norm_bwd(s[row:row + 1].clone(), gamma, dy[row:row + 1], dres[row:row + 1]), d[row:row + 1]), (H, row)
        assert _same(_run_norm_bwd(s.clone(), gamma, dy, dres, rows=(row, 1)), d[row:row + 1]), (H, row)
    assert _same(_run_norm_bwd(s.clone(), gamma, dy, dres, rows=(60, 5)), d[60:65])
    print(f"[train_glue] add_rmsnorm H={H}: rows of an m = 65 launch equal the rows launched alone, forward and backward")


# ================================================================================================ SwiGLU
SPECIAL_GATES = [65504.0, -65504.0, 20.0, -20.0, 0.0, -0.0, 2.0 ** -24, -(2.0 ** -20),                     # the first 8: every width
                 88.0, -88.0, 104.0, -104.0, 17.0, -17.0, 23.0, -23.0, 24.0, -24.0, 10.0, -10.0, 2.0 ** -14, -(2.0 ** -15), 1.0, -1.0]


def _swiglu_ops(m, n, scale, pads=(0, 0, 0, 0, 0)):
    """gate, up, dact (inputs) as banded views at strides n + pads[0..2]; the gates' first row starts with SPECIAL_GATES."""
    g = _gen(3, m, n, int(-math.log2(scale)))
    gate, up = _outlier_rows(m, n, g).half(), _outlier_rows(m, n, g, zero_row=False).half()
    k = min(n, len(SPECIAL_GATES))
    gate[0, :k] = torch.tensor(SPECIAL_GATES[:k], dtype=F16, device=DEV)
    if m > 1:
        gate[-1, -k:] = torch.tensor(SPECIAL_GATES[:k], dtype=F16, device=DEV)
    dact = (torch.randn(m, n, generator=g, device=DEV) * scale).half()
    return [_Banded(m, n, n + p, init=x) for x, p in zip((gate, up, dact), pads[:3])]


def _run_swiglu_fwd(gb, ub, rows=None):
    _lib, lib = _L()
    first, count = rows or (0, gb.rows)
    ob = _Banded(count, gb.width)
    _lib.check(lib.qeft_swiglu_fwd(gb.ptr(first), ub.ptr(first), ob.ptr(), count, gb.width, gb.stride, ub.stride, _st()))
    torch.cuda.synchronize()
    assert gb.intact() and ub.intact() and ob.intact()
    return ob.v


def _run_swiglu_bwd(gb, ub, db, pads=(0, 0), rows=None):
    _lib, lib = _L()
    first, count = rows or (0, gb.rows)
    n = gb.width
    dgb, dub = _Banded(count, n, n + pads[0]), _Banded(count, n, n + pads[1])
    _lib.check(lib.qeft_swiglu_bwd(gb.ptr(first), ub.ptr(first), db.ptr(first), dgb.ptr(), dub.ptr(), count, n, gb.stride, ub.stride, db.stride,
                                   dgb.stride, dub.stride, _st()))
    torch.cuda.synchronize()
    for b in (gb, ub, db, dgb, dub):
        assert b.intact()
    return dgb.v, dub.v


@pytest.mark.parametrize("n", SWIGLU_N)
def test_swiglu_forward_has_the_bits_of_qeft_silu_mul(n):
    _lib, lib = _L()
    for m in ROWS:
        for pads in ((0, 0, 0), (8, 264, 0)):
            gb, ub, _ = _swiglu_ops(m, n, 2.0 ** -4, pads)
            out = _run_swiglu_fwd(gb, ub)
            gd, ud = gb.v.contiguous(), ub.v.contiguous()
            want = torch.full((m, n), float("nan"), dtype=F16, device=DEV)
            _lib.check(lib.qeft_silu_mul(gd.data_ptr(), ud.data_ptr(), want.data_ptr(), m * n, _st()))
            torch.cuda.synchronize()
            assert _same(out, want), (n, m, pads)
            ref = gb.v.double() * torch.sigmoid(gb.v.double()) * ub.v.double()           # silu(65504) * up may leave fp16's range
            assert torch.isfinite(out[ref.abs() < 65000.0]).all()
    print(f"[train_glue] swiglu_fwd n={n}: bit-equal to qeft_silu_mul, m in {ROWS}, dense and padded strides")


@pytest.mark.parametrize("n", SWIGLU_N)
def test_swiglu_backward_against_fp64(n):
    for m in ROWS:
        for scale in GRAD_SCALES:
            for pads in ((0, 0, 0, 0, 0), (8, 264, 16, 24, 8)):
                gb, ub, db = _swiglu_ops(m, n, scale, pads)
                dgate, dup = _run_swiglu_bwd(gb, ub, db, pads[3:])
                G, Uu, D = gb.v.double(), ub.v.double(), db.v.double()
                assert (D * Uu).abs().max().item() < 2.0 ** 15                     # the premise of the capped c (module docstring)
                sig, oms = torch.sigmoid(G), torch.sigmoid(-G)
                c = (2 * G.abs() + 18).clamp_max(64.0)
                A = D * Uu * sig
                case = f"n={n} m={m} grads 2^{int(math.log2(scale))} pad={int(pads[0] != 0)}"
                ref = A * (1 + G * oms)
                _check("swiglu_bwd dgate", case, dgate, ref, _ulp16(ref) + 1.001 * c * U * (A.abs() + (A * G * oms).abs()))
                ref = D * G * sig
                _check("swiglu_bwd dup", case, dup, ref, _ulp16(ref) + 1.001 * c * U * ref.abs())
                assert dgate.abs().max() > 0 and dup.abs().max() > 0


@pytest.mark.parametrize("n", [8, 2056, 28672])
def test_swiglu_rows_do_not_depend_on_the_launch(n):
    m = 65
    gb, ub, db = _swiglu_ops(m, n, 2.0 ** -4)
    out = _run_swiglu_fwd(gb, ub)
    dgate, dup = _run_swiglu_bwd(gb, ub, db)
    for first, count in ((0, 1), (32, 1), (64, 1), (60, 5)):
        rows = slice(first, first + count)
        assert _same(_run_swiglu_fwd(gb, ub, rows=(first, count)), out[rows]), (n, first)
        a, b = _run_swiglu_bwd(gb, ub, db, rows=(first, count))
        assert _same(a, dgate[rows]) and _same(b, dup[rows]), (n, first)
    g2, u2, d2 = (_Banded(m, n, n + p, init=x.v) for x, p in zip((gb, ub, db), (264, 8, 520)))               # other strides
    assert _same(_run_swiglu_fwd(g2, u2), out)
    a, b = _run_swiglu_bwd(g2, u2, d2, pads=(8, 16))
    assert _same(a, dgate) and _same(b, dup)
    print(f"[train_glue] swiglu n={n}: rows of an m = 65 launch equal the rows launched alone and at other strides")


# ================================================================================================ autograd
def test_glue_functions_autograd_equals_the_entries():
    """.grad through add_rmsnorm and swiglu equals the direct entry calls bit for bit; an input that needs no gradient gets None;
    a missing output gradient behaves as zero."""
    from qeft_amd import add_rmsnorm, swiglu
    m, H = 37, 2056
    h, add, gamma, dy, dres = _norm_ops(m, H, 2.0 ** -4)
    s_want, y_want = _run_norm_fwd(h, add, gamma)
    leaf = lambda x, need=True: x.detach().clone().requires_grad_(need)

    def norm(need_h, need_add, use_s, use_y, with_add=True):
        hh, aa = leaf(h, need_h), (leaf(add, need_add) if with_add else None)
        s, y = add_rmsnorm(hh, aa, gamma, EPS)
        outs, grads = [], []
        if use_s:
            outs.append(s), grads.append(dres)
        if use_y:
            outs.append(y), grads.append(dy)
        torch.autograd.backward(outs, grads)
        return s, y, hh.grad, None if aa is None else aa.grad

    both = _run_norm_bwd(s_want, gamma, dy, dres)
    s, y, gh, ga = norm(True, True, True, True)
    assert _same(s, s_want) and _same(y, y_want) and _same(gh, both) and _same(ga, both)
    s, y, gh, ga = norm(True, False, True, True)
    assert ga is None and _same(gh, both)
    s, y, gh, ga = norm(False, True, True, True)
    assert gh is None and _same(ga, both)
    s, y, gh, ga = norm(True, True, False, True)                       # no gradient for s: dres = 0
    assert _same(gh, _run_norm_bwd(s_want, gamma, dy, None)) and _same(ga, gh)
    s, y, gh, ga = norm(True, True, True, False)                       # no gradient for y
    assert _same(gh, dres) and _same(ga, dres)
    s, y, gh, ga = norm(True, False, True, True, with_add=False)       # add = None: s is h, its gradient joins inside the launch
    assert _same(s, h) and _same(y, _run_norm_fwd(h, None, gamma)[1]) and _same(gh, _run_norm_bwd(h, gamma, dy, dres))
    s, y = add_rmsnorm(h, None, gamma, EPS)
    assert s is h

    m, n = 37, 2056
    gb, ub, db = _swiglu_ops(m, n, 2.0 ** -4)
    out_want = _run_swiglu_fwd(gb, ub)
    dg_want, du_want = _run_swiglu_bwd(gb, ub, db)
    for need_g, need_u in ((True, True), (True, False), (False, True)):
        gg, uu = leaf(gb.v, need_g), leaf(ub.v, need_u)
        act = swiglu(gg, uu)
        act.backward(db.v)
        assert _same(act, out_want)
        assert (gg.grad is None) == (not need_g) and (uu.grad is None) == (not need_u)
        assert (not need_g or _same(gg.grad, dg_want)) and (not need_u or _same(uu.grad, du_want))
    act3 = swiglu(gb.v.view(1, m, n), ub.v.view(1, m, n).clone())
    assert act3.shape == (1, m, n) and _same(act3.view(m, n), out_want)
    with pytest.raises(ValueError):
        swiglu(gb.v[:, :12], ub.v[:, :12])
    with pytest.raises(ValueError):
        add_rmsnorm(h[:, :12], None, gamma[:12], EPS)
    print("[train_glue] glue functions: grads equal the entries bit for bit; None for inputs without grad; missing grads are zero")


# ================================================================================================ model
def _dense_pass(model, dense, leaves, tok2, targets, dt):
    """Section 4.14's dense pass: causal-LM mean NLL of tok2 [B, T] over dense weights; each linear's last n_out columns are
    leaves[li][name]; k / v repeated under grouped queries.  dt = F64: all of it in fp64.  dt = F16: fp16 tensors and plain torch
    ops, rounded where causal_lm_loss(glue="torch") rounds."""
    s = model.shape
    lo = dt == F16
    up = F32 if lo else F64
    B, T = tok2.shape
    rep = s.n_heads // s.n_kv_heads
    cos, sin = model.rope_cos[:T, None, :].to(up), model.rope_sin[:T, None, :].to(up)

    def rms(x, g):
        xf = x.to(up)
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + s.rms_eps) * g.to(up)).to(dt)

    def rope(x):
        a, b = x[..., :64].to(up), x[..., 64:].to(up)
        return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1).to(dt)

    def lin(x, li, name):
        leaf = leaves[li][name]
        W = torch.cat([dense[li][name][:, :-leaf.shape[1]].to(dt), leaf.to(dt)], dim=1)
        return x @ W.t()

    h = model.model.embed_tokens.weight[tok2.reshape(-1)].to(dt)
    for li, L in enumerate(model.model.layers):
        x = rms(h, L.input_layernorm.weight)
        q = rope(lin(x, li, "q_proj").view(B, T, s.n_heads, 128))
        k = rope(lin(x, li, "k_proj").view(B, T, s.n_kv_heads, 128))
        v = lin(x, li, "v_proj").view(B, T, s.n_kv_heads, 128)
        if rep != 1:
            k, v = k.repeat_interleave(rep, 2), v.repeat_interleave(rep, 2)
        a = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True)
        a = a.transpose(1, 2).reshape(B * T, s.hidden)[:, L.self_attn.o_proj.reorder_ids]
        h = h + lin(a, li, "o_proj")
        x = rms(h, L.post_attention_layernorm.weight)
        act = (torch.nn.functional.silu(lin(x, li, "gate_proj").to(up)) * lin(x, li, "up_proj").to(up)).to(dt)
        h = h + lin(act, li, "down_proj")
    hn = rms(h, model.model.norm.weight)
    logits = (hn @ model.lm_head.weight.to(dt).t()).to(up)
    return torch.nn.functional.cross_entropy(logits, targets.long(), ignore_index=IGNORE, reduction="mean")


LOSS_SCALE = 1024.0
T_DOC = 200
_MODELS = {}


def _trainable(which):
    """(model, tokens, labels, params, reference(batch)) of the GQA 4 / 2 model or the tiny model, made once."""
    if which in _MODELS:
        return _MODELS[which]
    from qeft_amd import finetune
    from qeft_amd.llama import LlamaShape, QuantLlama, layer_linears, tiny_shape
    shape = LlamaShape(512, 512, 2, 4, 2, 512, max_seq=256) if which == "gqa" else tiny_shape(max_seq=256)
    model = QuantLlama(shape, DEV, seed=6)
    g = torch.Generator().manual_seed(4)
    tokens = torch.randint(0, shape.vocab, (T_DOC,), generator=g).to(DEV)
    labels = tokens.clone()
    labels[torch.tensor([0, 1, 2, 10, 11, 30, 99, 100, 150, 199])] = IGNORE
    dense = model.dense_weights()                                       # before begin(): oweight is still the fp16 buffer
    ow = [{nm: ql.oweight.detach().clone() for nm, ql in layer_linears(L)} for L in model.model.layers]
    params = finetune.begin(model)
    refs = {}

    def reference(batch):
        if batch not in refs:
            tok2 = tokens.view(batch, -1)
            targets = finetune.shift_labels(tok2, labels.view(batch, -1)).reshape(-1)
            out = []
            for dt in (F64, F16):
                leaves = [{nm: v.to(F64 if dt == F64 else F32).requires_grad_(True) for nm, v in d.items()} for d in ow]
                loss = _dense_pass(model, dense, leaves, tok2, targets, dt)
                (loss * (LOSS_SCALE if dt == F16 else 1.0)).backward()
                grads = [{nm: (v.grad.to(F64) / (LOSS_SCALE if dt == F16 else 1.0)) for nm, v in d.items()} for d in leaves]
                out += [loss.item(), grads]
            refs[batch] = tuple(out)
        return refs[batch]
    _MODELS[which] = (model, tokens, labels, params, reference)
    return _MODELS[which]


@pytest.mark.parametrize("attn", ["sdpa", "own"])
@pytest.mark.parametrize("checkpoint", [True, False], ids=["checkpoint", "plain"])
@pytest.mark.parametrize("batch", [1, 2], ids=["T200", "B2xT100"])
@pytest.mark.parametrize("which", ["gqa", "tiny"])
def test_causal_lm_loss_with_fused_glue(which, batch, checkpoint, attn):
    """Section 4.14's criterion for glue="fused": the loss error from an fp64 dense pass is at most 2 x that of the fp16 plain-torch
    dense pass + 2^-14, the relative L2 error of every d(oweight) at most 2 x that pass's own; and glue="torch" in the same
    process still gives, bit for bit, the loss it gave before the fused call."""
    from qeft_amd import causal_lm_loss
    from qeft_amd.llama import layer_linears
    model, tokens, labels, params, reference = _trainable(which)
    loss64, g64, loss16, g16 = reference(batch)
    tok = tokens.view(batch, -1) if batch > 1 else tokens
    lab = labels.view(batch, -1) if batch > 1 else labels
    with torch.no_grad():
        before = causal_lm_loss(model, tok, lab, checkpoint=False, attn=attn, glue="torch").item()
    for p in params:
        p.grad = None
    loss = causal_lm_loss(model, tok, lab, checkpoint=checkpoint, attn=attn, glue="fused")
    assert loss.dtype == F32 and loss.dim() == 0
    (loss * LOSS_SCALE).backward()
    e_own, e_16 = abs(loss.item() - loss64), abs(loss16 - loss64)
    worst, lines = 0.0, []
    for li, L in enumerate(model.model.layers):
        for nm, ql in layer_linears(L):
            assert ql.oweight.grad is not None and ql.oweight.grad.dtype == F32, (li, nm)
            assert torch.isfinite(ql.oweight.grad).all()
            ref = g64[li][nm]
            own = ((ql.oweight.grad.to(F64) / LOSS_SCALE - ref).norm() / ref.norm()).item()
            t16 = ((g16[li][nm] - ref).norm() / ref.norm()).item()
            worst = max(worst, own / t16)
            lines.append(f"{li}.{nm} {own:.2e}/{t16:.2e}")
    kind = f"{which} {'checkpoint' if checkpoint else 'plain'} batch {batch} attn {attn}"
    print(f"[train_glue] model {kind}: loss {loss.item():.6f} fp64 {loss64:.6f}  |d| fused {e_own:.3e}  fp16 torch {e_16:.3e}")
    print(f"[train_glue] model {kind}: rel L2 error of d(oweight), fused / fp16 torch: " + "  ".join(lines))
    print(f"[train_glue] model {kind}: largest ratio fused / fp16 torch = {worst:.3f} (allowed 2)")
    assert e_own <= 2 * e_16 + 2.0 ** -14, f"{kind}: loss error {e_own:.3e} > 2 x {e_16:.3e} + 2^-14"
    assert worst <= 2.0, f"{kind}: a d(oweight) is {worst:.2f} x the fp16 torch pass's error from fp64"
    with torch.no_grad():
        after = causal_lm_loss(model, tok, lab, checkpoint=False, attn=attn, glue="torch").item()
    assert after == before, (before, after)


ENTRIES = ("qeft_add_rmsnorm_fwd", "qeft_add_rmsnorm_bwd", "qeft_swiglu_fwd", "qeft_swiglu_bwd")


def test_fused_glue_launches_are_the_ones_that_run(monkeypatch):
    """causal_lm_loss(glue="fused") over n layers reaches each entry the documented number of times, plain and checkpointed
    (the recomputation reruns the forward entries), with either head; glue="torch" reaches none of them.

                                plain    checkpointed
        qeft_add_rmsnorm_fwd    2n + 1   4n + 1
        qeft_add_rmsnorm_bwd    2n + 1   2n + 1      where the embedding rows need a gradient; 2n with the embedding frozen
        qeft_swiglu_fwd         n        2n
        qeft_swiglu_bwd         n        n

    2n + 1 norms have a backward to run only if the input of layer 0's first norm needs a gradient.  finetune.begin() trains the
    oweight slices alone, the embedding rows need none, and autograd then never calls that norm's backward (on the torch route
    neither): 2n launches, not one of them spared by a torch op.  Both settings are asserted: the table as it stands with the
    embedding's requires_grad switched on for the call, and 2n as the model is trained."""
    from qeft_amd import _lib, causal_lm_loss
    model, tokens, labels, params, _ = _trainable("gqa")
    lib = _lib.lib()
    calls = []
    for name in ENTRIES:
        orig = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda o, nm: lambda *a: (calls.append(nm), o(*a))[1])(orig, name))
    n = model.shape.n_layers
    want = {False: (2 * n + 1, 2 * n + 1, n, n), True: (4 * n + 1, 2 * n + 1, 2 * n, n)}
    embed = model.model.embed_tokens.weight
    assert not embed.requires_grad
    for embed_grad in (True, False):
        for ckpt in (False, True):
            for attn, head in (("own", "fused"), ("sdpa", "torch")):
                calls.clear()
                embed.requires_grad_(embed_grad)
                try:
                    causal_lm_loss(model, tokens, labels, checkpoint=ckpt, attn=attn, head=head, glue="fused").backward()
                finally:
                    embed.requires_grad_(False)
                    embed.grad = None
                got = tuple(calls.count(nm) for nm in ENTRIES)
                exp = want[ckpt] if embed_grad else (want[ckpt][0], 2 * n) + want[ckpt][2:]
                assert got == exp, (embed_grad, ckpt, attn, head, dict(zip(ENTRIES, got)))
    calls.clear()
    causal_lm_loss(model, tokens, labels, glue="torch").backward()
    causal_lm_loss(model, tokens, labels, checkpoint=False).backward()
    assert calls == []
