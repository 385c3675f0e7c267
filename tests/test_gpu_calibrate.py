"""GPU tests of the calibrator (qeft_amd/calibrate.py, csrc/calib.hip).

qeft_hessian_accum against fp64 of the same fp16 rows.  The products of two fp16 values are exact in fp32, so only the summation
and the epilogue round.  With u = 2^-24, A = sum_t |x_ti x_tj| over a call's rows, n the rows rounded up to the staged tile of 64
(the padding adds exact zeros) and gamma(n) = n u / (1 - n u) -- the bound of ANY order of n fp32 additions, so it covers the MFMA's
order inside a k-step as well as the ascending order across them:
    call 1 (beta = 0):  |H1 - a1 S1| <= a1 A1 (gamma(n1) + 3u)          alpha's rounding, the product's, second order in the third u
    call 2:             |H2 - (b H1x + a2 S2)| <= b e1 + 3u b |H1x| + a2 A2 (gamma(n2) + 3u) + u |H2|
                        (beta's rounding, its product's and one u of second order; the final addition on |H2| <= b |H1x| + a2 A2)
    with |H1x| <= a1 A1 and b a1 = a2:   |H2 - ref| <= a2 (1 + 2^-10) [A1 (gamma(n1) + 7u) + A2 (gamma(n2) + 4u)]
No element is excluded and nothing is fitted; the test prints the largest observed ratio to the bound.  The rows hold no fp16
subnormals (the contract's "exact products" does not say what the matrix unit does with them, and the test does not ask).

qeft_gptq_block bit for bit against the same lines in torch on the CPU in fp32 (tests/calib_ref.block_lines).

gptq_reorder against the fp64 restatement (tests/calib_ref.gptq_reorder, tied to the reference by tests/test_calibrate_cpu.py):
bit parity cannot hold there (the trailing GEMM sums in another order and a near-tie then rounds the other way), hence the four
properties of test_gptq_reorder.
"""
import math
import os
import types

import numpy as np
import pytest
import torch

import calib_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def bits(t):
    return t.contiguous().view(torch.int32)


def fp16_rows(g, *shape):
    """Calibration-like rows: unit normals, every 5th channel x 8, rounded to fp16, no subnormals."""
    x = torch.randn(*shape, generator=g)
    x[..., ::5] *= 8
    x = x.half()
    x[(x != 0) & (x.abs() < 2.0 ** -14)] = 0
    return x


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "calib_case0.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


# ---------------------------------------------------------------------------------------------------- the Hessian
@pytest.mark.parametrize("t,k", [(1, 64), (65, 192), (200, 256)])
def test_hessian_accum(t, k):
    from qeft_amd import _lib
    from qeft_amd.calibrate import HessianAccumulator
    g = torch.Generator().manual_seed(100 + t)
    x1, x2 = fp16_rows(g, t, k), fp16_rows(g, 3, t, k)                    # B = 1 as [T, K], then B = 3

    def run():
        acc = HessianAccumulator(k, DEV)
        acc.H.fill_(float("nan"))                                         # beta == 0 must not read H
        acc.add_batch(x1.to(DEV))
        assert _lib.last_variant() == "hessian_accum_128x128"
        h1 = acc.H.clone()
        acc.add_batch(x2.to(DEV))
        assert acc.nsamples == 4
        return h1.cpu(), acc.H.cpu()

    h1, h2 = run()
    X1, X2 = x1.double(), x2.reshape(-1, k).double()
    S1, S2, A1, A2 = X1.T @ X1, X2.T @ X2, X1.abs().T @ X1.abs(), X2.abs().T @ X2.abs()
    pad = lambda n: 64 * math.ceil(n / 64)
    a1, a2, u = 2.0, 2.0 / 4, R.U
    b1 = a1 * (1 + 2.0 ** -10) * A1 * (R.gamma(pad(t)) + 3 * u)
    b2 = a2 * (1 + 2.0 ** -10) * (A1 * (R.gamma(pad(t)) + 7 * u) + A2 * (R.gamma(pad(3 * t)) + 4 * u))
    e1, e2 = (h1.double() - a1 * S1).abs(), (h2.double() - a2 * (S1 + S2)).abs()
    tiny = 2.0 ** -200                                                    # (a zero bound wants a zero error: asserted below)
    print(f"T = {t}, K = {k}: largest error / bound: call 1 {(e1 / b1.clamp_min(tiny)).max().item():.4f}, "
          f"call 2 {(e2 / b2.clamp_min(tiny)).max().item():.4f}")
    assert (e1 <= b1).all() and (e2 <= b2).all()
    assert torch.equal(bits(h1), bits(h1.T)) and torch.equal(bits(h2), bits(h2.T))
    g1, g2 = run()                                                        # the same calls again: the same bits
    assert torch.equal(bits(g1), bits(h1)) and torch.equal(bits(g2), bits(h2))


# ---------------------------------------------------------------------------------------------------- the block kernel
def block_case(n, count, maxq):
    """Strided operands inside larger W / Hinv.  Row 1 all zero; column 1 all zero; row 2 with a scale 4096 times too small and a
    zero point of 0, so that every value of it clamps (its one zero sits on code 0); the lower triangle of Hinv1 holds garbage.
    Returns the operands and the CPU's fp32 results."""
    g = torch.Generator().manual_seed(1000 * n + 10 * count + maxq)
    c0, ld_w = 8, count + 40
    W = torch.randn(n, ld_w, generator=g) * 0.02
    W[2] = 0.01 + W[2].abs()
    W[1, c0:c0 + count] = 0
    W[:, c0 + 1] = 0
    m = count + 5                                                         # a real factor: SPD, inverse, upper Cholesky
    A = torch.randn(m, 2 * m, generator=g, dtype=torch.float64)
    hinv = torch.linalg.cholesky(torch.linalg.inv(A @ A.T / (2 * m) + 0.1 * torch.eye(m, dtype=torch.float64)), upper=True).float()
    r0, k0, ld_h = 2, 3, m + 7
    Hbig = torch.full((m + 3, ld_h), 777.0)
    Hbig[r0:r0 + m, k0:k0 + m] = torch.triu(hinv) + torch.tril(torch.full((m, m), 777.0), -1)
    W1 = W[:, c0:c0 + count]
    h_off = (r0 + 1) * ld_h + k0 + 1                                      # a diagonal block of the factor, one row and column in
    Hinv1 = Hbig[r0 + 1:r0 + 1 + count, k0 + 1:k0 + 1 + count]
    scale, zero = R.minmax(W1, maxq)
    scale, zero = scale[:, 0].contiguous(), zero[:, 0].contiguous()
    scale[2], zero[2] = scale[2] / 4096, 0
    Qc, Ec, Wc = R.block_lines(W1, Hinv1, scale, zero, float(maxq))
    codes = torch.round(Qc[2] / scale[2] + zero[2])
    assert ((codes == 0) | (codes == maxq)).all() and (codes == maxq).any()                           # the cases are what they claim
    assert (Qc[1] == 0).all() and (Ec[1] == 0).all()
    return W, c0, ld_w, Hbig, h_off, ld_h, scale, zero, Qc, Ec, Wc


@pytest.mark.parametrize("maxq", [7, 15])
@pytest.mark.parametrize("count", [2, 64, 128])
@pytest.mark.parametrize("n", [8, 72, 260])
def test_gptq_block_bit_parity(n, count, maxq):
    """Q1, Err1 and the updated W1 are the CPU's bits (block_case); nothing outside the block's columns moves."""
    from qeft_amd import _lib
    W, c0, ld_w, Hbig, h_off, ld_h, scale, zero, Qc, Ec, Wc = block_case(n, count, maxq)
    Wg, Hg, sg, zg = W.to(DEV), Hbig.to(DEV), scale.to(DEV), zero.to(DEV)
    q1 = torch.full((n, count), float("nan"), device=DEV)
    e1 = torch.full((n, count), float("nan"), device=DEV)
    _lib.check(_lib.lib().qeft_gptq_block(Wg.data_ptr() + 4 * c0, ld_w, Hg.data_ptr() + 4 * h_off, ld_h,
                                          sg.data_ptr(), zg.data_ptr(), q1.data_ptr(), e1.data_ptr(), n, count, maxq,
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _lib.last_variant() == "gptq_block_row_per_lane"
    Wn = Wg.cpu()
    assert torch.equal(bits(q1.cpu()), bits(Qc))
    assert torch.equal(bits(e1.cpu()), bits(Ec))
    assert torch.equal(bits(Wn[:, c0:c0 + count]), bits(Wc))
    assert torch.equal(bits(Wn[:, :c0]), bits(W[:, :c0])) and torch.equal(bits(Wn[:, c0 + count:]), bits(W[:, c0 + count:]))
    assert torch.equal(Hg.cpu(), Hbig)


# ---------------------------------------------------------------------------------------------------- the whole reorder
@pytest.mark.parametrize("seed,shape", R.CASES)
def test_gptq_reorder(seed, shape, golden):
    from qeft_amd.calibrate import HessianAccumulator, frob_norm_error, gptq_reorder, select_outliers
    W, X, hot = R.make_case(seed, **shape)
    N, K, r, maxq = W.shape[0], W.shape[1], len(hot), 15
    if seed == 0:                                                         # the golden layer: the reference's own H and Frobenius term
        W, hot = golden["W"], golden["hot"]
        H, frob = golden["H"].to(DEV), golden["frob"].to(DEV)
    else:
        acc = HessianAccumulator(K, DEV)
        for j in range(X.shape[0]):
            acc.add_batch(X[j].to(DEV))
        H, frob = acc.H, frob_norm_error(W.to(DEV), 4, 128, "minmax")
    out_ids, ids = select_outliers(H, r, frob_norm=frob)
    assert out_ids.dtype == torch.int32 and torch.equal(out_ids.cpu().long(), hot)            # (4) exactly the scaled channels
    if seed == 0:
        assert torch.equal(out_ids.cpu(), golden["out_ids"])
    idc, Hc = ids.cpu(), H.cpu()
    Wp, Hp = W.float()[:, idc], Hc[idc][:, idc]
    Q64, _, _, h64 = R.gptq_reorder(Wp, Hp, K - r, torch.float64)
    l64, l_rtn = R.proxy_loss(Wp, Q64, Hp), R.proxy_loss(Wp, R.rtn(Wp, K - r), Hp)
    for hinv in (h64, None):                                              # the oracle's factor, then the GPU's own factorisation
        res = gptq_reorder(W.to(DEV), H, ids, r, hinv=hinv)
        w, s, z = res.weight.cpu(), res.scale_group.cpu(), res.zero_group.cpu()
        # (1) the grid, the shapes, the padding
        ng, ngl = K // 128, -(-(K - r) // 128)
        assert w.shape == (N, K) and w.dtype == torch.float16 and s.shape == (N, ng) and z.shape == (N, ng)
        assert s.dtype == torch.float32 and z.dtype == torch.float32 and (s > 0).all()
        assert torch.equal(z, z.round()) and z.min() >= 0 and z.max() <= maxq
        for j in range(ngl, ng):
            assert torch.equal(s[:, j], s[:, ngl - 1]) and torch.equal(z[:, j], z[:, ngl - 1])
        sf = torch.repeat_interleave(s, 128, 1)[:, :K - r]
        zf = torch.repeat_interleave(z, 128, 1)[:, :K - r]
        codes = torch.round(w[:, :K - r].float() / sf + zf)
        assert codes.min() >= 0 and codes.max() <= maxq
        assert torch.equal((sf * (codes - zf)).half(), w[:, :K - r])
        assert torch.isfinite(w).all() and torch.equal(res.out_ids.cpu(), out_ids.cpu()) and torch.equal(res.ids.cpu(), idc)
        # (2), (3)
        print(f"seed {seed}, hinv {'fp64' if hinv is not None else 'own'}: proxy loss {res.proxy_loss:.9g}, fp64 restatement "
              f"{l64:.9g} (relative {(res.proxy_loss - l64) / l64:+.3g}, margin {R.REL_MARGIN:.3g}), / RTN {res.proxy_loss / l_rtn:.3f}")
        assert res.proxy_loss <= (1 + R.REL_MARGIN) * l64
        assert res.proxy_loss < 0.6 * l_rtn


def grid_properties(res, N, K, r, maxq):
    """(1): every value on the grid of the returned (scale, zero), codes in 0..maxq, integral zeros, the reference's shapes and padding."""
    w, s, z = res.weight.cpu(), res.scale_group.cpu(), res.zero_group.cpu()
    ng, ngl = K // 128, -(-(K - r) // 128)
    assert w.shape == (N, K) and w.dtype == torch.float16 and s.shape == (N, ng) and z.shape == (N, ng)
    assert s.dtype == torch.float32 and z.dtype == torch.float32 and (s > 0).all()
    assert torch.equal(z, z.round()) and z.min() >= 0 and z.max() <= maxq
    for j in range(ngl, ng):
        assert torch.equal(s[:, j], s[:, ngl - 1]) and torch.equal(z[:, j], z[:, ngl - 1])
    sf = torch.repeat_interleave(s, 128, 1)[:, :K - r]
    zf = torch.repeat_interleave(z, 128, 1)[:, :K - r]
    codes = torch.round(w[:, :K - r].float() / sf + zf)
    assert codes.min() >= 0 and codes.max() <= maxq
    assert torch.equal((sf * (codes - zf)).half(), w[:, :K - r]) and torch.isfinite(w).all()


@pytest.mark.parametrize("seed,shape,nbits,tuning", [(0, {}, 3, "minmax"), (11, dict(N=256, K=512, r=128, S=4, T=160), 3, "minmax"),
                                                     (0, {}, 4, "mse"), (0, {}, 3, "mse")])
def test_gptq_reorder_3_bits_and_mse(seed, shape, nbits, tuning):
    """maxq = 7 and the restated MSE search through the whole loop, with the GPU's own factorisation.  (1) and (3) as in
    test_gptq_reorder, RTN being min-max rounding at the same bits (on the CPU the fp64 restatement gives 0.39 - 0.41 x RTN at 3
    bits with min-max and 0.33 - 0.39 with the search); (2) against the fp64 restatement where the parameters are min-max (the
    search's discrete choices may fall otherwise on another device, so its oracle is tests/golden/calib_mse0.npz on the CPU)."""
    from qeft_amd.calibrate import HessianAccumulator, frob_norm_error, gptq_reorder, select_outliers
    W, X, hot = R.make_case(seed, **shape)
    N, K, r, maxq = W.shape[0], W.shape[1], len(hot), 2 ** nbits - 1
    acc = HessianAccumulator(K, DEV)
    acc.add_batch(X.to(DEV))
    H = acc.H
    out_ids, ids = select_outliers(H, r, frob_norm=frob_norm_error(W.to(DEV), nbits, 128, tuning))
    assert torch.equal(out_ids.cpu().long(), hot)
    idc, Hc = ids.cpu(), H.cpu()
    Wp, Hp = W.float()[:, idc], Hc[idc][:, idc]
    res = gptq_reorder(W.to(DEV), H, ids, r, bits=nbits, tuning=tuning)
    grid_properties(res, N, K, r, maxq)
    l_rtn = R.proxy_loss(Wp, R.rtn(Wp, K - r, bits=nbits), Hp)
    print(f"seed {seed}, {nbits} bits, {tuning}: proxy loss {res.proxy_loss:.9g}, / RTN {res.proxy_loss / l_rtn:.3f}")
    assert res.proxy_loss < 0.6 * l_rtn
    if tuning == "minmax":
        l64 = R.proxy_loss(Wp, R.gptq_reorder(Wp, Hp, K - r, torch.float64, bits=nbits)[0], Hp)
        print(f"    fp64 restatement {l64:.9g} (relative {(res.proxy_loss - l64) / l64:+.3g}, margin {R.REL_MARGIN:.3g})")
        assert res.proxy_loss <= (1 + R.REL_MARGIN) * l64


# ---------------------------------------------------------------------------------------------------- through the kernels that ship
class Holder(torch.nn.Module):
    def __init__(self, layer):
        super().__init__()
        self.o_proj = layer


LAYERS = {   # case -> (layer, n_out, bits, name)
    "golden_o_proj": ("golden", 64, 4, "layers.0.self_attn.o_proj"),
    "down_proj_256x512": ("256x512", 128, 4, "layers.0.mlp.down_proj"),
    "w3_down_proj_256x512": ("256x512", 128, 3, "layers.0.mlp.down_proj"),
    "no_outliers_256x512": ("256x512", 0, 4, "layers.0.mlp.up_proj"),
}


@pytest.mark.parametrize("case", list(LAYERS))
def test_calibrate_linear_through_the_packed_kernels(case, golden, tmp_path):
    """The issue's two layers, plus the 3-bit layout and n_out = 0 (plain GPTQ) on the second.  On the CPU, with the fp64
    restatement's weights, the calibrated layer's error on these rows is 0.59 - 0.75 x the min-max layer's for the two added cases
    at m = 1 as at m = 16, so the comparison is asserted for both m everywhere."""
    from qeft_amd import checkpoint
    from qeft_amd.calibrate import HessianAccumulator, calibrate_linear
    from qeft_amd.qlinear import QuantLinear, unpack_intweight
    layer, r, nbits, name = LAYERS[case]
    if layer == "golden":
        W, X, H = golden["W"], golden["X"], golden["H"].to(DEV)
    else:
        W, X, _ = R.make_case(11, N=256, K=512, r=128, S=4, T=160)
        acc = HessianAccumulator(512, DEV)
        acc.add_batch(X.to(DEV))
        H = acc.H
    N, K = W.shape
    lin = torch.nn.Linear(K, N, bias=False).half().to(DEV)
    lin.weight.data = W.to(DEV)
    module, info = calibrate_linear(lin, H, r, name, bits=nbits)
    ids = info.ids.cpu()
    gathers = "o_proj" in name
    assert isinstance(module, QuantLinear) and module.outlierfeatures == r and (hasattr(module, "reorder_ids") == gathers)
    assert module.bits == nbits and info.bits == nbits and info.n_out == r
    sd = module.state_dict()
    want = {"qweight": torch.int16 if nbits == 4 else torch.int32, "scales": torch.float16, "scaled_zeros": torch.float16}
    if r > 0:
        want.update(oweight=torch.float16, oweight_interleaved=torch.float16, outlieridx=torch.int32)
        assert sd["oweight"].shape == (N, r) and torch.equal(sd["outlieridx"].cpu(), info.out_ids.cpu())
    else:
        assert torch.equal(ids, torch.arange(K)) and info.out_ids.numel() == 0
    if gathers:
        want["reorder_ids"] = torch.int64
        assert torch.equal(sd["reorder_ids"].cpu(), ids)
    assert {k: v.dtype for k, v in sd.items()} == want
    assert sd["qweight"].shape == ((N // 4, K) if nbits == 4 else (N // 16, (K - r) // 128 * 192)) and sd["scales"].shape == (K // 128, N)
    if nbits == 4:                                                        # the packed codes are the calibrated ones
        sf = torch.repeat_interleave(info.scale_group.cpu(), 128, 1)[:, :K - r]
        zf = torch.repeat_interleave(info.zero_group.cpu(), 128, 1)[:, :K - r]
        codes = torch.round(info.weight.cpu()[:, :K - r].float() / sf + zf)
        assert torch.equal(unpack_intweight(sd["qweight"].cpu())[:, :K - r].float(), codes)

    Qu = info.weight.cpu().double()[:, torch.argsort(ids)]                # the returned weight, un-permuted
    rows = X.reshape(-1, K)
    feed = (lambda x: x) if gathers or r == 0 else (lambda x: x[..., ids.to(x.device)].contiguous())
    # the same layer packed with plain min-max on the same outlier columns
    Qr, sr, zr = R.rtn(W.float()[:, ids], K - r, bits=nbits, return_params=True)
    plain = QuantLinear(nbits, K, N, False, torch.float16, r, 128, True, name)
    plain.pack(types.SimpleNamespace(weight=types.SimpleNamespace(data=Qr.half()), bias=None), scales=sr, zeros=zr,
               outlieridx=info.out_ids.cpu())
    plain = plain.to(DEV)
    plain.set_kernel()
    for m in (1, 16):
        x = rows[40:40 + m].contiguous()
        y = module(feed(x.to(DEV))).cpu().double()
        yq, y0 = x.double() @ Qu.T, x.double() @ W.double().T
        err = (y - yq).abs().max().item() / yq.abs().max().item()
        e_cal = (y - y0).norm().item()
        e_rtn = (plain(feed(x.to(DEV))).cpu().double() - y0).norm().item()
        print(f"{case}, m = {m}: module vs x Q^T {err:.3g}; error against the dense layer: calibrated {e_cal:.4g}, min-max {e_rtn:.4g}")
        assert y.shape == (m, N) and e_cal < e_rtn
        if r > 0:     # the standing bound of a packed linear WITH its fp16 outlier slice; without one the fp16 rounding of the scales
            assert err < 1e-3      # is no longer small against the output, and the codes above are compared exactly instead
    if gathers:                                                           # saves and loads like any other layer
        path = str(tmp_path / "calibrated.pth")
        checkpoint.save_packed(Holder(module), {"o_proj": info}, path)
        loaded = checkpoint.load_packed(Holder(torch.nn.Linear(K, N, bias=False).half()), path, device=DEV)
        x = rows[:16].to(DEV)
        assert torch.equal(loaded.o_proj(x), module(x))
