"""Tests of the row-owned GPTQ loop (qeft_gptq_rows, csrc/calib_rows.hip; gptq_reorder / calibrate_linear(loop="rows"); DESIGN.md
section 4.23).  Layers from calib_ref.make_case, the factor from calib_ref.factor in fp64 rounded to fp32.

The defining identity, in fp64, for every element:  D = W0 - [Q_live | Q_out] - Err . triu(U)[:n_nonout, :]  satisfies
|D| <= gamma(n_nonout + 8) (|W0| + |Err| . |U|): at most n_nonout - 1 rounded feedback products and as many fp32 partial sums
(any order), one subtraction from W0, the two roundings of e = (w - q) / d and the one of e d -- derived, not measured.
The last test is the CPU's: refusals only -- no call hands the launching entry a complete set of valid arguments."""
import functools
import os

import numpy as np
import pytest
import torch

import calib_ref as R

gpu = pytest.mark.gpu
DEV = "cuda:0"
# (N, K, r, bits): N < 16, blocks 128 + 64 | ragged last workgroup | no outliers | outlier start 8-byte aligned | 3 bits | depth 254
IDENTITY = [(8, 256, 64, 4), (72, 384, 128, 4), (16, 640, 0, 4), (24, 256, 2, 4), (256, 512, 128, 3), (24, 384, 130, 4)]


@functools.lru_cache(maxsize=None)
def layer(N, K, r):
    """CPU: (W, X, H fp64, ids, W0 = W in ids order fp32, U = the fp64 factor rounded to fp32)."""
    W, X, hot = R.make_case(100 + N + K + r, N=N, K=K, r=r, T=192)
    ids = R.dense_ids(hot, K)
    H = R.hessian64(X)
    U = R.factor(H[ids][:, ids], torch.float64)[0].float()
    return W, X, H, ids, W.float()[:, ids].contiguous(), U


def _placed(t, rows, ld, r0, c0):
    """The CPU image of t as a view at [r0, c0] of a NaN-filled [rows, ld] buffer (ld None: t itself), and the view's offset."""
    if ld is None:
        return t.contiguous(), 0
    big = torch.full((rows, ld), float("nan"))
    big[r0:r0 + t.shape[0], c0:c0 + t.shape[1]] = t
    return big, r0 * ld + c0


def run_rows(W0, U, nn, maxq, ld_w=None, ld_h=None, num=None):
    """One launch of qeft_gptq_rows (num None) or qeft_gptq_rows_mse (num ranges) through the C entry.  ld_w: W0 is a view at
    [1, 4] of a NaN-filled [n + 2, ld_w] buffer; ld_h: U is a view at [2, 8] of a NaN-filled [k + 3, ld_h] buffer with NaN written
    below the diagonal inside the view (both offsets are multiples of 4 floats).  The inputs, padding included, must come back
    with the bits they went in with; the outputs keep their dense strides and carry one NaN guard row that must stay NaN."""
    from qeft_amd import _lib
    n, k = W0.shape
    nan = float("nan")
    Uin = U if ld_h is None else torch.where(torch.ones_like(U, dtype=torch.bool).tril(-1), torch.full_like(U, nan), U)
    (wi, wo), (ui, uo) = _placed(W0, n + 2, ld_w, 1, 4), _placed(Uin, k + 3, ld_h, 2, 8)
    w, u = wi.to(DEV), ui.to(DEV)
    q, err, s, z = (torch.full((n + 1, cols), nan, device=DEV) for cols in (k, nn, k // 128, k // 128))
    args = (w.data_ptr() + 4 * wo, ld_w or k, u.data_ptr() + 4 * uo, ld_h or k, q.data_ptr(), err.data_ptr(), s.data_ptr(), z.data_ptr(),
            n, k, nn, maxq, 128)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().qeft_gptq_rows(*args, st) if num is None else _lib.lib().qeft_gptq_rows_mse(*args, num, st))
    torch.cuda.synchronize()
    assert _lib.last_variant() == ("gptq_rows_16" if num is None else f"gptq_rows_mse_w{3 + (maxq == 15)}")
    assert torch.equal(w.cpu().view(torch.int32), wi.view(torch.int32)) and torch.equal(u.cpu().view(torch.int32), ui.view(torch.int32))
    out = [t.cpu() for t in (q, err, s, z)]
    assert all(torch.isnan(t[n]).all() for t in out)
    return tuple(t[:n].contiguous() for t in out)


def assert_identity(W0, q, err, U, nn, what):
    W0, q, err = W0.double(), q.double(), err.double()
    T = torch.triu(U.double())[:nn]
    D, B = (W0 - q - err @ T).abs(), R.gamma(nn + 8) * (W0.abs() + err.abs() @ T.abs())
    print(f"{what}: largest |D| / bound {(D / B.clamp_min(2.0 ** -200)).max().item():.4f}")
    assert (D <= B).all()


@gpu
@pytest.mark.parametrize("N,K,r,bits", IDENTITY)
def test_defining_identity(N, K, r, bits):
    _, _, _, _, W0, U = layer(N, K, r)
    nn, maxq, ng, ngl = K - r, 2 ** bits - 1, K // 128, -(-(K - r) // 128)
    q, err, s, z = run_rows(W0, U, nn, maxq)
    assert q.shape == (N, K) and err.shape == (N, nn) and s.shape == (N, ng) and z.shape == (N, ng)
    assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in (q, err, s, z)) and (s > 0).all()
    assert torch.equal(z, z.round()) and z.min() >= 0 and z.max() <= maxq
    for j in range(ngl, ng):
        assert torch.equal(s[:, j], s[:, ngl - 1]) and torch.equal(z[:, j], z[:, ngl - 1])
    sf, zf = (torch.repeat_interleave(t, 128, 1)[:, :nn] for t in (s, z))
    codes = torch.round(q[:, :nn] / sf + zf)
    assert codes.min() >= 0 and codes.max() <= maxq and torch.equal(sf * (codes - zf), q[:, :nn])
    assert_identity(W0, q, err, U, nn, f"{N} x {K}, r = {r}, {bits} bits")


@gpu
@pytest.mark.parametrize("N,K,r", [(40, 256, 128), (40, 256, 192)])
def test_one_block_has_the_bits_of_the_block_route(N, K, r):
    """No left-looking term exists for the only live block: the same w at its start, hence the same bits."""
    from qeft_amd.calibrate import gptq_reorder
    W, _, H, ids, W0, U = layer(N, K, r)
    a, b = (gptq_reorder(W.to(DEV), H.float().to(DEV), ids.to(DEV), r, hinv=U, loop=loop) for loop in ("rows", "blocks"))
    assert torch.equal(a.weight[:, :K - r], b.weight[:, :K - r])
    assert torch.equal(a.scale_group, b.scale_group) and torch.equal(a.zero_group, b.zero_group)
    q, err, s, z = run_rows(W0, U, K - r, 15)
    assert torch.equal(q.half(), a.weight.cpu()) and torch.equal(s, a.scale_group.cpu()) and torch.equal(z, a.zero_group.cpu())
    assert_identity(W0, q, err, U, K - r, f"{N} x {K}, r = {r}")


@gpu
def test_rows_are_independent_and_reruns_identical():
    _, _, _, _, W0, U = layer(72, 384, 128)
    full, again, part = run_rows(W0, U, 256, 15), run_rows(W0, U, 256, 15), run_rows(W0[16:32], U, 256, 15)
    for a, b, c in zip(full, again, part):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a[16:32].view(torch.int32), c.view(torch.int32))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calib_case0.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


@gpu
@pytest.mark.parametrize("seed,shape", R.CASES)
def test_gptq_reorder_rows_end_to_end(seed, shape, golden):
    """The assertions (2) and (3) of test_gpu_calibrate.test_gptq_reorder, on the same layers, with the GPU's own factor."""
    from qeft_amd.calibrate import HessianAccumulator, frob_norm_error, gptq_reorder, select_outliers
    W, X, hot = R.make_case(seed, **shape)
    K, r = W.shape[1], len(hot)
    if seed == 0:
        W, H, frob = golden["W"], golden["H"].to(DEV), golden["frob"].to(DEV)
    else:
        acc = HessianAccumulator(K, DEV)
        for j in range(X.shape[0]):
            acc.add_batch(X[j].to(DEV))
        H, frob = acc.H, frob_norm_error(W.to(DEV), 4, 128, "minmax")
    out_ids, ids = select_outliers(H, r, frob_norm=frob)
    idc = ids.cpu()
    Wp, Hp = W.float()[:, idc], H.cpu()[idc][:, idc]
    l64, l_rtn = R.proxy_loss(Wp, R.gptq_reorder(Wp, Hp, K - r, torch.float64)[0], Hp), R.proxy_loss(Wp, R.rtn(Wp, K - r), Hp)
    res = gptq_reorder(W.to(DEV), H, ids, r, factor="own", loop="rows")
    print(f"seed {seed}, rows: proxy loss {res.proxy_loss:.9g}, fp64 restatement {l64:.9g} (relative "
          f"{(res.proxy_loss - l64) / l64:+.3g}, margin {R.REL_MARGIN:.3g}), / RTN {res.proxy_loss / l_rtn:.3f}")
    assert res.weight.dtype == torch.float16 and torch.equal(res.out_ids.cpu(), out_ids.cpu())
    assert res.proxy_loss <= (1 + R.REL_MARGIN) * l64 and res.proxy_loss < 0.6 * l_rtn


@gpu
def test_calibrate_linear_rows_through_the_packed_kernels(golden):
    """The golden o_proj layer as test_gpu_calibrate checks it: module(x) against x Q^T, and closer to the dense layer than min-max."""
    import types
    from qeft_amd.calibrate import calibrate_linear
    from qeft_amd.qlinear import QuantLinear
    W, X, r, name = golden["W"], golden["X"], 64, "layers.0.self_attn.o_proj"
    N, K = W.shape
    lin = torch.nn.Linear(K, N, bias=False).half().to(DEV)
    lin.weight.data = W.to(DEV)
    module, info = calibrate_linear(lin, golden["H"].to(DEV), r, name, loop="rows", pack="device", factor="own")
    ids = info.ids.cpu()
    Qu = info.weight.cpu().double()[:, torch.argsort(ids)]
    Qr, sr, zr = R.rtn(W.float()[:, ids], K - r, return_params=True)
    plain = QuantLinear(4, K, N, False, torch.float16, r, 128, True, name)
    plain.pack(types.SimpleNamespace(weight=types.SimpleNamespace(data=Qr.half()), bias=None), scales=sr, zeros=zr,
               outlieridx=info.out_ids.cpu())
    plain = plain.to(DEV)
    plain.set_kernel()
    for m in (1, 16):
        x = X.reshape(-1, K)[40:40 + m].contiguous()
        y = module(x.to(DEV)).cpu().double()
        yq, y0 = x.double() @ Qu.T, x.double() @ W.double().T
        err, e_cal = (y - yq).abs().max().item() / yq.abs().max().item(), (y - y0).norm().item()
        e_rtn = (plain(x.to(DEV)).cpu().double() - y0).norm().item()
        print(f"rows, m = {m}: module vs x Q^T {err:.3g}; against the dense layer: calibrated {e_cal:.4g}, min-max {e_rtn:.4g}")
        assert y.shape == (m, N) and err < 1e-3 and e_cal < e_rtn


def test_refusals_without_a_gpu():
    """SHAPE, then GROUP, then NULL, then ALIGN; every call below has something wrong."""
    from qeft_amd import _lib, build
    from qeft_amd.calibrate import gptq_reorder
    build.build(verbose=False)
    lib = _lib.lib()
    ERR_SHAPE, ERR_GROUP, ERR_NULL, ERR_ALIGN, P = 2, 3, 4, 6, 1 << 20
    def call(w=P, h=2 * P, q=3 * P, e=4 * P, s=5 * P, z=6 * P, n=32, k=256, ld_w=256, ld_h=256, nn=192, maxq=15, g=128):
        return lib.qeft_gptq_rows(w, ld_w, h, ld_h, q, e, s, z, n, k, nn, maxq, g, None)
    for bad in (dict(n=0), dict(k=0), dict(k=192, ld_w=192, ld_h=192, nn=128), dict(k=32768 + 128, ld_w=1 << 16, ld_h=1 << 16),
                dict(ld_w=252), dict(ld_w=258), dict(ld_h=128), dict(ld_h=262), dict(nn=0), dict(nn=258), dict(nn=191), dict(maxq=3)):
        assert call(**bad) == ERR_SHAPE and call(**bad, w=None, g=64) == ERR_SHAPE, bad
    assert call(g=64) == ERR_GROUP and call(g=256, w=None) == ERR_GROUP
    for name in ("w", "h", "q", "e", "s", "z"):
        assert call(**{name: None}) == ERR_NULL, name
    for bad in (dict(w=P + 8), dict(h=P + 8), dict(q=P + 8), dict(e=P + 8), dict(s=5 * P + 2), dict(z=6 * P + 1)):
        assert call(**bad) == ERR_ALIGN, bad
    assert lib.qeft_gptq_rows_blocks(0) == 0 and [lib.qeft_gptq_rows_blocks(n) for n in (1, 16, 17, 4096)] == [1, 1, 2, 256]
    W, H, ids = torch.zeros(16, 128), torch.eye(128), torch.arange(128)
    with pytest.raises(ValueError, match="between launches"):
        gptq_reorder(W, H, ids, 0, tuning="mse", loop="rows")
    with pytest.raises(ValueError, match="loop"):
        gptq_reorder(W, H, ids, 0, loop="columns")
    with pytest.raises(ValueError, match="GPU"):                          # no CPU path and no torch fallback
        gptq_reorder(W, H, ids, 0, loop="rows")
