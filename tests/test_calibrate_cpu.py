"""CPU checks of the calibrator (qeft_amd/calibrate.py, csrc/calib.hip): the boundary, the refusals, the
address enumeration of qeft_hessian_accum, select_outliers (plain torch), and the tie between tests/calib_ref.py -- the oracle of
tests/test_gpu_calibrate.py -- and the reference's own GPTQ_OWQ through tests/golden/calib_case0.npz.

THE RULE OF THIS FILE (that of tests/test_oweight_optim_cpu.py).  Tests without the `gpu` mark also run where a GPU is present, so
no test here passes a launching entry a complete set of valid arguments: made-up pointers appear only in calls that a check
refuses.  qeft_hessian_accum_check_extents takes no pointer and is the one place for complete geometry.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import calib_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6
P = 1 << 20                       # a 16-byte aligned non-null "pointer": no call below gets as far as using it


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "calib_case0.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_symbols_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    from qeft_amd import _lib
    p, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    want = {"qeft_hessian_accum": (i, [p, p, i, i, f, f, p]),
            "qeft_hessian_accum_check_extents": (ll, [i, i]),
            "qeft_gptq_block": (i, [p, i, p, i, p, p, p, p, i, i, i, p])}
    for name, (restype, argtypes) in want.items():
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/qeft_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == argtypes and _lib.RESTYPES[name] is restype, name
    import qeft_amd
    from qeft_amd import build
    for name in ("HessianAccumulator", "frob_norm_error", "select_outliers", "gptq_reorder", "calibrate_linear"):
        assert name in qeft_amd.__all__ and callable(getattr(qeft_amd, name)), name
    assert "calib.hip" in build.SOURCES and "calib.h" in build.HEADERS


def _hess(lib, x=P, h=P, t=65, k=192):
    return lib.qeft_hessian_accum(x, h, t, k, 0.5, 0.5, None)


BLOCK_PTRS = ("w1", "hinv1", "scale", "zero", "q1", "err1")


def _block(lib, w1=P, hinv1=P, scale=P, zero=P, q1=P, err1=P, ld_w=256, ld_h=256, n=72, count=64, maxq=15):
    return lib.qeft_gptq_block(w1, ld_w, hinv1, ld_h, scale, zero, q1, err1, n, count, maxq, None)


def test_the_entries_refuse_without_launching(lib):
    """SHAPE whatever the pointers are, then NULL, then ALIGN.  No call has every argument in order (the rule of this file)."""
    for bad in (dict(k=0), dict(k=32), dict(k=100), dict(k=64 * 3 + 32), dict(k=-64), dict(k=1 << 16), dict(t=0), dict(t=-5),
                dict(t=(1 << 24) + 1)):
        for ptr in ({}, dict(x=None, h=None), dict(x=3, h=3)):
            assert _hess(lib, **ptr, **bad) == ERR_SHAPE, (bad, ptr)
    assert _hess(lib, x=None) == ERR_NULL and _hess(lib, h=None) == ERR_NULL and _hess(lib, x=None, h=P + 2) == ERR_NULL
    assert _hess(lib, x=P + 8) == ERR_ALIGN and _hess(lib, h=P + 4) == ERR_ALIGN
    assert _hess(lib, t=1, k=64, x=None) == ERR_NULL and _hess(lib, t=1 << 24, k=1 << 15, h=None) == ERR_NULL    # the limits pass
    for bad in (dict(count=0), dict(count=-1), dict(count=129), dict(count=1000), dict(maxq=3), dict(maxq=8), dict(maxq=16),
                dict(maxq=0), dict(n=0), dict(n=-8), dict(ld_w=63), dict(ld_h=63)):
        for ptr in ({}, {q: None for q in BLOCK_PTRS}, {q: 3 for q in BLOCK_PTRS}):
            assert _block(lib, **ptr, **bad) == ERR_SHAPE, (bad, ptr)
    for name in BLOCK_PTRS:
        other = next(q for q in BLOCK_PTRS if q != name)
        assert _block(lib, **{name: None}) == ERR_NULL, name
        assert _block(lib, **{name: None, other: P + 2}) == ERR_NULL, name
        assert _block(lib, **{name: P + 2}) == ERR_ALIGN, name
        for good in (dict(count=1, ld_w=1, ld_h=1), dict(count=128, ld_w=128, ld_h=128, maxq=7)):                 # the limits pass
            assert _block(lib, **{name: None}, **good) == ERR_NULL, (name, good)


@pytest.mark.parametrize("k", [64, 192])
@pytest.mark.parametrize("t", [1, 63, 65, 200])
def test_no_address_outside_x_or_h(lib, t, k):
    """Every address of every thread of every block, ragged T included: none outside X [t][k] or H [k][k], every element of H
    written exactly once."""
    assert lib.qeft_hessian_accum_check_extents(t, k) == 0
    assert lib.qeft_hessian_accum_check_extents(t, k + 1) == -1 and lib.qeft_hessian_accum_check_extents(0, k) == -1
    assert lib.qeft_hessian_accum_check_extents(1, 4096 + 64) == -1          # the walk answers for K <= 4096 only


def test_the_python_interface_refuses_what_it_does_not_support():
    from qeft_amd import calibrate as C
    W, H, ids = torch.zeros(8, 256), torch.zeros(256, 256), torch.arange(256)
    for kw, word in ((dict(group_size=64), "128"), (dict(sym=True), "sym"), (dict(bits=2), "3 and 4"), (dict(bits=8), "3 and 4")):
        with pytest.raises(ValueError, match=word):
            C.gptq_reorder(W, H, ids, 64, **kw)
    with pytest.raises(ValueError, match="even"):
        C.gptq_reorder(W, H, ids, 63)
    with pytest.raises(ValueError, match="multiple of 128"):            # K = 192: K / 128 groups could not hold the two started ones
        C.gptq_reorder(torch.zeros(8, 192), torch.zeros(192, 192), torch.arange(192), 0)
    with pytest.raises(ValueError, match="GPU"):                        # no CPU path and no torch fallback
        C.gptq_reorder(W, H, ids, 64)
    with pytest.raises(ValueError, match="GPU"):
        C.HessianAccumulator(256, "cpu")
    with pytest.raises(ValueError, match="64"):
        C.HessianAccumulator(100, "cuda:0")


def test_select_outliers(golden):
    from qeft_amd.calibrate import select_outliers
    from qeft_amd.reorder import sparse_to_dense_ids
    H, K = golden["H"], golden["H"].shape[0]
    out_ids, ids = select_outliers(H, 64, frob_norm=golden["frob"])
    assert out_ids.dtype == torch.int32 and torch.equal(out_ids, golden["out_ids"])           # the reference's choice
    assert torch.equal(out_ids.long(), golden["hot"])                                          # ... the 64 scaled channels
    assert torch.equal(ids, sparse_to_dense_ids(out_ids, K)) and torch.equal(torch.sort(ids)[0], torch.arange(K))
    # the reference's ids hold the same columns; only the outliers' order among themselves differs (descending score there)
    assert torch.equal(ids[:K - 64], golden["ids"][:K - 64]) and torch.equal(torch.sort(golden["ids"][K - 64:])[0], ids[K - 64:])
    out2, ids2 = select_outliers(H, 64)                                                        # diag(H) alone
    assert torch.equal(ids2, sparse_to_dense_ids(out2, K)) and torch.equal(out2, torch.sort(out2)[0])
    given = torch.tensor([200, 3, 77, 5], dtype=torch.int64)
    out3, ids3 = select_outliers(H, 4, frob_norm=golden["frob"], outidx=given)
    assert out3.dtype == torch.int32 and torch.equal(out3.long(), given)
    assert torch.equal(ids3, sparse_to_dense_ids(given, K)) and torch.equal(ids3[-4:], given)
    assert torch.equal(H, golden["H"])                                                         # H is not modified


def test_frob_norm_error_is_the_reference_term(golden):
    from qeft_amd.calibrate import frob_norm_error
    torch.testing.assert_close(frob_norm_error(golden["W"], 4, 128, "minmax"), golden["frob"], rtol=1e-6, atol=0)


def test_mse_params_are_the_references_search():
    """tests/golden/calib_mse0.npz: one group of 128 columns (a zero row and a one-sided row among them) and what the reference's
    Quantizer.find_params(mse=True, num=40) returned for it at 4 and 3 bits.  The restatement is the same elementwise operations
    and the same row means in the same order, so scale and zero are the reference's bit for bit."""
    from qeft_amd.calibrate import mse_params
    z = np.load(os.path.join(ROOT, "tests", "golden", "calib_mse0.npz"))
    x = torch.from_numpy(z["x"])
    for nbits in (4, 3):
        s, zero = mse_params(x, nbits)
        assert torch.equal(s, torch.from_numpy(z[f"scale{nbits}"])) and torch.equal(zero, torch.from_numpy(z[f"zero{nbits}"])), nbits


def test_mse_params_stay_on_the_grid():
    """The restated search returns integral zeros in 0..maxq and a positive scale, and its 2.4-norm score beats min-max's (whose
    range is the search's last candidate) on average and is within 2 % of it on every row (the returned scale is recomputed from
    the best range, so single roundings can move)."""
    from qeft_amd.calibrate import mse_params
    from qeft_amd.quant import minmax_params, quantize
    x = torch.randn(16, 128, generator=torch.Generator().manual_seed(5)) * 0.02
    x[3] = 0
    s, z = mse_params(x, 4)
    assert s.shape == (16, 1) and (s > 0).all() and torch.equal(z, z.round()) and z.min() >= 0 and z.max() <= 15
    s0, z0 = minmax_params(x, 128, 4)
    score = lambda s, z: (x - quantize(x, s, z, 0, 15)).abs().pow(2.4).mean(1)
    assert (score(s, z) <= score(s0, z0) * 1.02).all() and score(s, z).mean() < score(s0, z0).mean()


def test_the_oracle_is_the_references_algorithm(golden):
    """The fp32 restatement of tests/calib_ref.py on the golden layer, in the REFERENCE's column order (its outliers sit in
    descending score, which reaches the factor's last bits): zero_group is the reference's exactly, scale_group bit for bit in
    the first group (the untouched weights); the second group's scale is (max - min) / 15 of columns that have seen one trailing
    GEMM, whose summation order is the BLAS's: with T = sum_k |Err1_k Hinv_kj| either side sits within gamma(128) T + u |w| of
    the exact column (any order of the 128 terms, then the subtraction), so two sides, two extremes and the two roundings of the
    scale itself give |ds| <= 2 (2 max_j dw_j) / 15 + 4 u s -- the factor and Err1 taken as the same bits, which is the one thing
    this does not cover (another LAPACK).  Where the golden was made the difference is 0.  The values are the reference's, and the proxy loss is the reference's within the margin of the GPU test.  In OUR
    column order -- what the GPU test runs -- the fp32 and fp64 restatements stay within the same margin of the reference."""
    W, H, K, r = golden["W"].float(), golden["H"], 256, 64
    l_ref = R.proxy_loss(W, golden["Q"], H)
    rid = golden["ids"]
    Q32, s32, z32, _ = R.gptq_reorder(W[:, rid], H[rid][:, rid], K - r, torch.float32)
    assert s32.shape == (32, 2) and z32.shape == (32, 2) and torch.equal(z32, golden["zero_group"])
    assert torch.equal(s32[:, 0], golden["scale_group"][:, 0])
    # the second group has seen W[:, 128:] -= Err1 @ Hinv[:128, 128:]: a 128-term fp32 dot in the BLAS's order, then one subtraction
    Wr, (h, _) = W[:, rid], R.factor(H[rid][:, rid], torch.float32)
    _, E1, _ = R.block_lines(Wr[:, :128], h[:128, :128], s32[:, 0], z32[:, 0], 15.0)
    T = E1.abs().double() @ h[:128, 128:K - r].abs().double()
    w2 = Wr[:, 128:K - r].double() - E1.double() @ h[:128, 128:K - r].double()
    dw = (R.gamma(128) * T + R.U * w2.abs()).max(1)[0]                    # one side's distance from the exact column, worst column
    ds = 2 * (2 * dw) / 15 + 4 * R.U * golden["scale_group"][:, 1].double()
    gap = (s32[:, 1].double() - golden["scale_group"][:, 1].double()).abs()
    print(f"second group's scale: largest |difference| / slack {(gap / ds).max().item():.3g} (slack / scale up to {(ds / s32[:, 1]).max().item():.3g})")
    assert (gap <= ds).all()
    same = (golden["Q"][:, rid][:, :K - r] == Q32[:, :K - r]).float().mean().item()
    l32r = R.proxy_loss(W[:, rid], Q32, H[rid][:, rid])
    print(f"reference order: live values equal to the reference's {same:.4f}; proxy loss reference {l_ref:.9g}, restatement {l32r:.9g}")
    assert same > 0.99 and abs(l32r - l_ref) <= R.REL_MARGIN * l_ref
    ids = R.dense_ids(golden["out_ids"], K)
    Wp, Hp = W[:, ids], H[ids][:, ids]
    for dtype in (torch.float32, torch.float64):
        Q, s, z, _ = R.gptq_reorder(Wp, Hp, K - r, dtype)
        loss = R.proxy_loss(Wp, Q, Hp)
        print(f"our order, {dtype}: proxy loss {loss:.9g} (reference {l_ref:.9g}, RTN {R.proxy_loss(Wp, R.rtn(Wp, K - r), Hp):.6g})")
        assert torch.equal(z.float(), golden["zero_group"]) and abs(loss - l_ref) <= R.REL_MARGIN * l_ref


def test_the_margin_is_what_the_restatements_measure():
    """REL_MARGIN = 16 x the largest relative difference between the fp32 and the fp64 restatement over the GPU tests' cases (R.CASES at 4 bits, R.CASES_W3 at 3)
    (with the fp32 restatement's own factor and with the fp64 factor).  Measured here and printed; the fp32 restatement itself
    must meet the GPU test's condition, which leaves the factor 16 for another BLAS's summation order."""
    worst = 0.0
    for seed, shape, nbits in [(s, sh, 4) for s, sh in R.CASES] + [(s, sh, 3) for s, sh in R.CASES_W3]:
        W, X, hot = R.make_case(seed, **shape)
        K, r = W.shape[1], len(hot)
        ids = R.dense_ids(hot, K)
        Wp, Hp = W.float()[:, ids], R.hessian64(X).float()[ids][:, ids]
        Q64, _, _, h64 = R.gptq_reorder(Wp, Hp, K - r, torch.float64, bits=nbits)
        l64 = R.proxy_loss(Wp, Q64, Hp)
        for hinv in (None, h64):
            l32 = R.proxy_loss(Wp, R.gptq_reorder(Wp, Hp, K - r, torch.float32, bits=nbits, hinv=hinv)[0], Hp)
            worst = max(worst, abs(l32 - l64) / l64)
        ratio = l64 / R.proxy_loss(Wp, R.rtn(Wp, K - r, bits=nbits), Hp)
        print(f"seed {seed}, {nbits} bits: fp64 loss {l64:.9g}, / RTN {ratio:.3f}, worst relative fp32 - fp64 so far {worst:.3g}")
        assert ratio < 0.5
    assert worst <= R.REL_MARGIN
