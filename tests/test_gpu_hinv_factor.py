"""Tests of the blocked factor of the inverse Hessian (qeft_hinv_factor, csrc/calib_factor.hip; calibrate.hinv_factor,
gptq_reorder(factor="own")).

The oracle is torch.linalg.cholesky(torch.linalg.inv(Hd64), upper=True) on the CPU, Hd64 the SAME fp32 matrix promoted to double.
Hd is a calib_ref.make_case Hessian (a quarter of the channels x 8) under a seeded permutation with percdamp = 0.01, as
gptq_reorder prepares it.  The bound on the own route is 2 x the Frobenius-relative error of the three torch calls in fp32 on the
GPU on the same input, computed in the same test: two fp32 algorithms with different summation orders, no absolute figure.

The last test is the CPU's: refusals only, under the rule of tests/test_train_rope_cpu.py -- no call hands the launching entry a
complete set of valid arguments."""
import functools
import os

import numpy as np
import pytest
import torch

import calib_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def case(K):
    """(Hd fp32 [K, K], the fp64 factor of its inverse), both on the CPU."""
    _, X, _ = R.make_case(40 + K, N=8, K=K, r=K // 4, S=2, T=K // 2 + 40)
    H = R.hessian64(X).float()
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    Hd = H[perm][:, perm].contiguous()
    Hd[range(K), range(K)] += 0.01 * torch.mean(torch.diag(Hd))
    return Hd, torch.linalg.cholesky(torch.linalg.inv(Hd.double()), upper=True)


@gpu
@pytest.mark.parametrize("K", [128, 256, 384, 1152])
def test_parity_with_the_fp64_factor(K):
    from qeft_amd import _lib, hinv_factor
    Hd, ref = case(K)
    g = Hd.to(DEV)
    u = hinv_factor(g).cpu()                                              # returns only with info == 0
    assert _lib.last_variant() == "hinv_factor_b128"
    assert torch.equal(g.cpu(), Hd)                                       # the caller's matrix is left alone
    three = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(g)), upper=True).cpu()
    rel = lambda t: ((t.double() - ref).norm() / ref.norm()).item()
    e_own, e_torch = rel(u), rel(three)
    print(f"K = {K}: Frobenius-relative error against the fp64 factor: own {e_own:.3g}, three torch calls {e_torch:.3g} "
          f"(ratio {e_own / e_torch:.3f})")
    assert u.shape == (K, K) and u.dtype == torch.float32
    assert torch.equal(torch.tril(u, -1), torch.zeros(K, K)) and (torch.diag(u) > 0).all()
    again = hinv_factor(Hd.to(DEV)).cpu()
    assert torch.equal(again.view(torch.int32), u.view(torch.int32))
    assert e_own <= 2 * e_torch


@gpu
def test_a_matrix_that_is_not_positive_definite():
    """Block 0 is the second block the sweep reaches; the smallest diagonal entry of it goes negative, so the matrix is indefinite.
    The pivot of a column depends on the rows and columns at or after it alone (the sweep starts at the bottom-right corner), so
    no column taken earlier sees the entry and exactly that column fails (test_gpu_calib_edges.test_the_status_names_the_column
    has the other positions).  A status, not a fault."""
    from qeft_amd import hinv_factor
    Hd = case(256)[0].clone()
    c = torch.argmin(torch.diag(Hd)[:128]).item()
    Hd[c, c] -= 2 * torch.mean(torch.diag(Hd))
    with pytest.raises(torch.linalg.LinAlgError, match="column") as e:
        hinv_factor(Hd.to(DEV))
    print(f"entry {c} made negative: info = {e.value.info}")
    assert e.value.info == c + 1


@gpu
@pytest.mark.parametrize("seed,shape", R.CASES)
def test_gptq_reorder_with_the_own_factor(seed, shape):
    """The cases and the two loss assertions of test_gpu_calibrate.test_gptq_reorder, with factor="own"."""
    from qeft_amd.calibrate import HessianAccumulator, frob_norm_error, gptq_reorder, select_outliers
    W, X, hot = R.make_case(seed, **shape)
    K, r = W.shape[1], len(hot)
    if seed == 0:                                                         # the golden layer: the reference's own H and Frobenius term
        z = np.load(os.path.join(ROOT, "tests", "golden", "calib_case0.npz"))
        W, H, frob = torch.from_numpy(z["W"]), torch.from_numpy(z["H"]).to(DEV), torch.from_numpy(z["frob"]).to(DEV)
    else:
        acc = HessianAccumulator(K, DEV)
        for j in range(X.shape[0]):
            acc.add_batch(X[j].to(DEV))
        H, frob = acc.H, frob_norm_error(W.to(DEV), 4, 128, "minmax")
    _, ids = select_outliers(H, r, frob_norm=frob)
    idc, Hc = ids.cpu(), H.cpu()
    Wp, Hp = W.float()[:, idc], Hc[idc][:, idc]
    l64 = R.proxy_loss(Wp, R.gptq_reorder(Wp, Hp, K - r, torch.float64)[0], Hp)
    l_rtn = R.proxy_loss(Wp, R.rtn(Wp, K - r), Hp)
    res = gptq_reorder(W.to(DEV), H, ids, r, factor="own")
    print(f"seed {seed}, factor own: proxy loss {res.proxy_loss:.9g}, fp64 restatement {l64:.9g} (relative "
          f"{(res.proxy_loss - l64) / l64:+.3g}, margin {R.REL_MARGIN:.3g}), / RTN {res.proxy_loss / l_rtn:.3f}")
    assert res.proxy_loss <= (1 + R.REL_MARGIN) * l64
    assert res.proxy_loss < 0.6 * l_rtn


def test_refusals_without_a_gpu():
    """SHAPE whatever the pointers are, then NULL, then ALIGN; every call below has something wrong."""
    import qeft_amd
    from qeft_amd import _lib, build, calibrate
    build.build(verbose=False)
    lib = _lib.lib()
    ERR_SHAPE, ERR_NULL, ERR_ALIGN, P = 2, 4, 6, 1 << 20
    call = lambda a=P, u=2 * P, info=3 * P, k=256, ld=256: lib.qeft_hinv_factor(a, ld, u, info, k, None)
    for bad in (dict(k=0, ld=0), dict(k=64, ld=64), dict(k=130, ld=132), dict(k=-128), dict(k=32768 + 128, ld=32768 + 128),
                dict(ld=252), dict(ld=258)):
        for ptr in ({}, dict(a=None, u=None, info=None), dict(a=3, u=3, info=3)):
            assert call(**ptr, **bad) == ERR_SHAPE, (bad, ptr)
    for name in ("a", "u", "info"):
        assert call(**{name: None}) == ERR_NULL and call(**{name: None}, k=32768, ld=32768) == ERR_NULL, name
        assert call(**{name: P + (8 if name != "info" else 2)}) == ERR_ALIGN, name
    assert call(u=P) == ERR_NULL                                          # in place is not offered
    assert [lib.qeft_hinv_factor_launches(k) for k in (128, 256, 4096, 11008, 64, 130)] == [1, 5, 95, 257, 0, 0]
    assert "hinv_factor" in qeft_amd.__all__ and "calib_factor.hip" in build.SOURCES and "calib_factor.h" in build.HEADERS
    with pytest.raises(ValueError, match="GPU"):                          # no CPU path and no torch fallback
        calibrate.hinv_factor(torch.eye(128))
    for bad in (torch.eye(128, dtype=torch.float64), torch.zeros(128, 256), torch.eye(192)):
        with pytest.raises(ValueError, match="fp32|multiple"):
            calibrate.hinv_factor(bad)
    with pytest.raises(ValueError, match="factor"):
        calibrate.gptq_reorder(torch.zeros(8, 128), torch.zeros(128, 128), torch.arange(128), 0, factor="hip")
