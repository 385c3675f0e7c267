"""CPU checks of the MSE parameter search (qeft_mse_search, csrc/calib_mse.hip; calibrate.mse_search): the boundary and the
refusals.  The rule of tests/test_calibrate_cpu.py holds: no call hands the launching entry a complete set of valid arguments."""
import ctypes

import pytest
import torch

ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6
P = 1 << 20                       # a non-null aligned "pointer": no call below gets as far as using it


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _search(lib, x=P, scale=P, zero=P, ld=131, n=67, g=128, maxq=15, num=40):
    return lib.qeft_mse_search(x, ld, n, g, maxq, num, scale, zero, None)


def test_symbol_and_refusals(lib):
    """Declared, exported, bound and public; then SHAPE whatever the pointers are, then NULL, then ALIGN."""
    import qeft_amd
    from qeft_amd import _lib, build
    p, i = ctypes.c_void_p, ctypes.c_int
    assert hasattr(lib, "qeft_mse_search")
    assert _lib.SIGNATURES["qeft_mse_search"] == [p, i, i, i, i, i, p, p, p] and _lib.RESTYPES["qeft_mse_search"] is i
    assert "mse_search" in qeft_amd.__all__ and callable(qeft_amd.mse_search)
    assert "calib_mse.hip" in build.SOURCES and "calib_mse.h" in build.HEADERS
    for bad in (dict(n=0), dict(n=-1), dict(g=0), dict(g=32769), dict(ld=127), dict(maxq=3), dict(maxq=8), dict(maxq=16), dict(maxq=0),
                dict(num=0), dict(num=41), dict(num=-40)):
        for ptr in ({}, dict(x=None, scale=None, zero=None), dict(x=3, scale=3, zero=3)):
            assert _search(lib, **ptr, **bad) == ERR_SHAPE, (bad, ptr)
    for name in ("x", "scale", "zero"):
        other = "scale" if name == "x" else "x"
        assert _search(lib, **{name: None}) == ERR_NULL and _search(lib, **{name: None, other: P + 2}) == ERR_NULL, name
        assert _search(lib, **{name: P + 2}) == ERR_ALIGN, name
        for good in (dict(n=1, g=1, ld=1, num=1, maxq=7), dict(g=32768, ld=32768)):                  # the limits pass
            assert _search(lib, **{name: None}, **good) == ERR_NULL, (name, good)


def test_the_python_interface_refuses_what_it_does_not_support():
    from qeft_amd import calibrate as C
    for call in (lambda: C.mse_search(torch.zeros(8, 128)), lambda: C.frob_norm_error(torch.zeros(8, 128), 4, 128, "mse")):
        with pytest.raises(ValueError, match="GPU"):                      # no CPU path and no torch fallback
            call()
    with pytest.raises(ValueError, match="mse_torch"):
        C._params(torch.zeros(8, 128), 4, "mse_hip")
    assert C._params(torch.zeros(2, 128), 4, "mse_torch")[0].shape == (2, 1)          # the comparison route is plain torch
    for bad in (torch.zeros(8, 128, dtype=torch.float16), torch.zeros(8, 128, dtype=torch.float64), torch.zeros(8)):
        with pytest.raises(ValueError, match="fp32"):
            C.mse_search(bad)
    with pytest.raises(ValueError, match="3 and 4"):
        C.mse_search(torch.zeros(8, 128), bits=2)
