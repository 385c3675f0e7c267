"""CPU checks of the training glue's boundary (csrc/train_glue.hip, qeft_amd/glue.py): the four entries and
the address enumeration are declared and exported and the glue functions are in qeft_amd.__all__; every entry refuses bad arguments
in the documented order -- QEFT_ERR_SHAPE with every pointer null and misaligned, then NULL, then ALIGN -- before any HIP call; the
host-side enumeration of every address a launch forms finds none outside its operand over the sweep of widths, row counts and
strides of tests/test_gpu_train_glue.py and returns -1 for what the entries refuse; finetune.causal_lm_loss refuses a bad `glue`
before anything is touched, and the glue functions refuse CPU tensors and bad shapes."""
import itertools
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["qeft_add_rmsnorm_fwd", "qeft_add_rmsnorm_bwd", "qeft_swiglu_fwd", "qeft_swiglu_bwd", "qeft_train_glue_check_extents"]
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6
OP_NORM_FWD, OP_NORM_BWD, OP_SWIGLU_FWD, OP_SWIGLU_BWD = range(4)
P = 1 << 20                       # a 16-byte aligned non-null "pointer": no entry below gets as far as using it
EPS = 1e-5


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_symbols_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/qeft_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    for i, name in enumerate(("ADD_RMSNORM_FWD", "ADD_RMSNORM_BWD", "SWIGLU_FWD", "SWIGLU_BWD")):
        assert re.search(r"#define\s+QEFT_GLUE_%s\s+%d\b" % (name, i), text), name
    import qeft_amd
    for name in ("add_rmsnorm", "swiglu"):
        assert name in qeft_amd.__all__
        assert callable(getattr(qeft_amd, name))
    assert lib.qeft_abi_version() == 1
    from qeft_amd import build
    assert "train_glue.hip" in build.SOURCES and "train_glue.h" in build.HEADERS


# ---- the entries with every argument overridable by name
def _norm_fwd(lib, h=P, add=P, gamma=P, sum_out=P, y=P, m=4, hidden=4096):
    return lib.qeft_add_rmsnorm_fwd(h, add, gamma, sum_out, y, m, hidden, EPS, None)


def _norm_bwd(lib, s=P, gamma=P, dy=P, dres=P, dsum=P, m=4, hidden=4096):
    return lib.qeft_add_rmsnorm_bwd(s, gamma, dy, dres, dsum, m, hidden, EPS, None)


def _sw_fwd(lib, gate=P, up=P, out=P, m=4, n=11008, gate_stride=None, up_stride=None):
    return lib.qeft_swiglu_fwd(gate, up, out, m, n, n if gate_stride is None else gate_stride, n if up_stride is None else up_stride, None)


def _sw_bwd(lib, gate=P, up=P, dact=P, dgate=P, dup=P, m=4, n=11008, strides=None):
    s = dict(gate=n, up=n, dact=n, dgate=n, dup=n)
    s.update(strides or {})
    return lib.qeft_swiglu_bwd(gate, up, dact, dgate, dup, m, n, s["gate"], s["up"], s["dact"], s["dgate"], s["dup"], None)


def _in_order(call, ptrs, bad_shapes, optional=()):
    """call(**kw) refuses every bad shape with SHAPE whatever the pointers are (all good, all null, all odd), then a null required
    pointer with NULL even when another pointer is misaligned, then a misaligned pointer with ALIGN."""
    nul, odd = {p: None for p in ptrs}, {p: 3 for p in ptrs}
    for bad in bad_shapes:
        for ptr in ({}, nul, odd):
            assert call(**ptr, **bad) == ERR_SHAPE, (bad, ptr)
    for name in ptrs:
        if name in optional:
            continue
        other = next(p for p in ptrs if p != name and p not in optional)
        assert call(**{name: None}) == ERR_NULL, name
        assert call(**{name: None, other: P + 2}) == ERR_NULL, name               # NULL before ALIGN
    # (no call here has every argument in order: that would be a launch on these made-up addresses wherever there is a GPU)
    for name in ptrs:
        assert call(**{name: P + 8}) == ERR_ALIGN, name


ROW_SHAPES = [dict(m=0), dict(m=-1), dict(m=2 ** 20 + 1)]


def test_add_rmsnorm_fwd_refuses_in_order_without_a_gpu(lib):
    call = lambda **kw: _norm_fwd(lib, **kw)
    _in_order(call, ("h", "add", "gamma", "sum_out", "y"), ROW_SHAPES + [dict(hidden=0), dict(hidden=4), dict(hidden=4100), dict(hidden=-8)],
              optional=("add", "sum_out"))
    assert call(add=None, sum_out=None, h=None) == ERR_NULL                        # the plain norm is taken up to the pointers
    assert call(add=None) == ERR_NULL and call(sum_out=None) == ERR_NULL           # sum_out is NULL iff add is
    assert call(add=None, sum_out=None, y=P + 8) == ERR_ALIGN
    assert call(m=2 ** 20, h=None) == ERR_NULL                                     # 2^20 rows are taken


def test_add_rmsnorm_bwd_refuses_in_order_without_a_gpu(lib):
    call = lambda **kw: _norm_bwd(lib, **kw)
    _in_order(call, ("s", "gamma", "dy", "dres", "dsum"), ROW_SHAPES + [dict(hidden=0), dict(hidden=12), dict(hidden=4100)],
              optional=("dy", "dres"))
    for ptr in ({}, dict(s=None, gamma=None, dsum=None), dict(s=3, gamma=3, dsum=3)):
        assert call(dy=None, dres=None, **ptr) == ERR_SHAPE                        # no gradient at all
    assert call(dy=None, s=None) == ERR_NULL and call(dres=None, s=None) == ERR_NULL
    assert call(dy=None, dsum=P + 8) == ERR_ALIGN and call(dres=None, dsum=P + 8) == ERR_ALIGN


def test_swiglu_refuses_in_order_without_a_gpu(lib):
    widths = [dict(n=0), dict(n=4), dict(n=11012), dict(n=-8)]
    _in_order(lambda **kw: _sw_fwd(lib, **kw), ("gate", "up", "out"),
              ROW_SHAPES + widths + [dict(gate_stride=11004), dict(gate_stride=11000), dict(up_stride=11012), dict(up_stride=8)])
    assert _sw_fwd(lib, gate_stride=22016, up_stride=22016, gate=None) == ERR_NULL                # halves of a fused gate|up buffer
    strides = [dict(strides={nm: v}) for nm in ("gate", "up", "dact", "dgate", "dup") for v in (11012, 11000)]
    _in_order(lambda **kw: _sw_bwd(lib, **kw), ("gate", "up", "dact", "dgate", "dup"), ROW_SHAPES + widths + strides)


# ---- the address enumeration, over the GPU tests' sweep
NORM_H = (8, 128, 2048, 2056, 4096, 5120, 8192)
ROWS = (1, 3, 65)
SWIGLU_N = (8, 512, 2056, 11008, 28672)


def test_no_address_outside_its_operand(lib):
    ext = lib.qeft_train_glue_check_extents
    n = 0
    for op, m, hidden in itertools.product((OP_NORM_FWD, OP_NORM_BWD), ROWS, NORM_H):
        assert ext(op, m, hidden, 0, 0, 0, 0, 0) == 0, (op, m, hidden)
        n += 1
    for m, width in itertools.product(ROWS, SWIGLU_N):
        for pad in (0, 8, width):
            assert ext(OP_SWIGLU_FWD, m, width, width + pad, width + 2 * pad, 0, 0, 0) == 0, (m, width, pad)
            assert ext(OP_SWIGLU_BWD, m, width, width + pad, width + 2 * pad, width + pad, width + 3 * pad, width) == 0, (m, width, pad)
            n += 2
    assert n == 2 * 3 * 7 + 3 * 5 * 3 * 2


def test_the_enumeration_refuses_what_the_entries_refuse(lib):
    ext = lib.qeft_train_glue_check_extents
    assert ext(OP_NORM_FWD, 0, 4096, 0, 0, 0, 0, 0) == -1 and ext(OP_NORM_BWD, 4, 4100, 0, 0, 0, 0, 0) == -1
    assert ext(OP_NORM_FWD, 2 ** 20 + 1, 8, 0, 0, 0, 0, 0) == -1
    assert ext(OP_SWIGLU_FWD, 4, 512, 504, 512, 0, 0, 0) == -1 and ext(OP_SWIGLU_FWD, 4, 516, 516, 516, 0, 0, 0) == -1
    assert ext(OP_SWIGLU_BWD, 4, 512, 512, 512, 512, 516, 512) == -1 and ext(OP_SWIGLU_BWD, 4, 512, 512, 512, 512, 512, 8) == -1
    assert ext(4, 4, 512, 512, 512, 512, 512, 512) == -1 and ext(-1, 4, 512, 512, 512, 512, 512, 512) == -1


# ---- Python
def test_causal_lm_loss_refuses_a_bad_glue_before_anything_is_touched():
    """A bare shape is all the 'model' has: the refusal comes before the weights, the tokens or the library are looked at."""
    from qeft_amd import finetune
    from qeft_amd.llama import LlamaShape
    model = types.SimpleNamespace(shape=LlamaShape(512, 512, 2, 4, 2, 512, max_seq=256))
    for bad in ("bogus", None, "Fused", 1):
        with pytest.raises(ValueError, match="glue"):
            finetune.causal_lm_loss(model, None, glue=bad)
        with pytest.raises(ValueError, match="glue"):
            finetune.causal_lm_loss(model, None, attn="own", head="torch", glue=bad)


def test_glue_functions_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from qeft_amd import add_rmsnorm, swiglu
    z = lambda *shape, dtype=torch.float16: torch.zeros(*shape, dtype=dtype)
    with pytest.raises(RuntimeError, match="GPU"):
        add_rmsnorm(z(4, 64), None, z(64), 1e-5)
    with pytest.raises(RuntimeError, match="GPU"):
        add_rmsnorm(z(4, 64), z(4, 64), z(64), 1e-5)
    with pytest.raises(RuntimeError, match="GPU"):
        swiglu(z(4, 64), z(4, 64))
    with pytest.raises(ValueError, match="fp16"):
        swiglu(_Fake(torch.float32, (4, 64)), _Fake(torch.float16, (4, 64)))
    f16 = torch.float16
    with pytest.raises(ValueError, match="multiple of 8"):
        add_rmsnorm(_Fake(f16, (4, 12)), None, _Fake(f16, (12,)), 1e-5)
    with pytest.raises(ValueError, match="gamma"):
        add_rmsnorm(_Fake(f16, (4, 64)), None, _Fake(f16, (32,)), 1e-5)
    with pytest.raises(ValueError, match="add"):
        add_rmsnorm(_Fake(f16, (4, 64)), _Fake(f16, (3, 64)), _Fake(f16, (64,)), 1e-5)
    with pytest.raises(ValueError, match=r"\[m, hidden\]"):
        add_rmsnorm(_Fake(f16, (2, 4, 64)), None, _Fake(f16, (64,)), 1e-5)
    with pytest.raises(ValueError, match="multiple of 8"):
        swiglu(_Fake(f16, (4, 20)), _Fake(f16, (4, 20)))
    with pytest.raises(ValueError, match="one shape"):
        swiglu(_Fake(f16, (4, 64)), _Fake(f16, (4, 32)))


def _Fake(dtype, shape):
    """A tensor that says it is on the GPU: the shape and dtype refusals come before any launch, so nothing dereferences it."""
    import torch

    class Fake(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    return torch.zeros(*shape, dtype=dtype).as_subclass(Fake)
