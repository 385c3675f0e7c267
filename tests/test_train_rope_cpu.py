"""CPU checks of the training rotary's boundary (qeft_rope_qk in csrc/train_glue.hip, qeft_amd.glue.rope_qk,
finetune.causal_lm_loss(rope="fused")): the entry and its address enumeration are declared and exported
and rope_qk is in qeft_amd.__all__; the entry refuses bad arguments in the documented order -- QEFT_ERR_SHAPE whatever the
pointers are, then NULL, then ALIGN -- before any HIP call; the host-side enumeration of every address a launch forms finds none
outside its operand over the whole sweep of tests/test_gpu_train_rope.py and returns -1 for what the entry refuses;
causal_lm_loss refuses a bad `rope` before anything is touched; rope_qk refuses CPU tensors and bad dtypes and shapes; and a
numpy restatement of the pinned arithmetic (each product rounded to fp32, their sum rounded to fp32, that converted to fp16;
in the backward + (+0) in fp16, the sum autograd forms over the two half-slices) equals finetune._rope and its autograd bit for
bit on the CPU -- the anchor of the contract the GPU tests hold the kernel to.

THE RULE OF THIS FILE.  Tests without the `gpu` mark also run on a machine that has a GPU, in a whole-suite run.  So no test here
may make a call that passes every check of a launching entry: that would be a launch on made-up addresses wherever a device is
present (an earlier version of this feature was withdrawn for exactly that; DESIGN.md sections 4.16 and 8).  Made-up addresses
appear only in calls that some check refuses -- `_in_order` below never calls with every argument in order.  The CPU-only
enumeration qeft_rope_qk_check_extents, which takes no pointer, is the one place where complete, valid geometry is passed.  The
fake "is_cuda" tensors reach refusals only: every rope_qk call on them is one a shape or dtype check turns away before the
library is touched."""
import itertools
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6
P = 1 << 20                       # a 16-byte aligned non-null "pointer": no call below gets as far as using it
PTRS = ("q", "k", "cos_tab", "sin_tab", "q_out", "k_out")

# the sweep of tests/test_gpu_train_rope.py: (n_heads, n_kv_heads, q_stride, k_stride)
T_LENS = (1, 5, 67)
BATCHES = (1, 3)
LAYOUTS = [(1, 1, 128, 128),              # dense
           (4, 2, 512, 256),              # dense
           (4, 2, 1024, 1024),            # views of an 8-head fused q|k|v buffer
           (33, 3, 33 * 128, 3 * 128),    # dense, more heads than a block has groups, an odd count
           (64, 8, 10240, 10240),         # views of an 80-head fused buffer
           (4, 2, 520, 264)]              # row strides padded by 8


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_symbols_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    for name in ("qeft_rope_qk", "qeft_rope_qk_check_extents"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/qeft_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    import ctypes
    from qeft_amd import _lib
    p, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["qeft_rope_qk"] == [p] * 6 + [i] * 7 + [p] and _lib.RESTYPES["qeft_rope_qk"] is i
    assert _lib.SIGNATURES["qeft_rope_qk_check_extents"] == [i] * 6 and _lib.RESTYPES["qeft_rope_qk_check_extents"] is ctypes.c_longlong
    import qeft_amd
    assert "rope_qk" in qeft_amd.__all__ and callable(qeft_amd.rope_qk)
    assert lib.qeft_abi_version() == 1


def _entry(lib, q=P, k=P, cos_tab=P, sin_tab=P, q_out=P, k_out=P, rows=10, t_len=5, n_heads=4, n_kv_heads=2, q_stride=None,
           k_stride=None, inverse=0):
    """qeft_rope_qk with every argument overridable by name."""
    return lib.qeft_rope_qk(q, k, cos_tab, sin_tab, q_out, k_out, rows, t_len, n_heads, n_kv_heads,
                            n_heads * 128 if q_stride is None else q_stride, n_kv_heads * 128 if k_stride is None else k_stride,
                            inverse, None)


BAD_SHAPES = [dict(rows=0), dict(rows=-5), dict(rows=2 ** 20 + 1, t_len=1), dict(t_len=0), dict(t_len=-5), dict(t_len=3), dict(t_len=20),
              dict(n_heads=0), dict(n_heads=-1), dict(n_heads=257), dict(n_kv_heads=0), dict(n_kv_heads=257),
              dict(q_stride=504), dict(q_stride=516), dict(q_stride=0), dict(q_stride=2 ** 24 + 8), dict(k_stride=248), dict(k_stride=260),
              dict(k_stride=-256), dict(inverse=2), dict(inverse=-1)]


def test_rope_qk_refuses_in_order_without_a_gpu(lib):
    """SHAPE whatever the pointers are (all good, all null, all odd), then a null pointer with NULL even when another pointer is
    misaligned, then a misaligned pointer with ALIGN.  No call has every argument in order (the rule of this file)."""
    call = lambda **kw: _entry(lib, **kw)
    nul, odd = {p: None for p in PTRS}, {p: 3 for p in PTRS}
    for bad in BAD_SHAPES:
        for ptr in ({}, nul, odd):
            assert call(**ptr, **bad) == ERR_SHAPE, (bad, ptr)
    for name in PTRS:
        other = next(p for p in PTRS if p != name)
        assert call(**{name: None}) == ERR_NULL, name
        assert call(**{name: None, other: P + 2}) == ERR_NULL, name               # NULL before ALIGN
        assert call(**{name: None}, inverse=1) == ERR_NULL, name
    for name in PTRS:
        assert call(**{name: P + 8}) == ERR_ALIGN, name
        assert call(**{name: P + 2}, inverse=1) == ERR_ALIGN, name
    # the limits themselves are taken up to the pointers
    assert call(rows=2 ** 20, t_len=2 ** 10, q=None) == ERR_NULL
    assert call(n_heads=256, n_kv_heads=256, k=None) == ERR_NULL
    assert call(q_stride=1024, k_stride=1024, q_out=None) == ERR_NULL                # views of a fused q|k|v buffer
    assert call(q_stride=520, k_stride=264, sin_tab=None) == ERR_NULL


def test_no_address_outside_its_operand(lib):
    ext = lib.qeft_rope_qk_check_extents
    n = 0
    for T, B, (H, Hkv, qs, ks) in itertools.product(T_LENS, BATCHES, LAYOUTS):
        assert ext(B * T, T, H, Hkv, qs, ks) == 0, (T, B, H, Hkv, qs, ks)
        n += 1
    assert n == 3 * 2 * 6
    # the model test's and the benchmark's geometry (a few rows of the latter: the enumeration walks every thread)
    assert ext(200, 200, 4, 2, 512, 256) == 0 and ext(200, 100, 4, 4, 512, 512) == 0
    assert ext(64, 32, 32, 32, 4096, 4096) == 0 and ext(256, 256, 256, 256, 32768, 32768 + 8) == 0


def test_the_enumeration_refuses_what_the_entry_refuses(lib):
    ext = lib.qeft_rope_qk_check_extents
    for bad in BAD_SHAPES:
        if "inverse" in bad:
            continue
        a = dict(rows=10, t_len=5, n_heads=4, n_kv_heads=2, q_stride=None, k_stride=None)
        a.update(bad)
        qs = a["n_heads"] * 128 if a["q_stride"] is None else a["q_stride"]
        ks = a["n_kv_heads"] * 128 if a["k_stride"] is None else a["k_stride"]
        assert ext(a["rows"], a["t_len"], a["n_heads"], a["n_kv_heads"], qs, ks) == -1, bad
    train = lib.qeft_train_glue_check_extents                    # the glue's enumeration did not grow an op
    assert train(4, 4, 512, 512, 512, 512, 512, 512) == -1


def test_causal_lm_loss_refuses_a_bad_rope_before_anything_is_touched():
    """A bare shape is all the 'model' has: the refusal comes before the weights, the tokens or the library are looked at."""
    from qeft_amd import finetune
    from qeft_amd.llama import LlamaShape
    model = types.SimpleNamespace(shape=LlamaShape(512, 512, 2, 4, 2, 512, max_seq=256))
    for bad in ("bogus", None, "Fused", 1, True):
        with pytest.raises(ValueError, match="rope"):
            finetune.causal_lm_loss(model, None, rope=bad)
        with pytest.raises(ValueError, match="rope"):
            finetune.causal_lm_loss(model, None, attn="own", head="torch", glue="fused", rope=bad)


def _Fake(dtype, shape):
    """A tensor that says it is on the GPU.  It only ever reaches a refusal: the shape and dtype checks come before the library is
    touched, so nothing dereferences it (the rule of this file)."""
    import torch

    class Fake(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    return torch.zeros(*shape, dtype=dtype).as_subclass(Fake)


def test_rope_qk_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from qeft_amd import rope_qk
    f16, f32 = torch.float16, torch.float32
    z = lambda *shape, dtype=f16: torch.zeros(*shape, dtype=dtype)
    with pytest.raises(RuntimeError, match="GPU"):
        rope_qk(z(1, 5, 4, 128), z(1, 5, 2, 128), z(5, 64, dtype=f32), z(5, 64, dtype=f32))
    with pytest.raises(RuntimeError, match="GPU"):                                   # q and k say GPU, the tables are the CPU's
        rope_qk(_Fake(f16, (1, 5, 4, 128)), _Fake(f16, (1, 5, 2, 128)), z(5, 64, dtype=f32), z(5, 64, dtype=f32))
    q, k, c, s = _Fake(f16, (1, 5, 4, 128)), _Fake(f16, (1, 5, 2, 128)), _Fake(f32, (5, 64)), _Fake(f32, (5, 64))
    with pytest.raises(ValueError, match="fp16"):
        rope_qk(_Fake(f32, (1, 5, 4, 128)), k, c, s)
    with pytest.raises(ValueError, match="fp16"):
        rope_qk(q, _Fake(torch.bfloat16, (1, 5, 2, 128)), c, s)
    with pytest.raises(ValueError, match="fp32"):
        rope_qk(q, k, _Fake(f16, (5, 64)), s)
    with pytest.raises(ValueError, match="128"):                                     # a head size other than 128
        rope_qk(_Fake(f16, (1, 5, 4, 64)), _Fake(f16, (1, 5, 2, 64)), c, s)
    with pytest.raises(ValueError, match="128"):
        rope_qk(_Fake(f16, (5, 4, 128)), _Fake(f16, (5, 2, 128)), c, s)              # no batch dimension
    with pytest.raises(ValueError, match=r"\[T, 64\]"):                              # a cos of the wrong length
        rope_qk(q, k, _Fake(f32, (6, 64)), s)
    with pytest.raises(ValueError, match=r"\[T, 64\]"):
        rope_qk(q, k, c, _Fake(f32, (5, 1, 64)))
    with pytest.raises(ValueError, match="k "):
        rope_qk(q, _Fake(f16, (1, 6, 2, 128)), c, s)
    with pytest.raises(ValueError, match="heads"):
        rope_qk(_Fake(f16, (1, 5, 257, 128)), k, c, s)


# ---- the pinned arithmetic, restated in numpy, against finetune._rope and its autograd
def pinned_rope(x, cos, sin, inverse=False):
    """x fp16 [..., T, heads, 128], cos / sin fp32 [T, 64]: every product a float32 of its own, their sum a float32, that value
    converted to fp16 (numpy rounds to nearest even).  inverse: the transpose, and + (+0) in fp16 at the end: autograd sums the
    gradients of the two half-slices of x, each padded with +0, so a -0 never leaves the torch route (everything else is unchanged
    by that add)."""
    f = np.float32
    a, b = x[..., :64].astype(f), x[..., 64:].astype(f)
    c, s = cos.astype(f)[:, None, :], sin.astype(f)[:, None, :]
    ac, bs, bc, as_ = (a * c).astype(f), (b * s).astype(f), (b * c).astype(f), (a * s).astype(f)
    lo, hi = (ac + bs if inverse else ac - bs).astype(f), (bc - as_ if inverse else bc + as_).astype(f)
    with np.errstate(over="ignore"):
        out = np.concatenate([lo, hi], -1).astype(np.float16)
    return out + np.float16(0.0) if inverse else out


def fma_rope(x, cos, sin):
    """What a contracted kernel would give: the difference formed exactly (fp64 holds both products) and rounded to fp32 once."""
    d = np.float64
    a, b = x[..., :64].astype(d), x[..., 64:].astype(d)
    c, s = cos.astype(d)[:, None, :], sin.astype(d)[:, None, :]
    bs, as_ = (b * s).astype(np.float32).astype(d), (a * s).astype(np.float32).astype(d)
    with np.errstate(over="ignore"):
        return np.concatenate([(a * c - bs).astype(np.float32), (b * c + as_).astype(np.float32)], -1).astype(np.float16)


def special_data(rng, shape):
    """N(0, 1) * 3 with +-65504 (an infinite result must equal an infinite result), fp16 subnormals and zeros mixed in."""
    x = (rng.standard_normal(shape) * 3).astype(np.float16)
    flat = x.reshape(-1)
    idx = rng.permutation(flat.size)[:flat.size // 8]
    vals = np.array([65504, -65504, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -15, -(2.0 ** -20), 0.0, -0.0, 30000, -30000], dtype=np.float16)
    flat[idx] = vals[np.arange(idx.size) % vals.size]
    return x


def rope_tables(T, rng=None):
    """The model's table (base 10000, as llama.QuantLlama builds it), or a random one in [-1, 1]."""
    if rng is not None:
        return rng.uniform(-1, 1, (T, 64)).astype(np.float32), rng.uniform(-1, 1, (T, 64)).astype(np.float32)
    from qeft_amd import qeft_cuda
    cos, sin = qeft_cuda.rope_cos_sin(10000.0, 64, T)
    return cos.numpy(), sin.numpy()


@pytest.mark.parametrize("table", ["model", "random"])
def test_the_pinned_arithmetic_is_the_torch_expression_bit_for_bit(table):
    import torch
    from qeft_amd import finetune
    rng = np.random.default_rng(11 if table == "model" else 12)
    B, T, H = 2, 67, 5
    cos, sin = rope_tables(T, None if table == "model" else rng)
    x, g = special_data(rng, (B, T, H, 128)), special_data(rng, (B, T, H, 128))
    bits = lambda a: np.ascontiguousarray(a).view(np.int16)
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    ct, st = torch.from_numpy(cos)[:, None, :], torch.from_numpy(sin)[:, None, :]
    out = finetune._rope(xt, ct, st)
    out.backward(torch.from_numpy(g.copy()))
    want_fwd, want_bwd = out.detach().numpy(), xt.grad.numpy()
    assert np.isinf(want_fwd).any() and np.isinf(want_bwd).any() and not np.isnan(want_fwd).any() and not np.isnan(want_bwd).any()
    got_fwd, got_bwd = pinned_rope(x, cos, sin), pinned_rope(g, cos, sin, inverse=True)
    assert np.array_equal(bits(got_fwd), bits(want_fwd))
    assert np.array_equal(bits(got_bwd), bits(want_bwd))
    neg = pinned_rope(g, cos, -sin)                          # the inverse is the forward on -sin, exactly, but for -0 -> +0
    differ = bits(neg) != bits(got_bwd)
    assert differ.any() and (bits(neg)[differ] == np.int16(-32768)).all() and (bits(got_bwd)[differ] == 0).all()
    assert np.array_equal(bits(neg + np.float16(0.0)), bits(got_bwd))
    # and the test can tell: a contracted form differs from both in a few of 10^5 values
    share = (bits(fma_rope(x, cos, sin)) != bits(want_fwd)).mean()
    print(f"[train_rope] cpu {table} table: pinned form == torch in {want_fwd.size} values, both directions; an FMA form differs in {share:.2e}")
    assert 0 < share < 1e-3
