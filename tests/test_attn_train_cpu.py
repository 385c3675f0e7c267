"""CPU checks of the training attention's boundary (csrc/attn_train.hip): the entries are declared and
exported, they refuse bad arguments in the documented order before any HIP call, the workspace size is 0 for what they refuse, the
host-side enumerations of every address the forward and the three backward launches form find none outside its operand over the
sweep of lengths, batch sizes, head layouts and strides, and finetune.causal_lm_loss refuses a bad `attn` or head split before any
launch.  The two enumerations take the geometry alone (as qeft_attn_prefill_check_extents), not operand sizes, so there is no
"one row shorter" case here."""
import itertools
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["qeft_attn_train_fwd", "qeft_attn_train_check_extents", "qeft_attn_train_bwd_workspace_bytes", "qeft_attn_train_bwd",
       "qeft_attn_train_bwd_check_extents"]
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6
P = 1 << 20                       # a 16-byte aligned non-null "pointer": no entry below gets as far as using it


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
    import qeft_amd
    assert "causal_attention" in qeft_amd.__all__


def _fwd(lib, q=P, k=P, v=P, out=P, lse=P, q_stride=4096, kv_stride=4096, out_stride=4096, n_seq=1, t=16, heads=32, kv=32):
    return lib.qeft_attn_train_fwd(q, q_stride, k, v, kv_stride, out, out_stride, lse, n_seq, t, heads, kv, None)


def _bwd(lib, ptr=None, strides=None, ws_bytes=None, n_seq=1, t=16, heads=32, kv=32):
    """ptr: overrides of the ten pointers by name; strides: overrides of the six strides by name."""
    p = dict(q=P, k=P, v=P, out=P, dout=P, lse=P, dq=P, dk=P, dv=P, ws=P)
    p.update(ptr or {})
    s = dict(q=heads * 128, kv=kv * 128, out=heads * 128, dout=heads * 128, dq=heads * 128, dkv=kv * 128)
    s.update(strides or {})
    if ws_bytes is None:
        ws_bytes = 4 * max(n_seq, 0) * max(t, 0) * heads
    return lib.qeft_attn_train_bwd(p["q"], s["q"], p["k"], p["v"], s["kv"], p["out"], s["out"], p["dout"], s["dout"], p["lse"],
                                   p["dq"], s["dq"], p["dk"], p["dv"], s["dkv"], p["ws"], ws_bytes, n_seq, t, heads, kv, None)


def test_forward_refuses_in_order_without_a_gpu(lib):
    """QEFT_ERR_SHAPE first, with every pointer null and misaligned: no pointer is looked at; then NULL; then ALIGN."""
    for bad in (dict(t=0), dict(t=-3), dict(n_seq=0), dict(n_seq=-1), dict(n_seq=1025, t=1024), dict(n_seq=2 ** 20, t=2 ** 20),
                dict(heads=32, kv=5), dict(heads=32, kv=0), dict(heads=0, kv=0), dict(q_stride=4100), dict(q_stride=4088),
                dict(out_stride=4100), dict(out_stride=2048), dict(kv_stride=4100), dict(kv_stride=1024),
                dict(heads=64, kv=8, q_stride=8192, out_stride=8192, kv_stride=1016)):
        assert _fwd(lib, **bad) == ERR_SHAPE, bad
        assert _fwd(lib, q=None, k=3, v=None, out=5, lse=1, **bad) == ERR_SHAPE, bad
    assert _fwd(lib, n_seq=1024, t=1024, q=None) == ERR_NULL            # 2^20 rows are taken
    for name in ("q", "k", "v", "out", "lse"):
        assert _fwd(lib, **{name: None}) == ERR_NULL, name
        assert _fwd(lib, **{name: None, "q" if name != "q" else "k": P + 2}) == ERR_NULL, name      # NULL before ALIGN
    for name in ("q", "k", "v", "out"):
        assert _fwd(lib, **{name: P + 8}) == ERR_ALIGN, name
    assert _fwd(lib, lse=P + 2) == ERR_ALIGN and _fwd(lib, lse=P + 1) == ERR_ALIGN


def test_backward_refuses_in_order_without_a_gpu(lib):
    nul = dict(q=None, k=None, v=None, out=None, dout=None, lse=None, dq=None, dk=None, dv=None, ws=None)
    odd = {k_: 3 for k_ in nul}
    shapes = [dict(t=0), dict(n_seq=0), dict(n_seq=1025, t=1024), dict(heads=32, kv=5), dict(heads=32, kv=0)]
    for bad in shapes:
        for ptr in (None, nul, odd):
            assert _bwd(lib, ptr=ptr, **bad) == ERR_SHAPE, (bad, ptr)
    for name, width in (("q", 4096), ("kv", 4096), ("out", 4096), ("dout", 4096), ("dq", 4096), ("dkv", 4096)):
        for stride in (width + 4, width - 8):
            for ptr in (None, nul, odd):
                assert _bwd(lib, ptr=ptr, strides={name: stride}) == ERR_SHAPE, (name, stride)
    need = lib.qeft_attn_train_bwd_workspace_bytes(1, 16, 32, 32)
    assert need == 4 * 16 * 32
    for ptr in (None, nul, odd):
        assert _bwd(lib, ptr=ptr, ws_bytes=need - 1) == ERR_SHAPE           # a short workspace is a shape error
    for name in nul:
        assert _bwd(lib, ptr={name: None}) == ERR_NULL, name
        other = "q" if name != "q" else "k"
        assert _bwd(lib, ptr={name: None, other: P + 2}) == ERR_NULL, name      # NULL before ALIGN
    for name in nul:
        assert _bwd(lib, ptr={name: P + (2 if name == "lse" else 8)}) == ERR_ALIGN, name


def test_workspace_bytes(lib):
    f = lib.qeft_attn_train_bwd_workspace_bytes
    assert f(3, 200, 64, 8) == 4 * 3 * 200 * 64
    assert f(1024, 1024, 32, 32) == 4 * 2 ** 20 * 32
    for bad in ((0, 16, 32, 32), (1, 0, 32, 32), (-1, 16, 32, 32), (1025, 1024, 32, 32), (1, 16, 32, 5), (1, 16, 32, 0), (1, 16, 0, 0),
                (1, 16, -32, -32)):
        assert f(*bad) == 0, bad


LENGTHS = (1, 7, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 513)
LAYOUTS = ((2, 2), (8, 1), (8, 2), (64, 8))


def test_no_address_outside_its_operand(lib):
    """Both enumerations over the sweep, with every stride at its minimum and padded (q, k, v as views of one fused buffer; the
    gradients in padded rows of their own)."""
    fwd, bwd = lib.qeft_attn_train_check_extents, lib.qeft_attn_train_bwd_check_extents
    n = 0
    for t, n_seq, (heads, kv) in itertools.product(LENGTHS, (1, 3), LAYOUTS):
        hw, kw, fused = heads * 128, kv * 128, (heads + 2 * kv) * 128
        for pad in (False, True):
            qs, ks, os_ = (fused, fused, hw + 64) if pad else (hw, kw, hw)
            assert fwd(qs, ks, os_, n_seq, t, heads, kv) == 0, (t, n_seq, heads, kv, pad)
            ds, dqs, dkvs = (hw + 8, fused, fused) if pad else (hw, hw, kw)
            assert bwd(qs, ks, os_, ds, dqs, dkvs, n_seq, t, heads, kv) == 0, (t, n_seq, heads, kv, pad)
            n += 1
    assert n == len(LENGTHS) * 2 * len(LAYOUTS) * 2


def test_the_enumerations_refuse_what_the_entries_refuse(lib):
    fwd, bwd = lib.qeft_attn_train_check_extents, lib.qeft_attn_train_bwd_check_extents
    assert fwd(4096, 4096, 4096, 1, 0, 32, 32) == -1 and fwd(4096, 4096, 4096, 0, 5, 32, 32) == -1
    assert fwd(4096, 4088, 4096, 1, 5, 32, 32) == -1 and fwd(4096, 4096, 4096, 1, 5, 32, 5) == -1
    assert bwd(4096, 4096, 4096, 4096, 4096, 4096, 1, 0, 32, 32) == -1
    assert bwd(4096, 4096, 4096, 4100, 4096, 4096, 1, 5, 32, 32) == -1
    assert bwd(4096, 4096, 4096, 4096, 4096, 1024, 1, 5, 32, 32) == -1


def test_causal_lm_loss_refuses_a_bad_attn_or_head_split_before_any_launch():
    """Both raise before the model's weights, the tokens or the library are looked at: a bare shape is all the 'model' has."""
    from qeft_amd import finetune
    from qeft_amd.llama import LlamaShape
    model = types.SimpleNamespace(shape=LlamaShape(512, 512, 2, 4, 2, 512, max_seq=256))
    with pytest.raises(ValueError, match="attn"):
        finetune.causal_lm_loss(model, None, attn="bogus")
    with pytest.raises(ValueError, match="attn"):
        finetune.causal_lm_loss(model, None, attn=None)
    for shape in (LlamaShape(768, 512, 2, 6, 4, 512), LlamaShape(512, 512, 2, 8, 2, 512)):       # 6 % 4; heads of 64
        with pytest.raises(ValueError, match="heads"):
            finetune.causal_lm_loss(types.SimpleNamespace(shape=shape), None, attn="own")


def test_causal_attention_refuses_bad_shapes_on_the_cpu():
    import torch
    from qeft_amd.attention import causal_attention
    q = torch.zeros(1, 4, 6, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="multiple"):
        causal_attention(q, torch.zeros(1, 4, 4, 128, dtype=torch.float16), torch.zeros(1, 4, 4, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="head size"):
        causal_attention(torch.zeros(1, 4, 6, 64, dtype=torch.float16), torch.zeros(1, 4, 2, 64, dtype=torch.float16),
                         torch.zeros(1, 4, 2, 64, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="GPU"):
        causal_attention(q, torch.zeros(1, 4, 2, 128, dtype=torch.float16), torch.zeros(1, 4, 2, 128, dtype=torch.float16))
