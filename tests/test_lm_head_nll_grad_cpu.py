"""CPU checks of the fused head's backward entry (csrc/lm_head_nll_grad.hip) and of finetune.shift_labels: the four entries are
declared, exported and bound and the Python names resolve; the entry refuses bad arguments before any HIP call, SHAPE before NULL
before ALIGN; the workspace stops growing at the chunk size; the host-side enumeration of every address the launches of every
chunk form finds none outside its operand over the sweep of rows, widths, vocabularies and strides."""
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["qeft_lm_head_nll_grad_chunk_rows", "qeft_lm_head_nll_grad_workspace_bytes", "qeft_lm_head_nll_grad",
       "qeft_lm_head_nll_grad_check_extents"]
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_symbols_declared_exported_and_bound(lib):
    from qeft_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/qeft_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    assert lib.qeft_abi_version() == 1
    assert "lm_head_nll_grad.hip" in build.SOURCES and "lm_head_nll_body.h" in build.HEADERS
    import qeft_amd
    from qeft_amd import finetune, scoring
    assert qeft_amd.lm_head_nll_loss is scoring.lm_head_nll_loss
    assert qeft_amd.causal_lm_loss is finetune.causal_lm_loss and qeft_amd.shift_labels is finetune.shift_labels
    assert callable(finetune.begin) and callable(finetune.end)


def test_entry_refuses_bad_arguments_without_a_gpu(lib):
    """Validation happens before any HIP call: SHAPE before any pointer is looked at, then NULL, then ALIGN."""
    P = 1 << 20
    e = lib.qeft_lm_head_nll_grad
    big = 1 << 40

    def call(x=P, x_stride=256, w=P, targets=P, lse=P, grad=P, dx=P, dx_stride=256, fp32=0, ws=P, ws_bytes=big, t=16, hidden=256,
             vocab=512):
        return e(x, x_stride, w, targets, lse, grad, dx, dx_stride, fp32, ws, ws_bytes, t, hidden, vocab, None)
    assert call(t=0) == ERR_SHAPE and call(t=-3) == ERR_SHAPE and call(vocab=0) == ERR_SHAPE
    assert call(hidden=96, x_stride=96, dx_stride=96) == ERR_SHAPE and call(hidden=32, x_stride=32, dx_stride=32) == ERR_SHAPE
    assert call(x_stride=248) == ERR_SHAPE and call(x_stride=260) == ERR_SHAPE
    assert call(dx_stride=248) == ERR_SHAPE and call(dx_stride=260) == ERR_SHAPE    # narrower than hidden / not a multiple of 8
    need = lib.qeft_lm_head_nll_grad_workspace_bytes(16, 256, 512)
    assert need == 2 * 16 * 512
    assert call(x=None, ws_bytes=need) == ERR_NULL                                   # exactly enough passes the shape check
    assert call(ws_bytes=need - 1) == ERR_SHAPE and call(ws_bytes=0) == ERR_SHAPE
    # SHAPE wins over NULL and ALIGN
    assert call(x=None, t=0) == ERR_SHAPE and call(dx=P + 2, dx_stride=260) == ERR_SHAPE and call(ws=None, ws_bytes=need - 1) == ERR_SHAPE
    # NULL wins over ALIGN; targets is required here
    for kw in ("x", "w", "targets", "lse", "grad", "dx", "ws"):
        assert call(**{kw: None}) == ERR_NULL, kw
        assert call(**{kw: None}, fp32=1) == ERR_NULL, kw
    assert call(targets=None, w=P + 2) == ERR_NULL
    for kw in ("x", "w", "dx", "ws"):
        assert call(**{kw: P + 8}) == ERR_ALIGN, kw
    for kw in ("targets", "lse", "grad"):
        assert call(**{kw: P + 2}) == ERR_ALIGN, kw


def test_workspace_stops_growing_at_the_chunk(lib):
    f, R = lib.qeft_lm_head_nll_grad_workspace_bytes, lib.qeft_lm_head_nll_grad_chunk_rows(4096, 32000)
    assert R >= 128 and lib.qeft_lm_head_nll_grad_chunk_rows(64, 1) >= 128
    for hidden, vocab in ((64, 1), (256, 512), (4096, 32000), (8192, 4097)):
        col = [f(t, hidden, vocab) for t in (1, 7, 64, 65, 200, R - 1, R)]
        assert col[0] > 0 and col == sorted(col) and len(set(col)) == len(col)
        assert f(R, hidden, vocab) == f(2 * R, hidden, vocab) == f(8 * R, hidden, vocab)
        assert f(R, hidden, vocab) >= 2 * R * vocab                                   # R rows of fp16 g
    assert f(0, 256, 512) == 0 and f(-1, 256, 512) == 0 and f(16, 96, 512) == 0 and f(16, 256, 0) == 0 and f(16, 0, 512) == 0


def test_no_address_outside_its_operand(lib):
    f, R = lib.qeft_lm_head_nll_grad_check_extents, lib.qeft_lm_head_nll_grad_chunk_rows(4096, 32000)
    n = 0
    for t, hidden, vocab in itertools.product((1, 7, 63, 64, 65, 127, 128, 129, 200, R - 1, R, R + 1, 2 * R + 5),
                                              (64, 256, 4096, 5120, 8192), (1, 9, 127, 128, 129, 4097, 32000)):
        for x_stride, dx_stride in ((hidden, hidden), (hidden + 8, hidden + 16), (3 * hidden, 2 * hidden)):
            assert f(x_stride, dx_stride, t, hidden, vocab) == 0, (t, hidden, vocab, x_stride, dx_stride)
            n += 1
    assert n == 13 * 5 * 7 * 3
    assert f(256, 256, 0, 256, 512) == -1 and f(96, 96, 4, 96, 512) == -1 and f(248, 256, 4, 256, 512) == -1
    assert f(256, 248, 4, 256, 512) == -1 and f(256, 260, 4, 256, 512) == -1 and f(256, 256, 4, 256, 0) == -1


def test_shift_labels():
    from qeft_amd.finetune import IGNORE_INDEX, shift_labels
    assert IGNORE_INDEX == -100
    tok = torch.tensor([5, 6, 7, 8])
    out = shift_labels(tok)
    assert out.dtype == torch.int32 and out.tolist() == [6, 7, 8, -100]
    assert shift_labels(tok, torch.tensor([-100, -100, 7, 8])).tolist() == [-100, 7, 8, -100]
    batch = torch.tensor([[1, 2, 3], [4, 5, 0]])
    assert shift_labels(batch).tolist() == [[2, 3, -100], [5, 0, -100]]                # no label crosses a sequence's end
    assert shift_labels(batch, torch.tensor([[1, 2, 3], [4, 5, -100]])).tolist() == [[2, 3, -100], [5, -100, -100]]
    assert shift_labels(torch.tensor([9])).tolist() == [-100]
    with pytest.raises(ValueError):
        shift_labels(tok, torch.tensor([1, 2, 3]))
