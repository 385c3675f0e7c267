"""qeft_rope_attn_decode_long / qeft_attn_long_workspace_bytes without a GPU: declared and exported with the parameter list of
qeft_rope_attn_decode; refusals in the documented order -- SHAPE whatever the pointers are, then NULL, then ALIGN -- before any
HIP call.  As in tests/test_train_rope_cpu.py, no call has every argument in order: made-up addresses reach refusals only."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6
P = 1 << 20                       # a 16-byte aligned non-null "pointer": no call below gets as far as using it
PTRS = ("q", "k", "v", "cos_tab", "sin_tab", "k_cache", "v_cache", "pos", "out", "workspace")


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _entry(lib, tab_rows=1, n_split=2, n_heads=8, n_kv_heads=2, max_seq=65536, **ptr):
    a = {name: ptr.get(name, P) for name in PTRS}
    return lib.qeft_rope_attn_decode_long(a["q"], a["k"], a["v"], a["cos_tab"], a["sin_tab"], tab_rows, a["k_cache"], a["v_cache"],
                                          a["pos"], None, a["out"], a["workspace"], n_split, n_heads, n_kv_heads, max_seq, None)


def test_symbols_declared_and_exported(lib):
    from qeft_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    for name in ("qeft_rope_attn_decode_long", "qeft_attn_long_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name), name
    assert _lib.SIGNATURES["qeft_rope_attn_decode_long"] == _lib.SIGNATURES["qeft_rope_attn_decode"]


BAD_SHAPES = [dict(max_seq=0), dict(max_seq=8), dict(max_seq=1048576 + 16), dict(max_seq=32776), dict(n_split=3), dict(n_split=128),
              dict(n_split=0), dict(n_heads=8, n_kv_heads=3), dict(n_heads=0), dict(n_kv_heads=0), dict(tab_rows=65535)]


@pytest.mark.parametrize("bad", BAD_SHAPES, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_shapes_are_refused_first(lib, bad):
    for ptrs in ({}, {n: None for n in PTRS}, {n: P + 2 for n in PTRS}):
        assert _entry(lib, **bad, **ptrs) == ERR_SHAPE


def test_null_then_align(lib):
    for name in PTRS:
        assert _entry(lib, **{name: None}, **{n: P + 2 for n in PTRS if n != name}) == ERR_NULL, name
    for name in ("k_cache", "v_cache", "workspace"):
        assert _entry(lib, **{name: P + 8}) == ERR_ALIGN, name
    assert _entry(lib, n_split=1, workspace=None, k_cache=P + 8) == ERR_ALIGN      # one split needs no workspace


def test_workspace_grows_with_heads_and_splits(lib):
    w = lib.qeft_attn_long_workspace_bytes
    assert [w(8, s) for s in (3, 128, 0)] == [0, 0, 0] and w(0, 2) == 0 and w(8, 1) == 0
    sizes = [w(8, s) for s in (2, 4, 8, 16, 32, 64)]
    assert sizes == sorted(set(sizes)) and sizes[0] > 0 and w(64, 64) > w(8, 64) >= (8 * 64 * 130 + 8) * 4
