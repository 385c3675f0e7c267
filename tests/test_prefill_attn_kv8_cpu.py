"""CPU checks of the boundary of the prompt attention over an e4m3 cache (csrc/prefill_attn_kv8.hip): the two entries are declared
and exported, the host-side enumeration of every address a launch forms -- over q, out, both code arrays, both scale arrays and
both new-row arrays -- finds none outside its operand over the sweep of starts, chunk lengths, cache sizes, head layouts and
strides, and the entry refuses bad arguments before any HIP call: shape first, then NULL, then alignment, each of the eight
pointers tried."""
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["qeft_attn_prefill_kv8", "qeft_attn_prefill_kv8_check_extents"]
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6


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
    assert lib.qeft_abi_version() == 1


def test_no_address_outside_its_operand(lib):
    f = lib.qeft_attn_prefill_kv8_check_extents
    n = 0
    for start, t in itertools.product((0, 1, 63, 64, 65, 1000), (1, 7, 63, 64, 65, 129)):
        for kv_rows in sorted({start + t, (start + t + 15) // 16 * 16, 4096}):
            for heads, kv in ((32, 32), (64, 8), (32, 1)):
                for q_stride in (heads * 128, (heads + 2 * kv) * 128):
                    for new_stride in (kv * 128, (heads + 2 * kv) * 128):
                        got = f(q_stride, kv_rows, new_stride, heads * 128, start, t, heads, kv)
                        assert got == 0, (start, t, kv_rows, heads, kv, q_stride, new_stride, got)
                        n += 1
    assert n >= 6 * 6 * 2 * 3 * 2 * 2


def test_the_enumeration_refuses_what_the_entry_refuses(lib):
    """A context that ends at the cache's last row is walked (and clean); one row more is no launch: -1, as from the entry."""
    f = lib.qeft_attn_prefill_kv8_check_extents
    assert f(4096, 64, 4096, 4096, 0, 64, 32, 32) == 0
    assert f(4096, 64, 4096, 4096, 30, 34, 32, 32) == 0
    assert f(4096, 64, 4096, 4096, 0, 65, 32, 32) == -1          # start + t > kv_rows
    assert f(4096, 64, 4096, 4096, 30, 35, 32, 32) == -1
    assert f(4096, 0, 4096, 4096, 0, 1, 32, 32) == -1            # kv_rows = 0
    assert f(8192, 64, 1016, 8192, 0, 8, 64, 8) == -1            # new rows narrower than the kv heads
    assert f(8192, 64, 1024, 8192, 0, 8, 64, 8) == 0
    assert f(8192, 64, 1028, 8192, 0, 8, 64, 8) == -1            # not a multiple of 8


def test_entry_refuses_bad_arguments_without_a_gpu(lib):
    """Validation happens before any HIP call and before any pointer is looked at."""
    P = 1 << 20
    e = lib.qeft_attn_prefill_kv8

    def call(q_stride=4096, kv_rows=256, new_stride=4096, out_stride=4096, start=0, t=16, heads=32, kv=32, ptrs=(P,) * 8):
        q, kc, vc, ks, vs, kn, vn, out = ptrs
        return e(q, q_stride, kc, vc, ks, vs, kv_rows, kn, vn, new_stride, out, out_stride, start, t, heads, kv, None)
    assert call(t=0) == ERR_SHAPE and call(t=-3) == ERR_SHAPE
    assert call(start=-1) == ERR_SHAPE
    assert call(start=250, t=7) == ERR_SHAPE and call(start=0, t=257) == ERR_SHAPE and call(start=2 ** 31 - 1, t=2) == ERR_SHAPE
    assert call(kv_rows=0) == ERR_SHAPE
    assert call(heads=32, kv=5) == ERR_SHAPE and call(heads=32, kv=0) == ERR_SHAPE
    assert call(q_stride=4100) == ERR_SHAPE and call(q_stride=4088) == ERR_SHAPE          # not a multiple of 8 / narrower than the heads
    assert call(out_stride=4100) == ERR_SHAPE and call(out_stride=2048) == ERR_SHAPE
    assert call(new_stride=4100) == ERR_SHAPE and call(new_stride=4088) == ERR_SHAPE
    assert call(heads=64, kv=8, q_stride=8192, out_stride=8192, new_stride=1016) == ERR_SHAPE
    assert call(ptrs=(None,) * 8, t=0) == ERR_SHAPE               # the shape comes first
    for i in range(8):
        null = tuple(None if j == i else P for j in range(8))
        assert call(ptrs=null) == ERR_NULL, i
        off = 2 if i in (3, 4) else 8                             # scales: 4-byte alignment; everything else: 16
        bad = tuple(P + off if j == i else P for j in range(8))
        assert call(ptrs=bad) == ERR_ALIGN, i
        assert call(ptrs=tuple(None if j == i else P + 2 for j in range(8))) == ERR_NULL, i      # NULL before alignment
    assert call(ptrs=(P, P, P, P + 4, P + 12, P, P, P), t=0) == ERR_SHAPE
