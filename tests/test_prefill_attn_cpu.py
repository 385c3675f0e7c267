"""CPU checks of the prompt attention's boundary (csrc/prefill_attn.hip): the two entries are declared and exported, the host-side
enumeration of every address a launch forms finds none outside its operand over the sweep of starts, chunk lengths, cache sizes,
head layouts and q strides, the entry refuses bad arguments before any HIP call, and the e4m3 decoder behind the transient fp16
image of an FP8 cache agrees with tests/kv8_ref.py on all 256 codes."""
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["qeft_attn_prefill", "qeft_attn_prefill_check_extents"]
ERR_SHAPE = 2


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
    f = lib.qeft_attn_prefill_check_extents
    n = 0
    for start, t in itertools.product((0, 1, 63, 64, 65, 1000), (1, 7, 63, 64, 65, 129)):
        for kv_rows in sorted({start + t, (start + t + 15) // 16 * 16, 4096}):
            for heads, kv in ((32, 32), (64, 8), (32, 1)):
                for q_stride in (heads * 128, (heads + 2 * kv) * 128):
                    assert f(q_stride, kv_rows, heads * 128, start, t, heads, kv) == 0, (start, t, kv_rows, heads, kv, q_stride)
                    n += 1
    assert n >= 6 * 6 * 2 * 3 * 2


def test_the_enumeration_refuses_what_the_entry_refuses(lib):
    """A context that ends at the cache's last row is walked (and clean); one row more is no launch: -1, as from the entry."""
    f = lib.qeft_attn_prefill_check_extents
    assert f(4096, 64, 4096, 0, 64, 32, 32) == 0
    assert f(4096, 64, 4096, 0, 65, 32, 32) == -1         # refused by the entry: start + t > kv_rows
    assert f(4096, 0, 4096, 0, 1, 32, 32) == -1


def test_entry_refuses_bad_arguments_without_a_gpu(lib):
    """Validation happens before any HIP call and before any pointer is looked at."""
    P = 1 << 20
    e = lib.qeft_attn_prefill

    def call(q_stride=4096, kv_rows=256, out_stride=4096, start=0, t=16, heads=32, kv=32):
        return e(P, q_stride, P, P, kv_rows, P, out_stride, start, t, heads, kv, None)
    assert call(t=0) == ERR_SHAPE and call(t=-3) == ERR_SHAPE
    assert call(start=-1) == ERR_SHAPE
    assert call(start=250, t=7) == ERR_SHAPE and call(start=0, t=257) == ERR_SHAPE and call(start=2 ** 31 - 1, t=2) == ERR_SHAPE
    assert call(heads=32, kv=5) == ERR_SHAPE and call(heads=32, kv=0) == ERR_SHAPE
    assert call(q_stride=4100) == ERR_SHAPE and call(q_stride=4088) == ERR_SHAPE          # not a multiple of 8 / narrower than the heads
    assert call(out_stride=4100) == ERR_SHAPE and call(out_stride=2048) == ERR_SHAPE
    assert e(None, 4096, P, P, 256, P, 4096, 0, 16, 32, 32, None) == 4                     # NULL
    assert e(P + 2, 4096, P, P, 256, P, 4096, 0, 16, 32, 32, None) == 6                    # alignment


def test_e4m3_decoder_matches_the_reference_on_all_codes():
    import kv8_ref
    from qeft_amd.llama import kv8_decode_rows
    codes = torch.arange(256, dtype=torch.uint8).view(2, 1, 128)
    for scale in (1.0, 0.0371, 3.0e-5, 517.0):
        scales = torch.full((2, 1), scale, dtype=torch.float32)
        got = kv8_decode_rows(codes, scales)
        want = kv8_ref.dequant_rows(codes, scales).half()            # code x row scale in fp32, rounded to fp16
        assert got.dtype == torch.float16 and torch.equal(got.view(torch.int16)[~torch.isnan(want)], want.view(torch.int16)[~torch.isnan(want)])
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(want).sum()) == 2     # 0x7f and 0xff
