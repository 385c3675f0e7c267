"""CPU-only checks of the verify pass over the e4m3 KV cache (csrc/decode_verify_kv8.hip, include/qeft_hip.h): the two entries are
declared and exported and reject bad arguments without a GPU, the workspace layout, the kernel compiles without spills or scratch,
and DecodeEngine._verify_unsupported honours the kv8_verify flag."""
import os
import re
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qeft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-kernarg-preload-count=16", "-S",
         "--cuda-device-only"]                      # qeft_amd/build.py's, as tests/test_isa_guards.py
NEW = ["qeft_attn_m_kv8_workspace_bytes", "qeft_rope_attn_decode_m_kv8"]
ERR_BATCH, ERR_SHAPE, ERR_NULL, ERR_ALIGN = 1, 2, 4, 6
P = 16          # a non-NULL, aligned dummy pointer: never dereferenced -- EVERY call below must fail validation
MIS = 18        # misaligned


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name


def _attn(lib, m=4, heads=4, kv=4, max_seq=64, split=1, tab_rows=None, kc=P, vc=P, ks=P, vs=P, pos=P, ws=P, out_stride=512, q=P):
    return lib.qeft_rope_attn_decode_m_kv8(q, P, P, 1536, P, P, 128, m if tab_rows is None else tab_rows, kc, vc, ks, vs, pos, None, P,
                                           out_stride, ws, split, heads, kv, max_seq, m, None)


def test_arguments_rejected_before_the_device(lib):
    for m in (0, 9):
        assert _attn(lib, m=m) == ERR_BATCH
        assert _attn(lib, m=m, split=3, ks=None) == ERR_BATCH       # the order of precedence: batch, shape, null, alignment
    assert _attn(lib, split=3) == ERR_SHAPE
    assert _attn(lib, split=3, ks=None) == ERR_SHAPE
    assert _attn(lib, max_seq=24) == ERR_SHAPE
    assert _attn(lib, max_seq=32784) == ERR_SHAPE
    assert _attn(lib, heads=6, kv=4) == ERR_SHAPE
    assert _attn(lib, tab_rows=5) == ERR_SHAPE
    assert _attn(lib, out_stride=256) == ERR_SHAPE
    for name in ("ks", "vs", "kc", "vc", "pos", "q"):
        assert _attn(lib, **{name: None}) == ERR_NULL, name
    assert _attn(lib, ks=None, kc=MIS) == ERR_NULL
    assert _attn(lib, ks=17) == ERR_ALIGN                            # scales at an odd address
    assert _attn(lib, vs=18) == ERR_ALIGN
    assert _attn(lib, kc=MIS) == ERR_ALIGN
    assert _attn(lib, vc=MIS) == ERR_ALIGN
    for split in (2, 4, 8):
        assert _attn(lib, split=split, ws=None) == ERR_NULL
    assert _attn(lib, split=4, ws=MIS) == ERR_ALIGN


def test_workspace_bytes(lib):
    f = lib.qeft_attn_m_kv8_workspace_bytes
    for m in (0, 9):
        assert f(32, 4, m) == 0
    for m in range(1, 9):
        assert f(32, 1, m) == 0
    for heads in (4, 32, 64):
        for m in range(1, 9):
            assert 0 < f(heads, 2, m) < f(heads, 4, m) < f(heads, 8, m), (heads, m)             # monotone in S
            if m > 1:
                assert all(f(heads, s, m) > f(heads, s, m - 1) for s in (2, 4, 8)), (heads, m)  # and in m
        # one record per (head, row, split) behind a counter area that does not depend on (m, S)
        rec = (f(heads, 2, 2) - f(heads, 2, 1)) // (heads * 2)      # bytes of a record
        assert rec >= 130 * 4
        fronts = {f(heads, s, m) - heads * m * s * rec for m in range(1, 9) for s in (2, 4, 8)}
        assert len(fronts) == 1 and fronts.pop() >= 4 * heads, heads
        assert f(heads, 8, 8) == lib.qeft_attn_m_workspace_bytes(heads, 8, 8)     # one layout with the fp16 m-row kernel


def _ns(**kw):
    from qeft_amd.llama import DecodeEngine
    ns = types.SimpleNamespace(**{**dict(tp=False, tp3=False, bits=4, v3=True), **kw})
    ns._m_row_unsupported = lambda: DecodeEngine._m_row_unsupported(ns)
    return DecodeEngine._verify_unsupported(ns)


def test_verify_unsupported_reads_the_flag():
    assert _ns(kv_dtype="fp8", kv8_verify=True) is None
    for why in (_ns(kv_dtype="fp8"), _ns(kv_dtype="fp8", kv8_verify=False)):
        assert why and "fp8" in why and "KV cache" in why
        assert "kv8_verify" in why                                   # the refusal names the way out
    assert "4-bit" in _ns(kv_dtype="fp8", kv8_verify=True, bits=3)
    assert _ns(kv_dtype="fp16", kv8_verify=True) is None
    assert _ns(kv_dtype="fp16") is None


def test_constructor_takes_the_flag():
    import inspect
    from qeft_amd.llama import DecodeEngine
    p = inspect.signature(DecodeEngine.__init__).parameters
    assert "kv8_verify" in p and p["kv8_verify"].default is False


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_compiles_without_spills_or_scratch(tmp_path):
    """tests/test_isa_guards.py, item 2, for the new file: the metadata of every instantiation."""
    out = tmp_path / "verify_kv8.s"
    subprocess.run([HIPCC, *FLAGS, "-o", str(out), os.path.join(CSRC, "decode_verify_kv8.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = out.read_text()
    names = set(re.findall(r"\.name:\s+(_ZN4qeft22rope_attn_m_kv8_kernel\w+)", text))
    assert len(names) >= 4, names
    for n in names:
        blk = text[text.index(".name:           " + n):][:1200]     # the fields follow the name within one kernel's entry
        md = {k: int(v) for k, v in re.findall(r"\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", blk)}
        assert {"vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"} <= set(md), (n, md)
        assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, (n, md)
