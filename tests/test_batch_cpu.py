"""CPU-only checks of batched decoding (qeft_amd/batch.py, csrc/decode_batch.hip): the C ABI's new entries are declared and
exported and reject bad arguments without a GPU, the new kernels compile without scratch, and the host's slot bookkeeping and
admission rules hold."""
import os
import re
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qeft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ["qeft_token_begin_norm_batch", "qeft_attn_batch_workspace_bytes", "qeft_rope_attn_decode_batch", "qeft_token_end_batch"]
ERR_BATCH, ERR_SHAPE, ERR_NULL, ERR_ALIGN = 1, 2, 4, 6
P = 16          # a non-NULL, aligned dummy pointer: never dereferenced, validation comes first
MIS = 18        # misaligned


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "qeft_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
    assert lib.qeft_abi_version() == 1


def _begin(lib, m=4, hidden=256, vocab=512, max_seq=64, n_slots=8, embed=P, h=P, slots=P):
    return lib.qeft_token_begin_norm_batch(embed, P, P, slots, P, h, P, P, P, P, hidden, vocab, max_seq, n_slots, m, None)


def _attn(lib, m=4, heads=4, kv=4, max_seq=64, split=1, tab_rows=None, n_slots=8, kc=P, slots=P, ws=P, out_stride=512):
    return lib.qeft_rope_attn_decode_batch(P, P, P, 1536, P, P, 128, m if tab_rows is None else tab_rows, kc, P, slots, P, P, None, P,
                                           out_stride, ws, split, n_slots, heads, kv, max_seq, m, None)


def _end(lib, m=4, vocab=1000, out_cap=16, n_slots=8, logits=P, slots=P, counter=P):
    return lib.qeft_token_end_batch(logits, slots, P, P, P, P, P, P, counter, vocab, out_cap, n_slots, m, None)


def test_row_count_rejected_before_the_device(lib):
    for m in (0, 9, -1):
        assert _begin(lib, m=m) == ERR_BATCH
        assert _attn(lib, m=m) == ERR_BATCH
        assert _end(lib, m=m) == ERR_BATCH
        assert lib.qeft_attn_batch_workspace_bytes(32, 4, m) == 0
    assert lib.qeft_attn_batch_workspace_bytes(32, 1, 8) == 0           # one split: no workspace
    assert lib.qeft_attn_batch_workspace_bytes(32, 4, 8) > lib.qeft_attn_batch_workspace_bytes(32, 4, 1) > 0


def test_bad_shapes_rejected_before_the_device(lib):
    # heads not a multiple of the kv heads, max_seq not a multiple of 16 / zero, split 3, a rotary table that is neither m rows
    # nor the whole cache, an output row shorter than the heads, no slots
    assert _attn(lib, heads=6, kv=4) == ERR_SHAPE
    assert _attn(lib, max_seq=60) == ERR_SHAPE
    assert _attn(lib, max_seq=0) == ERR_SHAPE
    assert _attn(lib, split=3) == ERR_SHAPE
    assert _attn(lib, tab_rows=5) == ERR_SHAPE
    assert _attn(lib, out_stride=256) == ERR_SHAPE
    assert _attn(lib, n_slots=0) == ERR_SHAPE
    assert _begin(lib, hidden=250) == ERR_SHAPE
    assert _begin(lib, max_seq=0) == ERR_SHAPE
    assert _begin(lib, n_slots=0) == ERR_SHAPE
    assert _end(lib, vocab=0) == ERR_SHAPE
    assert _end(lib, out_cap=0) == ERR_SHAPE
    assert _end(lib, n_slots=0) == ERR_SHAPE


def test_null_and_misaligned_pointers_rejected(lib):
    assert _begin(lib, slots=None) == ERR_NULL
    assert _begin(lib, embed=MIS) == ERR_ALIGN
    assert _begin(lib, h=MIS) == ERR_ALIGN
    assert _attn(lib, slots=None) == ERR_NULL
    assert _attn(lib, split=4, ws=None) == ERR_NULL
    assert _attn(lib, kc=MIS) == ERR_ALIGN
    assert _attn(lib, split=4, ws=MIS) == ERR_ALIGN
    assert _end(lib, slots=None) == ERR_NULL
    assert _end(lib, counter=None) == ERR_NULL
    assert _end(lib, logits=MIS) == ERR_ALIGN


def _metadata_all(text):
    out = {}
    for blk in text.split(".name:")[1:]:
        name = blk.split()[0]
        vals = {kk: int(v) for kk, v in re.findall(r"\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", blk[:1500])}
        if vals:
            out[name] = vals
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_have_no_scratch(tmp_path):
    out = tmp_path / "decode_batch.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-kernarg-preload-count=16",
                    "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "decode_batch.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    meta = {kk: v for kk, v in _metadata_all(open(out).read()).items() if kk.startswith("_ZN4qeft")}
    assert len(meta) == 6, sorted(meta)         # token begin, token end, attention for 1 / 2 / 4 / 8 heads per block
    for name, v in meta.items():
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, name
        assert v.get("private_segment_fixed_size", 0) == 0, name


def test_slot_table_bookkeeping():
    from qeft_amd.batch import SlotTable
    t = SlotTable(3)
    a, b, c = t.take(5, 9, -1), t.take(7, 12, 2), t.take(1, 1, -1)
    assert (a, b, c) == (0, 1, 2) and t.free_count() == 0
    with pytest.raises(RuntimeError, match="no free slot"):
        t.take(3, 4, -1)
    assert t.rows() == [0, 1, 2]
    t.record(0, [11], 5, 0)
    t.record(1, [4, 2], 9, 1)
    t.record(2, [8], 1, 2)
    assert t.rows() == [0] and t.finished() == {1: "eos", 2: "length"}
    assert t.get(1).tokens == [4, 2] and t.get(1).pos == 9
    t.release(1)
    with pytest.raises(KeyError):
        t.get(1)
    assert t.take(2, 3, -1) == 1 and t.rows() == [0, 1]         # the lowest free slot is reused
    t.record(0, [3, 3], 7, 0)
    assert t.get(0).tokens == [11, 3, 3] and t.get(0).reason is None


def test_admission_and_stop_rules():
    from qeft_amd.batch import length_limit, stop_code
    assert length_limit(10, 5, 64) == 14          # 10 prompt tokens, 5 new: the first + 4 passes -> position 14
    assert length_limit(60, 50, 64) == 64         # capped at max_seq
    assert length_limit(64, 3, 64) == 64          # a prompt that fills the cache: only its first token
    with pytest.raises(ValueError, match="does not fit"):
        length_limit(65, 1, 64)
    with pytest.raises(ValueError):
        length_limit(0, 1, 64)
    with pytest.raises(ValueError):
        length_limit(3, 0, 64)
    assert stop_code(7, 3, 10, 7) == 1 and stop_code(7, 10, 10, 7) == 1       # EOS before length
    assert stop_code(6, 10, 10, 7) == 2 and stop_code(6, 9, 10, 7) == 0
    assert stop_code(7, 3, 10, -1) == 0 and stop_code(7, 3, 10, None) == 0    # no EOS set


@pytest.mark.parametrize("why", ["the verify pass runs on the single-GPU engine only (this engine is tensor-parallel)",
                                 "the verify pass runs on 4-bit weights only (this engine has 3-bit weights)",
                                 "the verify pass runs on the v3 engine only (QEFT_ENGINE_V2=1, or shapes the v3 GEMV does not take)"])
def test_unsupported_engine_refused_before_any_allocation(why):
    from qeft_amd.batch import BatchDecodeEngine
    fake = types.SimpleNamespace(_verify_unsupported=lambda: why)
    with pytest.raises(RuntimeError, match="batched decoding runs on"):
        BatchDecodeEngine(fake)


def test_batch_size_bounds():
    from qeft_amd.batch import BatchDecodeEngine
    fake = types.SimpleNamespace(_verify_unsupported=lambda: None)
    for mb in (0, 9):
        with pytest.raises(ValueError, match="max_batch"):
            BatchDecodeEngine(fake, max_batch=mb)
