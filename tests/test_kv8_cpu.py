"""CPU-only checks of the e4m3 KV cache (csrc/decode_attn_kv8.hip, include/qeft_hip.h "FP8 KV cache"): the entries are declared
and exported and reject bad arguments without a GPU, the kernels compile without scratch, the reference recipe of
tests/kv8_ref.py checks itself, and the engines refuse what they do not serve."""
import os
import re
import subprocess

import pytest
import torch

import kv8_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qeft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ["qeft_attn_kv8_workspace_bytes", "qeft_rope_attn_decode_kv8", "qeft_kv8_store_rows"]
ERR_BATCH, ERR_SHAPE, ERR_NULL, ERR_ALIGN = 1, 2, 4, 6
P = 16          # a non-NULL, aligned dummy pointer: never dereferenced -- EVERY call below must fail validation (one that passed
                # would launch on a machine with a GPU)
MIS = 18        # misaligned


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "qeft_hip.h")).read()
    assert "448.0f / amax" in text and "amax / 448.0f" in text      # the recipe is documented where the ABI is
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name


def _attn(lib, m=4, heads=4, kv=4, max_seq=64, split=1, tab_rows=None, n_slots=8, kc=P, vc=P, ks=P, vs=P, slots=P, ws=P,
          out_stride=512, q=P):
    return lib.qeft_rope_attn_decode_kv8(q, P, P, 1536, P, P, 128, m if tab_rows is None else tab_rows, kc, vc, ks, vs, slots, P, P,
                                         None, P, out_stride, ws, split, n_slots, heads, kv, max_seq, m, None)


def _store(lib, T=4, p0=0, kv=4, max_seq=64, stride=1536, k=P, kc=P, ks=P, vs=P):
    return lib.qeft_kv8_store_rows(k, P, stride, kc, P, ks, vs, kv, max_seq, p0, T, None)


def test_attention_arguments_rejected_before_the_device(lib):
    for m in (0, 9, -1):
        assert _attn(lib, m=m) == ERR_BATCH
        assert lib.qeft_attn_kv8_workspace_bytes(32, 4, m) == 0
    assert lib.qeft_attn_kv8_workspace_bytes(32, 1, 8) == 0
    assert lib.qeft_attn_kv8_workspace_bytes(32, 4, 8) > lib.qeft_attn_kv8_workspace_bytes(32, 4, 1) > 0
    # one layout of counters and records with the fp16 batch kernel
    assert lib.qeft_attn_kv8_workspace_bytes(64, 8, 8) == lib.qeft_attn_batch_workspace_bytes(64, 8, 8)
    assert _attn(lib, heads=6, kv=4) == ERR_SHAPE
    assert _attn(lib, heads=0) == ERR_SHAPE
    assert _attn(lib, kv=0) == ERR_SHAPE
    assert _attn(lib, max_seq=60) == ERR_SHAPE
    assert _attn(lib, max_seq=0) == ERR_SHAPE
    assert _attn(lib, max_seq=32784) == ERR_SHAPE                   # above the ceiling
    assert _attn(lib, split=3) == ERR_SHAPE
    assert _attn(lib, split=16) == ERR_SHAPE
    assert _attn(lib, tab_rows=5) == ERR_SHAPE
    assert _attn(lib, out_stride=256) == ERR_SHAPE
    assert _attn(lib, n_slots=0) == ERR_SHAPE
    for name in ("q", "kc", "vc", "ks", "vs", "slots"):
        assert _attn(lib, **{name: None}) == ERR_NULL, name
    assert _attn(lib, split=4, ws=None) == ERR_NULL
    assert _attn(lib, kc=MIS) == ERR_ALIGN
    assert _attn(lib, vc=MIS) == ERR_ALIGN
    assert _attn(lib, ks=MIS) == ERR_ALIGN
    assert _attn(lib, split=4, ws=MIS) == ERR_ALIGN


def test_store_rows_arguments_rejected_before_the_device(lib):
    assert _store(lib, kv=0) == ERR_SHAPE
    assert _store(lib, max_seq=60) == ERR_SHAPE
    assert _store(lib, max_seq=32784) == ERR_SHAPE
    assert _store(lib, T=0) == ERR_SHAPE
    assert _store(lib, p0=-1) == ERR_SHAPE
    assert _store(lib, T=5, p0=60) == ERR_SHAPE                     # p0 + T <= max_seq
    assert _store(lib, T=65) == ERR_SHAPE
    assert _store(lib, stride=256) == ERR_SHAPE                     # a row shorter than the kv heads
    for name in ("k", "kc", "ks", "vs"):
        assert _store(lib, **{name: None}) == ERR_NULL, name
    assert _store(lib, ks=MIS) == ERR_ALIGN


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_compile_without_scratch(tmp_path):
    out = tmp_path / "kv8.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(CSRC, "decode_attn_kv8.hip")], stderr=subprocess.DEVNULL)
    text = out.read_text()
    seen = 0
    for blk in text.split(".name:")[1:]:
        if "kv8" not in blk.split()[0]:
            continue
        vals = dict(re.findall(r"\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", blk[:1500]))
        if vals:
            seen += 1
            assert all(int(v) == 0 for v in vals.values()), (blk.split()[0], vals)
    assert seen == 5                                                # store rows + the attention at R = 1, 2, 4, 8
    assert "v_cvt_pk_f32_fp8" in text and "v_cvt_pk_fp8_f32" in text


# ---- the helper checks itself ---------------------------------------------------------------------------------------------
def test_ref_amax_element_maps_to_the_largest_code():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 128, generator=g) * 0.7).half()
    codes, scales = kv8_ref.quant_rows(x)
    idx = x.float().abs().argmax(-1)
    top = codes[torch.arange(64), idx]
    assert set(top.tolist()) <= {0x7E, 0xFE}
    assert torch.equal(scales, x.float().abs().amax(-1) / 448.0)
    assert not (codes & 0x7F == 0x7F).any()                         # no NaN code
    # the largest fp16 value and the smallest subnormal as the row's maximum
    for amax in (65504.0, 2.0 ** -24):
        y = torch.zeros(128, dtype=torch.float16)
        y[3], y[7] = amax, -amax
        c, s = kv8_ref.quant_rows(y)
        assert c[3].item() == 0x7E and c[7].item() == 0xFE and s.item() > 0


def test_ref_zero_row():
    codes, scales = kv8_ref.quant_rows(torch.zeros(3, 128, dtype=torch.float16))
    assert codes.eq(0).all() and scales.eq(0).all()
    assert kv8_ref.dequant_rows(codes, scales).eq(0).all()


def test_ref_round_trip_within_one_sixteenth():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(256, 128, generator=g) * 2.0).half()
    codes, scales = kv8_ref.quant_rows(x)
    back = kv8_ref.dequant_rows(codes, scales, torch.float64)
    xd = x.double()
    normal = xd.abs() >= scales.double()[:, None] * 2.0 ** -6       # e4m3's normal range under this row's scale
    assert normal.float().mean() > 0.9
    rel = ((back - xd).abs() / xd.abs().clamp_min(1e-30))[normal]
    assert rel.max().item() <= 2.0 ** -4
    # below the normal range the error is absolute: half a subnormal step (2^-10 of the scaled unit)
    assert ((back - xd).abs()[~normal] <= scales.double()[:, None].expand_as(xd)[~normal] * 2.0 ** -10).all()


# ---- the engines' refusals that need no GPU --------------------------------------------------------------------------------
def test_batch_unsupported_splits_from_verify_unsupported():
    import types
    from qeft_amd.batch import batch_unsupported
    from qeft_amd.llama import DecodeEngine
    fp8 = types.SimpleNamespace(tp=False, tp3=False, bits=4, v3=True, kv_dtype="fp8")
    fp8._m_row_unsupported = lambda: DecodeEngine._m_row_unsupported(fp8)
    assert batch_unsupported(fp8) is None                           # batchable
    why = DecodeEngine._verify_unsupported(fp8)
    assert why and "fp8" in why and "KV cache" in why               # not verifiable
    fp16 = types.SimpleNamespace(tp=False, tp3=False, bits=4, v3=True, kv_dtype="fp16")
    fp16._m_row_unsupported = lambda: DecodeEngine._m_row_unsupported(fp16)
    assert DecodeEngine._verify_unsupported(fp16) is None
    w3 = types.SimpleNamespace(tp=False, tp3=False, bits=3, v3=True, kv_dtype="fp8")
    w3._m_row_unsupported = lambda: DecodeEngine._m_row_unsupported(w3)
    assert "batched decoding runs on 4-bit" in batch_unsupported(w3)
    assert "4-bit" in DecodeEngine._verify_unsupported(w3)
