"""CPU-only checks of the verify pass (m-row decode launches, DecodeEngine.verify, qeft_amd/assisted.py): the C ABI's new
entries are declared and exported and reject bad arguments without a GPU, every address of the m-row GEMV stays inside its
operands (host-side enumeration), the new kernels compile without scratch, and the host-side drafting / acceptance rules
match a plain restatement."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qeft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ["qeft_decode_linear_m", "qeft_gemv_v3_check_extents_m", "qeft_token_begin_norm_m", "qeft_attn_m_workspace_bytes",
       "qeft_rope_attn_decode_m", "qeft_lm_head_f16_m", "qeft_verify_greedy"]
ERR_BATCH, ERR_SHAPE = 1, 2


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


def test_row_count_rejected_before_the_device(lib):
    f = 0.0
    for m in (0, 9, -1):
        assert lib.qeft_decode_linear_m(None, None, None, None, None, None, 256, 256, 128, 128, 0, None, None, 0, f, None, None,
                                        None, m, None) == ERR_BATCH
        assert lib.qeft_token_begin_norm_m(None, None, None, None, None, None, None, None, None, 256, 512, 64, m, None) == ERR_BATCH
        assert lib.qeft_rope_attn_decode_m(None, None, None, 768, None, None, 128, m, None, None, None, None, None, 256, None, 1, 2,
                                           2, 64, m, None) == ERR_BATCH
        assert lib.qeft_lm_head_f16_m(None, None, None, None, 512, 1000, f, m, None) == ERR_BATCH
        assert lib.qeft_verify_greedy(None, None, m, 1000, 1, None, None, None, None, None) == ERR_BATCH
        assert lib.qeft_attn_m_workspace_bytes(32, 4, m) == 0
        assert lib.qeft_gemv_v3_check_extents_m(4096, 4096, 128, 128, m, 0, 0, 0) == -1


def test_bad_shapes_rejected_before_the_device(lib):
    f, p = 0.0, 16          # (a non-NULL, aligned dummy pointer: never dereferenced, the shape check comes first)
    # rows not a multiple of 16, K not a whole number of 128-steps, per-channel scales, mode 2
    for n, k, g, mode in ((24, 256, 128, 0), (256, 192, 64, 0), (256, 1024, 1024, 0), (256, 256, 128, 2)):
        assert lib.qeft_decode_linear_m(p, p, p, p, None, p, n, k, g, 128, mode, None, None, 0, f, None, None, None, 4, None) in (2, 3)
    # residual with PAIR, ssq_in count out of range
    assert lib.qeft_decode_linear_m(p, p, p, p, None, p, 256, 256, 128, 128, 1, p, None, 0, f, None, None, None, 4, None) == ERR_SHAPE
    assert lib.qeft_decode_linear_m(p, p, p, p, None, p, 256, 256, 128, 128, 0, None, p, 513, f, None, None, None, 4, None) == ERR_SHAPE
    # attention: heads not a multiple of the kv heads, max_seq not a multiple of 16, split 3, a table that is neither m rows
    # nor the whole cache, an output row shorter than the heads
    for heads, kv, ms, sp, tab, ostr in ((6, 4, 64, 1, 4, 768), (4, 4, 60, 1, 4, 512), (4, 4, 64, 3, 4, 512), (4, 4, 64, 1, 5, 512),
                                         (4, 4, 64, 1, 4, 256)):
        assert lib.qeft_rope_attn_decode_m(p, p, p, 1536, p, p, 128, tab, p, p, p, None, p, ostr, p, sp, heads, kv, ms, 4, None) == ERR_SHAPE
    assert lib.qeft_lm_head_f16_m(p, p, p, p, 640, 1000, f, 4, None) == ERR_SHAPE
    assert lib.qeft_lm_head_f16_m(p, p, p, p, 512, 0, f, 4, None) == ERR_SHAPE
    assert lib.qeft_verify_greedy(p, p, 4, 0, 1, p, p, p, p, None) == ERR_SHAPE
    assert lib.qeft_token_begin_norm_m(p, p, p, p, p, p, p, p, p, 250, 512, 64, 4, None) == ERR_SHAPE


# (n, k) of every linear of the engine: q|k|v, o_proj, gate|up, down_proj -- Llama-2-7B / 13B / 70B and the tests' tiny shapes
SHAPES = {
    "7b": [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)],
    "13b": [(15360, 5120), (5120, 5120), (27648, 5120), (5120, 13824)],
    "70b": [(10240, 8192), (8192, 8192), (57344, 8192), (8192, 28672)],
    "tiny": [(768, 256), (256, 256), (1024, 256), (256, 512)],
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_m_row_extents_in_range(lib, name):
    for j, (n, k) in enumerate(SHAPES[name]):
        mode = 1 if j == 2 else 0
        for m in range(2, 9):
            for n_ssq in ((0, 1, 256, 512) if mode == 0 else (256,)):
                assert lib.qeft_gemv_v3_check_extents_m(n, k, 128, 128, m, mode, n_ssq, 0) == 0, (n, k, m, mode, n_ssq)
            assert lib.qeft_gemv_v3_check_extents_m(n, k, 128, 0, m, mode, 0, 0) == 0, (n, k, m)


def test_m_row_extents_negative_control(lib):
    """Operands 16 rows short of what the launch covers: the enumeration must see the overrun."""
    for n, k in SHAPES["7b"] + SHAPES["tiny"]:
        for m in (2, 5, 8):
            assert lib.qeft_gemv_v3_check_extents_m(n, k, 128, 128, m, 0, 256, 16) > 0, (n, k, m)


def _metadata_all(text):
    out = {}
    for blk in text.split(".name:")[1:]:
        name = blk.split()[0]
        vals = {kk: int(v) for kk, v in re.findall(r"\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", blk[:1500])}
        if vals:
            out[name] = vals
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,prefix", [("gemv_v3_multi.hip", "_ZN4qeft14gemv_v3_kernel"),
                                        ("decode_verify.hip", "_ZN4qeft")])
def test_new_kernels_have_no_scratch(tmp_path, src, prefix):
    out = tmp_path / (src + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-kernarg-preload-count=16",
                    "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, src)], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    meta = {kk: v for kk, v in _metadata_all(open(out).read()).items() if kk.startswith(prefix)}
    assert len(meta) >= (40 if "gemv" in src else 11), sorted(meta)
    for name, v in meta.items():
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, name
        assert v.get("private_segment_fixed_size", 0) == 0, name


def _lookup_restated(ctx, k, max_n=3, min_n=1):
    for n in range(max_n, min_n - 1, -1):
        if len(ctx) <= n:
            continue
        hits = [s for s in range(len(ctx) - n) if ctx[s:s + n] == ctx[-n:]]
        for s in reversed(hits):
            if ctx[s + n:s + n + k]:
                return ctx[s + n:s + n + k]
    return []


def test_prompt_lookup_draft_matches_restatement():
    import random
    from qeft_amd.assisted import PromptLookupDraft
    d = PromptLookupDraft()
    assert d.propose([1, 2, 3, 4, 1, 2], 3) == [3, 4, 1]
    assert d.propose([5, 6, 7], 4) == []
    assert d.propose([1, 2, 3], 0) == []
    rng = random.Random(0)
    for _ in range(500):
        ctx = [rng.randrange(6) for _ in range(rng.randrange(1, 40))]
        k = rng.randrange(0, 8)
        assert d.propose(ctx, k) == (_lookup_restated(ctx, k) if k > 0 else []), (ctx, k)


def test_acceptance_rule():
    from qeft_amd.assisted import accepted_prefix
    assert accepted_prefix([5, 6, 7, 8], [4, 5, 6, 7]) == (3, [5, 6, 7, 8])      # all drafts accepted + bonus
    assert accepted_prefix([9, 6, 7, 8], [4, 5, 6, 7]) == (0, [9])               # none
    assert accepted_prefix([5, 6, 0, 8], [4, 5, 6, 7]) == (2, [5, 6, 0])         # partial
    assert accepted_prefix([3], [4]) == (0, [3])                                 # m = 1: a plain greedy step
