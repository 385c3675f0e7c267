"""The one-token attention (csrc/decode_attn.h, qeft_rope_attn_decode) where its prefetched runs are straight-line code: every
position at which a wave's set of live runs changes on a 512-row cache -- only the new token (0), 1, a run edge (15, 16, 17),
every wave holds a run (63, 64), the last prefetched run and the first loop run (255, 256, 257), 300 -- at head layouts (2, 2)
and (4, 1), splits 1 and 2, both rotary-table forms.

Fixture and reference are those of tests/test_gpu_attn_long.py (imported, not copied): cache rows past the context and the
token's own row are fp16 NaN before every launch, the reference is fp64 on the device over the cache as the launch left it,
acceptance per head |got - ref| <= 2e-3 + 2e-3 max|ref|.  Beyond that bound, per case: the output is finite; the whole-table
form and the selected-row form give identical bits; the cache after the launch equals the cache before it bit for bit except row
`pos`; row `pos` holds the fp16 rounding of the fp32-rotated k and the raw v; and output and appended rows equal, bit for bit,
what the commit before the rewrite produced for the same seeds (tests/golden/attn_decode_parent.npz, written once on the GPU
by tools/dump_attn_golden.py with that commit's library)."""
import os

import numpy as np
import pytest
import torch

import test_gpu_attn_long as AL

pytestmark = pytest.mark.gpu
DEV, HD = AL.DEV, AL.HD
LAYOUTS = [(2, 2), (4, 1)]
MAX_SEQ = 512
POSITIONS = [0, 1, 15, 16, 17, 63, 64, 255, 256, 257, 300]
SPLITS = (1, 2)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_decode_parent.npz")


def slots(heads, kv):
    return AL._Slots(heads, kv, MAX_SEQ, seed=1000 + heads * 16 + kv)


def run_position(A, pos):
    """One qkv row per position (drawn in the order of POSITIONS from the fixture's generator); every split x both forms over a
    freshly poisoned cache.  Returns qkv, the caches before, {(split, form): (out, k cache after, v cache after)}."""
    qkv = A.qkv(1)
    A.poison([pos])
    k_before, v_before = A.kc[0].clone(), A.vc[0].clone()
    res = {}
    for split in SPLITS:
        for form in ("pos", "rows"):
            kc, vc, o = k_before.clone(), v_before.clone(), A.out()
            A.one(qkv, pos, split, o, form, kc=kc, vc=vc)
            res[split, form] = (o, kc, vc)
    A.sync()
    return qkv, k_before, v_before, res


def key(heads, kv, pos, split):
    return f"h{heads}_kv{kv}_p{pos}_s{split}"


def _rot_as_kernel(x, c, s):
    """fp16 of the kernel's fp32 rotary of x [kv, 128] (fp32 from fp16): a c - fl32(b s) and b c + fl32(a s), each ONE fp32
    rounding (the first product is fused into the sum: an FMA, here exact in fp64 -- 11 x 24 significant bits), then one
    rounding to fp16.  The plain two-product formula differs from it by at most one fp16 unit (second assertion there)."""
    a, b = x[:, :64], x[:, 64:]
    r0 = (a.double() * c.double() - (b * s).double()).float()
    r1 = (b.double() * c.double() + (a * s).double()).float()
    return torch.cat([r0, r1], -1).half().contiguous()


def _i16(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def golden_entries(heads, kv):
    """What tools/dump_attn_golden.py stores: the bits of the output and of the appended k / v rows of every case."""
    A = slots(heads, kv)
    out = {}
    for pos in POSITIONS:
        _, _, _, res = run_position(A, pos)
        for split in SPLITS:
            o, kc, vc = res[split, "rows"]
            out[key(heads, kv, pos, split) + "_out"] = _i16(o)
            out[key(heads, kv, pos, split) + "_k"] = _i16(kc[:, pos])
            out[key(heads, kv, pos, split) + "_v"] = _i16(vc[:, pos])
    return out


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_overlap_positions_fp64_forms_cache_and_parent_bits(heads, kv, golden):
    A = slots(heads, kv)
    worst = 0.0
    for pos in POSITIONS:
        qkv, k_before, v_before, res = run_position(A, pos)
        kn = qkv[:1, heads * HD:(heads + kv) * HD].float().view(1, kv, HD)
        k_rot = AL._rot(kn, A.cos[pos:pos + 1, None], A.sin[pos:pos + 1, None])[0].half()      # fp32 rotary, one rounding
        k_fma = _rot_as_kernel(kn[0], A.cos[pos], A.sin[pos])
        v_raw = qkv[0, (heads + kv) * HD:].view(kv, HD)
        for split in SPLITS:
            what = (heads, kv, pos, split)
            o, kc, vc = res[split, "rows"]
            o_pos, kc_pos, vc_pos = res[split, "pos"]
            # the two table forms: identical bits, output and caches
            assert AL._same_bits(o, o_pos) and AL._same_bits(kc, kc_pos) and AL._same_bits(vc, vc_pos), what
            # the cache: untouched except row pos; row pos = fp16(fp32 rotary of k), raw v
            assert AL._same_bits(kc[:, :pos], k_before[:, :pos]) and AL._same_bits(kc[:, pos + 1:], k_before[:, pos + 1:]), what
            assert AL._same_bits(vc[:, :pos], v_before[:, :pos]) and AL._same_bits(vc[:, pos + 1:], v_before[:, pos + 1:]), what
            assert AL._same_bits(vc[:, pos], v_raw.contiguous()), what
            assert AL._same_bits(kc[:, pos], k_fma), (what, "appended k is not fp16(fp32 rotary)")
            dk = (kc[:, pos].float() - k_rot.float()).abs()
            assert (dk <= k_rot.float().abs() * 2.0 ** -10 + 2.0 ** -24).all(), (what, dk.max().item())
            A.check_append(qkv, 1, pos, k_before, v_before, kc, vc)
            # fp64 over the cache as the launch left it; _attn_close asserts finiteness too
            ref = A.reference(qkv, 1, pos, kc, vc)
            assert torch.isfinite(o.float()).all(), what
            worst = max(worst, AL._attn_close(o, ref, what))
            # the parent commit's bits
            k_ = key(heads, kv, pos, split)
            assert np.array_equal(_i16(o), golden[k_ + "_out"]), ("output differs from the parent's", what)
            assert np.array_equal(_i16(kc[:, pos]), golden[k_ + "_k"]), ("appended k differs from the parent's", what)
            assert np.array_equal(_i16(vc[:, pos]), golden[k_ + "_v"]), ("appended v differs from the parent's", what)
    print(f"[attn-overlap] heads={heads} kv={kv} max_seq={MAX_SEQ} splits=1,2 positions={POSITIONS} worst err/bound={worst:.3f}")
