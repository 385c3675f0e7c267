"""Every reachable instance of the v3 decode GEMV (csrc/gemv_v3.h) pinned to a shape and to float64.

gemv_v3_plan (csrc/gemv_v3.hip) chooses between the instantiations of one kernel template -- waves per block, row sets per block,
ring depth, outlier step, PLAIN / PAIR, 4 / 3 bits, the flag-free or the flagged half, one or several batch rows, x from LDS or
from global memory -- and qeft_last_variant calls them all "gemv_v3".  Each case below names the instance it must run
(nw, rs_cap, D, outl, mode, bits, fl, mb, xg), asserts it with == against qeft_gemv_v3_last_plan, and compares the whole output
with float64.  TIERS holds, per (nw, rs_cap, D), the smallest shape that reaches it and shapes next to the clause of the plan that
admits it (the reason says which), with nfull varied so that the outlier step falls on wave 0, on the last wave, and on a block
where nfull < nw leaves waves without a step -- where the row's range of nfull allows it: (8, 1, 4) lives on nfull 57 .. 63 and
(12, 1, 2) on nfull >= 64, so neither has nfull < nw, and no nfull of 57 .. 63 is a multiple of 8.  The first shape of a row (a
ragged one: some blocks hold rs_cap sets, the others one fewer) is crossed with outl x mode x bits on both halves.
EM / EM_XG hold the engine's m-row family (qeft_decode_linear_m, "gemv_v3_multi"): 2..8 rows with the engine's fused epilogues.
tests/test_gemv_v3_plan.py (no GPU) checks that these tables name exactly the instances a launch can reach.

Every launch goes through the C ABI with each output all-NaN between two NaN bands: the bands must stay NaN, the middle must become
finite, and a second launch must give the same bits (the plan fixes the summation order).

The reference is float64 on the UNROUNDED weights q * s + z (O.dequant_dense(round_fp16=False)): that is what this kernel multiplies
by (one fp32 FMA pair per step, no fp16 weight in between).  The oracle's default rounds every weight to fp16 first, as the
reference's own kernels do; at K = 256 with 3-bit per-channel scales that rounding alone, under an exact product rounded once to
fp16, puts 1 of 8224 outputs outside elem_err_ok (rel_err 3.787e-4 either way), and at K = 8192 with 4-bit per-channel scales, where
a row has 16 distinct weights whose 16 rounding errors add up coherently over 8192 columns, it moves a gate value by 4.7e-4 and the
PAIR output by 2.3e-3 of the largest (1.9e-4 against the unrounded weights) -- the reference's error, not the kernel's.

Bounds: rel_err < REL_TOL and elem_err_ok with its defaults (tests/util.py); PAIR 2e-3 and the consumer-side norm 3e-3 on rel_err,
as tests/test_gpu_gemv_v3.py (one more fp16 rounding: gate and up before the activation, h * gamma before the product).

Column probes (test_column_probes): see its docstring for the bound."""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import qeft_oracle as O
from util import REL_TOL, elem_err_ok, layer_to_torch, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 4096                      # NaN elements in front of and behind a banded buffer
PLAIN, PAIR = 0, 1
PERCH, XN, SZN, OWIL, XG, ENGINE_M, GATHER = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 29, 1 << 31
PLAN_INTS = 13
EPS = 1e-5

# entry: how the case reaches the kernel.  want: (nw, rs_cap, D, outl, mode, bits, fl, mb, xg).  flags: what the entry's operands set.
Case = collections.namedtuple("Case", "n k r g m mode bits entry flags want reason")

# (nw, rs_cap, D) -> [(n, K at n_out = 128, reason)]; without the outlier slice the same nfull is K - 128.
TIERS = {
    (8, 1, 2): [(16, 256, "the smallest launch: one block, nfull 1 < 8 waves (outlier step on wave 1, six waves without a step)"),
                (48, 1152, "three blocks; nfull 8: outlier step on wave 0"),
                (4096, 1024, "256 blocks: the last one-set grid, 32 blocks per XCD; nfull 7: outlier step on the last wave"),
                (16, 7296, "nfull 56: 7 loads per wave, the last shape under the deep ring")],
    (8, 1, 4): [(16, 7424, "nfull 57: ceil(57 / 8) = 8 loads per wave; outlier step on wave 1"),
                (48, 8192, "nfull 63: the last under the 12-wave form; outlier step on the last wave"),
                (4096, 7424, "256 blocks")],
    (12, 1, 2): [(16, 8320, "nfull 64: the first 12-wave shape; outlier step on wave 4"),
                 (48, 9344, "nfull 72 = 6 x 12: outlier step on wave 0"),
                 (16, 9216, "nfull 71: outlier step on the last wave (11)"),
                 (4096, 8320, "256 blocks")],
    (8, 2, 2): [(4112, 256, "257 sets on 129 blocks, 128 of two and one of one; nfull 1 < 8"),
                (4112, 1152, "nfull 8: outlier step on wave 0"),
                (4112, 1024, "nfull 7: outlier step on the last wave"),
                (4112, 3200, "nfull 24: 3 x 2 = 6 loads per wave, the last shape under the deep ring")],
    (8, 2, 4): [(4112, 3328, "nfull 25: ceil(25 / 8) x 2 = 8 loads per wave; outlier step on wave 1"),
                (4112, 4224, "nfull 32: outlier step on wave 0"),
                (4112, 4096, "nfull 31: outlier step on the last wave")],
    (8, 3, 2): [(8224, 256, "514 sets on 172 blocks, 170 of three and two of two; nfull 1 < 8"),
                (8208, 256, "the smallest: 513 sets on 171 blocks of three (512 would be 256 blocks of two)"),
                (8224, 1152, "nfull 8: outlier step on wave 0"),
                (8224, 1024, "nfull 7: outlier step on the last wave"),
                (8224, 2176, "nfull 16: 2 x 3 = 6 loads per wave, the last shape under the deep ring")],
    (8, 3, 6): [(8224, 2304, "nfull 17: ceil(17 / 8) x 3 = 9 loads per wave; outlier step on wave 1"),
                (8208, 2304, "the smallest: no short block"),
                (8224, 3200, "nfull 24: outlier step on wave 0"),
                (8224, 3072, "nfull 23: outlier step on the last wave")],
    (8, 4, 2): [(12304, 256, "769 sets on 193 blocks, 190 of four and three of three (768 would be 256 blocks of three); nfull 1 < 8"),
                (12304, 1152, "nfull 8: 1 x 4 = 4 loads per wave, the last shape under the deep ring; outlier step on wave 0"),
                (12304, 1024, "nfull 7: outlier step on the last wave")],
    (8, 4, 6): [(12304, 1280, "nfull 9: ceil(9 / 8) x 4 = 8 loads per wave; outlier step on wave 1"),
                (12304, 2176, "nfull 16: outlier step on wave 0"),
                (12304, 2048, "nfull 15: outlier step on the last wave")],
    (4, 3, 4): [(18448, 256, "1153 sets on 385 blocks, 383 of three and two of two: more than 256 blocks; nfull 1 < 4"),
                (18432, 256, "the smallest: 1152 sets, (1152 + 384) / 768 = 2: 512 blocks evened to 384 of three"),
                (18448, 512, "nfull 3 < 4: outlier step on the last wave"),
                (18448, 640, "nfull 4: outlier step on wave 0"),
                (18448, 1024, "nfull 7: two steps on three waves, one on the fourth")],
    (4, 4, 4): [(16400, 256, "1025 sets: five per block on 256 blocks, so ceil(1025 / 4) = 257 blocks, 254 of four and three of three; nfull 1 < 4"),
                (16400, 512, "nfull 3 < 4: outlier step on the last wave"),
                (16400, 640, "nfull 4: outlier step on wave 0"),
                (16400, 1024, "nfull 7: outlier step on the last wave")],
}

# Several batch rows (MB = 2; 8 waves, 4 bits, PLAIN, the flagged half): (rs_cap, D) -> (n, K at n_out = 128), at m = 2 through the
# gemv entry (partial sums of 8 batch rows per wave) and m = 9 through the GEMM entry (16 per wave).
MB = {(1, 2): (48, 1152), (1, 4): (16, 7424), (2, 2): (4112, 1152), (2, 4): (4112, 3328), (3, 2): (8224, 1152), (3, 6): (8224, 2304),
      (4, 2): (12304, 1152), (4, 6): (12304, 1280)}
# x fragments from global memory (xg): the entries ask for it when the m rows of x do not fit the block's 160 KB of LDS next to its
# scales, outlier slabs and partial sums; the ring is then deep whatever the load count.  (rs_cap, D) -> (entry, m, n, K with
# n_out = 128, K with n_out = 0): without the 4 KB outlier slabs more of x fits, so the two K differ.
MB_XG = {(1, 4): ("gemv", 7, 16, 11776, 11776), (2, 4): ("gemm", 16, 4112, 4352, 4224), (3, 6): ("gemm", 16, 8224, 3200, 3840),
         (4, 6): ("gemm", 16, 12304, 2688, 3200)}
# The engine's m-row launches (qeft_decode_linear_m: MB = 2 on the flag-free half, PLAIN and PAIR, 8 waves): (rs_cap, D) -> (n, K at
# n_out = 128), the smallest shape of each at m = 2.  x from global memory: the entry asks for it where the m rows of x do not fit the
# LDS (and only there: test_every_pinned_case_is_what_the_plan_says); (rs_cap, D) -> (n, K with n_out = 128, K with n_out = 0), the
# smallest K at m = 8.  One ragged m (5) on a row of each table: EM_M5 (n, K at n_out = 128, xg).
EM = {(1, 2): (16, 256), (1, 4): (16, 7424), (2, 2): (4112, 256), (2, 4): (4112, 3328), (3, 2): (8208, 256), (3, 6): (8208, 2304),
      (4, 2): (12304, 256), (4, 6): (12304, 1280)}
EM_XG = {(1, 4): (16, 8832, 9344), (2, 4): (4112, 8320, 8832), (3, 6): (8208, 7808, 8320), (4, 6): (12304, 6784, 7808)}
EM_M5 = {(2, 4): (4112, 3328, False), (1, 4): (16, 14464, True)}

ENTRY_FLAGS = {"engine_m": lambda r: ENGINE_M, "decode": lambda r: 0, "hnorm": lambda r: XN, "ckpt": lambda r: SZN | GATHER | (OWIL if r else 0),
               "gemv": lambda r: SZN | (OWIL if r else 0), "gemm": lambda r: SZN}


def _case(n, k128, outl, g_perch, m, mode, bits, entry, triple, reason, xg=False):
    r = 128 if outl else 0
    k = k128 if outl else k128 - 128
    flags = ENTRY_FLAGS[entry](r) | (XG if xg else 0)
    fl = int(entry != "engine_m" and (m > 1 or g_perch or flags != 0))
    nw, rs, d = triple
    return Case(n, k, r, k if g_perch else 128, m, mode, bits, entry, flags, (nw, rs, d, int(outl), mode, bits, fl, 2 if m > 1 else 1, int(xg)), reason)


def _cross_shape(triple):
    """The shape a row is crossed and probed on: its first one, with at least two full steps beside the outlier step (K = 128 has
    one group per row at group size 128 too: per-channel scales would set no flag there, and a probe's first step would be its last)."""
    n, k, _ = TIERS[triple][0]
    return n, max(k, 384)


def _build_cases():
    cases = []
    for triple, shapes in TIERS.items():
        for n, k, reason in shapes:                                  # the flag-free PLAIN 4-bit launch with the outlier step, every shape
            cases.append(_case(n, k, True, False, 1, PLAIN, 4, "decode", triple, reason))
        n, k = _cross_shape(triple)
        for outl in (True, False):
            for mode in (PLAIN, PAIR):
                for bits in (4, 3):
                    cases.append(_case(n, k, outl, False, 1, mode, bits, "decode", triple, "crossing of the row's first shape"))
                    cases.append(_case(n, k, outl, True, 1, mode, bits, "decode", triple, "the flagged half through per-channel scales"))
        cases.append(_case(n, k, True, False, 1, PLAIN, 4, "hnorm", triple, "the flagged half through the consumer-side norm"))
        cases.append(_case(n, k, True, False, 1, PAIR, 4, "hnorm", triple, "the consumer-side norm in PAIR mode"))
        cases.append(_case(n, k, True, False, 1, PLAIN, 4, "ckpt", triple, "the flagged half through the checkpoint-layout entry with a gather"))
    for (rs, d), (n, k) in MB.items():
        for outl in (True, False):
            cases.append(_case(n, k, outl, False, 2, PLAIN, 4, "gemv", (8, rs, d), "two batch rows: 8 rows of partial sums per wave"))
            cases.append(_case(n, k, outl, False, 9, PLAIN, 4, "gemm", (8, rs, d), "nine batch rows: 16 rows of partial sums per wave"))
    for (rs, d), (entry, m, n, k_on, k_off) in MB_XG.items():
        cases.append(_case(n, k_on, True, False, m, PLAIN, 4, entry, (8, rs, d), "the x rows do not fit the LDS", xg=True))
        cases.append(_case(n, k_off + 128, False, False, m, PLAIN, 4, entry, (8, rs, d), "the x rows do not fit the LDS", xg=True))
    for mode in (PLAIN, PAIR):
        for (rs, d), (n, k) in EM.items():
            for outl in (True, False):
                cases.append(_case(n, k, outl, False, 2, mode, 4, "engine_m", (8, rs, d), "two rows of the verify pass"))
        for (rs, d), (n, k_on, k_off) in EM_XG.items():
            cases.append(_case(n, k_on, True, False, 8, mode, 4, "engine_m", (8, rs, d), "eight x rows do not fit the LDS", xg=True))
            cases.append(_case(n, k_off + 128, False, False, 8, mode, 4, "engine_m", (8, rs, d), "eight x rows do not fit the LDS", xg=True))
        for (rs, d), (n, k, xg) in EM_M5.items():
            cases.append(_case(n, k, True, False, 5, mode, 4, "engine_m", (8, rs, d), "five rows: three waves without a row", xg=xg))
    unique = {c[:-1]: c for c in reversed(cases)}                   # (a crossing that is one of the row's own shapes: once)
    # cases that share a packed layer stand together (the cache below holds a few layers)
    return sorted(unique.values(), key=lambda c: (c.n, c.k, c.r, c.g, c.bits))


CASES = _build_cases()


def all_cases():
    return list(CASES)


def pinned_instances():
    """instance -> the first case that pins it."""
    out = {}
    for c in CASES:
        out.setdefault(c.want, c)
    return out


def blocks_of(c):
    from qeft_amd import _lib
    return _lib.lib().qeft_decode_linear_blocks(c.n)


def _id(c):
    w = c.want
    return (f"nw{w[0]}-rs{w[1]}-d{w[2]}-{'outl' if w[3] else 'noout'}-{'pair' if w[4] else 'plain'}-w{w[5]}-{'fl' if w[6] else 'nofl'}"
            f"{'-xg' if w[8] else ''}-{c.entry}-m{c.m}-{c.n}x{c.k}-g{c.g}")


_WORST = {}                      # instance -> (worst rel_err, case id)
_WORST_PROBE = {}                # instance -> (worst |error| / bound, case id)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_per_instance():
    yield
    print("\nworst rel_err per instance (nw, rs_cap, D, outl, mode, bits, fl, mb, xg) (tests/test_gpu_gemv_v3_tiers.py)")
    for inst in sorted(_WORST):
        err, case = _WORST[inst]
        print(f"  {str(inst):36s} {err:.3e}  at {case}")
    print("worst |error| / bound of the column probes per instance")
    for inst in sorted(_WORST_PROBE):
        ratio, case = _WORST_PROBE[inst]
        print(f"  {str(inst):36s} {ratio:.3f}  at {case}")


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


@functools.lru_cache(maxsize=3)
def _layer(n, k, r, g, bits=4):
    """One packed layer per shape: numpy buffers, the same on the GPU (with sz_packed), the dense float64 weights."""
    from qeft_amd import qeft_cuda
    bufs = O.make_layer(n, k, r, g, seed=n + k + r + g, bias=True, bits=bits)
    w64 = O.dequant_dense(bufs["qweight"], bufs["scales"], bufs["scaled_zeros"], bufs["oweight"] if r else None, g,
                          round_fp16=False).astype(np.float64)
    t = layer_to_torch(bufs, DEV)
    t["sz_packed"] = qeft_cuda.pack_scales(t["scales"], t["scaled_zeros"], n, k, g)
    return bufs, t, w64


class _Banded:
    """n elements of `dtype`, all NaN (or `init`), between two bands of NaN."""

    def __init__(self, n, dtype, init=None):
        self.raw = torch.full((n + 2 * BAND,), float("nan"), dtype=dtype, device=DEV)
        self.mid = self.raw[BAND:BAND + n]
        if init is not None:
            self.mid.copy_(init)
        assert self.mid.data_ptr() % 16 == 0

    def ptr(self):
        return self.mid.data_ptr()

    def still_poisoned(self):
        return bool(torch.isnan(self.raw[:BAND]).all() and torch.isnan(self.raw[-BAND:]).all())


def _plan(lib, c):
    out = (ctypes.c_int * PLAN_INTS)()
    rc = lib.qeft_gemv_v3_plan(c.n, c.k, c.g, c.r, c.m, c.mode, c.bits, c.flags - (1 << 32) if c.flags >> 31 else c.flags, out)
    assert rc == 0, (rc, c)
    return tuple(out)


def _last_plan(lib):
    out = (ctypes.c_int * PLAN_INTS)()
    assert lib.qeft_gemv_v3_last_plan(out) == 0
    return tuple(out)


def _instance(p):
    return p[4], p[1], p[5], p[6], p[7], p[8], p[9], p[10], p[11]


def _p(t):
    return t.data_ptr() if t is not None else None


def _silu_pair(full):
    """PAIR operand rows: set s = gate rows [16 s, 16 s + 8), up rows [16 s + 8, 16 s + 16) -> silu(gate) * up, n / 2 outputs."""
    v = full.reshape(full.shape[0], -1, 2, 8)
    gate, up = v[:, :, 0, :], v[:, :, 1, :]
    return (gate / (1 + np.exp(-gate)) * up).reshape(full.shape[0], -1)


def _inputs(c):
    """(the entry's x operands on the GPU, the float64 activation the weights are multiplied by)."""
    rng = np.random.default_rng(c.n + c.k + c.m)
    if c.entry == "hnorm":
        h = (rng.standard_normal(c.k) * 2).astype(np.float32)
        gamma = (1 + 0.1 * rng.standard_normal(c.k)).astype(np.float16)
        h64 = h.astype(np.float64)
        xn = h64 / np.sqrt((h64 ** 2).mean() + EPS) * gamma.astype(np.float64)
        return (torch.from_numpy(h).to(DEV), torch.from_numpy(gamma).to(DEV)), xn[None]
    x = O.make_activation(c.m, c.k, c.r, seed=c.m + 2)
    xt = torch.from_numpy(x).to(DEV)
    if c.entry == "ckpt":
        ids = rng.permutation(c.k).astype(np.int32)
        return (xt, torch.from_numpy(ids).to(DEV)), x.astype(np.float64)[:, ids]
    return (xt,), x.astype(np.float64)


def _launch(lib, c, t, ops, y):
    """One launch of the case's entry into the buffer `y` (a device pointer)."""
    from qeft_amd import _lib
    n, k, g, r = c.n, c.k, c.g, c.r
    ow, ow_il = (_p(t["oweight"]), _p(t["oweight_interleaved"])) if r else (None, None)
    if c.entry == "decode":
        entry = lib.qeft_decode_linear_w3 if c.bits == 3 else lib.qeft_decode_linear
        rc = entry(_p(ops[0]), _p(t["qweight"]), _p(t["sz_packed"]), ow, _p(t["bias"]), y, n, k, g, r, c.mode, None, None, 0, 0.0, None, None,
                   None, _st())
    elif c.entry == "hnorm":
        rc = lib.qeft_decode_linear_hnorm(_p(ops[0]), _p(ops[1]), _p(t["qweight"]), _p(t["sz_packed"]), ow, _p(t["bias"]), y, n, k, g, r, c.mode,
                                          EPS, _st())
    elif c.entry == "ckpt":
        rc = lib.qeft_gemv_w4_fused(_p(ops[0]), _p(t["qweight"]), _p(t["scales"]), _p(t["scaled_zeros"]), ow_il, _p(t["bias"]), _p(ops[1]), None,
                                    None, y, c.m, n, k, g, r, _st())
    elif c.entry == "gemv":
        rc = lib.qeft_gemv_w4_fused(_p(ops[0]), _p(t["qweight"]), _p(t["scales"]), _p(t["scaled_zeros"]), ow_il, _p(t["bias"]), None, None, None,
                                    y, c.m, n, k, g, r, _st())
    else:
        rc = lib.qeft_gemm_w4(_p(ops[0]), _p(t["qweight"]), _p(t["scales"]), _p(t["scaled_zeros"]), ow, _p(t["bias"]), y, c.m, n, k, g, r, _st())
    _lib.check(rc)


def _tolerance(c):
    return 3e-3 if c.entry == "hnorm" else 2e-3 if c.mode == PAIR else REL_TOL


ONE_ENTRY_CASES = [c for c in CASES if c.entry != "engine_m"]
ENGINE_M_CASES = [c for c in CASES if c.entry == "engine_m"]


@pytest.mark.parametrize("c", ONE_ENTRY_CASES, ids=[_id(c) for c in ONE_ENTRY_CASES])
def test_instance(c):
    from qeft_amd import _lib
    lib = _lib.lib()
    bufs, t, w64 = _layer(c.n, c.k, c.r, c.g, c.bits)
    ops, x64 = _inputs(c)
    n_y = c.m * (c.n // 2 if c.mode == PAIR else c.n)
    y, y2 = _Banded(n_y, torch.float16), _Banded(n_y, torch.float16)
    _launch(lib, c, t, ops, y.ptr())
    ran, variant = _last_plan(lib), _lib.last_variant()
    _launch(lib, c, t, ops, y2.ptr())
    torch.cuda.synchronize()
    assert _instance(ran) == c.want, (ran, c.want, c.reason)
    assert ran == _plan(lib, c) and ran[0] == lib.qeft_decode_linear_blocks(c.n), (ran, _plan(lib, c))
    assert variant == ("gemv_v3_mb_xg" if c.want[8] else "gemv_v3_mb" if c.m > 1 else
                       "gemv_v3" + ("_w3" if c.bits == 3 else "") + ("_pair" if c.mode == PAIR else "")), variant
    assert y.still_poisoned() and y2.still_poisoned(), c
    got = y.mid.cpu().numpy().astype(np.float64).reshape(c.m, -1)
    assert np.isfinite(got).all(), c
    assert torch.equal(y.mid, y2.mid), "a second launch of the same plan sums in the same order"
    ref = x64 @ w64.T + bufs["bias"].astype(np.float64)
    if c.mode == PAIR:
        ref = _silu_pair(ref)
    err = rel_err(got, ref)
    print(f"[v3 tier] {_id(c)}: rel_err {err:.3e}")
    if c.want not in _WORST or err > _WORST[c.want][0]:
        _WORST[c.want] = (err, _id(c))
    assert err < _tolerance(c), (c, err)
    if c.mode == PLAIN and c.entry != "hnorm":
        assert elem_err_ok(got, ref), c


# ------------------------------------------------------------------------------------------- the engine's m-row family
@pytest.mark.parametrize("c", ENGINE_M_CASES, ids=[_id(c) for c in ENGINE_M_CASES])
def test_engine_m_instance(c):
    """qeft_decode_linear_m on m rows in the engine's forms: PAIR with ssq_in (gate|up); PLAIN with ssq_in (q|k|v: 300 producer sums,
    both 256-float pieces) and PLAIN with the fp32 residual, gamma_out -> ynorm and ssq_out [m][blocks] (o_proj, down_proj).  Every
    launch must have run the instance the case names (qeft_gemv_v3_last_plan ==), under the family's variant name, and every output
    is compared whole with float64: rel_err < REL_TOL and elem_err_ok for PLAIN, the one-row PAIR bound (2e-3) for PAIR."""
    from qeft_amd import _lib
    lib = _lib.lib()
    n, k, m = c.n, c.k, c.m
    bufs, t, w64 = _layer(n, k, c.r, c.g)
    x = O.make_activation(m, k, c.r, seed=m + 2)
    xt = torch.from_numpy(x).to(DEV)
    rng = np.random.default_rng(n + k + m)
    n_ssq = 300
    ssq = (rng.random((m, n_ssq)) * 10 + 1).astype(np.float32)
    rs_norm = 1.0 / np.sqrt(ssq.astype(np.float64).sum(1, keepdims=True) / k + EPS)
    ssq_t = torch.from_numpy(ssq).to(DEV)
    prod, bias = x.astype(np.float64) @ w64.T, bufs["bias"].astype(np.float64)
    nblk = lib.qeft_decode_linear_blocks(n)
    want_plan = _plan(lib, c)
    want_variant = "gemv_v3_multi_xg" if c.want[8] else "gemv_v3_multi_pair" if c.mode == PAIR else "gemv_v3_multi"

    def launch(y, residual=None, ssq_in=None, gamma_out=None, ynorm=None, ssq_out=None):
        _lib.check(lib.qeft_decode_linear_m(_p(xt), _p(t["qweight"]), _p(t["sz_packed"]), _p(t["oweight"]) if c.r else None, _p(t["bias"]), y,
                                            n, k, c.g, c.r, c.mode, residual, ssq_in, n_ssq if ssq_in else 0, EPS, gamma_out, ynorm, ssq_out, m,
                                            _st()))
        ran = _last_plan(lib)
        assert _instance(ran) == c.want and ran == want_plan and ran[0] == nblk, (ran, c.want, c.reason)
        assert _lib.last_variant() == want_variant

    def worst(err):
        print(f"[v3 tier] {_id(c)}: rel_err {err:.3e}")
        if c.want not in _WORST or err > _WORST[c.want][0]:
            _WORST[c.want] = (err, _id(c))

    n_y = m * (n // 2 if c.mode == PAIR else n)
    y, y2 = _Banded(n_y, torch.float16), _Banded(n_y, torch.float16)
    launch(y.ptr(), ssq_in=_p(ssq_t))
    launch(y2.ptr(), ssq_in=_p(ssq_t))
    torch.cuda.synchronize()
    assert y.still_poisoned() and y2.still_poisoned(), c
    got = y.mid.cpu().numpy().astype(np.float64).reshape(m, -1)
    assert np.isfinite(got).all(), c
    assert torch.equal(y.mid, y2.mid), "a second launch of the same plan sums in the same order"
    ref = prod * rs_norm + bias
    if c.mode == PAIR:
        err = rel_err(got, _silu_pair(ref))
        worst(err)
        assert err < 2e-3, (c, err)
        return
    err = rel_err(got, ref)
    worst(err)
    assert err < REL_TOL and elem_err_ok(got, ref), (c, err)
    # the producer form: y32 = W x + bias + residual (fp32, in place), ynorm = fp16(y32 * gamma), ssq_out[row][block]
    h0 = rng.standard_normal((m, n)).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(n)).astype(np.float16)
    gt = torch.from_numpy(gamma).to(DEV)
    y32 = _Banded(m * n, torch.float32, init=torch.from_numpy(h0).to(DEV).reshape(-1))
    ynorm, so = _Banded(m * n, torch.float16), _Banded(m * nblk, torch.float32)
    launch(y32.ptr(), residual=y32.ptr(), gamma_out=_p(gt), ynorm=ynorm.ptr(), ssq_out=so.ptr())
    torch.cuda.synchronize()
    for b in (y32, ynorm, so):
        assert b.still_poisoned() and bool(torch.isfinite(b.mid).all()), c
    href = h0.astype(np.float64) + prod + bias
    h = y32.mid.cpu().numpy().astype(np.float64).reshape(m, n)
    err = rel_err(h, href)
    worst(err)
    assert err < REL_TOL and elem_err_ok(h, href), (c, err)
    yn, ynref = ynorm.mid.cpu().numpy().astype(np.float64).reshape(m, n), href * gamma.astype(np.float64)
    assert rel_err(yn, ynref) < REL_TOL and elem_err_ok(yn, ynref), c
    sums, sref = so.mid.cpu().numpy().astype(np.float64).reshape(m, nblk).sum(1), (href ** 2).sum(1)
    assert (np.abs(sums - sref) / sref).max() < REL_TOL, c


# ------------------------------------------------------------------------------------ the producer epilogue on ragged blocks
PRODUCER = [(4112, 256, (8, 2, 2)), (12304, 256, (8, 4, 2)), (16400, 256, (4, 4, 4)), (12304, 1280, (8, 4, 6))]


@pytest.mark.parametrize("n,k,triple", PRODUCER, ids=[f"nw{t[0]}-rs{t[1]}-d{t[2]}-{n}x{k}" for n, k, t in PRODUCER])
def test_producer_epilogue_on_ragged_blocks(n, k, triple):
    """y32 = W x + residual, ynorm = fp16(y32 * gamma), ssq_out[block] = sum of y32^2 over the block's rows, on launches whose
    blocks hold rs_cap and rs_cap - 1 row sets; then ssq_out -- qeft_decode_linear_blocks(n) entries, not a multiple of 4 -- as the
    ssq_in of a consumer.  The consumer's K must be a multiple of 128 and these n are not, so it takes the first k2 = n - n % 128
    elements of ynorm; the kernel scales by rsqrt(sum(ssq_in) / k2 + eps), and the float64 chain says the same."""
    from qeft_amd import _lib
    lib = _lib.lib()
    r, g = 128, 128
    bufs, t, w64 = _layer(n, k, r, g)
    nblk = lib.qeft_decode_linear_blocks(n)
    assert nblk % 4 != 0 and n % nblk != 0
    rng = np.random.default_rng(n)
    x = O.make_activation(1, k, r, seed=6)
    xt = torch.from_numpy(x[0]).to(DEV)
    h0 = rng.standard_normal(n).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(n)).astype(np.float16)
    h0t, gt = torch.from_numpy(h0).to(DEV), torch.from_numpy(gamma).to(DEV)
    want = (triple[0], triple[1], triple[2], 1, PLAIN, 4, 0, 1, 0)

    def launch(y, residual, gamma_out=None, ynorm=None, ssq=None):
        _lib.check(lib.qeft_decode_linear(_p(xt), _p(t["qweight"]), _p(t["sz_packed"]), _p(t["oweight"]), _p(t["bias"]), y, n, k, g, r, PLAIN,
                                          residual, None, 0, 0.0, gamma_out, ynorm, ssq, _st()))
        assert _instance(_last_plan(lib)) == want

    ref = h0.astype(np.float64) + (x.astype(np.float64) @ w64.T + bufs["bias"].astype(np.float64))[0]
    apart = _Banded(n, torch.float32)
    launch(apart.ptr(), _p(h0t))                                     # the residual apart from the output
    alias = _Banded(n, torch.float32, init=h0t)
    launch(alias.ptr(), alias.ptr())                                 # in place
    y32, ynorm, ssq = _Banded(n, torch.float32), _Banded(n, torch.float16), _Banded(nblk, torch.float32)
    launch(y32.ptr(), _p(h0t), _p(gt), ynorm.ptr(), ssq.ptr())
    torch.cuda.synchronize()
    for b in (apart, alias, y32, ynorm, ssq):
        assert b.still_poisoned() and bool(torch.isfinite(b.mid).all())
    err = rel_err(apart.mid.cpu().numpy(), ref)
    print(f"[v3 producer] {n}x{k}: y32 rel_err {err:.3e}")
    assert err < REL_TOL
    assert torch.equal(alias.mid, apart.mid) and torch.equal(y32.mid, apart.mid)
    assert torch.equal(ynorm.mid, (y32.mid * gt.float()).half())
    total = float((y32.mid.double() ** 2).sum())
    print(f"[v3 producer] {n}x{k}: sum(ssq_out) off by {abs(float(ssq.mid.double().sum()) - total) / total:.3e} of it")
    assert abs(float(ssq.mid.double().sum()) - total) <= 1e-4 * total
    # consumer: deferred 1 / rms from the partial sums, x = the first k2 elements of ynorm
    n2, k2 = 48, n - n % 128
    b2, t2, w2 = _layer(n2, k2, r, g)
    y = _Banded(n2, torch.float16)
    _lib.check(lib.qeft_decode_linear(ynorm.ptr(), _p(t2["qweight"]), _p(t2["sz_packed"]), _p(t2["oweight"]), None, y.ptr(), n2, k2, g, r, PLAIN,
                                      None, ssq.ptr(), nblk, EPS, None, None, None, _st()))
    torch.cuda.synchronize()
    assert y.still_poisoned() and ssq.still_poisoned()
    hv = y32.mid.cpu().numpy().astype(np.float64)
    xn = (hv * gamma.astype(np.float64))[:k2] / np.sqrt((hv ** 2).sum() / k2 + EPS)
    err = rel_err(y.mid.cpu().numpy(), w2 @ xn)
    print(f"[v3 producer] {n}x{k}: consumer rel_err {err:.3e}")
    assert err < 2e-3           # x gamma is rounded to fp16 before the product (one more rounding than the float64 chain)


# ----------------------------------------------------------------------------------------------------- column probes
def _probe_columns(k, r):
    """Every column of the first 128-k step, of the last INT step and of the outlier step; the first and last column of every other
    step: at most 2 nfull + 384."""
    nfull = (k - r) // 128
    cols = set(range(0, 128)) | set(range((nfull - 1) * 128, nfull * 128)) | set(range(k - r, k))
    for s in range(nfull):
        cols |= {s * 128, s * 128 + 127}
    return np.array(sorted(cols))


def _exact_columns(bufs, cols, k, r, g, bits):
    """(w, |q s|, |z|) of the probed columns in float64, [len(cols)][n]: w = q * s + z exactly (a 4-bit, an 11-bit and an 11-bit
    number: float64 holds the sum), the outlier columns the fp16 values themselves."""
    q = (O.unpack_w3(bufs["qweight"]) if bits == 3 else O.unpack_intweight(bufs["qweight"])).astype(np.float64)
    kq = k - r
    ic = np.minimum(cols, kq - 1)
    qs = q[:, ic].T * bufs["scales"].astype(np.float64)[ic // g]
    z = bufs["scaled_zeros"].astype(np.float64)[ic // g]
    w = qs + z
    out = cols >= kq
    if out.any():
        w[out] = bufs["oweight"].astype(np.float64)[:, cols[out] - kq].T
    return w, np.abs(qs), np.abs(z), out


PROBES = [(triple, bits) for triple in TIERS for bits in (4, 3)]


@pytest.mark.parametrize("triple,bits", PROBES, ids=[f"nw{t[0]}-rs{t[1]}-d{t[2]}-w{b}" for t, b in PROBES])
def test_column_probes(triple, bits):
    """x = e_j (1.0 in column j, no bias): the launch must return column j of the dense weight on every row, so one column that
    takes its neighbour's scale, nibble or step cannot hide in a sum over K.

    The bound, from the kernel's arithmetic (csrc/gemv_v3.h, step 4 and 5).  With x = e_j every product of the step's MFMAs is an
    integer below 2048 in fp32: P = 1 * (1024 + q) - 1024 * 1 = q (high nibbles: 1024 + 16 q, then * 0.0625), exactly; the bias sum is
    -1024 exactly; every other step and every other wave contributes exactly 0.  The fold is
        acc = fma(s, q, 0)                    -- 11 x 4 bits: exact, and at most half an ulp of fp32 if it were not: 2^-24 |q s|
        acc = fma(z * -2^-10, -1024, acc)     -- the product is z exactly; the sum rounds once: 2^-24 |w|, allow 2^-24 |z| for the product
    the waves' partial sums add zeros, rs_norm is 1, and y = fp16(acc): 2^-11 |w| (2^-25 below the fp16 normal range).  The reference
    is the unrounded w = q s + z in float64, so
        |y - w| <= 2^-11 |w| + 2^-24 (|q s| + |z| + |w|) + 2^-25.
    An outlier column's weight is an fp16 number that passes through one MFMA (times 1.0, plus zeros) and back to fp16: equal.
    The worst |y - w| / bound per instance is printed with the module's table."""
    from qeft_amd import _lib
    lib = _lib.lib()
    n, k = _cross_shape(triple)
    r, g = 128, 128
    bufs, t, _ = _layer(n, k, r, g, bits)
    cols = _probe_columns(k, r)
    assert len(cols) <= 2 * ((k - r) // 128) + 384
    x = torch.zeros(len(cols), k, dtype=torch.float16, device=DEV)
    x[torch.arange(len(cols), device=DEV), torch.from_numpy(cols).to(DEV)] = 1.0
    y = torch.full((len(cols), n), float("nan"), dtype=torch.float16, device=DEV)
    entry = lib.qeft_decode_linear_w3 if bits == 3 else lib.qeft_decode_linear
    want = triple + (1, PLAIN, bits, 0, 1, 0)
    for i in range(len(cols)):
        _lib.check(entry(x[i].data_ptr(), _p(t["qweight"]), _p(t["sz_packed"]), _p(t["oweight"]), None, y[i].data_ptr(), n, k, g, r, PLAIN, None,
                         None, 0, 0.0, None, None, None, _st()))
    assert _instance(_last_plan(lib)) == want
    torch.cuda.synchronize()
    got = y.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    w, aqs, az, out = _exact_columns(bufs, cols, k, r, g, bits)
    bound = 2.0 ** -11 * np.abs(w) + 2.0 ** -24 * (aqs + az + np.abs(w)) + 2.0 ** -25
    ratio = np.abs(got - w)[~out] / bound[~out]
    worst = float(ratio.max())
    i, row = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"[v3 probe] {triple} w{bits} {n}x{k}: {len(cols)} columns, worst |y - w| / bound {worst:.3f} (column {cols[~out][i]}, row {row})")
    _WORST_PROBE[want] = (worst, f"{n}x{k}")
    assert worst <= 1.0, (triple, bits, worst, int(cols[~out][i]), int(row))
    assert np.array_equal(got[out], w[out]), "an outlier column is the fp16 weight itself"
