"""Which launches of the v3 decode GEMV take a compile-time-K instance (csrc/gemv_v3_dispatch.h: V3_CTK, v3_ctk_pick, called by
gemv_v3_plan; queried through qeft_gemv_v3_plan_kct).  Host arithmetic, no GPU.

The instances are built for the Llama-2-7B and -13B launches of the decode engine and for nothing else: flag-free half, one batch
row, 4 bits, with the outlier step, and the (waves, ring depth, row sets, mode) the plan gives those shapes.  TABLE restates
them; the tests ask the library for each kind, for its neighbours in K, for every other form of launch on the same shapes, and
over a sweep of row-set counts and K that the answer is K exactly where the plan's instance and K are a row of TABLE."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, PAIR = 0, 1
PERCH, XN, SZN, OWIL, XG, GATHER = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 31

# kind -> (n, k, mode, (nw, D, rs_cap))
KINDS = {
    "7b-qkv": (12288, 4096, PLAIN, (8, 6, 3)), "7b-gate_up": (22016, 4096, PAIR, (4, 4, 3)), "7b-o_proj": (4096, 4096, PLAIN, (8, 2, 1)),
    "7b-down": (4096, 11008, PLAIN, (12, 2, 1)),
    "13b-qkv": (15360, 5120, PLAIN, (8, 6, 4)), "13b-gate_up": (27648, 5120, PAIR, (4, 4, 4)), "13b-o_proj": (5120, 5120, PLAIN, (8, 4, 2)),
    "13b-down": (5120, 13824, PLAIN, (8, 4, 2)),
}
TABLE = {(nw, d, rs, mode, k) for (_, k, mode, (nw, d, rs)) in KINDS.values()}


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def kct(lib, n, k, g=128, r=128, m=1, mode=PLAIN, bits=4, flags=0):
    return lib.qeft_gemv_v3_plan_kct(n, k, g, r, m, mode, bits, flags - (1 << 32) if flags >> 31 else flags)


def plan(lib, n, k, g=128, r=128, m=1, mode=PLAIN, bits=4, flags=0):
    out = (ctypes.c_int * 13)()
    assert lib.qeft_gemv_v3_plan(n, k, g, r, m, mode, bits, flags, out) == 0
    return tuple(out)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_engine_launches_take_their_instance(lib, kind):
    n, k, mode, (nw, d, rs) = KINDS[kind]
    p = plan(lib, n, k, mode=mode)
    assert (p[4], p[5], p[1], p[6], p[7], p[8], p[9], p[10], p[11]) == (nw, d, rs, 1, mode, 4, 0, 1, 0), p
    assert kct(lib, n, k, mode=mode) == k


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_everything_else_on_the_same_shape_keeps_the_run_time_k(lib, kind):
    n, k, mode, _ = KINDS[kind]
    for dk in (-128, 128):
        assert kct(lib, n, k + dk, mode=mode) == 0, dk
    assert kct(lib, n, k, mode=PAIR if mode == PLAIN else PLAIN) == 0          # the other mode's instance of this K is not built
    assert kct(lib, n, k, r=0, mode=mode) == 0                                  # no outlier step
    assert kct(lib, n, k, mode=mode, bits=3) == 0
    assert kct(lib, n, k, g=k, mode=mode) == 0                                  # per-channel scales: a flag
    assert kct(lib, n, k, mode=mode, flags=XN) == 0                             # the consumer-side norm
    for m in (2, 7, 8, 16):                                                     # batch rows (PLAIN only; the plan refuses m rows in PAIR mode)
        for flags in (0, SZN, SZN | OWIL, SZN | OWIL | GATHER, XG):
            assert kct(lib, n, k, m=m, mode=PLAIN, flags=flags) in (0, -1), (m, flags)
    for flags in (SZN, OWIL, SZN | OWIL, GATHER, SZN | OWIL | GATHER):          # checkpoint-layout operands, the gather
        assert kct(lib, n, k, mode=PLAIN, flags=flags) == 0, flags


def test_the_choice_is_the_table_over_a_sweep(lib):
    """Every row-set count that changes the grid rule, crossed with every K near a table K: compile-time K exactly where the plan's
    (waves, ring, row sets, mode) and K form a row of TABLE."""
    nsets_all = sorted(set(range(1, 40)) | {t + d for t in (240, 256, 320, 432, 459, 512, 768, 960, 1024, 1152, 1376, 1728) for d in (-1, 0, 1)})
    ks = sorted({k + d for k in (4096, 5120, 11008, 13824) for d in (-256, -128, 0, 128, 256)} | {256, 1024, 8192, 16384})
    hits = set()
    for nsets in nsets_all:
        for k in ks:
            for mode in (PLAIN, PAIR):
                for r in (0, 128):
                    p = plan(lib, nsets * 16, k, r=r, mode=mode)
                    want = k if r and (p[4], p[5], p[1], mode, k) in TABLE else 0
                    got = kct(lib, nsets * 16, k, r=r, mode=mode)
                    assert got == want, (nsets, k, mode, r, p, got)
                    if got:
                        hits.add((p[4], p[5], p[1], mode, k))
    assert hits == TABLE


def test_the_query_refuses_what_the_plan_refuses(lib):
    assert kct(lib, 24, 4096) == -1 and kct(lib, 16, 4096, r=64) == -1 and kct(lib, 4096, 4096, m=17) == -1
    assert kct(lib, 4096, 4096, m=2, mode=PAIR) == -1


def test_the_environment_switch_keeps_every_launch_on_the_run_time_k():
    """QEFT_GEMV_CTK=0 is read once per process, like the other overrides of the plan: asked of a child."""
    src = ("import sys; sys.path.insert(0, %r)\nfrom qeft_amd import _lib\nl = _lib.lib()\n"
           "print([l.qeft_gemv_v3_plan_kct(n, k, 128, 128, 1, mode, 4, 0) for n, k, mode in %r])") % (ROOT, [v[:3] for v in KINDS.values()])
    for value, want in (("0", [0] * len(KINDS)), ("1", [v[1] for v in KINDS.values()])):
        out = subprocess.run([sys.executable, "-c", src], env=dict(os.environ, QEFT_GEMV_CTK=value), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip() == repr(want), (value, out.stdout, out.stderr[-2000:])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_address_enumeration_at_the_compiled_k(lib, kind):
    """The compile-time-K instances form their addresses with the functions the enumerator walks (tests/test_gemv_v3_extents.py), now
    folded by the compiler: every access of the kind's launch stays inside its operand, with the engine's partial sums of squares and
    with a small grid of the same K (the shapes of tests/test_gpu_gemv_v3_ctk.py), and the negative control still counts."""
    n, k, _, _ = KINDS[kind]
    for rows in (n, 16, 32, 80, 96):
        for n_ssq in (0, 300, 512):
            assert lib.qeft_gemv_v3_check_extents(rows, k, 128, 128, n_ssq, 0) == 0, (rows, k, n_ssq)
    assert lib.qeft_gemv_v3_check_extents(n, k, 128, 128, 0, 16) > 0
