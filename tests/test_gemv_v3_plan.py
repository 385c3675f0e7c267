"""The plan of the v3 decode GEMV launcher (csrc/gemv_v3.hip gemv_v3_plan) against an independent
restatement, and the census of its instances against the pinned GPU cases.

gemv_v3_launch chooses between the 232 instantiations of one kernel template that it and gemv_v3_plain.hip build (and the 8 with a
compile-time K, tests/test_gemv_v3_ctk_plan.py), gemv_v3_multi_launch between the 48 of the engine's m-row family
(gemv_v3_multi.hip), and qeft_last_variant calls all of the former "gemv_v3" and the latter "gemv_v3_multi".  qeft_gemv_v3_plan says which one a launch would run: host arithmetic, no GPU.  Below, the rules are written down a
second time in plain Python -- blocks, waves, ring depth, the template's D, the half, the LDS bytes, the refusals -- and compared
with the library over a sweep; then the set of instances the sweep reaches must be exactly the set that
tests/test_gpu_gemv_v3_tiers.py pins to a shape, and the instances that are built but that no shape reaches must be exactly
UNREACHABLE.

The sweep.  The geometry of a plan is a function of (nsets, nfull, m > 1, xg) alone; mode and bits pass through, and the flags
enter the half, the LDS bytes and the refusals.  So
  * every nsets of 1..1300 and {1376, 1536, 1792, 2048, 3001, 3584} is crossed with every K of 128..16384 and both n_out for the
    one-row PLAIN 4-bit launch without flags (334 336 queries), and
  * m, mode, bits and the flags are crossed with each other, with both n_out, with the K next to every value of nfull at which
    ceil(nfull / waves) * RSC can pass 8 or nfull passes 64 (K_EDGE), and with the nsets next to every threshold of the blocks rule
    plus every 16th one and the six large ones (NSETS_EDGE);
  * per-channel scales (group_size == K) are crossed with NSETS_EDGE, every K, both n_out and m of 1 and 2;
  * the engine's m-row family (ENGINE_M, with and without XG) is crossed with m of 2, 5, 8 and the refused 1 and 9, both modes, both
    n_out, NSETS_EDGE and K_EDGE, and at m = 2 with 3 bits, each run-time flag and per-channel scales (all refused).
The full product of all axes would be some 10^8 queries."""
import ctypes
import functools

import pytest

PLAN = ("nblk", "rs_cap", "sets_q", "sets_r", "nw", "D", "outl", "mode", "bits", "fl", "mb", "xg", "smem")
PERCH, XN, SZN, OWIL, XG, ENGINE_M, GATHER = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 29, 1 << 31
PLAIN, PAIR = 0, 1

NSETS = list(range(1, 1301)) + [1376, 1536, 1792, 2048, 3001, 3584]
KS = list(range(128, 16384 + 1, 128))
MS = (1, 2, 7, 8, 9, 16)
MS_ENGINE = (1, 2, 5, 8, 9)       # the engine's m-row launches take 2..8
NSETS_EDGE = sorted({t + d for t in (256, 512, 1024, 1152) for d in (-2, -1, 0, 1, 2)} | set(NSETS[::16]) | set(NSETS[-6:]) | {1300})
NFULL_EDGE = (1, 7, 8, 9, 16, 17, 24, 25, 32, 33, 56, 57, 63, 64, 65, 84, 85, 96, 127)
K_EDGE = sorted({(f + d) * 128 for f in NFULL_EDGE for d in (0, 1)})
FLAG_SETS = (0, XN, SZN, OWIL, GATHER, XG, SZN | OWIL, SZN | OWIL | GATHER)

# Instances (nw, rs_cap, D) that gemv_v3_dispatch.h instantiates for every (outl, mode, bits, fl) and that no shape reaches:
UNREACHABLE = {
    (4, 1, 4): "4-wave blocks need more than 256 blocks; gemv_v3_blocks gives more than 256 only from 512 row sets on, where a "
               "block holds ceil(nsets / (256 k)) >= 2 sets, and evening the load (ceil(nsets / RS) blocks) keeps RS",
    (4, 2, 4): "two sets per block above 256 blocks would need 513 .. 767 row sets on 512 blocks, but 512 blocks are chosen from "
               "(nsets + 384) / 768 = 2, that is from 1152 row sets on: three sets per block; QEFT_GEMV_NW=4 / QEFT_GEMV_BLOCKS reach both",
}
# What launch_d can be asked for and refuses (no instantiation behind it): 12-wave blocks with more than one row set.  The plan never
# asks: 12 waves are chosen only with rs_cap == 1.
REFUSED_BY_DISPATCH = [(12, rs) for rs in (2, 3, 4)]


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the restatement
def _cd(a, b):
    return -(-a // b)


def _up1k(v):
    return _cd(v, 1024) * 1024


@functools.lru_cache(maxsize=None)
def blocks(nsets):
    """One set per block up to 256; two per block under 512; then about 256 k blocks of ~3 sets, at most 4 sets per block, and as
    few blocks as carry the fullest block's count."""
    if nsets <= 256:
        return nsets
    if nsets < 512:
        return _cd(nsets, 2)
    nblk = 256 * max((nsets + 384) // 768, 1)
    if _cd(nsets, nblk) > 4:
        nblk = _cd(nsets, 4)
    return _cd(nsets, _cd(nsets, nblk))


def lds_bytes(k, ngroups, n_out, rs, m, nw, xn, szn, gather, xg):
    xb = _up1k(2 * k)
    red = _up1k(rs * nw * (16 if m > 8 else 8) * 16 * 4) if m > 1 else _up1k(rs * 16 * 16 * 4 + 64)
    total = 0 if xg else _up1k(m * (xb + (16 if m > 1 else 0)))
    total += rs * _up1k(64 * ngroups) + (rs * 4096 if n_out else 0) + 1024 + 2048 + red
    total += (_up1k(4 * k) + xb) if xn else 0
    total += 2 * rs * _up1k(32 * ngroups) if szn else 0
    total += (_up1k(4 * k) + m * xb) if gather else 0
    return total


def restated_plan(nsets, k, g, n_out, m, mode, bits, flags):
    """The 13 integers of qeft_gemv_v3_plan, or None where the launcher refuses."""
    if k % 128 or k < 128 or g not in (128, k) or not (n_out == 0 or (n_out == 128 and k > 128)):
        return None
    perch = g == k and k > 128
    if (flags & PERCH and not perch) or (flags & OWIL and not n_out):
        return None
    xn, szn, gather, xg, em = bool(flags & XN), bool(flags & SZN), bool(flags & GATHER), bool(flags & XG), bool(flags & ENGINE_M)
    if m > 16 or (m > 1 and ((mode == PAIR and not em) or bits == 3 or xn)) or (xg and (m == 1 or gather)) or (szn and xn):
        return None
    # the engine's m-row launches: 2..8 rows, 4 bits, no run-time flag; PLAIN or PAIR on the flag-free MB = 2 instances
    if em and (not 2 <= m <= 8 or bits == 3 or perch or flags & (XN | SZN | OWIL | GATHER)):
        return None
    nfull, ngroups = (k - n_out) // 128, 1 if g == k else k // 128
    nblk = blocks(nsets)
    rs = _cd(nsets, nblk)
    nw = 4 if nblk > 256 and m == 1 else 8
    if m == 1 and nblk <= 256 and rs == 1 and nfull >= 64:
        nw = 12
    deep = xg or (nblk <= 256 and _cd(nfull, nw) * rs >= 8)
    d = 4 if nw == 4 else 2 if nw == 12 else (6 if rs >= 3 else 4) if deep else 2
    fl = int(not em and (m > 1 or perch or (flags & (XN | SZN | OWIL | GATHER)) != 0))
    smem = lds_bytes(k, ngroups, n_out, rs, m, nw, xn, szn, gather, xg)
    if smem > 160 * 1024 or nblk >= 65536:
        return None
    return (nblk, rs, nsets // nblk, nsets % nblk, nw, d, int(n_out > 0), mode, bits, fl, 2 if m > 1 else 1, int(xg), smem)


def instance(p):
    """The template arguments of a plan: (nw, rs_cap, D, outl, mode, bits, fl, mb, xg)."""
    return p[4], p[1], p[5], p[6], p[7], p[8], p[9], p[10], p[11]


def query(lib, nsets, k, g, n_out, m, mode, bits, flags, _out=(ctypes.c_int * len(PLAN))()):
    rc = lib.qeft_gemv_v3_plan(nsets * 16, k, g, n_out, m, mode, bits, flags - (1 << 32) if flags >> 31 else flags, _out)
    assert rc in (0, -1), rc
    return tuple(_out) if rc == 0 else None


def sweep():
    """(nsets, k, g, n_out, m, mode, bits, flags) of every query of the module."""
    for nsets in NSETS:
        for k in KS:
            for n_out in (0, 128):
                yield nsets, k, 128, n_out, 1, PLAIN, 4, 0
    for nsets in NSETS_EDGE:
        for k in K_EDGE:
            for n_out in (0, 128):
                for m in MS:
                    for mode in (PLAIN, PAIR):
                        for bits in (4, 3):
                            for flags in FLAG_SETS:
                                yield nsets, k, 128, n_out, m, mode, bits, flags
        for k in KS:
            for n_out in (0, 128):
                for m in (1, 2):
                    yield nsets, k, k, n_out, m, PLAIN, 4, 0
                for mode, bits in ((PAIR, 4), (PLAIN, 3), (PAIR, 3)):
                    yield nsets, k, k, n_out, 1, mode, bits, 0
        for k in K_EDGE:
            for n_out in (0, 128):
                for mode in (PLAIN, PAIR):
                    for flags in (ENGINE_M, ENGINE_M | XG):
                        for m in MS_ENGINE:
                            yield nsets, k, 128, n_out, m, mode, 4, flags
                        yield nsets, k, 128, n_out, 2, mode, 3, flags
                        yield nsets, k, k, n_out, 2, mode, 4, flags
                        for f in (XN, SZN, OWIL, GATHER):
                            yield nsets, k, 128, n_out, 2, mode, 4, flags | f


@pytest.fixture(scope="module")
def reached(lib):
    """instance -> the first query that reached it, for the whole sweep; every answer compared with the restatement on the way."""
    seen, bad, n, refused = {}, [], 0, 0
    for q in sweep():
        got, want = query(lib, *q), restated_plan(*q)
        n += 1
        refused += got is None
        if got != want:
            bad.append((q, got, want))
        elif got is not None:
            seen.setdefault(instance(got), q)
    assert not bad, (len(bad), bad[:5])
    assert n > 1_500_000 and refused > 100_000 and n - refused > 500_000, (n, refused)      # (batch rows in PAIR mode, with 3 bits, with XN: refused)
    return seen


# --------------------------------------------------------------------------------------------------------- tests
def test_the_plan_is_the_restatement_over_the_sweep(reached):
    assert len(reached) >= 100


def test_the_issue_table_of_smallest_shapes(lib):
    """The smallest shape of every (nw, rs_cap, D) of the one-row PLAIN 4-bit launch with n_out = 128, with its blocks, sets_r and
    nfull: found by walking n upwards and K upwards, compared with the table DESIGN.md prints."""
    want = {(8, 1, 2): (16, 256, 1, 0), (8, 1, 4): (16, 7424, 1, 0), (12, 1, 2): (16, 8320, 1, 0), (8, 2, 2): (4112, 256, 129, 128),
            (8, 2, 4): (4112, 3328, 129, 128), (8, 3, 2): (8208, 256, 171, 0), (8, 3, 6): (8208, 2304, 171, 0),
            (8, 4, 2): (12304, 256, 193, 190), (8, 4, 6): (12304, 1280, 193, 190), (4, 3, 4): (18432, 256, 384, 0),
            (4, 4, 4): (16400, 256, 257, 254)}
    first = {}
    for nsets in NSETS:
        for k in KS[1:]:
            p = query(lib, nsets, k, 128, 128, 1, PLAIN, 4, 0)
            if p is not None:
                first.setdefault((p[4], p[1], p[5]), (nsets * 16, k, p[0], p[3]))
    assert first == want


def test_census_every_reachable_instance_has_a_pinned_gpu_case(reached):
    """The instances the sweep reaches == the instances the tables of tests/test_gpu_gemv_v3_tiers.py name: a new threshold, a new
    instantiation or a newly reachable one cannot arrive without a case that asserts it ran and compares it with float64."""
    import test_gpu_gemv_v3_tiers as tiers
    pinned = tiers.pinned_instances()
    missing = sorted(set(reached) - set(pinned))
    stale = sorted(set(pinned) - set(reached))
    assert not missing, ("reachable, no pinned case", len(missing), [(i, reached[i]) for i in missing[:8]])
    assert not stale, ("pinned, but the sweep does not reach it", len(stale), [(i, pinned[i]) for i in stale[:8]])


def test_every_pinned_case_is_what_the_plan_says(lib):
    """Each row of the GPU tables, asked of the plan on the CPU: the expected tuple is the plan's, so a table that has drifted from
    the launcher fails here and not only on a GPU."""
    import test_gpu_gemv_v3_tiers as tiers
    cases = tiers.all_cases()
    assert len(cases) >= 200
    for c in cases:
        p = query(lib, c.n // 16, c.k, c.g, c.r, c.m, c.mode, c.bits, c.flags)
        assert p is not None and instance(p) == c.want and p[0] == tiers.blocks_of(c) and restated_plan(c.n // 16, c.k, c.g, c.r, c.m, c.mode, c.bits, c.flags) == p, (c, p)
        if c.entry == "engine_m":       # qeft_decode_linear_m asks without XG first: an xg case is one that this refuses, and no other
            assert (query(lib, c.n // 16, c.k, c.g, c.r, c.m, c.mode, c.bits, ENGINE_M) is None) == bool(c.flags & XG), c


def test_the_unreachable_list_is_exact(reached):
    """Built (gemv_v3_dispatch.h names them) and never reached: exactly UNREACHABLE.  The build keeps them for the lab overrides."""
    built = {(4, rs, 4) for rs in (1, 2, 3, 4)} | {(12, 1, 2)} | {(8, rs, d) for rs in (1, 2, 3, 4) for d in (2, 6 if rs >= 3 else 4)}
    got = {i[:3] for i in reached}
    assert got <= built and built - got == set(UNREACHABLE), (sorted(built - got), sorted(got - built))
    assert not {(nw, rs) for nw, rs, _ in got} & set(REFUSED_BY_DISPATCH)
    # every one-row instance exists in both halves, both modes, both widths, with and without the outlier step
    for t in got:
        assert {i[3:] for i in reached if i[:3] == t and i[7] == 1} == {(o, md, b, f, 1, 0) for o in (0, 1) for md in (0, 1) for b in (4, 3) for f in (0, 1)}, t
    # several batch rows: 8 waves, 4 bits, PLAIN, the flagged half; xg on the deep rings only
    mb = {i for i in reached if i[7] == 2 and i[6] == 1}
    assert mb == {(8, rs, d, o, 0, 4, 1, 2, x) for rs in (1, 2, 3, 4) for d in (2, 6 if rs >= 3 else 4) for o in (0, 1) for x in (0, 1)
                  if not (x and d == 2)}
    # the engine's m-row family: the same geometries on the flag-free half, PLAIN and PAIR: the 48 instances of gemv_v3_multi.hip
    em = {i for i in reached if i[7] == 2 and i[6] == 0}
    assert em == {(8, rs, d, o, md, 4, 0, 2, x) for rs in (1, 2, 3, 4) for d in (2, 6 if rs >= 3 else 4) for o in (0, 1) for md in (0, 1)
                  for x in (0, 1) if not (x and d == 2)} and len(em) == 48


def test_the_query_refuses_what_the_launcher_refuses(lib):
    out = (ctypes.c_int * len(PLAN))()
    q = lib.qeft_gemv_v3_plan
    assert q(16, 256, 128, 128, 1, 0, 4, 0, None) == 4                     # QEFT_ERR_NULL
    assert q(16, 256, 128, 128, 1, 0, 4, 0, out) == 0 and tuple(out) == (1, 1, 1, 0, 8, 2, 1, 0, 4, 0, 1, 0, lds_bytes(256, 2, 128, 1, 1, 8, 0, 0, 0, 0))
    for bad in ((24, 256, 128, 128, 1, 0, 4, 0), (16, 192, 64, 0, 1, 0, 4, 0), (16, 256, 64, 0, 1, 0, 4, 0), (16, 128, 128, 128, 1, 0, 4, 0),
                (16, 512, 128, 256, 1, 0, 4, 0), (16, 256, 128, 0, 0, 0, 4, 0), (16, 256, 128, 0, 17, 0, 4, 0), (16, 256, 128, 0, 1, 2, 4, 0),
                (16, 256, 128, 0, 1, 0, 5, 0), (16, 256, 128, 0, 1, 0, 4, 1 << 20), (16, 256, 128, 0, 1, 0, 4, PERCH), (16, 256, 128, 0, 1, 0, 4, OWIL),
                (16, 256, 128, 0, 2, 1, 4, 0), (16, 256, 128, 0, 2, 0, 3, 0), (16, 256, 128, 0, 2, 0, 4, XN), (16, 256, 128, 0, 1, 0, 4, XG),
                (16, 256, 128, 0, 2, 0, 4, XG | GATHER - (1 << 32)), (16, 256, 128, 0, 1, 0, 4, XN | SZN), (16, 16384, 128, 0, 16, 0, 4, 0),
                (16 * 4 * 65536, 256, 128, 0, 1, 0, 4, 0)):
        assert q(*bad, out) == -1, bad
    assert q(16, 16384, 128, 0, 16, 0, 4, XG, out) == 0 and out[11] == 1 and out[5] == 4      # the x rows leave the LDS: it fits
    # the engine's m-row launches: two PAIR rows on the flag-free half; refused: 1 and 9 rows, 3 bits, per-channel scales, every
    # run-time flag, a bit that is neither flag nor plan bit, x rows that do not fit the LDS (taken with XG)
    assert q(16, 256, 128, 128, 2, 1, 4, ENGINE_M, out) == 0 and tuple(out) == (1, 1, 1, 0, 8, 2, 1, 1, 4, 0, 2, 0, lds_bytes(256, 2, 128, 1, 2, 8, 0, 0, 0, 0))
    for bad in ((16, 256, 128, 128, 1, 0, 4, ENGINE_M), (16, 256, 128, 128, 9, 0, 4, ENGINE_M), (16, 256, 128, 128, 2, 0, 3, ENGINE_M),
                (16, 256, 256, 128, 2, 0, 4, ENGINE_M), (16, 256, 128, 128, 2, 0, 4, ENGINE_M | XN), (16, 256, 128, 128, 2, 0, 4, ENGINE_M | SZN),
                (16, 256, 128, 128, 2, 0, 4, ENGINE_M | OWIL), (16, 256, 128, 128, 2, 0, 4, (ENGINE_M | GATHER) - (1 << 32)),
                (16, 256, 128, 128, 1, 0, 4, ENGINE_M | XG), (16, 256, 128, 128, 2, 0, 4, ENGINE_M | 1 << 30), (16, 11008, 128, 128, 8, 0, 4, ENGINE_M)):
        assert q(*bad, out) == -1, bad
    assert q(16, 11008, 128, 128, 8, 0, 4, ENGINE_M | XG, out) == 0 and out[11] == 1 and out[5] == 4 and out[9] == 0


def test_the_last_plan_query_needs_no_gpu(lib):
    """The record is per thread, as qeft_last_variant: a thread that has launched nothing reads zeros, and the plan query leaves
    the record alone."""
    import threading
    assert lib.qeft_gemv_v3_last_plan(None) == 4
    seen = []

    def fresh_thread():
        out = (ctypes.c_int * len(PLAN))(*([7] * len(PLAN)))
        assert lib.qeft_gemv_v3_plan(16, 256, 128, 128, 1, 0, 4, 0, out) == 0 and out[0] == 1
        seen.append((lib.qeft_gemv_v3_last_plan(out), tuple(out)))
    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert seen == [(0, (0,) * len(PLAN))]
