"""The plan of the engine's m-row v3 GEMV launches (gemv_v3_plan under V3_PLAN_ENGINE_M) against a
recorded table.

tests/golden/gemv_v3_multi_plan_parent.npz holds what gemv_v3_multi_launch did BEFORE it asked gemv_v3_plan, when it had a planner
and a dispatch ladder of its own: that file run on a CPU with the launch macro replaced by a recorder
(profiles/gemv_v3_one_plan_refactor.log has the commands).  One row per call: the inputs (n, k, n_out, m, mode), ok (0: refused),
the grid and the two packed geometry dwords taken apart (nblk, rs_cap, sets_q, sets_r), the template arguments of the kernel it
launched (nw, D, outl, kmode, bits, mb, fl, xg, kct), the dynamic LDS bytes, the value it gave hipFuncSetAttribute (-1: no call)
and the block size.  The rows are the twelve Llama-2 7B / 13B / 70B engine shapes and a ninth of a sweep over the thresholds of
the blocks rule x the K next to every ring threshold x both n_out x m = 2..8 x both modes, with every instance at every m.

The launcher asks the plan without XG and, where that is refused, with it; the test does the same through the C ABI.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XG, ENGINE_M = 1 << 28, 1 << 29
PLAN = ("nblk", "rs_cap", "sets_q", "sets_r", "nw", "D", "outl", "mode", "bits", "fl", "mb", "xg", "smem")
ENGINE_SHAPES = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (15360, 5120), (5120, 5120), (27648, 5120), (5120, 13824),
                 (10240, 8192), (8192, 8192), (57344, 8192), (8192, 28672)]


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def table():
    z = np.load(os.path.join(ROOT, "tests", "golden", "gemv_v3_multi_plan_parent.npz"))
    cols = [str(c) for c in z["columns"]]
    return [dict(zip(cols, map(int, r))) for r in z["rows"]]


def _plan(lib, row):
    """What the launcher would run for the row's inputs: the plan without XG, else with it; None where both refuse."""
    out = (ctypes.c_int * len(PLAN))()
    for flags in (ENGINE_M, ENGINE_M | XG):
        rc = lib.qeft_gemv_v3_plan(row["n"], row["k"], 128, row["n_out"], row["m"], row["mode"], 4, flags, out)
        assert rc in (0, -1), (rc, row)
        if rc == 0:
            p = dict(zip(PLAN, out))
            p["kct"] = lib.qeft_gemv_v3_plan_kct(row["n"], row["k"], 128, row["n_out"], row["m"], row["mode"], 4, flags)
            return p
    return None


def _mismatch(row, p):
    """What of the recorded launch the plan does not reproduce ('' when it reproduces all of it)."""
    if (p is not None) != bool(row["ok"]):
        return f"ok {int(p is not None)} != {row['ok']}"
    if p is None:
        return ""
    want = {c: row[c] for c in ("nblk", "rs_cap", "sets_q", "sets_r", "nw", "D", "outl", "bits", "fl", "mb", "xg", "smem", "kct")}
    want["mode"] = row["kmode"]
    bad = [f"{c} {p[c]} != {v}" for c, v in want.items() if p[c] != v]
    if row["attr"] != (p["smem"] if p["smem"] > 64 * 1024 else -1):
        bad.append(f"hipFuncSetAttribute {row['attr']} for {p['smem']} bytes")
    if row["block"] != p["nw"] * 64:
        bad.append(f"block {row['block']}")
    return "; ".join(bad)


def test_the_plan_reproduces_the_recorded_launches(lib, table):
    assert len(table) >= 10000
    bad = [(m, row) for row in table for m in [_mismatch(row, _plan(lib, row))] if m]
    assert not bad, (len(bad), bad[:5])


def test_an_altered_row_fails_the_comparison(lib, table):
    """Negative control: the comparison is not vacuous."""
    row = next(r for r in table if r["ok"] and r["D"] == 6 and not r["xg"])
    assert _mismatch(row, _plan(lib, row)) == ""
    assert "D 6 != 2" in _mismatch(dict(row, D=2), _plan(lib, row))
    assert "xg 0 != 1" in _mismatch(dict(row, xg=1), _plan(lib, row))
    assert "rs_cap" in _mismatch(dict(row, rs_cap=row["rs_cap"] % 4 + 1), _plan(lib, row))
    assert "smem" in _mismatch(dict(row, smem=row["smem"] + 1024), _plan(lib, row))
    assert _mismatch(dict(row, ok=0), _plan(lib, row)).startswith("ok")
    refused = next(r for r in table if not r["ok"])
    assert _mismatch(refused, _plan(lib, refused)) == "" and _mismatch(dict(refused, ok=1), _plan(lib, refused)).startswith("ok")


def test_the_table_covers_the_family(table):
    """All 48 instances, each at every m of 2..8 its x source allows; every engine shape at every m, in both modes, with and
    without outliers; refusals of the row count and of the block count."""
    ok = [r for r in table if r["ok"]]
    inst = {(r["nw"], r["rs_cap"], r["D"], r["outl"], r["kmode"], r["bits"], r["fl"], r["mb"], r["xg"], r["kct"]) for r in ok}
    assert inst == {(8, rs, d, o, md, 4, 0, 2, x, 0) for rs in (1, 2, 3, 4) for d in (2, 6 if rs >= 3 else 4) for o in (0, 1) for md in (0, 1)
                    for x in (0, 1) if not (x and d == 2)}
    for x in (0, 1):
        for rs in (1, 2, 3, 4):
            assert {r["m"] for r in ok if r["xg"] == x and r["rs_cap"] == rs} >= set(range(5 if x else 2, 9)), (x, rs)
    seen = {(r["n"], r["k"], r["n_out"], r["m"], r["mode"]) for r in ok}
    assert seen >= {(n, k, o, m, md) for n, k in ENGINE_SHAPES for o in (0, 128) for m in range(2, 9) for md in (0, 1)}
    refused = [r for r in table if not r["ok"]]
    assert {r["m"] for r in refused} >= {0, 1, 9} and any(r["n"] >= 16 * 4 * 65536 for r in refused)
