"""The launch plans of the GEMM forward, dX and d(oweight) (csrc/gemm_w4.h) against a recorded table.

tests/golden/gemm_plan_parent.npz holds what the launchers did BEFORE the plans existed: the ladder of gemm_w4.hip as it then
was, run on a CPU with the launch macro replaced by a recorder (profiles/gemm_plan_refactor.log has the commands), over the
case tables of tests/test_gpu_gemm_tiers.py, sweeps across every threshold of the ladder (tile counts, k-tiles, LDS sizes,
divisibility of N and n_out, group sizes, workspace absent / exact / one byte short / ample) and every value of every override.
`rows` is one launch per line with the columns named in `columns` (variant: an index into `variants`, -1 where the launcher
answered hipErrorNotSupported), `workspace_bytes` the size it was given (-1: a NULL workspace).

The plan entries of the C ABI make no HIP call, so all of this runs without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import test_variant_census as census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, DX, DOW = 0, 1, 2
OV = ["ov_gemm_v3", "ov_gemm_v3m", "ov_gemm_v3s", "ov_gemm_nwv", "ov_dx_v3", "ov_dow_bn", "ov_gemm_abl", "ov_gemm_v1"]
PLAN = ("tier", "gx", "gy", "gz", "threads", "lds", "S", "reduce", "fused", "supported")


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def table():
    z = np.load(os.path.join(ROOT, "tests", "golden", "gemm_plan_parent.npz"))
    cols = [str(c) for c in z["columns"]]
    rows = [dict(zip(cols, map(int, r)), ws=int(w)) for r, w in zip(z["rows"], z["workspace_bytes"])]
    return rows, [str(v) for v in z["variants"]]


def _plan(lib, row):
    """The plan of the row's launcher for the row's inputs, as a dict, with the tier's name."""
    out = (ctypes.c_int * len(PLAN))()
    ov = (ctypes.c_int * len(OV))(*[row[c] for c in OV])
    ws = max(row["ws"], 0)
    if row["kind"] == FWD:
        rc = lib.qeft_gemm_w4_plan(row["m"], row["n"], row["k"], row["g"], row["n_out"], row["bits"], row["gate"], ws, ov, out)
    elif row["kind"] == DX:
        rc = lib.qeft_gemm_w4_dx_plan(row["m"], row["n"], row["k"], row["g"], row["n_out"], row["bits"], ws, ov, out)
    else:
        rc = lib.qeft_grad_oweight_plan(row["n"], row["k"], row["n_out"], ov, out)
    assert rc == 0, (rc, row)
    p = dict(zip(PLAN, out))
    p["name"] = lib.qeft_gemm_tier_name(p["tier"]).decode()
    return p


def _mismatch(row, variants, p):
    """What of the recorded launch the plan does not reproduce ('' when it reproduces all of it)."""
    if p["supported"] != row["supported"]:
        return f"supported {p['supported']} != {row['supported']}"
    if not row["supported"]:
        return "" if p["name"] == "" else f"a tier ({p['name']}) on an unsupported shape"
    want = dict(name=variants[row["variant"]], **{c: row[c] for c in ("gx", "gy", "gz", "threads", "lds", "S", "reduce", "fused")})
    return "; ".join(f"{c} {p[c]} != {v}" for c, v in want.items() if p[c] != v)


def test_the_plans_reproduce_the_recorded_launches(lib, table):
    rows, variants = table
    assert len(rows) >= 5000
    bad = [(m, row) for row in rows for m in [_mismatch(row, variants, _plan(lib, row))] if m]
    assert not bad, (len(bad), bad[:5])


def test_a_row_with_another_variant_fails_the_comparison(lib, table):
    """Negative control: the comparison is not vacuous."""
    rows, variants = table
    row = next(r for r in rows if r["supported"] and variants[r["variant"]] == "gemm_v3_128x128")
    assert _mismatch(row, variants, _plan(lib, row)) == ""
    altered = dict(row, variant=variants.index("gemm_v2_128x128"))
    assert "name gemm_v3_128x128 != gemm_v2_128x128" in _mismatch(altered, variants, _plan(lib, altered))
    assert "S 1 != 2" in _mismatch(dict(row, S=2), variants, _plan(lib, row))
    assert _mismatch(dict(row, supported=0), variants, _plan(lib, row)).startswith("supported")


def test_the_name_query_leaves_the_last_variant_alone(lib):
    """qeft_gemm_tier_name reads the table the launchers set qeft_last_variant from; asking is not launching."""
    before = lib.qeft_last_variant()
    assert lib.qeft_gemm_tier_name(1) == b"gemm_v1" and lib.qeft_gemm_tier_name(0) == b"" and lib.qeft_gemm_tier_name(99) == b""
    assert lib.qeft_last_variant() == before and b"gemm_v1" != before


def test_the_table_covers_the_ladder(table):
    """Every name gemm_w4.hip can report, every value of every override, every gate kind and bit width, every kind of workspace."""
    rows, variants = table
    names = {n for n, where in census._variants_in_csrc().items() if where.startswith("gemm_w4.hip:")}
    assert len(names) == 21 and names == {variants[r["variant"]] for r in rows if r["supported"]}
    values = {c: {r[c] for r in rows} for c in OV + ["gate", "bits", "kind"]}
    assert values["ov_gemm_v3"] >= {-1, 0, 1} and values["ov_gemm_v3m"] >= {-1, 0, 1} and values["ov_gemm_v3s"] >= {-1, 0}
    assert values["ov_gemm_nwv"] >= {0, 4, 8} and values["ov_dx_v3"] >= {-1, 0, 1} and values["ov_dow_bn"] >= {0, 32, 64}
    assert values["ov_gemm_abl"] >= set(range(7)) and values["ov_gemm_v1"] == {0, 1}
    assert values["gate"] == {0, 1, 2} and values["bits"] == {3, 4} and values["kind"] == {FWD, DX, DOW}
    for kind, size in ((FWD, lambda r: r["m"] * r["n"] * 4), (DX, lambda r: r["m"] * r["k"] * 4)):
        split = [r for r in rows if r["kind"] == kind and r["reduce"]]
        assert any(r["ws"] == r["S"] * size(r) for r in split) and any(r["ws"] > 2 * r["S"] * size(r) for r in split)      # exact, ample
        mine = [r for r in rows if r["kind"] == kind]
        assert any(r["ws"] == -1 for r in mine) and any(r["ws"] % 4 == 3 for r in mine)                                     # absent, one short


def test_the_tier_tables_are_in_the_table(table):
    """Every row of the FWD, DX and DOW case tables of tests/test_gpu_gemm_tiers.py is a recorded launch.  (FWD rows of up to 64
    rows name the tier gemm_impl routes them to before the launcher is asked; the record is the launcher's own answer.)"""
    import test_gpu_gemm_tiers as tiers
    rows, variants = table
    default = [r for r in rows if all(r[c] == u for c, u in zip(OV, (-1, -1, -1, 0, -1, 0, 0, 0)))]
    fwd = {(r["m"], r["n"], r["k"], r["n_out"], r["g"]): variants[r["variant"]] for r in default
           if r["kind"] == FWD and r["bits"] == 4 and r["gate"] == 0 and r["ws"] > 1 << 39}
    for m, n, k, r_, g, want, _ in tiers.FWD:
        assert (m, n, k, r_, g) in fwd, (m, n, k, r_, g)
        if m > 64:
            assert fwd[(m, n, k, r_, g)] == want, (m, n, k, r_, g)
    dx = {(r["m"], r["n"], r["k"], r["n_out"], r["g"], r["bits"]): variants[r["variant"]] for r in default if r["kind"] == DX and r["ws"] > 1 << 39}
    for m, n, k, r_, g, bits, want, _ in tiers.DX:
        assert dx.get((m, n, k, r_, g, bits)) == want, (m, n, k, r_, g, bits)
    dow = {(r["n"], r["k"], r["n_out"]): variants[r["variant"]] for r in default if r["kind"] == DOW}
    for m, n, k, r_, want, _ in tiers.DOW:
        assert dow.get((n, k, r_)) == want, (n, k, r_)


def test_the_support_queries_agree_with_the_plans(lib, table):
    """qeft_gemm_w3_supported, qeft_gemm_w3_dx_supported and qeft_gemm_w4_gateup_supported on every row of their kind (the
    gate|up query also applies check_common: rows it would refuse on those grounds are not its kind)."""
    rows, _ = table
    seen = {"w3": 0, "w3_dx": 0, "gateup": 0}
    for row in rows:
        m, n, k, g, r = (row[c] for c in ("m", "n", "k", "g", "n_out"))
        if row["kind"] == FWD and row["bits"] == 3 and row["gate"] == 0:
            assert lib.qeft_gemm_w3_supported(m, n, k, g, r) == _plan(lib, row)["supported"], row
            seen["w3"] += 1
        elif row["kind"] == DX and row["bits"] == 3:
            assert lib.qeft_gemm_w3_dx_supported(m, n, k, g, r) == _plan(lib, row)["supported"], row
            seen["w3_dx"] += 1
        elif row["kind"] == FWD and row["bits"] == 4 and row["gate"] == 2 and n % 4 == 0 and k % 64 == 0 and g % 32 == 0 and k % g == 0 \
                and r % 32 == 0 and r < k and (r == 0 or n % 8 == 0):
            assert lib.qeft_gemm_w4_gateup_supported(m, n, k, g, r) == _plan(lib, row)["supported"], row
            seen["gateup"] += 1
    assert min(seen.values()) >= 100, seen


def test_a_plan_fits_the_workspace_it_was_given(lib, table):
    rows, _ = table
    split = 0
    for row in rows:
        p = _plan(lib, row)
        assert p["reduce"] == (p["S"] > 1)
        if p["S"] > 1:
            split += 1
            assert p["S"] * row["m"] * (row["k"] if row["kind"] == DX else row["n"]) * 4 <= row["ws"], (row, p)
    assert split >= 500
