"""The launch plan of the round-1 decode GEMV (csrc/gemv_w4.h) against a recorded table.

tests/golden/gemv_w4_plan_parent.npz holds what the launchers did BEFORE the plan existed: the ladders of gemv_w4.hip and
gemv_w3.hip as they then were, run on a CPU with the launch macro replaced by a recorder (profiles/gemv_w4_plan_refactor.log has the
commands), over the GEMV, small-M, group and silu shapes of the GPU tests, the 7B / 13B / 70B linears with their row shards, sweeps
across every threshold of the ladders and, at 4 bits, every value of the two overrides (3 bits obeyed neither before the plan).
`values` is [column][row] with the columns named in `columns`: the call (kind 0 rows, 1 small-M, 2 group, 3 silu; gather and xt_aux
as the flags of qeft_gemv_w4_plan; on a rows or silu call xt_aux says that a residual was passed), the overrides, the return code,
the variant (an index into `variants`, -1 where nothing was launched), the number of launches, and those launches as up to two
runs a_ / b_ of `count` equal launches each: the kernel's template
arguments (taken from its symbol), grid, block, LDS bytes, rs_cap (-1: a VALU kernel), blk_end (-1: no group), the value
hipFuncSetAttribute was given (-1: not called), m_rt (where the kernel is the run-time-M instance, else -1), the first batch row
of the run and the rows from one launch to the next.

The plan entry of the C ABI makes no HIP call, so all of this runs without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import test_variant_census as census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, SMALLM, GROUP, SILU = 0, 1, 2, 3
PLAN = ("rc", "variant", "mfma", "bits", "D", "rgi", "outl", "xg", "xt", "threads", "be0", "be1", "be2",
        "b_count", "b_rows", "b_M", "b_grid", "b_lds", "b_rs_cap", "t_count", "t_rows", "t_M", "t_grid", "t_lds", "t_rs_cap")
RUN = ("count", "mfma", "group", "M", "D", "rgi", "outl", "xg", "xt", "kbits", "grid", "block", "lds", "rs_cap", "be0", "be1", "be2", "attr",
       "m_rt", "row0", "step")
NOT_SUPPORTED, INVALID_VALUE = 801, 1        # hipErrorNotSupported, hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def table():
    z = np.load(os.path.join(ROOT, "tests", "golden", "gemv_w4_plan_parent.npz"))
    cols = [str(c) for c in z["columns"]]
    return [dict(zip(cols, map(int, r))) for r in z["values"].T], [str(v) for v in z["variants"]]


def _plan(lib, row):
    """The plan for the row's call, as a dict, with the variant's name."""
    out = (ctypes.c_int * len(PLAN))()
    n = (ctypes.c_int * 3)(row["n0"], row["n1"], row["n2"])
    ov = (ctypes.c_int * 2)(row["ov_blocks"], row["ov_depth"])
    rc = lib.qeft_gemv_w4_plan(row["kind"], row["bits"], row["m"], row["nparts"], n, row["k"], row["g"], row["n_out"],
                               row["gather"] | (row["xt_aux"] << 1 if row["kind"] == GROUP else 0), ov, out)
    assert rc == 0, (rc, row)
    p = dict(zip(PLAN, out))
    p["name"] = lib.qeft_gemv_w4_variant_name(p["variant"]).decode()
    return p


def _launches(p):
    """The plan's launches in order: the body `count` times, then the tail, each with its first batch row."""
    out, row0 = [], 0
    for tag in "bt":
        for _ in range(p[tag + "_count"]):
            out.append(dict(rows=p[tag + "_rows"], M=p[tag + "_M"], grid=p[tag + "_grid"], lds=p[tag + "_lds"], rs_cap=p[tag + "_rs_cap"], row0=row0))
            row0 += p[tag + "_rows"]
    return out


def _runs(row, p):
    """The plan's launches as the recorder writes them: what each launch passes to the launch macro and to hipFuncSetAttribute,
    consecutive launches that differ in nothing but their rows folded into one run."""
    group, runs = int(row["kind"] == GROUP), []
    for l in _launches(p):
        rec = dict(mfma=p["mfma"], group=group, M=l["M"], D=p["D"], rgi=p["rgi"], outl=p["outl"], xg=p["xg"], xt=p["xt"], kbits=p["bits"],
                   grid=l["grid"], block=p["threads"], lds=l["lds"], rs_cap=l["rs_cap"] if p["mfma"] else -1,
                   be0=p["be0"] if group else -1, be1=p["be1"] if group else -1, be2=p["be2"] if group else -1,
                   attr=l["lds"] if l["lds"] > 64 * 1024 else -1, m_rt=l["rows"] if l["M"] == 16 else -1)
        if runs and all(runs[-1][c] == v for c, v in rec.items()):
            if runs[-1]["count"] == 1:
                runs[-1]["step"] = l["row0"] - runs[-1]["row0"]
            assert l["row0"] == runs[-1]["row0"] + runs[-1]["count"] * runs[-1]["step"], (row, p)
            runs[-1]["count"] += 1
        else:
            runs.append(dict(rec, count=1, row0=0 if group else l["row0"], step=0))
    return runs


def _mismatch(row, variants, p):
    """What of the recorded call the plan does not reproduce ('' when it reproduces all of it)."""
    if p["rc"] != row["rc"]:
        return f"rc {p['rc']} != {row['rc']}"
    want = variants[row["variant"]] if row["variant"] >= 0 else ""
    if p["name"] != want:
        return f"name {p['name']} != {want}"
    runs = _runs(row, p)
    recorded = [{c: row[tag + c] for c in RUN} for tag in ("a_", "b_") if row[tag + "count"]]
    if sum(r["count"] for r in runs) != row["launches"] or len(runs) != len(recorded):
        return f"launches {[r['count'] for r in runs]} != {[r['count'] for r in recorded]}"
    return "; ".join(f"run {i} {c} {mine[c]} != {v}" for i, (mine, rec) in enumerate(zip(runs, recorded)) for c, v in rec.items() if mine[c] != v)


def test_the_plan_reproduces_the_recorded_launches(lib, table):
    rows, variants = table
    assert len(rows) >= 5000
    bad = [(m, row) for row in rows for m in [_mismatch(row, variants, _plan(lib, row))] if m]
    assert not bad, (len(bad), bad[:5])


def test_an_altered_row_fails_the_comparison(lib, table):
    """Negative control: the comparison is not vacuous."""
    rows, variants = table
    row = next(r for r in rows if r["variant"] >= 0 and variants[r["variant"]] == "gemv_mfma" and r["b_count"] and r["ov_depth"] == 0)
    assert _mismatch(row, variants, _plan(lib, row)) == ""
    assert "name gemv_mfma != gemv_valu" in _mismatch(dict(row, variant=variants.index("gemv_valu")), variants, _plan(lib, row))
    for col, other in (("a_D", 2), ("a_grid", row["a_grid"] + 1), ("a_lds", row["a_lds"] + 16), ("a_rs_cap", row["a_rs_cap"] + 1),
                       ("b_M", 16), ("a_xg", 1 - row["a_xg"]), ("a_attr", 7), ("b_row0", row["b_row0"] + 1), ("a_kbits", 3)):
        assert f"{col[2:]} " in _mismatch(dict(row, **{col: other}), variants, _plan(lib, row)), col
    assert _mismatch(dict(row, rc=NOT_SUPPORTED), variants, _plan(lib, row)).startswith("rc")
    assert _mismatch(dict(row, launches=row["launches"] + 1), variants, _plan(lib, row)).startswith("launches")
    grouped = next(r for r in rows if r["kind"] == GROUP and r["launches"] and r["nparts"] == 3)
    assert "be1" in _mismatch(dict(grouped, a_be1=grouped["a_be1"] + 1), variants, _plan(lib, grouped))


def test_the_name_query_leaves_the_last_variant_alone(lib):
    before = lib.qeft_last_variant()
    assert lib.qeft_gemv_w4_variant_name(1) == b"gemv_valu" and lib.qeft_gemv_w4_variant_name(0) == b"" and lib.qeft_gemv_w4_variant_name(99) == b""
    assert lib.qeft_last_variant() == before and b"gemv_valu" != before


def test_the_table_covers_the_ladders(table):
    """Every round-1 GEMV name the census finds, every kind, both bit widths, every override value; conditions of the sample: at
    least 100 rows of every (kind, bits, family) that exists, refusals of both codes."""
    rows, variants = table
    names = {n for n, where in census._variants_in_csrc().items() if where.startswith(("gemv_w4.hip:", "gemv_w3.hip:"))}
    assert len(names) == 11 and names == {variants[r["variant"]] for r in rows if r["variant"] >= 0}
    assert {r["ov_blocks"] for r in rows} == {0, 2, 256} and {r["ov_depth"] for r in rows} == {0, 4, 6}
    assert {(r["ov_blocks"], r["ov_depth"]) for r in rows if r["bits"] == 4} == {(b, d) for b in (0, 2, 256) for d in (0, 4, 6)}
    assert {(r["ov_blocks"], r["ov_depth"]) for r in rows if r["bits"] == 3} == {(0, 0)}      # the ladder of gemv_w3.hip read neither
    count = {}
    for r in rows:
        if r["launches"]:
            key = (r["kind"], r["bits"], r["a_mfma"])
            count[key] = count.get(key, 0) + 1
    assert set(count) == {(ROWS, 4, 0), (ROWS, 4, 1), (ROWS, 3, 1), (SMALLM, 4, 1), (GROUP, 4, 0), (GROUP, 4, 1), (GROUP, 3, 1),
                          (SILU, 4, 0), (SILU, 4, 1), (SILU, 3, 1)}, count
    assert min(count.values()) >= 100, count
    refused = {code: {(r["kind"], r["bits"]) for r in rows if r["rc"] == code} for code in (NOT_SUPPORTED, INVALID_VALUE)}
    assert refused[NOT_SUPPORTED] == {(SMALLM, 4), (ROWS, 3), (GROUP, 3), (SILU, 3)}, refused       # no VALU fallback
    assert refused[INVALID_VALUE] == {(ROWS, 4), (GROUP, 4), (SILU, 4), (ROWS, 3), (SILU, 3)}, refused
    # every selector value of the launch site, and the row slicing: m = 0 .. 17, small-M up to 64, two runs
    launched = [r for r in rows if r["launches"]]
    assert {r["a_M"] for r in launched} | {r["b_M"] for r in launched if r["b_count"]} == set(range(1, 8)) | {16}
    assert {(r["a_mfma"], r["a_D"]) for r in launched} == {(0, 2), (0, 4), (1, 4), (1, 6)} and {r["a_rgi"] for r in launched} == {0, 1, 2, 4}
    assert {(r["a_xt"], r["a_xg"], r["a_outl"]) for r in launched} >= {(0, 0, 0), (0, 1, 1), (1, 0, 1), (2, 0, 0)}
    assert {r["m"] for r in rows if r["kind"] == ROWS} >= set(range(18)) and {r["m"] for r in rows if r["kind"] == SMALLM} >= set(range(65))
    assert any(r["b_count"] for r in rows) and any(r["a_attr"] > 0 for r in rows) and any(r["a_rs_cap"] > 1 for r in rows)


def _params(fn, names):
    """The argument list of the function's @pytest.mark.parametrize(names, ...)."""
    return next(mark.args[1] for mark in fn.pytestmark if mark.name == "parametrize" and mark.args[0] == names)


def test_the_gpu_tables_are_in_the_table(table):
    """Every row of the GEMV, GEMV_GATHER and GROUPED tables and the gemv_smallm rows of FWD in tests/test_gpu_gemm_tiers.py, the
    shapes of tests/test_gpu_gemv.py, test_gpu_w3.py and test_gpu_decode.py that call these launchers, and the four launches of
    every case of tests/test_gpu_engine_round1.py: each is a recorded call, with the variant its test names where it names one."""
    import test_gpu_decode as decode
    import test_gpu_engine_round1 as engine
    import test_gpu_gemm_tiers as tiers
    import test_gpu_gemv as gemv
    import test_gpu_w3 as w3
    rows, variants = table
    got = {(r["kind"], r["bits"], r["m"], r["n0"], r["n1"], r["n2"], r["k"], r["n_out"], r["g"], r["xt_aux"], r["gather"]):
           variants[r["variant"]] if r["variant"] >= 0 else "" for r in rows if r["ov_blocks"] == 0 and r["ov_depth"] == 0}

    def call(kind, bits, m, ns, k, r_, g, flag=0, gather=0):
        key = (kind, bits, m) + tuple(ns) + (0,) * (3 - len(ns)) + (k, r_, g, flag, gather)
        assert key in got, key
        return got[key]

    for m, n, k, r_, g, residual, want, _ in tiers.GEMV:
        assert call(ROWS, 4, m, [n], k, r_, g, int(residual)) == want, (m, n, k, r_, g)
    for m, n, k, r_, g, want, _ in tiers.GEMV_GATHER:
        assert call(ROWS, 4, m, [n], k, r_, g, 0, 1) == want, (m, n, k, r_, g)
    smallm = [c for c in tiers.FWD if c[5] == "gemv_smallm"]
    assert len(smallm) >= 7
    for m, n, k, r_, g, want, _ in smallm:
        assert call(SMALLM, 4, m, [n], k, r_, g) == want, (m, n, k, r_, g)
    for ns, k, r_, g, form, _ in tiers.GROUPED:
        for norm in (0, 1):
            assert call(GROUP, 4, 1, ns, k, r_, g, norm) == form[0], (ns, k, r_, g)
        assert call(SILU, 4, 1, ns[:1], k, r_, g, 1) == form[1], (ns, k, r_, g)
    # tests/test_gpu_gemv.py (whether v3 takes a shape first is the entry's business: here the launcher's own answer is on record)
    for n, k, r_, g in _params(gemv.test_gemv_shapes_and_groups, "n,k,r,g"):
        for m in (1, 3):
            assert call(ROWS, 4, m, [n], k, r_, g) in ("gemv_mfma", "gemv_valu"), (n, k, r_, g, m)
    for n, k in _params(gemv.test_gemv_llama_shapes, "n,k"):
        for m in range(1, 8):
            assert call(ROWS, 4, m, [n], k, 128, 128) == "gemv_mfma", (n, k, m)
    # tests/test_gpu_w3.py
    for n, k, r_, g in _params(w3.test_gemv_w3_vs_oracle, "n,k,r,g"):
        for m in _params(w3.test_gemv_w3_vs_oracle, "m"):
            assert call(ROWS, 3, m, [n], k, r_, g) == ("gemv_w3" if m == 1 else "gemv_w3_rows"), (n, k, r_, g, m)
    for ns, k in _params(w3.test_w3_group_norm_and_silu_variants, "ns,k"):
        assert call(GROUP, 3, 1, ns, k, 128, 128, 1) == "gemv_w3_group" and call(SILU, 3, 1, ns[:1], k, 128, 128, 1) == "gemv_w3_silu", (ns, k)
    # tests/test_gpu_decode.py
    for ns, k, r_ in _params(decode.test_grouped_gemv_equals_separate_launches, "ns,k,r"):
        assert call(GROUP, 4, 1, ns, k, r_, 128).endswith("_group"), (ns, k, r_)
    for ns, k in _params(decode.test_fused_rmsnorm_group_equals_unfused, "ns,k"):
        assert call(GROUP, 4, 1, ns, k, 128, 128, 1) == "gemv_mfma_group", (ns, k)
    for n, k in _params(decode.test_fused_silu_down_equals_unfused, "n,k"):
        assert call(SILU, 4, 1, [n], k, 128, 128, 1) == "gemv_mfma_silu" and call(ROWS, 4, 1, [n], k, 128, 128, 1) == "gemv_mfma", (n, k)
    # tests/test_gpu_engine_round1.py: q|k|v, o_proj, gate|up, down_proj of every case
    for name, (shape, _, _, (group, rows_, silu)) in engine.CASES.items():
        hidden, inter, heads, kv = (shape.get(c, d) for c, d in (("hidden", 256), ("inter", 512), ("heads", 2), ("kv", 2)))
        g, r_, bits, kvd = shape.get("group_size", 128), shape["n_out"], shape.get("bits", 4), kv * (hidden // heads)
        assert call(GROUP, bits, 1, [hidden, kvd, kvd], hidden, r_, g, 1) == group and call(GROUP, bits, 1, [inter, inter], hidden, r_, g, 1) == group, name
        assert call(ROWS, bits, 1, [hidden], hidden, r_, g, 1) == rows_ and call(SILU, bits, 1, [hidden], inter, r_, g, 1) == silu, name


def test_a_supported_plan_is_sound(lib, table):
    """LDS within 160 KB, block boundaries that rise with at least one block per part, rows x launches = m."""
    rows, _ = table
    planned = 0
    for row in rows:
        p = _plan(lib, row)
        if p["rc"]:
            assert all(p[c] == 0 for c in PLAN[1:]), (row, p)
            continue
        planned += 1
        m = row["m"] if row["kind"] in (ROWS, SMALLM) else 1
        assert p["b_count"] * p["b_rows"] + p["t_count"] * p["t_rows"] == m and p["t_count"] in (0, 1), (row, p)
        assert p["t_rows"] < p["b_rows"] or not p["t_count"], (row, p)
        for l in _launches(p):
            assert 0 < l["lds"] <= 160 * 1024 and l["grid"] >= 1 and l["M"] in (1, 2, 3, 4, 5, 6, 7, 16), (row, p)
            assert l["rows"] <= 16 if l["M"] == 16 else (l["rows"] == l["M"] or (l["M"] == 7 and l["rows"] > 7)), (row, p)
        if row["kind"] == GROUP:
            ends = [p["be0"], p["be1"], p["be2"]]
            assert ends[0] >= 1 and all(b - a >= 1 for a, b in zip(ends[:row["nparts"] - 1], ends[1:row["nparts"]])), (row, p)
            assert all(e == ends[row["nparts"] - 1] for e in ends[row["nparts"]:]) and ends[2] == p["b_grid"], (row, p)
    assert planned >= 5000
