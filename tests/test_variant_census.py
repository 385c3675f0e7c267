"""Census of the kernel variant names (qeft_last_variant): every name a launcher in qeft_amd/csrc/*.hip can report must be
named by a GPU test, so that a tier added later cannot arrive without a test that says which kernel ran.

A name counts as pinned when it appears as a quoted string in some tests/test_gpu_*.py.  The few names an existing test asserts
through an f-string or a substring are listed in VIA_PATTERN with the file and the text that does it; that text must still be in
that file.  Nothing else is exempt.  Runs without a GPU: it only reads source text."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# variant -> (test file, the source text in it that asserts the name without quoting it whole).  Empty today: the names that older
# tests only reach through a pattern (f"gemm_v3_{tile}_w3" in test_gpu_w3.py, "+silu" in variant in test_gpu_gemm.py) are quoted
# whole in test_gpu_gemm_tiers.py.  An entry added here must name text that is really in that file (checked below).
VIA_PATTERN = {}


def _variants_in_csrc():
    """name -> file:line of every non-empty string literal in a statement that assigns g_last_variant (up to its ';', so an
    assignment that wraps onto further lines keeps its names)."""
    names = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "qeft_amd", "csrc", "*.hip"))):
        with open(path) as f:
            text = f.read()
        for m in re.finditer(r"\bg_last_variant\s*=(?!=)[^;]*;", text):
            for lit in re.findall(r'"([^"\\]*)"', m.group(0)):
                if lit:
                    names.setdefault(lit, f"{os.path.basename(path)}:{text.count(chr(10), 0, m.start()) + 1}")
    return names


def _gpu_test_sources():
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))):
        with open(path) as f:
            out[os.path.basename(path)] = f.read()
    return out


def test_the_census_finds_the_launchers():
    """The scan itself: it sees the names of every family of launcher (a change of the assignment's spelling must not empty it)."""
    names = _variants_in_csrc()
    for want in ("gemm_v1", "gemm_v2_128x256", "gemm_v2_128x128+splitk", "gemm_v3_256x128+silu_pair", "gemm_v3_128x128_w3", "gemm_ws",
                 "dx64+split", "dx128", "dx128v3_w3", "grad_oweight_fma", "grad_oweight_mfma_n64", "gemv_smallm", "gemv_valu_group",
                 "gemv_mfma_silu", "gemv_w3_rows", "gemv_v3_mb_xg", "gemv_v3_w3_pair", "gemv_v3_multi_pair", "attn_prefill_kv8", "sqa_generic"):
        assert want in names, want
    assert "" not in names and len(names) >= 45, sorted(names)


def _quoted(name, tests):
    return any(f'"{name}"' in src or f"'{name}'" in src for src in tests.values())


def test_the_scan_reads_a_wrapped_assignment(tmp_path, monkeypatch):
    d = tmp_path / "qeft_amd" / "csrc"
    d.mkdir(parents=True)
    (d / "a.hip").write_text('if (g_last_variant == "no") {}\ng_last_variant = wide ? "one"\n    : "two";\nx = "three";\n')
    monkeypatch.setattr(sys.modules[__name__], "ROOT", str(tmp_path))
    assert _variants_in_csrc() == {"one": "a.hip:2", "two": "a.hip:2"}


def test_every_variant_is_named_by_a_gpu_test():
    names, tests = _variants_in_csrc(), _gpu_test_sources()
    missing = [f"{name} ({where})" for name, where in sorted(names.items()) if name not in VIA_PATTERN and not _quoted(name, tests)]
    assert not missing, "variants no tests/test_gpu_*.py names: " + ", ".join(missing)


def test_the_pattern_exemptions_hold():
    """An exempted name is one that csrc sets, that no test quotes whole, and whose asserting text is still in the named file."""
    names, tests = _variants_in_csrc(), _gpu_test_sources()
    for name, (fname, text) in VIA_PATTERN.items():
        assert name in names, f"{name}: no launcher sets it any more -- drop the exemption"
        assert text in tests.get(fname, ""), f"{name}: {fname} no longer holds {text!r}"
        assert not _quoted(name, tests), f"{name} is quoted now -- drop the exemption"
