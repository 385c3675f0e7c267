"""CPU checks of the drop-in boundary: the C-ABI library builds/loads and exports every symbol that
include/qeft_hip.h declares; argument validation that needs no GPU; the product has no CPU fallback."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "qeft_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(qeft_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_all_exported(lib):
    syms = declared_symbols()
    assert len(syms) >= 11
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/qeft_hip.h but not exported"
    from qeft_amd import _lib
    assert set(syms) == set(_lib.SIGNATURES), "ctypes table and header disagree"


def test_binding_parser_agrees_with_an_independent_extraction():
    """qeft_amd/_lib.py derives the ctypes tables from the header.  The names it finds are those of declared_symbols() (another
    regex, which knows nothing of types), and it yields one prototype per name: none parsed twice, none dropped."""
    from qeft_amd import _lib
    protos = _lib.parse_header(open(os.path.join(ROOT, "include", "qeft_hip.h")).read())
    names = [name for name, _, _ in protos]
    assert sorted(names) == declared_symbols()          # declared_symbols() is a sorted set: equal lists = no duplicate either
    assert len(protos) == len(declared_symbols()) >= 101
    assert _lib.SIGNATURES == {name: argtypes for name, _, argtypes in protos}
    assert _lib.RESTYPES == {name: restype for name, restype, _ in protos}


def test_binding_of_one_entry_per_type_class(lib):
    """Expected types written out from the header by hand, one entry per kind of thing the parser has to get right; the loaded
    functions carry them."""
    from qeft_amd import _lib
    p, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    want = {
        "qeft_abi_version": (i, []),                                              # (void)
        "qeft_error_string": (ctypes.c_char_p, [i]),                              # returns const char*
        "qeft_lm_head_nll_workspace_bytes": (ll, [i, i]),                         # returns long long
        "qeft_gemm_w4_ws": (i, [p] * 8 + [ll] + [i] * 5 + [p]),                   # a long long parameter
        "qeft_gemv_w4_group": (i, [p, p, f, i] + [p] * 8 + [i] * 3 + [p]),        # float, const void* const*, void* const*
        "qeft_oneshot_ipc_export": (i, [p, p]),                                   # a comment inside the parameter list
        "qeft_rope_attn_decode_kv8": (i, [p, p, p, i, p, p, i, i] + [p] * 9 + [i, p] + [i] * 6 + [p]),      # 26 parameters
        "qeft_attn_train_bwd_part": (i, [p, i, p, p, i, p, i, p, i, p, p, i, p, p, i, p, ll] + [i] * 5 + [p]),
    }
    assert len(want["qeft_rope_attn_decode_kv8"][1]) == 26 and len(want["qeft_attn_train_bwd_part"][1]) == 23
    for name, (restype, argtypes) in want.items():
        assert _lib.RESTYPES[name] is restype, name
        assert _lib.SIGNATURES[name] == argtypes, name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_binding_parser_refuses_what_it_does_not_know():
    """An unknown type raises and names the entry and the type: an int assumed where the header has something else would hand a
    kernel a truncated address or count.  The parser takes text, so the real header is not touched."""
    from qeft_amd import _lib
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    good = """
        #define QEFT_X 1  /* a macro that looks like a call: qeft_not_an_entry(1) */
        typedef void* qeft_stream_t;
        long long qeft_split(const void* x,   /* the input, */
                             int rows,        // then a count (and a stray paren
                             void* const* out /* 64 bytes; host */, long long bytes, float eps,
                             qeft_stream_t stream);
        const char * qeft_name(void);
    """
    assert _lib.parse_header(good) == [("qeft_split", ll, [p, i, p, ll, ctypes.c_float, p]), ("qeft_name", ctypes.c_char_p, [])]
    for bad, word in (("int qeft_bad(const void* x, double scale);", "double"),
                      ("int qeft_bad(const void* x, size_t n);", "size_t"),
                      ("int qeft_bad(struct qeft_opts opts, int n);", "struct qeft_opts"),
                      ("int qeft_bad(unsigned n);", "unsigned"),
                      ("double qeft_bad(int n);", "double"),
                      ("void* qeft_bad(int n);", "void*"),
                      ("size_t qeft_bad(void);", "size_t")):
        with pytest.raises(_lib.QeftHipError, match=r"qeft_bad.*" + re.escape(word)):
            _lib.parse_header(bad)


def test_missing_header_fails_loudly(monkeypatch):
    from qeft_amd import _lib
    monkeypatch.setattr(_lib, "HEADER", "/nonexistent/qeft_hip.h")
    with pytest.raises(_lib.QeftHipError, match="/nonexistent/qeft_hip.h"):
        _lib._read_header()


def test_every_included_header_is_a_build_dependency():
    """needs_build() looks at build.HEADERS alone: a header some source includes but the list lacks could be edited without a
    rebuild, and the suite would run the old library."""
    from qeft_amd import build
    deps = {os.path.normpath(os.path.join(build.CSRC, h)) for h in build.HEADERS}
    assert os.path.join(ROOT, "include", "qeft_hip.h") in deps
    files = [f for f in sorted(os.listdir(build.CSRC)) if f.endswith((".hip", ".h"))]
    assert set(build.SOURCES) <= set(files)
    for f in files:
        for inc in re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(os.path.join(build.CSRC, f)).read(), flags=re.M):
            path = os.path.normpath(os.path.join(build.CSRC, inc))
            assert os.path.isfile(path), f"{f} includes {inc}, which does not exist"
            assert path in deps, f"{f} includes {inc}, which is not in build.HEADERS"


def test_abi_version_and_error_strings(lib):
    assert lib.qeft_abi_version() == 1
    assert lib.qeft_error_string(1).decode() == "Unsupported batch size for gemv kernel."
    assert lib.qeft_error_string(0).decode() == "ok"


def test_argument_validation_without_gpu(lib):
    """Validation happens before any HIP call, so these run on a GPU-less host."""
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    g = lib.qeft_gemv_w4
    assert g(p, p, p, p, p, 8, 64, 512, 128, None) == 1       # batch
    assert g(p, p, p, p, p, 0, 64, 512, 128, None) == 1
    assert g(p, p, p, p, p, 1, 62, 512, 128, None) == 2       # N % 4
    assert g(p, p, p, p, p, 1, 64, 500, 128, None) == 2       # K % 64
    assert g(p, p, p, p, p, 1, 64, 512, 48, None) == 3        # group
    assert g(None, p, p, p, p, 1, 64, 512, 128, None) == 4    # null
    assert g(p + 2, p, p, p, p, 1, 64, 512, 128, None) == 6   # alignment
    q = lib.qeft_gemv_w4_qeft
    assert q(p, p, p, p, None, p, 1, 64, 512, 128, 128, None) == 4
    assert q(p, p, p, p, p, p, 1, 64, 512, 128, 100, None) == 2
    assert q(p, p, p, p, p, p, 1, 60, 512, 128, 128, None) == 2   # outliers need N % 8
    assert lib.qeft_gemm_w4(p, p, p, p, None, None, p, 0, 64, 512, 128, 0, None) == 2


def test_no_cpu_fallback():
    """A CPU tensor must raise, never silently compute on the host."""
    from qeft_amd import qeft_cuda
    x = torch.zeros(1, 128, dtype=torch.float16)
    qw = torch.zeros(2, 128, dtype=torch.int16)
    s = torch.zeros(1, 8, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        qeft_cuda.gemv_4bit(x, qw, s, s, 1, 8, 128, 128)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        qeft_cuda.gemm_4bit(x, qw, s, s)


def test_missing_library_fails_loudly(monkeypatch):
    from qeft_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libqeft_hip.so")
    with pytest.raises(_lib.QeftHipError, match="no CPU fallback"):
        _lib.lib()


def test_product_does_not_import_oracle():
    import glob
    for path in glob.glob(os.path.join(ROOT, "qeft_amd", "**", "*.py"), recursive=True) + \
            [os.path.join(ROOT, "qeft_cuda.py")]:
        src = open(path).read()
        assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S), f"{path} references the oracle"


def test_binding_puts_torch_hip_runtime_first():
    """The library links the system libamdhip64, torch ships its own: torch has to be loaded before the library or the
    process ends up with two HIP runtimes (launches then fail with hipErrorNoDevice, seen as build() + smoke() in one
    process).  The binding module therefore imports torch itself."""
    import subprocess
    import sys
    code = "import sys; from qeft_amd import _lib; assert 'torch' in sys.modules; print('ok')"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_shim_exports_the_reference_module_surface():
    """Every function the reference binds in qeft_cuda.cpp:10-27 exists in the module a reference caller imports, with
    the reference's positional parameters (the two FT entries keep their pybind defaults, qeft_cuda.cpp:23-26)."""
    import inspect
    import qeft_cuda
    want = {
        "gemm_4bit": ["in_feats", "kernel", "scales", "zeros"],
        "gemv_4bit": ["in_feats", "kernel", "scaling_factors", "zeros", "m", "n", "k", "group_size"],
        "gemv_4bit_qeft": ["in_feats", "kernel", "scaling_factors", "zeros", "oweight", "m", "n", "k", "group_size"],
        "layernorm_forward_cuda": ["x", "gamma", "out", "eps"],
        "single_query_attention": ["q", "k", "v", "k_cache", "v_cache", "length_per_sample_", "alibi_slopes_", "timestep",
                                   "rotary_embedding_dim", "rotary_base", "neox_rotary_style"],
    }
    for name, params in want.items():
        sig = inspect.signature(getattr(qeft_cuda, name))
        assert list(sig.parameters) == params, name
    d = inspect.signature(qeft_cuda.single_query_attention).parameters
    assert d["rotary_embedding_dim"].default == 0 and d["rotary_base"].default == 10000.0 and d["neox_rotary_style"].default is True
    x = torch.zeros(1, 2, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError):        # CPU tensors raise: no host fallback for the FT entries either
        qeft_cuda.layernorm_forward_cuda(x, torch.ones(128, dtype=torch.float16), torch.empty_like(x), 1e-5)


def test_round2_entries_reject_bad_arguments_without_a_gpu():
    """Argument validation happens before any HIP call: NULL operands, misaligned pointers and shapes the kernels do not
    take come back as error codes (no launch, no GPU needed)."""
    from qeft_amd import _lib
    lib = _lib.lib()
    ok_ptr = 1 << 20            # a non-NULL, 16-byte aligned address: validation must fail before anything dereferences it
    # decode GEMVs: K not a multiple of 128 / n not a multiple of 16 / an outlier width the kernel does not take
    for entry in (lib.qeft_decode_linear, lib.qeft_decode_linear_w3):
        assert entry(ok_ptr, ok_ptr, ok_ptr, ok_ptr, None, ok_ptr, 4096, 4000, 128, 128, 0, None, None, 0, 0.0, None, None, None, None) != 0
        assert entry(ok_ptr, ok_ptr, ok_ptr, ok_ptr, None, ok_ptr, 4090, 4096, 128, 128, 0, None, None, 0, 0.0, None, None, None, None) != 0
        assert entry(ok_ptr, ok_ptr, ok_ptr, ok_ptr, None, ok_ptr, 4096, 4096, 128, 64, 0, None, None, 0, 0.0, None, None, None, None) != 0
        assert entry(None, ok_ptr, ok_ptr, ok_ptr, None, ok_ptr, 4096, 4096, 128, 128, 0, None, None, 0, 0.0, None, None, None, None) != 0
        assert entry(ok_ptr + 2, ok_ptr, ok_ptr, ok_ptr, None, ok_ptr, 4096, 4096, 128, 128, 0, None, None, 0, 0.0, None, None, None, None) != 0
        # gamma_out without a residual, and more partial sums than a consumer accepts
        assert entry(ok_ptr, ok_ptr, ok_ptr, ok_ptr, None, ok_ptr, 4096, 4096, 128, 128, 0, None, None, 0, 0.0, ok_ptr, ok_ptr, ok_ptr, None) != 0
        assert entry(ok_ptr, ok_ptr, ok_ptr, ok_ptr, None, ok_ptr, 4096, 4096, 128, 128, 0, None, ok_ptr, 513, 1e-5, None, None, None, None) != 0
    assert lib.qeft_decode_linear_hnorm(ok_ptr, None, ok_ptr, ok_ptr, ok_ptr, None, ok_ptr, 4096, 4096, 128, 128, 0, 1e-5, None) != 0
    assert lib.qeft_decode_linear_hnorm(ok_ptr, ok_ptr, ok_ptr, ok_ptr, ok_ptr, None, ok_ptr, 4096, 4100, 128, 128, 0, 1e-5, None) != 0
    assert lib.qeft_lm_head_f16(ok_ptr, ok_ptr, ok_ptr, ok_ptr, 4000, 32000, 1e-5, None) != 0      # hidden not a multiple of 512
    assert lib.qeft_lm_head_f16(ok_ptr, ok_ptr, None, ok_ptr, 4096, 32000, 1e-5, None) != 0
    assert lib.qeft_rope_rows(None, ok_ptr, ok_ptr, 4, 2, 256, None) != 0
    assert lib.qeft_rope_rows(ok_ptr, ok_ptr, ok_ptr, 0, 2, 256, None) != 0
    assert lib.qeft_rope_rows(ok_ptr, ok_ptr, ok_ptr, 4, 2, 128, None) != 0      # rows narrower than their heads
    assert lib.qeft_decode_linear_blocks(4096) == 256 and lib.qeft_decode_linear_blocks(22016) == 459
    assert lib.qeft_decode_linear_blocks(5120) == 160          # between 256 and 512 row sets: two per block


def test_attention_entries_refuse_a_cache_above_the_ceiling(lib):
    """include/qeft_hip.h: max_seq <= 32768 on the four attention entries that share a cache (the one-token kernel keeps one
    raw fp32 score per cache row in LDS).  32768 + 16 is a multiple of 16 and nothing else about the call is wrong, so the
    ceiling alone answers QEFT_ERR_SHAPE, before any pointer is looked at; at 32768 the same calls pass the shape checks
    (their NULL cache is what is refused then).  qeft_single_query_attention_generic has the same ceiling for the same reason,
    without the multiple-of-16 rule: 32769 is refused, and it looks at its pointers first."""
    P, ERR_SHAPE, ERR_NULL = 1 << 20, 2, 4
    heads, kv = 32, 8

    def calls(max_seq, kc):
        return {
            "qeft_rope_attn_decode": lib.qeft_rope_attn_decode(P, P, P, P, P, 1, kc, P, P, None, P, P, 8, heads, kv, max_seq, None),
            "qeft_rope_attn_decode_m": lib.qeft_rope_attn_decode_m(P, P, P, 6144, P, P, 128, 4, kc, P, P, None, P, heads * 128, P, 8,
                                                                   heads, kv, max_seq, 4, None),
            "qeft_rope_attn_decode_batch": lib.qeft_rope_attn_decode_batch(P, P, P, 6144, P, P, 128, 4, kc, P, P, P, P, None, P,
                                                                           heads * 128, P, 8, 8, heads, kv, max_seq, 4, None),
            "qeft_single_query_attention": lib.qeft_single_query_attention(P, P, P, P, P, 1, kc, P, P, P, heads, kv, max_seq, None),
            "qeft_single_query_attention_alibi": lib.qeft_single_query_attention_alibi(P, P, P, P, P, 1, kc, P, P, P, heads, kv,
                                                                                       max_seq, P, None),
        }
    for name, code in calls(32768 + 16, P).items():
        assert code == ERR_SHAPE, (name, code)
    for name, code in calls(32768, None).items():
        assert code == ERR_NULL, (name, code)
    # the generic entry keeps one score per cache row in LDS too: the same ceiling, without the multiple-of-16 rule
    generic = lib.qeft_single_query_attention_generic
    assert generic(P, P, P, P, P, P, P, heads, kv, 32768 + 1, 64, None, None) == ERR_SHAPE
    assert generic(P, P, P, None, P, P, P, heads, kv, 32768, 64, None, None) == ERR_NULL
    # the whole-table rotary form at the ceiling's far side: still the shape, not the table
    assert lib.qeft_rope_attn_decode(P, P, P, P, P, 32768 + 16, P, P, P, None, P, P, 8, heads, kv, 32768 + 16, None) == ERR_SHAPE
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "qeft_hip.h")).read())
    assert text.count("max_seq <= 32768") >= 3 and "at most 32768" in text        # stated where the entries are declared


def test_generic_single_query_attention_refusals(lib):
    """qeft_single_query_attention_generic refuses, in this order, a NULL operand (QEFT_ERR_NULL; alibi_slopes alone is optional),
    a shape it does not take (QEFT_ERR_SHAPE: head_dim outside the multiples of 8 in [8, 256], n_heads % n_kv_heads, an empty
    cache) and a cache that is not 16-byte aligned (QEFT_ERR_ALIGN).  Operands are made-up addresses: every call has something
    wrong, so none reaches a launch."""
    P, ERR_SHAPE, ERR_NULL, ERR_ALIGN = 1 << 20, 2, 4, 6
    generic = lib.qeft_single_query_attention_generic

    def call(ptrs=None, heads=8, kv=2, max_seq=64, head_dim=64, alibi=None):
        return generic(*(ptrs or [P] * 7), heads, kv, max_seq, head_dim, alibi, None)

    names = ["q", "k", "v", "k_cache_ft", "v_cache", "pos", "out"]
    for i, name in enumerate(names):
        ptrs = [P] * 7
        ptrs[i] = None
        assert call(ptrs) == ERR_NULL, name
        assert call(ptrs, alibi=P) == ERR_NULL, name
        assert call(ptrs, head_dim=12) == ERR_NULL, name                # NULL is looked at before the shape
    for head_dim in (0, 4, 12, 264, -8):
        assert call(head_dim=head_dim) == ERR_SHAPE, head_dim
    assert call(heads=8, kv=3) == ERR_SHAPE
    assert call(heads=0) == ERR_SHAPE and call(kv=0) == ERR_SHAPE
    assert call(max_seq=0) == ERR_SHAPE
    for i in (3, 4):
        ptrs = [P] * 7
        ptrs[i] = P + 2
        assert call(ptrs) == ERR_ALIGN, names[i]
        assert call(ptrs, alibi=P) == ERR_ALIGN, names[i]
        assert call(ptrs, head_dim=12) == ERR_SHAPE, names[i]           # the shape before the alignment
        assert call(ptrs, max_seq=0) == ERR_SHAPE, names[i]


def test_refusals_are_those_recorded_before_the_argument_builders(lib):
    """tests/golden/capi_refusals_parent.json.gz: 52 348 calls that capi.hip refused before its argument builders existed, recorded
    on a CPU by tools/capi_record.cpp (profiles/capi_builders_refactor.log) -- the GEMV, GEMM forward, decode-linear and row-wise
    attention entries with one argument wrong (NULL, misaligned by 2 / 4 / 8, a list of integers) and with two wrong at once, which
    pins the precedence of the checks.  Each row is [entry, arguments, code]; operands are made-up addresses, so a row must be
    refused before anything looks at them: a complete set of valid arguments would launch where a GPU is present (DESIGN.md
    section 8), hence no row with code 0 is ever called."""
    import gzip
    import json
    from qeft_amd import _lib
    with gzip.open(os.path.join(ROOT, "tests", "golden", "capi_refusals_parent.json.gz")) as f:
        rows = json.load(f)
    assert len(rows) == 52348
    assert len({entry for entry, _, _ in rows}) == 21
    wrong = []
    for entry, args, code in rows:
        assert code in (1, 2, 3, 4, 6), (entry, args, code)       # never QEFT_OK, never QEFT_ERR_LAUNCH
        argtypes = _lib.SIGNATURES[entry]
        assert len(args) == len(argtypes), entry
        call = []
        for v in args:
            if isinstance(v, dict):
                v = (ctypes.c_int * 3)(*v["ints"])
            elif isinstance(v, list):
                v = (ctypes.c_void_p * 3)(*v)
            call.append(v)
        got = getattr(lib, entry)(*call)
        if got != code:
            wrong.append((entry, args, code, got))
    assert not wrong, f"{len(wrong)} rows, the first: {wrong[:3]}"


def test_gemm_workspace_follows_the_row_routing(lib):
    """No compute: the split-K workspace the shim asks for matches where gemm_impl will send the rows -- up to 16 rows of a shape
    the decode GEMV serves ride on it (no workspace), 17 .. 64 rows take the weight-stationary tier (gemm_ws.hip, one launch, no
    workspace), from 65 rows on the split-K tier wants its partial-sum buffer, enough tiles need none."""
    f = lib.qeft_gemm_w4_workspace_bytes
    for (n, k) in ((4096, 4096), (11008, 4096), (4096, 11008), (13824, 5120)):
        for m in (8, 12, 16):
            assert f(m, n, k, 128) == 0, (m, n, k)                # gemv_v3_mb / gemv_v3_mb_xg
        for m in (17, 24, 64):
            assert f(m, n, k, 128) == 0, (m, n, k)                # gemm_ws
        assert f(96, n, k, 128) >= 2 * 96 * n * 4, (n, k)           # split-K partial sums
    assert f(24, 4096, 4160, 128) >= 2 * 24 * 4096 * 4              # K % 128 != 0: not a shape the weight-stationary tier takes
    assert f(4096, 4096, 4096, 128) == 0
    assert f(16, 4096, 4160, 128) == 0                              # K % 128 != 0: the round-1 small-M route, no workspace either
