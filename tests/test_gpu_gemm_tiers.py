"""Every tier of the GEMM forward, dX and d(oweight) launchers pinned to a shape and to float64.

gemm_w4_launch, gemm_w4_dx_launch and grad_oweight_launch choose between some twenty kernels by chains of shape predicates
(csrc/gemm_w4.hip, the GEMM entries of csrc/capi.hip).  Each case below is (m, n, k, r, g, variant, reason): it sits just inside
or just outside one clause of a predicate (the reason names it), asserts with == the variant that ran, and compares the whole
output with float64 -- so a kernel that only serves as the fallback of a newer tier cannot go wrong unseen, and a predicate
that stops admitting a shape cannot move it onto another kernel unnoticed ("Variant -> admission predicate ->
pinning test").  The same file calls the C ABI directly on the ragged cases, with the output and a workspace of exactly the
queried size between bands of NaN.

Bounds: rel_err < REL_TOL and elem_err_ok with its defaults (tests/util.py); the split tiers (fp32 partials in a workspace,
summed in a fixed order) keep the 2e-3 of test_dx_split_over_n_vs_oracle for rel_err and are bit-identical on a second call."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from oracle import qeft_oracle as O
from util import REL_TOL, elem_err_ok, layer_to_torch, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 4096                      # NaN elements in front of and behind a banded buffer
SPLIT_TOL = 2e-3

_WORST = {}                      # variant -> (worst rel_err, case)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_per_tier():
    yield
    print("\nworst rel_err per tier (tests/test_gpu_gemm_tiers.py)")
    for variant in sorted(_WORST):
        err, case = _WORST[variant]
        print(f"  {variant:28s} {err:.3e}  at {case}")


def _record(variant, err, case):
    print(f"[tier] {variant} {case}: rel_err {err:.3e}")
    if variant not in _WORST or err > _WORST[variant][0]:
        _WORST[variant] = (err, case)


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


@functools.lru_cache(maxsize=2)
def _layer(n, k, r, g, bits=4):
    """One packed layer per shape: numpy buffers, the same on the GPU, the dense float64 weights."""
    bufs = O.make_layer(n, k, r, g, seed=n + k + r + g, bias=True, bits=bits)
    w64 = O.dequant_dense(bufs["qweight"], bufs["scales"], bufs["scaled_zeros"], bufs["oweight"] if r else None, g).astype(np.float64)
    return bufs, layer_to_torch(bufs, DEV), w64


def _forward_ref(bufs, x, r, g):
    return O.quant_linear(x, bufs["qweight"], bufs["scales"], bufs["scaled_zeros"], bufs["oweight"] if r else None, bufs["bias"],
                          g).astype(np.float64)


def _dy(m, n):
    return (np.random.default_rng(m + n).standard_normal((m, n)) * 0.1).astype(np.float16)


def _check(got, ref, variant, case):
    """The bounds of this file; records the figure first."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), (variant, case)
    err = rel_err(got, ref)
    _record(variant, err, case)
    assert err < (SPLIT_TOL if "+split" in variant else REL_TOL), (variant, case, err)
    assert elem_err_ok(got, ref), (variant, case)


class _Banded:
    """n elements of `dtype`, all NaN, between two bands of NaN (as in tests/test_gpu_prefill_attn_kv8.py)."""

    def __init__(self, n, dtype):
        self.raw = torch.full((n + 2 * BAND,), float("nan"), dtype=dtype, device=DEV)
        self.mid = self.raw[BAND:BAND + n]
        assert self.mid.data_ptr() % 16 == 0

    def still_poisoned(self):
        return bool(torch.isnan(self.raw[:BAND]).all() and torch.isnan(self.raw[-BAND:]).all())


# ---------------------------------------------------------------------------------------------------------------- forward
FWD = [
    # gemm_v1: whatever the DMA-ring kernels do not take
    (129, 136, 128, 0, 64, "gemm_v1", "two k-tiles, under kStages"),
    (65, 8, 64, 32, 32, "gemm_v1", "one k-tile, half of it outliers"),
    (130, 264, 256, 32, 128, "gemm_v1", "n_out % 64 != 0"),
    (200, 128, 384, 96, 96, "gemm_v1", "group not a power of two, r = 96"),
    (130, 128, 768, 0, 192, "gemm_v1", "group not a power of two"),
    (130, 128, 8192, 0, 32, "gemm_v1", "the v2 scale array [K/G][128] exceeds 160 KB"),
    (17, 24, 192, 0, 96, "gemm_v1", "17 rows of a 128-row tile, N of 24"),
    # gemm_v2_128x128: K / 64 >= kStages, a power-of-two group, n_out % 64 == 0; under every loader-wave tier
    (129, 136, 192, 0, 64, "gemm_v2_128x128", "exactly kStages k-tiles"),
    (130, 136, 256, 0, 128, "gemm_v2_128x128", "four k-tiles: kStages + 1, still under G3_BST"),
    (130, 256, 256, 64, 32, "gemm_v2_128x128", "group 32: two groups per k-tile"),
    (200, 264, 320, 64, 64, "gemm_v2_128x128", "five k-tiles, one under G3_BST; ragged N"),
    # + split-K through the workspace
    (200, 512, 1088, 0, 64, "gemm_v2_128x128+splitk", "17 k-tiles: gemm_v3_split finds no divisor; S = 2"),
    (200, 512, 2048, 128, 32, "gemm_v2_128x128+splitk", "group 32 keeps it off the v3 split; S = 3, outlier tiles in the last part"),
    # gemm_v2_128x256: N % 256 == 0, 256 blocks, M >= 2048, and the 256-row loader-wave tier refuses (ok3 false)
    (2048, 4096, 256, 0, 64, "gemm_v2_128x256", "four k-tiles: ok3 false; 256 blocks"),
    (2048, 4096, 384, 64, 32, "gemm_v2_128x256", "group 32: ok3 false"),
    (2100, 4096, 320, 0, 64, "gemm_v2_128x256", "ragged M"),
    # gemv_smallm: up to 64 rows without a workspace, 16 per weight pass, where the newer small-M tiers refuse
    (40, 64, 128, 0, 128, "gemv_smallm", "k < 256: not the weight-stationary tier; slices 16 + 16 + 8"),
    (35, 48, 2048, 0, 2048, "gemv_smallm", "per-channel: not the weight-stationary tier; slices 16 + 16 + 3"),
    (19, 64, 512, 128, 512, "gemv_smallm", "per-channel with outliers; slices 16 + 3"),
    (12, 64, 1024, 256, 128, "gemv_smallm", "m <= 16 with n_out = 256: the decode GEMV refuses"),
    (17, 64, 128, 0, 128, "gemv_smallm", "slices 16 + 1: the tail on the fixed-M kernel at M = 1 (its grid from mfma_grid)"),
    (18, 64, 128, 0, 128, "gemv_smallm", "slices 16 + 2: the tail on the fixed-M kernel at M = 2"),
    (20, 48, 5248, 0, 5248, "gemv_smallm", "16 rows of K = 5248 exceed the 160 KB LDS plan, 14 fit: slices 14 + 6"),
    # the workspace query (it assumes group 128) against the route (it knows the group)
    (64, 4104, 1024, 0, 64, "gemm_v3_128x128+splitk", "group 64, N % 16 != 0: query and route agree on the split"),
    (40, 256, 1024, 256, 128, "gemm_v3_128x128+splitk", "n_out = 256: neither small-M tier; query and route agree"),
    (40, 256, 1024, 0, 64, "gemm_v2_128x128", "query answers 0 (it sees a weight-stationary shape), group 64 runs unsplit"),
    # the tiers above the floor, one small shape each
    (1025, 3704, 384, 64, 64, "gemm_v3_256x128", "145 tiles of 256 rows in one round against two rounds of 128-row tiles"),
    (129, 7176, 384, 64, 64, "gemm_v3_128x128", "114 tiles of 128 rows (>= 112), M > 128, nothing to split"),
    (40, 256, 1024, 128, 128, "gemm_ws", "17 .. 64 rows, group 128, n_out = 128"),
]


@pytest.mark.parametrize("m,n,k,r,g,want,reason", FWD, ids=[f"{c[5]}-{c[0]}x{c[1]}x{c[2]}-r{c[3]}-g{c[4]}" for c in FWD])
def test_forward_tier(m, n, k, r, g, want, reason):
    from qeft_amd import _lib, qeft_cuda
    bufs, t, _ = _layer(n, k, r, g)
    x = O.make_activation(m, k, r, seed=m)
    xt = torch.from_numpy(x).to(DEV)
    need = _lib.lib().qeft_gemm_w4_workspace_bytes(m, n, k, r)
    y = qeft_cuda.gemm_4bit_qeft(xt, t["qweight"], t["scales"], t["scaled_zeros"], t["oweight"] if r else None, t["bias"])
    variant = _lib.last_variant()
    y2 = qeft_cuda.gemm_4bit_qeft(xt, t["qweight"], t["scales"], t["scaled_zeros"], t["oweight"] if r else None, t["bias"])
    torch.cuda.synchronize()
    assert variant == want, (variant, want, reason)
    if "+splitk" in want:
        assert need >= 2 * m * n * 4, (need, reason)          # the wrapper brought what the query asked for: at least two parts
    _check(y.cpu().numpy(), _forward_ref(bufs, x, r, g), variant, (m, n, k, r, g))
    if "+splitk" in want:
        assert torch.equal(y, y2)                     # ordered sum of the partials


def test_workspace_query_against_the_route():
    """qeft_gemm_w4_workspace_bytes does not know the group size (it assumes 128) while gemm_impl routes by the real one.  Where
    they disagree the query may ask for a workspace the launch leaves alone, or for none where group 128 would have split -- never
    for less than the tier that runs needs (the band tests below all run on exactly the queried size).  The three shapes FWD
    pins, and the one where the query plans a 16-part split and group 32 drops the launch to gemm_v1."""
    from qeft_amd import _lib
    q = _lib.lib().qeft_gemm_w4_workspace_bytes
    assert q(64, 4104, 1024, 0) == 2 * 64 * 4104 * 4            # gemm_v3_128x128+splitk at group 64, S = 2
    assert q(40, 256, 1024, 256) == 2 * 40 * 256 * 4            # the same tier, n_out = 256
    assert q(40, 256, 1024, 0) == 0                             # a weight-stationary shape at group 128; group 64: gemm_v2_128x128
    assert q(130, 128, 8192, 0) == 16 * 130 * 128 * 4           # unused at group 32 (gemm_v1: no split)


SILU = [(1025, 3704, 384, 64, 64, "gemm_v3_256x128+silu", "the 256-row tier with a gate tensor, N % 8 == 0")]


@pytest.mark.parametrize("m,n,k,r,g,want,reason", SILU)
def test_forward_tier_silu_epilogue(m, n, k, r, g, want, reason):
    """silu(gate) * (x . W^T + bias) in the 256-row kernel's epilogue.  The product is rounded to fp16 before the activation and
    the result once more: two fp16 roundings (2^-11 each) against the unrounded float64 value fit the default bounds."""
    from qeft_amd import _lib, qeft_cuda
    bufs, t, w64 = _layer(n, k, r, g)
    x = O.make_activation(m, k, r, seed=m)
    gate = np.random.default_rng(n).standard_normal((m, n)).astype(np.float16)
    y = qeft_cuda.gemm_4bit_qeft_silu_mul(torch.from_numpy(x).to(DEV), t["qweight"], t["scales"], t["scaled_zeros"],
                                          t["oweight"] if r else None, torch.from_numpy(gate).to(DEV), t["bias"])
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == want, (variant, reason)
    g64 = gate.astype(np.float64)
    ref = g64 / (1 + np.exp(-g64)) * (x.astype(np.float64) @ w64.T + bufs["bias"].astype(np.float64))
    _check(y.cpu().numpy(), ref, variant, (m, n, k, r, g))


def test_forward_tier_gate_up_pair():
    """gate_proj | up_proj interleaved by 64 rows, SiLU(gate) * up in the epilogue: gemm_v3_256x128+silu_pair at any row count the
    entry supports (here 300 rows, 256 + 256 columns, six k-tiles)."""
    from qeft_amd import _lib, fuse, qeft_cuda
    m, n, k, r, g, want = 300, 256, 384, 0, 128, "gemm_v3_256x128+silu_pair"
    ls, refs = [], []
    x = O.make_activation(m, k, r, seed=m)
    for seed in (1, 2):
        b = O.make_layer(n, k, r, g, seed=seed + n, bias=True)
        t = layer_to_torch(b, DEV)
        ls.append(types.SimpleNamespace(qweight=t["qweight"], scales=t["scales"], scaled_zeros=t["scaled_zeros"], oweight=None,
                                        bias=t["bias"], outfeatures=n, infeatures=k, group_size=g, outlierfeatures=r, bits=4))
        w64 = O.dequant_dense(b["qweight"], b["scales"], b["scaled_zeros"], None, g).astype(np.float64)
        refs.append(x.astype(np.float64) @ w64.T + b["bias"].astype(np.float64))
    op = fuse.pair64_gemm_operand(*ls)
    assert qeft_cuda.gemm_gateup_supported(m, op)
    y = qeft_cuda.gemm_4bit_gateup(torch.from_numpy(x).to(DEV), op)
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == want, variant
    _check(y.cpu().numpy(), refs[0] / (1 + np.exp(-refs[0])) * refs[1], variant, (m, n, k, r, g))


W3 = [(129, 7168, 384, 0, 128, "gemm_v3_128x128_w3", "112 tiles of 128 rows, M > 128"),
      (1025, 3712, 384, 128, 128, "gemm_v3_256x128_w3", "145 tiles of 256 rows; four INT3 k-tiles and the outlier pair")]


@pytest.mark.parametrize("m,n,k,r,g,want,reason", W3, ids=[c[5] for c in W3])
def test_forward_tier_3bit_stream(m, n, k, r, g, want, reason):
    from qeft_amd import _lib, qeft_cuda
    bufs, t, _ = _layer(n, k, r, g, 3)
    x = O.make_activation(m, k, r, seed=m)
    y = qeft_cuda.gemm_3bit_qeft(torch.from_numpy(x).to(DEV), t["qweight"], t["scales"], t["scaled_zeros"], t["oweight"] if r else None,
                                 t["bias"])
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == want, (variant, reason)
    _check(y.cpu().numpy(), _forward_ref(bufs, x, r, g), variant, (m, n, k, r, g))


# decode GEMV entries: the two forms below the v3 kernel (gemv_w4.hip mfma_ok decides between them)
GEMV = [(3, 24, 384, 0, 128, False, "gemv_valu", "N % 16 != 0"),
        (1, 128, 640, 96, 32, False, "gemv_valu", "group 32, r = 96, K % 128 == 0 yet n_out % 128 != 0"),
        (2, 40, 576, 32, 64, False, "gemv_valu", "K % 128 != 0"),
        (2, 64, 512, 128, 128, True, "gemv_mfma", "a residual keeps the launch off the v3 kernel; mfma_ok holds"),
        (7, 48, 2048, 0, 2048, True, "gemv_mfma", "per-channel, residual, seven rows"),
        # the launch site's selectors no other GPU test reaches (qeft_gemv_w4_plan names them): the deep ring, RGI 4 and 2
        (1, 24, 6272, 0, 128, False, "gemv_valu", "K > 6144 on the VALU form: ring depth 4"),
        (1, 16, 6272, 0, 128, True, "gemv_mfma", "K > 6144 on the MFMA form: ring depth 6, one row set"),
        (1, 4096, 128, 0, 64, False, "gemv_valu", "group 64; 256 blocks of four row-groups: RGI 4"),
        (1, 2048, 128, 0, 64, False, "gemv_valu", "group 64; 256 blocks of two row-groups: RGI 2"),
        (7, 40, 576, 32, 64, False, "gemv_valu", "seven rows on the VALU form")]


@pytest.mark.parametrize("m,n,k,r,g,residual,want,reason", GEMV, ids=[f"{c[6]}-{c[0]}x{c[1]}x{c[2]}-r{c[3]}-g{c[4]}" for c in GEMV])
def test_gemv_entry_form(m, n, k, r, g, residual, want, reason):
    from qeft_amd import _lib, qeft_cuda
    bufs, t, w64 = _layer(n, k, r, g)
    x = O.make_activation(m, k, r, seed=m)
    res = (np.random.default_rng(n).standard_normal((m, n)) * 0.5).astype(np.float16) if residual else None
    y = qeft_cuda.gemv_4bit_fused(torch.from_numpy(x).to(DEV), t["qweight"], t["scales"], t["scaled_zeros"],
                                  t["oweight_interleaved"] if r else None, t["bias"], None,
                                  torch.from_numpy(res).to(DEV) if residual else None, m, n, k, g)
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == want, (variant, reason)
    # the unrounded value: with a residual, a sum of the fp16-rounded product would carry that rounding into a cancelling sum
    ref = x.astype(np.float64) @ w64.T + bufs["bias"].astype(np.float64)
    if residual:
        ref = ref + res.astype(np.float64)
    _check(y.cpu().numpy(), ref, variant, (m, n, k, r, g))


GEMV_GATHER = [(3, 24, 384, 32, 128, "gemv_valu", "N % 16 != 0, n_out = 32: x gathered through reorder_ids on the VALU form")]


@pytest.mark.parametrize("m,n,k,r,g,want,reason", GEMV_GATHER, ids=[f"{c[5]}-{c[0]}x{c[1]}x{c[2]}-r{c[3]}-g{c[4]}" for c in GEMV_GATHER])
def test_gemv_entry_form_with_gather(m, n, k, r, g, want, reason):
    """The o_proj launch (x through reorder_ids while it is staged) where only the VALU form takes the shape."""
    from qeft_amd import _lib, qeft_cuda
    bufs, t, w64 = _layer(n, k, r, g)
    x = O.make_activation(m, k, r, seed=m)
    ids = O.sparse_to_dense_ids(np.sort(np.random.default_rng(n).choice(k, size=r, replace=False)), k)
    y = qeft_cuda.gemv_4bit_fused(torch.from_numpy(x).to(DEV), t["qweight"], t["scales"], t["scaled_zeros"], t["oweight_interleaved"],
                                  t["bias"], torch.from_numpy(ids.astype(np.int32)).to(DEV), None, m, n, k, g)
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == want, (variant, reason)
    ref = np.take(x, ids, axis=-1).astype(np.float64) @ w64.T + bufs["bias"].astype(np.float64)      # unrounded, as above
    _check(y.cpu().numpy(), ref, variant, (m, n, k, r, g, "gather"))


# grouped (q|k|v, gate|up) and SiLU-staging launches of the decode engine's older GEMV: both forms
VALU, MFMA = ("gemv_valu_group", "gemv_valu_silu"), ("gemv_mfma_group", "gemv_mfma_silu")
GROUPED = [((264, 72), 576, 32, 64, VALU, "K % 128 != 0"),
           ((40, 24, 24), 384, 0, 128, VALU, "N % 16 != 0"),
           ((128, 64), 640, 96, 32, VALU, "n_out % 128 != 0, group 32"),
           ((256, 64, 64), 512, 128, 128, MFMA, "three parts, one block per row set"),
           ((64, 32), 1024, 0, 1024, MFMA, "per-channel, no outlier slice"),
           ((24, 24), 6272, 0, 128, VALU, "K > 6144 on the VALU form: ring depth 4"),
           ((4096, 64), 128, 0, 64, VALU, "group 64; 260 and 256 blocks of four row-groups: RGI 4"),
           ((2048, 8), 128, 0, 64, VALU, "group 64; 257 and 256 blocks of two row-groups: RGI 2")]


def _ptrs(ts):
    a = (ctypes.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        a[i] = t.data_ptr()
    return a


@pytest.mark.parametrize("ns,k,r,g,form,reason", GROUPED, ids=[f"{c[4][0]}-{'+'.join(map(str, c[0]))}x{c[1]}-r{c[2]}-g{c[3]}" for c in GROUPED])
def test_grouped_and_silu_gemv_form(ns, k, r, g, form, reason):
    """qeft_gemv_w4_group (plain and with the RMSNorm folded into the staging) and qeft_gemv_w4_silu against float64 on the
    oracle-dequantised weights, in the MFMA form where mfma_ok (gemv_w4.hip) holds and in the VALU form where it does not.  Every
    launch keeps the full bounds: the reference takes the staged activation as the kernel rounds it to fp16 -- the MFMA form
    stages fp16(x * gamma) and applies 1/rms to the finished dot products (gemv_w4_mfma.h), the VALU form stages
    fp16(x / rms * gamma) (gemv_w4_kernel.h); silu(gate) * up is taken as qeft_silu_mul rounds it (the staging rounds the same
    way).  What is left against float64 is then the fp32 accumulation and the one fp16 rounding of y, as in the plain launch."""
    from qeft_amd import _lib, qeft_cuda
    lib = _lib.lib()
    bufs = [O.make_layer(n, k, r, g, seed=50 + i) for i, n in enumerate(ns)]
    layers = [layer_to_torch(b, DEV) for b in bufs]
    ws = [O.dequant_dense(b["qweight"], b["scales"], b["scaled_zeros"], b["oweight"] if r else None, g).astype(np.float64) for b in bufs]
    szp = [qeft_cuda.pack_scales(l["scales"], l["scaled_zeros"], n, k, g) for l, n in zip(layers, ns)] if form is MFMA else None
    torch.manual_seed(8)
    x = (torch.randn(1, k, device=DEV) * 2).half()
    gamma = (1 + 0.1 * torch.randn(k, device=DEV)).half()
    packs = (_ptrs([l["qweight"] for l in layers]), _ptrs([l["scales"] for l in layers]), _ptrs([l["scaled_zeros"] for l in layers]),
             _ptrs([l["oweight_interleaved"] for l in layers]) if r else None)
    nn_ = (ctypes.c_int * len(ns))(*ns)
    x64 = x.cpu().numpy().astype(np.float64)[0]
    gamma64, inv_rms = gamma.cpu().numpy().astype(np.float64), 1 / np.sqrt((x64 ** 2).mean() + 1e-5)
    if form is MFMA:
        xn64, post = (x64 * gamma64).astype(np.float16).astype(np.float64), inv_rms
    else:
        xn64, post = (x64 * inv_rms * gamma64).astype(np.float16).astype(np.float64), 1.0
    for gam, xin, scale in ((None, x64, 1.0), (gamma, xn64, post)):
        ys = [torch.full((1, n), float("nan"), device=DEV, dtype=torch.float16) for n in ns]
        _lib.check(lib.qeft_gemv_w4_group(x.data_ptr(), gam.data_ptr() if gam is not None else None, 1e-5, len(ns), *packs, None,
                                          _ptrs(szp) if szp else None, _ptrs(ys), nn_, k, g, r, _st()))
        variant = _lib.last_variant()
        torch.cuda.synchronize()
        assert variant == form[0], (variant, reason)
        for n, y, w in zip(ns, ys, ws):
            _check(y.cpu().numpy()[0], scale * (w @ xin), variant, (n, k, r, g) + (("norm folded",) if gam is not None else ()))
    n, l, w = ns[0], layers[0], ws[0]
    gate = (torch.randn(k, device=DEV) * 2).half()
    up = torch.randn(k, device=DEV).half()
    res = torch.randn(1, n, device=DEV).half()
    act = torch.empty_like(gate)
    y1 = torch.full((1, n), float("nan"), device=DEV, dtype=torch.float16)
    _lib.check(lib.qeft_silu_mul(gate.data_ptr(), up.data_ptr(), act.data_ptr(), k, _st()))
    _lib.check(lib.qeft_gemv_w4_silu(gate.data_ptr(), up.data_ptr(), l["qweight"].data_ptr(), l["scales"].data_ptr(),
                                     l["scaled_zeros"].data_ptr(), l["oweight_interleaved"].data_ptr() if r else None, None,
                                     res.data_ptr(), szp[0].data_ptr() if szp else None, y1.data_ptr(), n, k, g, r, _st()))
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == form[1], (variant, reason)
    _check(y1.cpu().numpy()[0], w @ act.cpu().numpy().astype(np.float64) + res.cpu().numpy().astype(np.float64)[0], variant, (n, k, r, g))


# --------------------------------------------------------------------------------------------------------------------- dX
DX = [
    # dx128: K % 128 == 0 and 512 blocks of 128 x 128, where the loader-wave tiles refuse (gemm_dx_v3_ok)
    (2048, 136, 4096, 64, 64, 4, "dx128", "512 blocks; G % 128 != 0; N % 64 != 0"),
    (2048, 64, 4096, 0, 128, 4, "dx128", "N < 256"),
    (2100, 264, 4096, 32, 32, 4, "dx128", "ragged M; r = 32: a quarter of the 128-k tile"),
    # dx64: everything else
    (130, 136, 192, 32, 32, 4, "dx64", "K % 128 != 0; r = 32: half a 64-k tile; group 32"),
    (1, 8, 64, 0, 64, 4, "dx64", "one row, one n-tile of 8, one k-tile"),
    (200, 384, 384, 96, 96, 4, "dx64", "group not a power of two, r = 96"),
    # + split over n
    (130, 2056, 256, 64, 64, 4, "dx64+split", "33 n-tiles, 8 blocks: S = 2; ragged last n-tile"),
    (300, 4096, 512, 128, 128, 4, "dx64+split", "64 n-tiles, 24 blocks: S = 4"),
    # the loader-wave tiles, one small shape each
    (1025, 256, 4096, 128, 128, 4, "dx256", "160 tiles of 256 rows in one round against two of 128-row tiles; four n-tiles"),
    (530, 320, 3072, 0, 128, 4, "dx128v3", "120 tiles of 128 rows (>= 112); five n-tiles"),
    (1025, 320, 4096, 0, 256, 3, "dx256_w3", "the 3-bit stream, group 256"),
    (530, 704, 3072, 128, 128, 3, "dx128v3_w3", "the 3-bit stream, eleven n-tiles"),
]


@pytest.mark.parametrize("m,n,k,r,g,bits,want,reason", DX, ids=[f"{c[6]}-{c[0]}x{c[1]}x{c[2]}-r{c[3]}-g{c[4]}" for c in DX])
def test_dx_tier(m, n, k, r, g, bits, want, reason):
    from qeft_amd import _lib, qeft_cuda
    _, t, w64 = _layer(n, k, r, g, bits)
    dy = _dy(m, n)
    dyt = torch.from_numpy(dy).to(DEV)
    ow = t["oweight"] if r else None
    need = _lib.lib().qeft_gemm_w4_dx_workspace_bytes(m, n, k)

    def run():
        if bits == 3:
            return qeft_cuda.gemm_3bit_dx(dyt, t["qweight"], t["scales"], t["scaled_zeros"], ow, k)
        return qeft_cuda.gemm_4bit_dx(dyt, t["qweight"], t["scales"], t["scaled_zeros"], ow)
    dx = run()
    variant = _lib.last_variant()
    dx2 = run()
    torch.cuda.synchronize()
    assert variant == want, (variant, want, reason)
    assert (need >= 2 * m * k * 4) if "+split" in want else (need == 0), (need, reason)
    _check(dx.cpu().numpy(), dy.astype(np.float64) @ w64, variant, (m, n, k, r, g))
    if "+split" in want:
        assert torch.equal(dx, dx2)


# ------------------------------------------------------------------------------------------------------------ d(oweight)
DOW = [
    (130, 100, 72, 5, "grad_oweight_fma", "n % 8 != 0"),
    (1, 8, 64, 3, "grad_oweight_fma", "one row; r % 8 != 0"),
    (257, 264, 320, 100, "grad_oweight_fma", "r % 8 != 0: two j blocks, the second partly filled; five n blocks"),
    (64, 128, 100, 8, "grad_oweight_fma", "k % 8 != 0"),
    (33, 68, 136, 136, "grad_oweight_fma", "r == k, n % 8 != 0"),
    (130, 136, 192, 32, "grad_oweight_mfma", "16-byte row pieces: N, r, K all multiples of 8"),
    (33, 8456, 128, 72, "grad_oweight_mfma_n64", "265 n blocks x 2 j blocks > 512: 64 columns of dy per block"),
]


def _dow_inputs(m, n, k, r):
    return _dy(m, n), O.make_activation(m, k, r, seed=m + k)


@pytest.mark.parametrize("m,n,k,r,want,reason", DOW, ids=[f"{c[4]}-{c[0]}x{c[1]}x{c[2]}-r{c[3]}" for c in DOW])
def test_grad_oweight_tier(m, n, k, r, want, reason):
    from qeft_amd import _lib, qeft_cuda
    dy, x = _dow_inputs(m, n, k, r)
    dow = qeft_cuda.grad_oweight(torch.from_numpy(dy).to(DEV), torch.from_numpy(x).to(DEV), r)
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == want, (variant, reason)
    assert dow.shape == (n, r) and dow.dtype == torch.float32
    _check(dow.cpu().numpy(), dy.astype(np.float64).T @ x[:, k - r:].astype(np.float64), variant, (m, n, k, r))


# ------------------------------------------------------- the C ABI itself: writes outside the tile, the workspace promise
def _pick(table, shapes):
    """The cases of `table` on `shapes` (m, n, k, r, g); a shape that is not in the table is an error, not a case dropped."""
    rows = {c[:5]: c for c in table}
    assert len(rows) == len(table), "a shape twice in one table"
    return [rows[s] for s in shapes]


BAND_FWD = [c[:6] for c in _pick(FWD, [(130, 264, 256, 32, 128), (17, 24, 192, 0, 96), (130, 128, 8192, 0, 32), (200, 264, 320, 64, 64),
                                       (40, 256, 1024, 0, 64), (2100, 4096, 320, 0, 64), (200, 512, 1088, 0, 64), (200, 512, 2048, 128, 32),
                                       (35, 48, 2048, 0, 2048), (18, 64, 128, 0, 128), (64, 4104, 1024, 0, 64)])]
BAND_DX = [c[:5] + (c[6],) for c in _pick(DX, [(2048, 136, 4096, 64, 64), (2100, 264, 4096, 32, 32), (130, 136, 192, 32, 32), (1, 8, 64, 0, 64),
                                               (130, 2056, 256, 64, 64), (300, 4096, 512, 128, 128)])]
BAND_DOW = [c[:5] for c in DOW if c[4] == "grad_oweight_fma"]


def test_the_band_tables_hold_every_fallback_tier():
    """Needs no GPU itself; it stands here with the tables it guards (the whole file is marked gpu)."""
    assert {c[5] for c in BAND_FWD} >= {"gemm_v1", "gemm_v2_128x128", "gemm_v2_128x256", "gemm_v2_128x128+splitk", "gemv_smallm"}
    assert {c[5] for c in BAND_DX} == {"dx128", "dx64", "dx64+split"}
    assert {c[4] for c in BAND_DOW} == {"grad_oweight_fma"}


@pytest.mark.parametrize("m,n,k,r,g,want", BAND_FWD, ids=[f"{c[5]}-{c[0]}x{c[1]}x{c[2]}-r{c[3]}-g{c[4]}" for c in BAND_FWD])
def test_forward_c_abi_between_nan_bands(m, n, k, r, g, want):
    """qeft_gemm_w4_ws on an all-NaN output and a workspace of exactly qeft_gemm_w4_workspace_bytes, each between NaN bands:
    every element written and within the bounds, no band touched ("whichever tier the launch takes, it fits"), the result the
    wrapper's bit for bit."""
    from qeft_amd import _lib, qeft_cuda
    lib = _lib.lib()
    bufs, t, _ = _layer(n, k, r, g)
    x = O.make_activation(m, k, r, seed=m)
    xt = torch.from_numpy(x).to(DEV)
    need = lib.qeft_gemm_w4_workspace_bytes(m, n, k, r)
    assert need % 4 == 0
    out = _Banded(m * n, torch.float16)
    ws = _Banded(need // 4, torch.float32) if need else None
    _lib.check(lib.qeft_gemm_w4_ws(xt.data_ptr(), t["qweight"].data_ptr(), t["scales"].data_ptr(), t["scaled_zeros"].data_ptr(),
                                   t["oweight"].data_ptr() if r else None, t["bias"].data_ptr(), out.mid.data_ptr(),
                                   ws.mid.data_ptr() if ws else None, need, m, n, k, g, r, _st()))
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == want, variant
    assert out.still_poisoned() and (ws is None or ws.still_poisoned()), variant
    _check(out.mid.cpu().numpy().reshape(m, n), _forward_ref(bufs, x, r, g), variant, (m, n, k, r, g))
    y = qeft_cuda.gemm_4bit_qeft(xt, t["qweight"], t["scales"], t["scaled_zeros"], t["oweight"] if r else None, t["bias"])
    torch.cuda.synchronize()
    assert _lib.last_variant() == want and torch.equal(y.reshape(-1), out.mid)


@pytest.mark.parametrize("m,n,k,r,g,want", BAND_DX, ids=[f"{c[5]}-{c[0]}x{c[1]}x{c[2]}-r{c[3]}-g{c[4]}" for c in BAND_DX])
def test_dx_c_abi_between_nan_bands(m, n, k, r, g, want):
    """qeft_gemm_w4_dx_ws, as above, with exactly qeft_gemm_w4_dx_workspace_bytes of workspace."""
    from qeft_amd import _lib, qeft_cuda
    lib = _lib.lib()
    _, t, w64 = _layer(n, k, r, g)
    dy = _dy(m, n)
    dyt = torch.from_numpy(dy).to(DEV)
    need = lib.qeft_gemm_w4_dx_workspace_bytes(m, n, k)
    assert need % 4 == 0
    out = _Banded(m * k, torch.float16)
    ws = _Banded(need // 4, torch.float32) if need else None
    _lib.check(lib.qeft_gemm_w4_dx_ws(dyt.data_ptr(), t["qweight"].data_ptr(), t["scales"].data_ptr(), t["scaled_zeros"].data_ptr(),
                                      t["oweight"].data_ptr() if r else None, out.mid.data_ptr(), ws.mid.data_ptr() if ws else None,
                                      need, m, n, k, g, r, _st()))
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == want, variant
    assert out.still_poisoned() and (ws is None or ws.still_poisoned()), variant
    _check(out.mid.cpu().numpy().reshape(m, k), dy.astype(np.float64) @ w64, variant, (m, n, k, r, g))
    dx = qeft_cuda.gemm_4bit_dx(dyt, t["qweight"], t["scales"], t["scaled_zeros"], t["oweight"] if r else None)
    torch.cuda.synchronize()
    assert _lib.last_variant() == want and torch.equal(dx.reshape(-1), out.mid)


@pytest.mark.parametrize("m,n,k,r,want", BAND_DOW, ids=[f"{c[4]}-{c[0]}x{c[1]}x{c[2]}-r{c[3]}" for c in BAND_DOW])
def test_grad_oweight_c_abi_between_nan_bands(m, n, k, r, want):
    from qeft_amd import _lib, qeft_cuda
    dy, x = _dow_inputs(m, n, k, r)
    dyt, xt = torch.from_numpy(dy).to(DEV), torch.from_numpy(x).to(DEV)
    out = _Banded(n * r, torch.float32)
    _lib.check(_lib.lib().qeft_grad_oweight(dyt.data_ptr(), xt.data_ptr(), out.mid.data_ptr(), m, n, k, r, _st()))
    variant = _lib.last_variant()
    torch.cuda.synchronize()
    assert variant == want, variant
    assert out.still_poisoned()
    _check(out.mid.cpu().numpy().reshape(n, r), dy.astype(np.float64).T @ x[:, k - r:].astype(np.float64), variant, (m, n, k, r))
    assert torch.equal(qeft_cuda.grad_oweight(dyt, xt, r).reshape(-1), out.mid)
