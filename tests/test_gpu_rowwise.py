"""fp64 net under the row-wise kernels of csrc/decode_aux.hip (RMSNorm in its four forms, prefill rotary, SiLU * up, final norm +
fp16 head, one row and m rows) and under the prompt pass built from them (llama.prefill).

Every kernel is compared with tests/rowwise_ref.py -- fp64 from the kernel's own fp16 / fp32 inputs, never from another
kernel's output -- within a bound derived from the arithmetic:

  B1  results formed in fp32 and rounded once to fp16 (norm outputs, silu * up, rotary): |got - ref| <= ulp16(ref).  The final
      rounding costs 1/2 ulp; the fp32 chain in front of it (a sum of squares over at most 32 serial + 8 tree terms, rsqrtf,
      __expf and the hardware reciprocal at a few fp32 ulps each, two fp32 products) stays well under 1/4 ulp; the rest is
      room for a tie that flips.  Rotary adds 2 ** -22 * (|a c| + |b s|) for the cancellation in a c - b s.
  B2  head logits: |got - ref| <= ulp16(ref) + 2 ** -11 * sum_k |W[r, k] xn[k]|: the second term carries 1/2-ulp perturbations
      of the fp16 norm vector through the dot product.

Outputs live inside a larger allocation filled with one byte pattern, 64 elements of margin on either side, and both margins
must come back bit-identical: an overrun shows without a read or write outside memory the test owns.  Every launch uses
arguments the C entry accepts (refusals: test_cabi.py).  The largest err / bound of every case is printed ([rowwise] ...)."""
import numpy as np
import pytest
import torch

import rowwise_ref as R
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
MARGIN = 64
FILL = 0xA5
F16, F32 = torch.float16, torch.float32

WORST = {}


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from qeft_amd import _lib as L
    return L, L.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """A tensor of `shape` inside a larger allocation whose every byte is FILL, MARGIN elements before and after it."""

    def __init__(self, shape, dtype, init=None):
        es = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape))
        self.raw = torch.full(((n + 2 * MARGIN) * es,), FILL, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = MARGIN * es, (MARGIN + n) * es
        self.t = self.raw[self.lo:self.hi].view(dtype).view(*shape)
        if init is not None:
            self.t.copy_(init if torch.is_tensor(init) else torch.full(tuple(shape), init, dtype=dtype))

    def ptr(self):
        return self.t.data_ptr()

    def margins_intact(self):
        return bool((self.raw[:self.lo] == FILL).all().item() and (self.raw[self.hi:] == FILL).all().item())

    def untouched(self):
        return bool((self.raw == FILL).all().item())

    def numpy(self):
        return self.t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _check(kernel, case, got, ref, bound):
    got = np.asarray(got).astype(np.float64)
    assert np.all(np.isfinite(got)), f"{kernel} {case}: non-finite output"
    ratio = np.abs(got - ref) / bound
    worst = float(ratio.max())
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    print(f"[rowwise] {kernel} {case}: max err / bound = {worst:.4f}")
    i = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert worst <= 1.0, f"{kernel} {case}: err / bound {worst:.3f} at {i}: got {got[i]!r}, ref {ref[i]!r}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\n[rowwise] {k}: largest err / bound over all cases = {WORST[k]:.4f}", end="")
    print()


# ------------------------------------------------------------------------------------------------ RMSNorm, four forms
KINDS = ("normal", "massive", "zero", "big", "scales")


def _norm_rows(kind, m, H, rng):
    """[m][H] float64 inputs of one family and the per-row scale a companion `add` may have.  Row m // 2 is the special one:
    massive = 4 channels of +-2000 over ~0.02 noise, zero, big = every element +-60000; scales = every row its own scale, so a
    kernel that takes a row's statistic from a neighbour fails."""
    x = rng.standard_normal((m, H))
    add_scale = np.ones((m, 1))
    r = m // 2
    if kind == "massive":
        x[r] = 0.02 * rng.standard_normal(H)
        x[r, rng.choice(H, 4, replace=False)] = 2000.0 * rng.choice([-1.0, 1.0], 4)
        add_scale[r] = 0.02
    elif kind == "zero":
        x[r] = 0.0
        add_scale[r] = 0.0
    elif kind == "big":
        x[r] = 60000.0 * rng.choice([-1.0, 1.0], H)
        add_scale[r] = 0.0
    elif kind == "scales":
        sc = 4.0 ** ((np.arange(m) % 7) - 3.0)
        x *= sc[:, None]
        add_scale = sc[:, None]
    return x, add_scale


def _gamma(H, rng):
    return (1 + 0.1 * rng.standard_normal(H)).astype(np.float16)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


RMS_H = (8, 264, 2048, 2056, 4096, 5120, 8192)
RMS_CASES = [("normal", m, H) for m in (1, 5, 300) for H in RMS_H] + [(k, 5, H) for k in KINDS[1:] for H in RMS_H]


@pytest.mark.parametrize("kind,m,H", RMS_CASES)
def test_rmsnorm(kind, m, H):
    L, lib = _lib()
    rng = _rng(1, KINDS.index(kind), m, H)
    x64, add_scale = _norm_rows(kind, m, H, rng)
    x, add, gamma = x64.astype(np.float16), (rng.standard_normal((m, H)) * add_scale).astype(np.float16), _gamma(H, rng)
    xd, ad, gd = _dev(x), _dev(add), _dev(gamma)
    case = f"{kind} m={m} H={H}"
    # plain
    y = Guarded((m, H), F16)
    L.check(lib.qeft_rmsnorm(xd.data_ptr(), None, gd.data_ptr(), None, y.ptr(), m, H, EPS, _st()))
    torch.cuda.synchronize()
    assert y.margins_intact()
    ref = R.rmsnorm(x, gamma, EPS)
    _check("qeft_rmsnorm", case, y.numpy(), ref, R.ulp16(ref))
    if kind == "zero":
        assert np.all(y.numpy()[m // 2] == 0)
    # h = x + add, res_out = h, y = norm(h)
    y2, res = Guarded((m, H), F16), Guarded((m, H), F16)
    L.check(lib.qeft_rmsnorm(xd.data_ptr(), ad.data_ptr(), gd.data_ptr(), res.ptr(), y2.ptr(), m, H, EPS, _st()))
    torch.cuda.synchronize()
    assert y2.margins_intact() and res.margins_intact()
    assert np.array_equal(_bits(res.numpy()), _bits(R.residual_sum(x, add).astype(np.float16)))
    ref = R.rmsnorm(x, gamma, EPS, add=add)
    _check("qeft_rmsnorm(add)", case, y2.numpy(), ref, R.ulp16(ref))
    if kind == "zero":
        assert np.all(y2.numpy()[m // 2] == 0)
    # the same without res_out
    y3 = Guarded((m, H), F16)
    L.check(lib.qeft_rmsnorm(xd.data_ptr(), ad.data_ptr(), gd.data_ptr(), None, y3.ptr(), m, H, EPS, _st()))
    torch.cuda.synchronize()
    assert y3.margins_intact() and torch.equal(y3.t, y2.t)


F32_H = (8, 264, 2056, 4096, 8192)
F32_CASES = ([("normal", m, H) for m in (1, 3, 8) for H in F32_H] + [(k, 3, H) for k in KINDS[1:] for H in F32_H] +
             [("scales", 8, H) for H in F32_H])


@pytest.mark.parametrize("kind,m,H", F32_CASES)
def test_rmsnorm_f32(kind, m, H):
    L, lib = _lib()
    rng = _rng(2, KINDS.index(kind), m, H)
    x = _norm_rows(kind, m, H, rng)[0].astype(np.float32)
    gamma = _gamma(H, rng)
    xd, gd = _dev(x), _dev(gamma)
    y = Guarded((m, H), F16)
    L.check(lib.qeft_rmsnorm_f32(xd.data_ptr(), gd.data_ptr(), y.ptr(), m, H, EPS, _st()))
    torch.cuda.synchronize()
    assert y.margins_intact()
    ref = R.rmsnorm(x, gamma, EPS)
    _check("qeft_rmsnorm_f32", f"{kind} m={m} H={H}", y.numpy(), ref, R.ulp16(ref))
    if kind == "zero":
        assert np.all(y.numpy()[m // 2] == 0)


PRODUCER_H = (8, 2056, 5120, 8192)


def _check_partials(kernel, case, ssq, h_out, hidden):
    """ssq[b] against the fp64 sum of h_out ** 2 over block b's own 2048 elements, 1e-5 relative, block by block."""
    assert np.all(np.isfinite(ssq))
    worst = 0.0
    for b in range(ssq.size):
        want = float((h_out[b * 2048:min((b + 1) * 2048, hidden)].astype(np.float64) ** 2).sum())
        err = abs(float(ssq[b]) - want) / want
        worst = max(worst, err)
        assert err <= 1e-5, f"{kernel} {case}: ssq[{b}] = {ssq[b]!r}, fp64 {want!r}"
    print(f"[rowwise] {kernel} {case}: largest ssq partial rel err = {worst:.2e} (bound 1e-5)")


@pytest.mark.parametrize("with_gamma", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("hidden", PRODUCER_H)
def test_residual_norm(hidden, with_add, with_gamma):
    L, lib = _lib()
    rng = _rng(3, hidden, with_add, with_gamma)
    h = (rng.standard_normal(hidden) * 3).astype(np.float32)
    add, gamma = rng.standard_normal(hidden).astype(np.float16), _gamma(hidden, rng)
    nb = lib.qeft_token_begin_norm_blocks(hidden)
    assert nb == (hidden + 2047) // 2048
    hd, ad, gd = _dev(h), _dev(add), _dev(gamma)
    h_out, hnorm, ssq = Guarded((hidden,), F32), Guarded((hidden,), F16), Guarded((nb,), F32)
    L.check(lib.qeft_residual_norm(hd.data_ptr(), ad.data_ptr() if with_add else None, gd.data_ptr() if with_gamma else None,
                                   h_out.ptr(), hnorm.ptr(), ssq.ptr(), hidden, _st()))
    torch.cuda.synchronize()
    assert h_out.margins_intact() and hnorm.margins_intact() and ssq.margins_intact()
    want = h + add.astype(np.float32) if with_add else h
    ho = h_out.numpy()
    assert np.array_equal(_bits(ho), _bits(want))
    case = f"hidden={hidden} add={int(with_add)} gamma={int(with_gamma)}"
    if not with_gamma:
        assert hnorm.untouched() and ssq.untouched()
        return
    ref = ho.astype(np.float64) * gamma.astype(np.float64)
    _check("qeft_residual_norm", case, hnorm.numpy(), ref, R.ulp16(ref))
    _check_partials("qeft_residual_norm", case, ssq.numpy(), ho, hidden)


@pytest.mark.parametrize("tok,pos", [(0, 0), (10, 15), (16, 23), (-3, -2)])
@pytest.mark.parametrize("hidden", PRODUCER_H)
def test_token_begin_norm(hidden, tok, pos):
    """vocab 11, 16 positions: the first and last token / position, and values past either end (they clamp)."""
    L, lib = _lib()
    vocab, max_seq = 11, 16
    rng = _rng(4, hidden)
    embed = (rng.standard_normal((vocab, hidden)) * 0.5).astype(np.float16)
    tab = rng.uniform(-1, 1, (max_seq, 128)).astype(np.float32)
    gamma = _gamma(hidden, rng)
    nb = lib.qeft_token_begin_norm_blocks(hidden)
    assert nb == (hidden + 2047) // 2048
    ed, td, gd = _dev(embed), _dev(tab), _dev(gamma)
    tk, ps = torch.tensor([tok], dtype=torch.long, device=DEV), torch.tensor([pos], dtype=torch.int32, device=DEV)
    h, row = Guarded((hidden,), F32), Guarded((128,), F32)
    hnorm, ssq = Guarded((hidden,), F16), Guarded((nb,), F32)
    L.check(lib.qeft_token_begin_norm(ed.data_ptr(), tk.data_ptr(), td.data_ptr(), ps.data_ptr(), h.ptr(), row.ptr(), gd.data_ptr(),
                                      hnorm.ptr(), ssq.ptr(), hidden, vocab, max_seq, _st()))
    torch.cuda.synchronize()
    assert h.margins_intact() and row.margins_intact() and hnorm.margins_intact() and ssq.margins_intact()
    assert int(tk.item()) == tok and int(ps.item()) == pos                      # inputs are read, not clamped in place
    e = embed[min(max(tok, 0), vocab - 1)]
    assert np.array_equal(_bits(h.numpy()), _bits(e.astype(np.float32)))
    assert np.array_equal(_bits(row.numpy()), _bits(tab[min(max(pos, 0), max_seq - 1)]))
    case = f"hidden={hidden} tok={tok} pos={pos}"
    ref = e.astype(np.float64) * gamma.astype(np.float64)
    _check("qeft_token_begin_norm", case, hnorm.numpy(), ref, R.ulp16(ref))
    _check_partials("qeft_token_begin_norm", case, ssq.numpy(), h.numpy(), hidden)


# ------------------------------------------------------------------------------------------------ SiLU * up
def _silu_case(case, g, u):
    L, lib = _lib()
    n = g.size
    assert n % 8 == 0
    gd, ud = _dev(g), _dev(u)
    out = Guarded((n,), F16)
    L.check(lib.qeft_silu_mul(gd.data_ptr(), ud.data_ptr(), out.ptr(), n, _st()))
    torch.cuda.synchronize()
    assert out.margins_intact()
    got, ref = out.numpy(), R.silu_mul(g, u)
    assert not np.isnan(got).any()
    _check("qeft_silu_mul", case, got, ref, R.ulp16(ref))
    return got


@pytest.mark.parametrize("n", [8, 2040, 2048, 2056, 4096, 11008, 5 * 11008])
def test_silu_mul_random(n):
    rng = _rng(5, n)
    _silu_case(f"random n={n}", (rng.standard_normal(n) * 3).astype(np.float16), rng.standard_normal(n).astype(np.float16))


@pytest.mark.parametrize("up", ["one", "random"])
def test_silu_mul_every_finite_gate(up):
    """Every finite fp16 bit pattern as the gate (63488 values, both zeros and the subnormals included; __expf saturates towards
    either end of the range).  `up` is 1, or uniform in [-1, 1] so that no product leaves the fp16 range."""
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    bits = bits[(bits & 0x7C00) != 0x7C00]
    assert bits.size == 63488
    g = np.concatenate([bits.view(np.float16), np.zeros(-bits.size % 8, np.float16)])
    u = np.ones(g.size, np.float16) if up == "one" else np.random.default_rng(6).uniform(-1, 1, g.size).astype(np.float16)
    got = _silu_case(f"all finite gates, up={up}", g, u)
    zero = g == 0
    assert zero.sum() >= 2 and np.all(got[zero] == 0)
    if up == "one":
        assert np.array_equal(np.signbit(got[zero]), np.signbit(g[zero]))          # -0 -> -0, +0 -> +0


# ------------------------------------------------------------------------------------------------ prefill rotary
# (heads rotated, row_stride): plain [T][heads][128] tensors, the fused q|k|v widths, one row with padding columns
ROPE_LAYOUTS = ([(h, h * 128) for h in (1, 3, 4, 6, 33)] + [(2 + 2, 6 * 128), (4 + 2, 8 * 128), (64 + 8, 80 * 128)] +
                [(3, 3 * 128 + 24)])


def _rope_tables(kind, T):
    if kind == "model":                                   # the model's own table construction, theta 10000
        from qeft_amd import qeft_cuda
        cos, sin = qeft_cuda.rope_cos_sin(10000.0, 64, T)
        return cos.numpy(), sin.numpy()
    rng = _rng(7, T)
    return rng.uniform(-1, 1, (T, 64)).astype(np.float32), rng.uniform(-1, 1, (T, 64)).astype(np.float32)


ROPE_T = (1, 5, 67)
ROPE_CASES = ([(T, h, rs, "model") for T in ROPE_T for h, rs in ROPE_LAYOUTS] +
              [(T, 4 + 2, 8 * 128, "random") for T in ROPE_T])       # one random table, values in [-1, 1]


@pytest.mark.parametrize("T,heads,row_stride,table", ROPE_CASES)
def test_rope_rows(T, heads, row_stride, table):
    L, lib = _lib()
    rng = _rng(8, T, heads, row_stride)
    x = rng.standard_normal((T, row_stride)).astype(np.float16)
    cos, sin = _rope_tables(table, T)
    cd, sd = _dev(cos), _dev(sin)
    bufs = [Guarded((T, row_stride), F16, init=torch.from_numpy(x)) for _ in range(2)]
    for b in bufs:
        L.check(lib.qeft_rope_rows(b.ptr(), cd.data_ptr(), sd.data_ptr(), T, heads, row_stride, _st()))
    torch.cuda.synchronize()
    assert all(b.margins_intact() for b in bufs)
    got = bufs[0].numpy()
    assert np.array_equal(_bits(got), _bits(bufs[1].numpy()))                    # two copies: the same bits
    assert np.array_equal(_bits(got[:, heads * 128:]), _bits(x[:, heads * 128:]))   # un-rotated heads and padding: the input's bits
    ref = R.rope_rows(x, cos, sin, heads)
    bound = R.ulp16(ref) + 2.0 ** -22 * R.rope_rows_terms(x, cos, sin, heads)
    rot = slice(0, heads * 128)
    _check("qeft_rope_rows", f"T={T} heads={heads} row_stride={row_stride} table={table}", got[:, rot], ref[:, rot], bound[:, rot])


# ------------------------------------------------------------------------------------------------ final norm + fp16 head
HEAD_H = (512, 1024, 2048, 4096, 5120, 8192)
HEAD_V = (1, 7, 8, 9, 777, 4095, 4096, 4097)           # the block plan switches at vocab >= 4096; a block holds 8 rows
_HEADS = {}


def _head_inputs(hidden):
    """One head of 4097 rows per hidden size (vocab v uses its first v rows: W is [vocab][hidden], rows are independent), the
    two h32 vectors -- N(0, 3^2), and a massive-activation one (4 channels of +-2000 over 0.06 noise) -- and their fp64 logits,
    computed once and shared by every vocab of that hidden size."""
    if hidden not in _HEADS:
        rng = _rng(9, hidden)
        W = (rng.standard_normal((max(HEAD_V), hidden)) * 0.05).astype(np.float16)
        gamma = _gamma(hidden, rng)
        normal = (rng.standard_normal(hidden) * 3).astype(np.float32)
        massive = (rng.standard_normal(hidden) * 0.06).astype(np.float32)
        massive[rng.choice(hidden, 4, replace=False)] = 2000.0 * rng.choice([-1.0, 1.0], 4)
        h32 = {"normal": normal, "massive": massive}
        _HEADS[hidden] = dict(W=W, gamma=gamma, h32=h32, Wd=_dev(W), gd=_dev(gamma),
                              ref={k: R.lm_head(v, gamma, W, EPS) for k, v in h32.items()})
    return _HEADS[hidden]


def _head_check(kernel, case, got, ref, mag):
    _check(kernel, case, got, ref, R.ulp16(ref) + 2.0 ** -11 * mag)


@pytest.mark.parametrize("vocab", HEAD_V)
@pytest.mark.parametrize("hidden", HEAD_H)
def test_lm_head_f16(hidden, vocab):
    L, lib = _lib()
    d = _head_inputs(hidden)
    for kind, h32 in d["h32"].items():
        hd = _dev(h32)
        logits = Guarded((vocab,), F16, init=float("nan"))
        L.check(lib.qeft_lm_head_f16(hd.data_ptr(), d["gd"].data_ptr(), d["Wd"].data_ptr(), logits.ptr(), hidden, vocab, EPS, _st()))
        torch.cuda.synchronize()
        assert logits.margins_intact()
        ref, mag = d["ref"][kind]
        _head_check("qeft_lm_head_f16", f"{kind} hidden={hidden} vocab={vocab}", logits.numpy(), ref[:vocab], mag[:vocab])


@pytest.mark.parametrize("hidden", [4096, 8192])
def test_lm_head_f16_llama_vocab(hidden):
    """vocab 32000 (Llama-2's; 63 rows a block under the 512-block plan), at 7B's and 70B's hidden size."""
    L, lib = _lib()
    vocab = 32000
    gen = torch.Generator(device=DEV).manual_seed(hidden)
    Wd = (torch.randn(vocab, hidden, device=DEV, generator=gen) * 0.05).half()
    W = Wd.cpu().numpy()
    d = _head_inputs(hidden)
    refs, mags = R.lm_head(np.stack(list(d["h32"].values())), d["gamma"], W, EPS)      # both vectors over one pass of the head
    for (kind, h32), ref, mag in zip(d["h32"].items(), refs, mags):
        hd = _dev(h32)
        logits = Guarded((vocab,), F16, init=float("nan"))
        L.check(lib.qeft_lm_head_f16(hd.data_ptr(), d["gd"].data_ptr(), Wd.data_ptr(), logits.ptr(), hidden, vocab, EPS, _st()))
        torch.cuda.synchronize()
        assert logits.margins_intact()
        _head_check("qeft_lm_head_f16", f"{kind} hidden={hidden} vocab={vocab}", logits.numpy(), ref, mag)


@pytest.mark.parametrize("vocab", [9, 4097])
@pytest.mark.parametrize("hidden", HEAD_H)
@pytest.mark.parametrize("m", [2, 8])
def test_lm_head_f16_m(m, hidden, vocab):
    """m rows of different scales (4 ** -2 .. 4 ** 2 around N(0, 3^2)): a row normalised by another row's statistic fails."""
    L, lib = _lib()
    d = _head_inputs(hidden)
    rng = _rng(10, m, hidden)
    h32 = (rng.standard_normal((m, hidden)) * 3 * 4.0 ** ((np.arange(m) % 5) - 2.0)[:, None]).astype(np.float32)
    hd = _dev(h32)
    logits = Guarded((m, vocab), F16, init=float("nan"))
    L.check(lib.qeft_lm_head_f16_m(hd.data_ptr(), d["gd"].data_ptr(), d["Wd"].data_ptr(), logits.ptr(), hidden, vocab, EPS, m, _st()))
    torch.cuda.synchronize()
    assert logits.margins_intact()
    ref, mag = R.lm_head(h32, d["gamma"], d["W"][:vocab], EPS)
    _head_check("qeft_lm_head_f16_m", f"m={m} hidden={hidden} vocab={vocab}", logits.numpy(), ref, mag)


# ------------------------------------------------------------------------------------------------ the prompt pass
PROMPT_T = (1, 7, 8, 9, 33)       # per-linear GEMV route below 8 rows, the threshold, not a multiple of 8, several 8-row blocks
LOGIT_TOL = 2e-2                   # of the largest reference logit: the bound of test_gpu_decode.py's prefill test
CACHE_TOL = 2e-3                   # one more fp16 rounding than the reference (accumulation order + the rotary rounding)
_PROMPT = {}


def _prompt_model(name):
    """The model, 33 prompt tokens, the fp32 dense logits of all 33 (causal: row t depends on tokens [0, t] only, so the
    first T rows are the reference of the T-token prompt) and layer 0's K (rotated) / V in fp64, from the dense weights."""
    if name not in _PROMPT:
        from qeft_amd.llama import LlamaShape, QuantLlama, tiny_shape
        shape = (tiny_shape(n_layers=2, hidden=256, inter=512, n_heads=2, vocab=384, max_seq=64) if name == "mha" else
                 LlamaShape(512, 512, 2, 4, 2, 384, max_seq=64))
        model = QuantLlama(shape, DEV, seed=11)
        tokens = torch.randint(0, shape.vocab, (max(PROMPT_T),), generator=torch.Generator().manual_seed(12)).to(DEV)
        dense = model.dense_weights()
        ref_logits = model.forward_dense_reference(tokens, dense)
        L0 = model.model.layers[0]
        emb = model.model.embed_tokens.weight[tokens].cpu().numpy()
        xn = R.rmsnorm(emb, L0.input_layernorm.weight.cpu().numpy(), shape.rms_eps).astype(np.float16).astype(np.float64)
        proj = lambda nm: (xn @ dense[0][nm].cpu().numpy().astype(np.float64).T).astype(np.float16).astype(np.float64)   # noqa: E731
        k, v = proj("k_proj"), proj("v_proj")                                # [33][n_kv * 128]
        cos, sin = model.rope_cos[:max(PROMPT_T)].cpu().numpy(), model.rope_sin[:max(PROMPT_T)].cpu().numpy()
        _PROMPT[name] = dict(model=model, shape=shape, tokens=tokens, ref_logits=ref_logits, v=v,
                             k_rot=R.rope_rows(k, cos, sin, shape.n_kv_heads), v_rot=R.rope_rows(v, cos, sin, shape.n_kv_heads),
                             runs={})
    return _PROMPT[name]


def _prefill_run(name, T):
    """prefill(tokens[:T]) into a fresh engine, once per (model, T): logits, layer 0's caches, the engine's position."""
    d = _prompt_model(name)
    if T not in d["runs"]:
        from qeft_amd.llama import DecodeEngine, prefill
        eng = DecodeEngine(d["model"], use_graph=False)
        logits = prefill(d["model"], d["tokens"][:T], engine=eng).float()
        torch.cuda.synchronize()
        d["runs"][T] = dict(logits=logits, kc=eng.kc[0].cpu().numpy(), vc=eng.vc[0].cpu().numpy(), pos=int(eng.pos.item()))
    return d["runs"][T]


def _logit_err(got, ref):
    return (got - ref).abs().max().item() / ref.abs().max().item()


@pytest.mark.parametrize("T", PROMPT_T)
@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_prefill_layer0_cache_vs_fp64(name, T):
    """Layer 0's K / V rows [0, T) against fp64 from the dense weights: fp16(rmsnorm(embedding rows)) times k_proj / v_proj,
    rounded to fp16, rotary on K only.  A wrong head count, row stride or grouped-query slice shows here at full precision,
    before the later layers blur it."""
    d, run = _prompt_model(name), _prefill_run(name, T)
    n_kv, max_seq = d["shape"].n_kv_heads, d["shape"].max_seq
    assert run["kc"].shape == (n_kv, max_seq, 128) and run["vc"].shape == run["kc"].shape
    rows = lambda c: c[:, :T].transpose(1, 0, 2).reshape(T, n_kv * 128).astype(np.float64)      # noqa: E731
    got_k, got_v = rows(run["kc"]), rows(run["vc"])
    ek, ev = rel_err(got_k, d["k_rot"][:T]), rel_err(got_v, d["v"][:T])
    print(f"[rowwise] prefill {name} T={T}: layer-0 K rel err {ek:.2e}, V rel err {ev:.2e} (bound {CACHE_TOL:.0e})")
    assert ek < CACHE_TOL and ev < CACHE_TOL
    if T > 1:                    # position 0 rotates by nothing
        plain, rotated = np.abs(got_v[1:] - d["v"][1:T]).max(), np.abs(got_v[1:] - d["v_rot"][1:T]).max()
        assert plain < rotated, (plain, rotated)
    assert not run["kc"][:, T:].any() and not run["vc"][:, T:].any()


@pytest.mark.parametrize("T", PROMPT_T)
@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_prefill_logits_vs_dense_model(name, T):
    d, run = _prompt_model(name), _prefill_run(name, T)
    assert run["logits"].shape == (T, d["shape"].vocab) and run["pos"] == T
    err = _logit_err(run["logits"], d["ref_logits"][:T])
    print(f"[rowwise] prefill {name} T={T}: logits err {err:.2e} of the largest (bound {LOGIT_TOL:.0e})")
    assert err < LOGIT_TOL


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_prefill_is_causal(name):
    from qeft_amd.llama import DecodeEngine, prefill
    d = _prompt_model(name)
    long, short = _prefill_run(name, 33)["logits"], _prefill_run(name, 9)["logits"]
    assert _logit_err(long[:9], short) < LOGIT_TOL
    tokens = d["tokens"][:9].clone()
    tokens[8] = (tokens[8] + 1) % d["shape"].vocab
    other = prefill(d["model"], tokens, engine=DecodeEngine(d["model"], use_graph=False)).float()
    torch.cuda.synchronize()
    assert _logit_err(other[:8], short[:8]) < LOGIT_TOL
    assert not torch.equal(other[8], short[8])              # the replaced token did reach its own row
