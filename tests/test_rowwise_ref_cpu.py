"""The fp64 references of tests/rowwise_ref.py against independent formulations (torch float64 ops, a complex product for the
rotary), and ulp16 against numpy's own fp16 spacing.  No GPU."""
import numpy as np
import pytest
import torch

import rowwise_ref as R

RTOL = 1e-12


def _close(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max() if scale is None else scale
    return float(np.abs(a - b).max()) <= RTOL * max(float(scale), 1e-300)


@pytest.mark.parametrize("m,h,dtype", [(1, 8, np.float16), (3, 264, np.float16), (5, 2056, np.float32), (2, 4096, np.float16)])
def test_rmsnorm_vs_torch_float64(m, h, dtype):
    rng = np.random.default_rng(m * 1000 + h)
    x = (rng.standard_normal((m, h)) * rng.uniform(0.01, 50, (m, 1))).astype(dtype)
    gamma = (1 + 0.1 * rng.standard_normal(h)).astype(np.float16)
    eps = 1e-5
    xt, gt = torch.from_numpy(x).double(), torch.from_numpy(gamma).double()
    e32 = float(np.float32(eps))
    ref = xt * torch.rsqrt(xt.pow(2).mean(-1, keepdim=True) + e32) * gt
    got = R.rmsnorm(x, gamma, eps)
    assert got.dtype == np.float64 and _close(got, ref.numpy())
    if dtype is np.float16:
        add = rng.standard_normal((m, h)).astype(np.float16)
        hs = (xt.float() + torch.from_numpy(add).float()).half()          # the documented rounding point
        assert np.array_equal(R.residual_sum(x, add), hs.double().numpy())
        hd = hs.double()
        ref = hd * torch.rsqrt(hd.pow(2).mean(-1, keepdim=True) + e32) * gt
        assert _close(R.rmsnorm(x, gamma, eps, add=add), ref.numpy())


def test_rmsnorm_zero_row_is_zero():
    y = R.rmsnorm(np.zeros((2, 16), np.float16), np.ones(16, np.float16), 1e-5)
    assert np.all(y == 0) and np.all(np.isfinite(y))


@pytest.mark.parametrize("T,heads,row", [(1, 1, 128), (5, 3, 384), (7, 4, 6 * 128), (4, 2, 2 * 128 + 24)])
def test_rope_rows_vs_complex_product(T, heads, row):
    rng = np.random.default_rng(T * 100 + heads)
    x = rng.standard_normal((T, row)).astype(np.float16)
    ang = rng.uniform(-np.pi, np.pi, (T, 64))
    cos, sin = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    got = R.rope_rows(x, cos, sin, heads)
    xt = torch.from_numpy(x).double()
    v = xt[:, :heads * 128].reshape(T, heads, 128)
    z = torch.complex(v[..., :64], v[..., 64:]) * torch.complex(torch.from_numpy(cos).double(), torch.from_numpy(sin).double())[:, None, :]
    ref = xt.clone()
    ref[:, :heads * 128] = torch.cat([z.real, z.imag], -1).reshape(T, heads * 128)
    assert _close(got, ref.numpy())
    assert np.array_equal(got[:, heads * 128:], x[:, heads * 128:].astype(np.float64))      # untouched columns: exactly
    terms = R.rope_rows_terms(x, cos, sin, heads)
    assert np.all(terms[:, heads * 128:] == 0) and np.all(terms[:, :heads * 128] + 1e-300 >= np.abs(got[:, :heads * 128]) * (1 - 1e-12))
    # one element by hand
    t, hd, i = T - 1, heads - 1, 17
    a, b = float(x[t, hd * 128 + i]), float(x[t, hd * 128 + 64 + i])
    c, s = float(cos[t, i]), float(sin[t, i])
    assert terms[t, hd * 128 + i] == pytest.approx(abs(a * c) + abs(b * s), rel=1e-14)
    assert terms[t, hd * 128 + 64 + i] == pytest.approx(abs(b * c) + abs(a * s), rel=1e-14)


def test_silu_mul_vs_torch_float64():
    rng = np.random.default_rng(3)
    g = np.concatenate([(rng.standard_normal(4096) * 4), [0.0, -0.0, 30.0, -30.0, 65504.0, -65504.0, 6e-8, -6e-8]]).astype(np.float16)
    u = rng.standard_normal(g.size).astype(np.float16)
    ref = torch.nn.functional.silu(torch.from_numpy(g).double()) * torch.from_numpy(u).double()
    got = R.silu_mul(g, u)
    assert np.all(np.isfinite(got))
    assert np.abs(got - ref.numpy()).max() <= RTOL * np.abs(ref.numpy()).max()
    # x * sigmoid(x) written the other way round: x * e^x / (1 + e^x) for x < 0
    neg = g.astype(np.float64) < 0
    gd = g.astype(np.float64)[neg]
    alt = gd * np.exp(gd) / (1 + np.exp(gd)) * u.astype(np.float64)[neg]
    assert np.abs(got[neg] - alt).max() <= RTOL * np.abs(alt).max()
    assert got[4097] == 0 and np.signbit(R.silu_mul(np.float16(-0.0), np.float16(1.0)))


@pytest.mark.parametrize("m,h,vocab", [(None, 512, 9), (3, 1024, 37)])
def test_lm_head_vs_torch_float64(m, h, vocab):
    rng = np.random.default_rng(h + vocab)
    h32 = (rng.standard_normal(h if m is None else (m, h)) * 3).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(h)).astype(np.float16)
    W = (rng.standard_normal((vocab, h)) * 0.05).astype(np.float16)
    logits, mag = R.lm_head(h32, gamma, W, 1e-5, chunk=8)                  # several chunks, a ragged last one
    xt = torch.from_numpy(h32).double()
    xn = (xt * torch.rsqrt(xt.pow(2).mean(-1, keepdim=True) + float(np.float32(1e-5))) * torch.from_numpy(gamma).double())
    xn = xn.half().double()                                                # the norm output is fp16 before the product
    Wt = torch.from_numpy(W).double()
    ref = xn @ Wt.T
    ref_mag = (Wt[None] * xn.reshape(-1, 1, h)).abs().sum(-1)
    assert logits.shape == ((vocab,) if m is None else (m, vocab)) and mag.shape == logits.shape
    assert _close(logits.reshape(-1, vocab), ref.reshape(-1, vocab).numpy(), scale=ref_mag.max().item())
    assert _close(mag.reshape(-1, vocab), ref_mag.numpy())
    assert np.all(mag + 1e-300 >= np.abs(logits))


def test_ulp16_is_the_fp16_spacing():
    bits = np.arange(0, 0x7BFF, dtype=np.uint16)            # every finite non-negative fp16 below the largest (whose spacing is inf)
    v = bits.view(np.float16)
    assert np.array_equal(R.ulp16(v), np.spacing(v).astype(np.float64))
    assert np.array_equal(R.ulp16(-v), np.spacing(v).astype(np.float64))
    assert R.ulp16(np.float16(65504.0)) == 32.0
    assert R.ulp16(0.0) == 2.0 ** -24 and R.ulp16(2.0 ** -24) == 2.0 ** -24 and R.ulp16(2.0 ** -14) == 2.0 ** -24
    assert R.ulp16(2.0 ** -13) == 2.0 ** -23
    for e in range(-13, 16):                                  # powers of two and their neighbours on both sides
        assert R.ulp16(2.0 ** e) == 2.0 ** (e - 10)
        assert R.ulp16(np.nextafter(2.0 ** e, 0.0)) == max(2.0 ** (e - 11), 2.0 ** -24)
        assert R.ulp16(np.nextafter(2.0 ** e, np.inf)) == 2.0 ** (e - 10)
    # values between fp16 numbers take the spacing of the binade they lie in
    assert R.ulp16(1000.3) == 0.5 and R.ulp16(-0.3) == 2.0 ** -12 and R.ulp16(1e-9) == 2.0 ** -24
    assert np.array_equal(R.ulp16(np.array([[1.0, 3.0], [0.0, -5.0]])), np.array([[2.0 ** -10, 2.0 ** -9], [2.0 ** -24, 2.0 ** -8]]))
