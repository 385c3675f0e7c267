"""fp64 references of the row-wise kernels between the packed linears (csrc/decode_aux.hip: RMSNorm, prefill rotary, SiLU * up,
final norm + fp16 head), in numpy.  Every function takes the fp16 / fp32 inputs exactly (cast to float64) and returns float64.
Where a kernel's contract fixes a rounding point the reference applies the same one (include/qeft_hip.h): the fused residual
sum is fp16(fp32(x) + fp32(add)), and the head multiplies the norm output AFTER its rounding to fp16."""
import numpy as np


def _f64(a):
    return np.asarray(a).astype(np.float64)


def ulp16(v):
    """Spacing of fp16 at |v|: 2 ** (floor(log2 |v|) - 10), floored at the subnormal spacing 2 ** -24 (v = 0 included)."""
    v = np.abs(_f64(v))
    _, e = np.frexp(v)                     # |v| = m * 2 ** e with m in [0.5, 1): floor(log2 |v|) = e - 1, exactly
    return np.maximum(np.where(v > 0, np.ldexp(1.0, e - 11), 0.0), 2.0 ** -24)


def residual_sum(x, add):
    """The fused residual of qeft_rmsnorm: fp16(fp32(x) + fp32(add)), as float64."""
    return (np.asarray(x).astype(np.float32) + np.asarray(add).astype(np.float32)).astype(np.float16).astype(np.float64)


def rmsnorm(x, gamma, eps, add=None):
    """y = h * rsqrt(mean(h ** 2) + eps) * gamma over the last axis, h = x or residual_sum(x, add).  x fp16 or fp32 [.., H]."""
    h = _f64(x) if add is None else residual_sum(x, add)
    eps = float(np.float32(eps))           # the entry takes eps as a C float
    return h / np.sqrt((h * h).mean(-1, keepdims=True) + eps) * _f64(gamma)


def rope_rows(x, cos, sin, heads):
    """NeoX rotary (pairs i, i + 64) of the first `heads` heads of every row: x [T][row] (row >= heads * 128), cos / sin
    [T][64].  Columns past heads * 128 come back as they are."""
    out = _f64(x).copy()
    T = out.shape[0]
    v = out[:, :heads * 128].reshape(T, heads, 128)
    a, b = v[..., :64].copy(), v[..., 64:].copy()
    c, s = _f64(cos)[:, None, :], _f64(sin)[:, None, :]
    v[..., :64] = a * c - b * s
    v[..., 64:] = b * c + a * s
    out[:, :heads * 128] = v.reshape(T, heads * 128)
    return out


def rope_rows_terms(x, cos, sin, heads):
    """|a * c| + |b * s| (|b * c| + |a * s| for the upper half) of every rotated element, zero elsewhere: what the
    difference in rope_rows() cancels from."""
    out = np.zeros(np.asarray(x).shape, dtype=np.float64)
    T = out.shape[0]
    v = np.abs(_f64(x)[:, :heads * 128].reshape(T, heads, 128))
    c, s = np.abs(_f64(cos))[:, None, :], np.abs(_f64(sin))[:, None, :]
    t = np.concatenate([v[..., :64] * c + v[..., 64:] * s, v[..., 64:] * c + v[..., :64] * s], -1)
    out[:, :heads * 128] = t.reshape(T, heads * 128)
    return out


def silu_mul(g, u):
    """g / (1 + exp(-g)) * u."""
    g = _f64(g)
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g)) * _f64(u)


def lm_head(h32, gamma, W, eps, chunk=4096):
    """The token tail: xn = fp16(rmsnorm(h32) * gamma), logits = W . xn.  h32 [H] or [m][H] fp32, W [vocab][H] fp16.
    Returns (logits, mag): [vocab] or [m][vocab] each, mag[r] = sum_k |W[r, k] * xn[k]|."""
    xn = rmsnorm(h32, gamma, eps).astype(np.float16).astype(np.float64)
    rows = np.atleast_2d(xn)
    vocab = W.shape[0]
    logits = np.empty((rows.shape[0], vocab), dtype=np.float64)
    mag = np.empty_like(logits)
    for r0 in range(0, vocab, chunk):          # a 32000 x 8192 head is 2 GB as float64
        w = _f64(W[r0:r0 + chunk])
        logits[:, r0:r0 + chunk] = (w @ rows.T).T
        mag[:, r0:r0 + chunk] = (np.abs(w, out=w) @ np.abs(rows).T).T
    if xn.ndim == 1:
        return logits[0], mag[0]
    return logits, mag
