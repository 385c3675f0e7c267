"""Torch restatement of the calibration arithmetic (qeft_amd/calibrate.py, csrc/calib.h), any dtype, any device: the block lines of
qeft_gptq_block, the whole reorder loop, round-to-nearest on the same groups, the proxy loss and the recipe of the test layers.
A helper, not a test.  gptq_reorder(..., dtype=torch.float64) is the oracle of tests/test_gpu_calibrate.py;
tests/test_calibrate_cpu.py ties it to the reference's own GPTQ_OWQ through tests/golden/calib_case0.npz."""
import math

import torch

U = 2.0 ** -24          # unit roundoff of fp32
# the layers of the reorder tests: (seed, make_case keywords).  On each the reference's own proxy loss is 0.30 .. 0.43 x RTN's
# and its hessian_sorting picks exactly the scaled channels (tests/golden/make_golden_calib.py prints both).
CASES = [(0, {}), (1, {}), (2, {}), (3, {}), (4, dict(N=72, K=384, r=128))]
# 16 x the largest relative difference between the proxy losses of the fp32 and the fp64 restatement over CASES (2.9e-8, measured
# on the CPU by tests/test_calibrate_cpu.py::test_the_margin_is_what_the_restatements_measure)
REL_MARGIN = 16 * 2.9e-8
# the 3-bit layers of test_gptq_reorder_3_bits_and_mse: (seed, make_case keywords); they are part of the margin's measurement
CASES_W3 = [(0, {}), (11, dict(N=256, K=512, r=128, S=4, T=160))]


def make_case(seed, N=32, K=256, r=64, S=4, T=96):
    """W ~ N(0, 0.02^2) rounded to fp16; X = Z (0.6 I + 0.4 G / sqrt(K)), r random channels x 8, rounded to fp16 [S, T, K]."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).half()
    A = 0.6 * torch.eye(K) + 0.4 * torch.randn(K, K, generator=g) / math.sqrt(K)
    X = torch.randn(S, T, K, generator=g) @ A
    hot = torch.randperm(K, generator=g)[:r]
    X[..., hot] *= 8
    return W, X.half(), torch.sort(hot)[0]


def hessian64(X):
    """(2 / S) sum of x x^T over every row of the fp16 X [S, T, K], in fp64."""
    Xf = X.reshape(-1, X.shape[-1]).double()
    return (2.0 / X.shape[0]) * (Xf.T @ Xf)


def minmax(x, maxq):
    """One group over every column of x: (scale, zero) [N, 1]  (reference quant.py:80-82, 149-158)."""
    z0 = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    xmin = torch.minimum(x.min(1)[0], z0)
    xmax = torch.maximum(x.max(1)[0], z0)
    t = (xmin == 0) & (xmax == 0)
    xmin[t] = -1
    xmax[t] = 1
    s = (xmax - xmin) / maxq
    z = torch.round(-xmin / s)
    return s[:, None], z[:, None]


def block_lines(W1, Hinv1, scale, zero, maxq):
    """The pinned sequence of qeft_gptq_block, elementwise (every operation rounded once in W1's dtype).  W1 [N, count] (not
    modified), Hinv1 [count, count] (upper triangle read), scale / zero [N].  Returns (Q1, Err1, W1 updated)."""
    W1 = W1.clone()
    Q1 = torch.zeros_like(W1)
    E1 = torch.zeros_like(W1)
    for i in range(W1.shape[1]):
        w = W1[:, i]
        x = w / scale
        c = torch.clamp(torch.round(x) + zero, 0, maxq)
        q = scale * (c - zero)
        e = (w - q) / Hinv1[i, i]
        W1[:, i:] = W1[:, i:] - e[:, None] * Hinv1[i, i:][None, :]
        Q1[:, i] = q
        E1[:, i] = e
    return Q1, E1, W1


def factor(Hp, dtype, percdamp=0.01):
    """Dead columns, damping and the three Cholesky calls of recon.py:506-522 on a copy of Hp.  Returns (hinv, dead)."""
    H = Hp.to(dtype).clone()
    K = H.shape[0]
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    H[range(K), range(K)] += percdamp * torch.mean(torch.diag(H))
    H = torch.linalg.cholesky(H)
    H = torch.cholesky_inverse(H)
    return torch.linalg.cholesky(H, upper=True), dead


def gptq_reorder(Wp, Hp, n_nonout, dtype, bits=4, percdamp=0.01, g=128, hinv=None):
    """recon.py:488-566 with min-max parameters at each group start, on columns already in `ids` order.  Returns
    (Q [N, K] with the outlier columns carrying their feedback, scale_group, zero_group [N, K / g], hinv)."""
    maxq = 2 ** bits - 1
    W = Wp.to(dtype).clone()
    K = W.shape[1]
    h, dead = factor(Hp, dtype, percdamp)
    W[:, dead] = 0
    hinv = h if hinv is None else hinv.to(dtype)
    Q = torch.zeros_like(W)
    ss, zz = [], []
    for i1 in range(0, n_nonout, g):
        i2 = min(i1 + g, n_nonout)
        s, z = minmax(W[:, i1:i2], maxq)
        Q1, E1, _ = block_lines(W[:, i1:i2], hinv[i1:i2, i1:i2], s[:, 0], z[:, 0], maxq)
        Q[:, i1:i2] = Q1
        W[:, i2:] -= E1 @ hinv[i1:i2, i2:]
        ss.append(s)
        zz.append(z)
    for _ in range(K // g - len(ss)):
        ss.append(ss[-1])
        zz.append(zz[-1])
    Q[:, n_nonout:] = W[:, n_nonout:]
    return Q, torch.cat(ss, 1), torch.cat(zz, 1), hinv


def rtn(Wp, n_nonout, bits=4, g=128, return_params=False):
    """Round to nearest on the same groups; the outlier columns unchanged.  return_params: also the padded (scale, zero) groups."""
    maxq = 2 ** bits - 1
    Q = Wp.float().clone()
    ss, zz = [], []
    for i1 in range(0, n_nonout, g):
        i2 = min(i1 + g, n_nonout)
        s, z = minmax(Q[:, i1:i2], maxq)
        Q[:, i1:i2] = s * (torch.clamp(torch.round(Q[:, i1:i2] / s) + z, 0, maxq) - z)
        ss.append(s)
        zz.append(z)
    for _ in range(Q.shape[1] // g - len(ss)):
        ss.append(ss[-1])
        zz.append(zz[-1])
    return (Q, torch.cat(ss, 1), torch.cat(zz, 1)) if return_params else Q


def proxy_loss(W, Q, H):
    """tr((W - Q) H (W - Q)^T) in fp64."""
    E = (W.double() - Q.double())
    return torch.einsum("nk,kj,nj->", E, H.double(), E).item()


def dense_ids(out_ids, K):
    keep = torch.ones(K, dtype=torch.bool)
    keep[out_ids.long()] = False
    return torch.cat([torch.arange(K)[keep], out_ids.long()])


def gamma(n):
    return n * U / (1 - n * U)
