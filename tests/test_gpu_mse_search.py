"""GPU tests of the MSE parameter search (qeft_mse_search, csrc/calib_mse.hip; calibrate.mse_search).

The reference, built here on the CPU: every candidate's residuals d by the pinned fp32 lines of calibrate.mse_params, scored as
sum |d|^2.4 in float64, the first argmin, and each candidate's final (scale, zero) by the pinned closing lines.  Per row, G = 1e-4:
  (1) the kernel's (scale, zero) is, bit for bit, the final pair of SOME candidate; zero integral in 0..maxq, scale >= 1e-8;
  (2) that candidate's fp64 score is <= (1 + G) x the best fp64 score;
  (3) where the best fp64 score is 0, or the next distinct score lies a relative gap >= G above it, the pair is the reference's.
G is a condition on the inputs, not an accuracy claim: any score with relative error below G / 2 meets all three (the hardware
log2 / exp2 sequence sits near 1e-6 by reasoning; the largest observed excess is printed).  (3) may leave out 10 % of a case."""
import os

import numpy as np
import pytest
import torch

import calib_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 1e-4


def bits_of(t):
    return t.contiguous().view(torch.int32)


def candidates(x, nbits, num=40):
    """(scores fp64 [C, N], pairs fp32 [C, 2, N]) of the num * 2^nbits candidates in the reference's order."""
    maxq = 2 ** nbits - 1
    zeros, eps = torch.zeros(x.shape[0]), torch.tensor(1e-8)
    xmin, xmax = torch.minimum(x.min(1)[0], zeros), torch.maximum(x.max(1)[0], zeros)
    xrange, tmp_min = xmax - xmin, torch.zeros_like(xmin)
    scores, pairs = [], []
    for i in range(1, num + 1):
        tmp_max = xrange / num * i
        delta = torch.max((tmp_max - tmp_min) / maxq, eps)
        scale = delta.reshape(-1, 1)
        x_round = torch.round(x / scale)
        for zp in range(maxq + 1):
            new_min, new_max = tmp_min - zp * delta, tmp_max - zp * delta
            zero = torch.clamp(0 - torch.round(new_min / delta), 0, maxq).reshape(-1, 1)
            d = x - scale * (torch.clamp(x_round + zero, 0, maxq) - zero)
            scores.append(d.double().abs().pow(2.4).sum(1))
            lo, hi = torch.min(new_min, zeros), torch.max(new_max, zeros)
            s = torch.max((hi - lo) / maxq, eps)
            pairs.append(torch.stack([s, torch.clamp(0 - torch.round(lo / s), 0, maxq)]))
    return torch.stack(scores), torch.stack(pairs)


CASES = [(b, g, 67, False) for b in (4, 3) for g in (1, 2, 127, 128, 129, 640)] + [(4, 129, 67, True), (3, 128, 1, False)]


@pytest.mark.parametrize("nbits,g,n,strided", CASES)
def test_mse_search_against_the_fp64_scores(nbits, g, n, strided):
    from qeft_amd import _lib, mse_search
    gen = torch.Generator().manual_seed(1000 * nbits + g + n)
    x = (torch.randn(n, g, generator=gen) * 0.02).half().float() + torch.randn(n, g, generator=gen) * 1e-4
    if g > 1 and n > 4:
        x[0] = 0
        x[1], x[2] = x[1].abs(), -x[2].abs()
        x[3, g // 2] = 0.5
        x[4] = x[4, 0]
    xg = x.to(DEV)
    if strided:                                                           # ld = g + 3, NaN everywhere outside the view
        big = torch.full((n + 2, g + 3), float("nan"), device=DEV)
        xg = big[1:n + 1, 2:2 + g]
        xg.copy_(x)
    s, z = mse_search(xg, nbits)
    assert _lib.last_variant() == ("mse_search_w4" if nbits == 4 else "mse_search_w3")
    assert s.shape == (n, 1) and z.shape == (n, 1) and s.dtype == torch.float32 and z.dtype == torch.float32
    s, z, maxq = s.cpu()[:, 0], z.cpu()[:, 0], 2 ** nbits - 1
    scores, pairs = candidates(x, nbits)
    best, first = scores.min(0)[0], scores.argmin(0)
    # (1)
    member = (bits_of(pairs[:, 0]) == bits_of(s)) & (bits_of(pairs[:, 1]) == bits_of(z))
    assert member.any(0).all() and torch.equal(z, z.round()) and z.min() >= 0 and z.max() <= maxq and s.min() >= 1e-8
    # (2): the best-scoring candidate among those that lead to the kernel's pair
    mine = torch.where(member, scores, torch.full_like(scores, float("inf"))).min(0)[0]
    excess = torch.where(best > 0, mine / best.clamp_min(1e-300) - 1, mine)
    # (3)
    nxt = torch.where(scores > best, scores, torch.full_like(scores, float("inf"))).min(0)[0]
    clear = (best == 0) | (nxt - best >= G * best)
    ref = pairs[first, :, torch.arange(n)]                                # [N, 2]
    same = (bits_of(ref[:, 0]) == bits_of(s)) & (bits_of(ref[:, 1]) == bits_of(z))
    print(f"{nbits} bits, g = {g}, N = {n}{', strided' if strided else ''}: largest score excess {excess.max().item():.3g}, rows left out "
          f"of (3) {(~clear).sum().item()} / {n}, rows with another pair than the reference's {(~same).sum().item()}")
    assert (mine <= (1 + G) * best).all()
    assert (~clear).sum().item() <= 0.1 * n
    assert same[clear].all()


@pytest.mark.parametrize("nbits", [4, 3])
def test_mse_search_returns_the_references_own_outputs(nbits):
    """tests/golden/calib_mse0.npz: what the reference's find_params(mse=True, num=40) returned for 16 rows.  The smallest
    runner-up gap on it is 3.2e-4 at 4 bits and 1.3e-3 at 3 bits (fp64, on a CPU), so no row is left out."""
    from qeft_amd import mse_search
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calib_mse0.npz"))
    s, zero = mse_search(torch.from_numpy(z["x"]).to(DEV), nbits)
    assert torch.equal(bits_of(s.cpu()), bits_of(torch.from_numpy(z[f"scale{nbits}"])))
    assert torch.equal(bits_of(zero.cpu()), bits_of(torch.from_numpy(z[f"zero{nbits}"])))


@pytest.mark.parametrize("nbits", [4, 3])
def test_gptq_reorder_mse_is_mse_torch_on_the_first_group(nbits):
    """The first group's columns are the untouched weights on both routes, so "mse" must return the torch search's bits there:
    those of mse_params ON THE CPU, where the kernel's sequence is pinned.  On the GPU torch divides a tensor by a Python number
    as a multiplication by the rounded reciprocal (measured on the MI355X: t / 15 differs from the CPU's quotient on 63 % of
    100 000 values, tensor / tensor on none), so "mse_torch" there differs from the CPU in the scale's last bits on 27 (4 bits)
    and 25 (3 bits) of these 32 rows, in no zero (printed).  "mse_torch" is compared with mse_params on the GPU: all it is."""
    from qeft_amd.calibrate import HessianAccumulator, gptq_reorder, mse_params, select_outliers
    W, X, hot = R.make_case(0)
    acc = HessianAccumulator(W.shape[1], DEV)
    acc.add_batch(X.to(DEV))
    _, ids = select_outliers(acc.H, len(hot))
    own = gptq_reorder(W.to(DEV), acc.H, ids, len(hot), bits=nbits, tuning="mse")
    ref = gptq_reorder(W.to(DEV), acc.H, ids, len(hot), bits=nbits, tuning="mse_torch")
    first = W.float()[:, ids.cpu()][:, :128]                               # no column of it is dead: the working matrix's first group
    s_cpu, z_cpu = mse_params(first, nbits)
    s_gpu, z_gpu = mse_params(first.to(DEV), nbits)
    ds = bits_of(ref.scale_group[:, 0].cpu()) != bits_of(s_cpu[:, 0])
    dz = bits_of(ref.zero_group[:, 0].cpu()) != bits_of(z_cpu[:, 0])
    print(f"{nbits} bits, first group: torch on the GPU against torch on the CPU: scale differs on {ds.sum().item()} / {ds.numel()} "
          f"rows, zero on {dz.sum().item()}")
    assert torch.equal(bits_of(own.scale_group[:, 0].cpu()), bits_of(s_cpu[:, 0]))
    assert torch.equal(bits_of(own.zero_group[:, 0].cpu()), bits_of(z_cpu[:, 0]))
    assert torch.equal(bits_of(ref.scale_group[:, 0]), bits_of(s_gpu[:, 0])) and torch.equal(bits_of(ref.zero_group[:, 0]), bits_of(z_gpu[:, 0]))
