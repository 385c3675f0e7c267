"""Per-linear calibration: the GPTQ/OWQ reconstruction of an fp16 linear into a packed QuantLinear (reference qeft/recon.py:
GPTQ_OWQ.add_batch / hessian_sorting / fasterquant_reorder; main.py:130-171 for one layer).  DESIGN.md section 4.20.

    acc = HessianAccumulator(K, device);  acc.add_batch(x) per calibration batch        (qeft_hessian_accum)
    module, info = calibrate_linear(linear, acc.H, n_out, name)                         (qeft_gptq_block per 128 columns)

GPU tensors only: the two kernels have no CPU path and no torch fallback.  Around them the reference's own torch expressions
remain: dead columns, damping, the three Cholesky calls, the trailing update `W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:]` and the
group parameters, which are computed between launches (group size == block size == 128, so a group starts where a block does).

Out of scope, still: whole-model calibration (layer-by-layer activation capture, the shared outlier index, make_reorder's folding
of the permutation into norms and embeddings), act_order, sym=True, and a kernel for the MSE parameter search.
"""
import types

import torch

from . import _lib
from .qlinear import QuantLinear
from .quant import minmax_params, quantize
from .reorder import sparse_to_dense_ids

BLOCK = 128          # columns per qeft_gptq_block launch == the only supported group size


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _need_gpu(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise ValueError(f"{what} must be a GPU tensor: the calibration kernels have no CPU path")


class HessianAccumulator:
    """H = (2 / nsamples) * sum over every calibration row of x x^T, kept in fp32 [K, K] (reference add_batch, recon.py:35-57).

    add_batch(x): x fp16 [T, K] (one sequence) or [B, T, K].  nsamples counts sequences; with n the count before the call,
    H <- (n / (n + B)) H + (2 / (n + B)) X^T X in one launch.  The reference rounds sqrt(2 / n) x to fp32 before its fp32 GEMM; here
    the fp16 products are exact in fp32, summed in fp32 in one fixed order, and the two factors (rounded to fp32) are applied in
    the epilogue.  Both triangles of H carry the same bits."""

    def __init__(self, columns, device):
        if columns < 64 or columns % 64 != 0:
            raise ValueError(f"columns = {columns}: qeft_hessian_accum needs K % 64 == 0")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("HessianAccumulator needs a GPU device: the kernel has no CPU path")
        self.columns = columns
        self.H = torch.zeros((columns, columns), dtype=torch.float32, device=device)
        self.nsamples = 0

    def add_batch(self, x):
        _need_gpu(x, "x")
        if x.dtype != torch.float16:
            raise ValueError(f"x is {x.dtype}: qeft_hessian_accum reads fp16 rows")
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[-1] != self.columns:
            raise ValueError(f"x has shape {tuple(x.shape)}: want [T, {self.columns}] or [B, T, {self.columns}]")
        b = x.shape[0]
        x2 = x.reshape(-1, self.columns).contiguous()
        n = self.nsamples
        _lib.check(_lib.lib().qeft_hessian_accum(x2.data_ptr(), self.H.data_ptr(), x2.shape[0], self.columns, 2.0 / (n + b),
                                                 n / (n + b), _stream(x.device)))
        self.nsamples = n + b
        return self


def mse_params(x, bits=4, num=40, norm=2.4):
    """Quantizer.find_params(mse=True, num=40) of the reference (quant.py:87-141, asymmetric branch): a grid search over `num`
    ranges x 2^bits zero points per row, scored by mean |x - q|^2.4.  x [N, g]; returns (scale, zero) fp32 [N, 1].  Plain torch,
    num * 2^bits passes over x: slow plumbing until a kernel exists."""
    x = x.float()
    minq, maxq, n_levels = 0, 2 ** bits - 1, 2 ** bits
    zeros = torch.zeros(x.shape[0], device=x.device)
    eps = torch.tensor(1e-8, device=x.device)
    xmin = torch.minimum(x.min(1)[0], zeros)
    xmax = torch.maximum(x.max(1)[0], zeros)
    best_score = torch.zeros_like(xmin) + 1e10
    best_min, best_max = xmin.clone(), xmax.clone()
    xrange = xmax - xmin
    tmp_min = torch.zeros_like(xmin)
    for i in range(1, num + 1):
        tmp_max = xrange / num * i
        delta = torch.max((tmp_max - tmp_min) / (maxq - minq), eps)
        scale = delta.reshape(-1, 1)
        x_round = torch.round(x / scale)
        for zp in range(n_levels):
            new_min = tmp_min - zp * delta
            new_max = tmp_max - zp * delta
            zero = torch.clamp(minq - torch.round(new_min / delta), minq, maxq).reshape(-1, 1)
            x_q = scale * (torch.clamp(x_round + zero, minq, maxq) - zero)
            score = (x - x_q).abs().pow(norm).mean(1)
            better = score < best_score
            best_min = torch.where(better, new_min, best_min)
            best_max = torch.where(better, new_max, best_max)
            best_score = torch.min(best_score, score)
    min_val_neg = torch.min(best_min, torch.zeros_like(best_min))
    max_val_pos = torch.max(best_max, torch.zeros_like(best_max))
    scale = torch.max((max_val_pos - min_val_neg) / (maxq - minq), eps)
    zero = torch.clamp(minq - torch.round(min_val_neg / scale), minq, maxq)
    return scale.reshape(-1, 1), zero.reshape(-1, 1)


def _params(x, bits, tuning):
    """(scale, zero) fp32 [N, 1] of ONE group holding every column of x."""
    if tuning == "minmax":
        return minmax_params(x, x.shape[1], bits)
    if tuning == "mse":
        return mse_params(x, bits)
    raise ValueError(f"tuning = {tuning!r}: 'minmax' or 'mse'")


def frob_norm_error(W, bits=4, group_size=128, tuning="minmax"):
    """The per-column squared error of plain rounding that weighs the Hessian diagonal in select_outliers (reference
    main.py:132-138).  As there, the parameters are found per ROW over the whole row: Quantizer.find_params(W, weight=True) does
    not look at its group size, which is accepted for the call's symmetry alone."""
    del group_size
    W = W.float()
    scale, zero = _params(W, bits, tuning)
    return (W - quantize(W, scale, zero, 0, 2 ** bits - 1)).pow(2).sum(dim=0)


def select_outliers(H, n_out, frob_norm=None, outidx=None):
    """Which n_out columns stay fp16 (reference hessian_sorting(actorder=False), recon.py:60-100): the largest diag(H) (times
    frob_norm where given), or `outidx` as given.  Returns (out_ids, ids): out_ids int32, sorted ascending (`outidx` unchanged);
    ids = the other columns ascending, then out_ids -- exactly reorder.sparse_to_dense_ids(out_ids, K), the gather that
    QuantLinear.set_kernel installs for o_proj.  (The reference orders the outlier columns among themselves by descending score
    inside ids; they are never quantised, so only the order of the factorisation differs.)  Plain torch on H's device."""
    K = H.shape[0]
    if not 0 < n_out < K:
        raise ValueError(f"n_out = {n_out}: want 0 < n_out < K = {K}")
    if outidx is not None:
        out_ids = outidx.to(device=H.device, dtype=torch.int32)
    else:
        score = torch.diag(H).clone()
        if frob_norm is not None:
            score = score * frob_norm.to(score)
        out_ids = torch.sort(torch.argsort(score, descending=True)[:n_out])[0].to(torch.int32)
    return out_ids, sparse_to_dense_ids(out_ids, K)


def gptq_reorder(W, H, ids, n_out, bits=4, group_size=128, percdamp=0.01, tuning="minmax", hinv=None, sym=False):
    """The reference's fasterquant_reorder (recon.py:488-573) of one weight matrix on the GPU, 128 columns per launch.

    W [N, K] (any float dtype), H fp32 [K, K] as accumulated, ids the column order (select_outliers), the last n_out columns of
    which stay unquantised.  Returns a namespace:
      weight       fp16 [N, K], columns in `ids` order: dequantised values, then the outlier columns WITH the error feedback they
                   received (the reference's Q[:, n_nonout:] = W[:, n_nonout:])
      scale_group, zero_group   fp32 [N, K / 128]: one pair per started group of live columns, the last repeated up to K / 128
                   (recon.py:560-563); K - n_out need not be a multiple of 128 -- the last block and group are short
      out_ids (int32), ids, bits, group_size, n_out
      proxy_loss   tr((W - Q) H (W - Q)^T) on the undamped H in fp64, Q the fp32 values before the rounding to fp16
    tuning: 'minmax' (quant.minmax_params on the block's current columns) or 'mse' (mse_params, the reference's default; ours
    stays 'minmax' until the search has a kernel).  hinv: the upper Cholesky factor of the inverse damped Hessian in `ids` order,
    for a caller that has one (it replaces the three factorisation calls)."""
    if group_size != BLOCK:
        raise ValueError(f"group_size = {group_size}: only {BLOCK} is supported (a group must start where a block does)")
    if sym:
        raise ValueError("sym=True is not supported: the block kernel clamps to 0..maxq (asymmetric grid only)")
    if bits not in (3, 4):
        raise ValueError(f"bits = {bits}: only 3 and 4 are supported")
    if n_out % 2 != 0:
        raise ValueError(f"n_out = {n_out}: must be even (the packed outlier slice)")
    N, K = W.shape
    if K % BLOCK != 0:
        raise ValueError(f"K = {K}: must be a multiple of {BLOCK} (scale_group / zero_group hold K / {BLOCK} groups)")
    _need_gpu(W, "W")
    _need_gpu(H, "H")
    if H.shape != (K, K) or not 0 <= n_out < K:
        raise ValueError(f"H {tuple(H.shape)} / n_out {n_out} do not fit W {tuple(W.shape)}")
    dev = W.device
    ids = ids.to(dev).long()
    maxq = 2 ** bits - 1
    n_nonout = K - n_out

    W0 = W.float()[:, ids].contiguous()
    Hp = H.float()[ids][:, ids].contiguous()
    H0 = Hp.double()
    Wk = W0.clone()
    dead = torch.diag(Hp) == 0
    Hp[dead, dead] = 1
    Wk[:, dead] = 0
    if hinv is None:
        damp = percdamp * torch.mean(torch.diag(Hp))
        diag = torch.arange(K, device=dev)
        Hp[diag, diag] += damp
        Hp = torch.linalg.cholesky(Hp)
        Hp = torch.cholesky_inverse(Hp)
        hinv = torch.linalg.cholesky(Hp, upper=True)
    hinv = hinv.to(device=dev, dtype=torch.float32).contiguous()
    if hinv.shape != (K, K):
        raise ValueError(f"hinv {tuple(hinv.shape)}: want [{K}, {K}]")

    lib, st = _lib.lib(), _stream(dev)
    Q = torch.zeros_like(Wk)
    scales, zeros = [], []
    for i1 in range(0, n_nonout, BLOCK):
        i2 = min(i1 + BLOCK, n_nonout)
        count = i2 - i1
        scale, zero = _params(Wk[:, i1:i2], bits, tuning)
        scale, zero = scale.contiguous(), zero.contiguous()
        q1 = torch.empty((N, count), dtype=torch.float32, device=dev)
        err1 = torch.empty((N, count), dtype=torch.float32, device=dev)
        _lib.check(lib.qeft_gptq_block(Wk.data_ptr() + 4 * i1, K, hinv.data_ptr() + 4 * (i1 * K + i1), K, scale.data_ptr(),
                                       zero.data_ptr(), q1.data_ptr(), err1.data_ptr(), N, count, maxq, st))
        Q[:, i1:i2] = q1
        if i2 < K:
            Wk[:, i2:] -= err1.matmul(hinv[i1:i2, i2:])
        scales.append(scale)
        zeros.append(zero)
    for _ in range(K // group_size - len(scales)):
        scales.append(scales[-1])
        zeros.append(zeros[-1])
    Q[:, n_nonout:] = Wk[:, n_nonout:]
    E = (W0 - Q).double()
    proxy_loss = ((E @ H0) * E).sum().item()
    return types.SimpleNamespace(weight=Q.to(torch.float16), scale_group=torch.cat(scales, 1), zero_group=torch.cat(zeros, 1),
                                 out_ids=ids[n_nonout:].to(torch.int32), ids=ids, bits=bits, group_size=group_size, n_out=n_out,
                                 proxy_loss=proxy_loss)


def calibrate_linear(linear, H, n_out, name, bits=4, group_size=128, frob_norm=True, outidx=None, **kw):
    """One fp16 nn.Linear + its accumulated Hessian -> (QuantLinear, quantinfo): select_outliers -> gptq_reorder ->
    QuantLinear.pack(outlieridx=out_ids, scales=scale_group, zeros=zero_group) -> set_kernel().

    frob_norm: True = weigh diag(H) by frob_norm_error(W) as the reference does by default, False/None = diag(H) alone, or the
    tensor to use.  outidx: fixed outlier columns instead of a selection.  Other keywords go to gptq_reorder (percdamp, tuning,
    hinv).  The quantinfo namespace carries what checkpoint.save_packed / quant.lm_pack read (bits, sym, group_size, n_out,
    reorder, scale_group, zero_group, out_ids) plus ids and proxy_loss, so the layer saves and loads like any other.

    The packed columns are in `ids` order.  A module whose name contains 'o_proj' or 'out_proj' gathers its own input
    (set_kernel installs reorder_ids == ids); for any other name the caller feeds x[..., ids] until the offline global reordering
    exists.  n_out = 0 is plain GPTQ: nothing is selected and ids is the identity."""
    W = linear.weight.data
    _need_gpu(W, "linear.weight")
    _need_gpu(H, "H")
    tuning = kw.get("tuning", "minmax")
    if frob_norm is True and n_out > 0:
        frob_norm = frob_norm_error(W, bits, group_size, tuning)
    elif frob_norm is False:
        frob_norm = None
    if n_out == 0:                                      # plain GPTQ: no fp16 columns, the columns stay where they are
        out_ids, ids = torch.zeros(0, dtype=torch.int32, device=H.device), torch.arange(H.shape[0], device=H.device)
    else:
        out_ids, ids = select_outliers(H, n_out, frob_norm=frob_norm, outidx=outidx)
    res = gptq_reorder(W, H, ids, n_out, bits=bits, group_size=group_size, **kw)
    N, K = W.shape
    module = QuantLinear(bits, K, N, linear.bias is not None, torch.float16, n_out, group_size, True, name)
    # pack() is host-side layout arithmetic (the checkpoint path runs it on the CPU)
    bias = linear.bias.detach().cpu() if linear.bias is not None else None
    holder = types.SimpleNamespace(weight=types.SimpleNamespace(data=res.weight.cpu()), bias=bias)
    module.pack(holder, scales=res.scale_group.cpu(), zeros=res.zero_group.cpu(), outlieridx=out_ids.cpu())
    module = module.to(W.device)
    module.set_kernel()
    info = types.SimpleNamespace(bits=bits, sym=False, group_size=group_size, n_out=n_out, reorder=True,
                                 scale_group=res.scale_group, zero_group=res.zero_group, out_ids=out_ids, ids=ids,
                                 proxy_loss=res.proxy_loss, weight=res.weight)
    return module, info
