"""Per-linear calibration: the GPTQ/OWQ reconstruction of an fp16 linear into a packed QuantLinear (reference qeft/recon.py:
GPTQ_OWQ.add_batch / hessian_sorting / fasterquant_reorder; main.py:130-171 for one layer).  DESIGN.md section 4.20.

    acc = HessianAccumulator(K, device);  acc.add_batch(x) per calibration batch        (qeft_hessian_accum)
    module, info = calibrate_linear(linear, acc.H, n_out, name)                         (qeft_gptq_block per 128 columns)
    scale, zero = mse_search(x, bits)       the reference's MSE parameter search, what tuning="mse" runs    (qeft_mse_search)

    U = hinv_factor(Hd)                     the upper factor of Hd^-1 the loop runs on, what factor="own" calls    (qeft_hinv_factor)
    module, info = calibrate_linear(..., pack="device")     the packing step on the GPU as well, DESIGN.md section 4.22  (qeft_quant_pack)
    module, info = rtn_linear(linear, n_out, name, H)       round to nearest, the reference's --nearest / --nearest_owq  (qeft_quant_pack)
    module, info = calibrate_linear(..., loop="rows")       the whole error-feedback loop in ONE launch, a workgroup per 16 rows,
                                                            DESIGN.md section 4.23                                 (qeft_gptq_rows)
    module, info = calibrate_linear(..., loop="rows", tuning="mse_fused")   that launch with the MSE search of every block start
                                                            inside it, DESIGN.md section 4.24                  (qeft_gptq_rows_mse)
    module, info = calibrate_linear(..., group_size=-1)     per-channel, the reference's default: one pair per row, found before
                                                            the loop, DESIGN.md section 4.26   (qeft_gptq_rows_pc, qeft_quant_pack_pc)

GPU tensors only: the kernels have no CPU path and no torch fallback.  Around them the reference's own torch expressions
remain: dead columns, damping, the three Cholesky calls (factor="torch", the default), the trailing update `W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:]` and the
group parameters, which are computed between launches (group size == block size == 128, so a group starts where a block does).
With loop="rows" the last two are inside the one launch as well: nothing of the loop then runs outside HIP.

Out of scope, still: whole-model calibration (layer-by-layer activation capture, the shared outlier index, make_reorder's folding
of the permutation into norms and embeddings), act_order and sym=True.
"""
import types

import torch

from . import _lib
from .qlinear import QuantLinear
from .quant import minmax_params, quantize
from .reorder import sparse_to_dense_ids

BLOCK = 128          # columns per qeft_gptq_block launch == the only supported group size besides -1 (per-channel)


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


def mse_search(x, bits=4, num=40):
    """The same search as mse_params in one launch of qeft_mse_search (csrc/calib_mse.hip): x fp32 [N, g] on the GPU, g <= 32768,
    bits 3 or 4, 1 <= num <= 40; returns (scale, zero) fp32 [N, 1].  A view with stride(1) == 1 is read where it lies (the
    reorder loop passes columns of its working matrix); anything else is copied first.  No CPU path and no torch fallback.

    Every candidate's residuals x - q, and the pair a winning candidate leads to, are the fp32 bits mse_params gives on the CPU.
    The score sum |x - q|^2.4 is the kernel's own (hardware log2 / exp2, ascending columns, the sum and not the mean): relative
    error near 1e-6, so among candidates closer than that another one than torch's may win; exact ties go to the first in the
    reference's order.  Non-finite input, and scores at or above the reference's initial 1e10, are outside the contract."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError(f"x is {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}: qeft_mse_search reads fp32 [N, g]")
    if bits not in (3, 4):
        raise ValueError(f"bits = {bits}: only 3 and 4 are supported")
    _need_gpu(x, "x")
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    n, g = x.shape
    scale = torch.empty((n, 1), dtype=torch.float32, device=x.device)
    zero = torch.empty((n, 1), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().qeft_mse_search(x.data_ptr(), x.stride(0), n, g, 2 ** bits - 1, num, scale.data_ptr(), zero.data_ptr(),
                                          _stream(x.device)))
    return scale, zero


def _params(x, bits, tuning):
    """(scale, zero) fp32 [N, 1] of ONE group holding every column of x."""
    if tuning == "minmax":
        return minmax_params(x, x.shape[1], bits)
    if tuning in ("mse", "mse_fused"):                  # "mse_fused" names where gptq_reorder searches; a whole row is no tile
        return mse_search(x, bits)
    if tuning == "mse_torch":
        return mse_params(x, bits)
    raise ValueError(f"tuning = {tuning!r}: 'minmax', 'mse', 'mse_fused' or 'mse_torch'")


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


def hinv_factor(Hd):
    """The upper-triangular U with Hd^-1 = U^T U -- what cholesky(cholesky_inverse(cholesky(Hd)), upper=True) returns -- by
    qeft_hinv_factor (csrc/calib_factor.hip): ONE blocked factorisation Hd = V V^T from the bottom-right
    corner up and the triangular inverse U = V^-1 riding on the same sweep, 3 K / 128 - 1 launches, fp32, bit-reproducible.
    Hd fp32 [K, K] on the GPU, symmetric positive definite (already permuted and damped), K % 128 == 0; it is not modified (the
    entry works on a copy).  No CPU path and no torch fallback.  Reads the status once (one synchronisation, as the torch route
    has) and raises torch.linalg.LinAlgError naming the column whose pivot was not positive (its .info holds the entry's status)."""
    if not isinstance(Hd, torch.Tensor) or Hd.dtype != torch.float32 or Hd.dim() != 2 or Hd.shape[0] != Hd.shape[1]:
        raise ValueError(f"Hd is {getattr(Hd, 'dtype', type(Hd))} {tuple(getattr(Hd, 'shape', ()))}: qeft_hinv_factor reads fp32 [K, K]")
    K = Hd.shape[0]
    if K < BLOCK or K % BLOCK != 0:
        raise ValueError(f"K = {K}: qeft_hinv_factor needs a multiple of {BLOCK}")
    _need_gpu(Hd, "Hd")
    a = Hd.clone(memory_format=torch.contiguous_format)             # the entry destroys its input
    u = torch.empty_like(a)
    info = torch.empty(1, dtype=torch.int32, device=Hd.device)
    _lib.check(_lib.lib().qeft_hinv_factor(a.data_ptr(), K, u.data_ptr(), info.data_ptr(), K, _stream(Hd.device)))
    code = info.item()
    if code != 0:
        err = torch.linalg.LinAlgError(f"hinv_factor: the pivot of column {code - 1} is not a positive finite number "
                                       f"(info = {code}): the matrix is not positive definite")
        err.info = code
        raise err
    return u


def gptq_reorder(W, H, ids, n_out, bits=4, group_size=128, percdamp=0.01, tuning="minmax", hinv=None, sym=False, factor="torch",
                 loop="blocks"):
    """The reference's fasterquant_reorder (recon.py:488-573) of one weight matrix on the GPU, 128 columns per launch
    (loop="blocks") or the whole loop in one (loop="rows").

    W [N, K] (any float dtype), H fp32 [K, K] as accumulated, ids the column order (select_outliers), the last n_out columns of
    which stay unquantised.  Returns a namespace:
      weight       fp16 [N, K], columns in `ids` order: dequantised values, then the outlier columns WITH the error feedback they
                   received (the reference's Q[:, n_nonout:] = W[:, n_nonout:])
      scale_group, zero_group   fp32 [N, K / 128]: one pair per started group of live columns, the last repeated up to K / 128
                   (recon.py:560-563); K - n_out need not be a multiple of 128 -- the last block and group are short.
                   group_size=-1: fp32 [N, 1], the reference's quantizer.scale shape
      out_ids (int32), ids, bits, group_size, n_out
      proxy_loss   tr((W - Q) H (W - Q)^T) on the undamped H in fp64, Q the fp32 values before the rounding to fp16
    tuning: 'minmax' (quant.minmax_params on the block's current columns), 'mse_fused' (below), 'mse' (mse_search: the reference's default search in
    one launch per block) or 'mse_torch' (mse_params, the same search as 640 torch passes: the comparison route).  hinv: the upper Cholesky factor of the inverse damped Hessian in `ids` order,
    for a caller that has one (it replaces the factorisation).  factor: how that matrix is computed otherwise -- 'torch' (the
    reference's three Cholesky calls) or 'own' (hinv_factor: one blocked factorisation in HIP).
    loop: 'blocks' (the default: per 128 columns a torch min-max, one qeft_gptq_block launch and a rocBLAS GEMM for the trailing
    update) or 'rows' (qeft_gptq_rows, DESIGN.md section 4.23: ONE launch in which a workgroup owns 16 rows and sweeps every
    column of them, the trailing update formed left-looking on the matrix unit; min-max parameters only -- the same lines and,
    from the same block-start columns, the same bits; the trailing sums have another order than rocBLAS's, so the two routes
    agree as closely as either agrees with fp64, not bit for bit).
    tuning='mse_fused' (with loop='rows' only; qeft_gptq_rows_mse): the reference's search, 40 ranges x
    2^bits zero points over each block's current columns, INSIDE the one launch, in the registers of the 16 lanes that hold the
    row's block.  The same candidates and residuals as 'mse'; the score sums have that kernel's own order, so among near-tied
    candidates another one may win: its own name, no bit parity with 'mse'.
    group_size: 128, or -1 = per-channel, the reference's default: ONE pair per row, found over the row's
    live columns of the working matrix before the loop (recon.py:504; here after the dead columns are zeroed, which moves neither a
    min-max that includes 0 nor a score) and used by every block.  loop='blocks' finds it by the tuning's whole-row route and hands
    it to every launch; loop='rows' finds it in a prologue of the one launch (qeft_gptq_rows_pc, or qeft_gptq_rows_pc_mse for
    'mse_fused': the search's scores then have that kernel's own order -- tile sums, tiles ascending)."""
    if loop not in ("blocks", "rows"):
        raise ValueError(f"loop = {loop!r}: 'blocks' or 'rows'")
    if tuning == "mse_fused" and loop != "rows":
        raise ValueError(f"tuning = 'mse_fused' with loop={loop!r}: the search inside the launch exists for loop='rows' only "
                         "-- use tuning='mse' here")
    if loop == "rows" and tuning not in ("minmax", "mse_fused"):
        raise ValueError(f"tuning = {tuning!r} with loop='rows': the MSE search runs between launches -- use loop='blocks', or "
                         "tuning='mse_fused' for the search inside the one launch")
    if group_size not in (BLOCK, -1):
        raise ValueError(f"group_size = {group_size}: only {BLOCK} is supported (a group must start where a block does), or -1: "
                         "per-channel, one pair per row")
    if sym:
        raise ValueError("sym=True is not supported: the block kernel clamps to 0..maxq (asymmetric grid only)")
    if bits not in (3, 4):
        raise ValueError(f"bits = {bits}: only 3 and 4 are supported")
    if n_out % 2 != 0:
        raise ValueError(f"n_out = {n_out}: must be even (the packed outlier slice)")
    N, K = W.shape
    if K % BLOCK != 0:
        raise ValueError(f"K = {K}: must be a multiple of {BLOCK} (scale_group / zero_group hold K / {BLOCK} groups)")
    if factor not in ("torch", "own"):
        raise ValueError(f"factor = {factor!r}: 'torch' or 'own'")
    _need_gpu(W, "W")
    _need_gpu(H, "H")
    if H.shape != (K, K) or not 0 <= n_out < K:
        raise ValueError(f"H {tuple(H.shape)} / n_out {n_out} do not fit W {tuple(W.shape)}")
    dev = W.device
    ids = ids.to(dev).long()
    maxq = 2 ** bits - 1
    n_nonout = K - n_out
    per_channel = group_size == -1

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
        if factor == "own":
            hinv = hinv_factor(Hp)
        else:
            Hp = torch.linalg.cholesky(Hp)
            Hp = torch.cholesky_inverse(Hp)
            hinv = torch.linalg.cholesky(Hp, upper=True)
    hinv = hinv.to(device=dev, dtype=torch.float32).contiguous()
    if hinv.shape != (K, K):
        raise ValueError(f"hinv {tuple(hinv.shape)}: want [{K}, {K}]")

    lib, st = _lib.lib(), _stream(dev)
    if loop == "rows":
        Q = torch.empty_like(Wk)
        err = torch.empty((N, n_nonout), dtype=torch.float32, device=dev)
        scale_group = torch.empty((N, 1 if per_channel else K // BLOCK), dtype=torch.float32, device=dev)
        zero_group = torch.empty_like(scale_group)
        args = (Wk.data_ptr(), K, hinv.data_ptr(), K, Q.data_ptr(), err.data_ptr(), scale_group.data_ptr(), zero_group.data_ptr(),
                N, K, n_nonout, maxq)
        if per_channel:
            _lib.check(lib.qeft_gptq_rows_pc_mse(*args, 40, st) if tuning == "mse_fused" else lib.qeft_gptq_rows_pc(*args, st))
        else:
            _lib.check(lib.qeft_gptq_rows_mse(*args, group_size, 40, st) if tuning == "mse_fused" else
                       lib.qeft_gptq_rows(*args, group_size, st))
        return _reorder_result(W0, Q, H0, scale_group, zero_group, ids, n_nonout, bits, group_size, n_out)
    Q = torch.zeros_like(Wk)
    scales, zeros = [], []
    if per_channel:                                     # the reference's find_params before its loop: one pair, every launch
        scale, zero = (t.contiguous() for t in _params(Wk[:, :n_nonout], bits, tuning))
    for i1 in range(0, n_nonout, BLOCK):
        i2 = min(i1 + BLOCK, n_nonout)
        count = i2 - i1
        if not per_channel:
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
    for _ in range(K // BLOCK - len(scales)):
        scales.append(scales[-1])
        zeros.append(zeros[-1])
    Q[:, n_nonout:] = Wk[:, n_nonout:]
    if per_channel:
        scales, zeros = [scale], [zero]
    return _reorder_result(W0, Q, H0, torch.cat(scales, 1), torch.cat(zeros, 1), ids, n_nonout, bits, group_size, n_out)


def _reorder_result(W0, Q, H0, scale_group, zero_group, ids, n_nonout, bits, group_size, n_out):
    """What gptq_reorder returns, from either loop: the fp16 weight, the groups and the proxy loss in fp64 on the undamped H."""
    E = (W0 - Q).double()
    proxy_loss = ((E @ H0) * E).sum().item()
    return types.SimpleNamespace(weight=Q.to(torch.float16), scale_group=scale_group, zero_group=zero_group,
                                 out_ids=ids[n_nonout:].to(torch.int32), ids=ids, bits=bits, group_size=group_size, n_out=n_out,
                                 proxy_loss=proxy_loss)


def calibrate_linear(linear, H, n_out, name, bits=4, group_size=128, frob_norm=True, outidx=None, pack="host", **kw):
    """One fp16 nn.Linear + its accumulated Hessian -> (QuantLinear, quantinfo): select_outliers -> gptq_reorder ->
    QuantLinear.pack(outlieridx=out_ids, scales=scale_group, zeros=zero_group) -> set_kernel().

    frob_norm: True = weigh diag(H) by frob_norm_error(W) as the reference does by default, False/None = diag(H) alone, or the
    tensor to use.  outidx: fixed outlier columns instead of a selection.  Other keywords go to gptq_reorder (percdamp, tuning,
    hinv, factor, loop; tuning="mse_fused" needs loop="rows", and the whole-row search of frob_norm_error is then mse_search's).
    The quantinfo namespace carries what checkpoint.save_packed / quant.lm_pack read (bits, sym, group_size, n_out,
    reorder, scale_group, zero_group, out_ids) plus ids and proxy_loss, so the layer saves and loads like any other.

    The packed columns are in `ids` order.  A module whose name contains 'o_proj' or 'out_proj' gathers its own input
    (set_kernel installs reorder_ids == ids); for any other name the caller feeds x[..., ids] until the offline global reordering
    exists.  n_out = 0 is plain GPTQ: nothing is selected and ids is the identity.

    pack: "host" (the default) copies the reconstruction to the CPU, runs QuantLinear.pack there and copies the module back;
    "device" runs QuantLinear.pack_device (one launch of qeft_quant_pack): the same buffers bit for bit,
    and no tensor leaves the GPU.  group_size=-1: a per-channel layer (scales [1, N]; "device" is qeft_quant_pack_pc)."""
    if pack not in ("host", "device"):
        raise ValueError(f"pack = {pack!r}: 'host' or 'device'")
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
    if pack == "device":
        holder = types.SimpleNamespace(weight=types.SimpleNamespace(data=res.weight), bias=linear.bias)
        module = module.to(W.device)
        module.pack_device(holder, scales=res.scale_group, zeros=res.zero_group, outlieridx=out_ids)
    else:
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


def rtn_linear(linear, n_out, name, H=None, outidx=None, bits=4, group_size=128, frob_norm=True, tuning="minmax"):
    """Round to nearest: the reference's --nearest (n_out == 0) and --nearest_owq (GPTQ_OWQ.fasterquant_nearest_owq_reorder,
    recon.py:327-384) of one fp16 nn.Linear on the GPU -> (QuantLinear, quantinfo), with no error feedback and no factorisation.

    n_out > 0: the outlier columns come from select_outliers (diag(H), weighed by frob_norm as in calibrate_linear, or `outidx`
    as given; one of H and outidx is required) and stay fp16; the other columns, in `ids` order, are quantised per 128-column
    group with the min-max parameters of the group's live columns -- gather, search, rounding and packing in ONE launch of
    qeft_quant_pack (QuantLinear.pack_device in find mode); group_size=-1: per ROW, over all its live
    columns, in one launch of qeft_quant_pack_pc.  The quantinfo namespace has the fields
    calibrate_linear returns (proxy_loss is None: no Hessian is needed here; weight is not kept), so the layer saves and loads
    like any other, and the same rule for o_proj / out_proj names applies.  Only tuning="minmax": the MSE search is refused."""
    if tuning != "minmax":
        raise ValueError(f"tuning = {tuning!r}: rtn_linear finds min-max parameters inside the pack launch; the MSE search "
                         "runs only in calibrate_linear")
    if group_size not in (BLOCK, -1):
        raise ValueError(f"group_size = {group_size}: only {BLOCK} is supported, or -1: per-channel")
    if bits not in (3, 4):
        raise ValueError(f"bits = {bits}: only 3 and 4 are supported")
    W = linear.weight.data
    _need_gpu(W, "linear.weight")
    N, K = W.shape
    if n_out % 2 != 0 or not 0 <= n_out < K:
        raise ValueError(f"n_out = {n_out}: must be even and in 0 .. K - 1 = {K - 1}")
    dev = W.device
    if n_out == 0:
        out_ids, ids, col_ids = torch.zeros(0, dtype=torch.int32, device=dev), torch.arange(K, device=dev), None
    else:
        if H is None and outidx is None:
            raise ValueError("rtn_linear with n_out > 0 needs H (to select the outlier columns) or outidx")
        if H is None:
            out_ids = outidx.to(device=dev, dtype=torch.int32)
            ids = sparse_to_dense_ids(out_ids, K)
        else:
            _need_gpu(H, "H")
            if frob_norm is True:
                frob_norm = frob_norm_error(W, bits, group_size, tuning)
            elif frob_norm is False:
                frob_norm = None
            out_ids, ids = select_outliers(H, n_out, frob_norm=frob_norm, outidx=outidx)
        col_ids = ids.to(torch.int32)
    module = QuantLinear(bits, K, N, linear.bias is not None, torch.float16, n_out, group_size, True, name).to(dev)
    holder = types.SimpleNamespace(weight=types.SimpleNamespace(data=W.to(torch.float16)), bias=linear.bias)
    scale, zero = module.pack_device(holder, None, None, out_ids, col_ids=col_ids)
    module.set_kernel()
    info = types.SimpleNamespace(bits=bits, sym=False, group_size=group_size, n_out=n_out, reorder=True, scale_group=scale,
                                 zero_group=zero, out_ids=out_ids, ids=ids, proxy_loss=None, weight=None)
    return module, info
