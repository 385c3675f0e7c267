"""The glue of a training step on the project's own kernels (csrc/train_glue.hip): what sits between the
linears, attention and the head of finetune.causal_lm_loss(glue="fused").

    add_rmsnorm(h, add, gamma, eps) -> (s, y)   s = fp16(h + add) (h itself when add is None), y = rmsnorm(s) * gamma
    swiglu(gate, up)                -> act      fp16(silu(gate) * up)

Each is a torch.autograd.Function over one forward and one backward entry: fp32 math, every result rounded to fp16 once, nothing
saved but the operands (the norm's statistic is recomputed).  add_rmsnorm's backward takes the gradient of s -- what reaches the
residual stream from further on -- and the gradient of y in one launch and returns their sum through the norm with a single
rounding, so a decoder layer that threads
(s, delta) through add_rmsnorm has no residual add left for torch in either direction.  gamma is frozen: it gets no gradient.  A
missing output gradient is zero, an input that needs no gradient gets None.  fp16 GPU tensors only: there is no CPU path and no
fallback to torch ops -- a shape the entries refuse is a ValueError.
"""
import torch

from . import _lib

MAX_ROWS = 1 << 20


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _need_gpu_f16(name, **tensors):
    for nm, x in tensors.items():
        if x is None:
            continue
        if not torch.is_tensor(x):
            raise ValueError(f"{name}: {nm} must be a tensor")
        if not x.is_cuda:
            raise RuntimeError(f"{name} needs GPU tensors (there is no CPU path): {nm} is on {x.device}")
        if x.dtype != torch.float16:
            raise ValueError(f"{name} takes fp16, got {nm} {x.dtype}")


def _dense(x):
    """x itself where it is contiguous and 16-byte aligned, else a copy that is."""
    x = x.contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone()


def _rows2d(x):
    """x [..., n] as rows the SwiGLU entries take: [m, n] with unit column stride, a row stride that is a multiple of 8 and 16-byte
    aligned -- a view where x already is that (a slice of a fused gate|up buffer passes), a dense copy otherwise."""
    n = x.shape[-1]
    if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.stride(0) >= n and x.data_ptr() % 16 == 0:
        return x
    return _dense(x.reshape(-1, n))


# ------------------------------------------------------------------------------------------------ RMSNorm + residual add
def add_rmsnorm_fwd(h, add, gamma, eps):
    """The forward entry on dense [m, hidden] tensors: (s, y); s is h itself without add."""
    m, hidden = h.shape
    y = torch.empty_like(h)
    s = h if add is None else torch.empty_like(h)
    _lib.check(_lib.lib().qeft_add_rmsnorm_fwd(h.data_ptr(), None if add is None else add.data_ptr(), gamma.data_ptr(),
                                               None if add is None else s.data_ptr(), y.data_ptr(), m, hidden, eps, _stream(h.device)))
    return s, y


def add_rmsnorm_bwd(s, gamma, dy, dres, eps):
    """The backward entry: dsum [m, hidden] from s, the gradient dy of y and the gradient dres of s (either may be None)."""
    m, hidden = s.shape
    dsum = torch.empty_like(s)
    _lib.check(_lib.lib().qeft_add_rmsnorm_bwd(s.data_ptr(), gamma.data_ptr(), None if dy is None else dy.data_ptr(),
                                               None if dres is None else dres.data_ptr(), dsum.data_ptr(), m, hidden, eps,
                                               _stream(s.device)))
    return dsum


class _AddRmsNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, add, gamma, eps):
        s, y = add_rmsnorm_fwd(h, add, gamma, eps)
        ctx.save_for_backward(s, gamma)
        ctx.eps, ctx.has_add = eps, add is not None
        ctx.set_materialize_grads(False)
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        need_h, need_add = ctx.needs_input_grad[0], ctx.has_add and ctx.needs_input_grad[1]
        if (ds is None and dy is None) or not (need_h or need_add):
            return None, None, None, None
        s, gamma = ctx.saved_tensors
        dsum = add_rmsnorm_bwd(s, gamma, None if dy is None else _dense(dy), None if ds is None else _dense(ds), ctx.eps)
        return dsum if need_h else None, dsum if need_add else None, None, None


def add_rmsnorm(h, add, gamma, eps):
    """s = fp16(h + add) and y = fp16(s * rsqrt(mean s^2 + eps) * gamma) over the rows of h [m, hidden] (fp16, GPU); gamma
    [hidden] fp16, frozen.  add=None: no sum is formed and s is h (the very tensor when h needs no gradient, else an alias that
    carries the fused backward).  Differentiable in h and add: both receive fp16(ds + d(norm)(dy)) from one launch, rounded once;
    ds or dy may be missing.  The bits of s and y are qeft_rmsnorm's."""
    _need_gpu_f16("add_rmsnorm", h=h, add=add, gamma=gamma)
    if h.dim() != 2:
        raise ValueError(f"add_rmsnorm takes h [m, hidden], got {tuple(h.shape)}")
    m, hidden = h.shape
    if add is not None and add.shape != h.shape:
        raise ValueError(f"add_rmsnorm: add {tuple(add.shape)} for h {tuple(h.shape)}")
    if gamma.shape != (hidden,):
        raise ValueError(f"add_rmsnorm: gamma {tuple(gamma.shape)} for hidden {hidden}")
    if hidden < 8 or hidden % 8 != 0:
        raise ValueError(f"add_rmsnorm takes a hidden size that is a multiple of 8, got {hidden}")
    if not 1 <= m <= MAX_ROWS:
        raise ValueError(f"add_rmsnorm takes 1 .. 2^20 rows, got {m}")
    hd = _dense(h)
    s, y = _AddRmsNorm.apply(hd, None if add is None else _dense(add), _dense(gamma), float(eps))
    if add is None and hd is h and not (h.requires_grad and torch.is_grad_enabled()):
        s = h
    return s, y


# ------------------------------------------------------------------------------------------------ SwiGLU
def swiglu_fwd(gate, up):
    m, n = gate.shape
    out = torch.empty(m, n, dtype=torch.float16, device=gate.device)
    _lib.check(_lib.lib().qeft_swiglu_fwd(gate.data_ptr(), up.data_ptr(), out.data_ptr(), m, n, gate.stride(0), up.stride(0),
                                          _stream(gate.device)))
    return out


def swiglu_bwd(gate, up, dact):
    m, n = gate.shape
    dgate = torch.empty(m, n, dtype=torch.float16, device=gate.device)
    dup = torch.empty(m, n, dtype=torch.float16, device=gate.device)
    _lib.check(_lib.lib().qeft_swiglu_bwd(gate.data_ptr(), up.data_ptr(), dact.data_ptr(), dgate.data_ptr(), dup.data_ptr(), m, n,
                                          gate.stride(0), up.stride(0), dact.stride(0), n, n, _stream(gate.device)))
    return dgate, dup


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        ctx.save_for_backward(gate, up)
        ctx.set_materialize_grads(False)
        return swiglu_fwd(gate, up)

    @staticmethod
    def backward(ctx, dact):
        need = ctx.needs_input_grad
        if dact is None or not (need[0] or need[1]):
            return None, None
        gate, up = ctx.saved_tensors
        dgate, dup = swiglu_bwd(gate, up, _rows2d(dact))
        return dgate if need[0] else None, dup if need[1] else None


def swiglu(gate, up):
    """fp16(silu(gate) * up) over gate, up [..., n] (fp16, GPU; n % 8 == 0), the bits of qeft_silu_mul; returns the same shape,
    dense.  Differentiable in both through qeft_swiglu_bwd; the fp32 temporaries of the torch expression never exist."""
    _need_gpu_f16("swiglu", gate=gate, up=up)
    if gate.shape != up.shape or gate.dim() < 1:
        raise ValueError(f"swiglu: gate {tuple(gate.shape)} and up {tuple(up.shape)} must have one shape")
    n = gate.shape[-1]
    if n < 8 or n % 8 != 0:
        raise ValueError(f"swiglu takes a width that is a multiple of 8, got {n}")
    m = gate.numel() // n
    if not 1 <= m <= MAX_ROWS:
        raise ValueError(f"swiglu takes 1 .. 2^20 rows, got {m}")
    return _SwiGLU.apply(_rows2d(gate), _rows2d(up)).view(gate.shape)
