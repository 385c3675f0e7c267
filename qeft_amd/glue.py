"""The glue of a training step on the project's own kernels (csrc/train_glue.hip): what sits between the
linears, attention and the head of finetune.causal_lm_loss(glue="fused").

    add_rmsnorm(h, add, gamma, eps) -> (s, y)   s = fp16(h + add) (h itself when add is None), y = rmsnorm(s) * gamma
    swiglu(gate, up)                -> act      fp16(silu(gate) * up)
    rope_qk(q, k, cos, sin)         -> (q_rot, k_rot)   the rotary of every head of q and k in one launch (section 4.17;
                                                causal_lm_loss(rope="fused")), the bits of finetune._rope in both directions

Each is a torch.autograd.Function over one forward and one backward entry: fp32 math, every result rounded to fp16 once, nothing
saved but the operands (the norm's statistic is recomputed).  rope_qk is one entry in both directions, saves the tables alone
and rounds where the torch expression rounds.  add_rmsnorm's backward takes the gradient of s -- what reaches the
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


# ------------------------------------------------------------------------------------------------ rotary of q and k
HEAD = 128


def _head_rows(x):
    """x [B, T, heads, 128] as qeft_rope_qk takes it, as attention._rows does: heads * 128 dense fp16 per row, a row stride that
    is a multiple of 8, batch b at row b * T, 16-byte aligned -- a [B, T] view of a fused q|k|v buffer passes as it lies -- or a
    dense copy."""
    B, T, Hn, _ = x.shape
    ok = x.stride(3) == 1 and x.stride(2) == HEAD and x.stride(1) % 8 == 0 and Hn * HEAD <= x.stride(1) <= 1 << 24 \
        and x.data_ptr() % 16 == 0 and (B == 1 or x.stride(0) == T * x.stride(1))
    return x if ok else _dense(x)


def rope_qk_entry(q, k, cos, sin, inverse=False):
    """The entry on q [B, T, H, 128], k [B, T, Hkv, 128] (rows as _head_rows leaves them) and dense cos / sin [T, 64] fp32:
    (q_out, k_out), dense.  inverse: the transpose -- the backward, on the gradients of the outputs."""
    B, T, H, _ = q.shape
    Hkv = k.shape[2]
    q_out = torch.empty(B, T, H, HEAD, dtype=torch.float16, device=q.device)
    k_out = torch.empty(B, T, Hkv, HEAD, dtype=torch.float16, device=q.device)
    _lib.check(_lib.lib().qeft_rope_qk(q.data_ptr(), k.data_ptr(), cos.data_ptr(), sin.data_ptr(), q_out.data_ptr(), k_out.data_ptr(),
                                       B * T, T, H, Hkv, q.stride(1), k.stride(1), 1 if inverse else 0, _stream(q.device)))
    return q_out, k_out


class _RopeQK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin):
        ctx.save_for_backward(cos, sin)
        ctx.shapes = (q.shape, k.shape)
        ctx.set_materialize_grads(False)
        return rope_qk_entry(q, k, cos, sin)

    @staticmethod
    def backward(ctx, dq, dk):
        need_q, need_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (dq is None and dk is None) or not (need_q or need_k):
            return None, None, None, None
        cos, sin = ctx.saved_tensors
        # one launch for both; a missing gradient is zero, and the transpose of zero is exactly zero
        dq = torch.zeros(ctx.shapes[0], dtype=torch.float16, device=cos.device) if dq is None else _head_rows(dq)
        dk = torch.zeros(ctx.shapes[1], dtype=torch.float16, device=cos.device) if dk is None else _head_rows(dk)
        gq, gk = rope_qk_entry(dq, dk, cos, sin, inverse=True)
        return gq if need_q else None, gk if need_k else None, None, None


def rope_qk(q, k, cos, sin):
    """The NeoX rotary of finetune._rope on q [B, T, H, 128] and k [B, T, Hkv, 128] (fp16, GPU) in one launch of qeft_rope_qk:
    cos / sin fp32 [T, 64], row t of every sequence at position t.  Returns (q_rot, k_rot), dense, in the inputs' shapes, with
    the bits of the torch expression (each product and their sum rounded to fp32, then to fp16); differentiable in q and k through
    one inverse launch on (dq_rot, dk_rot), which gives the bits of that expression's autograd.  Inputs and gradients are taken
    as views where they already are rows at a legal stride, as a dense copy otherwise."""
    _need_gpu_f16("rope_qk", q=q, k=k)
    for nm, x in (("cos", cos), ("sin", sin)):
        if not torch.is_tensor(x):
            raise ValueError(f"rope_qk: {nm} must be a tensor")
        if not x.is_cuda:
            raise RuntimeError(f"rope_qk needs GPU tensors (there is no CPU path): {nm} is on {x.device}")
        if x.dtype != torch.float32:
            raise ValueError(f"rope_qk takes fp32 tables, got {nm} {x.dtype}")
    if q.dim() != 4 or k.dim() != 4 or q.shape[3] != HEAD or k.shape[3] != HEAD:
        raise ValueError(f"rope_qk takes q [B, T, H, 128] and k [B, T, Hkv, 128], got {tuple(q.shape)} and {tuple(k.shape)}")
    B, T, H, _ = q.shape
    if k.shape[:2] != (B, T):
        raise ValueError(f"rope_qk: k {tuple(k.shape)} for q {tuple(q.shape)}")
    if not (1 <= H <= 256 and 1 <= k.shape[2] <= 256):
        raise ValueError(f"rope_qk takes 1 .. 256 heads, got {H} and {k.shape[2]}")
    if T < 1 or not 1 <= B * T <= MAX_ROWS:
        raise ValueError(f"rope_qk takes 1 .. 2^20 rows, got {B} x {T}")
    if cos.shape != (T, HEAD // 2) or sin.shape != (T, HEAD // 2):
        raise ValueError(f"rope_qk: cos {tuple(cos.shape)} and sin {tuple(sin.shape)} for T = {T}: both must be [T, 64]")
    return _RopeQK.apply(_head_rows(q), _head_rows(k), _dense(cos), _dense(sin))
