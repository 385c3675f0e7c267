"""Causal attention for training on the project's own kernels.

    causal_attention(q, k, v)       q [B, T, H, 128], k / v [B, T, Hkv, 128] fp16 -> [B, T, H, 128] fp16, differentiable

The forward is qeft_attn_train_fwd -- the body of the prompt attention (qeft_attn_prefill) reading K and V from the projections'
own row-major output, with the per-row log-sum-exp kept for the backward; the backward is qeft_attn_train_bwd: delta, dK / dV and
dQ launches, no atomics, every sequence's gradients independent of the batch around it bit for bit.  Grouped-query layouts are
read in place: no repeat_interleave, no H-head dK / dV to sum back.  Every sequence of the batch starts at position 0 and
attends itself alone; there is no mask other than the causal one, no dropout and no CPU path.
"""
import torch

from . import _lib

HEAD = 128

_workspace = {}              # device -> uint8 buffer for the backward's delta, grown on demand (as scoring's workspaces)


def _rows(x):
    """x [B, T, heads, 128] as the entries take it -- rows of heads * 128 dense fp16, a row stride that is a multiple of 8, batch
    b at row b * T, 16-byte aligned -- or a contiguous copy.  A [B * T] view of a fused q|k|v buffer passes as it lies."""
    B, T, Hn, _ = x.shape
    ok = x.stride(3) == 1 and x.stride(2) == HEAD and x.stride(1) % 8 == 0 and x.stride(1) >= Hn * HEAD and x.data_ptr() % 16 == 0 \
        and (B == 1 or x.stride(0) == T * x.stride(1))
    return x if ok else x.contiguous()


def attn_train_fwd(q, k, v):
    """The forward entry on [B, T, heads, 128] tensors: (out fp16 [B, T, H, 128] contiguous, lse fp32 [B, T, H])."""
    B, T, H, _ = q.shape
    Hkv = k.shape[2]
    q, k, v = _rows(q), _rows(k), _rows(v)
    if k.stride(1) != v.stride(1):
        k, v = k.contiguous(), v.contiguous()
    dev = q.device
    out = torch.empty(B, T, H, HEAD, dtype=torch.float16, device=dev)
    lse = torch.empty(B, T, H, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().qeft_attn_train_fwd(q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1), out.data_ptr(),
                                              H * HEAD, lse.data_ptr(), B, T, H, Hkv, torch.cuda.current_stream(dev).cuda_stream))
    return out, lse


def attn_train_bwd(q, k, v, out, lse, dout):
    """The backward entry: (dq [B, T, H, 128], dk, dv [B, T, Hkv, 128]) fp16 contiguous, from the forward's out and lse."""
    B, T, H, _ = q.shape
    Hkv = k.shape[2]
    q, k, v, out, dout = _rows(q), _rows(k), _rows(v), _rows(out), _rows(dout)
    if k.stride(1) != v.stride(1):
        k, v = k.contiguous(), v.contiguous()
    lse = lse.contiguous()
    dev = q.device
    lib = _lib.lib()
    need = lib.qeft_attn_train_bwd_workspace_bytes(B, T, H, Hkv)
    if need == 0:
        raise ValueError(f"qeft_attn_train_bwd does not take B={B}, T={T}, {H} / {Hkv} heads")
    ws = _workspace.get(dev)
    if ws is None or ws.numel() < need:
        _workspace[dev] = None
        ws = _workspace[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    dq = torch.empty(B, T, H, HEAD, dtype=torch.float16, device=dev)
    dk = torch.empty(B, T, Hkv, HEAD, dtype=torch.float16, device=dev)
    dv = torch.empty(B, T, Hkv, HEAD, dtype=torch.float16, device=dev)
    _lib.check(lib.qeft_attn_train_bwd(q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1), out.data_ptr(),
                                       out.stride(1), dout.data_ptr(), dout.stride(1), lse.data_ptr(), dq.data_ptr(), H * HEAD,
                                       dk.data_ptr(), dv.data_ptr(), Hkv * HEAD, ws.data_ptr(), ws.numel(), B, T, H, Hkv,
                                       torch.cuda.current_stream(dev).cuda_stream))
    return dq, dk, dv


class _CausalAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v):
        out, lse = attn_train_fwd(q, k, v)
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = attn_train_bwd(q, k, v, out, lse, dout)
        need = ctx.needs_input_grad
        return dq if need[0] else None, dk if need[1] else None, dv if need[2] else None


def causal_attention(q, k, v):
    """Causal softmax(q k^T / sqrt(128)) v per sequence and head: q [B, T, H, 128], k and v [B, T, Hkv, 128], fp16 on the GPU,
    H % Hkv == 0 (query head h reads kv head h // (H // Hkv)); returns [B, T, H, 128] fp16.  Differentiable in q, k and v
    through qeft_attn_train_bwd; an input that does not require a gradient gets None.  Inputs whose last two dims are not dense
    (or whose k / v row strides differ) are copied contiguous first; views of a fused q|k|v buffer are read in place."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError(f"causal_attention takes q [B, T, H, 128] and k, v [B, T, Hkv, 128], got {tuple(q.shape)}, "
                         f"{tuple(k.shape)}, {tuple(v.shape)}")
    B, T, H, D = q.shape
    if D != HEAD or k.shape[3] != HEAD or v.shape[3] != HEAD:
        raise ValueError(f"causal_attention is built for a head size of {HEAD}, got {D}, {k.shape[3]}, {v.shape[3]}")
    if k.shape != v.shape or k.shape[:2] != (B, T):
        raise ValueError(f"k {tuple(k.shape)} and v {tuple(v.shape)} must both be [{B}, {T}, Hkv, {HEAD}]")
    Hkv = k.shape[2]
    if H < 1 or Hkv < 1 or H % Hkv != 0:
        raise ValueError(f"{H} query heads are no multiple of {Hkv} kv heads")
    if not (q.dtype == k.dtype == v.dtype == torch.float16):
        raise ValueError(f"causal_attention takes fp16, got {q.dtype}, {k.dtype}, {v.dtype}")
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise RuntimeError("causal_attention needs GPU tensors (there is no CPU path)")
    if B * T == 0:
        raise ValueError("causal_attention needs at least one row")
    return _CausalAttention.apply(q, k, v)
