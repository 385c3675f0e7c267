"""Reference of the e4m3 KV cache (include/qeft_hip.h, "FP8 KV cache"; csrc/decode_attn_kv8.hip) in torch: the recipe that turns a
row of 128 fp16 values into codes and a scale, the dequantiser, and an fp64 attention over a dequantised cache.  The fp32 divides
and the fp32 product are torch's (correctly rounded, as the kernel's); torch's cast to float8_e4m3fn rounds to nearest even and
does NOT saturate, so the clamp comes first."""
import torch

HD = 128
FP8_MAX = 448.0
NAN8 = 0x7F                 # an e4m3fn NaN code


def quant_rows(x):
    """x [..., 128] (the fp16 values an fp16 cache would hold) -> (codes uint8 [..., 128], scales fp32 [...])."""
    x = x.float()
    amax = x.abs().amax(-1)
    zero = amax == 0
    safe = torch.where(zero, torch.ones_like(amax), amax)
    inv = torch.tensor(FP8_MAX, dtype=torch.float32, device=x.device) / safe
    scale = safe / torch.tensor(FP8_MAX, dtype=torch.float32, device=x.device)
    y = (x * inv[..., None]).clamp(-FP8_MAX, FP8_MAX)
    codes = y.to(torch.float8_e4m3fn).view(torch.uint8)
    codes = torch.where(zero[..., None], torch.zeros_like(codes), codes)
    return codes, torch.where(zero, torch.zeros_like(scale), scale)


def dequant_rows(codes, scales, dtype=torch.float32):
    """float(code) * scale, the product taken in `dtype` (exact in fp64: 4 x 24 significant bits)."""
    return codes.view(torch.float8_e4m3fn).to(dtype) * scales[..., None].to(dtype)


def rot(x, c, s):
    """neox-style rotary as the kernels: x [..., 128] fp32, c / s [..., 64]."""
    a, b = x[..., :64], x[..., 64:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def attention_fp64(q, kc, vc, ks, vs, pos):
    """One query token: q [heads, 128] (rotated, scaled, rounded to fp16 by the caller) against rows [0, pos] of ONE slot's cache
    (codes [n_kv, max_seq, 128], scales [n_kv, max_seq]) as the launch left it -> fp64 [heads * 128]."""
    heads, grp = q.shape[0], q.shape[0] // kc.shape[0]
    Lk = pos + 1
    out = torch.empty(heads, HD, dtype=torch.float64, device=q.device)
    for h0 in range(0, heads, 8):           # 8 heads at a time: a 32768-key fp64 cache of all heads would be gigabytes
        hs = torch.arange(h0, min(h0 + 8, heads), device=q.device)
        K = dequant_rows(kc[hs // grp, :Lk], ks[hs // grp, :Lk], torch.float64)
        V = dequant_rows(vc[hs // grp, :Lk], vs[hs // grp, :Lk], torch.float64)
        sc = torch.einsum("hd,hld->hl", q[hs].double(), K)
        out[hs] = torch.einsum("hl,hld->hd", sc.softmax(-1), V)
    return out.reshape(heads * HD)
