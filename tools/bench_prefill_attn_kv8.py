"""The prompt attention over an e4m3 cache (qeft_attn_prefill_kv8) against the route it replaces: one GPU, one
process, HIP events, a warm-up before every measurement, the sides of a point alternating (medians of --reps windows) --
tools/bench_prefill_attn.py's method and helpers.

    python tools/bench_prefill_attn_kv8.py [--reps 10] [--skip-e2e] > profiles/prefill_attn_kv8_bench.json.log

Per layer-piece, head layouts (32, 32) and (64, 8), (start, t) = (2048, 512), (14336, 512), (14336, 2048):
  a  the image route: cat(kv8_decode_rows(codes[:, :start], scales[:, :start]), the chunk's rows), for K and for V, and
     qeft_attn_prefill over the two images -- what llama._own_attention did on an fp8 cache before the kernel;
  b  qeft_attn_prefill alone on an fp16 cache that holds the same values (the image of a, built once);
  c  qeft_attn_prefill_kv8 on the codes, the scales and the chunk's rows;
and the peak of torch.cuda.max_memory_allocated above what was allocated before the call, for a and for c.  c and a are compared
bit for bit before they are timed.
End to end: DecodeEngine(kv_dtype="fp8").extend of 512 tokens at positions 2048 and 14336 on the Llama-2-7B shape (synthetic
weights, max_seq 16384), as the package runs it and with llama._own_attention replaced by the image route (the previous
commit's function, same library, same process).
Every step runs under its own time limit and the first failure ends the run.  One JSON line per point; c_over_a <= 1 and
extend_over_image_route <= 1 are the expectation, c_over_b is reported."""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_prefill_attn import DEV, HD, limit, medians_us, st  # noqa: E402


def quant_rows(x):
    """include/qeft_hip.h, THE RECIPE, in torch: x [..., 128] fp16 -> (codes uint8, scales fp32)."""
    x = x.float()
    amax = x.abs().amax(-1)
    safe = torch.where(amax == 0, torch.ones_like(amax), amax)
    codes = (x * (448.0 / safe)[..., None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, torch.where(amax == 0, torch.zeros_like(amax), safe / 448.0)


def image(codes, scales, rows, start):
    from qeft_amd.llama import kv8_decode_rows
    return torch.cat([kv8_decode_rows(codes[:, :start], scales[:, :start]), rows.transpose(0, 1)], 1).contiguous()


def peak_above_base(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def kernel_points(reps):
    from qeft_amd import _lib
    lib, ck = _lib.lib(), _lib.check
    g = torch.Generator(device=DEV).manual_seed(0)
    for heads, kv in ((32, 32), (64, 8)):
        for start, t in ((2048, 512), (14336, 512), (14336, 2048)):
            with limit(300):
                L = start + t
                qkv = torch.randn(t, (heads + 2 * kv) * HD, generator=g, device=DEV).half()
                kc, ks = quant_rows((torch.randn(kv, L, HD, generator=g, device=DEV) * 0.5).half())
                vc, vs = quant_rows((torch.randn(kv, L, HD, generator=g, device=DEV) * 0.5).half())
                k = qkv[:, heads * HD:(heads + kv) * HD].view(t, kv, HD)          # views of q|k|v, as prefill holds them
                v = qkv[:, (heads + kv) * HD:].view(t, kv, HD)
                out_a, out_b, out_c = (torch.empty(t, heads * HD, dtype=torch.float16, device=DEV) for _ in range(3))

                def f16_launch(kimg, vimg, out):
                    ck(lib.qeft_attn_prefill(qkv.data_ptr(), qkv.stride(0), kimg.data_ptr(), vimg.data_ptr(), L, out.data_ptr(),
                                             out.stride(0), start, t, heads, kv, st()))

                def a():
                    f16_launch(image(kc, ks, k, start), image(vc, vs, v, start), out_a)
                kimg, vimg = image(kc, ks, k, start), image(vc, vs, v, start)

                def b():
                    f16_launch(kimg, vimg, out_b)

                def c():
                    ck(lib.qeft_attn_prefill_kv8(qkv.data_ptr(), qkv.stride(0), kc.data_ptr(), vc.data_ptr(), ks.data_ptr(),
                                                 vs.data_ptr(), L, k.data_ptr(), v.data_ptr(), k.stride(0), out_c.data_ptr(),
                                                 out_c.stride(0), start, t, heads, kv, st()))
                a(), b(), c()
                torch.cuda.synchronize()
                same = torch.equal(out_a.view(torch.int16), out_c.view(torch.int16))
                peak_a, peak_c = peak_above_base(a), peak_above_base(c)
                u_a, u_b, u_c = medians_us((a, b, c), reps, inner=4)
                flops = 4.0 * heads * HD * (t * start + t * (t + 1) / 2)
                print(json.dumps(dict(bench="attn_prefill_kv8", heads=heads, kv=kv, start=start, t=t, reps=reps,
                                      a_image_route_us=round(u_a, 1), b_fp16_launch_us=round(u_b, 1), c_kv8_launch_us=round(u_c, 1),
                                      c_over_a=round(u_c / u_a, 4), c_over_b=round(u_c / u_b, 3),
                                      c_TFLOPs=round(flops / u_c * 1e-6, 1), c_bits_equal_a=same,
                                      a_peak_bytes=peak_a, c_peak_bytes=peak_c, image_bytes=2 * kv * L * HD * 2)), flush=True)
                if not same:
                    raise SystemExit("qeft_attn_prefill_kv8 and the image route disagree")
                del qkv, kc, ks, vc, vs, kimg, vimg
                torch.cuda.empty_cache()


def image_route_attention(kv, li, q, k, v, start, T, n_heads, n_kv):
    """llama._own_attention on an fp8 cache as it was before qeft_attn_prefill_kv8."""
    from qeft_amd import _lib
    kv.store_kv(li, k, v, T, start)
    kimg, vimg = image(kv.kc[li], kv.ks[li], k, start), image(kv.vc[li], kv.vs[li], v, start)
    if not (q.stride(2) == 1 and q.stride(1) == 128 and q.stride(0) % 8 == 0):
        q = q.contiguous()
    out = torch.empty(T, n_heads * 128, dtype=torch.float16, device=q.device)
    _lib.check(_lib.lib().qeft_attn_prefill(q.data_ptr(), q.stride(0), kimg.data_ptr(), vimg.data_ptr(), kimg.shape[1],
                                            out.data_ptr(), out.stride(0), start, T, n_heads, n_kv, st()))
    return out


def e2e_points(reps):
    from qeft_amd import llama
    t = 512
    with limit(400):
        model = llama.QuantLlama(dataclasses.replace(llama.LLAMA2_7B, max_seq=16384), DEV, seed=0, fast_init=True)
        eng = llama.DecodeEngine(model, use_graph=False, kv_dtype="fp8")
        g = torch.Generator(device=DEV).manual_seed(2)
        for codes, scales in zip(eng.kc + eng.vc, eng.ks + eng.vs):           # a past of plausible rows in every layer
            codes.copy_(torch.randint(0, 0x7f, codes.shape, generator=g, device=DEV, dtype=torch.uint8))
            scales.fill_(2.0 / 448)
        toks = torch.randint(0, model.shape.vocab, (t,), generator=torch.Generator().manual_seed(1)).to(DEV)
        own = llama._own_attention

    for pos in (2048, 14336):
        def run(route):
            llama._own_attention = route
            try:
                eng.set_position(pos)
                return eng.extend(toks)
            finally:
                llama._own_attention = own
        with limit(600):
            new, old = run(own), run(image_route_attention)
            torch.cuda.synchronize()
            same = torch.equal(new.view(torch.int16), old.view(torch.int16))
            peak_new, peak_old = peak_above_base(lambda: run(own)), peak_above_base(lambda: run(image_route_attention))
            u_new, u_old = medians_us((lambda: run(own), lambda: run(image_route_attention)), reps, inner=1, warm=1)
        print(json.dumps(dict(bench="extend_e2e_kv8", model="Llama-2-7B shape, synthetic weights, kv_dtype=fp8", position=pos, tokens=t,
                              reps=reps, extend_ms=round(u_new * 1e-3, 2), extend_image_route_ms=round(u_old * 1e-3, 2),
                              extend_over_image_route=round(u_new / u_old, 4), logits_bits_equal=same,
                              peak_bytes=peak_new, image_route_peak_bytes=peak_old)), flush=True)
        if not same:
            raise SystemExit("extend on qeft_attn_prefill_kv8 and on the image route disagree")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    print(json.dumps(dict(bench="prefill_attn_kv8", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    kernel_points(a.reps)
    if not a.skip_e2e:
        e2e_points(a.reps)
