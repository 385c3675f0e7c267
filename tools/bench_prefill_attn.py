"""The prompt attention kernel (qeft_attn_prefill) against what serves the same rows without it: one GPU, one
process, HIP events, a warm-up before every measurement, the sides of a point alternating (medians of --reps windows).

    python tools/bench_prefill_attn.py [--reps 10] [--skip-e2e] > profiles/prefill_attn_bench.json.log

start = 0, t = 512 / 2048 on the head layouts (32, 32) and (64, 8): one launch of the kernel (q a view of the fused q|k|v output,
K / V read from a cache image) against the scaled_dot_product_attention call llama.prefill makes on the same tensors in the same
run -- the call alone, and with the repeat_interleave of K / V in front of it and the transpose + copy of its output behind it
that the SDPA path needs and the kernel does not.
start > 0, (start, t) = (2048, 512) and (14336, 2048): against SDPA over the concatenated keys with an explicit boolean mask,
the only way to serve a continued chunk without the kernel (mask built outside the timing).
End to end: DecodeEngine.extend of 512 tokens at position 2048 on the Llama-2-7B shape against 64 verify passes of 8 tokens over
the same positions.
Every step runs under its own time limit (a watchdog ends the process when a step overruns it) and the first failure ends the
run: nothing is tried twice.  One JSON line per point; no threshold."""
import argparse
import dataclasses
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
HD = 128


def st():
    return torch.cuda.current_stream().cuda_stream


class limit:
    """`with limit(seconds):` -- the process exits (with a traceback) if the block is still running after `seconds`."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        return False


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner       # us per call


def medians_us(fns, reps, inner, warm=3):
    """The sides alternate: per side the median over `reps` windows of `inner` back-to-back calls, after `warm` calls each."""
    for _ in range(warm):
        for fn in fns:
            timed(fn, 1)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            t.append(timed(fn, inner))
    return [statistics.median(t) for t in ts]


def kernel_points(reps):
    from qeft_amd import _lib
    lib, ck = _lib.lib(), _lib.check
    sdpa = torch.nn.functional.scaled_dot_product_attention
    g = torch.Generator(device=DEV).manual_seed(0)
    for heads, kv in ((32, 32), (64, 8)):
        rep = heads // kv
        for start, t in ((0, 512), (0, 2048), (2048, 512), (14336, 2048)):
            with limit(240):
                L = start + t
                qkv = torch.randn(t, (heads + 2 * kv) * HD, generator=g, device=DEV).half()
                kc = (torch.randn(kv, L, HD, generator=g, device=DEV) * 0.5).half()
                vc = (torch.randn(kv, L, HD, generator=g, device=DEV) * 0.5).half()
                out = torch.empty(t, heads * HD, dtype=torch.float16, device=DEV)
                q = qkv[:, :heads * HD].view(t, heads, HD)
                k, v = kc.transpose(0, 1), vc.transpose(0, 1)                       # [L, kv, 128], as prefill holds them

                def own():
                    ck(lib.qeft_attn_prefill(qkv.data_ptr(), qkv.stride(0), kc.data_ptr(), vc.data_ptr(), L, out.data_ptr(),
                                             out.stride(0), start, t, heads, kv, st()))
                mask = None
                if start > 0:
                    mask = torch.arange(L, device=DEV)[None, :] <= (start + torch.arange(t, device=DEV))[:, None]
                kk, vv = (k, v) if rep == 1 else (k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1))

                def sdpa_call():
                    return sdpa(q.transpose(0, 1)[None], kk.transpose(0, 1)[None], vv.transpose(0, 1)[None], attn_mask=mask,
                                is_causal=mask is None)[0]

                def sdpa_path():
                    k2, v2 = (k, v) if rep == 1 else (k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1))
                    a = sdpa(q.transpose(0, 1)[None], k2.transpose(0, 1)[None], v2.transpose(0, 1)[None], attn_mask=mask,
                             is_causal=mask is None)[0]
                    return a.transpose(0, 1).reshape(t, heads * HD).contiguous()
                own()
                ref = sdpa_path().float()
                torch.cuda.synchronize()
                err = (out.float() - ref).abs().max().item()
                u_own, u_call, u_path = medians_us((own, sdpa_call, sdpa_path), reps, inner=20 if L <= 4096 else 4)
                flops = 4.0 * heads * HD * (t * start + t * (t + 1) / 2)                # the causal part only
                print(json.dumps(dict(bench="attn_prefill", heads=heads, kv=kv, start=start, t=t, reps=reps,
                                      own_us=round(u_own, 1), sdpa_call_us=round(u_call, 1), sdpa_path_us=round(u_path, 1),
                                      own_over_sdpa_call=round(u_own / u_call, 3), own_over_sdpa_path=round(u_own / u_path, 3),
                                      own_TFLOPs=round(flops / u_own * 1e-6, 1), max_abs_diff_vs_sdpa=round(err, 5),
                                      sdpa="causal" if mask is None else "explicit mask over the concatenated keys")), flush=True)
                del qkv, kc, vc, kk, vv, mask, ref
                torch.cuda.empty_cache()


def e2e_point(reps):
    from qeft_amd.llama import LLAMA2_7B, DecodeEngine, QuantLlama
    pos, t = 2048, 512
    with limit(360):
        model = QuantLlama(dataclasses.replace(LLAMA2_7B, max_seq=4096), DEV, seed=0, fast_init=True)
        eng = DecodeEngine(model, use_graph=True)
        toks = torch.randint(0, model.shape.vocab, (t,), generator=torch.Generator().manual_seed(1))
        dev_toks = toks.to(DEV)

        def extend():
            eng.set_position(pos)
            eng.extend(dev_toks)

        def verify64():
            eng.set_position(pos)
            for i in range(0, t, 8):
                eng.verify(toks[i:i + 8])
        extend()
        verify64()
        torch.cuda.synchronize()
    with limit(300):
        u_ext, u_ver = medians_us((extend, verify64), reps, inner=1, warm=1)
    print(json.dumps(dict(bench="extend_e2e", model="Llama-2-7B shape, synthetic weights", position=pos, tokens=t, reps=reps,
                          extend_ms=round(u_ext * 1e-3, 2), verify_64x8_ms=round(u_ver * 1e-3, 2),
                          extend_over_verify=round(u_ext / u_ver, 3))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    print(json.dumps(dict(bench="prefill_attn", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    kernel_points(a.reps)
    if not a.skip_e2e:
        e2e_point(a.reps)
