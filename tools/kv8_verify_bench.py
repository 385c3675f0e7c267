"""The m-row verify attention over an e4m3 KV cache against the fp16 m-row launch: one GPU, one process, the
two launches alternating.

    python tools/kv8_verify_bench.py [--reps 20] > profiles/kv8_verify_bench.json.log

One launch of qeft_rope_attn_decode_m_kv8 against one of qeft_rope_attn_decode_m at contexts 1024, 4096, 16384, 32768 (the m rows
are the context's last), m = 1, 4, 8, head layouts (32, 32) and (64, 8), splits 1, 2, 4, 8: per point the median of --reps
alternating pairs after a warm-up, each launch timed by events around 4 back-to-back launches.  Between two launches of one side
the other side's cache streams through, and the caches of a point are 2 x n_kv x context rows per side; achieved bytes/s count
the K and V rows (and scales) of the context once per kv head.  ratio = fp8 / fp16; the byte ratio is 132 / 256 = 0.516.
One JSON line per point."""
import argparse
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


def timed(fn, inner=4):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner       # us per launch


def points(reps, layouts):
    from qeft_amd import _lib
    lib, ck = _lib.lib(), _lib.check
    g = torch.Generator(device=DEV).manual_seed(0)
    for heads, kv in layouts:
        for ctx in (1024, 4096, 16384, 32768):
            max_seq = ctx
            kc16 = (torch.randn(kv, max_seq, HD, generator=g, device=DEV) * 0.5).half()
            vc16 = (torch.randn(kv, max_seq, HD, generator=g, device=DEV) * 0.5).half()
            kc8 = torch.randint(0, 0x78, (kv, max_seq, HD), generator=g, device=DEV, dtype=torch.uint8)
            vc8 = torch.randint(0, 0x78, (kv, max_seq, HD), generator=g, device=DEV, dtype=torch.uint8)
            ks = torch.rand(kv, max_seq, generator=g, device=DEV) * 0.01
            vs = torch.rand(kv, max_seq, generator=g, device=DEV) * 0.01
            ang = torch.randn(max_seq, 64, generator=g, device=DEV)
            cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
            nq = (heads + 2 * kv) * HD
            qkv = torch.randn(8, nq, generator=g, device=DEV).half()
            out = torch.zeros(8, heads * HD, dtype=torch.float16, device=DEV)
            ws16 = torch.zeros(lib.qeft_attn_m_workspace_bytes(heads, 8, 8) // 4, device=DEV)
            ws8 = torch.zeros(lib.qeft_attn_m_kv8_workspace_bytes(heads, 8, 8) // 4, device=DEV)
            qp = qkv.data_ptr()
            q3 = (qp, qp + heads * HD * 2, qp + (heads + kv) * HD * 2, nq, cos.data_ptr(), sin.data_ptr(), 64, max_seq)
            for m in (1, 4, 8):
                pos = torch.full((1,), ctx - m, dtype=torch.int32, device=DEV)
                for split in (1, 2, 4, 8):
                    def f16():
                        ck(lib.qeft_rope_attn_decode_m(*q3, kc16.data_ptr(), vc16.data_ptr(), pos.data_ptr(), None, out.data_ptr(),
                                                       heads * HD, ws16.data_ptr(), split, heads, kv, max_seq, m, st()))

                    def f8():
                        ck(lib.qeft_rope_attn_decode_m_kv8(*q3, kc8.data_ptr(), vc8.data_ptr(), ks.data_ptr(), vs.data_ptr(),
                                                           pos.data_ptr(), None, out.data_ptr(), heads * HD, ws8.data_ptr(), split,
                                                           heads, kv, max_seq, m, st()))
                    for fn in (f16, f8, f16, f8):
                        timed(fn)
                    t16, t8 = [], []
                    for _ in range(reps):
                        t16.append(timed(f16))
                        t8.append(timed(f8))
                    u16, u8 = statistics.median(t16), statistics.median(t8)
                    b16, b8 = kv * ctx * 2 * HD * 2, kv * ctx * 2 * (HD + 4)
                    print(json.dumps(dict(bench="attn_m", heads=heads, kv=kv, context=ctx, m=m, split=split, reps=reps,
                                          fp16_us=round(u16, 2), fp8_us=round(u8, 2), ratio=round(u8 / u16, 3),
                                          fp16_min_us=round(min(t16), 2), fp8_min_us=round(min(t8), 2),
                                          fp16_GBps=round(b16 / u16 * 1e-3, 1), fp8_GBps=round(b8 / u8 * 1e-3, 1))), flush=True)
            del kc16, vc16, kc8, vc8, ks, vs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layouts", default="32/32,64/8")
    a = ap.parse_args()
    print(json.dumps(dict(bench="kv8_verify", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    points(a.reps, [tuple(int(x) for x in lay.split("/")) for lay in a.layouts.split(",")])
