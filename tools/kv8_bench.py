"""e4m3 against fp16 KV cache: one GPU, one process, the two sides interleaved.

    python tools/kv8_bench.py [--reps 30] [--no-attn] [--no-e2e] > profiles/kv8_bench.json.log

attn   one launch of qeft_rope_attn_decode_kv8 against one of qeft_rope_attn_decode_batch (the fp16 kernel) at contexts 1024,
       4096, 16384, 32768, m = 1 and 8, head layouts (32, 32) and (64, 8), splits 1, 2, 4, 8: per point the median of --reps
       alternating pairs after a warm-up, each launch timed by events around 4 back-to-back launches on caches far larger than
       the caches of the chip (every slot its own cache; 8 rows x 2 arrays x n_kv x context rows); achieved bytes/s count the K
       and V rows (and scales) of the context once per kv head.
e2e    BatchDecodeEngine on the synthetic Llama-2-7B at 8 rows, fp8 and fp16 caches, contexts about 4096 and 16384: tokens/s
       over 64 passes, best of 3, the two engines alternating.
One JSON line per point."""
import argparse
import dataclasses
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


def attn_points(reps):
    from qeft_amd import _lib
    lib, ck = _lib.lib(), _lib.check
    g = torch.Generator(device=DEV).manual_seed(0)
    for heads, kv in ((32, 32), (64, 8)):
        for ctx in (1024, 4096, 16384, 32768):
            max_seq, n_slots = ctx, 8
            kc16 = (torch.randn(n_slots, kv, max_seq, HD, generator=g, device=DEV) * 0.5).half()
            vc16 = (torch.randn(n_slots, kv, max_seq, HD, generator=g, device=DEV) * 0.5).half()
            kc8 = torch.randint(0, 0x78, (n_slots, kv, max_seq, HD), generator=g, device=DEV, dtype=torch.uint8)
            vc8 = torch.randint(0, 0x78, (n_slots, kv, max_seq, HD), generator=g, device=DEV, dtype=torch.uint8)
            ks = torch.rand(n_slots, kv, max_seq, generator=g, device=DEV) * 0.01
            vs = torch.rand(n_slots, kv, max_seq, generator=g, device=DEV) * 0.01
            ang = torch.randn(max_seq, 64, generator=g, device=DEV)
            cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
            nq = (heads + 2 * kv) * HD
            qkv = torch.randn(8, nq, generator=g, device=DEV).half()
            out = torch.zeros(8, heads * HD, dtype=torch.float16, device=DEV)
            ws16 = torch.zeros(lib.qeft_attn_batch_workspace_bytes(heads, 8, 8) // 4, device=DEV)
            ws8 = torch.zeros(lib.qeft_attn_kv8_workspace_bytes(heads, 8, 8) // 4, device=DEV)
            slots = torch.arange(8, dtype=torch.int32, device=DEV)
            pos = torch.full((8,), ctx - 1, dtype=torch.int32, device=DEV)
            qp = qkv.data_ptr()
            q3 = (qp, qp + heads * HD * 2, qp + (heads + kv) * HD * 2, nq, cos.data_ptr(), sin.data_ptr(), 64, max_seq)
            for m in (1, 8):
                for split in (1, 2, 4, 8):
                    def f16():
                        ck(lib.qeft_rope_attn_decode_batch(*q3, kc16.data_ptr(), vc16.data_ptr(), slots.data_ptr(), pos.data_ptr(),
                                                           None, None, out.data_ptr(), heads * HD, ws16.data_ptr(), split, n_slots,
                                                           heads, kv, max_seq, m, st()))

                    def f8():
                        ck(lib.qeft_rope_attn_decode_kv8(*q3, kc8.data_ptr(), vc8.data_ptr(), ks.data_ptr(), vs.data_ptr(),
                                                         slots.data_ptr(), pos.data_ptr(), None, None, out.data_ptr(), heads * HD,
                                                         ws8.data_ptr(), split, n_slots, heads, kv, max_seq, m, st()))

                    def timed(fn, inner=4):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(inner):
                            fn()
                        b.record()
                        b.synchronize()
                        return a.elapsed_time(b) * 1e3 / inner       # us per launch
                    for fn in (f16, f8, f16, f8):
                        timed(fn)
                    t16, t8 = [], []
                    for _ in range(reps):
                        t16.append(timed(f16))
                        t8.append(timed(f8))
                    u16, u8 = statistics.median(t16), statistics.median(t8)
                    b16, b8 = m * kv * ctx * 2 * HD * 2, m * kv * ctx * 2 * (HD + 4)
                    print(json.dumps(dict(bench="attn", heads=heads, kv=kv, context=ctx, m=m, split=split, reps=reps,
                                          fp16_us=round(u16, 2), fp8_us=round(u8, 2), ratio=round(u8 / u16, 3),
                                          fp16_min_us=round(min(t16), 2), fp8_min_us=round(min(t8), 2),
                                          fp16_GBps=round(b16 / u16 * 1e-3, 1), fp8_GBps=round(b8 / u8 * 1e-3, 1))), flush=True)
            del kc16, vc16, kc8, vc8, ks, vs
            torch.cuda.empty_cache()


def e2e_points():
    from qeft_amd.batch import BatchDecodeEngine
    from qeft_amd.llama import LLAMA2_7B, DecodeEngine, QuantLlama
    n_pass, rows = 64, 8
    for ctx in (4096, 16384):
        shape = dataclasses.replace(LLAMA2_7B, max_seq=ctx + 256, name=f"llama2-7b-synthetic-ctx{ctx}")
        model = QuantLlama(shape, DEV, seed=0, fast_init=True)
        engines = {}
        for kvd in ("fp16", "fp8"):
            be = BatchDecodeEngine(DecodeEngine(model, use_graph=True, kv_dtype=kvd), max_batch=rows)
            for r in range(rows):
                be.admit(torch.arange(4) + r, shape.max_seq)
            engines[kvd] = be

        def place(be, p):       # every row at position p: the caches hold zeros there, which cost what any content costs
            be.state[0].fill_(p)
            be.state[3].zero_()
            for s in range(rows):
                q = be.table.get(s)
                q.pos, q.reason = p, None
        best = {}
        for rnd in range(4):    # round 0 captures the graphs
            for kvd, be in engines.items():
                place(be, ctx - n_pass)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                be.run(n_pass)
                b.record()
                b.synchronize()
                if rnd:
                    best[kvd] = min(best.get(kvd, 1e30), a.elapsed_time(b) * 1e-3)
        kv_bytes = {k: sum(t.numel() * t.element_size() for grp in (be.kc, be.vc, be.ks or [], be.vs or []) for t in grp)
                    for k, be in engines.items()}
        print(json.dumps(dict(bench="e2e", model=shape.name, rows=rows, context=ctx, passes=n_pass,
                              fp16_tok_s=round(rows * n_pass / best["fp16"], 1), fp8_tok_s=round(rows * n_pass / best["fp8"], 1),
                              speedup=round(best["fp16"] / best["fp8"], 3), fp16_cache_GB=round(kv_bytes["fp16"] / 1e9, 2),
                              fp8_cache_GB=round(kv_bytes["fp8"] / 1e9, 2))), flush=True)
        del engines, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-attn", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    print(json.dumps(dict(bench="kv8", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    if not a.no_attn:
        attn_points(a.reps)
    if not a.no_e2e:
        e2e_points()
