"""Batched decoding on Llama-2-7B shapes (one GPU, 4-bit v3 engine, max_seq 2304): the time of a graph-replayed batched pass of
B = 1, 2, 4, 8 rows with every row at position 128, 1024 and 2048, and of B = 8 rows spread over 64 .. 2048; aggregate tokens/s
(B tokens per pass) and its ratio to the same run's single-sequence DecodeEngine.run() tokens/s at the same position.  The
rows' caches hold zeros (the time does not depend on their values).  Prints a table and one JSON line.

    python tools/bench_batch.py [--iters 50]
    python tools/bench_batch.py --profile 8 --pos 2048      # replay only B = 8 passes at one position (rocprofv3)
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIXED = [64, 300, 600, 900, 1200, 1500, 1800, 2048]


def _time(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3     # us


def _batch_at(eng, positions):
    """A BatchDecodeEngine with len(positions) rows at the given positions (admitted with one-token prompts, then placed)."""
    from qeft_amd.batch import BatchDecodeEngine
    s = eng.m.shape
    be = BatchDecodeEngine(eng, max_batch=len(positions))
    for p in positions:
        slot = be.admit([1], s.max_seq)
        q = be.table.get(slot)
        q.pos = q.limit = s.max_seq               # host bound: the split follows the pass's own positions below
    pos0 = torch.tensor(positions, dtype=torch.int32, device=eng.dev)
    be.state[0].copy_(pos0)
    be.limit.fill_(s.max_seq)
    rows = be.table.rows()
    m = len(rows)
    be.slot_tab[:m].copy_(torch.tensor(rows, dtype=torch.int32))
    be.rows = rows
    sp = be._split_for(max(positions))

    def one():
        be.state[0].copy_(pos0)                   # every pass at the same positions
        be._pass(m, sp, 1)
    return be, one, sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--tokens", type=int, default=64, help="tokens of the single-sequence run() reference")
    ap.add_argument("--profile", type=int, default=0, help="replay only passes of this batch size (profiling)")
    ap.add_argument("--pos", type=int, default=2048)
    args = ap.parse_args()
    from qeft_amd.llama import LLAMA2_7B, DecodeEngine, QuantLlama
    shape = dataclasses.replace(LLAMA2_7B, max_seq=2304)
    model = QuantLlama(shape, "cuda:0", seed=0, fast_init=True)
    eng = DecodeEngine(model, use_graph=True)
    if args.profile:
        be, one, sp = _batch_at(eng, [args.pos] * args.profile)
        for _ in range(10):
            one()
        torch.cuda.synchronize()
        print(json.dumps({"profiled_b": args.profile, "pos": args.pos, "split": sp}))
        return
    rec = {"model": "llama-2-7b shapes (w4 g128 r128), max_seq 2304", "single": {}, "batch": {}}
    eng.greedy = True
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for p in (128, 1024, 2048):
        eng.set_position(p)
        eng.tok.fill_(1)
        eng.precapture(p + args.tokens + 8)
        eng.run(8)
        eng.set_position(p)
        torch.cuda.synchronize()
        a.record()
        eng.run(args.tokens)
        b.record()
        torch.cuda.synchronize()
        rec["single"][p] = round(args.tokens / (a.elapsed_time(b) / 1e3), 1)
    cases = [(B, [p] * B, p) for p in (128, 1024, 2048) for B in (1, 2, 4, 8)] + [(8, MIXED, "mixed")]
    lines = []
    for B, positions, key in cases:
        be, one, sp = _batch_at(eng, positions)
        us = _time(one, args.iters)
        tps = B * 1e6 / us
        single = rec["single"][key if key != "mixed" else 1024]
        rec["batch"][f"B{B}_p{key}"] = {"us_per_pass": round(us, 1), "tokens_per_s": round(tps, 1), "split": sp,
                                        "over_single_run": round(tps / single, 2)}
        lines.append(f"B={B} pos={key!s:>5} split={sp}: {us:8.1f} us/pass  {tps:8.1f} tokens/s  {tps / single:5.2f}x single run()")
        del be
        torch.cuda.empty_cache()
    print("single-sequence run() tokens/s:", rec["single"], "(the mixed case is compared with position 1024)")
    print("\n".join(lines))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
