"""Sampled decoding on Llama-2-7B shapes (one GPU, 4-bit v3 engine): the sampling kernel's time per launch at vocab 32000 for
m = 1 and 8 rows and three parameter sets, on spread logits (N(0, 3^2)) and on flat ones (N(0, 0.05^2): every key in a few
histogram bins), against the argmax token ends (token_end / token_end_b); sampled against greedy DecodeEngine.run() tokens/s at
position 128; sampled against greedy batched passes at m = 8, position 128, alternated over --reps repetitions.  Kernel times are
HIP events over a captured graph of 100 launches.  Prints a table and one JSON line.  QEFT_HIP_LIB=<other build> times another
build of the same ABI (A/B).

    python tools/bench_sample.py [--iters 20] [--reps 5]
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (0.7, 0, 0.9)]


def _graph_us(launch, n=100, iters=20):
    """us per launch: a graph of n launches, replayed `iters` times"""
    launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            launch()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (iters * n)


def kernel_times(iters, scale, tag):
    from qeft_amd import _lib
    from qeft_amd.sampling import SamplingParams
    lib, ck = _lib.lib(), _lib.check
    vocab, dev = 32000, "cuda:0"
    g = torch.Generator().manual_seed(0)
    lg = (torch.randn(8, vocab, generator=g) * scale).half().to(dev)
    st = lambda: torch.cuda.current_stream().cuda_stream           # noqa: E731
    tok = torch.zeros(8, dtype=torch.long, device=dev)
    pos = torch.zeros(8, dtype=torch.int32, device=dev)
    ctr = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.zeros(8, 4, dtype=torch.long, device=dev)
    slots = torch.arange(8, dtype=torch.int32, device=dev)
    limit = torch.full((8,), 2 ** 30, dtype=torch.int32, device=dev)
    eos = torch.full((8,), -1, dtype=torch.int32, device=dev)
    done = torch.zeros(8, dtype=torch.int32, device=dev)
    res = {f"{tag}_token_end_m1": _graph_us(lambda: ck(lib.qeft_token_end(lg.data_ptr(), tok.data_ptr(), pos.data_ptr(), vocab, 1, st())),
                                     iters=iters),
           f"{tag}_token_end_b_m8": _graph_us(lambda: ck(lib.qeft_token_end_batch(
               lg.data_ptr(), slots.data_ptr(), tok.data_ptr(), pos.data_ptr(), limit.data_ptr(), eos.data_ptr(), done.data_ptr(),
               out.data_ptr(), ctr.data_ptr(), vocab, 4, 8, 8, st())), iters=iters)}
    for T, k, p in CONFIGS:
        rec = torch.tensor([SamplingParams(T, k, p, seed=7 + r).record() for r in range(8)], dtype=torch.int32, device=dev)
        name = f"{tag}_T{T}_k{k}_p{p}"
        res[f"token_end_sample_m1_{name}"] = _graph_us(lambda: ck(lib.qeft_token_end_sample(
            lg.data_ptr(), tok.data_ptr(), pos.data_ptr(), vocab, rec.data_ptr(), st())), iters=iters)
        res[f"token_end_sample_b_m8_{name}"] = _graph_us(lambda: ck(lib.qeft_token_end_sample_batch(
            lg.data_ptr(), slots.data_ptr(), tok.data_ptr(), pos.data_ptr(), limit.data_ptr(), eos.data_ptr(), done.data_ptr(),
            out.data_ptr(), ctr.data_ptr(), rec.data_ptr(), vocab, 4, 8, 8, st())), iters=iters)
    return {k: round(v, 2) for k, v in res.items()}


def run_tps(eng, params, n_tok, reps):
    """DecodeEngine.run() tokens/s from position 128 (best of reps)"""
    eng.set_sampling(params)
    eng.greedy = params is None
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 0.0
    for _ in range(reps + 1):
        eng.set_position(128)
        eng.tok.fill_(1)
        torch.cuda.synchronize()
        a.record()
        eng.run(n_tok)
        b.record()
        torch.cuda.synchronize()
        best = max(best, n_tok / (a.elapsed_time(b) / 1e3))
    return round(best, 1)


def batch_pass(eng, sampled):
    """a BatchDecodeEngine of 8 rows at position 128 (rows' records: T = 0.7, top_p = 0.9 when sampled) and one pass of it"""
    from qeft_amd.batch import BatchDecodeEngine
    from qeft_amd.sampling import SamplingParams
    s = eng.m.shape
    be = BatchDecodeEngine(eng, max_batch=8)
    for r in range(8):
        slot = be.admit([1], s.max_seq, sampling=SamplingParams(0.7, 0, 0.9, seed=r) if sampled else None)
        q = be.table.get(slot)
        q.pos = q.limit = s.max_seq
    pos0 = torch.full((8,), 128, dtype=torch.int32, device=eng.dev)
    be.limit.fill_(s.max_seq)
    rows = be.table.rows()
    be.slot_tab[:8].copy_(torch.tensor(rows, dtype=torch.int32))
    be.rows = rows
    sp = be._split_for(128)

    def one():
        be.state[0].copy_(pos0)
        be._pass(8, sp, 1, sampled)
    for _ in range(5):
        one()
    torch.cuda.synchronize()
    return be, one


def time_us(one, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        one()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from qeft_amd.llama import LLAMA2_7B, DecodeEngine, QuantLlama
    from qeft_amd.sampling import SamplingParams
    rec = {"model": "llama-2-7b shapes (w4 g128 r128), max_seq 512", "lib": os.environ.get("QEFT_HIP_LIB", "in-tree"),
           "kernel_us": {**kernel_times(args.iters, 3.0, "spread"), **kernel_times(args.iters, 0.05, "flat")}}
    model = QuantLlama(dataclasses.replace(LLAMA2_7B, max_seq=512), "cuda:0", seed=0, fast_init=True)
    eng = DecodeEngine(model, use_graph=True)
    sp = SamplingParams(0.7, 50, 0.9, seed=1)
    for params in (None, sp):                  # warm-up: capture every graph the timed runs use
        run_tps(eng, params, args.tokens, 0)
    greedy, sampled = [], []
    for _ in range(3):                         # interleaved
        greedy.append(run_tps(eng, None, args.tokens, 1))
        sampled.append(run_tps(eng, sp, args.tokens, 1))
    rec["run_tokens_per_s_pos128"] = {"greedy": max(greedy), "sampled_T0.7_k50_p0.9": max(sampled),
                                      "ratio": round(max(sampled) / max(greedy), 4)}
    eng.set_sampling(None)
    (bg, g_one), (bs, s_one) = batch_pass(eng, False), batch_pass(eng, True)
    g_us, s_us = [], []
    for _ in range(args.reps):                 # alternated
        g_us.append(time_us(g_one, args.iters))
        s_us.append(time_us(s_one, args.iters))
    med = lambda v: sorted(v)[len(v) // 2]     # noqa: E731
    rec["batch_m8_pos128_us_per_pass"] = {
        "greedy_median": round(med(g_us), 1), "greedy_min_max": [round(min(g_us), 1), round(max(g_us), 1)],
        "sampled_T0.7_p0.9_median": round(med(s_us), 1), "sampled_min_max": [round(min(s_us), 1), round(max(s_us), 1)],
        "ratio_tokens_per_s_median": round(med(g_us) / med(s_us), 4)}
    for k, v in rec["kernel_us"].items():
        print(f"{k:44s} {v:8.2f} us")
    print("run() tokens/s at 128:", rec["run_tokens_per_s_pos128"])
    print("batched pass m = 8 at 128:", rec["batch_m8_pos128_us_per_pass"])
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
