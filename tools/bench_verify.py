"""Verify pass on Llama-2-7B shapes (one GPU, 4-bit v3 engine): the time of a graph-replayed verify pass of m = 1..8 tokens
against one step(), and greedy assisted decoding tokens/s with an ORACLE draft (the target's own greedy continuation: every
draft accepted, the upper bound; k = 4 and 7 drafts = 5- and 8-row passes) and with a draft that is wrong every j-th token.  Prints one JSON line.

    python tools/bench_verify.py [--pos 128] [--iters 50] [--tokens 256] [--kv-dtype fp16|fp8] [--max-seq 1024] [--start 0]

--kv-dtype fp8 runs the engine on an e4m3 KV cache with kv8_verify=True; --start is the position the greedy and
assisted runs begin at (the cache below it holds zeros, which cost what any content costs: the run is for timing, its tokens mean nothing), --max-seq the cache length.
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


class _Scripted:
    """A draft that proposes the given continuation, with every j-th proposed token made wrong (j = 0: never)."""

    def __init__(self, ref, vocab, wrong_every=0, start=0):
        self.ref, self.vocab, self.j, self.count, self.start = ref, vocab, wrong_every, 0, start

    def propose(self, ctx, k):
        i = len(ctx) - 1 - self.start        # ref[i] is the token after ctx[-1]
        out = []
        for t in self.ref[i:i + k]:
            self.count += 1
            out.append((t + 1) % self.vocab if self.j and self.count % self.j == 0 else t)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pos", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--only-m", type=int, default=0, help="replay only the verify pass of this m (profiling)")
    ap.add_argument("--kv-dtype", default="fp16", choices=["fp16", "fp8"])
    ap.add_argument("--max-seq", type=int, default=1024)
    ap.add_argument("--start", type=int, default=0, help="position the greedy and assisted runs begin at")
    args = ap.parse_args()
    from qeft_amd.assisted import assisted_generate
    from qeft_amd.llama import LLAMA2_7B, DecodeEngine, QuantLlama
    shape = dataclasses.replace(LLAMA2_7B, max_seq=args.max_seq)
    model = QuantLlama(shape, "cuda:0", seed=0, fast_init=True)
    eng = DecodeEngine(model, use_graph=True, kv_dtype=args.kv_dtype, kv8_verify=args.kv_dtype == "fp8")
    rec = {"model": "llama-2-7b shapes (w4 g128 r128)", "pos": args.pos, "kv_dtype": args.kv_dtype, "start": args.start}
    context = [0] * args.start
    eng.greedy = False
    if args.only_m:
        for _ in range(3):
            eng.set_position(args.pos)
            eng.verify(list(range(1, args.only_m + 1)))
        torch.cuda.synchronize()
        print(json.dumps({"profiled_m": args.only_m}))
        return

    def step():
        eng.set_position(args.pos)
        eng.step()
    rec["step_us"] = round(_time(step, args.iters), 1)
    rec["verify_us"] = {}
    for m in range(1, 9):
        toks = list(range(1, m + 1))

        def ver():
            eng.set_position(args.pos)
            eng.verify(toks)
        rec["verify_us"][m] = round(_time(ver, args.iters), 1)
    rec["verify_over_step"] = {m: round(v / rec["step_us"], 3) for m, v in rec["verify_us"].items()}
    # assisted decoding from position 0.  The oracle draft proposes the sequence the TARGET produces under assisted decoding
    # with every draft accepted: a fixed point, found by feeding each run's output back as the next run's draft (a random-weight
    # model has many near-ties, where the m-row and one-row roundings may pick different tokens; a fixed one-row greedy
    # sequence would stop being the target's continuation at the first of them).  The same for drafts wrong every j-th token:
    # the right tokens are those the target produces under that draft.
    eng.greedy = True
    n = args.tokens
    eng.set_position(args.start)
    eng.tok.fill_(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.run(8)
    eng.set_position(args.start)
    eng.tok.fill_(1)
    torch.cuda.synchronize()
    a.record()
    eng.run(n)
    b.record()
    torch.cuda.synchronize()
    rec["greedy_run_tokens_per_s"] = round(n / (a.elapsed_time(b) / 1e3), 1)
    rec["assisted"] = {}
    for k in (4, 7):
        for j in (0, 4, 2):
            ref = [0] * (n + 8)
            for _ in range(12):                              # fixed point: the draft's "right" tokens are the target's own
                eng.set_position(args.start)
                out, acc = assisted_generate(eng, _Scripted(ref, shape.vocab, j, args.start), 1, n, k, context=context)
                if out == ref[:n]:
                    break
                ref = out + [0] * 8
            eng.set_position(args.start)
            torch.cuda.synchronize()
            a.record()
            out, acc = assisted_generate(eng, _Scripted(ref, shape.vocab, j, args.start), 1, n, k, context=context)
            b.record()
            torch.cuda.synchronize()
            t = a.elapsed_time(b) / 1e3
            rec["assisted"][f"k{k}_" + ("oracle" if j == 0 else f"wrong_every_{j}")] = {
                "tokens_per_s": round(n / t, 1), "passes": len(acc), "mean_accepted": round(sum(acc) / len(acc), 2),
                "fixed_point": out == ref[:n]}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
