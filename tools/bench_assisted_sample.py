"""Sampled assisted decoding on Llama-2-7B shapes (one GPU, 4-bit v3 engine).  One run measures
  (1) the graph-replayed sampled verify pass (verify_sample) of m = 1..8 tokens next to the greedy verify pass of the same run,
      and qeft_sample alone on m = 8 rows (the yardstick for the excess);
  (2) sampled assisted tokens/s with a replay draft (the target's own sampled continuation: every draft accepted) at 4 and 7
      drafts, next to sampled run();
  (3) the acceptance per pass of a coupled EngineDraft: a second engine on the same model, the same with a seed of its own (the
      control), and a 3-bit engine quantised from the same dense weights, coupled and with its own seed.
Prints one JSON line.

    python tools/bench_assisted_sample.py [--pos 128] [--iters 50] [--tokens 256]
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


class _Replay:
    """Proposes the recorded continuation ref (ref[i]: the token after a context of i + 1 tokens)."""

    def __init__(self, ref):
        self.ref = ref

    def propose(self, ctx, k):
        return self.ref[len(ctx) - 1:len(ctx) - 1 + k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pos", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--only-m", type=int, default=0, help="replay only the sampled verify pass of this m (profiling)")
    args = ap.parse_args()
    from qeft_amd import _lib
    from qeft_amd.assisted import EngineDraft, assisted_generate
    from qeft_amd.llama import LLAMA2_7B, DecodeEngine, QuantLlama
    from qeft_amd.sampling import SamplingParams
    dev = "cuda:0"
    shape = dataclasses.replace(LLAMA2_7B, max_seq=1024)
    model = QuantLlama(shape, dev, seed=0, fast_init=True)
    eng = DecodeEngine(model, use_graph=True)
    sp = SamplingParams(0.8, 40, 0.95, seed=20261016)
    rec = {"model": "llama-2-7b shapes (w4 g128 r128)", "pos": args.pos,
           "sampling": {"temperature": sp.temperature, "top_k": sp.top_k, "top_p": sp.top_p}}
    eng.set_sampling(sp)
    if args.only_m:
        for _ in range(3):
            eng.set_position(args.pos)
            eng.verify_sample(list(range(1, args.only_m + 1)))
        torch.cuda.synchronize()
        print(json.dumps({"profiled_m": args.only_m}))
        return

    # (1) the verify pass, sampled and greedy, interleaved per m
    eng.greedy = True
    rec["verify_sample_us"], rec["verify_greedy_us"] = {}, {}
    for m in range(1, 9):
        toks = list(range(1, m + 1))

        def ver_s():
            eng.set_position(args.pos)
            eng.verify_sample(toks)

        def ver_g():
            eng.set_position(args.pos)
            eng.verify(toks)
        rec["verify_greedy_us"][m] = round(_time(ver_g, args.iters), 1)
        rec["verify_sample_us"][m] = round(_time(ver_s, args.iters), 1)
    rec["sample_over_greedy"] = {m: round(rec["verify_sample_us"][m] / rec["verify_greedy_us"][m], 4) for m in range(1, 9)}
    rec["excess_us"] = {m: round(rec["verify_sample_us"][m] - rec["verify_greedy_us"][m], 1) for m in range(1, 9)}
    # qeft_sample alone on the last pass's 8 logits rows (a graph of 20 launches)
    lib, ck = _lib.lib(), _lib.check
    recs = torch.tensor([sp.record()] * 8, dtype=torch.int32, device=dev)
    pos8 = torch.arange(args.pos + 1, args.pos + 9, dtype=torch.int32, device=dev)
    out8 = torch.zeros(8, dtype=torch.long, device=dev)
    for m in (1, 8):
        def launch():
            ck(lib.qeft_sample(eng.logits_m.data_ptr(), shape.vocab, m, recs.data_ptr(), pos8.data_ptr(), out8.data_ptr(),
                               torch.cuda.current_stream().cuda_stream))
        launch()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                launch()
        rec[f"qeft_sample_m{m}_us"] = round(_time(g.replay, args.iters) / 20, 1)

    # (2) sampled run() and sampled assisted decoding with a replay draft (a fixed point, as tools/bench_verify.py's oracle)
    n = args.tokens
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.set_sampling(sp)
    eng.reset()
    eng.tok.fill_(1)
    eng.run(8)
    eng.reset()
    eng.tok.fill_(1)
    torch.cuda.synchronize()
    a.record()
    eng.run(n)
    b.record()
    torch.cuda.synchronize()
    rec["sampled_run_tokens_per_s"] = round(n / (a.elapsed_time(b) / 1e3), 1)
    eng.set_sampling(None)
    rec["assisted_replay"] = {}
    for k in (4, 7):
        ref = [0] * (n + 8)
        for _ in range(64):              # (each run fixes the stream up to its next rounding-sensitive position)
            eng.reset()
            out, acc = assisted_generate(eng, _Replay(ref), 1, n, k, sampling=sp)
            if out == ref[:n]:
                break
            ref = out + [0] * 8
        eng.reset()
        torch.cuda.synchronize()
        a.record()
        out, acc = assisted_generate(eng, _Replay(ref), 1, n, k, sampling=sp)
        b.record()
        torch.cuda.synchronize()
        tps = n / (a.elapsed_time(b) / 1e3)
        rec["assisted_replay"][f"k{k}"] = {"tokens_per_s": round(tps, 1), "over_sampled_run": round(tps / rec["sampled_run_tokens_per_s"], 2),
                                           "passes": len(acc), "mean_accepted": round(sum(acc) / len(acc), 2),
                                           "fixed_point": out == ref[:n]}

    # (3) acceptance of engine drafts, k = 4 and 7 drafts per pass
    class OwnSeed(EngineDraft):
        def set_sampling(self, params):
            super().set_sampling(dataclasses.replace(params, seed=params.seed ^ 0x5555_5555) if params is not None else None)
    rec["engine_draft_acceptance"] = {}

    def acceptance(name, make):
        for k in (4, 7):
            eng.reset()
            out, acc = assisted_generate(eng, make(), 1, n, k, sampling=sp)
            offered = sum(min(k, n - 1 - (sum(acc[:i]) + i)) for i in range(len(acc)))
            rec["engine_draft_acceptance"][f"{name}_k{k}"] = {"accepted_over_offered": round(sum(acc) / max(offered, 1), 4),
                                                              "mean_accepted_per_pass": round(sum(acc) / len(acc), 3),
                                                              "passes": len(acc)}
    same = DecodeEngine(model, use_graph=True)
    acceptance("same_model_coupled", lambda: EngineDraft(same))
    acceptance("same_model_own_seed", lambda: OwnSeed(same))
    del same
    try:
        model3 = QuantLlama(dataclasses.replace(shape, bits=3), dev, seed=0, fast_init=True)     # the same dense weights, 3 bits
        w3 = DecodeEngine(model3, use_graph=True)
        acceptance("w3_same_dense_weights_coupled", lambda: EngineDraft(w3))
        acceptance("w3_same_dense_weights_own_seed", lambda: OwnSeed(w3))
    except Exception as e:          # noqa: BLE001 -- the record says why the 3-bit draft is missing
        rec["engine_draft_acceptance"]["w3_error"] = f"{type(e).__name__}: {e}"[:300]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
