"""The fused lm_head + cross-entropy entry (qeft_lm_head_nll) against the head stage it replaces: one GPU, one
process, HIP events, a warm-up before every measurement, the sides of a point alternating (medians of --reps windows).

    python tools/bench_lm_head_nll.py [--reps 20] [--skip-e2e] > profiles/lm_head_nll_bench.json.log

T = 512 / 2048 rows x hidden 4096 / 8192 x vocab 32000, random operands:
  (a) the old head stage: torch.matmul(hn, W.t()) -> fp16 logits, then nll_from_logits's cross-entropy on their fp32 copy;
  (b) that matmul alone (hipBLASLt);
  (c) the fused entry, both of its launches, through scoring.lm_head_nll (output allocations included, workspace cached).
Per point: the three medians, TFLOP/s of (b) and (c) on 2 T hidden vocab operations, the peak memory each side adds to the operands.
End to end: eval_nll over 8 windows of 2048 on the Llama-2-7B shape (synthetic weights), the old route (prefill + nll_from_logits per
window, the reference's formula) against scoring.eval_nll.
Every step runs under its own time limit (a watchdog ends the process when a step overruns it) and the first failure ends the
run: nothing is tried twice.  One JSON line per point; no threshold."""
import argparse
import dataclasses
import faulthandler
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


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


def peak_rise(fn):
    """Bytes by which one call of fn lifts the allocator's peak over what is allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise


def kernel_points(reps):
    from qeft_amd import scoring
    vocab = 32000
    g = torch.Generator(device=DEV).manual_seed(0)
    for hidden in (4096, 8192):
        w = (torch.randn(vocab, hidden, generator=g, device=DEV) * 0.02).half()
        for t in (512, 2048):
            with limit(240):
                hn = torch.randn(t, hidden, generator=g, device=DEV).half()
                targets = torch.randint(0, vocab, (t,), generator=g, device=DEV)
                tg32 = targets.to(torch.int32)

                def old():
                    logits = torch.matmul(hn, w.t())
                    return torch.nn.functional.cross_entropy(logits.float(), targets)

                def mm():
                    return torch.matmul(hn, w.t())

                def fused():
                    return scoring.lm_head_nll(hn, w, tg32)
                lse, tl, _ = fused()
                nll_new = -(tl - lse).double().mean().item()
                nll_old = old().item()
                torch.cuda.synchronize()
                mem_old, mem_new = peak_rise(old), peak_rise(fused)      # (the workspace is already cached: counted below)
                ws = scoring._workspace[torch.device(DEV)].numel()
                u_old, u_mm, u_new = medians_us((old, mm, fused), reps, inner=10)
                flops = 2.0 * t * hidden * vocab
                print(json.dumps(dict(bench="lm_head_nll", t=t, hidden=hidden, vocab=vocab, reps=reps,
                                      old_head_us=round(u_old, 1), matmul_us=round(u_mm, 1), fused_us=round(u_new, 1),
                                      fused_over_old=round(u_new / u_old, 3), fused_over_matmul=round(u_new / u_mm, 3),
                                      matmul_TFLOPs=round(flops / u_mm * 1e-6, 1), fused_TFLOPs=round(flops / u_new * 1e-6, 1),
                                      old_peak_MB=round(mem_old / 2 ** 20, 1), fused_peak_MB=round((mem_new + ws) / 2 ** 20, 1),
                                      nll_old=round(nll_old, 6), nll_fused=round(nll_new, 6))), flush=True)
                del hn, targets, tg32
                torch.cuda.empty_cache()
        del w


def e2e_point():
    from qeft_amd import scoring
    from qeft_amd.llama import LLAMA2_7B, QuantLlama, nll_from_logits, prefill
    seqlen, n = 2048, 8
    with limit(420):
        model = QuantLlama(dataclasses.replace(LLAMA2_7B, max_seq=seqlen), DEV, seed=0, fast_init=True)
        toks = torch.randint(0, model.shape.vocab, (n * seqlen,), generator=torch.Generator().manual_seed(1)).to(DEV)

        def old_route():
            total = 0.0
            for i in range(n):
                win = toks[i * seqlen:(i + 1) * seqlen]
                total += nll_from_logits(prefill(model, win), win) * seqlen
            return total / (n * seqlen)

        def new_route():
            return scoring.eval_nll(model, toks, seqlen=seqlen)["nll"]
        old_route(), new_route()                                          # warm-up: operands, code objects, the workspace
        torch.cuda.synchronize()
    with limit(300):
        res = {}
        for _ in range(2):                                                # alternate; keep the better of two
            for name, fn in (("old", old_route), ("new", new_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                v = fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res[name] = (min(dt, res.get(name, (dt, v))[0]), v)
    print(json.dumps(dict(bench="eval_nll_e2e", model="Llama-2-7B shape, synthetic weights", windows=n, seqlen=seqlen,
                          old_route_s=round(res["old"][0], 3), eval_nll_s=round(res["new"][0], 3),
                          new_over_old=round(res["new"][0] / res["old"][0], 3), nll_old=round(res["old"][1], 6),
                          nll_new=round(res["new"][1], 6))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    print(json.dumps(dict(bench="lm_head_nll", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    kernel_points(a.reps)
    if not a.skip_e2e:
        e2e_point()
