"""The fused head's forward + backward (scoring.lm_head_nll_loss: qeft_lm_head_nll, qeft_lm_head_nll_grad)
against the torch head it replaces in training: one GPU, one process, HIP events, a warm-up before every measurement, the sides
of a point alternating (medians of --reps windows).

    python tools/bench_lm_head_grad.py [--reps 10] [--layers 4] [--skip-e2e] > profiles/lm_head_grad_bench.json.log

T = 512 / 2048 rows x hidden 4096 / 8192 x vocab 32000, random operands, the loss the mean NLL, the gradient taken in hn:
  (a) torch.matmul(hn, W.t()) -> fp32 copy -> cross_entropy, forward and backward;
  (c) lm_head_nll_loss(hn, W, targets).mean(), forward and backward; also its backward entry alone (both launches of every chunk).
Per point: the medians, c / a, TFLOP/s of the backward entry on 4 T hidden vocab operations (logits again, then g W), the peak
memory each side adds to the operands (the cached workspaces counted), and the largest difference of the two gradients.
End to end: one finetune.causal_lm_loss forward + backward on the Llama-2-7B shape (synthetic weights, --layers decoder layers,
T = 2048, gradient checkpointing on), head="fused" against head="torch": time and peak memory over the model.
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


def medians_us(fns, reps, inner, warm=2):
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
                hn = torch.randn(t, hidden, generator=g, device=DEV).half().requires_grad_(True)
                targets = torch.randint(0, vocab, (t,), generator=g, device=DEV)
                tg32 = targets.to(torch.int32)

                def torch_head():
                    hn.grad = None
                    torch.nn.functional.cross_entropy(torch.matmul(hn, w.t()).float(), targets).backward()
                    return hn.grad

                def fused():
                    hn.grad = None
                    scoring.lm_head_nll_loss(hn, w, tg32).mean().backward()
                    return hn.grad
                lse = scoring.lm_head_nll(hn.detach(), w, tg32)[0]
                gn = torch.full((t,), 1.0 / t, device=DEV)

                def grad_only():
                    return scoring.lm_head_nll_grad(hn.detach(), w, tg32, lse, gn)
                g_new, g_old = fused().float().clone(), torch_head().float().clone()
                diff = (g_new - g_old).abs().max().item() / g_old.abs().max().item()
                torch.cuda.synchronize()
                mem_old, mem_new = peak_rise(torch_head), peak_rise(fused)        # (the workspaces are already cached: counted below)
                ws = scoring._workspace[torch.device(DEV)].numel() + scoring._grad_workspace[torch.device(DEV)].numel()
                u_old, u_new, u_grad = medians_us((torch_head, fused, grad_only), reps, inner=5)
                flops = 4.0 * t * hidden * vocab
                print(json.dumps(dict(bench="lm_head_grad", t=t, hidden=hidden, vocab=vocab, reps=reps,
                                      torch_fwd_bwd_us=round(u_old, 1), fused_fwd_bwd_us=round(u_new, 1),
                                      fused_over_torch=round(u_new / u_old, 3), grad_entry_us=round(u_grad, 1),
                                      grad_entry_TFLOPs=round(flops / u_grad * 1e-6, 1),
                                      torch_peak_MiB=round(mem_old / 2 ** 20, 1), fused_peak_MiB=round((mem_new + ws) / 2 ** 20, 1),
                                      max_grad_diff_rel=float(f"{diff:.3e}"))), flush=True)
                del hn, targets, tg32, lse, gn, g_new, g_old
                torch.cuda.empty_cache()
        del w


def e2e_point(layers):
    from qeft_amd import finetune, scoring
    from qeft_amd.llama import LLAMA2_7B, QuantLlama
    T = 2048
    with limit(420):
        model = QuantLlama(dataclasses.replace(LLAMA2_7B, max_seq=T, n_layers=layers), DEV, seed=0, fast_init=True)
        toks = torch.randint(0, model.shape.vocab, (T,), generator=torch.Generator().manual_seed(1)).to(DEV)
        params = finetune.begin(model)

        def step(head):
            for p in params:
                p.grad = None
            loss = finetune.causal_lm_loss(model, toks, head=head)
            (loss * 1024.0).backward()
            return loss.item()
        for head in ("fused", "torch"):                                   # warm-up: code objects, workspaces
            step(head)
        torch.cuda.synchronize()
    with limit(300):
        res = {}
        for _ in range(3):                                                # alternate; keep the best of three
            for head in ("fused", "torch"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                v = step(head)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res[head] = (min(dt, res.get(head, (dt, v))[0]), v)
        mem = {}
        for head in ("fused", "torch"):
            for p in params:
                p.grad = None
            scoring._workspace.clear()
            scoring._grad_workspace.clear()
            mem[head] = peak_rise(lambda: step(head))
    print(json.dumps(dict(bench="causal_lm_loss_e2e", model=f"Llama-2-7B shape, {layers} layers, synthetic weights", T=T, checkpoint=True,
                          fused_s=round(res["fused"][0], 4), torch_s=round(res["torch"][0], 4),
                          fused_over_torch=round(res["fused"][0] / res["torch"][0], 3),
                          fused_peak_MiB=round(mem["fused"] / 2 ** 20, 1), torch_peak_MiB=round(mem["torch"] / 2 ** 20, 1),
                          loss_fused=round(res["fused"][1], 6), loss_torch=round(res["torch"][1], 6))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    print(json.dumps(dict(bench="lm_head_grad", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    kernel_points(a.reps)
    if not a.skip_e2e:
        e2e_point(a.layers)
