"""The training glue (qeft_amd.glue: add_rmsnorm, swiglu, rope_qk over csrc/train_glue.hip) against the torch
expressions finetune.causal_lm_loss runs by default: one GPU, one process, HIP events, a warm-up before every measurement, the
two sides of a point alternating (medians of --reps windows of 5 calls).

    python tools/bench_train_glue.py [--reps 10] [--step] > profiles/train_glue_bench.json.log

Per op, forward + backward under autograd at T = 2048 rows on the 7B widths (hidden 4096, MLP 11008) and the 70B widths (8192,
28672):
  add_rmsnorm   (s, y) = add_rmsnorm(h, add, gamma) with gradients arriving for both s and y, against s = h + add,
                y = finetune._rmsnorm(s) -- the residual add and the sum of the two gradients are part of both sides;
  swiglu        against (silu(gate.float()) * up.float()).half();
  rope_qk       (q_rot, k_rot) = rope_qk(q, k, cos, sin) at 32 / 32 and 64 / 8 heads, against finetune._rope on q and on k; its
                algorithmic bytes are 4 per element of q and k and direction (read once, written once) plus the two tables.
Per point: the medians in us, fused / torch, GB/s on the algorithmic bytes (every operand read once and every result written once,
forward and backward: 16 bytes per element) against the 8 TB/s peak, the
peak memory each side adds to its operands, and the largest difference of the two routes' gradients.  At these sizes the fused
side of a point is partly the autograd function's Python (two ctypes calls, three to four allocations), so the forward and the
backward entry are also timed alone (glue.*_fwd / *_bwd, outputs allocated per call), with their own GB/s.
--step adds the whole step: the Llama-2-7B shape cut to 4 layers, T = 2048, checkpointing on, attn="own"; glue="torch",
glue="fused" with rope="torch" and glue="fused" with rope="fused" in alternating windows, with each side's peak memory over the
model.
Every point runs under its own time limit (a watchdog ends the process when it overruns) and the first failure ends the run.  One
JSON line per point; no threshold."""
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
PEAK_GBS = 8000.0


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


def report(res, fused, torch_route, leaves, nbytes, reps, kern_fwd, kern_bwd):
    """Both sides return their leaves' gradients; times, GB/s, peaks and the largest gradient difference go into res.  kern_fwd /
    kern_bwd: the two entries alone, each moving half of nbytes."""
    def clear():
        for x in leaves:
            x.grad = None

    def side(fn):
        def run():
            clear()
            fn()
            return [x.grad for x in leaves]
        return run

    f, t = side(fused), side(torch_route)
    gf = [x.float().clone() for x in f()]
    gt = [x.float().clone() for x in t()]
    res["max_grad_diff_rel"] = [float(f"{((a - b).abs().max() / b.abs().max()).item():.3e}") for a, b in zip(gf, gt)]
    del gf, gt
    mem_f, mem_t = peak_rise(f), peak_rise(t)
    us = medians_us([f, t, kern_fwd, kern_bwd], reps, 5)
    clear()
    res.update(fwd_entry_us=round(us[2], 1), bwd_entry_us=round(us[3], 1), fwd_entry_GBs=round(nbytes / 2 / us[2] * 1e-3, 0),
               bwd_entry_GBs=round(nbytes / 2 / us[3] * 1e-3, 0))
    res.update(fused_us=round(us[0], 1), torch_us=round(us[1], 1), fused_over_torch=round(us[0] / us[1], 3),
               fused_GBs=round(nbytes / us[0] * 1e-3, 0), torch_GBs=round(nbytes / us[1] * 1e-3, 0),
               fused_of_peak=round(nbytes / us[0] * 1e-3 / PEAK_GBS, 3), fused_peak_MiB=round(mem_f / 2 ** 20, 1),
               torch_peak_MiB=round(mem_t / 2 ** 20, 1), reps=reps)
    print(json.dumps(res), flush=True)


def points(name, T, hidden, inter, reps):
    from qeft_amd import finetune, glue
    g = torch.Generator(device=DEV).manual_seed(hidden + T)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device=DEV) * scale).half()
    eps = 1e-5
    # ---- add_rmsnorm
    h, add = rn(T, hidden).requires_grad_(True), rn(T, hidden).requires_grad_(True)
    gamma = (1 + 0.1 * torch.randn(hidden, generator=g, device=DEV)).half()
    ds, dy = rn(T, hidden, scale=2.0 ** -4), rn(T, hidden, scale=2.0 ** -4)

    def norm_fused():
        s, y = glue.add_rmsnorm(h, add, gamma, eps)
        torch.autograd.backward([s, y], [ds, dy])

    def norm_torch():
        s = h + add
        torch.autograd.backward([s, finetune._rmsnorm(s, gamma, eps)], [ds, dy])

    with limit(120):
        hd, ad = h.detach(), add.detach()
        report(dict(bench="train_glue", op="add_rmsnorm", widths=name, t=T, hidden=hidden), norm_fused, norm_torch, [h, add],
               16 * T * hidden, reps, lambda: glue.add_rmsnorm_fwd(hd, ad, gamma, eps), lambda: glue.add_rmsnorm_bwd(hd, gamma, dy, ds, eps))
    del h, add, ds, dy
    # ---- SwiGLU
    gate, up = rn(T, inter).requires_grad_(True), rn(T, inter).requires_grad_(True)
    dact = rn(T, inter, scale=2.0 ** -4)

    def swiglu_fused():
        glue.swiglu(gate, up).backward(dact)

    def swiglu_torch():
        (torch.nn.functional.silu(gate.float()) * up.float()).half().backward(dact)

    with limit(120):
        gd, ud = gate.detach(), up.detach()
        report(dict(bench="train_glue", op="swiglu", widths=name, t=T, n=inter), swiglu_fused, swiglu_torch, [gate, up],
               16 * T * inter, reps, lambda: glue.swiglu_fwd(gd, ud), lambda: glue.swiglu_bwd(gd, ud, dact))


def rope_points(T, reps):
    """rope_qk at the 7B (32 / 32) and 70B (64 / 8) head counts, one sequence of T rows."""
    from qeft_amd import finetune, glue, qeft_cuda
    cos, sin = (x.to(DEV) for x in qeft_cuda.rope_cos_sin(10000.0, 64, T))
    c3, s3 = cos[:, None, :], sin[:, None, :]
    for H, Hkv in ((32, 32), (64, 8)):
        g = torch.Generator(device=DEV).manual_seed(H + T)
        rn = lambda h, scale=1.0: (torch.randn(1, T, h, 128, generator=g, device=DEV) * scale).half()
        q, k = rn(H).requires_grad_(True), rn(Hkv).requires_grad_(True)
        dq, dk = rn(H, 2.0 ** -4), rn(Hkv, 2.0 ** -4)

        def rope_fused():
            torch.autograd.backward(list(glue.rope_qk(q, k, cos, sin)), [dq, dk])

        def rope_torch():
            torch.autograd.backward([finetune._rope(q, c3, s3), finetune._rope(k, c3, s3)], [dq, dk])

        with limit(120):
            qd, kd = q.detach(), k.detach()
            report(dict(bench="train_glue", op="rope_qk", heads=f"{H}/{Hkv}", t=T), rope_fused, rope_torch, [q, k],
                   2 * (4 * T * (H + Hkv) * 128 + 2 * 4 * T * 64), reps, lambda: glue.rope_qk_entry(qd, kd, cos, sin),
                   lambda: glue.rope_qk_entry(dq, dk, cos, sin, inverse=True))
        del q, k, dq, dk


def step(T, layers, reps):
    """The whole training step on attn="own": glue="torch", glue="fused" and glue="fused" with rope="fused", alternating."""
    from qeft_amd import finetune
    from qeft_amd.llama import LLAMA2_7B, QuantLlama
    model = QuantLlama(dataclasses.replace(LLAMA2_7B, max_seq=T, n_layers=layers), DEV, seed=0, fast_init=True)
    toks = torch.randint(0, model.shape.vocab, (T,), generator=torch.Generator().manual_seed(1)).to(DEV)
    params = finetune.begin(model)
    losses = {}

    def side(glue, rope):
        def run():
            for p in params:
                p.grad = None
            loss = finetune.causal_lm_loss(model, toks, attn="own", glue=glue, rope=rope)
            (loss * 1024.0).backward()
            losses[glue, rope] = loss
        return run

    f, t, r = side("fused", "torch"), side("torch", "torch"), side("fused", "fused")
    f(), t(), r()
    mem_f, mem_t, mem_r = peak_rise(f), peak_rise(t), peak_rise(r)
    us = medians_us([f, t, r], reps, 5)
    print(json.dumps(dict(bench="train_glue", op="step", layers=layers, t=T, attn="own", checkpoint=True, reps=reps,
                          fused_ms=round(us[0] * 1e-3, 3), torch_ms=round(us[1] * 1e-3, 3), fused_over_torch=round(us[0] / us[1], 4),
                          fused_rope_ms=round(us[2] * 1e-3, 3), fused_rope_over_fused=round(us[2] / us[0], 4),
                          fused_peak_over_model_MiB=round(mem_f / 2 ** 20, 1), torch_peak_over_model_MiB=round(mem_t / 2 ** 20, 1),
                          fused_rope_peak_over_model_MiB=round(mem_r / 2 ** 20, 1),
                          loss_fused=round(losses["fused", "torch"].item(), 6), loss_torch=round(losses["torch", "torch"].item(), 6),
                          loss_fused_rope=round(losses["fused", "fused"].item(), 6))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--T", type=int, default=2048)
    ap.add_argument("--step", action="store_true", help="also time the 4-layer 7B training step on both routes")
    a = ap.parse_args()
    print(json.dumps(dict(bench="train_glue", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    points("7B", a.T, 4096, 11008, a.reps)
    torch.cuda.empty_cache()
    points("70B", a.T, 8192, 28672, a.reps)
    torch.cuda.empty_cache()
    rope_points(a.T, a.reps)
    torch.cuda.empty_cache()
    if a.step:
        with limit(400):
            step(a.T, 4, a.reps)
