"""--steps finetune.causal_lm_loss forward + backward steps on the Llama-2-7B shape cut to --layers decoder layers (synthetic
weights, T = 2048, gradient checkpointing on: DESIGN.md §4.14's setting): the run `rocprofv3 --kernel-trace --stats` is pointed
at, per attention route once with 1 step and once with 3, so that the difference of the two tables is two steps without the
model's construction and the first step's one-off work.

    rocprofv3 --kernel-trace --stats -d OUT3 -o run --output-format csv -- python tools/finetune_step_run.py --attn own --steps 3
    rocprofv3 --kernel-trace --stats -d OUT1 -o run --output-format csv -- python tools/finetune_step_run.py --attn own --steps 1
    python tools/finetune_step_run.py --group OUT3/.../run_kernel_stats.csv --minus OUT1/.../run_kernel_stats.csv --steps 2

--group reads the per-kernel tables and prints their difference grouped into linears / attention / head / own glue (the kernels of
csrc/train_glue.hip) / torch glue, per step.  --glue fused runs the step with those kernels, --rope fused with the rotary kernel
(§4.17); the default is the torch route.  A plain run (no profiler) also prints the wall time of every step and the last step's peak memory over the model."""
import argparse
import csv
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(attn, layers, T, steps, glue="torch", rope="torch"):
    import time
    import torch
    from qeft_amd import finetune
    from qeft_amd.llama import LLAMA2_7B, QuantLlama
    dev = "cuda:0"
    model = QuantLlama(dataclasses.replace(LLAMA2_7B, max_seq=T, n_layers=layers), dev, seed=0, fast_init=True)
    toks = torch.randint(0, model.shape.vocab, (T,), generator=torch.Generator().manual_seed(1)).to(dev)
    params = finetune.begin(model)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    ms = []
    for _ in range(steps):
        for p in params:
            p.grad = None
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        loss = finetune.causal_lm_loss(model, toks, attn=attn, glue=glue, rope=rope)
        (loss * 1024.0).backward()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    # wall time of the later steps (the first carries one-off work) and the last step's peak over the model and its gradients' home
    print(json.dumps(dict(run="finetune_step", attn=attn, glue=glue, rope=rope, layers=layers, T=T, steps=steps, loss=round(loss.item(), 6),
                          step_ms=[round(x, 2) for x in ms], median_later_ms=round(sorted(ms[1:])[len(ms[1:]) // 2], 2) if steps > 1 else None,
                          peak_over_model_MiB=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))), flush=True)


def family(name):
    n = name.lower()
    if "lm_head_nll" in n:
        return "head"
    if "add_rmsnorm" in n or "swiglu" in n or "rope_qk" in n:
        return "own glue"
    if "attn_train" in n or "prefill_attn" in n or "attention" in n or "fmha" in n or "flash" in n or "softmax" in n or "cijk_" in n \
            or "bmm" in n or "aotriton" in n or "attn_" in n or "bwd_kernel_d" in n or "bwd_preprocess" in n:
        return "attention"
    if "qeft" in n and ("gemm" in n or "dx" in n or "grad_oweight" in n or "gemv" in n):
        return "linears"
    return "torch glue"


def table(path):
    with open(path, newline="") as f:
        return {r["Name"]: (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)}


def group(path, minus, steps):
    full, less = table(path), table(minus) if minus else {}
    rows = []
    for name, (calls, ns) in full.items():
        c0, n0 = less.get(name, (0, 0))
        if calls - c0 > 0:
            rows.append((name, calls - c0, max(ns - n0, 0)))
    total = sum(r[2] for r in rows)
    fam = {}
    for name, calls, ns in rows:
        d = fam.setdefault(family(name), [0, 0, []])
        d[0] += calls
        d[1] += ns
        d[2].append((ns, calls, name))
    print(f"{path}: {len(rows)} kernels, {total / steps * 1e-6:.3f} ms of kernel time per step ({steps} steps)")
    for key in ("linears", "attention", "head", "own glue", "torch glue"):
        calls, ns, items = fam.get(key, [0, 0, []])
        print(f"  {key:<11} {ns / steps * 1e-6:8.3f} ms  {100.0 * ns / max(total, 1):5.1f} %  {calls // steps:5d} launches per step")
        for ns_i, calls_i, name in sorted(items, reverse=True)[:6]:
            print(f"      {ns_i / steps * 1e-6:8.3f} ms  {calls_i // steps:5d} x  {name[:110]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn", default="own", choices=("own", "sdpa"))
    ap.add_argument("--glue", default="torch", choices=("torch", "fused"))
    ap.add_argument("--rope", default="torch", choices=("torch", "fused"))
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--T", type=int, default=2048)
    ap.add_argument("--group")
    ap.add_argument("--minus")
    ap.add_argument("--steps", type=int, default=2)
    a = ap.parse_args()
    if a.group:
        group(a.group, a.minus, a.steps)
    else:
        run(a.attn, a.layers, a.T, a.steps, a.glue, a.rope)
