"""The fine-tune step over sequences of unequal length, three ways: one GPU, one process, HIP events, a warm-up
of every side before any measurement, the sides alternating (medians of --reps windows of --inner steps).

    python tools/bench_packed_step.py [--reps 7] [--inner 3] > profiles/packed_step_bench.json.log

The Llama-2-7B shape cut to 4 layers, glue="fused", rope="fused", attn="own", checkpointing on, loss scaled by 1024, and ONE list
of 16 sequence lengths between 40 and 600 that sums to 2052 (LENS below, chosen once and not tuned: roughly the long-tailed mix
of an instruction set, in no particular order).  A step is forward + backward over all 16 sequences with the gradients of the
outlier slices accumulated:
  (a) packed        one causal_lm_loss(tokens [2052], seq_lens=LENS): causal_attention_packed, the rotary restarting per sequence;
  (b) one by one    16 calls causal_lm_loss(tokens [T_i]) and 16 backward passes, the reference's per_device_train_batch_size = 1;
  (c) right-padded  one causal_lm_loss(tokens [16, 600]) with the padding labelled -100.
Per side: the step's median time, tokens / s over the 2052 real tokens, the peak memory the step adds to the model; then the
attention entries alone at 32 / 32 heads, forward + backward, packed against padded (and against the 16 single launches).
Every part runs under its own time limit (a watchdog ends the process when it overruns).  One JSON line per part; no threshold."""
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
LENS = [155, 40, 600, 62, 90, 290, 46, 125, 50, 200, 41, 80, 105, 55, 70, 43]
LOSS_SCALE = 1024.0


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
    return [statistics.median(t) for t in ts], [(min(t), max(t)) for t in ts]


def peak_rise(fn):
    """Bytes by which one call of fn lifts the allocator's peak over what is allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def step(layers, reps, inner):
    from qeft_amd import finetune
    from qeft_amd.llama import LLAMA2_7B, QuantLlama
    model = QuantLlama(dataclasses.replace(LLAMA2_7B, max_seq=max(LENS), n_layers=layers), DEV, seed=0, fast_init=True)
    g = torch.Generator().manual_seed(1)
    seqs = [torch.randint(0, model.shape.vocab, (n,), generator=g).to(DEV) for n in LENS]
    packed = torch.cat(seqs)
    tok_pad = torch.zeros(len(LENS), max(LENS), dtype=torch.long, device=DEV)
    lab_pad = torch.full_like(tok_pad, finetune.IGNORE_INDEX)
    for i, s in enumerate(seqs):
        tok_pad[i, :len(s)] = lab_pad[i, :len(s)] = s
    params = finetune.begin(model)
    route = dict(attn="own", glue="fused", rope="fused", checkpoint=True)
    n_targets = sum(LENS) - len(LENS)
    losses = {}

    def zero():
        for p in params:
            p.grad = None

    def a():
        zero()
        loss = finetune.causal_lm_loss(model, packed, seq_lens=LENS, **route)
        (loss * LOSS_SCALE).backward()
        losses["packed"] = loss

    def b():
        zero()
        total = 0.0
        for s in seqs:                                   # each sequence's mean NLL weighted back to the mean over all targets
            loss = finetune.causal_lm_loss(model, s, **route)
            (loss * (LOSS_SCALE * (len(s) - 1) / n_targets)).backward()
            total = total + loss.detach() * ((len(s) - 1) / n_targets)
        losses["one_by_one"] = total

    def c():
        zero()
        loss = finetune.causal_lm_loss(model, tok_pad, lab_pad, **route)
        (loss * LOSS_SCALE).backward()
        losses["padded"] = loss

    sides = (("packed", a), ("one_by_one", b), ("padded", c))
    for _, fn in sides:
        fn()
    mem = {name: peak_rise(fn) for name, fn in sides}
    us, spread = medians_us([fn for _, fn in sides], reps, inner)
    res = dict(bench="packed_step", op="step", layers=layers, lens=LENS, tokens=sum(LENS), padded_rows=len(LENS) * max(LENS), reps=reps,
               inner=inner, **route)
    for (name, _), t, (lo, hi) in zip(sides, us, spread):
        res[f"{name}_ms"] = round(t * 1e-3, 3)
        res[f"{name}_ms_min_max"] = [round(lo * 1e-3, 3), round(hi * 1e-3, 3)]
        res[f"{name}_tokens_per_s"] = round(sum(LENS) / (t * 1e-6))
        res[f"{name}_peak_over_model_MiB"] = round(mem[name] / 2 ** 20, 1)
        res[f"loss_{name}"] = round(float(losses[name].detach()), 6)
    res["packed_over_one_by_one"] = round(us[0] / us[1], 4)
    res["packed_over_padded"] = round(us[0] / us[2], 4)
    print(json.dumps(res), flush=True)


def attention_alone(heads, kv, reps, inner):
    """The attention entries alone, forward + backward, outputs allocated per call as under autograd."""
    from qeft_amd import attention as at
    g = torch.Generator(device=DEV).manual_seed(2)
    R, T, B = sum(LENS), max(LENS), len(LENS)
    mk = lambda rows, h: torch.randn(rows, h, 128, generator=g, device=DEV).half()
    q, k, v, do = mk(R, heads), mk(R, kv), mk(R, kv), mk(R, heads) * 2.0 ** -4
    q4, k4, v4, do4 = (mk(B * T, h).view(B, T, h, 128) for h in (heads, kv, kv, heads))
    cu = [0]
    for n in LENS:
        cu.append(cu[-1] + n)
    ones = [tuple(x[cu[i]:cu[i + 1]][None] for x in (q, k, v, do)) for i in range(B)]

    def a():
        out, lse = at.attn_train_varlen_fwd(q, k, v, LENS)
        at.attn_train_varlen_bwd(q, k, v, out, lse, do, LENS)

    def b():
        for q1, k1, v1, d1 in ones:
            out, lse = at.attn_train_fwd(q1, k1, v1)
            at.attn_train_bwd(q1, k1, v1, out, lse, d1)

    def c():
        out, lse = at.attn_train_fwd(q4, k4, v4)
        at.attn_train_bwd(q4, k4, v4, out, lse, do4)

    us, spread = medians_us([a, b, c], reps, 10 * inner)
    print(json.dumps(dict(bench="packed_step", op="attention fwd + bwd", heads=heads, kv_heads=kv, lens=LENS, reps=reps,
                          inner=10 * inner, packed_us=round(us[0], 1), one_by_one_us=round(us[1], 1), padded_us=round(us[2], 1),
                          packed_us_min_max=[round(x, 1) for x in spread[0]], padded_us_min_max=[round(x, 1) for x in spread[2]],
                          packed_over_padded=round(us[0] / us[2], 4), packed_over_one_by_one=round(us[0] / us[1], 4))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--layers", type=int, default=4)
    a = ap.parse_args()
    print(json.dumps(dict(bench="packed_step", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    with limit(120):
        attention_alone(32, 32, a.reps, a.inner)
    with limit(400):
        step(a.layers, a.reps, a.inner)
