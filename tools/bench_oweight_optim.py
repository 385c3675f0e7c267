"""The training update against the torch route on the same tensors: one GPU, one process, HIP events, a warm-up
of every side before any measurement, the sides alternating (medians of --reps windows of back-to-back steps).

    python tools/bench_oweight_optim.py [--reps 7] [--inner 100] > profiles/oweight_optim_bench.json.log
    python tools/bench_oweight_optim.py --one torch_foreach --steps 3      K steps of one side and nothing else, for a kernel trace

Arenas of the Llama-2-7B layout (224 tensors [N, 128], 174 M fp32) and of the 13B layout (280 tensors, 273 M), gradients of
N(0, 1e-6^2) at a loss scale of 1 so that neither route's in-place unscaling and clipping changes them from step to step (the
norm stays below max_grad_norm: the clip multiplies by 1, at the same cost).
  own           OWeightAdamW.step(): qeft_oweight_grad_stats + qeft_oweight_adamw, 32 bytes per weight (g; then p, g, m, v read
                and p, m, v written), at 1, 2 and 4 chunks per thread per iteration, g loaded plainly and non-temporally
  torch         torch._foreach_mul_(grads, 1 / scale) -> clip_grad_norm_(foreach=True) -> torch.optim.AdamW.step(), foreach=True and
                fused=True where this build accepts it, each with and without the found_inf.item() a GradScaler performs
Per side: the median time of a step, the spread, and for the own sides bytes / time as a fraction of 8 TB/s.
Then the 4-layer packed step of §4.18 (tools/bench_packed_step.py's model, lengths and route), whole: finetune.train_step against
the same forward + backward followed by the torch route (foreach, with the .item()).
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
LENS = [155, 40, 600, 62, 90, 290, 46, 125, 50, 200, 41, 80, 105, 55, 70, 43]          # tools/bench_packed_step.py
PEAK_BYTES_PER_S = 8e12
BYTES_PER_WEIGHT = 32
MAX_NORM = 0.3


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


def medians_us(fns, reps, inners, warm=3):
    """The sides alternate: per side the median over `reps` windows of its `inner` back-to-back calls, after `warm` calls each."""
    for _ in range(warm):
        for fn in fns:
            timed(fn, 1)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t, inner in zip(fns, ts, inners):
            t.append(timed(fn, inner))
    return [statistics.median(t) for t in ts], [(min(t), max(t)) for t in ts]


def layout_shapes(shape, r=128):
    """The oweight shapes of a model, in finetune.begin's order: q, k, v, o, gate, up, down of every layer, [N, r]."""
    kv = shape.hidden // shape.n_heads * shape.n_kv_heads
    outs = [shape.hidden, kv, kv, shape.hidden, shape.inter, shape.inter, shape.hidden]
    return [(n, r) for _ in range(shape.n_layers) for n in outs]


def torch_route(params, opt, inv_scale, item):
    """What a user assembles today: unscale, clip, (look at found_inf), AdamW."""
    grads = [q.grad for q in params]
    torch._foreach_mul_(grads, inv_scale)
    norm = torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
    found_inf = ~torch.isfinite(norm)
    if item and found_inf.item():
        return
    opt.step()


def torch_optimisers(params):
    """{'foreach': AdamW, 'fused': AdamW or the refusal's text}"""
    out = {"foreach": torch.optim.AdamW(params, lr=2e-4, weight_decay=0.0, foreach=True)}
    try:
        out["fused"] = torch.optim.AdamW(params, lr=2e-4, weight_decay=0.0, fused=True)
    except Exception as e:                               # this build does not take fused=True here: the log says so
        out["fused"] = f"{type(e).__name__}: {e}"
    return out


def make_arena(shape):
    from qeft_amd import OWeightAdamW
    g = torch.Generator(device=DEV).manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g, device=DEV) * 0.02) for s in layout_shapes(shape)]
    own = OWeightAdamW(params, loss_scale=None, max_grad_norm=MAX_NORM)
    own.arena.g.copy_(torch.randn(own.arena.n, generator=g, device=DEV) * 1e-6)
    return params, own


def arena_bench(shape, reps, inner):
    from qeft_amd import _lib
    lib = _lib.lib()
    params, own = make_arena(shape)
    n = own.arena.n
    assert lib.qeft_oweight_optim_blocks(n) == own._blocks == 2048
    sides, names, inners = [], [], []

    def own_side(u, nt):
        def run():
            lib.qeft_oweight_optim_lab(u, nt)              # host-side switch; the grid is 2048 blocks in every geometry at this size
            own.step()
        return run
    try:
        for u in (1, 2, 4):
            for nt in (0, 1):
                assert lib.qeft_oweight_optim_lab(u, nt) == 0 and lib.qeft_oweight_optim_blocks(n) == 2048
                sides.append(own_side(u, nt))
                names.append(f"own_u{u}" + ("_nt" if nt else ""))
                inners.append(inner)
        opts = torch_optimisers(params)
        refused = {k: v for k, v in opts.items() if isinstance(v, str)}
        for kind, opt in opts.items():
            if isinstance(opt, str):
                continue
            for item in (False, True):
                sides.append(lambda opt=opt, item=item: torch_route(params, opt, 1.0, item))
                names.append(f"torch_{kind}" + ("_item" if item else ""))
                inners.append(max(1, inner // 5))
        us, spread = medians_us(sides, reps, inners)
    finally:
        lib.qeft_oweight_optim_lab(0, 0)
    own.arena.check_grads()
    rec = own.stats()
    res = dict(bench="oweight_optim", op="update", layout=shape.name, tensors=len(params), n=n, reps=reps, inner=inner,
               bytes_per_weight=BYTES_PER_WEIGHT, own_launches_per_step=2, torch_launches_per_step="not measured here (kernel trace)",
               own_steps_applied=rec["step"], own_steps_skipped=rec["n_skipped"])
    if refused:
        res["torch_refused"] = refused
    for name, t, (lo, hi) in zip(names, us, spread):
        res[f"{name}_us"] = round(t, 1)
        res[f"{name}_us_min_max"] = [round(lo, 1), round(hi, 1)]
        if name.startswith("own"):
            res[f"{name}_share_of_8TBps"] = round(BYTES_PER_WEIGHT * n / (t * 1e-6) / PEAK_BYTES_PER_S, 4)
    best_torch = min(t for name, t in zip(names, us) if name.startswith("torch"))
    res["own_u2_over_best_torch"] = round(us[names.index("own_u2")] / best_torch, 4)
    print(json.dumps(res), flush=True)


def step_bench(layers, reps, inner):
    from qeft_amd import OWeightAdamW, finetune
    from qeft_amd.llama import LLAMA2_7B, QuantLlama
    model = QuantLlama(dataclasses.replace(LLAMA2_7B, max_seq=max(LENS), n_layers=layers), DEV, seed=0, fast_init=True)
    g = torch.Generator().manual_seed(1)
    packed = torch.cat([torch.randint(0, model.shape.vocab, (n,), generator=g) for n in LENS]).to(DEV)
    params = finetune.begin(model)
    own = OWeightAdamW(params, loss_scale=1024.0, max_grad_norm=MAX_NORM)
    topt = torch.optim.AdamW(params, lr=2e-4, weight_decay=0.0, foreach=True)
    route = dict(attn="own", glue="fused", rope="fused", checkpoint=True)
    views = own.arena.views(own.arena.g)
    losses = {}

    def a():
        for q, view in zip(params, views):                  # side b sets the gradients to None, as a torch loop does
            q.grad = view
        losses["train_step"] = finetune.train_step(model, own, [(packed, None, LENS)], **route)

    def b():
        for q in params:
            q.grad = None
        loss = finetune.causal_lm_loss(model, packed, seq_lens=LENS, **route)
        (loss * 1024.0).backward()
        torch_route(params, topt, 1.0 / 1024.0, True)
        losses["torch_route"] = loss.detach()

    def c():                                                # forward + backward alone: what both sides share
        for q in params:
            q.grad = None
        loss = finetune.causal_lm_loss(model, packed, seq_lens=LENS, **route)
        (loss * 1024.0).backward()

    us, spread = medians_us([a, b, c], reps, [inner, inner, inner], warm=2)
    rec = own.stats()
    res = dict(bench="oweight_optim", op="packed step + update", layers=layers, tokens=sum(LENS), n=own.arena.n, reps=reps, inner=inner,
               **route, own_steps_applied=rec["step"], own_steps_skipped=rec["n_skipped"])
    for name, t, (lo, hi) in zip(("train_step", "torch_route", "fwd_bwd_alone"), us, spread):
        res[f"{name}_ms"] = round(t * 1e-3, 3)
        res[f"{name}_ms_min_max"] = [round(lo * 1e-3, 3), round(hi * 1e-3, 3)]
        res[f"{name}_tokens_per_s"] = round(sum(LENS) / (t * 1e-6))
    res["loss_train_step"] = round(float(losses["train_step"]), 6)
    res["loss_torch_route"] = round(float(losses["torch_route"]), 6)
    res["train_step_over_torch_route"] = round(us[0] / us[1], 4)
    print(json.dumps(res), flush=True)


def one_side(side, steps):
    """`steps` steps of one side on the 7B arena, for a kernel trace of its launches."""
    from qeft_amd.llama import LLAMA2_7B
    params, own = make_arena(LLAMA2_7B)
    if side == "own":
        fn = own.step
    else:
        opt = torch_optimisers(params)[side.split("_")[1]]
        if isinstance(opt, str):
            raise SystemExit(f"{side}: {opt}")
        fn = lambda: torch_route(params, opt, 1.0, False)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(bench="oweight_optim", op="one side", side=side, steps=steps, n=own.arena.n)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--one", choices=["own", "torch_foreach", "torch_fused"])
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    if a.one:
        with limit(120):
            one_side(a.one, a.steps)
        sys.exit(0)
    from qeft_amd.llama import LLAMA2_7B, LLAMA2_13B
    print(json.dumps(dict(bench="oweight_optim", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    with limit(240):
        arena_bench(LLAMA2_7B, a.reps, a.inner)
    with limit(240):
        arena_bench(LLAMA2_13B, a.reps, a.inner)
    with limit(400):
        step_bench(a.layers, a.reps, 3)
