"""The training attention (attention.causal_attention: qeft_attn_train_fwd, qeft_attn_train_bwd) against the
attention finetune.causal_lm_loss runs by default: one GPU, one process, HIP events, a warm-up before every measurement, the
sides of a point alternating (medians of --reps windows).

    python tools/bench_attn_train.py [--reps 10] > profiles/attn_train_bench.json.log

Head layouts 32 / 32 and 64 / 8 at T = 512, 2048, 8192, B = 1, random operands, the gradient taken in q, k and v:
  (a) torch's scaled_dot_product_attention forward + backward as finetune calls it, repeat_interleave of k / v included;
  (c) causal_attention forward + backward;
  F / D / Kv / Q  the four launches alone (forward, delta, dK / dV, dQ); P  qeft_attn_prefill at start = 0 over a cache holding
  the same K / V, the kernel whose body the forward shares.
Per point: the medians, c / a, TFLOP/s on the causal FLOP count (T^2 / 2 (row, key) pairs, 256 FLOPs per pair and product: the
forward runs 2 products, dK / dV 4, dQ 3; a and c are rated on the 7 products a backward needs at least, not on the 9 that c
runs), the peak memory each side adds to the operands, and the largest difference of the two routes' gradients.
A shape at which route a cannot allocate is skipped for a and says so; nothing else is caught.  Every step runs under its own
time limit (a watchdog ends the process when a step overruns it) and the first failure ends the run.  One JSON line per point;
no threshold."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
HD = 128


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


def point(heads, kv, T, reps):
    from qeft_amd import _lib, attention
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=DEV).manual_seed(heads + kv + T)
    rep = heads // kv
    q = torch.randn(1, T, heads, HD, generator=g, device=DEV).half().requires_grad_(True)
    k = torch.randn(1, T, kv, HD, generator=g, device=DEV).half().requires_grad_(True)
    v = torch.randn(1, T, kv, HD, generator=g, device=DEV).half().requires_grad_(True)
    dout = (torch.randn(1, T, heads, HD, generator=g, device=DEV) * 2.0 ** -4).half()

    def clear():
        q.grad = k.grad = v.grad = None

    def sdpa():
        clear()
        kk, vv = (k.repeat_interleave(rep, 2), v.repeat_interleave(rep, 2)) if rep != 1 else (k, v)
        a = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), kk.transpose(1, 2), vv.transpose(1, 2), is_causal=True)
        a.transpose(1, 2).backward(dout)
        return q.grad, k.grad, v.grad

    def own():
        clear()
        attention.causal_attention(q, k, v).backward(dout)
        return q.grad, k.grad, v.grad

    res = dict(bench="attn_train", heads=heads, kv=kv, t=T, reps=reps)
    g_own = [x.float().clone() for x in own()]
    mem_own = peak_rise(own) + attention._workspace[torch.device(DEV)].numel()
    have_a = True
    try:
        g_ref = [x.float().clone() for x in sdpa()]
    except torch.cuda.OutOfMemoryError:
        have_a = False
        res["sdpa"] = "skipped: out of memory"
        clear()
        torch.cuda.empty_cache()
    if have_a:
        res["max_grad_diff_rel"] = [float(f"{((a - b).abs().max() / b.abs().max()).item():.3e}") for a, b in zip(g_own, g_ref)]
        mem_a = peak_rise(sdpa)
        del g_ref
    del g_own
    clear()

    # the four launches alone, and the prompt attention on a cache with the same K / V
    qd, kd, vd = q.detach(), k.detach(), v.detach()
    out, lse = attention.attn_train_fwd(qd, kd, vd)
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    need = lib.qeft_attn_train_bwd_workspace_bytes(1, T, heads, kv)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    kc, vc = kd[0].transpose(0, 1).contiguous(), vd[0].transpose(0, 1).contiguous()
    pout = torch.empty(T, heads * HD, dtype=torch.float16, device=DEV)
    H, K = heads * HD, kv * HD

    def fwd():
        _lib.check(lib.qeft_attn_train_fwd(qd.data_ptr(), H, kd.data_ptr(), vd.data_ptr(), K, out.data_ptr(), H, lse.data_ptr(), 1, T,
                                           heads, kv, st))

    def part(i):
        def run():
            _lib.check(lib.qeft_attn_train_bwd_part(qd.data_ptr(), H, kd.data_ptr(), vd.data_ptr(), K, out.data_ptr(), H, dout.data_ptr(),
                                                    H, lse.data_ptr(), dq.data_ptr(), H, dk.data_ptr(), dv.data_ptr(), K, ws.data_ptr(),
                                                    need, 1, T, heads, kv, i, st))
        return run

    def prefill():
        _lib.check(lib.qeft_attn_prefill(qd.data_ptr(), H, kc.data_ptr(), vc.data_ptr(), T, pout.data_ptr(), H, 0, T, heads, kv, st))

    inner = 5 if T <= 2048 else 2
    sides = [own, fwd, part(0), part(1), part(2), prefill] + ([sdpa] if have_a else [])
    us = medians_us(sides, reps, inner)
    torch.cuda.synchronize()
    assert torch.equal(out.view(T, H), pout), "the forward and qeft_attn_prefill(start = 0) disagree"
    pair = T * T / 2 * 2 * HD * heads                                     # FLOPs of one product over the causal pairs
    tf = lambda n, t_us: round(n * pair / t_us * 1e-6, 1)
    res.update(own_fwd_bwd_us=round(us[0], 1), fwd_us=round(us[1], 1), delta_us=round(us[2], 1), dkv_us=round(us[3], 1),
               dq_us=round(us[4], 1), prefill_us=round(us[5], 1), fwd_over_prefill=round(us[1] / us[5], 4),
               own_TFLOPs=tf(7, us[0]), fwd_TFLOPs=tf(2, us[1]), dkv_TFLOPs=tf(4, us[3]), dq_TFLOPs=tf(3, us[4]),
               own_peak_MiB=round(mem_own / 2 ** 20, 1))
    if have_a:
        res.update(sdpa_fwd_bwd_us=round(us[6], 1), own_over_sdpa=round(us[0] / us[6], 3), sdpa_TFLOPs=tf(7, us[6]),
                   sdpa_peak_MiB=round(mem_a / 2 ** 20, 1))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lengths", type=int, nargs="*", default=[512, 2048, 8192])
    a = ap.parse_args()
    backends = {n: bool(getattr(torch.backends.cuda, n)()) for n in ("flash_sdp_enabled", "mem_efficient_sdp_enabled", "math_sdp_enabled")
                if hasattr(torch.backends.cuda, n)}
    print(json.dumps(dict(bench="attn_train", device=torch.cuda.get_device_name(0), torch=torch.__version__, sdpa_backends=backends)),
          flush=True)
    for heads, kv in ((32, 32), (64, 8)):
        for T in a.lengths:
            with limit(180):
                point(heads, kv, T, a.reps)
            torch.cuda.empty_cache()
