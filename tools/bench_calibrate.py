"""The calibrator against the torch route on the same tensors: one GPU, one process, HIP events, a warm-up
of every side before any measurement, the sides alternating (medians of --reps runs).

    python tools/bench_calibrate.py [--reps 5] > profiles/calib_bench.json.log

  add_batch      HessianAccumulator.add_batch (qeft_hessian_accum) against the reference's own lines on the GPU
                 (H *= n / (n + 1); x = sqrt(2 / n) * x.float(); H += x.T @ x) at (T, K) = (2048, 4096) and (2048, 11008);
                 in windows of back-to-back calls of 0.1 s and more; for the own side the useful T K (K + 128) FLOP (one
                 triangle of tiles) over the END-TO-END time per call -- event time of the window, Python and launch gaps
                 included, not kernel time -- as a share of the dense fp16 matrix peak
  reconstruction gptq_reorder (qeft_gptq_block per 128 columns) against tests/calib_ref.gptq_reorder in fp32 on the GPU -- the
                 reference's own expressions, one python iteration per column -- at N x K = 4096 x 4096, 11008 x 4096 and
                 4096 x 11008 with 128 outlier columns; then the own side's parts, each timed alone over the same tensors:
                 the factorisation (damping + three Cholesky calls), the block launches, the trailing GEMMs, the parameter search
One JSON line per part; no threshold.  Every part runs under its own time limit."""
import argparse
import faulthandler
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
PEAK_F16_FLOPS = 2.5e15          # dense fp16 matrix peak of the MI355X


class limit:
    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        return False


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def medians_ms(fns, reps, warm=1):
    for _ in range(warm):
        for fn in fns:
            timed_ms(fn)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            t.append(timed_ms(fn))
    return [statistics.median(t) for t in ts], [(min(t), max(t)) for t in ts]


def rows(t, k, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(t, k, generator=g, device=DEV)
    x[:, ::37] *= 8
    return x.half()


def add_batch_bench(t, k, reps, inner):
    from qeft_amd.calibrate import HessianAccumulator
    x = rows(t, k, 1)
    acc = HessianAccumulator(k, DEV)
    H = torch.zeros(k, k, device=DEV)

    def own():
        for _ in range(inner):
            acc.add_batch(x)

    state = dict(n=0)

    def ref():
        nonlocal H
        for _ in range(inner):
            H *= state["n"] / (state["n"] + 1)
            state["n"] += 1
            inp = math.sqrt(2 / state["n"]) * x.float().t()
            H += inp.matmul(inp.t())

    us, spread = medians_ms([own, ref], reps)
    rel = ((acc.H - H).abs().max() / H.abs().max()).item()           # the same number of batches on both sides
    res = dict(bench="calibrate", op="add_batch", t=t, k=k, reps=reps, inner=inner, own_ms=round(us[0] / inner, 4),
               own_ms_min_max=[round(v / inner, 4) for v in spread[0]], torch_ms=round(us[1] / inner, 4),
               torch_ms_min_max=[round(v / inner, 4) for v in spread[1]], own_over_torch=round(us[0] / us[1], 4),
               own_end_to_end_share_of_f16_peak=round(t * k * (k + 128.0) / (us[0] / inner * 1e-3) / PEAK_F16_FLOPS, 4),
               max_abs_diff_over_max=rel)
    print(json.dumps(res), flush=True)


def recon_bench(n, k, r, reps):
    import calib_ref as R
    from qeft_amd import _lib
    from qeft_amd.calibrate import BLOCK, HessianAccumulator, _params, gptq_reorder
    g = torch.Generator(device=DEV).manual_seed(2)
    W = (torch.randn(n, k, generator=g, device=DEV) * 0.02).half()
    acc = HessianAccumulator(k, DEV)
    acc.add_batch(rows(2048, k, 3))
    H = acc.H
    ids = torch.arange(k, device=DEV)
    out = {}

    def own():
        out["own"] = gptq_reorder(W, H, ids, r)

    def ref():
        out["ref"] = R.gptq_reorder(W.float(), H, k - r, torch.float32)

    us, spread = medians_ms([own, ref], reps, warm=1)
    Wf = W.float()
    l_own, l_ref = out["own"].proxy_loss, R.proxy_loss(Wf, out["ref"][0], H)
    # the own side's parts, alone
    hinv = out["ref"][3].contiguous()
    Wk = Wf.clone()
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    blocks = [(i1, min(i1 + BLOCK, k - r)) for i1 in range(0, k - r, BLOCK)]
    par = [_params(Wk[:, i1:i2], 4, "minmax") for i1, i2 in blocks]
    par = [(s.contiguous(), z.contiguous()) for s, z in par]
    q1 = torch.empty(n, BLOCK, device=DEV)
    e1 = torch.empty(n, BLOCK, device=DEV)

    def factorisation():
        R.factor(H, torch.float32)

    def launches():
        for (i1, i2), (s, z) in zip(blocks, par):
            _lib.check(lib.qeft_gptq_block(Wk.data_ptr() + 4 * i1, k, hinv.data_ptr() + 4 * (i1 * k + i1), k, s.data_ptr(), z.data_ptr(),
                                           q1.data_ptr(), e1.data_ptr(), n, i2 - i1, 15, st))

    def gemms():
        for i1, i2 in blocks:
            Wk[:, i2:] -= e1[:, :i2 - i1].matmul(hinv[i1:i2, i2:])

    def search():
        for i1, i2 in blocks:
            _params(Wk[:, i1:i2], 4, "minmax")

    e1.zero_()                                                        # the GEMMs then leave Wk as it is
    parts, pspread = medians_ms([factorisation, launches, gemms, search], reps, warm=1)
    res = dict(bench="calibrate", op="reconstruction", n=n, k=k, n_out=r, reps=reps, blocks=len(blocks),
               own_ms=round(us[0], 2), own_ms_min_max=[round(v, 2) for v in spread[0]], torch_ms=round(us[1], 2),
               torch_ms_min_max=[round(v, 2) for v in spread[1]], own_over_torch=round(us[0] / us[1], 4),
               own_factorisation_ms=round(parts[0], 2), own_block_launches_ms=round(parts[1], 2),
               own_block_launch_us_each=round(parts[1] * 1e3 / len(blocks), 1), own_trailing_gemms_ms=round(parts[2], 2),
               own_parameter_search_ms=round(parts[3], 2), proxy_loss_own=l_own, proxy_loss_torch=l_ref,
               proxy_loss_rtn=R.proxy_loss(Wf, R.rtn(Wf, k - r), H))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--only-add-batch", action="store_true")
    a = ap.parse_args()
    print(json.dumps(dict(bench="calibrate", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    for t, k, inner in ([(128, 256, 8)] if a.small else [(2048, 4096, 1000), (2048, 11008, 200)]):
        with limit(240):
            add_batch_bench(t, k, a.reps, inner)
    for n, k in ([] if a.only_add_batch else [(64, 384)] if a.small else [(4096, 4096), (11008, 4096), (4096, 11008)]):
        with limit(400):
            recon_bench(n, k, 128, a.reps)
