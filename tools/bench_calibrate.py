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
  --only-mse     (> profiles/calib_mse_bench.json.log) the MSE parameter search: mse_search (one launch of qeft_mse_search)
                 against calibrate.mse_params (640 torch passes) at [4096, 128], [11008, 128] and [4096, 4096] (the whole-row
                 search of frob_norm_error), with the rows on which the two return another pair; then the 4096 x 4096
                 reconstruction with tuning = "minmax", "mse" and "mse_torch", the three sides alternating
  --only-factor  (> profiles/calib_factor_bench.json.log) the factor of the inverse Hessian at K = 4096 and 11008: the three torch
                 calls against hinv_factor (qeft_hinv_factor, 3 K / 128 - 1 launches) on the same damped matrix, then a whole
                 4096 x K reconstruction with factor = "torch" and factor = "own" 
  --only-pack    (> profiles/quant_pack_bench.json.log) the packing step: calibrate_linear(factor="own") end
                 to end with pack="host" and pack="device", alternating, at N x K = 4096 x 4096, 11008 x 4096 and 4096 x 11008
                 with 128 outlier columns; then the qeft_quant_pack launch alone, given and find mode, in windows of back-to-back
                 launches through the C entry on preallocated outputs -- over ONE weight matrix (it fits the Infinity Cache) and
                 cycling 8 (they do not) -- with its algorithmic bytes 2 N K + N K / 2 + 12 N K / 128 over that time as a
                 share of 8 TB/s
  --only-loop    (> profiles/calib_rows_bench.json.log) the error-feedback loop alone: gptq_reorder with a
                 precomputed hinv, loop = "blocks" against loop = "rows", alternating, at N x K = 4096 x 4096, 11008 x 4096 and
                 4096 x 11008 with 128 outlier columns; then the qeft_gptq_rows launch alone on preallocated outputs
  --only-rows-mse  (> profiles/calib_rows_mse_bench.json.log) the MSE search inside the one launch:
                 gptq_reorder with a precomputed hinv at the same three shapes with loop = "blocks", tuning = "mse" (the parent's
                 only way to the search), loop = "rows", tuning = "minmax" (the price of the search inside the launch) and
                 loop = "rows", tuning = "mse_fused", alternating; then the qeft_gptq_rows_mse launch alone on preallocated outputs
  --only-pc      (> profiles/calib_pc_bench.json.log) per-channel grids, group_size = -1: gptq_reorder with
                 a precomputed hinv at the same three shapes, loop = "rows" / "blocks" x min-max / the search, alternating; the
                 qeft_gptq_rows_pc and qeft_gptq_rows_pc_mse launches alone; qeft_quant_pack_pc given and find in windows of launches
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


def mse_search_bench(n, g, reps):
    """The search alone: one launch of qeft_mse_search against calibrate.mse_params (640 torch passes) on the same rows."""
    from qeft_amd.calibrate import mse_params, mse_search
    gen = torch.Generator(device=DEV).manual_seed(4)
    x = (torch.randn(n, g, generator=gen, device=DEV) * 0.02).half().float()
    out = {}

    def own():
        out["own"] = mse_search(x, 4)

    def ref():
        out["ref"] = mse_params(x, 4)

    us, spread = medians_ms([own, ref], reps)
    differ = ((out["own"][0] != out["ref"][0]) | (out["own"][1] != out["ref"][1])).sum().item()
    res = dict(bench="calibrate", op="mse_search", n=n, g=g, bits=4, reps=reps, own_ms=round(us[0], 4),
               own_ms_min_max=[round(v, 4) for v in spread[0]], torch_ms=round(us[1], 2),
               torch_ms_min_max=[round(v, 2) for v in spread[1]], own_over_torch=round(us[0] / us[1], 6),
               candidate_elements_per_s=round(n * g * 640.0 / (us[0] * 1e-3), 0), rows_with_another_pair=differ)
    print(json.dumps(res), flush=True)


def mse_recon_bench(n, k, r, reps):
    """One reconstruction with each parameter search: min-max, the search kernel, the torch search."""
    import calib_ref as R
    from qeft_amd.calibrate import HessianAccumulator, gptq_reorder
    g = torch.Generator(device=DEV).manual_seed(2)
    W = (torch.randn(n, k, generator=g, device=DEV) * 0.02).half()
    acc = HessianAccumulator(k, DEV)
    acc.add_batch(rows(2048, k, 3))
    H = acc.H
    ids = torch.arange(k, device=DEV)
    tunings = ("minmax", "mse", "mse_torch")
    out = {}

    def side(tuning):
        def run():
            out[tuning] = gptq_reorder(W, H, ids, r, tuning=tuning)
        return run

    us, spread = medians_ms([side(t) for t in tunings], reps)
    Wf = W.float()
    res = dict(bench="calibrate", op="reconstruction_by_tuning", n=n, k=k, n_out=r, reps=reps, blocks=(k - r + 127) // 128)
    for t, ms, sp in zip(tunings, us, spread):
        res[f"{t}_ms"] = round(ms, 2)
        res[f"{t}_ms_min_max"] = [round(v, 2) for v in sp]
        res[f"proxy_loss_{t}"] = out[t].proxy_loss
    res["mse_over_mse_torch"] = round(us[1] / us[2], 5)
    res["mse_over_minmax"] = round(us[1] / us[0], 4)
    res["proxy_loss_rtn"] = R.proxy_loss(Wf, R.rtn(Wf, k - r), H)
    print(json.dumps(res), flush=True)


def factor_bench(n, k, r, reps):
    """The factor of the inverse Hessian alone (the three torch calls against hinv_factor on the same damped matrix), then one
    n x k reconstruction with factor = "torch" and "own", the sides alternating."""
    from qeft_amd import _lib
    from qeft_amd.calibrate import HessianAccumulator, gptq_reorder, hinv_factor
    g = torch.Generator(device=DEV).manual_seed(2)
    W = (torch.randn(n, k, generator=g, device=DEV) * 0.02).half()
    acc = HessianAccumulator(k, DEV)
    acc.add_batch(rows(2048, k, 3))
    H = acc.H
    Hd = H.clone()
    Hd.diagonal().add_(0.01 * torch.mean(torch.diag(H)))
    ids = torch.arange(k, device=DEV)
    out = {}

    def three_calls():
        out["torch"] = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(Hd)), upper=True)

    def own():
        out["own"] = hinv_factor(Hd)

    us, spread = medians_ms([three_calls, own], reps)
    diff = ((out["own"] - out["torch"]).norm() / out["torch"].norm()).item()
    del out["torch"], out["own"]

    def side(factor):
        def run():
            out[factor] = gptq_reorder(W, H, ids, r, factor=factor).proxy_loss
        return run

    rec, rspread = medians_ms([side("torch"), side("own")], reps)
    res = dict(bench="calibrate", op="hinv_factor", k=k, n=n, n_out=r, reps=reps, launches=_lib.lib().qeft_hinv_factor_launches(k),
               factor_torch_ms=round(us[0], 3), factor_torch_ms_min_max=[round(v, 3) for v in spread[0]],
               factor_own_ms=round(us[1], 3), factor_own_ms_min_max=[round(v, 3) for v in spread[1]],
               factor_own_over_torch=round(us[1] / us[0], 4), own_useful_tflops=round(2.0 / 3.0 * k ** 3 / (us[1] * 1e-3) / 1e12, 2),
               factor_own_vs_torch_frobenius=diff,
               reconstruction_torch_ms=round(rec[0], 2), reconstruction_torch_ms_min_max=[round(v, 2) for v in rspread[0]],
               reconstruction_own_ms=round(rec[1], 2), reconstruction_own_ms_min_max=[round(v, 2) for v in rspread[1]],
               reconstruction_own_over_torch=round(rec[1] / rec[0], 4), proxy_loss_torch=out["torch"], proxy_loss_own=out["own"])
    print(json.dumps(res), flush=True)


def pack_bench(n, k, r, reps, inner):
    """The packing step: the whole per-linear calibration with the host pack and with the device pack, then the launch alone."""
    from qeft_amd import _lib
    from qeft_amd.calibrate import HessianAccumulator, calibrate_linear
    g = torch.Generator(device=DEV).manual_seed(2)
    lin = torch.nn.Linear(k, n, bias=False).half().to(DEV)
    lin.weight.data = (torch.randn(n, k, generator=g, device=DEV) * 0.02).half()
    acc = HessianAccumulator(k, DEV)
    acc.add_batch(rows(2048, k, 3))
    ids = torch.arange(k - r, k, device=DEV, dtype=torch.int32)
    out = {}

    def side(pack):
        def run():
            out[pack] = calibrate_linear(lin, acc.H, r, "q_proj", outidx=ids, factor="own", pack=pack)
        return run

    e2e, spread = medians_ms([side("host"), side("device")], reps)
    sd_h, sd_d = out["host"][0].state_dict(), out["device"][0].state_dict()
    same = list(sd_h) == list(sd_d) and all(torch.equal(sd_h[key], sd_d[key]) for key in sd_h)
    W, scale, zero = out["device"][1].weight, out["device"][1].scale_group.contiguous(), out["device"][1].zero_group.contiguous()
    del out, sd_h, sd_d
    copies = [W] + [W.clone() for _ in range(7)]
    q = torch.empty(n // 4, k, dtype=torch.int16, device=DEV)
    s16, z16 = (torch.empty(k // 128, n, dtype=torch.float16, device=DEV) for _ in range(2))
    s32, z32 = torch.empty_like(scale), torch.empty_like(zero)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def window(find, n_w):
        def run():
            for i in range(inner):
                w = copies[i % n_w]
                _lib.check(lib.qeft_quant_pack(w.data_ptr(), k, None, None if find else scale.data_ptr(), None if find else zero.data_ptr(),
                                               q.data_ptr(), s16.data_ptr(), z16.data_ptr(), s32.data_ptr() if find else None,
                                               z32.data_ptr() if find else None, n, k, r, 4, 128, st))
        return run

    names = ("given_one_matrix", "given_eight_matrices", "find_one_matrix", "find_eight_matrices")
    ks, kspread = medians_ms([window(False, 1), window(False, 8), window(True, 1), window(True, 8)], reps)
    nbytes = 2.0 * n * k + n * k / 2 + 12.0 * n * k / 128
    res = dict(bench="calibrate", op="quant_pack", n=n, k=k, n_out=r, bits=4, reps=reps, inner=inner,
               calibrate_linear_host_pack_ms=round(e2e[0], 2), calibrate_linear_host_pack_ms_min_max=[round(v, 2) for v in spread[0]],
               calibrate_linear_device_pack_ms=round(e2e[1], 2), calibrate_linear_device_pack_ms_min_max=[round(v, 2) for v in spread[1]],
               device_over_host=round(e2e[1] / e2e[0], 4), same_state_dict=same, algorithmic_bytes=int(nbytes))
    for name, ms, sp in zip(names, ks, kspread):
        res[f"launch_{name}_us"] = round(ms * 1e3 / inner, 2)
        res[f"launch_{name}_us_min_max"] = [round(v * 1e3 / inner, 2) for v in sp]
        res[f"launch_{name}_share_of_8TBps"] = round(nbytes / (ms * 1e-3 / inner) / 8e12, 4)
    print(json.dumps(res), flush=True)


def loop_bench(n, k, r, reps):
    """The loop alone: gptq_reorder on a given factor with each loop (the factorisation is outside both sides), then the one
    launch of the "rows" side without the torch around it (the gathers, the clones and the fp64 proxy loss)."""
    from qeft_amd import _lib
    from qeft_amd.calibrate import HessianAccumulator, gptq_reorder, hinv_factor
    g = torch.Generator(device=DEV).manual_seed(2)
    W = (torch.randn(n, k, generator=g, device=DEV) * 0.02).half()
    acc = HessianAccumulator(k, DEV)
    acc.add_batch(rows(2048, k, 3))
    H = acc.H
    Hd = H.clone()
    Hd.diagonal().add_(0.01 * torch.mean(torch.diag(H)))
    hinv = hinv_factor(Hd)
    del Hd
    ids = torch.arange(k, device=DEV)
    out = {}

    def side(loop):
        def run():
            out[loop] = gptq_reorder(W, H, ids, r, hinv=hinv, loop=loop)
        return run

    us, spread = medians_ms([side("blocks"), side("rows")], reps)
    a, b = out["blocks"], out["rows"]
    differ = (a.weight != b.weight).float().mean().item()
    W0 = W.float()
    q, sc = torch.empty_like(W0), torch.empty(n, k // 128, device=DEV)
    err, ze = torch.empty(n, k - r, device=DEV), torch.empty_like(sc)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.qeft_gptq_rows(W0.data_ptr(), k, hinv.data_ptr(), k, q.data_ptr(), err.data_ptr(), sc.data_ptr(), ze.data_ptr(),
                                      n, k, k - r, 15, 128, st))

    ls, lspread = medians_ms([launch], reps)
    res = dict(bench="calibrate", op="gptq_loop", n=n, k=k, n_out=r, reps=reps, workgroups=lib.qeft_gptq_rows_blocks(n),
               blocks_ms=round(us[0], 2), blocks_ms_min_max=[round(v, 2) for v in spread[0]],
               rows_ms=round(us[1], 2), rows_ms_min_max=[round(v, 2) for v in spread[1]], rows_over_blocks=round(us[1] / us[0], 4),
               rows_launch_alone_ms=round(ls[0], 3), rows_launch_alone_ms_min_max=[round(v, 3) for v in lspread[0]],
               rows_launch_useful_tflops=round(n * float(k - r) * (k + r) / (ls[0] * 1e-3) / 1e12, 2),
               proxy_loss_blocks=a.proxy_loss, proxy_loss_rows=b.proxy_loss, share_of_fp16_weights_that_differ=differ)
    print(json.dumps(res), flush=True)


def rows_mse_bench(n, k, r, reps):
    """The three routes on one given factor, then the one launch of the fused route without the torch around it."""
    from qeft_amd import _lib
    from qeft_amd.calibrate import HessianAccumulator, gptq_reorder, hinv_factor
    g = torch.Generator(device=DEV).manual_seed(2)
    W = (torch.randn(n, k, generator=g, device=DEV) * 0.02).half()
    acc = HessianAccumulator(k, DEV)
    acc.add_batch(rows(2048, k, 3))
    H = acc.H
    Hd = H.clone()
    Hd.diagonal().add_(0.01 * torch.mean(torch.diag(H)))
    hinv = hinv_factor(Hd)
    del Hd
    ids = torch.arange(k, device=DEV)
    sides = (("blocks_mse", "blocks", "mse"), ("rows_minmax", "rows", "minmax"), ("rows_mse_fused", "rows", "mse_fused"))
    out = {}

    def side(name, loop, tuning):
        def run():
            out[name] = gptq_reorder(W, H, ids, r, hinv=hinv, loop=loop, tuning=tuning).proxy_loss
        return run

    us, spread = medians_ms([side(*s) for s in sides], reps)
    W0 = W.float()
    q, sc = torch.empty_like(W0), torch.empty(n, k // 128, device=DEV)
    err, ze = torch.empty(n, k - r, device=DEV), torch.empty_like(sc)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.qeft_gptq_rows_mse(W0.data_ptr(), k, hinv.data_ptr(), k, q.data_ptr(), err.data_ptr(), sc.data_ptr(),
                                          ze.data_ptr(), n, k, k - r, 15, 128, 40, st))

    ls, lspread = medians_ms([launch], reps)
    res = dict(bench="calibrate", op="gptq_rows_mse", n=n, k=k, n_out=r, bits=4, reps=reps, workgroups=lib.qeft_gptq_rows_blocks(n))
    for (name, _, _), ms, sp in zip(sides, us, spread):
        res[f"{name}_ms"] = round(ms, 2)
        res[f"{name}_ms_min_max"] = [round(v, 2) for v in sp]
        res[f"proxy_loss_{name}"] = out[name]
    res.update(fused_over_blocks_mse=round(us[2] / us[0], 4), fused_over_rows_minmax=round(us[2] / us[1], 4),
               fused_launch_alone_ms=round(ls[0], 3), fused_launch_alone_ms_min_max=[round(v, 3) for v in lspread[0]])
    print(json.dumps(res), flush=True)


def pc_bench(n, k, r, reps, inner):
    """Per-channel grids (group_size=-1): the four routes of gptq_reorder on one given factor, alternating;
    each rows launch alone on preallocated outputs; then qeft_quant_pack_pc in windows of `inner` launches on eight matrices."""
    from qeft_amd import _lib
    from qeft_amd.calibrate import HessianAccumulator, gptq_reorder, hinv_factor
    g = torch.Generator(device=DEV).manual_seed(2)
    W = (torch.randn(n, k, generator=g, device=DEV) * 0.02).half()
    acc = HessianAccumulator(k, DEV)
    acc.add_batch(rows(2048, k, 3))
    H = acc.H
    Hd = H.clone()
    Hd.diagonal().add_(0.01 * torch.mean(torch.diag(H)))
    hinv = hinv_factor(Hd)
    del Hd
    ids = torch.arange(k, device=DEV)
    sides = (("rows_minmax", "rows", "minmax"), ("rows_mse_fused", "rows", "mse_fused"), ("blocks_minmax", "blocks", "minmax"),
             ("blocks_mse", "blocks", "mse"))
    out = {}

    def side(name, loop, tuning):
        def run():
            out[name] = gptq_reorder(W, H, ids, r, group_size=-1, hinv=hinv, loop=loop, tuning=tuning)
        return run

    us, spread = medians_ms([side(*s) for s in sides], reps)
    W0 = W.float()
    q, err = torch.empty_like(W0), torch.empty(n, k - r, device=DEV)
    sc, ze = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    args = (W0.data_ptr(), k, hinv.data_ptr(), k, q.data_ptr(), err.data_ptr(), sc.data_ptr(), ze.data_ptr(), n, k, k - r, 15)
    ls, lspread = medians_ms([lambda: _lib.check(lib.qeft_gptq_rows_pc(*args, st)),
                              lambda: _lib.check(lib.qeft_gptq_rows_pc_mse(*args, 40, st))], reps)
    res = dict(bench="calibrate", op="per_channel", n=n, k=k, n_out=r, bits=4, reps=reps, inner=inner)
    for (name, _, _), ms, sp in zip(sides, us, spread):
        res[f"{name}_ms"] = round(ms, 2)
        res[f"{name}_ms_min_max"] = [round(v, 2) for v in sp]
        res[f"proxy_loss_{name}"] = out[name].proxy_loss
    for name, ms, sp in zip(("rows_pc", "rows_pc_mse"), ls, lspread):
        res[f"{name}_launch_alone_ms"] = round(ms, 3)
        res[f"{name}_launch_alone_ms_min_max"] = [round(v, 3) for v in sp]
    Wq, scale, zero = out["rows_minmax"].weight, out["rows_minmax"].scale_group.contiguous(), out["rows_minmax"].zero_group.contiguous()
    del out
    copies = [Wq] + [Wq.clone() for _ in range(7)]
    qw = torch.empty(n // 4, k, dtype=torch.int16, device=DEV)
    s16, z16 = (torch.empty(1, n, dtype=torch.float16, device=DEV) for _ in range(2))
    s32, z32 = torch.empty_like(scale), torch.empty_like(zero)

    def window(find):
        def run():
            for i in range(inner):
                _lib.check(lib.qeft_quant_pack_pc(copies[i % 8].data_ptr(), k, None, None if find else scale.data_ptr(),
                                                  None if find else zero.data_ptr(), qw.data_ptr(), s16.data_ptr(), z16.data_ptr(),
                                                  s32.data_ptr() if find else None, z32.data_ptr() if find else None, n, k, r, 4, st))
        return run

    ks, kspread = medians_ms([window(False), window(True)], reps)
    for name, ms, sp in zip(("given", "find"), ks, kspread):
        res[f"quant_pack_pc_{name}_us"] = round(ms * 1e3 / inner, 2)
        res[f"quant_pack_pc_{name}_us_min_max"] = [round(v * 1e3 / inner, 2) for v in sp]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--only-add-batch", action="store_true")
    ap.add_argument("--only-mse", action="store_true", help="the MSE search parts alone (profiles/calib_mse_bench.json.log)")
    ap.add_argument("--only-factor", action="store_true", help="the inverse-Hessian factor alone (profiles/calib_factor_bench.json.log)")
    ap.add_argument("--only-pack", action="store_true", help="the packing step alone (profiles/quant_pack_bench.json.log)")
    ap.add_argument("--only-loop", action="store_true", help="the error-feedback loop alone (profiles/calib_rows_bench.json.log)")
    ap.add_argument("--only-rows-mse", action="store_true", help="the MSE search inside the launch (profiles/calib_rows_mse_bench.json.log)")
    ap.add_argument("--only-pc", action="store_true", help="per-channel grids, group_size=-1 (profiles/calib_pc_bench.json.log)")
    a = ap.parse_args()
    print(json.dumps(dict(bench="calibrate", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    if a.only_pc:
        for n, k in ([(72, 384)] if a.small else [(4096, 4096), (11008, 4096), (4096, 11008)]):
            with limit(300):
                pc_bench(n - n % 16, k, 128, a.reps, 8 if a.small else 2000)
        sys.exit(0)
    if a.only_rows_mse:
        for n, k in ([(72, 384)] if a.small else [(4096, 4096), (11008, 4096), (4096, 11008)]):
            with limit(300):
                rows_mse_bench(n, k, 128, a.reps)
        sys.exit(0)
    if a.only_loop:
        for n, k in ([(72, 384)] if a.small else [(4096, 4096), (11008, 4096), (4096, 11008)]):
            with limit(300):
                loop_bench(n, k, 128, a.reps)
        sys.exit(0)
    if a.only_pack:
        for n, k in ([(64, 384)] if a.small else [(4096, 4096), (11008, 4096), (4096, 11008)]):
            with limit(300):
                pack_bench(n, k, 128, a.reps, 8 if a.small else 2000)
        sys.exit(0)
    if a.only_factor:
        for n, k in ([(64, 384)] if a.small else [(4096, 4096), (4096, 11008)]):
            with limit(400):
                factor_bench(n, k, 128, a.reps)
        sys.exit(0)
    if a.only_mse:
        for n, g in ([(67, 129)] if a.small else [(4096, 128), (11008, 128), (4096, 4096)]):
            with limit(240):
                mse_search_bench(n, g, a.reps)
        with limit(400):
            mse_recon_bench(*((64, 384) if a.small else (4096, 4096)), 128, a.reps)
        sys.exit(0)
    for t, k, inner in ([(128, 256, 8)] if a.small else [(2048, 4096, 1000), (2048, 11008, 200)]):
        with limit(240):
            add_batch_bench(t, k, a.reps, inner)
    for n, k in ([] if a.only_add_batch else [(64, 384)] if a.small else [(4096, 4096), (11008, 4096), (4096, 11008)]):
        with limit(400):
            recon_bench(n, k, 128, a.reps)
