"""The compile-time-K instances of the v3 decode GEMV (csrc/gemv_v3.h: KCT; csrc/gemv_v3_dispatch.h: V3_CTK) against the
run-time-K instances they shadow: the same operands, once on each, must give the same bits, and both must agree with float64.

The instances exist for the (waves, ring, row sets, mode, K) of the decode engine's Llama-2 launches, which are large; the
smallest shapes that reach them need the lab overrides of the plan, and those -- like QEFT_GEMV_CTK=0, the switch under test --
are read once per process.  So every (overrides, switch) pair is one child process, all of them started together by one fixture;
the tests compare what the children left.  Each child runs with PYTORCH_NO_CUDA_MEMORY_CACHING=1: every operand and every output
is its own allocation, so a staging piece or a ring load that leaves its operand leaves its mapping (tests/test_gpu_zz_alloc_guard.py).

  geometry                      instance (nw, D, RSC, mode)   shapes (N x K)
  QEFT_GEMV_BLOCKS=2            (8, 6, 3, PLAIN)              96 x 4096: two full blocks;  80 x 4096: one block of three sets, one of two
  QEFT_GEMV_BLOCKS=2, _NW=4     (4, 4, 3, PAIR)               the same two
  (none)                        (8, 2, 1, PLAIN)              16 x 4096
  (none)                        (12, 2, 1, PLAIN)             32 x 11008: two blocks
Outlier step on throughout.  Forms: PLAIN with ssq_in (300 partial sums: both 256-float pieces), PLAIN with residual + gamma_out +
ssq_out, and PAIR (with ssq_in, as the engine launches gate|up).

Bounds, as tests/test_gpu_gemv_v3_tiers.py has them for these forms, against float64 on the unrounded weights: a consumer of
ssq_in 2e-3 (x = fp16(v * gamma) carries one more rounding than the chain), PAIR 2e-3, the residual form REL_TOL with
ynorm == fp16(y32 * gamma) and sum(ssq_out) within 1e-4 of sum(y32^2)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMETRIES = {
    "rs3": ({"QEFT_GEMV_BLOCKS": "2"}, [(96, 4096), (80, 4096)], ("consumer", "producer"), (8, 6, 3)),
    "pair": ({"QEFT_GEMV_BLOCKS": "2", "QEFT_GEMV_NW": "4"}, [(96, 4096), (80, 4096)], ("pair",), (4, 4, 3)),
    "rs1": ({}, [(16, 4096), (32, 11008)], ("consumer", "producer"), None),
}
RS1_INSTANCE = {4096: (8, 2, 1), 11008: (12, 2, 1)}

CHILD = r'''
import ctypes, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np, torch
from oracle import qeft_oracle as O
from util import REL_TOL, layer_to_torch, rel_err
from qeft_amd import qeft_cuda, _lib
import types
DEV, EPS, R, G = "cuda:0", 1e-5, 128, 128
shapes, forms, want_kct, out_path = %(shapes)r, %(forms)r, %(kct)r, %(out)r
lib = _lib.lib()

def silu_pair(full):
    v = full.reshape(-1, 2, 8)
    return (v[:, 0, :] / (1 + np.exp(-v[:, 0, :])) * v[:, 1, :]).reshape(-1)

def ran():
    p = (ctypes.c_int * 13)()
    assert lib.qeft_gemv_v3_last_plan(p) == 0
    return [p[4], p[5], p[1], p[7], p[0], p[3], lib.qeft_gemv_v3_last_kct()]      # nw, D, RSC, mode, blocks, sets_r, kct

saved = {}
for (n, k) in shapes:
    b = O.make_layer(n, k, R, G, seed=n + k, bias=True)
    w64 = O.dequant_dense(b["qweight"], b["scales"], b["scaled_zeros"], b["oweight"], G, round_fp16=False).astype(np.float64)
    t = layer_to_torch(b, DEV)
    op = types.SimpleNamespace(qweight=t["qweight"], sz_packed=qeft_cuda.pack_scales(t["scales"], t["scaled_zeros"], n, k, G), oweight=t["oweight"],
                               bias=t["bias"], outfeatures=n, infeatures=k, group_size=G, outlierfeatures=R)
    rng = np.random.default_rng(n + k)
    x = O.make_activation(1, k, R, seed=5)
    xt = torch.from_numpy(x[0]).to(DEV)
    wx = (x.astype(np.float64) @ w64.T)[0]
    bias = b["bias"].astype(np.float64)
    ssq = (rng.random(300) * (2.0 * k / 300)).astype(np.float32)             # partial sums of some v^2 with mean(v^2) about 1
    rs = 1.0 / np.sqrt(ssq.astype(np.float64).sum() / k + EPS)
    for form in forms:
        key = "%%s-%%dx%%d" %% (form, n, k)
        if form in ("consumer", "pair"):
            mode = qeft_cuda.V3_PAIR if form == "pair" else qeft_cuda.V3_PLAIN
            y = qeft_cuda.decode_linear(xt, op, mode=mode, ssq_in=torch.from_numpy(ssq).to(DEV), eps=EPS)
            saved[key + "-plan"] = np.array(ran())
            torch.cuda.synchronize()
            ref = wx * rs + bias
            ref = silu_pair(ref) if form == "pair" else ref
            got = y.cpu().numpy()
            assert got.shape == ref.shape and np.isfinite(got).all(), key
            err = rel_err(got, ref)
            print("[ctk] %%s kct %%d: rel_err %%.3e" %% (key, saved[key + "-plan"][6], err))
            assert err < 2e-3, (key, err)
            saved[key + "-y"] = got
        else:
            h0 = rng.standard_normal(n).astype(np.float32)
            gamma = (1 + 0.1 * rng.standard_normal(n)).astype(np.float16)
            gt = torch.from_numpy(gamma).to(DEV)
            y32, ynorm, sq = qeft_cuda.decode_linear(xt, op, residual=torch.from_numpy(h0).to(DEV), gamma_out=gt)
            saved[key + "-plan"] = np.array(ran())
            torch.cuda.synchronize()
            ref = h0.astype(np.float64) + wx + bias
            err = rel_err(y32.cpu().numpy(), ref)
            print("[ctk] %%s kct %%d: rel_err %%.3e" %% (key, saved[key + "-plan"][6], err))
            assert err < REL_TOL, (key, err)
            assert torch.equal(ynorm, (y32 * gt.float()).half()), key
            total = float((y32.double() ** 2).sum())
            assert sq.numel() == saved[key + "-plan"][4] and abs(float(sq.double().sum()) - total) <= 1e-4 * total, key
            saved[key + "-y32"], saved[key + "-ynorm"], saved[key + "-ssq_out"] = y32.cpu().numpy(), ynorm.cpu().numpy(), sq.cpu().numpy()
        assert saved[key + "-plan"][6] == (k if want_kct else 0), (key, saved[key + "-plan"])
np.savez(out_path, **saved)
print("CTK-OK")
'''


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """(geometry, switch) -> the arrays its child saved; the six children run side by side."""
    tmp = tmp_path_factory.mktemp("ctk")
    procs = {}
    for name, (over, shapes, forms, _) in GEOMETRIES.items():
        for ctk in (1, 0):
            env = {k: v for k, v in os.environ.items() if not k.startswith("QEFT_GEMV_")}
            env.update(over, PYTORCH_NO_CUDA_MEMORY_CACHING="1")
            if not ctk:
                env["QEFT_GEMV_CTK"] = "0"
            out = str(tmp / f"{name}-{ctk}.npz")
            src = CHILD % {"root": ROOT, "shapes": shapes, "forms": forms, "kct": ctk, "out": out}
            procs[name, ctk] = (subprocess.Popen([sys.executable, "-c", src], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), out)
    got = {}
    for key, (p, out) in procs.items():
        so, se = p.communicate(timeout=600)
        print(so)
        assert p.returncode == 0 and "CTK-OK" in so, (key, p.returncode, so[-2000:], se[-4000:])
        got[key] = dict(np.load(out))
    return got


CASES = [(g, form, n, k) for g, (_, shapes, forms, _) in GEOMETRIES.items() for (n, k) in shapes for form in forms]


@pytest.mark.parametrize("geom,form,n,k", CASES, ids=[f"{g}-{f}-{n}x{k}" for g, f, n, k in CASES])
def test_compile_time_k_gives_the_run_time_bits(children, geom, form, n, k):
    on, off = children[geom, 1], children[geom, 0]
    key = f"{form}-{n}x{k}"
    nw, d, rsc = GEOMETRIES[geom][3] or RS1_INSTANCE[k]
    nsets = n // 16
    blocks = 2 if geom != "rs1" else nsets
    want = [nw, d, rsc, 1 if form == "pair" else 0, blocks, nsets % blocks]
    assert list(on[key + "-plan"]) == want + [k], "the compile-time-K instance of the launch kind"
    assert list(off[key + "-plan"]) == want + [0], "QEFT_GEMV_CTK=0: the same instance with K at run time"
    outs = ("y",) if form != "producer" else ("y32", "ynorm", "ssq_out")
    for o in outs:
        a, b = on[f"{key}-{o}"], off[f"{key}-{o}"]
        assert a.dtype == b.dtype and a.shape == b.shape and a.size > 0
        assert np.array_equal(a, b), (key, o, int((a != b).sum()))
