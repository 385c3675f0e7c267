"""CPU checks of the training update (csrc/oweight_optim.hip, csrc/oweight_optim.h, qeft_amd/optim.py: OWeightAdamW,
finetune.train_step / warmup_constant_lr): the entries are declared, exported and bound, the Python names
are in qeft_amd.__all__; both launching entries refuse in the documented order -- SHAPE whatever the pointers are, then NULL, then
ALIGN -- before any HIP call; the host-side walk of every address a launch forms finds none outside [0, n) and no chunk visited
twice or never, over the sizes of tests/test_gpu_oweight_optim.py, and answers -1 for what the entries refuse; the grid is the
stated formula; the arena's bookkeeping (offsets, padding, identity, gradients accumulating in place, the replaced-.grad check,
load_state_dict's layout check) on CPU tensors through optim.Arena, which makes no launch; the schedule; and a numpy fp32
restatement of the pinned sequence against fp64 within the bounds the GPU test applies to the kernel.

THE RULE OF THIS FILE (that of tests/test_train_rope_cpu.py).  Tests without the `gpu` mark also run where a GPU is present, so no
test here passes a launching entry a complete set of valid arguments: made-up pointers appear only in calls that a check refuses.
The CPU-only functions (blocks, thread_elems, check_extents), which take no pointer, are the one place for complete geometry.

THE REFERENCE AND THE BOUNDS (shared with the GPU test).  reference_step is fp64 numpy of the documented formulas on the same fp32
inputs and the fp32-rounded hyperparameters; it forms its own norm and coefficient.  With u = 2^-24 (half an fp32 ulp, the
relative error of one correctly rounded operation) and eta = 2^-149 (one fp32 subnormal step, covering a result that underflows),
counting the roundings of the sequence csrc/oweight_optim.h pins:

  norm   x = g * inv carries 2 (inv, the product), x * x doubles that and adds 1: 5; a thread's k - 1 sequential adds; 8 tree
         levels (6 in the wave, 2 across the waves): k + 12 in the sum of squares, all terms positive; the double fold adds
         nothing visible; the square root halves it, the conversion to fp32 adds one rounding, a factor 2 covers that and the
         second order:            |norm - ref| <= dn ref,  dn = 2 ((k + 12) / 2) u
  coef   norm + 1e-6 and the division: dc = dn + 2u (min(1, .) does not widen it); 0 with clipping off (coef is exactly 1)
  gh     inv, g * inv, * coef: eg = 3u + dc
  m'     gh - m (1), c1 = 1 - beta1 (1), the product (1), the final add (1, on |m'| <= |m| + |gh|), and gh's own eg through c1 <= 1:
                                  |m' - ref| <= (7u + dc) (|m| + |gh|) (1 + 2^-10) + 8 eta
  v'     gh * gh (2 eg + 1), c2 = 1 - beta2 (1), the product (1), beta2 * v (1), the final add (1):
                                  |v' - ref| <= (10u + 2 dc) (beta2 v + c2 gh^2) (1 + 2^-10) + 8 eta
  p'     decay = 1 - lr * wd (1), p * decay (1), the final subtraction (1, on |p'|); the update term U = a m' / (sqrt(v') / r + eps)
         carries m's error through a / den, v's through the square root -- ds, the largest move of sqrt over [v' - dv, v' + dv],
         exact rather than first order, so that v' = 0 needs no special case -- and 7 roundings of its own (sqrt, r, the division, + eps,
         m' / den, a, the product), 8 with the second order:
                                  dU = a dm / den + |U| (ds / (sqrt(bc2) den) + 8u)
                                  |p' - ref| <= (u |p'| + 2u |p| + dU) (1 + 2^-10) + 4 eta
Every bound is evaluated per element in fp64 and no element is excluded."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6
P = 1 << 20                       # a 16-byte aligned non-null "pointer": no call below gets as far as using it
CEILING = 2 ** 31 - 2 ** 20
ARENA_SHAPES = [(8, 6), (16, 128), (24, 32), (4, 1)]
U32, ETA, SLACK = 2.0 ** -24, 2.0 ** -149, 1 + 2.0 ** -10


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def chunks_per_thread(lib):
    """U of the geometry: an arena of 64 elements is one iteration, so a thread's share is U chunks of 4."""
    return lib.qeft_oweight_optim_thread_elems(64) // 4


def sweep_sizes(lib):
    """The sizes of the GPU test: one chunk row; less than one block-iteration per block; past the grid cap with a ragged tail."""
    return [64, 3008, 256 * 4 * chunks_per_thread(lib) * 2048 + 64 * 37]


# ---------------------------------------------------------------------------------------------------- the boundary
def test_symbols_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    from qeft_amd import _lib
    p, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    want = {"qeft_oweight_grad_stats": (i, [p, ll, p, p, p]),
            "qeft_oweight_adamw": (i, [p] * 4 + [ll] + [p] * 3 + [f] * 8 + [i, i, p]),
            "qeft_oweight_optim_blocks": (i, [ll]),
            "qeft_oweight_optim_thread_elems": (ll, [ll]),
            "qeft_oweight_optim_check_extents": (ll, [ll]),
            "qeft_oweight_optim_lab": (i, [i, i])}
    for name, (restype, argtypes) in want.items():
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/qeft_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == argtypes and _lib.RESTYPES[name] is restype, name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    import qeft_amd
    from qeft_amd import build
    for name in ("OWeightAdamW", "train_step", "warmup_constant_lr"):
        assert name in qeft_amd.__all__ and callable(getattr(qeft_amd, name)), name
    assert "oweight_optim.hip" in build.SOURCES and "oweight_optim.h" in build.HEADERS
    assert lib.qeft_abi_version() == 1


STATS_PTRS = ("g", "state_in", "partials")
ADAMW_PTRS = ("p", "g", "m", "v", "state_in", "state_out", "partials")
BAD_N = [0, -64, 63, 100, 64 * 5 + 32, CEILING + 64, 2 ** 31, 2 ** 40]
BAD_HYPER = [dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=1.5), dict(beta2=1.0), dict(beta2=-1e-3), dict(eps=0.0), dict(eps=-1e-8),
             dict(growth_factor=0.0), dict(growth_factor=-2.0), dict(backoff_factor=0.0), dict(backoff_factor=-0.5), dict(lr=-1e-4),
             dict(weight_decay=-0.1), dict(max_norm=-0.3), dict(growth_interval=0), dict(dynamic=2), dict(dynamic=-1),
             dict(beta1=float("nan")), dict(eps=float("nan")), dict(lr=float("nan"))]


def _stats(lib, g=P, state_in=P, partials=P, n=3008):
    return lib.qeft_oweight_grad_stats(g, n, state_in, partials, None)


def _adamw(lib, p=P, g=P, m=P, v=P, state_in=P, state_out=P + 32, partials=P, n=3008, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8,
           weight_decay=0.0, max_norm=0.3, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, dynamic=1):
    return lib.qeft_oweight_adamw(p, g, m, v, n, state_in, state_out, partials, lr, beta1, beta2, eps, weight_decay, max_norm,
                                  growth_factor, backoff_factor, growth_interval, dynamic, None)


def test_the_entries_refuse_in_order_without_a_gpu(lib):
    """SHAPE whatever the pointers are (all good, all null, all odd), then a null pointer with NULL even when another pointer is
    misaligned, then a misaligned pointer with ALIGN.  No call has every argument in order (the rule of this file)."""
    for call, ptrs, bads in ((lambda **kw: _stats(lib, **kw), STATS_PTRS, [dict(n=n) for n in BAD_N]),
                             (lambda **kw: _adamw(lib, **kw), ADAMW_PTRS, [dict(n=n) for n in BAD_N] + BAD_HYPER)):
        nul, odd = {q: None for q in ptrs}, {q: 3 for q in ptrs}
        for bad in bads:
            for ptr in ({}, nul, odd):
                assert call(**ptr, **bad) == ERR_SHAPE, (bad, ptr)
        for name in ptrs:
            other = next(q for q in ptrs if q != name)
            assert call(**{name: None}) == ERR_NULL, name
            assert call(**{name: None, other: P + 2}) == ERR_NULL, name            # NULL before ALIGN
            assert call(**{name: P + 8}) == ERR_ALIGN, name
            assert call(**{name: P + 4}, n=64) == ERR_ALIGN, name
        # the limits themselves are taken up to the pointers
        assert call(n=CEILING, g=None) == ERR_NULL and call(n=64, partials=None) == ERR_NULL
    assert _adamw(lib, state_out=P) == ERR_NULL                                     # one record for both: the second is missing
    assert _adamw(lib, beta1=0.0, beta2=0.0, max_norm=0.0, lr=0.0, growth_interval=1, dynamic=0, p=None) == ERR_NULL
    assert lib.qeft_oweight_optim_lab(3, 0) == ERR_SHAPE and lib.qeft_oweight_optim_lab(2, 2) == ERR_SHAPE
    assert lib.qeft_oweight_optim_lab(-1, 0) == ERR_SHAPE


def test_no_address_outside_the_arena(lib):
    ext = lib.qeft_oweight_optim_check_extents
    sizes = sweep_sizes(lib)
    assert sizes[2] > 2048 * 256 * 4 * chunks_per_thread(lib) and sizes[2] % 64 == 0
    for n in sizes + [128, 64 * 33, 256 * 4 * chunks_per_thread(lib), 256 * 4 * chunks_per_thread(lib) + 64, 2944]:
        assert ext(n) == 0, n
    for n in BAD_N:
        assert ext(n) == -1, n
        assert lib.qeft_oweight_optim_blocks(n) == 0 and lib.qeft_oweight_optim_thread_elems(n) == 0, n
    try:                                            # the lab geometries walk clean too, and the functions follow the override
        for u in (1, 2, 4):
            assert lib.qeft_oweight_optim_lab(u, 0) == 0
            assert chunks_per_thread(lib) == u
            for n in (64, 3008, 256 * 4 * u * 2048 + 64 * 37):
                assert ext(n) == 0, (u, n)
    finally:
        assert lib.qeft_oweight_optim_lab(0, 0) == 0


def test_the_grid_is_the_stated_formula(lib):
    blocks, U = lib.qeft_oweight_optim_blocks, chunks_per_thread(lib)
    assert U in (1, 2, 4)
    last = 0
    for n in list(range(64, 64 * 200, 64)) + [64 * 2 ** k for k in range(8, 25)] + [64 * (2 ** k + 1) for k in range(8, 25)] + [CEILING]:
        want = min(-(-(n // 4) // (256 * U)), 2048)
        assert blocks(n) == want, n
        assert 1 <= blocks(n) <= 2048
    for n in sorted(set(list(range(64, 64 * 200, 64)) + [64 * 2 ** k for k in range(8, 25)] + [CEILING])):
        assert blocks(n) >= last, n
        last = blocks(n)
    assert blocks(CEILING) == 2048
    # k of the norm's bound: iterations x U chunks x 4 elements
    for n in sweep_sizes(lib):
        iters = -(-(n // 4) // (blocks(n) * 256 * U))
        assert lib.qeft_oweight_optim_thread_elems(n) == iters * U * 4, n
    assert lib.qeft_oweight_optim_thread_elems(sweep_sizes(lib)[2]) == 2 * U * 4


# ---------------------------------------------------------------------------------------------------- the arena (no launch)
def _cpu_params(seed=0, shapes=ARENA_SHAPES):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g) * 0.02) for s in shapes]


def test_arena_layout_identity_and_gradients():
    import torch
    from qeft_amd import optim
    offsets, n = optim.arena_layout(ARENA_SHAPES)
    assert offsets == [0, 64, 64 + 2048, 64 + 2048 + 768] and n == 2944
    assert all(o % 64 == 0 for o in offsets) and n % 64 == 0
    params = _cpu_params()
    before, ids = [q.detach().clone() for q in params], [id(q) for q in params]
    a = optim.Arena(params)
    assert a.n == 2944 and a.offsets == offsets and a.layout() == {"n": 2944, "shapes": [list(s) for s in ARENA_SHAPES], "offsets": offsets}
    assert [id(q) for q in a.params] == ids and all(isinstance(q, torch.nn.Parameter) and q.requires_grad for q in params)
    used = torch.zeros(n, dtype=torch.bool)
    for q, was, off in zip(params, before, offsets):
        assert torch.equal(q.detach(), was) and q.shape == was.shape
        assert q.data_ptr() == a.p.data_ptr() + 4 * off and q.grad.data_ptr() == a.g.data_ptr() + 4 * off
        assert torch.equal(a.p[off:off + q.numel()].view(q.shape), was)
        used[off:off + q.numel()] = True
    assert used.sum().item() == 48 + 2048 + 768 + 4
    for flat in (a.p, a.g, a.m, a.v):
        assert flat.dtype == torch.float32 and flat.shape == (n,) and not flat[~used].any()
    assert not a.g.any() and not a.m.any() and not a.v.any()
    # a torch backward through the re-homed parameters lands in g, a second one sums there
    w = [torch.randn(q.shape, generator=torch.Generator().manual_seed(5 + i)) for i, q in enumerate(params)]
    for rounds in (1, 2):
        sum((q * q * wi).sum() for q, wi in zip(params, w)).backward()
        a.check_grads()
        for q, wi, off in zip(params, w, offsets):
            assert q.grad.data_ptr() == a.g.data_ptr() + 4 * off
            one = 2 * q.detach() * wi
            assert torch.equal(a.g[off:off + q.numel()].view(q.shape), one if rounds == 1 else one + one)
        assert not a.g[~used].any()
    a.zero_grad()
    assert not a.g.any() and all(q.grad.data_ptr() == a.g.data_ptr() + 4 * off for q, off in zip(params, offsets))
    # a write through the arena is a write to the parameter
    a.p[offsets[1]] = 7.0
    assert params[1][0, 0].item() == 7.0


def test_a_replaced_grad_raises():
    import torch
    from qeft_amd import optim
    params = _cpu_params(1)
    a = optim.Arena(params)
    a.check_grads()
    params[2].grad = None                                             # zero_grad(set_to_none=True) from elsewhere
    with pytest.raises(RuntimeError, match="parameter 2"):
        a.check_grads()
    params[2].grad = torch.zeros_like(params[2])
    with pytest.raises(RuntimeError, match="parameter 2"):
        a.check_grads()
    params[2].grad = a.views(a.g)[2]
    a.check_grads()
    params[0].data = params[0].detach().clone()
    with pytest.raises(RuntimeError, match="parameter 0"):
        a.check_grads()


def test_the_arena_refuses_before_it_touches_anything():
    import torch
    from qeft_amd import optim
    ok = _cpu_params(2)
    bad = {"fp32": torch.nn.Parameter(torch.zeros(8, 8, dtype=torch.float16)),
           "contiguous": torch.nn.Parameter(torch.zeros(8, 16).t()),
           "require grad": torch.nn.Parameter(torch.zeros(8, 8), requires_grad=False)}
    for what, q in bad.items():
        with pytest.raises(ValueError, match=what):
            optim.Arena(ok + [q])
        assert all(p.grad is None for p in ok), what                   # nothing was re-homed
    with pytest.raises(ValueError, match="twice"):
        optim.Arena(ok + [ok[0]])
    with pytest.raises(ValueError, match="no parameters"):
        optim.Arena([])
    assert all(p.grad is None for p in ok)
    assert optim.MAX_ELEMS == CEILING


def test_load_state_dict_refuses_another_layout():
    """OWeightAdamW itself needs a GPU; the layout check of its load_state_dict is Arena.load_moments, which makes no launch."""
    import torch
    from qeft_amd import optim
    a = optim.Arena(_cpu_params(3))
    other = optim.Arena(_cpu_params(3, shapes=ARENA_SHAPES[:3] + [(4, 2)]))
    assert a.layout() != other.layout() and other.n == a.n              # the same length, another shape: still refused
    good = {"m": torch.ones(a.n), "v": torch.ones(a.n), "record": torch.arange(8, dtype=torch.int32), "layout": a.layout()}
    with pytest.raises(ValueError, match="layout"):
        a.load_moments(dict(good, layout=other.layout()))
    with pytest.raises(ValueError, match="layout"):
        a.load_moments({k: v for k, v in good.items() if k != "layout"})
    with pytest.raises(ValueError, match="fp32"):
        a.load_moments(dict(good, m=torch.ones(a.n + 64)))
    with pytest.raises(ValueError, match="fp32"):
        a.load_moments(dict(good, v=torch.ones(a.n, dtype=torch.float64)))
    assert not a.m.any() and not a.v.any()
    a.load_moments(good)
    assert a.m.all() and a.v.all()


def test_oweight_adamw_refuses_cpu_parameters_and_bad_settings():
    from qeft_amd import OWeightAdamW
    params = _cpu_params(4)
    with pytest.raises(RuntimeError, match="GPU"):
        OWeightAdamW(params)
    assert all(p.grad is None for p in params)
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(eps=0.0), dict(weight_decay=-1.0), dict(max_grad_norm=-1.0),
                dict(growth_factor=0.0), dict(backoff_factor=0.0), dict(growth_interval=0), dict(loss_scale="static"),
                dict(loss_scale=0.0), dict(loss_scale=True), dict(init_scale=float("inf"))):
        with pytest.raises(ValueError):
            OWeightAdamW(params, **bad)


def test_warmup_constant_lr():
    from qeft_amd import warmup_constant_lr as lr
    base = 2e-4
    assert lr(0, 100, base) == 0.0                                     # 3 warm-up updates of 100: 0, 1/3, 2/3, then the rate itself
    assert lr(1, 100, base) == base * 1 / 3 and lr(2, 100, base) == base * 2 / 3
    assert lr(3, 100, base) == base and lr(99, 100, base) == base
    assert lr(0, 1000, base, warmup_ratio=0.0) == base                 # no warm-up: constant from the first update
    assert [lr(i, 10, 1.0) for i in range(3)] == [0.0, 1.0, 1.0]       # ceil(0.3) = 1
    assert lr(16, 1875, base) == pytest.approx(base * 16 / 57) and lr(57, 1875, base) == base        # ceil(56.25) = 57
    with pytest.raises(ValueError):
        lr(-1, 10, base)
    with pytest.raises(ValueError):
        lr(0, 0, base)


# ---------------------------------------------------------------------------------------------------- the arithmetic
def hyper(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.3):
    """The hyperparameters as the kernel receives them: rounded to fp32 (ctypes c_float), held as Python floats."""
    r = lambda x: float(np.float32(x))
    return dict(lr=r(lr), beta1=r(betas[0]), beta2=r(betas[1]), eps=r(eps), wd=r(weight_decay), max_norm=r(max_norm))


def _powi(b, t):
    """beta^t by repeated squaring in double, the kernel's loop."""
    r = 1.0
    while t > 0:
        if t & 1:
            r *= b
        b *= b
        t >>= 1
    return r


def pinned_sumsq_partials(g, scale, U, blocks):
    """Launch 1 restated: fp32 partials [blocks], every operation a float32 of its own, a thread's sum in program order
    (iteration, slot, element), the butterfly over the 64 lanes, then (w0 + w1) + (w2 + w3)."""
    f = np.float32
    n = g.size
    chunks = n // 4
    iters = -(-chunks // (blocks * 256 * U))
    inv = f(1.0) / f(scale)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        x = (g.astype(f) * inv).astype(f)
        sq = np.zeros(iters * blocks * U * 256 * 4, dtype=f)
        sq[:n] = (x * x).astype(f)
        sq = sq.reshape(iters, blocks, U, 256, 4)                       # chunk = ((it * blocks + block) * U + s) * 256 + tid
        acc = np.zeros((blocks, 256), dtype=f)
        for it in range(iters):
            for s in range(U):
                for j in range(4):
                    acc = (acc + sq[it, :, s, :, j]).astype(f)
        acc = acc.reshape(blocks, 4, 64)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[:, :, lanes ^ o]).astype(f)
        w = acc[:, :, 0]
        return ((w[:, 0] + w[:, 1]).astype(f) + (w[:, 2] + w[:, 3]).astype(f)).astype(f)


def pinned_step(p, g, m, v, scale, step, H, U, blocks):
    """Both launches restated in numpy: None when the step is skipped, else (p', m', v', norm, coef) with the bits the header
    pins (fp32, one rounding per operation, nothing contracted)."""
    f = np.float32
    total = 0.0
    for part in pinned_sumsq_partials(g, scale, U, blocks):
        total += float(part)
    if not math.isfinite(total):
        return None
    norm = f(math.sqrt(total))
    coef = min(f(1.0), f(H["max_norm"]) / (norm + f(1e-6))) if H["max_norm"] > 0 else f(1.0)
    t = step + 1
    bc1, bc2 = 1.0 - _powi(H["beta1"], t), 1.0 - _powi(H["beta2"], t)
    a, r = f(H["lr"] / bc1), f(math.sqrt(bc2))
    inv = f(1.0) / f(scale)
    decay, c1, c2 = f(1.0) - f(H["lr"]) * f(H["wd"]), f(1.0) - f(H["beta1"]), f(1.0) - f(H["beta2"])
    beta2, eps = f(H["beta2"]), f(H["eps"])
    with np.errstate(under="ignore"):
        x = g * inv
        gh = x * coef
        p1 = p * decay
        d = gh - m
        m1 = m + d * c1
        sq = gh * gh
        v1 = beta2 * v + c2 * sq
        den = np.sqrt(v1) / r + eps
        q = m1 / den
        p2 = p1 - a * q
    for arr in (x, gh, p1, m1, v1, den, q, p2):
        assert arr.dtype == f
    return p2, m1, v1, norm, coef


def reference_step(p, g, m, v, scale, step, H):
    """fp64 of the documented formulas on the same fp32 inputs; its own norm and coefficient."""
    d = np.float64
    p, g, m, v = p.astype(d), g.astype(d), m.astype(d), v.astype(d)
    x = g / float(scale)
    norm = math.sqrt(float(np.sum(x * x)))
    coef = min(1.0, H["max_norm"] / (norm + float(np.float32(1e-6)))) if H["max_norm"] > 0 else 1.0
    gh = x * coef
    t = step + 1
    bc1, bc2 = 1.0 - H["beta1"] ** t, 1.0 - H["beta2"] ** t
    a = H["lr"] / bc1
    p1 = p * (1.0 - H["lr"] * H["wd"])
    m1 = m + (gh - m) * (1.0 - H["beta1"])
    v1 = H["beta2"] * v + (1.0 - H["beta2"]) * gh * gh
    den = np.sqrt(v1) / math.sqrt(bc2) + H["eps"]
    upd = a * m1 / den
    return dict(norm=norm, coef=coef, gh=gh, m=m1, v=v1, den=den, U=upd, p=p1 - upd, a=a, bc2=bc2, p0=p, m0=m, v0=v)


def step_bounds(ref, k, H):
    """(dn, bound_p, bound_m, bound_v) of the module docstring; dn relative, the others per element."""
    u = U32
    dn = 2 * ((k + 12) / 2) * u
    dc = dn + 2 * u if H["max_norm"] > 0 else 0.0
    gh, c2 = np.abs(ref["gh"]), 1.0 - H["beta2"]
    bm = (7 * u + dc) * (np.abs(ref["m0"]) + gh) * SLACK + 8 * ETA
    bv = (10 * u + 2 * dc) * (H["beta2"] * ref["v0"] + c2 * gh * gh) * SLACK + 8 * ETA
    root = np.sqrt(ref["v"])
    ds = np.maximum(np.sqrt(ref["v"] + bv) - root, root - np.sqrt(np.maximum(ref["v"] - bv, 0.0)))
    dU = ref["a"] * bm / ref["den"] + np.abs(ref["U"]) * (ds / (math.sqrt(ref["bc2"]) * ref["den"]) + 8 * u)
    bp = (u * np.abs(ref["p"]) + 2 * u * np.abs(ref["p0"]) + dU) * SLACK + 4 * ETA
    return dn, bp, bm, bv


def check_step(tag, got_p, got_m, got_v, got_norm, p, g, m, v, scale, step, H, k):
    """The per-element check of one applied step against fp64 from the pre-step arrays: prints max(err / bound) for p, m, v and
    the norm, asserts each <= 1, returns them."""
    ref = reference_step(p, g, m, v, scale, step, H)
    dn, bp, bm, bv = step_bounds(ref, k, H)
    d = np.float64
    rp = float(np.max(np.abs(got_p.astype(d) - ref["p"]) / bp))
    rm = float(np.max(np.abs(got_m.astype(d) - ref["m"]) / bm))
    rv = float(np.max(np.abs(got_v.astype(d) - ref["v"]) / bv))
    rn = abs(float(got_norm) - ref["norm"]) / (dn * ref["norm"]) if ref["norm"] > 0 else float(got_norm != 0)
    print(f"[oweight_optim] {tag}: n {p.size} k {k} norm {ref['norm']:.4e} coef {ref['coef']:.4f}  max err/bound  p {rp:.3f}  m {rm:.3f}  "
          f"v {rv:.3f}  norm {rn:.3f}")
    assert rn <= 1, f"{tag}: norm {got_norm} vs {ref['norm']}: {rn:.3f} x the bound"
    assert rp <= 1 and rm <= 1 and rv <= 1, f"{tag}: err / bound p {rp:.3f} m {rm:.3f} v {rv:.3f}"
    return rp, rm, rv, rn


def make_inputs(n, scale, seed, warm=True, U=2, blocks=1):
    """p ~ N(0, 0.02^2), g ~ scale N(0, 1e-3^2) with a few exact zeros and a few values near the fp32 subnormal edge; m and v from
    two warm-up steps of the restated sequence on other gradients (also carrying zeros and tiny values), so neither is zero."""
    rng = np.random.default_rng(seed)
    f = np.float32

    def grad():
        g = (rng.standard_normal(n) * 1e-3 * scale).astype(f)
        idx = rng.permutation(n)[:max(6, n // 200)]
        vals = np.array([0.0, -0.0, 2.0 ** -126, -(2.0 ** -127), 2.0 ** -140, 1.5 * 2.0 ** -120], dtype=f)
        g[idx] = vals[np.arange(idx.size) % vals.size]
        return g
    p = (rng.standard_normal(n) * 0.02).astype(f)
    m, v = np.zeros(n, dtype=f), np.zeros(n, dtype=f)
    if warm:
        H = hyper()
        for s in range(2):
            p, m, v, _, _ = pinned_step(p, grad(), m, v, scale, s, H, U, blocks)
    return p, grad(), m, v


@pytest.mark.parametrize("case", [dict(), dict(max_norm=0.0), dict(max_norm=0.01), dict(weight_decay=0.1), dict(step=999),
                                  dict(scale=1024.0), dict(scale=3.0, betas=(0.3, 0.7), weight_decay=0.1, lr=1e-2)])
def test_the_pinned_sequence_stays_within_the_bounds_of_fp64(lib, case):
    """The numpy fp32 restatement of oweight_optim.h against reference_step, with the bounds the GPU test applies to the kernel:
    the constants are checked here before any GPU sees them."""
    case = dict(case)
    scale, step = case.pop("scale", 65536.0), case.pop("step", 2)
    H = hyper(**case)
    U = chunks_per_thread(lib)
    for n in (64, 3008, 64 * 1200 + 64 * 37):
        blocks = lib.qeft_oweight_optim_blocks(n)
        k = lib.qeft_oweight_optim_thread_elems(n)
        p, g, m, v = make_inputs(n, scale, seed=n % 1000 + step, U=U, blocks=blocks)
        assert m.any() and v.any() and (g == 0).any() and (np.abs(g[g != 0]) < 2.0 ** -119).any()
        out = pinned_step(p, g, m, v, scale, step, H, U, blocks)
        assert out is not None
        p2, m2, v2, norm, coef = out
        check_step(f"numpy {case or 'default'} scale {scale} step {step}", p2, m2, v2, norm, p, g, m, v, scale, step, H, k)
        assert not np.array_equal(p2, p) and not np.array_equal(m2, m)
    # the norm is about 1e-3 sqrt(n): below the default max_norm at these sizes, well above 0.01
    ref = reference_step(p, g, m, v, scale, step, H)
    assert (ref["coef"] < 0.1) if case.get("max_norm") == 0.01 else (ref["coef"] == 1.0)
    # a non-finite gradient anywhere is a skip
    for bad in (np.inf, -np.inf, np.nan):
        for where in (0, n - 1):
            gb = g.copy()
            gb[where] = bad
            assert pinned_step(p, gb, m, v, scale, step, H, U, blocks) is None
    # the update of (0, 0, 0, 0) is 0: padding stays zero
    z = np.zeros(64, dtype=np.float32)
    pz, mz, vz, nz, cz = pinned_step(z, z, z, z, scale, step, H, U, 1)
    assert not pz.any() and not mz.any() and not vz.any() and nz == 0


def test_a_contracted_sequence_would_be_told_apart(lib):
    """What FMA contraction of m' = m + d * c1 would give differs from the pinned bits in a visible share of elements, so the GPU
    test's bit comparison with pinned_step can tell whether the kernel was compiled as pinned."""
    U = chunks_per_thread(lib)
    n = 3008
    p, g, m, v = make_inputs(n, 65536.0, seed=9, U=U, blocks=lib.qeft_oweight_optim_blocks(n))
    H = hyper()
    _, m1, _, _, coef = pinned_step(p, g, m, v, 65536.0, 2, H, U, lib.qeft_oweight_optim_blocks(n))
    f, d = np.float32, np.float64
    gh = (g * (f(1.0) / f(65536.0))) * coef
    dd = gh - m
    fused = (m.astype(d) + dd.astype(d) * d(f(1.0) - f(H["beta1"]))).astype(f)
    share = float((fused != m1).mean())
    print(f"[oweight_optim] an FMA form of m' differs from the pinned one in {share:.3f} of {n} elements")
    assert 0.01 < share < 0.9
