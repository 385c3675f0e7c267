"""fp64 net under the training update (csrc/oweight_optim.hip: variants "oweight_grad_stats_u2" and "oweight_adamw_u2", the
measurement geometries "oweight_grad_stats_u1", "oweight_grad_stats_u4", "oweight_adamw_u1", "oweight_adamw_u4" and their
non-temporal forms "oweight_adamw_u1_nt", "oweight_adamw_u2_nt", "oweight_adamw_u4_nt"), under optim.OWeightAdamW and under
finetune.train_step.

The reference is fp64 numpy of the documented formulas on the same fp32 inputs, forming its own norm and clip coefficient; every
bound is derived by counting the roundings of the sequence csrc/oweight_optim.h pins (tests/test_oweight_optim_cpu.py states the
count: 7u + dc on m', 10u + 2 dc on v', u |p'| + 2u |p| + dU on p', (k + 12) u on the norm, k from the geometry functions), is
evaluated per element in fp64 with no element excluded, and was met by a numpy restatement of the sequence before any GPU saw
it.  On top of the bounds the kernel's p', m', v', norm and coefficient are compared with that restatement bit for bit: the
sequence is pinned, so a kernel compiled with a contracted multiply-add, another summation order or a flushed subnormal shows.

Sizes: n = 64 (one chunk row, most threads idle), 3008 (the four odd tensors of the CPU test and one more: less than one
block-iteration per block), 256 * 4 * U * 2048 + 64 * 37 (past the grid cap: the grid stride and a ragged tail both run).
Every test prints its figures ([oweight_optim] ...)."""
import functools
import os

import numpy as np
import pytest
import torch

from test_oweight_optim_cpu import (ARENA_SHAPES, check_step, chunks_per_thread, hyper, make_inputs, pinned_step,
                                    pinned_sumsq_partials, reference_step)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def _L():
    from qeft_amd import _lib
    return _lib, _lib.lib()


def _shapes(which, U=None):
    """Parameter shapes whose arena has exactly the size asked for, the last element of the arena a live one."""
    U = U or chunks_per_thread(_L()[1])
    return {"row": [(1, 64)],                                                        # 64
            "odd": ARENA_SHAPES + [(1, 64)],                                         # 2944 + 64 = 3008
            "big": [(2048 * U, 1024), (36, 64), (1, 64)]}[which]                     # 256 * 4 * U * 2048 + 64 * 37


def _new(shapes, **kw):
    from qeft_amd import OWeightAdamW
    params = [torch.nn.Parameter(torch.zeros(*s, dtype=F32, device=DEV)) for s in shapes]
    return OWeightAdamW(params, **kw)


def _live(opt):
    """Boolean numpy mask [n] of the elements that belong to a tensor (the rest is padding)."""
    mask = np.zeros(opt.arena.n, dtype=bool)
    for off, shape in zip(opt.arena.offsets, opt.arena.shapes):
        mask[off:off + int(np.prod(shape))] = True
    return mask


def _load(opt, p, g, m, v, step=None):
    """The four arenas from numpy (padding zeroed) and, where given, the record's step."""
    live = _live(opt)
    out = []
    for flat, a in zip((opt.arena.p, opt.arena.g, opt.arena.m, opt.arena.v), (p, g, m, v)):
        a = np.where(live, a, np.float32(0)).astype(np.float32)
        flat.copy_(torch.from_numpy(a))
        out.append(a)
    if step is not None:
        opt._records[opt._cur, 1] = step
    return out


def _read(opt):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in (opt.arena.p, opt.arena.g, opt.arena.m, opt.arena.v))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _H(opt, lr=None):
    return hyper(lr=opt.lr if lr is None else lr, betas=opt.betas, eps=opt.eps, weight_decay=opt.weight_decay, max_norm=opt.max_grad_norm)


def _geometry(n):
    lib = _L()[1]
    return chunks_per_thread(lib), lib.qeft_oweight_optim_blocks(n), lib.qeft_oweight_optim_thread_elems(n)


@functools.lru_cache(maxsize=None)
def _unit_inputs(n, seed, U, blocks):
    return make_inputs(n, 1.0, seed, U=U, blocks=blocks)


def _inputs(n, scale, seed):
    """make_inputs once per (n, seed), shared and left unchanged: g is made at scale 1 and multiplied up (exact for the powers of
    two, one more rounding for the odd scale -- it is data either way)."""
    U, blocks, _ = _geometry(n)
    p, g, m, v = _unit_inputs(n, seed, U, blocks)
    return p, (g * np.float32(scale)).astype(np.float32), m, v


def _one_checked_step(tag, opt, p, g, m, v, scale, step, lr=None, variants=("oweight_grad_stats_u2", "oweight_adamw_u2")):
    """opt.step() on loaded arenas, then everything a finite step owes: the fp64 bounds, the restatement's bits, g untouched, the
    padding zero, the record."""
    _lib, lib = _L()
    U, blocks, k = _geometry(opt.arena.n)
    H = _H(opt, lr)
    before = opt.stats()
    assert before["scale"] == scale and before["step"] == step
    # launch 1 on its own: the partials are the restatement's, bit for bit (NaN-free here), one per block and no more
    parts = torch.full((blocks + 4,), float("nan"), dtype=F32, device=DEV)
    _lib.check(lib.qeft_oweight_grad_stats(opt.arena.g.data_ptr(), opt.arena.n, opt._records[opt._cur].data_ptr(), parts.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _lib.last_variant() == variants[0]
    assert np.array_equal(_bits(parts[:blocks].cpu().numpy()), _bits(pinned_sumsq_partials(g, scale, U, blocks)))
    assert torch.isnan(parts[blocks:]).all()
    opt.step(lr)
    p2, g2, m2, v2 = _read(opt)
    assert _lib.last_variant() == variants[1]
    after = opt.stats()
    rp, rm, rv, rn = check_step(tag, p2, m2, v2, after["grad_norm"], p, g, m, v, scale, step, H, k)
    want = pinned_step(p, g, m, v, scale, step, H, U, blocks)
    assert want is not None
    differ = [int((_bits(a) != _bits(b)).sum()) for a, b in zip((p2, m2, v2), want[:3])]
    print(f"[oweight_optim] {tag}: elements whose bits differ from the numpy restatement  p {differ[0]}  m {differ[1]}  v {differ[2]}; "
          f"norm {after['grad_norm']!r} vs {float(want[3])!r}, coef {after['clip_coef']!r} vs {float(want[4])!r}")
    assert np.float32(after["grad_norm"]) == want[3] and np.float32(after["clip_coef"]) == want[4]
    assert differ == [0, 0, 0]
    assert np.array_equal(_bits(g2), _bits(g)), "step() wrote to g"
    live = _live(opt)
    for a in (p2, m2, v2):
        assert not a[~live].any(), "padding no longer zero"
    assert after["step"] == step + 1 and after["skipped_last"] == 0 and after["n_skipped"] == before["n_skipped"]
    return after, (p2, m2, v2)


def _differs_from_torch_adamw(got, p, g, m, v, scale, step, H):
    """Information, not a requirement (bit parity with torch.optim.AdamW is not a goal): how many elements of (p, m, v) differ
    from one torch step on the same arrays with the same state.  For a step that does not clip."""
    tp = torch.nn.Parameter(torch.from_numpy(p).to(DEV))
    tp.grad = torch.from_numpy(g).to(DEV) / scale
    opt = torch.optim.AdamW([tp], lr=H["lr"], betas=(H["beta1"], H["beta2"]), eps=H["eps"], weight_decay=H["wd"], foreach=False)
    opt.state[tp] = dict(step=torch.tensor(float(step)), exp_avg=torch.from_numpy(m).to(DEV), exp_avg_sq=torch.from_numpy(v).to(DEV))
    opt.step()
    theirs = (tp.detach().cpu().numpy(), opt.state[tp]["exp_avg"].cpu().numpy(), opt.state[tp]["exp_avg_sq"].cpu().numpy())
    return [int((_bits(a) != _bits(b)).sum()) for a, b in zip(got, theirs)]


CASES = {"default": dict(),                                                  # dynamic scale 65536; clipped where the norm tops 0.3
         "clip-hard": dict(max_grad_norm=0.01),                             # the norm is above max_grad_norm at every size but 64
         "clip-off": dict(max_grad_norm=0.0),
         "decay": dict(weight_decay=0.1),
         "no-scale": dict(loss_scale=None),
         "scale-1024": dict(loss_scale=1024.0),
         "step-1000": dict(step=999),
         "odd-hyper": dict(loss_scale=3.0, betas=(0.3, 0.7), weight_decay=0.1, lr=1e-2, max_grad_norm=0.01)}


# every case on the two small arenas; on the large one the four that differ in more than a scalar the small ones already cover
RUNS = [(which, case) for which in ("row", "odd") for case in sorted(CASES)] + \
       [("big", case) for case in ("default", "clip-off", "step-1000", "odd-hyper")]


@pytest.mark.parametrize("which,case", RUNS)
def test_a_step_against_fp64(which, case):
    kw = dict(CASES[case])
    step = kw.pop("step", 0)
    opt = _new(_shapes(which), **kw)
    scale = opt.stats()["scale"]
    assert scale == {"no-scale": 1.0, "scale-1024": 1024.0, "odd-hyper": 3.0}.get(case, 65536.0)
    U, blocks, k = _geometry(opt.arena.n)
    p, g, m, v = _load(opt, *_inputs(opt.arena.n, scale, seed=1), step=step)
    assert m.any() and v.any() and (g == 0).any() and (np.abs(g[g != 0]) < 2.0 ** -100).any()
    after, got = _one_checked_step(f"{which} {case}", opt, p, g, m, v, scale, step)
    assert after["good_steps"] == 1 and after["scale"] == scale
    if case == "clip-off":
        d = _differs_from_torch_adamw(got, p, g, m, v, scale, step, _H(opt))
        print(f"[oweight_optim] {which} {case}: of {p.size} elements, bits that differ from one torch.optim.AdamW step  p {d[0]}  m {d[1]}  v {d[2]}")
    ref = reference_step(p, g, m, v, scale, step, _H(opt))
    if case == "clip-hard" and which != "row":
        assert ref["coef"] < 1 and after["clip_coef"] < 1
    if case == "clip-off" or (case == "default" and which != "big"):
        assert after["clip_coef"] == 1.0
    if case == "default" and which == "big":
        assert after["grad_norm"] > 0.3 and after["clip_coef"] < 1


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_skips_the_step(bad):
    """inf / NaN in element 0 and in the last element of the ragged tail of the large arena, dynamic and static scale: p, m, v keep
    their bits, step stays, skipped_last = 1, n_skipped counts, the scale is halved when dynamic and kept when static; the next
    finite step updates (checked against fp64 at the scale the record then holds)."""
    for where, kw in ((-1, dict()), (0, dict()), (-1, dict(loss_scale=1024.0)), (0, dict(loss_scale=None))):
        opt = _new(_shapes("big"), **kw)
        dynamic, scale = opt.dynamic, opt.stats()["scale"]
        p, g, m, v = _load(opt, *_inputs(opt.arena.n, scale, seed=1), step=5)
        good = g[where]
        opt.arena.g[where] = bad
        opt.step()
        p2, g2, m2, v2 = _read(opt)
        rec = opt.stats()
        tag = f"{'nan' if bad != bad else 'inf'} at {where} {'dynamic' if dynamic else 'static'}"
        print(f"[oweight_optim] skip {tag}: {rec}")
        assert np.array_equal(_bits(p2), _bits(p)) and np.array_equal(_bits(m2), _bits(m)) and np.array_equal(_bits(v2), _bits(v)), tag
        assert rec["step"] == 5 and rec["skipped_last"] == 1 and rec["n_skipped"] == 1 and rec["good_steps"] == 0, tag
        assert rec["scale"] == (scale * 0.5 if dynamic else scale), tag
        opt.arena.g[where] = float(good)
        after, _ = _one_checked_step(f"after the skip, {tag}", opt, p, g, m, v, rec["scale"], 5)
        assert after["n_skipped"] == 1 and after["good_steps"] == 1


def test_the_scale_grows_after_growth_interval_good_steps():
    opt = _new(_shapes("odd"), growth_interval=2)
    p, g, m, v = _load(opt, *_inputs(opt.arena.n, 65536.0, seed=1))
    seen = []
    for i in range(5):
        opt.step()
        seen.append(opt.stats())
    print("[oweight_optim] growth: " + "  ".join(f"step {s['step']} scale {s['scale']:g} good {s['good_steps']}" for s in seen))
    assert [s["scale"] for s in seen] == [65536.0, 131072.0, 131072.0, 262144.0, 262144.0]
    assert [s["good_steps"] for s in seen] == [1, 0, 1, 0, 1] and [s["step"] for s in seen] == [1, 2, 3, 4, 5]
    static = _new(_shapes("odd"), growth_interval=2, loss_scale=1024.0)
    _load(static, p, g, m, v)
    for i in range(3):
        static.step()
    assert static.stats()["scale"] == 1024.0 and static.stats()["good_steps"] == 3
    assert float(static.scale.item()) == 1024.0 and static.scale.dim() == 0 and static.scale.is_cuda


def test_two_optimisers_agree_bit_for_bit_and_a_state_dict_continues():
    """Three steps on the large arena from the same arrays: p, m, v and the records bit-identical.  And state_dict -> a new
    optimiser -> load_state_dict -> one step equals stepping on."""
    a, b = _new(_shapes("big"), weight_decay=0.1, growth_interval=2), _new(_shapes("big"), weight_decay=0.1, growth_interval=2)
    data = _inputs(a.arena.n, 65536.0, seed=1)
    _load(a, *data, step=7)
    _load(b, *data, step=7)
    for i in range(3):
        a.step()
        b.step()
    ra, rb = _read(a), _read(b)
    for x, y in zip(ra, rb):
        assert np.array_equal(_bits(x), _bits(y))
    assert torch.equal(a._records[a._cur].cpu(), b._records[b._cur].cpu()) and a.stats()["step"] == 10
    sd = a.state_dict()
    assert sd["m"].device.type == "cpu" and sd["record"].shape == (8,) and sd["layout"]["n"] == a.arena.n
    c = _new(_shapes("big"), weight_decay=0.1, growth_interval=2)
    _load(c, ra[0], ra[1], np.zeros_like(ra[0]), np.zeros_like(ra[0]))
    c.load_state_dict(sd)
    assert c.stats() == a.stats()
    a.step()
    c.step()
    for x, y in zip(_read(a), _read(c)):
        assert np.array_equal(_bits(x), _bits(y))
    assert c.stats() == a.stats()
    other = _new(_shapes("odd"))
    with pytest.raises(ValueError, match="layout"):
        other.load_state_dict(sd)


def test_zero_grad_scale_loss_and_the_replaced_grad():
    opt = _new(_shapes("odd"), loss_scale=1024.0)
    ptrs = [q.grad.data_ptr() for q in opt.params]
    loss = sum((q * q).sum() for q in opt.params) + opt.params[0].sum()
    scaled = opt.scale_loss(loss, accum=4)
    assert scaled.is_cuda and scaled.dim() == 0
    scaled.backward()
    opt.scale_loss(sum(q.sum() for q in opt.params), accum=4).backward()
    assert [q.grad.data_ptr() for q in opt.params] == ptrs
    assert torch.equal(opt.params[0].grad, torch.full_like(opt.params[0], 512.0))          # 1024 / 4 from each backward
    assert torch.equal(opt.params[1].grad, torch.full_like(opt.params[1], 256.0))
    opt.step()
    opt.zero_grad()
    assert not opt.arena.g.any() and [q.grad.data_ptr() for q in opt.params] == ptrs
    opt.params[1].grad = None
    with pytest.raises(RuntimeError, match="parameter 1"):
        opt.step()
    assert opt.stats()["step"] == 1                                             # refused before any launch


@pytest.mark.parametrize("u", [1, 2, 4])
def test_the_measurement_geometries_compute_the_same_update(u):
    """qeft_oweight_optim_lab: 1, 2 or 4 chunks per thread per iteration, g loaded non-temporally or not.  Each geometry past its own
    grid cap meets the fp64 bounds and its own restatement's bits; the non-temporal form gives the bits of the plain one."""
    _lib, lib = _L()
    try:
        assert lib.qeft_oweight_optim_lab(u, 0) == 0
        assert chunks_per_thread(lib) == u
        opt = _new(_shapes("big", U=u), weight_decay=0.1)
        assert opt.arena.n == 256 * 4 * u * 2048 + 64 * 37 and opt._blocks == 2048
        p, g, m, v = _load(opt, *_inputs(opt.arena.n, 65536.0, seed=1), step=3)
        after, plain = _one_checked_step(f"lab u {u}", opt, p, g, m, v, 65536.0, 3,
                                         variants=(f"oweight_grad_stats_u{u}", f"oweight_adamw_u{u}"))
        assert lib.qeft_oweight_optim_lab(u, 1) == 0
        nt = _new(_shapes("big", U=u), weight_decay=0.1)
        _load(nt, p, g, m, v, step=3)
        nt.step()
        out = _read(nt)
        assert _lib.last_variant() == f"oweight_adamw_u{u}_nt"
        for x, y in zip(plain, (out[0], out[2], out[3])):
            assert np.array_equal(_bits(x), _bits(y))
        assert np.array_equal(_bits(out[1]), _bits(g)) and nt.stats() == after
    finally:
        assert lib.qeft_oweight_optim_lab(0, 0) == 0


# ---------------------------------------------------------------------------------------------------- end to end
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEQ_LENS = (30, 23, 17, 9)


def _model(which):
    from qeft_amd.llama import QuantLlama, tiny_shape
    if which == "tiny":
        return QuantLlama(tiny_shape(max_seq=64), DEV, seed=6), dict(attn="own", glue="fused", rope="fused")
    return QuantLlama.from_packed(os.path.join(GOLDEN, "ref_ckpt_llama2l.pth"), device=DEV, max_seq=64), dict()


@pytest.mark.parametrize("which", ["tiny", "llama2l"])
def test_train_step_end_to_end(which, tmp_path):
    """begin, OWeightAdamW(growth_interval=2), four train_step calls over two packed micro-batches of unequal sequences.  Every step
    is checked per element against fp64 from the arenas before it and the g it saw (a skipped one must have changed nothing); the
    loss on the same batches falls, and it also falls when the parameters are the fp64 AdamW trajectory over the same gradients;
    after end() the inference copies are those of the arena and save_finetuned writes the parameters' own shapes."""
    from qeft_amd import OWeightAdamW, causal_lm_loss, checkpoint, finetune, train_step
    from qeft_amd.llama import layer_linears, prefill
    from qeft_amd.qlinear import pack_oweight
    model, route = _model(which)
    gen = torch.Generator().manual_seed(12)
    seqs = [torch.randint(0, model.shape.vocab, (n,), generator=gen) for n in SEQ_LENS]
    batches = finetune.pack_sequences(seqs, budget=48)
    assert [b[2] for b in batches] == [[30, 17], [23, 9]]
    params = finetune.begin(model)
    ids = [id(q) for q in params]
    opt = OWeightAdamW(params, growth_interval=2)
    assert [id(ql.oweight) for L in model.model.layers for _, ql in layer_linears(L) if ql.outlierfeatures > 0] == ids
    U, blocks, k = _geometry(opt.arena.n)
    H = _H(opt)

    def mean_loss():
        with torch.no_grad():
            return sum(causal_lm_loss(model, t, l, seq_lens=s, **route).item() for t, l, s in batches) / len(batches)
    loss0 = mean_loss()
    p64 = opt.arena.p.cpu().numpy().astype(np.float64)
    m64, v64, t64 = np.zeros_like(p64), np.zeros_like(p64), 0
    applied, worst = 0, [0.0, 0.0, 0.0]
    for i in range(4):
        p, _, m, v = _read(opt)
        before = opt.stats()
        loss = train_step(model, opt, batches, **route)
        assert loss.is_cuda and loss.dim() == 0 and loss.dtype == F32
        p2, g, m2, v2 = _read(opt)
        after = opt.stats()
        assert not g[~_live(opt)].any()
        if after["skipped_last"]:
            assert not np.isfinite(g).all(), "a step was skipped over a finite gradient"
            assert np.array_equal(_bits(p2), _bits(p)) and np.array_equal(_bits(m2), _bits(m)) and np.array_equal(_bits(v2), _bits(v))
            assert after["step"] == before["step"] and after["scale"] == before["scale"] * 0.5
            print(f"[oweight_optim] {which} step {i}: loss {loss.item():.6f} skipped, scale {before['scale']:g} -> {after['scale']:g}")
            continue
        rp, rm, rv, rn = check_step(f"{which} step {i} (loss {loss.item():.6f}, scale {before['scale']:g})", p2, m2, v2, after["grad_norm"],
                                    p, g, m, v, before["scale"], before["step"], H, k)
        worst = [max(a, b) for a, b in zip(worst, (rp, rm, rv))]
        applied += 1
        ref = reference_step(p64, g, m64, v64, before["scale"], t64, H)                # the fp64 trajectory over the same gradients
        p64, m64, v64, t64 = ref["p"], ref["m"], ref["v"], t64 + 1
    print(f"[oweight_optim] {which}: {applied} of 4 steps applied, max err/bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}; "
          f"record {opt.stats()}")
    assert applied >= 2 and opt.stats()["step"] == applied
    loss1 = mean_loss()
    own = opt.arena.p.clone()
    opt.arena.p.copy_(torch.from_numpy(p64.astype(np.float32)))
    loss64 = mean_loss()
    opt.arena.p.copy_(own)
    print(f"[oweight_optim] {which}: loss {loss0:.6f} -> {loss1:.6f} (own), -> {loss64:.6f} (fp64 AdamW on the same gradients)")
    assert loss64 < loss0 and loss1 < loss0
    # back to inference: the copies the decode GEMV reads are those of the arena, the parameters kept their identity
    finetune.end(model)
    linears = [ql for L in model.model.layers for _, ql in layer_linears(L) if ql.outlierfeatures > 0]
    assert [id(ql.oweight) for ql in linears] == ids
    for ql, view in zip(linears, opt.arena.views(opt.arena.p)):
        assert ql.oweight.data_ptr() == view.data_ptr() and torch.equal(ql.oweight.detach(), view)
        assert torch.equal(ql.oweight_interleaved, pack_oweight(view.half()))
    tokens = seqs[0].to(DEV)
    with torch.no_grad():
        logits = prefill(model, tokens)
    dense = model.forward_dense_reference(tokens)                       # the arena's values, dequantised as fp16
    assert (logits.float() - dense).abs().max().item() / dense.abs().max().item() < 5e-3
    saved = torch.load(checkpoint.save_finetuned(model, "base", str(tmp_path / "ft")))["oweight_state_dict"]
    assert [tuple(t.shape) for t in saved.values()] == opt.arena.shapes and all(t.dtype == torch.float16 for t in saved.values())
    for t, view in zip(saved.values(), opt.arena.views(opt.arena.p)):
        assert torch.equal(t, view.half().cpu())
