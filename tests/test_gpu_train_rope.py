"""The training rotary (qeft_rope_qk in csrc/train_glue.hip) through the C ABI, through qeft_amd.glue.rope_qk and through
finetune.causal_lm_loss(rope="fused")  (DESIGN.md section 4.17).

Every operand of every launch is a view inside a buffer of NaN with at least 64 elements of margin on either side (NaN gaps
between padded rows; the un-rotated heads of a fused q|k|v buffer carry data, and must be bit-identical after the call); outputs
start as NaN, and after a launch everything around the views is still NaN.

  fp64 net.   Both directions against rowwise_ref.rope_rows formed from the kernel's own inputs (the inverse: with the negated sin
              table), element-wise |got - ref| <= ulp16(ref) + 2^-22 (|a c| + |b s|): B1 of the rotary (DESIGN.md section 4.4b,
              tests/test_gpu_rowwise.py), the terms from rowwise_ref.rope_rows_terms.  No value is excluded.
  torch bits. The forward equals finetune._rope on q and on k, .grad through rope_qk equals .grad through _rope, bit for bit (+-65504
              and fp16 subnormals in the data: inf equals inf, and the +0 autograd's sum of the two half-slice gradients leaves
              where the transpose alone would leave -0).
  independence, autograd, the model (section 4.14's criterion; bit equality with rope="torch"), launch counts.
Every case prints its largest error / bound ([train_rope] ...); DESIGN.md section 4.17 records them."""
import itertools

import numpy as np
import pytest
import torch

import rowwise_ref
from test_gpu_train_glue import LOSS_SCALE, _trainable

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
MARGIN = 64
T_LENS = [1, 5, 67]
BATCHES = [1, 3]
# (n_heads, n_kv_heads, placement): dense; "fused": views of one q|k|v buffer of `total` heads; "padded": row strides + 8
LAYOUTS = [(1, 1, "dense", 0), (4, 2, "dense", 0), (4, 2, "fused", 8), (33, 3, "dense", 0), (64, 8, "fused", 80), (4, 2, "padded", 0)]
LAYOUT_IDS = ["1x1", "4x2", "4x2-of-8", "33x3", "64x8-of-80", "4x2-pad8"]
GRAD_SCALES = [2.0 ** -4, 2.0 ** -16]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _L():
    from qeft_amd import _lib
    return _lib, _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _gen(*key):
    seed = 7
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator(device=DEV).manual_seed(seed % (2 ** 31))


_TABLES = {}


def _tables(T, kind):
    """cos / sin fp32 [T, 64] inside NaN: the model's table (llama.QuantLlama's, base 10000) or a random one in [-1, 1]; made once."""
    if (T, kind) not in _TABLES:
        if kind == "model":
            from qeft_amd import qeft_cuda
            cos, sin = (x.to(DEV) for x in qeft_cuda.rope_cos_sin(10000.0, 64, T))
        else:
            g = _gen(99, T)
            cos, sin = (torch.rand(T, 64, generator=g, device=DEV) * 2 - 1 for _ in range(2))
        _TABLES[T, kind] = tuple(_Held(x, 64) for x in (cos, sin))
    return _TABLES[T, kind]


class _Held:
    """rows x width elements, rows `stride` apart, inside a NaN buffer with MARGIN elements on either side: .v is the view, .raw
    the buffer; intact(others) says that everything outside this view (and the views `others` of the same buffer) still is NaN."""

    def __init__(self, init, stride=None, dtype=None, raw=None, offset=0):
        rows, width = init.shape
        self.rows, self.width, self.stride, self.offset = rows, width, stride or width, offset
        dtype = dtype or init.dtype
        if raw is None:
            raw = torch.full((2 * MARGIN + rows * self.stride,), float("nan"), dtype=dtype, device=DEV)
        self.raw = raw
        self.v = raw[MARGIN:MARGIN + rows * self.stride].view(rows, self.stride)[:, offset:offset + width]
        assert self.v.data_ptr() % 16 == 0
        self.v[:] = init

    def intact(self, others=()):
        tmp = self.raw.clone()
        for h in (self, *others):
            tmp[MARGIN:MARGIN + h.rows * h.stride].view(h.rows, h.stride)[:, h.offset:h.offset + h.width] = float("nan")
        return bool(torch.isnan(tmp).all())

    def ptr(self, row=0):
        return self.v[row].data_ptr()


class _Case:
    """q [rows, H * 128] and k [rows, Hkv * 128] placed as the layout says.  "fused": one buffer of `total` heads per row, q first,
    then k, then heads that are not rotated (v, and whatever else) holding data that must come back bit-identical."""

    def __init__(self, q, k, place, total=0):
        rows, H, Hkv = q.shape[0], q.shape[1] // 128, k.shape[1] // 128
        self.rows, self.H, self.Hkv = rows, H, Hkv
        self.rest = None
        if place == "fused":
            g = _gen(5, rows, total)
            rest = torch.randn(rows, (total - H - Hkv) * 128, generator=g, device=DEV).half()
            self.q = _Held(q, total * 128)
            self.k = _Held(k, total * 128, raw=self.q.raw, offset=H * 128)
            self.rest = _Held(rest, total * 128, raw=self.q.raw, offset=(H + Hkv) * 128)
            self.rest_want = rest
        else:
            pad = 8 if place == "padded" else 0
            self.q, self.k = _Held(q, H * 128 + pad), _Held(k, Hkv * 128 + pad)
        self.q_want, self.k_want = q.clone(), k.clone()

    def inputs_intact(self):
        if self.rest is not None:
            ok = self.q.intact((self.k, self.rest)) and _same(self.rest.v, self.rest_want)
        else:
            ok = self.q.intact() and self.k.intact()
        return ok and _same(self.q.v, self.q_want) and _same(self.k.v, self.k_want)


def _run(case, T, cos, sin, inverse=0, rows=None, pos0=0):
    """One launch of the entry on `case` (rows = (first, count): that slice alone, through pointers into the same buffers, with the
    tables starting at row pos0 and t_len = T); returns (q_out, k_out), dense [count, heads * 128]."""
    _lib, lib = _L()
    first, count = rows or (0, case.rows)
    qo = _Held(torch.full((count, case.H * 128), float("nan"), dtype=F16, device=DEV))
    ko = _Held(torch.full((count, case.Hkv * 128), float("nan"), dtype=F16, device=DEV))
    _lib.check(lib.qeft_rope_qk(case.q.ptr(first), case.k.ptr(first), cos.ptr(pos0), sin.ptr(pos0), qo.ptr(), ko.ptr(), count, T,
                                case.H, case.Hkv, case.q.stride, case.k.stride, inverse, _st()))
    torch.cuda.synchronize()
    assert case.inputs_intact() and qo.intact() and ko.intact() and cos.intact() and sin.intact()
    return qo.v, ko.v


def _net_data(rows, width, g, scale):
    """N(0, 1) * 3 * scale with, from 3 rows on, one all-zero row and one row of +-30000 * scale."""
    x = torch.randn(rows, width, generator=g, device=DEV) * 3.0
    if rows >= 3:
        x[rows // 2] = 0.0
        x[rows - 1] = torch.where(torch.rand(width, generator=g, device=DEV) < 0.5, -30000.0, 30000.0)
    return (x * scale).half()


def _bits_data(rows, width, g):
    """N(0, 1) * 3 with +-65504, fp16 subnormals, +-0 and +-30000 in one value of eight; the first 16 pairs of every row's first
    head are (65504, -65504), whose rotation is 65504 (c + s) or 65504 (c - s): infinite wherever that factor passes 1."""
    x = (torch.randn(rows, width, generator=g, device=DEV) * 3.0).half()
    vals = torch.tensor([65504.0, -65504.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -15, -(2.0 ** -20), 0.0, -0.0, 30000.0, -30000.0],
                        dtype=F16, device=DEV)
    pick = torch.rand(rows, width, generator=g, device=DEV) < 0.125
    idx = torch.randint(0, len(vals), (rows, width), generator=g, device=DEV)
    x = torch.where(pick, vals[idx], x)
    x[:, :16], x[:, 64:80] = 65504.0, -65504.0
    return x


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\n[train_rope] {k}: largest err / bound over all cases = {WORST[k]:.4f}", end="")
    print()


def _net_check(kind, case_name, got, x, cos, sin, heads):
    """got against fp64 of the kernel's own inputs: B1 of the rotary, no value excluded."""
    xn, cn, sn = x.cpu().numpy(), cos.cpu().numpy(), sin.cpu().numpy()
    T = cn.shape[0]
    reps = xn.shape[0] // T
    cn, sn = np.tile(cn, (reps, 1)), np.tile(sn, (reps, 1))
    ref = rowwise_ref.rope_rows(xn, cn, sn, heads)
    bound = rowwise_ref.ulp16(ref) + 2.0 ** -22 * rowwise_ref.rope_rows_terms(xn, cn, sn, heads)
    gn = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(gn).all(), f"{kind} {case_name}: non-finite output"
    ratio = np.abs(gn - ref) / bound
    worst = float(ratio.max())
    WORST[kind] = max(WORST.get(kind, 0.0), worst)
    assert worst <= 1.0, f"{kind} {case_name}: err / bound {worst:.4f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


# ================================================================================================ fp64 net
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_rope_qk_against_fp64(layout):
    H, Hkv, place, total = layout
    for T, B, table in itertools.product(T_LENS, BATCHES, ("model", "random")):
        cos, sin = _tables(T, table)
        rows = B * T
        for inverse, scale in ((0, 1.0), (1, GRAD_SCALES[0]), (1, GRAD_SCALES[1])):
            g = _gen(1, T, B, H, Hkv, inverse, int(-np.log2(scale)))
            q, k = _net_data(rows, H * 128, g, scale), _net_data(rows, Hkv * 128, g, scale)
            case = _Case(q, k, place, total)
            qo, ko = _run(case, T, cos, sin, inverse)
            sgn = -1.0 if inverse else 1.0
            kind = "rope_qk inverse" if inverse else "rope_qk forward"
            name = f"{H}x{Hkv} {place} T={T} B={B} {table} table scale 2^{int(np.log2(scale))}"
            w = max(_net_check(kind, name + " q", qo, q, cos.v, sgn * sin.v, H), _net_check(kind, name + " k", ko, k, cos.v, sgn * sin.v, Hkv))
            print(f"[train_rope] {kind} {name}: largest err / bound = {w:.4f}")
            if rows >= 3:
                assert (qo[rows // 2] == 0).all() and (ko[rows // 2] == 0).all()                  # the all-zero row: exactly 0
            assert qo.abs().max() > 0 or rows < 2


# ================================================================================================ the bits of the torch route
def _torch_route(q4, k4, cos, sin, dq4=None, dk4=None):
    """finetune._rope on q and on k [B, T, heads, 128]; with output gradients also (q.grad, k.grad)."""
    from qeft_amd import finetune
    ql, kl = q4.detach().clone().requires_grad_(dq4 is not None), k4.detach().clone().requires_grad_(dk4 is not None)
    c, s = cos[:, None, :], sin[:, None, :]
    qr, kr = finetune._rope(ql, c, s), finetune._rope(kl, c, s)
    if dq4 is None:
        return qr, kr
    torch.autograd.backward([qr, kr], [dq4, dk4])
    return qr.detach(), kr.detach(), ql.grad, kl.grad


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_rope_qk_has_the_bits_of_the_torch_route(layout):
    """Entry, forward and inverse, against finetune._rope and its autograd.  64 x 8 at T = 67, B = 3 compares 2 x 1.8e6 values per
    direction: a contracted product (7e-5 of the values differ, tests/test_train_rope_cpu.py) cannot slip through."""
    H, Hkv, place, total = layout
    most = 0
    for T, B, table in itertools.product(T_LENS, BATCHES, ("model", "random")):
        cos, sin = _tables(T, table)
        rows = B * T
        g = _gen(2, T, B, H, Hkv)
        q, k, dq, dk = (_bits_data(rows, w * 128, g) for w in (H, Hkv, H, Hkv))
        qo, ko = _run(_Case(q, k, place, total), T, cos, sin, 0)
        gq, gk = _run(_Case(dq, dk, place, total), T, cos, sin, 1)
        v4 = lambda x, h: x.view(B, T, h, 128)
        want = _torch_route(v4(q, H), v4(k, Hkv), cos.v, sin.v, v4(dq, H), v4(dk, Hkv))
        for nm, got, ref, h in (("q_rot", qo, want[0], H), ("k_rot", ko, want[1], Hkv), ("dq", gq, want[2], H), ("dk", gk, want[3], Hkv)):
            assert not torch.isnan(ref).any()
            assert _same(v4(got, h), ref), f"{nm} {layout} T={T} B={B} {table}: {int((_bits(v4(got, h)) != _bits(ref)).sum())} values differ"
        if T * B >= 5:
            assert torch.isinf(want[0]).any() and torch.isinf(want[2]).any()             # inf equals inf is part of what was compared
        most = max(most, qo.numel() + ko.numel())
    if (H, Hkv) == (64, 8):
        assert most >= 5 * 10 ** 5
    print(f"[train_rope] {H}x{Hkv} {place}: forward and inverse bit-equal to finetune._rope and its autograd, up to {most} values per call")


# ================================================================================================ independence
def test_a_heads_bits_do_not_depend_on_the_launch():
    """Heads of the 64 x 8 launch (views of an 80-head buffer, T = 67, B = 3) equal the same head launched alone (1 x 1, dense),
    at another stride, and as a single row b T + t of the batch; inverse = 1 equals inverse = 0 on the negated sin table."""
    T, B, H, Hkv = 67, 3, 64, 8
    rows = B * T
    cos, sin = _tables(T, "random")
    g = _gen(3)
    q, k = _bits_data(rows, H * 128, g), _bits_data(rows, Hkv * 128, g)
    big = _Case(q, k, "fused", 80)
    for inverse in (0, 1):
        qo, ko = _run(big, T, cos, sin, inverse)
        for hq, hk in ((0, 0), (31, 3), (33, 5), (63, 7)):                               # alone: one head of q with one of k
            one = _Case(q[:, hq * 128:(hq + 1) * 128].contiguous(), k[:, hk * 128:(hk + 1) * 128].contiguous(), "dense")
            q1, k1 = _run(one, T, cos, sin, inverse)
            assert _same(q1, qo[:, hq * 128:(hq + 1) * 128]) and _same(k1, ko[:, hk * 128:(hk + 1) * 128]), (inverse, hq, hk)
        q2, k2 = _run(_Case(q, k, "padded"), T, cos, sin, inverse)                       # other strides
        assert _same(q2, qo) and _same(k2, ko), inverse
        q3, k3 = _run(_Case(q, k, "dense"), T, cos, sin, inverse)
        assert _same(q3, qo) and _same(k3, ko), inverse
        for b, t in ((0, 0), (1, 66), (2, 30)):                                          # row b T + t alone, as a T = 1 launch at position t
            r = b * T + t
            q4, k4 = _run(big, 1, cos, sin, inverse, rows=(r, 1), pos0=t)
            assert _same(q4, qo[r:r + 1]) and _same(k4, ko[r:r + 1]), (inverse, b, t)
        q5, k5 = _run(big, T, cos, sin, inverse, rows=(T, 2 * T))                        # sequences 1 and 2 as a batch of two
        assert _same(q5, qo[T:]) and _same(k5, ko[T:]), inverse
    # the inverse is the forward on -sin: bit for bit but for the +0 of autograd's slice sum (a -0 of the transpose comes out +0)
    neg = _Held(-sin.v, 64)
    qi, ki = _run(big, T, cos, sin, 1)
    qn, kn = _run(big, T, cos, neg, 0)
    for a, b in ((qi, qn), (ki, kn)):
        assert _same(a, b + torch.zeros((), dtype=F16, device=DEV))
        differ = _bits(a) != _bits(b)
        assert (_bits(b)[differ] == -32768).all() and (_bits(a)[differ] == 0).all()
    print("[train_rope] independence: heads of 64 x 8 == alone == other strides == single rows == a sub-batch; inverse == forward(-sin) "
          f"but for {int(differ.sum())} results of -0 in k that come out +0")


# ================================================================================================ autograd
def test_rope_qk_autograd_equals_the_entry():
    from qeft_amd import rope_qk
    T, B, H, Hkv = 67, 2, 4, 2
    rows = B * T
    cos, sin = _tables(T, "model")
    g = _gen(4)
    q, k, dq, dk = (_bits_data(rows, w * 128, g) for w in (H, Hkv, H, Hkv))
    case = _Case(q, k, "fused", 8)
    qo, ko = _run(case, T, cos, sin, 0)
    gq, gk = _run(_Case(dq, dk, "dense"), T, cos, sin, 1)
    v4 = lambda x, h: x.view(B, T, h, 128)
    fused = case.q.raw[MARGIN:MARGIN + rows * 1024].view(B, T, 8, 128)                    # the q|k|v buffer as the model would hold it
    for need_q, need_k in ((True, True), (True, False), (False, True)):
        ql, kl = fused[:, :, :H].detach().requires_grad_(need_q), fused[:, :, H:H + Hkv].detach().requires_grad_(need_k)
        qr, kr = rope_qk(ql, kl, cos.v, sin.v)
        assert qr.is_contiguous() and kr.is_contiguous() and _same(qr, v4(qo, H)) and _same(kr, v4(ko, Hkv))
        torch.autograd.backward([qr, kr], [v4(dq, H), v4(dk, Hkv)])
        assert (ql.grad is None) == (not need_q) and (kl.grad is None) == (not need_k)
        assert (not need_q or _same(ql.grad, v4(gq, H))) and (not need_k or _same(kl.grad, v4(gk, Hkv)))
    assert case.inputs_intact()
    # non-contiguous gradients: the transposed one SDPA returns, and an expanded one; a missing gradient is zero
    ql, kl = v4(q, H).clone().requires_grad_(True), v4(k, Hkv).clone().requires_grad_(True)
    qr, kr = rope_qk(ql, kl, cos.v, sin.v)
    dq_t = v4(dq, H).transpose(1, 2).contiguous().transpose(1, 2)
    assert not dq_t.is_contiguous()
    torch.autograd.backward([qr, kr], [dq_t, v4(dk, Hkv)[:, :, :1].expand(B, T, Hkv, 128)])
    assert _same(ql.grad, v4(gq, H))
    dk_e = v4(dk, Hkv)[:, :, :1].expand(B, T, Hkv, 128).contiguous().view(rows, Hkv * 128)
    assert _same(kl.grad, v4(_run(_Case(dq, dk_e, "dense"), T, cos, sin, 1)[1], Hkv))
    ql.grad = kl.grad = None
    qr, kr = rope_qk(ql, kl, cos.v, sin.v)
    qr.backward(v4(dq, H))
    assert _same(ql.grad, v4(gq, H)) and (kl.grad is None or not kl.grad.any())
    # no gradient wanted at all: no backward launch, and inputs that are not rows at a legal stride are copied
    qr, kr = rope_qk(v4(q, H).transpose(0, 1).contiguous().transpose(0, 1), v4(k, Hkv)[:, :, ::2].repeat_interleave(2, 2)[:, :, ::2], cos.v, sin.v)
    assert _same(qr, v4(qo, H)) and _same(kr[:, :, 0], v4(ko, Hkv)[:, :, 0])
    with pytest.raises(ValueError):
        rope_qk(v4(q, H), v4(k, Hkv), cos.v[:5], sin.v[:5])
    with pytest.raises(ValueError):
        rope_qk(v4(q, H).float(), v4(k, Hkv), cos.v, sin.v)
    print("[train_rope] rope_qk: outputs and grads equal the entry bit for bit; None for inputs without grad; views and copies alike")


# ================================================================================================ model
@pytest.mark.parametrize("attn", ["sdpa", "own"])
@pytest.mark.parametrize("glue", ["torch", "fused"])
@pytest.mark.parametrize("checkpoint", [True, False], ids=["checkpoint", "plain"])
@pytest.mark.parametrize("batch", [1, 2], ids=["T200", "B2xT100"])
@pytest.mark.parametrize("which", ["gqa", "tiny"])
def test_causal_lm_loss_with_fused_rope(which, batch, checkpoint, glue, attn):
    """rope="fused" gives the bits of rope="torch": the loss under no_grad bit for bit, and on the deterministic route
    (attn="own") every d(oweight) bit for bit; section 4.14's criterion holds unchanged (loss error from an fp64 dense pass at most
    2 x the fp16 plain-torch dense pass's + 2^-14, the relative L2 error of every d(oweight) at most 2 x that pass's own); and
    rope="torch" gives the identical loss before and after."""
    from qeft_amd import causal_lm_loss
    from qeft_amd.llama import layer_linears
    model, tokens, labels, params, reference = _trainable(which)
    loss64, g64, loss16, g16 = reference(batch)
    tok = tokens.view(batch, -1) if batch > 1 else tokens
    lab = labels.view(batch, -1) if batch > 1 else labels
    kw = dict(checkpoint=checkpoint, attn=attn, glue=glue)
    with torch.no_grad():
        before = causal_lm_loss(model, tok, lab, rope="torch", **kw)
        fused = causal_lm_loss(model, tok, lab, rope="fused", **kw)
    assert _same(before, fused), (before.item(), fused.item())

    def grads(rope):
        for p in params:
            p.grad = None
        loss = causal_lm_loss(model, tok, lab, rope=rope, **kw)
        (loss * LOSS_SCALE).backward()
        return loss, [[(nm, ql.oweight.grad.clone()) for nm, ql in layer_linears(L)] for L in model.model.layers]

    loss, got = grads("fused")
    assert loss.dtype == F32 and loss.dim() == 0 and _same(loss.detach(), before)
    e_own, e_16 = abs(loss.item() - loss64), abs(loss16 - loss64)
    worst = 0.0
    for li, layer in enumerate(got):
        for nm, gr in layer:
            assert gr.dtype == F32 and torch.isfinite(gr).all(), (li, nm)
            ref = g64[li][nm]
            own = ((gr.to(F64) / LOSS_SCALE - ref).norm() / ref.norm()).item()
            t16 = ((g16[li][nm] - ref).norm() / ref.norm()).item()
            worst = max(worst, own / t16)
    kind = f"{which} {'checkpoint' if checkpoint else 'plain'} batch {batch} glue {glue} attn {attn}"
    print(f"[train_rope] model {kind}: loss {loss.item():.6f} fp64 {loss64:.6f}  |d| fused rope {e_own:.3e}  fp16 torch {e_16:.3e}; "
          f"largest d(oweight) error ratio fused rope / fp16 torch = {worst:.3f} (allowed 2)")
    assert e_own <= 2 * e_16 + 2.0 ** -14, f"{kind}: loss error {e_own:.3e} > 2 x {e_16:.3e} + 2^-14"
    assert worst <= 2.0, f"{kind}: a d(oweight) is {worst:.2f} x the fp16 torch pass's error from fp64"
    if attn == "own":
        _, want = grads("torch")
        for li, (a, b) in enumerate(zip(got, want)):
            for (nm, x), (_, y) in zip(a, b):
                assert _same(x, y), f"{kind}: d(oweight) of {li}.{nm} differs between rope='fused' and rope='torch'"
    with torch.no_grad():
        after = causal_lm_loss(model, tok, lab, rope="torch", **kw)
    assert _same(after, before)


def test_fused_rope_launches_are_the_ones_that_run(monkeypatch):
    """causal_lm_loss(rope="fused") over n layers reaches qeft_rope_qk with inverse = 0 n times plain and 2 n times checkpointed
    (the recomputation reruns the forward), with inverse = 1 n times, on either glue and attn; rope="torch" never reaches it."""
    from qeft_amd import _lib, causal_lm_loss
    model, tokens, labels, params, _ = _trainable("gqa")
    lib = _lib.lib()
    calls = []
    orig = lib.qeft_rope_qk
    monkeypatch.setattr(lib, "qeft_rope_qk", lambda *a: (calls.append(a[12]), orig(*a))[1])
    n = model.shape.n_layers
    for ckpt, glue, attn in itertools.product((False, True), ("torch", "fused"), ("own", "sdpa")):
        calls.clear()
        causal_lm_loss(model, tokens, labels, checkpoint=ckpt, attn=attn, glue=glue, rope="fused").backward()
        assert (calls.count(0), calls.count(1), len(calls)) == (2 * n if ckpt else n, n, (3 if ckpt else 2) * n), (ckpt, glue, attn, calls)
    calls.clear()
    causal_lm_loss(model, tokens, labels, glue="fused", attn="own", rope="torch").backward()
    causal_lm_loss(model, tokens, labels, checkpoint=False).backward()
    assert calls == []
    for p in params:
        p.grad = None
