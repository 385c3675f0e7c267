"""fp64 net under the fused head's backward (csrc/lm_head_nll_grad.hip, variant "lm_head_nll_grad"), under
scoring.lm_head_nll_loss and under finetune.causal_lm_loss.

The kernel reference is fp64 from the kernel's own fp16 inputs; lse is taken from a forward launch (qeft_lm_head_nll), as the
autograd function hands it over.  With E_ij and mag_ij as in tests/test_gpu_lm_head_nll.py (E = (hidden / 16 + 8) 2^-23 mag), the
bound on the fp32 output is derived, not measured:

  delta_ij = E_ij + (max_j E_ij + 2^-14) + 2^-16        error of logit - lse: the logit, the forward's lse, the subtraction and __expf
  a_ij     = 1.01 delta_ij p_ij                          error of p = exp(logit - lse)
           + 2^-11 |g_ij| + 2^-25                        g = p - onehot rounded once to fp16; fp16's subnormal step
           + (vocab / 16 + 8) 2^-23 (1 + 2^-10) |g_ij|   the MFMA chain over the vocabulary
  |dx_ik - ref_ik| <= |grad_nll_i| sum_j a_ij |w_jk| + 2^-23 |ref_ik|

and the fp16 output adds half an fp16 ulp of the value (it must also equal fp32_out.half() as integers).  x is a view inside a
NaN buffer, the weight sits inside a NaN buffer, dx is a strided view between NaN bands that must stay NaN, workspace and dx sit
between guard margins that must come back intact.  Every test prints its worst error / bound ratio ([lm_head_nll_grad] ...).

The model-level tests compare causal_lm_loss with the dense pass of tests/dense_ref.py, run once in fp64 and once with fp16 tensors
and plain torch ops: the project's route may be off the fp64 pass by at most twice what the fp16 torch pass is (the same rounding
points summed in another order, plus the backward's dY rounded to fp16 once more)."""
import math
import os

import pytest
import torch

from dense_ref import dense_pass

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 64
FILL = 0xA5
NAN = float("nan")
F16, F32, F64, I32 = torch.float16, torch.float32, torch.float64, torch.int32
IGNORE = -100


def _L():
    from qeft_amd import _lib
    return _lib, _lib.lib()


def _R():
    return _L()[1].qeft_lm_head_nll_grad_chunk_rows(4096, 32000)


class Guarded:
    """`n` elements of `dtype` between two margins of FILL bytes; the elements start as NaN."""

    def __init__(self, n, dtype):
        es = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((n + 2 * MARGIN) * es,), FILL, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = MARGIN * es, (MARGIN + n) * es
        self.t = self.raw[self.lo:self.hi].view(dtype)
        self.t.fill_(NAN)

    def margins_intact(self):
        return bool((self.raw[:self.lo] == FILL).all().item() and (self.raw[self.hi:] == FILL).all().item())


def _poisoned_x(x, pad=8, stride=None):
    """x [t, hidden] as a view of a NaN buffer: one NaN row before, two after, `pad` NaN elements left of every row, the rest of
    the stride right of it."""
    t, hidden = x.shape
    stride = stride or hidden + 2 * pad
    buf = torch.full((t + 3, stride), NAN, dtype=F16, device=DEV)
    view = buf[1:1 + t, pad:pad + hidden]
    view.copy_(x)
    return view


def _poisoned_w(w):
    vocab, hidden = w.shape
    buf = torch.full((vocab * hidden + 2 * MARGIN,), NAN, dtype=F16, device=DEV)
    view = buf[MARGIN:MARGIN + vocab * hidden].view(vocab, hidden)
    view.copy_(w)
    return view


def _forward_lse(x, w, targets):
    """lse fp32 [t] of one qeft_lm_head_nll launch."""
    _lib, lib = _L()
    t, hidden = x.shape
    vocab = w.shape[0]
    need = lib.qeft_lm_head_nll_workspace_bytes(t, vocab)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    lse, tgt = torch.empty(t, dtype=F32, device=DEV), torch.empty(t, dtype=F32, device=DEV)
    tg = targets.to(device=DEV, dtype=I32).contiguous()
    _lib.check(lib.qeft_lm_head_nll(x.data_ptr(), x.stride(0), w.data_ptr(), tg.data_ptr(), lse.data_ptr(), tgt.data_ptr(), None,
                                    ws.data_ptr(), need, t, hidden, vocab, torch.cuda.current_stream().cuda_stream))
    return lse


def _launch(x, w, targets, lse, grad_nll, fp32, pad=8, dx_stride=None):
    """One call of the C entry: dx a strided view between NaN bands inside a guarded buffer, the workspace guarded and exactly
    sized.  Returns dx [t, hidden] (a clone)."""
    _lib, lib = _L()
    t, hidden = x.shape
    vocab = w.shape[0]
    assert x.stride(1) == 1 and w.is_contiguous()
    R = _R()
    need = lib.qeft_lm_head_nll_grad_workspace_bytes(t, hidden, vocab)
    assert need == 2 * min(t, R) * ((vocab + 127) // 128 * 128)
    ws = Guarded(need // 2, F16)
    dt = F32 if fp32 else F16
    stride = dx_stride or hidden + 2 * pad
    out = Guarded(t * stride, dt)
    grid = out.t.view(t, stride)
    dx = grid[:, pad:pad + hidden]
    tg = targets.to(device=DEV, dtype=I32).contiguous()
    gn = grad_nll.to(device=DEV, dtype=F32).contiguous()
    _lib.check(lib.qeft_lm_head_nll_grad(x.data_ptr(), x.stride(0), w.data_ptr(), tg.data_ptr(), lse.data_ptr(), gn.data_ptr(),
                                         dx.data_ptr(), stride, int(fp32), ws.t.data_ptr(), need, t, hidden, vocab,
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _lib.last_variant() == "lm_head_nll_grad"
    assert ws.margins_intact(), "workspace: a guard margin was written"
    assert out.margins_intact(), "dx: a guard margin was written"
    assert torch.isnan(grid[:, :pad]).all() and torch.isnan(grid[:, pad + hidden:]).all(), "dx: a band between the rows was written"
    return dx.clone()


def _ref64(x, w):
    """fp64 logits and mag [t, vocab] of fp16 operands, the vocabulary in pieces."""
    xd = x.to(F64)
    xa = xd.abs()
    t, vocab = x.shape[0], w.shape[0]
    logits, mag = torch.empty(t, vocab, dtype=F64, device=DEV), torch.empty(t, vocab, dtype=F64, device=DEV)
    for c0 in range(0, vocab, 4096):
        wd = w[c0:c0 + 4096].to(F64)
        logits[:, c0:c0 + 4096] = xd @ wd.t()
        mag[:, c0:c0 + 4096] = xa @ wd.abs_().t()
    return logits, mag


def _ref_dx(x, w, targets, grad_nll):
    """(ref, bound, live): the fp64 gradient [t, hidden], the derived bound on the fp32 output and the mask of scored rows."""
    t, hidden = x.shape
    vocab = w.shape[0]
    logits, mag = _ref64(x, w)
    E = (hidden / 16 + 8) * 2.0 ** -23 * mag
    delta = E + (E.max(dim=1, keepdim=True).values + 2.0 ** -14) + 2.0 ** -16
    tg = targets.to(DEV).long()
    live = (tg >= 0) & (tg < vocab)
    p = torch.softmax(logits, dim=1)
    g = p.clone()
    rows = live.nonzero()[:, 0]
    g[rows, tg[rows]] -= 1.0
    g[~live] = 0.0
    a = 1.01 * delta * p + 2.0 ** -11 * g.abs() + 2.0 ** -25 + (vocab / 16 + 8) * 2.0 ** -23 * (1 + 2.0 ** -10) * g.abs()
    gw, aw = torch.zeros(t, hidden, dtype=F64, device=DEV), torch.zeros(t, hidden, dtype=F64, device=DEV)
    for c0 in range(0, vocab, 4096):
        wd = w[c0:c0 + 4096].to(F64)
        gw += g[:, c0:c0 + 4096] @ wd
        aw += a[:, c0:c0 + 4096] @ wd.abs_()
    gn = grad_nll.to(device=DEV, dtype=F64)[:, None]
    ref = gn * gw
    return ref, gn.abs() * aw + 2.0 ** -23 * ref.abs(), live


def _half_ulp16(v):
    """Half an fp16 ulp of |v| (2^-25 below the normal range)."""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 11)


WORST = {}


def _check(tag, dx32, dx16, ref, bound, live):
    """Both outputs of rows [0, t) against the reference rows; asserts the bounds and the exact zeros, records the ratios."""
    t = dx32.shape[0]
    ref, bound, live = ref[:t], bound[:t], live[:t]
    assert dx32.dtype == F32 and dx16.dtype == F16
    assert torch.equal(dx16.view(torch.int16), dx32.half().view(torch.int16)), f"{tag}: the fp16 output is not the rounding of the fp32 output"
    assert (dx32[~live].view(I32) == 0).all() and (dx16[~live].view(torch.int16) == 0).all(), f"{tag}: an ignored row is not +0.0"
    r32 = r16 = 0.0
    if bool(live.any()):
        assert torch.isfinite(dx32[live]).all(), f"{tag}: non-finite dx"
        r32 = ((dx32.to(F64) - ref).abs() / bound)[live].max().item()
        r16 = ((dx16.to(F64) - ref).abs() / (bound + _half_ulp16(ref.abs() + bound)))[live].max().item()
    rel = (bound[live] / ref[live].abs().clamp_min(1e-300)).median().item() if bool(live.any()) else 0.0
    key = tag.split(" ")[0]
    WORST[key] = max(WORST.get(key, 0.0), r32, r16)
    print(f"[lm_head_nll_grad] {tag}: err / bound  fp32 {r32:.4f}  fp16 {r16:.4f}  (median bound / |ref| {rel:.2e})")
    assert r32 <= 1.0 and r16 <= 1.0, f"{tag}: fp32 {r32:.3f}, fp16 {r16:.3f} of the bound"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\n[lm_head_nll_grad] {k}: largest err / bound over all cases = {WORST[k]:.4f}", end="")


_OPERANDS = {}


def _operands(hidden, vocab, rows):
    """Random operands of one shape with their fp64 reference: made once, shared, never written.  x ~ N(0, 1), w ~ N(0, 0.02^2)
    inside a NaN buffer, grad_nll ~ N(0, 1) of both signs, targets with every kind of row (row 0 is a scored one)."""
    key = (hidden, vocab)
    if key not in _OPERANDS or _OPERANDS[key][0].shape[0] < rows:
        g = torch.Generator(device=DEV).manual_seed(hidden * 5 + vocab)
        x = torch.randn(rows, hidden, generator=g, device=DEV).half()
        w = _poisoned_w((torch.randn(vocab, hidden, generator=g, device=DEV) * 0.02).half())
        targets = torch.randint(0, vocab, (rows,), generator=g, device=DEV).to(I32)
        special = torch.tensor([IGNORE, -1, vocab, vocab - 1, 0, vocab + 5, (vocab - 1) // 128 * 128], dtype=I32, device=DEV)
        every5 = torch.arange(3, rows, 5, device=DEV)                 # ignored rows, both ends, the first column of the last tile
        targets[every5] = special[torch.arange(every5.numel(), device=DEV) % 7]
        grad_nll = torch.randn(rows, generator=g, device=DEV)
        ref, bound, live = _ref_dx(x, w, targets, grad_nll)
        _OPERANDS[key] = (x, w, targets, grad_nll, ref, bound, live)
    return _OPERANDS[key]


def _both(x, w, targets, grad_nll, **kw):
    xv = _poisoned_x(x)
    lse = _forward_lse(xv, w, targets)
    return _launch(xv, w, targets, lse, grad_nll, True, **kw), _launch(xv, w, targets, lse, grad_nll, False, **kw)


SMALL = [(256, 512), (512, 9), (512, 127), (512, 129), (1024, 4097)]
CASES = [(h, v, t) for h, v in SMALL for t in (1, 7, 64, 65, 129, 200)] + [(4096, 32000, t) for t in (1, 65)]
ROWS = {(4096, 32000): 65}


@pytest.mark.parametrize("hidden,vocab,t", CASES)
def test_parity_fp64_poisoned(hidden, vocab, t):
    x, w, targets, gn, ref, bound, live = _operands(hidden, vocab, ROWS.get((hidden, vocab), 200))
    dx32, dx16 = _both(x[:t], w, targets[:t], gn[:t])
    _check(f"parity hidden={hidden} vocab={vocab} t={t}", dx32, dx16, ref, bound, live)


@pytest.mark.parametrize("which", ["R-1", "R+1", "2R+5"])
def test_parity_over_the_chunk_loop(which):
    R = _R()
    t = {"R-1": R - 1, "R+1": R + 1, "2R+5": 2 * R + 5}[which]
    x, w, targets, gn, ref, bound, live = _operands(256, 512, 2 * R + 5)
    dx32, dx16 = _both(x[:t], w, targets[:t], gn[:t])
    _check(f"chunks hidden=256 vocab=512 t={which}={t}", dx32, dx16, ref, bound, live)


def test_ignored_rows_are_plus_zero_whatever_grad_nll_holds():
    x, w, targets, gn, ref, bound, live = _operands(256, 512, 200)
    t = 200
    xv = _poisoned_x(x[:t])
    lse = _forward_lse(xv, w, targets[:t])
    base = _launch(xv, w, targets[:t], lse, gn[:t], True)
    bad = gn[:t].clone()
    bad[~live[:t]] = NAN
    assert int((~live[:t]).sum()) >= 10
    for fp32 in (True, False):
        got = _launch(xv, w, targets[:t], lse, bad, fp32)
        want = base if fp32 else base.half()
        bits = I32 if fp32 else torch.int16
        assert (got[~live[:t]].view(bits) == 0).all(), "an ignored row with grad_nll = NaN is not +0.0"
        assert torch.equal(got.view(bits), want.view(bits)), "NaN on ignored rows changed another row"
    print("[lm_head_nll_grad] ignored rows: +0.0 under grad_nll = NaN, the other rows unchanged bit for bit")


def test_p_comes_from_fp32_logits():
    """Peaked rows: logits of tens, p close to one-hot.  A softmax of fp16-rounded logits misses the bound (fourfold in a CPU
    emulation of the arithmetic); fp32 logits and an fp32 exp stay inside it."""
    hidden, vocab, t = 256, 512, 64
    g = torch.Generator(device=DEV).manual_seed(21)
    x = (torch.randn(t, hidden, generator=g, device=DEV) * 6).half()
    w = _poisoned_w((torch.randn(vocab, hidden, generator=g, device=DEV) * 0.05).half())
    targets = torch.randint(0, vocab, (t,), generator=g, device=DEV).to(I32)
    gn = torch.randn(t, generator=g, device=DEV)
    ref, bound, live = _ref_dx(x, w, targets, gn)
    dx32, dx16 = _both(x, w, targets, gn)
    _check("peaked hidden=256 vocab=512 t=64", dx32, dx16, ref, bound, live)


def test_row_invariance_bit_for_bit():
    """A row of dx does not depend on t, on the row's index in the launch or its chunk, or on either stride."""
    R = _R()
    x, w, targets, gn, _, _, _ = _operands(256, 512, 2 * R + 5)
    for fp32 in (True, False):
        bits = I32 if fp32 else torch.int16
        xv = _poisoned_x(x[:200])
        lse = _forward_lse(xv, w, targets[:200])
        full = _launch(xv, w, targets[:200], lse, gn[:200], fp32)
        for a, b in ((0, 64), (64, 65), (65, 200)):
            part = _launch(_poisoned_x(x[a:b]), w, targets[a:b], lse[a:b].contiguous(), gn[a:b], fp32)
            assert torch.equal(full[a:b].view(bits), part.view(bits)), f"rows [{a}, {b}) launched alone differ (fp32={fp32})"
        other = _launch(_poisoned_x(x[:200], pad=0, stride=3 * 256), w, targets[:200], lse, gn[:200], fp32, pad=16, dx_stride=2 * 256 + 64)
        assert torch.equal(full.view(bits), other.view(bits)), f"another x_stride / dx_stride differs (fp32={fp32})"
        t = R + 5
        xv = _poisoned_x(x[:t])
        lse = _forward_lse(xv, w, targets[:t])
        full = _launch(xv, w, targets[:t], lse, gn[:t], fp32)
        tail = _launch(_poisoned_x(x[R:t]), w, targets[R:t], lse[R:t].contiguous(), gn[R:t], fp32)
        assert torch.equal(full[R:t].view(bits), tail.view(bits)), f"rows R .. R + 4 launched alone differ (fp32={fp32})"
    print("[lm_head_nll_grad] invariance: 3 sub-launches, a second pair of strides and the second chunk's rows, bit for bit")


def test_autograd_function():
    from qeft_amd import lm_head_nll, lm_head_nll_loss
    _lib, _ = _L()
    x, w, targets, gn, ref, bound, live = _operands(256, 512, 200)
    t = 200
    hn = x[:t].clone().requires_grad_(True)
    nll = lm_head_nll_loss(hn, w, targets[:t])
    lse, tgt, _ = lm_head_nll(hn.detach(), w, targets[:t])
    want = torch.where(live[:t], lse - tgt, torch.zeros_like(lse))
    assert nll.dtype == F32 and torch.equal(nll.view(I32), want.view(I32)), "nll is not lse - tgt_logit of lm_head_nll"
    seen = []                                  # the backward runs on autograd's thread, and the variant name is per thread:
    hn.register_hook(lambda grad: seen.append(_lib.last_variant()))      # read it there, right after the entry returned
    (nll * gn[:t]).sum().backward()
    assert seen == ["lm_head_nll_grad"], seen
    direct = _launch(hn.detach(), w, targets[:t], lse, gn[:t], False)
    assert hn.grad.dtype == F16 and torch.equal(hn.grad.view(torch.int16), direct.view(torch.int16))
    hn2 = x[:t].clone().requires_grad_(True)
    lm_head_nll_loss(hn2, w, targets[:t]).sum().backward()
    ones = _launch(hn2.detach(), w, targets[:t], lse, torch.ones(t, device=DEV), False)
    assert torch.equal(hn2.grad.view(torch.int16), ones.view(torch.int16))
    wg = w.clone().requires_grad_(True)
    with pytest.raises(ValueError):
        lm_head_nll_loss(hn, wg, targets[:t])


def test_torch_route_for_a_width_the_entry_refuses(monkeypatch):
    from qeft_amd import lm_head_nll_loss
    _lib, lib = _L()
    hidden, vocab, t = 96, 300, 5
    g = torch.Generator(device=DEV).manual_seed(22)
    x = torch.randn(t, hidden, generator=g, device=DEV).half()
    w = (torch.randn(vocab, hidden, generator=g, device=DEV) * 0.05).half()
    targets = torch.tensor([0, 299, IGNORE, 128, vocab], dtype=I32)
    gn = torch.randn(t, generator=g, device=DEV)
    assert lib.qeft_lm_head_nll_grad_workspace_bytes(t, hidden, vocab) == 0
    calls = []
    orig = lib.qeft_lm_head_nll_grad
    monkeypatch.setattr(lib, "qeft_lm_head_nll_grad", lambda *a: (calls.append(a), orig(*a))[1])
    hn = x.clone().requires_grad_(True)
    (lm_head_nll_loss(hn, w, targets) * gn).sum().backward()
    assert calls == [], "the refused width was launched"
    ref, bound, live = _ref_dx(x, w, targets, gn)
    assert hn.grad.dtype == F16
    _check("torch-route hidden=96 vocab=300 t=5", hn.grad.float(), hn.grad, ref, bound, live)


def test_no_logits_in_memory():
    """hn [2048, 512], W [32000, 512], forward + backward: the peak rises by less than 128 MiB over the operands (the fp32 logits
    alone are 250 MiB); at T = 4096 it rises by no more than the added outputs (nll and hn.grad) plus 1 MiB."""
    from qeft_amd import lm_head_nll_loss, scoring
    g = torch.Generator(device=DEV).manual_seed(23)
    w = (torch.randn(32000, 512, generator=g, device=DEV) * 0.02).half()
    rises = {}
    for T in (2048, 4096):
        hn = torch.randn(T, 512, generator=g, device=DEV).half().requires_grad_(True)
        targets = torch.randint(0, 32000, (T,), generator=g, device=DEV).to(I32)
        scoring._workspace.clear()
        scoring._grad_workspace.clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        seen = []
        hn.register_hook(lambda grad: seen.append(_L()[0].last_variant()))        # on autograd's thread (the name is per thread)
        nll = lm_head_nll_loss(hn, w, targets)
        nll.sum().backward()
        torch.cuda.synchronize()
        rises[T] = torch.cuda.max_memory_allocated() - base
        assert seen == ["lm_head_nll_grad"] and torch.isfinite(nll).all() and torch.isfinite(hn.grad).all()
        del nll, hn
    added = 2048 * (512 * 2 + 4)
    print(f"[lm_head_nll_grad] memory: peak rise {rises[2048] / 2 ** 20:.2f} MiB at T = 2048, {rises[4096] / 2 ** 20:.2f} MiB at T = 4096 "
          f"(added outputs {added / 2 ** 20:.2f} MiB)")
    assert rises[2048] < 128 * 2 ** 20
    assert rises[4096] - rises[2048] <= added + 2 ** 20


# ---- the tiny model: causal_lm_loss against the dense pass of tests/dense_ref.py, in fp64 and in fp16
T_DOC = 48

NAMES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
SCALE = 1024.0


@pytest.fixture(scope="module")
def tiny_train():
    from qeft_amd import finetune
    from qeft_amd.llama import QuantLlama, layer_linears, tiny_shape
    model = QuantLlama(tiny_shape(), DEV, seed=6)
    g = torch.Generator().manual_seed(4)
    tokens = torch.randint(0, model.shape.vocab, (T_DOC,), generator=g).to(DEV)
    labels = tokens.clone()
    labels[torch.tensor([0, 1, 2, 10, 11, 30, 47])] = IGNORE
    dense = model.dense_weights()                                       # before begin(): oweight is still the fp16 buffer
    ow = [{nm: ql.oweight.detach().clone() for nm, ql in layer_linears(L)} for L in model.model.layers]
    params = finetune.begin(model)
    assert len(params) == 7 * model.shape.n_layers and all(p.dtype == F32 and p.requires_grad for p in params)
    assert not any(p.requires_grad for n, p in model.named_parameters() if "oweight" not in n)
    refs = {}

    def reference(batch):
        """(loss64, grads64, loss16, grads16) of the [batch, T_DOC / batch] view, made once per view."""
        if batch not in refs:
            tok2 = tokens.view(batch, -1)
            targets = finetune.shift_labels(tok2, labels.view(batch, -1)).reshape(-1)
            out = []
            for dt in (F64, F16):
                leaves = [{nm: v.to(F64 if dt == F64 else F32).requires_grad_(True) for nm, v in d.items()} for d in ow]
                loss = dense_pass(model, dense, leaves, tok2, targets, dt)
                (loss * (SCALE if dt == F16 else 1.0)).backward()
                grads = [{nm: (v.grad.to(F64) / (SCALE if dt == F16 else 1.0)) for nm, v in d.items()} for d in leaves]
                out += [loss.item(), grads]
            refs[batch] = tuple(out)
        return refs[batch]
    return model, tokens, labels, params, reference


@pytest.mark.parametrize("kind", ["checkpoint", "plain", "torch-head", "batch"])
def test_causal_lm_loss_on_the_tiny_model(tiny_train, kind):
    from qeft_amd import causal_lm_loss
    from qeft_amd.llama import layer_linears
    model, tokens, labels, params, reference = tiny_train
    batch = 2 if kind == "batch" else 1
    loss64, g64, loss16, g16 = reference(batch)
    for p in params:
        p.grad = None
    tok = tokens.view(batch, -1) if batch > 1 else tokens
    lab = labels.view(batch, -1) if batch > 1 else labels
    loss = causal_lm_loss(model, tok, lab, checkpoint=kind != "plain", head="torch" if kind == "torch-head" else "fused")
    assert loss.dtype == F32 and loss.dim() == 0
    (loss * SCALE).backward()
    e_own, e_16 = abs(loss.item() - loss64), abs(loss16 - loss64)
    print(f"[lm_head_nll_grad] tiny {kind}: loss {loss.item():.6f} fp64 {loss64:.6f}  |d| own {e_own:.3e}  fp16 torch {e_16:.3e}")
    worst = 0.0
    lines = []
    for li, L in enumerate(model.model.layers):
        for nm, ql in layer_linears(L):
            assert ql.oweight.grad is not None and ql.oweight.grad.dtype == F32, (li, nm)
            ref = g64[li][nm]
            own = ((ql.oweight.grad.to(F64) / SCALE - ref).norm() / ref.norm()).item()
            t16 = ((g16[li][nm] - ref).norm() / ref.norm()).item()
            worst = max(worst, own / t16)
            lines.append(f"{li}.{nm} {own:.2e}/{t16:.2e}")
    print(f"[lm_head_nll_grad] tiny {kind}: rel L2 error of d(oweight), own / fp16 torch: " + "  ".join(lines))
    print(f"[lm_head_nll_grad] tiny {kind}: largest ratio own / fp16 torch = {worst:.3f} (allowed 2)")
    assert e_own <= 2 * e_16 + 2.0 ** -14, f"{kind}: loss error {e_own:.3e} > 2 x {e_16:.3e} + 2^-14"
    assert worst <= 2.0, f"{kind}: a d(oweight) is {worst:.2f} x the fp16 torch pass's error from fp64"


def _ulp16(v):
    return 2.0 ** (math.floor(math.log2(v)) - 10)


def test_train_then_use(tmp_path):
    """One SGD step lowers the loss; after end() scoring and a new engine see the trained weights, an engine built before
    refuses to run, and save_finetuned -> from_packed round-trips the trained slices."""
    import numpy as np
    from qeft_amd import causal_lm_loss, checkpoint, finetune, score
    from qeft_amd.llama import DecodeEngine, QuantLlama, layer_linears, prefill
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ckpt = os.path.join(golden, "ref_ckpt_llama2l.pth")
    model = QuantLlama.from_packed(ckpt, device=DEV, max_seq=64)
    tokens = torch.from_numpy(np.load(os.path.join(golden, "ref_ckpt_llama2l_io.npz"))["tokens"]).to(DEV)[:T_DOC]
    assert tokens.numel() >= 8
    stale = DecodeEngine(model, use_graph=False)
    params = finetune.begin(model)
    loss0 = causal_lm_loss(model, tokens)
    (loss0 * SCALE).backward()
    gmax = max(p.grad.abs().max().item() for p in params)
    assert gmax > 0 and all(torch.isfinite(p.grad).all() for p in params)
    with torch.no_grad():
        for p in params:                                               # plain SGD; the rate moves the largest entry by 5e-4
            p -= (5e-4 / gmax) * p.grad
        loss1 = causal_lm_loss(model, tokens).item()
    print(f"[lm_head_nll_grad] train: loss {loss0.item():.6f} -> {loss1:.6f} after one SGD step")
    assert loss1 < loss0.item()
    finetune.end(model)
    assert model._prefill_ops is None
    with torch.no_grad():
        sc = score(model, tokens)
        logits = prefill(model, tokens)
        hn = prefill(model, tokens, _head=False)
    _, mag = _ref64(hn, model.lm_head.weight)
    tol = _ulp16(logits.float().abs().max().item()) + 2 * (model.shape.hidden / 16 + 8) * 2.0 ** -23 * mag.max().item() + 2.0 ** -14
    used = -sc.logprob[:-1].mean().item()
    print(f"[lm_head_nll_grad] use: -mean logprob of score() {used:.6f} vs trained loss {loss1:.6f} (tol {tol:.3e})")
    assert abs(used - loss1) <= tol
    dense = model.forward_dense_reference(tokens)                      # the fp32 oweight parameters, dequantised as fp16
    assert (logits.float() - dense).abs().max().item() / dense.abs().max().item() < 5e-3
    with pytest.raises(RuntimeError, match="build a new DecodeEngine"):
        stale.step()
    fresh = DecodeEngine(model, use_graph=False)
    got = fresh.teacher_forced_logits(tokens)
    assert (got.float() - logits.float()[-got.shape[0]:]).abs().max().item() <= 2e-2 * logits.float().abs().max().item()
    path = checkpoint.save_finetuned(model, ckpt, str(tmp_path / "ft"))
    again = QuantLlama.from_packed(path, device=DEV, max_seq=64)
    for L0, L1 in zip(model.model.layers, again.model.layers):
        for (nm, a), (_, b) in zip(layer_linears(L0), layer_linears(L1)):
            assert b.oweight.dtype == F16 and torch.equal(a.oweight.detach().half(), b.oweight), nm
    changed = sum(not torch.equal(a.oweight.detach().half(), b.oweight)
                  for L0, L1 in zip(QuantLlama.from_packed(ckpt, device=DEV, max_seq=64).model.layers, again.model.layers)
                  for (_, a), (_, b) in zip(layer_linears(L0), layer_linears(L1)))
    assert changed > 0, "the step changed no outlier slice"
