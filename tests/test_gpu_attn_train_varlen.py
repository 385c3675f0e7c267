"""The packed (variable-length) training attention (the varlen launches of csrc/attn_train.hip: qeft_attn_train_varlen_fwd,
qeft_attn_train_varlen_bwd) through the C ABI, through qeft_amd.attention.causal_attention_packed and through
finetune.causal_lm_loss(seq_lens=...)  (DESIGN.md section 4.18).

Every launch is poisoned the way tests/test_gpu_attn_train.py does it: q, k, v are views of one fused [R][(H + 2 Hkv) 128] buffer
that sits in the middle of a larger buffer of fp16 NaN; out, lse, dout, dq, dk, dv sit in NaN buffers of their own, the outputs
start as NaN and have NaN gaps between their rows; after a launch everything around the views is still NaN.  A row or a byte
that a launch must not read makes a result NaN.

The kernels are the fixed-length kernels' bodies behind another prologue, so the yardstick of tests 1 - 4 is equality of bits
with qeft_attn_train_fwd / _bwd on each sequence alone (n_seq = 1); those are under the fp64 net of tests/test_gpu_attn_train.py
at these lengths, and no tolerance is needed here.  A sequence's content depends on its id, its length and the layout alone,
so the same sequence can be packed in another place, order or stride and must keep its bits.

Test 5 (the step) compares three passes over the same sequences with the fp64 dense pass of tests/dense_ref.py: packed, the
same sequences right-padded to [B, T] with the padding labelled -100 (existing behaviour), and -- inside the bound -- nothing
else.  The packed pass's error from fp64 may be at most twice the padded pass's own plus one fp16 ulp of the tensor's RMS: for
the loss |e| <= 2 |e_padded| + 2^-10 |loss|, for every d(oweight) rel L2 <= 2 rel L2_padded + 2^-10 (section 4.14's margin for a
route that rounds elsewhere: the two passes run the same kernels over other row counts, so the GEMM tiers, the split of the head's
vocabulary sweep and the order of the d(oweight) row sums differ).  Every test prints what it measured ([attn_varlen] ...);
DESIGN.md section 4.18 records it."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 128
BAND = 8192                      # NaN elements in front of and behind every operand
F16, F32, F64 = torch.float16, torch.float32, torch.float64
IGNORE = -100
LENGTH_LISTS = [[1], [1, 1, 1], [64, 65], [127, 1, 128, 129], [200, 7, 257, 64, 3]]
LAYOUTS = [(4, 2), (2, 2), (8, 1)]
NAMES5 = ("out", "lse", "dq", "dk", "dv")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _L():
    from qeft_amd import _lib
    return _lib, _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def _prefix(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


class _Banded:
    """rows x width elements, rows `stride` apart, in the middle of a NaN buffer: .v is the view, intact() says that everything
    around it still is NaN."""

    def __init__(self, rows, width, stride=None, dtype=F16):
        self.rows, self.width, self.stride = rows, width, stride or width
        self.raw = torch.full((2 * BAND + rows * self.stride,), float("nan"), dtype=dtype, device=DEV)
        self.v = self.raw[BAND:BAND + rows * self.stride].view(rows, self.stride)[:, :width]
        assert self.v.data_ptr() % 16 == 0

    def intact(self):
        tmp = self.raw.clone()
        tmp[BAND:BAND + self.rows * self.stride].view(self.rows, self.stride)[:, :self.width] = float("nan")
        return bool(torch.isnan(tmp).all())


_CONTENT = {}


def _content(heads, kv, sid, n):
    """(fused q|k|v rows [n, (H + 2 Hkv) 128], dout rows [n, H 128]) of sequence `sid` of length n on a layout; made once."""
    key = (heads, kv, sid, n)
    if key not in _CONTENT:
        g = torch.Generator(device=DEV).manual_seed(100003 * heads + 1009 * kv + 7919 * sid + n)
        W = (heads + 2 * kv) * HD
        _CONTENT[key] = (torch.randn(n, W, generator=g, device=DEV).half(),
                         (torch.randn(n, heads * HD, generator=g, device=DEV) * 2.0 ** -4).half())
    return _CONTENT[key]


class _Packed:
    """Sequences `ids` (default 0 .. n - 1) of lengths `lens` packed on one head layout: the fused q|k|v buffer, dout, and (after
    fwd() / bwd()) out, lse, dq, dk, dv, all banded.  pad: extra elements in every row stride; nan_seq: that sequence's q, k, v and
    dout rows are NaN."""

    def __init__(self, heads, kv, lens, ids=None, pad=0, nan_seq=None):
        self.heads, self.kv, self.lens, self.pad = heads, kv, list(lens), pad
        self.ids = list(range(len(lens))) if ids is None else list(ids)
        self.cu = _prefix(lens)
        self.R = R = self.cu[-1]
        self.cu_c = (ctypes.c_int * len(self.cu))(*self.cu)
        W = (heads + 2 * kv) * HD
        self.fused = _Banded(R, W, W + pad)
        self.dout_b = _Banded(R, heads * HD, heads * HD + pad)
        for i, (sid, n) in enumerate(zip(self.ids, self.lens)):
            f, d = _content(heads, kv, sid, n)
            self.fused.v[self.cu[i]:self.cu[i + 1]] = f
            self.dout_b.v[self.cu[i]:self.cu[i + 1]] = d
        self.nan_seq = nan_seq
        if nan_seq is not None:
            self.fused.v[self.cu[nan_seq]:self.cu[nan_seq + 1]] = float("nan")
            self.dout_b.v[self.cu[nan_seq]:self.cu[nan_seq + 1]] = float("nan")
        self.q = self.fused.v[:, :heads * HD]
        self.k = self.fused.v[:, heads * HD:(heads + kv) * HD]
        self.v = self.fused.v[:, (heads + kv) * HD:]
        self.dout = self.dout_b.v

    def _finite_but_the_nan_sequence(self, x):
        ok = torch.isfinite(x).reshape(self.R, -1).all(1)
        if self.nan_seq is not None:
            ok[self.cu[self.nan_seq]:self.cu[self.nan_seq + 1]] = True
        return bool(ok.all())

    def fwd(self):
        _lib, lib = _L()
        R, H = self.R, self.heads
        self.out_b = _Banded(R, H * HD, H * HD + 64 + self.pad)
        self.lse_b = _Banded(R, H, dtype=F32)
        _lib.check(lib.qeft_attn_train_varlen_fwd(self.q.data_ptr(), self.q.stride(0), self.k.data_ptr(), self.v.data_ptr(),
                                                  self.k.stride(0), self.out_b.v.data_ptr(), self.out_b.stride, self.lse_b.v.data_ptr(),
                                                  self.cu_c, len(self.lens), H, self.kv, _st()))
        torch.cuda.synchronize()
        assert _lib.last_variant() == "attn_train_varlen_fwd"
        assert self.out_b.intact() and self.lse_b.intact() and self.fused.intact()
        self.out, self.lse = self.out_b.v, self.lse_b.v
        assert self._finite_but_the_nan_sequence(self.out) and self._finite_but_the_nan_sequence(self.lse)
        return self

    def _bwd_args(self, ws, need):
        return (self.q.data_ptr(), self.q.stride(0), self.k.data_ptr(), self.v.data_ptr(), self.k.stride(0), self.out.data_ptr(),
                self.out.stride(0), self.dout.data_ptr(), self.dout.stride(0), self.lse.data_ptr(), self.dq_b.v.data_ptr(),
                self.dq_b.stride, self.dk_b.v.data_ptr(), self.dv_b.v.data_ptr(), self.dk_b.stride, ws.v.data_ptr(), need, self.cu_c,
                len(self.lens), self.heads, self.kv)

    def bwd(self, parts=False):
        """parts: the three launches one by one through qeft_attn_train_varlen_bwd_part, each naming its kernel."""
        _lib, lib = _L()
        R, H, kv = self.R, self.heads, self.kv
        self.dq_b = _Banded(R, H * HD, H * HD + 8 + self.pad)
        self.dk_b = _Banded(R, kv * HD, kv * HD + 16 + self.pad)
        self.dv_b = _Banded(R, kv * HD, kv * HD + 16 + self.pad)
        need = lib.qeft_attn_train_varlen_bwd_workspace_bytes(self.cu_c, len(self.lens), H, kv)
        assert need == 4 * R * H
        ws = _Banded(R * H, 1, dtype=F32)
        if parts:
            for part, name in enumerate(("attn_train_delta", "attn_train_varlen_dkv", "attn_train_varlen_dq")):
                _lib.check(lib.qeft_attn_train_varlen_bwd_part(*self._bwd_args(ws, need), part, _st()))
                torch.cuda.synchronize()
                assert _lib.last_variant() == name
                if part < 2:
                    assert torch.isnan(self.dq_b.v).all()
                if part == 0:
                    assert torch.isnan(self.dk_b.v).all() and torch.isnan(self.dv_b.v).all()
        else:
            _lib.check(lib.qeft_attn_train_varlen_bwd(*self._bwd_args(ws, need), _st()))
            torch.cuda.synchronize()
            assert _lib.last_variant() == "attn_train_varlen_dq"          # the last of the three launches
        for b in (self.dq_b, self.dk_b, self.dv_b, ws, self.fused, self.dout_b, self.out_b, self.lse_b):
            assert b.intact()
        self.dq, self.dk, self.dv = self.dq_b.v, self.dk_b.v, self.dv_b.v
        for x in (self.dq, self.dk, self.dv):
            assert self._finite_but_the_nan_sequence(x)
        return self

    def five(self, i):
        """out, lse, dq, dk, dv of packed sequence i, as bits."""
        a, b = self.cu[i], self.cu[i + 1]
        return [_bits(x[a:b]) for x in (self.out, self.lse, self.dq, self.dk, self.dv)]


_ALONE = {}


def _alone(heads, kv, sid, n):
    """The five results, as bits, of sequence `sid` alone through the FIXED-length entries (n_seq = 1, t = n); made once."""
    key = (heads, kv, sid, n)
    if key in _ALONE:
        return _ALONE[key]
    _lib, lib = _L()
    f, dout = _content(heads, kv, sid, n)
    W, hw, kw = (heads + 2 * kv) * HD, heads * HD, kv * HD
    q, k, v = f[:, :hw], f[:, hw:hw + kw], f[:, hw + kw:]
    nan = lambda *s, dt=F16: torch.full(s, float("nan"), dtype=dt, device=DEV)
    out, lse, dq, dk, dv = nan(n, hw), nan(n, heads, dt=F32), nan(n, hw), nan(n, kw), nan(n, kw)
    _lib.check(lib.qeft_attn_train_fwd(q.data_ptr(), W, k.data_ptr(), v.data_ptr(), W, out.data_ptr(), hw, lse.data_ptr(), 1, n, heads, kv,
                                       _st()))
    need = lib.qeft_attn_train_bwd_workspace_bytes(1, n, heads, kv)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.qeft_attn_train_bwd(q.data_ptr(), W, k.data_ptr(), v.data_ptr(), W, out.data_ptr(), hw, dout.data_ptr(), hw,
                                       lse.data_ptr(), dq.data_ptr(), hw, dk.data_ptr(), dv.data_ptr(), kw, ws.data_ptr(), need, 1, n,
                                       heads, kv, _st()))
    torch.cuda.synchronize()
    assert _lib.last_variant() == "attn_train_dq"
    for x in (out, lse, dq, dk, dv):
        assert torch.isfinite(x).all()
    _ALONE[key] = [_bits(x) for x in (out, lse, dq, dk, dv)]
    return _ALONE[key]


def _same_as_alone(p, tag):
    for i, (sid, n) in enumerate(zip(p.ids, p.lens)):
        for name, got, want in zip(NAMES5, p.five(i), _alone(p.heads, p.kv, sid, n)):
            assert torch.equal(got, want), (tag, f"sequence {i} (id {sid}, {n} rows)", name)


# ---- 1. bit parity with the fixed-length kernels
@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_packed_bits_are_those_of_each_sequence_alone(heads, kv):
    """out, lse, dq, dk, dv of every sequence of a packed launch equal qeft_attn_train_fwd / _bwd on that sequence alone."""
    for lens in LENGTH_LISTS:
        _same_as_alone(_Packed(heads, kv, lens).fwd().bwd(), (heads, kv, lens))
    print(f"[attn_varlen] parity ({heads},{kv}): {len(LENGTH_LISTS)} length lists, every sequence bit-equal to the fixed-length "
          f"entries on it alone (out, lse, dq, dk, dv)")


def test_packed_bits_wide_layout_many_sequences_and_the_launches_one_by_one():
    """(64, 8) on the longest list; 128 one-row sequences (the cap) on (4, 2); and the three backward launches through
    qeft_attn_train_varlen_bwd_part, each naming its kernel, leave the whole entry's bits."""
    lens = [200, 7, 257, 64, 3]
    _same_as_alone(_Packed(64, 8, lens).fwd().bwd(), "(64,8)")
    _same_as_alone(_Packed(4, 2, [1] * 128).fwd().bwd(), "128 x 1")
    whole, parts = _Packed(8, 1, lens).fwd().bwd(), _Packed(8, 1, lens).fwd().bwd(parts=True)
    for i in range(len(lens)):
        for name, a, b in zip(NAMES5, whole.five(i), parts.five(i)):
            assert torch.equal(a, b), (i, name)
    print("[attn_varlen] parity (64,8) on [200,7,257,64,3] and (4,2) on 128 x [1]: bit-equal; delta / varlen_dkv / varlen_dq one by "
          "one = the whole entry")


# ---- 2. isolation
@pytest.mark.parametrize("victim", [0, 2, 4], ids=["first", "middle", "last"])
def test_a_nan_sequence_reaches_no_other(victim):
    """One sequence's q, k, v and dout are NaN: every other sequence's five results are finite and keep the clean run's bits."""
    heads, kv, lens = 4, 2, [200, 7, 257, 64, 3]
    clean = _Packed(heads, kv, lens).fwd().bwd()
    dirty = _Packed(heads, kv, lens, nan_seq=victim).fwd().bwd()          # fwd() / bwd() assert the others finite
    a, b = dirty.cu[victim], dirty.cu[victim + 1]
    assert torch.isnan(dirty.out[a:b]).all()                              # the poison was where it should be
    for i in range(len(lens)):
        if i != victim:
            for name, got, want in zip(NAMES5, dirty.five(i), clean.five(i)):
                assert torch.equal(got, want), (victim, i, name)
    print(f"[attn_varlen] isolation: sequence {victim} of {lens} all NaN, the other four bit-equal to the clean run")


# ---- 3. order and stride invariance
@pytest.mark.parametrize("heads,kv", [(4, 2), (8, 1)])
def test_order_and_strides_do_not_change_a_sequence(heads, kv):
    lens = [200, 7, 257, 64, 3]
    for order, pad in (([4, 3, 2, 1, 0], 0), ([2, 0, 4, 1, 3], 256), ([0, 1, 2, 3, 4], 512), ([1, 3], 8)):
        p = _Packed(heads, kv, [lens[j] for j in order], ids=order, pad=pad).fwd().bwd()
        _same_as_alone(p, (heads, kv, order, pad))
    print(f"[attn_varlen] invariance ({heads},{kv}): 4 orders / subsets of {lens} at 4 sets of strides, every sequence keeps its bits")


# ---- 4. causal_attention_packed under autograd
def test_causal_attention_packed_autograd_equals_the_entries():
    """.grad of q, k, v through causal_attention_packed equals the entry's bits -- views of the fused buffer, contiguous inputs and
    k / v at different row strides; an input that needs no grad gets None."""
    from qeft_amd import _lib, causal_attention_packed
    heads, kv, lens = 8, 2, [70, 1, 130, 33]
    base = _Packed(heads, kv, lens).fwd().bwd()
    R = base.R
    q3, k3, v3 = base.q.view(R, heads, HD), base.k.view(R, kv, HD), base.v.view(R, kv, HD)         # views of the fused rows
    dout = base.dout.reshape(R, heads, HD)
    want = [base.out.reshape(R, heads, HD), base.dq.reshape(R, heads, HD), base.dk.reshape(R, kv, HD), base.dv.reshape(R, kv, HD)]

    def run(q, k, v, need=(True, True, True)):
        q, k, v = (x.detach().requires_grad_(n) for x, n in zip((q, k, v), need))
        out = causal_attention_packed(q, k, v, lens)
        assert _lib.last_variant() == "attn_train_varlen_fwd"
        out.backward(dout)
        return out, q.grad, k.grad, v.grad

    for kind in ("fused views", "contiguous", "odd v stride"):
        if kind == "fused views":
            q, k, v = q3, k3, v3
        elif kind == "contiguous":
            q, k, v = q3.contiguous(), k3.contiguous(), v3.contiguous()
        else:
            q, k = q3.contiguous(), k3.contiguous()
            v = torch.empty(R, kv * HD + 64, dtype=F16, device=DEV)[:, :kv * HD].view(R, kv, HD)
            v[:] = v3
        for name, g, w in zip(("out", "dq", "dk", "dv"), run(q, k, v), want):
            assert g is not None and g.shape == w.shape and torch.equal(_bits(g), _bits(w)), (kind, name)
    out, gq, gk, gv = run(q3, k3, v3, need=(True, False, True))
    assert gk is None and torch.equal(_bits(gq), _bits(want[1])) and torch.equal(_bits(gv), _bits(want[3]))
    out, gq, gk, gv = run(q3, k3, v3, need=(False, True, False))
    assert gq is None and gv is None and torch.equal(_bits(gk), _bits(want[2]))
    with pytest.raises(ValueError):
        causal_attention_packed(q3, k3, v3, [70, 1, 130, 32])
    with pytest.raises(ValueError):
        causal_attention_packed(q3, k3[:, :1].expand(R, 3, HD), v3[:, :1].expand(R, 3, HD), lens)        # 8 % 3
    print("[attn_varlen] causal_attention_packed: out and grads equal the entries bit for bit on 3 input layouts; None for inputs "
          "without grad")


# ---- 5. the step
LOSS_SCALE = 1024.0
STEP_LENS = [70, 23, 129, 5]
_STEP = {}


def _step_model():
    """The tiny model of the existing loss tests (tiny_shape, 2 layers), four sequences of unequal length, their right-padded
    [B, T] form, and the fp64 dense pass over the padded form (tests/dense_ref.py): (loss64, grads64)."""
    if _STEP:
        return _STEP
    from dense_ref import dense_pass
    from qeft_amd import finetune
    from qeft_amd.llama import QuantLlama, layer_linears, tiny_shape
    model = QuantLlama(tiny_shape(max_seq=256), DEV, seed=6)
    g = torch.Generator().manual_seed(11)
    seqs = [torch.randint(0, model.shape.vocab, (n,), generator=g) for n in STEP_LENS]
    labs = [s.clone() for s in seqs]
    labs[0][torch.tensor([0, 1, 2, 10, 69])] = IGNORE
    labs[2][torch.tensor([5, 64, 128])] = IGNORE
    T = max(STEP_LENS)
    tok_pad = torch.zeros(len(seqs), T, dtype=torch.long)
    lab_pad = torch.full((len(seqs), T), IGNORE, dtype=torch.long)
    for i, (s_, l_) in enumerate(zip(seqs, labs)):
        tok_pad[i, :len(s_)], lab_pad[i, :len(s_)] = s_, l_
    dense = model.dense_weights()                                       # before begin(): oweight is still the fp16 buffer
    ow = [{nm: ql.oweight.detach().clone() for nm, ql in layer_linears(L)} for L in model.model.layers]
    params = finetune.begin(model)
    tok_pad, lab_pad = tok_pad.to(DEV), lab_pad.to(DEV)
    leaves = [{nm: v.to(F64).requires_grad_(True) for nm, v in d.items()} for d in ow]
    loss = dense_pass(model, dense, leaves, tok_pad, finetune.shift_labels(tok_pad, lab_pad).reshape(-1), F64)
    loss.backward()
    _STEP.update(model=model, params=params, tokens=torch.cat(seqs).to(DEV), labels=torch.cat(labs).to(DEV), tok_pad=tok_pad,
                 lab_pad=lab_pad, loss64=loss.item(), g64=[{nm: v.grad for nm, v in d.items()} for d in leaves])
    return _STEP


def _loss_and_grads(S, packed, **route):
    from qeft_amd import causal_lm_loss
    from qeft_amd.llama import layer_linears
    for p in S["params"]:
        p.grad = None
    if packed:
        loss = causal_lm_loss(S["model"], S["tokens"], S["labels"], seq_lens=STEP_LENS, **route)
    else:
        loss = causal_lm_loss(S["model"], S["tok_pad"], S["lab_pad"], **route)
    assert loss.dtype == F32 and loss.dim() == 0
    (loss * LOSS_SCALE).backward()
    grads = [{nm: ql.oweight.grad.to(F64) / LOSS_SCALE for nm, ql in layer_linears(L)} for L in S["model"].model.layers]
    return loss.item(), grads


@pytest.mark.parametrize("attn", ["own", "sdpa"])
@pytest.mark.parametrize("rope", ["torch", "fused"])
@pytest.mark.parametrize("glue", ["torch", "fused"])
def test_packed_step_against_the_padded_step_and_fp64(glue, rope, attn):
    """causal_lm_loss(tokens [R], labels, seq_lens=...) against the same sequences right-padded to [4, 129] (padding labelled
    -100) on the same route, both measured from the fp64 dense pass: loss |e| <= 2 |e_padded| + 2^-10 |loss|; every d(oweight)
    rel L2 <= 2 x the padded pass's + 2^-10 (module docstring).  attn="sdpa" packed is the per-sequence SDPA loop."""
    S = _step_model()
    route = dict(attn=attn, glue=glue, rope=rope)
    loss_pad, g_pad = _loss_and_grads(S, False, **route)
    loss_pk, g_pk = _loss_and_grads(S, True, **route)
    loss64, g64 = S["loss64"], S["g64"]
    e_pk, e_pad = abs(loss_pk - loss64), abs(loss_pad - loss64)
    kind = f"attn={attn} glue={glue} rope={rope}"
    print(f"[attn_varlen] step {kind}: loss packed {loss_pk:.6f} padded {loss_pad:.6f} fp64 {loss64:.6f}  |e| packed {e_pk:.3e}  "
          f"padded {e_pad:.3e}  allowed {2 * e_pad + 2.0 ** -10 * abs(loss64):.3e}")
    worst, lines = 0.0, []
    for li in range(len(g64)):
        for nm, ref in g64[li].items():
            own = ((g_pk[li][nm] - ref).norm() / ref.norm()).item()
            pad = ((g_pad[li][nm] - ref).norm() / ref.norm()).item()
            worst = max(worst, own / (2 * pad + 2.0 ** -10))
            lines.append(f"{li}.{nm} {own:.2e}/{pad:.2e}")
    print(f"[attn_varlen] step {kind}: rel L2 error of d(oweight), packed / padded: " + "  ".join(lines))
    print(f"[attn_varlen] step {kind}: largest rel L2 / (2 x padded + 2^-10) = {worst:.3f}")
    assert e_pk <= 2 * e_pad + 2.0 ** -10 * abs(loss64), f"{kind}: loss error {e_pk:.3e} > 2 x {e_pad:.3e} + 2^-10 |loss|"
    assert worst <= 1.0, f"{kind}: a d(oweight) is {worst:.2f} x its allowance"


def test_packed_step_checkpointing_and_the_launches_that_run(monkeypatch):
    """attn="own" with seq_lens reaches the varlen entries -- forward once per layer, twice under checkpointing (the recomputation
    reruns the forward entry), backward once -- and none of the fixed-length ones; the loss does not depend on checkpoint=."""
    from qeft_amd import _lib, causal_lm_loss
    S = _step_model()
    lib = _lib.lib()
    calls = []
    for nm, tag in (("qeft_attn_train_varlen_fwd", "vf"), ("qeft_attn_train_varlen_bwd", "vb"), ("qeft_attn_train_fwd", "f"),
                    ("qeft_attn_train_bwd", "b")):
        orig = getattr(lib, nm)
        monkeypatch.setattr(lib, nm, lambda *a, _o=orig, _t=tag: (calls.append(_t), _o(*a))[1])
    n = S["model"].shape.n_layers
    got = {}
    for ckpt, want_f in ((False, n), (True, 2 * n)):
        calls.clear()
        for p in S["params"]:
            p.grad = None
        loss = causal_lm_loss(S["model"], S["tokens"], S["labels"], seq_lens=STEP_LENS, checkpoint=ckpt, attn="own", glue="fused",
                              rope="fused")
        (loss * LOSS_SCALE).backward()
        assert calls.count("vf") == want_f and calls.count("vb") == n and "f" not in calls and "b" not in calls, (ckpt, calls)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in S["params"])
        got[ckpt] = loss.item()
    assert got[False] == got[True]
    print("[attn_varlen] step: varlen forward n / 2n times (plain / checkpoint), backward n times, no fixed-length launch; same loss")


# ---- 6. defaults unchanged
def test_without_seq_lens_nothing_changes():
    """seq_lens=None and no such argument are one call: the same loss and d(oweight) bits on a [B, T] batch, on the route with
    every own kernel (none of them uses float atomics, so two runs of one call agree bit for bit)."""
    from qeft_amd import causal_lm_loss
    S = _step_model()
    for route in (dict(attn="own", glue="fused", rope="fused"),):
        res = []
        for kw in (dict(), dict(seq_lens=None)):
            for p in S["params"]:
                p.grad = None
            loss = causal_lm_loss(S["model"], S["tok_pad"], S["lab_pad"], **route, **kw)
            (loss * LOSS_SCALE).backward()
            res.append([loss.detach().clone()] + [p.grad.clone() for p in S["params"]])
        for a, b in zip(*res):
            assert torch.equal(a, b), route
    print("[attn_varlen] defaults: causal_lm_loss(seq_lens=None) = causal_lm_loss() bit for bit on [4, 129]")
