"""The training attention (csrc/attn_train.hip: qeft_attn_train_fwd, qeft_attn_train_bwd) through the C ABI, through
qeft_amd.attention.causal_attention and through finetune.causal_lm_loss(attn="own")  (DESIGN.md section 4.15).

Every launch is poisoned the way tests/test_gpu_prefill_attn.py does it: q, k, v are views of one fused [rows][(H + 2 Hkv) 128]
buffer that sits in the middle of a larger buffer of fp16 NaN; out, lse, dout, dq, dk, dv sit in NaN buffers of their own, the
outputs start as NaN and have NaN gaps between their rows; after a launch everything around the views is still NaN.  A row or a
byte that a launch must not read makes a result NaN.

Tolerances (u = 2^-24, the unit roundoff of fp32; SC = the fp32 value of 128^-0.5; r16(x) = 2^-10 |x| + 2^-24, one fp16 ulp of x
with fp16's subnormal step, which bounds |fp16(a) - fp16(b)| - |a - b| for a, b next to x):

  lse.   The scaled score of (row i, key j) is an MFMA chain of 128 exact products in fp32 and one multiplication:
         |error| <= E_ij = SC 129 u sum_d |q_id k_jd|   (section 4.13's E).  log-sum-exp moves by at most the largest move of
         an argument, so |lse - lse64| <= max_j E_ij + 2^-23 (|lse| + 4) + 2^-20 (1 + tiles): the second term is the roundings of
         m + logf(l) and logf itself, the third the relative error of l -- per 64-key tile one __expf per term (2^-21), the
         running sum and one rescale.

  Backward, element-wise against fp64 (test 2).  torch autograd has no place for a rounding in the middle of a gradient, so the
  reference writes the backward of softmax attention out in fp64 -- p = exp(s - lse), dV = P^T dO, dP = dO V^T, delta =
  rowsum(dO out), dS = p (dP - delta), dK = SC dS^T Q, dQ = SC dS K, with lse and out from the forward LAUNCH -- and applies the
  kernel's roundings and nothing else: P to fp16 before dV, dS to fp16 before dK and dQ, SC in fp32.  Without the two roundings
  the same formulas agree with torch.autograd in fp64 to 1e-9 (asserted in test 3).  The bound is the sum of the terms' absolute
  errors:
     p:      dp_ij  = p_ij (E_ij + 2 u (|s_ij| + |lse_i|) + 2^-21 + 2^-23 |s_ij - lse_i|)     score, the subtraction, __expf
     P16:    dP16   = dp + r16(p)
     dV:     sum_i dP16_ij |dO_id| + n u sum_i P16_ij |dO_id| + 2^-11 |dV| + 2^-25,  n = (H / Hkv) t  (the MFMA chain's length)
     dP:     129 u sum_d |dO_id V_jd|;     delta: 16 u sum_d |dO_id out_id|
     dS:     ddS    = dp |dP - delta| + p (ddP + ddelta) + 2 u |dS|;     dS16: ddS + r16(dS)
     dK:     SC (sum_i ddS16_ij |q_id| + n u sum_i |dS16_ij q_id|) + (u + 2^-11) |dK| + 2^-25
     dQ:     SC (sum_j ddS16_ij |k_jd| + t u sum_j |dS16_ij k_jd|) + (u + 2^-11) |dQ| + 2^-25
  all of it times 1.001 for the second-order terms.  dout is N(0, 1) 2^-4, what a loss-scaled step produces; one case runs it
  times 2^-12, where most of dS lies in fp16's subnormal range and the 2^-24 of r16 carries the bound.

  Backward against an independent fp16 route (test 3): plain torch -- fp16 matmuls, softmax in fp32 rounded to fp16, autograd,
  repeat_interleave under grouped queries.  For dq, dk, dv the relative L2 error from fp64 autograd is at most 2 x that route's
  own, plus one fp16 ulp of the tensor's RMS (2^-10 relative): section 4.14's margin against a route that rounds in more places.

Every test prints its worst error / bound ([attn_train] ...); DESIGN.md section 4.15 records them."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 128
BAND = 8192                      # NaN elements in front of and behind every operand
F16, F32, F64 = torch.float16, torch.float32, torch.float64
SC = float(torch.tensor(128 ** -0.5, dtype=torch.float32))
U = 2.0 ** -24
LAYOUTS = [(32, 32), (64, 8), (32, 1), (40, 8)]
LENGTHS = [1, 7, 64, 65, 129, 200, 257]     # one and several Q tiles, a partial last key block, idle waves, the 128-key block edge
IGNORE = -100


def _st():
    return torch.cuda.current_stream().cuda_stream


def _L():
    from qeft_amd import _lib
    return _lib, _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


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


class _Ops:
    """n_seq sequences of t rows on one head layout: the fused q|k|v buffer, dout, and (after fwd() / bwd()) out, lse, dq, dk, dv.
    pad: extra elements in every row stride (the second set of strides of the invariance tests)."""

    def __init__(self, heads, kv, n_seq, t, seed, pad=0, scale=1.0, dout_scale=2.0 ** -4, like=None, seq_of=None):
        self.heads, self.kv, self.n_seq, self.t, self.pad = heads, kv, n_seq, t, pad
        rows, W = n_seq * t, (heads + 2 * kv) * HD
        self.fused = _Banded(rows, W, W + pad)
        self.dout_b = _Banded(rows, heads * HD, heads * HD + pad)
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.fused.v[:] = (torch.randn(rows, W, generator=g, device=DEV) * scale).half()
        self.dout_b.v[:] = (torch.randn(rows, heads * HD, generator=g, device=DEV) * dout_scale).half()
        if like is not None:     # sequence seq_of[0] of `like` as this one's sequence seq_of[1]; the others hold other values
            a, b = seq_of
            self.fused.v[b * t:(b + 1) * t] = like.fused.v[a * t:(a + 1) * t]
            self.dout_b.v[b * t:(b + 1) * t] = like.dout_b.v[a * t:(a + 1) * t]
        self.q = self.fused.v[:, :heads * HD]
        self.k = self.fused.v[:, heads * HD:(heads + kv) * HD]
        self.v = self.fused.v[:, (heads + kv) * HD:]
        self.dout = self.dout_b.v
        self.out_b = self.lse_b = None

    def fwd(self):
        _lib, lib = _L()
        rows, H = self.n_seq * self.t, self.heads
        self.out_b = _Banded(rows, H * HD, H * HD + 64 + self.pad)
        self.lse_b = _Banded(rows, H, dtype=F32)
        _lib.check(lib.qeft_attn_train_fwd(self.q.data_ptr(), self.q.stride(0), self.k.data_ptr(), self.v.data_ptr(), self.k.stride(0),
                                           self.out_b.v.data_ptr(), self.out_b.stride, self.lse_b.v.data_ptr(), self.n_seq, self.t,
                                           H, self.kv, _st()))
        torch.cuda.synchronize()
        assert _lib.last_variant() == "attn_train_fwd"
        assert self.out_b.intact() and self.lse_b.intact() and self.fused.intact()
        self.out, self.lse = self.out_b.v, self.lse_b.v
        assert torch.isfinite(self.out).all() and torch.isfinite(self.lse).all()
        return self

    def bwd(self, dout=None, out=None, lse=None):
        _lib, lib = _L()
        rows, H, kv = self.n_seq * self.t, self.heads, self.kv
        dout = self.dout if dout is None else dout
        out = self.out if out is None else out
        lse = self.lse if lse is None else lse
        self.dq_b = _Banded(rows, H * HD, H * HD + 8 + self.pad)
        self.dk_b = _Banded(rows, kv * HD, kv * HD + 16 + self.pad)
        self.dv_b = _Banded(rows, kv * HD, kv * HD + 16 + self.pad)
        need = lib.qeft_attn_train_bwd_workspace_bytes(self.n_seq, self.t, H, kv)
        assert need == 4 * rows * H
        ws = _Banded(rows * H, 1, dtype=F32)
        _lib.check(lib.qeft_attn_train_bwd(self.q.data_ptr(), self.q.stride(0), self.k.data_ptr(), self.v.data_ptr(), self.k.stride(0),
                                           out.data_ptr(), out.stride(0), dout.data_ptr(), dout.stride(0), lse.data_ptr(),
                                           self.dq_b.v.data_ptr(), self.dq_b.stride, self.dk_b.v.data_ptr(), self.dv_b.v.data_ptr(),
                                           self.dk_b.stride, ws.v.data_ptr(), need, self.n_seq, self.t, H, kv, _st()))
        torch.cuda.synchronize()
        assert _lib.last_variant() == "attn_train_dq"            # the last of the three launches
        for b in (self.dq_b, self.dk_b, self.dv_b, ws, self.fused, self.dout_b):
            assert b.intact()
        self.dq, self.dk, self.dv = self.dq_b.v, self.dk_b.v, self.dv_b.v
        for x in (self.dq, self.dk, self.dv):
            assert torch.isfinite(x).all()
        return self

    def seq(self, x, b, heads):
        """[t, heads, 128] of sequence b of a [rows, heads * 128] operand."""
        return x[b * self.t:(b + 1) * self.t].reshape(self.t, heads, HD)


_CACHE = {}


def _ran(heads, kv, n_seq, t):
    """The random case of a shape, run forward and backward once and shared by the tests (never written afterwards)."""
    key = (heads, kv, n_seq, t)
    if key not in _CACHE:
        _CACHE[key] = _Ops(heads, kv, n_seq, t, seed=1000 * heads + 10 * kv + n_seq + 7 * t).fwd().bwd()
    return _CACHE[key]


# ---- fp64 references
def _heads_first(x, rep=1):
    x = x.double().permute(1, 0, 2)
    return x.repeat_interleave(rep, 0) if rep > 1 else x


def _lse64(q, k):
    """fp64 log-sum-exp [t, H] of one sequence and section 4.13's E: the largest score error a row can see."""
    T, H, _ = q.shape
    rep = H // k.shape[1]
    Q, K = _heads_first(q), _heads_first(k, rep)
    vis = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    s = (Q @ K.transpose(1, 2) * SC).masked_fill(~vis, float("-inf"))
    E = (SC * 129 * U * (Q.abs() @ K.abs().transpose(1, 2))).masked_fill(~vis, 0.0).amax(-1)
    return torch.logsumexp(s, -1).t(), E.t()


def _bwd64(q, k, v, out, lse, dout, rounded=True):
    """One sequence: (dq, dk, dv) in fp64 by the written-out backward with the kernel's roundings, and the bound of each (module
    docstring).  q, out, dout [t, H, 128], k, v [t, Hkv, 128] fp16, lse [t, H] fp32."""
    T, H, _ = q.shape
    Hkv = k.shape[1]
    rep = H // Hkv
    Q, K, V = _heads_first(q), _heads_first(k, rep), _heads_first(v, rep)
    dO, O, L = _heads_first(dout), _heads_first(out), lse.double().t()[:, :, None]
    vis = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    zero = torch.zeros((), dtype=F64, device=DEV)
    S = Q @ K.transpose(1, 2) * SC
    X = S - L
    p = torch.where(vis, torch.exp(X), zero)
    P16 = p.half().double() if rounded else p
    dVh = P16.transpose(1, 2) @ dO
    dP = dO @ V.transpose(1, 2)
    delta = (dO * O).sum(-1)[:, :, None]
    dS = p * (dP - delta)
    dS16 = dS.half().double() if rounded else dS
    dKh = SC * (dS16.transpose(1, 2) @ Q)
    dQ = SC * (dS16 @ K)
    grp = lambda x: x.view(Hkv, rep, T, HD).sum(1)
    dK, dV = grp(dKh), grp(dVh)

    r16 = lambda x: 2.0 ** -10 * x.abs() + 2.0 ** -24
    E = SC * 129 * U * (Q.abs() @ K.abs().transpose(1, 2))
    dp = p * (E + 2 * U * (S.abs() + L.abs()) + 2.0 ** -21 + 2.0 ** -23 * X.abs())
    dP16 = torch.where(vis, dp + r16(p), zero)
    n = rep * T
    bdV = grp(dP16.transpose(1, 2) @ dO.abs() + n * U * (P16.transpose(1, 2) @ dO.abs())) + 2.0 ** -11 * dV.abs() + 2.0 ** -25
    ddP = 129 * U * (dO.abs() @ V.abs().transpose(1, 2))
    ddelta = 16 * U * (dO.abs() * O.abs()).sum(-1)[:, :, None]
    ddS = dp * (dP - delta).abs() + p * (ddP + ddelta) + 2 * U * dS.abs()
    ddS16 = torch.where(vis, ddS + r16(dS), zero)
    bdK = grp(SC * (ddS16.transpose(1, 2) @ Q.abs() + n * U * (dS16.abs().transpose(1, 2) @ Q.abs()))) \
        + (U + 2.0 ** -11) * dK.abs() + 2.0 ** -25
    bdQ = SC * (ddS16 @ K.abs() + T * U * (dS16.abs() @ K.abs())) + (U + 2.0 ** -11) * dQ.abs() + 2.0 ** -25
    back = lambda x: x.permute(1, 0, 2)
    return (back(dQ), back(dK), back(dV)), (1.001 * back(bdQ), 1.001 * back(bdK), 1.001 * back(bdV))


def _check_bwd(o, b, tag):
    """Sequence b of a run case against _bwd64: asserts every element within its bound, returns the worst error / bound per tensor."""
    H, kv = o.heads, o.kv
    ref, bound = _bwd64(o.seq(o.q, b, H), o.seq(o.k, b, kv), o.seq(o.v, b, kv), o.seq(o.out, b, H), o.lse[b * o.t:(b + 1) * o.t],
                        o.seq(o.dout, b, H))
    worst = []
    for name, got, r, bd, hh in (("dq", o.dq, ref[0], bound[0], H), ("dk", o.dk, ref[1], bound[1], kv), ("dv", o.dv, ref[2], bound[2], kv)):
        ratio = ((o.seq(got, b, hh).double() - r).abs() / bd).max().item()
        assert ratio <= 1.0, f"{tag} seq {b}: {name} is {ratio:.3f} x its bound"
        worst.append(ratio)
    return worst


# ---- 1. forward
@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_forward_bits_of_the_prompt_attention_and_lse(heads, kv):
    """out: bit-equal, per sequence, to qeft_attn_prefill(start = 0) over a cache filled with the sequence's K / V.
    lse: |lse - lse64| <= max_j E_ij + 2^-23 (|lse| + 4) + 2^-20 (1 + tiles)   (module docstring)."""
    _lib, lib = _L()
    worst = 0.0
    for n_seq in (1, 3):
        for t in LENGTHS:
            o = _ran(heads, kv, n_seq, t)
            for b in range(n_seq):
                q, k, v = o.seq(o.q, b, heads), o.seq(o.k, b, kv), o.seq(o.v, b, kv)
                kc, vc = k.permute(1, 0, 2).contiguous(), v.permute(1, 0, 2).contiguous()
                qc = q.reshape(t, heads * HD).contiguous()
                want = torch.full((t, heads * HD), float("nan"), dtype=F16, device=DEV)
                _lib.check(lib.qeft_attn_prefill(qc.data_ptr(), heads * HD, kc.data_ptr(), vc.data_ptr(), t, want.data_ptr(), heads * HD,
                                                 0, t, heads, kv, _st()))
                torch.cuda.synchronize()
                assert torch.equal(_bits(o.out[b * t:(b + 1) * t]), _bits(want)), (heads, kv, n_seq, t, b)
                lse64, E = _lse64(q, k)
                bound = E + 2.0 ** -23 * (lse64.abs() + 4) + 2.0 ** -20 * (1 + (t + 63) // 64)
                ratio = ((o.lse[b * t:(b + 1) * t].double() - lse64).abs() / bound).max().item()
                assert ratio <= 1.0, (heads, kv, n_seq, t, b, ratio)
                worst = max(worst, ratio)
    print(f"[attn_train] forward ({heads},{kv}): out bit-equal to qeft_attn_prefill; lse worst error / bound = {worst:.4f}")


# ---- 2. backward, element-wise against fp64
@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_backward_elementwise_against_fp64(heads, kv, n_seq):
    """Every element of dq, dk, dv of every sequence within the bound of the module docstring."""
    worst = [0.0, 0.0, 0.0]
    for t in LENGTHS:
        o = _ran(heads, kv, n_seq, t)
        for b in range(n_seq):
            worst = [max(a, c) for a, c in zip(worst, _check_bwd(o, b, (heads, kv, n_seq, t)))]
    print(f"[attn_train] backward ({heads},{kv}) n_seq {n_seq}: worst error / bound  dq {worst[0]:.4f}  dk {worst[1]:.4f}  dv {worst[2]:.4f}")


def test_backward_small_dout_underflows_ds_within_bound():
    """dout 2^-12 smaller: dS sits in fp16's subnormal range, the 2^-24 step of r16 carries the bound."""
    o = _Ops(64, 8, 1, 200, seed=31, dout_scale=2.0 ** -16).fwd().bwd()
    worst = _check_bwd(o, 0, "small dout")
    assert o.dq.abs().max() > 0 and o.dv.abs().max() > 0
    print(f"[attn_train] backward, dout x 2^-12 (64,8) t 200: worst error / bound  dq {worst[0]:.4f}  dk {worst[1]:.4f}  dv {worst[2]:.4f}")


# ---- 3. backward against an independent fp16 route
def _autograd64(q, k, v, dout):
    T, H, _ = q.shape
    rep = H // k.shape[1]
    q, k, v = (x.double().requires_grad_(True) for x in (q, k, v))
    vis = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    s = torch.einsum("ihd,jhd->hij", q, k.repeat_interleave(rep, 1)) * SC
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
    o = torch.einsum("hij,jhd->ihd", p, v.repeat_interleave(rep, 1))
    o.backward(dout.double())
    return q.grad, k.grad, v.grad


def _route16(q, k, v, dout):
    """Plain torch in fp16: fp16 matmuls, softmax in fp32 rounded to fp16, autograd, repeat_interleave."""
    T, H, _ = q.shape
    rep = H // k.shape[1]
    q, k, v = (x.clone().requires_grad_(True) for x in (q, k, v))
    vis = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    kk, vv = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    s = (q.transpose(0, 1) @ kk.permute(1, 2, 0)) * SC                        # [H, T, T] fp16
    p = torch.softmax(s.float().masked_fill(~vis, float("-inf")), -1).half()
    o = (p @ vv.transpose(0, 1)).transpose(0, 1)
    o.backward(dout)
    return q.grad.double(), k.grad.double(), v.grad.double()


@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_backward_against_the_fp16_torch_route(heads, kv):
    """rel L2 error from fp64 autograd <= 2 x the fp16 torch route's own + 2^-10, for dq, dk, dv; and the written-out fp64
    backward of test 2, without its two roundings, is torch.autograd's gradient."""
    worst = [0.0, 0.0, 0.0]
    for n_seq, t in ((1, 65), (1, 257), (3, 200)):
        o = _ran(heads, kv, n_seq, t)
        for b in range(n_seq):
            q, k, v, dout = o.seq(o.q, b, heads), o.seq(o.k, b, kv), o.seq(o.v, b, kv), o.seq(o.dout, b, heads)
            ref = _autograd64(q, k, v, dout)
            lse64, _ = _lse64(q, k)
            out64 = torch.einsum("hij,jhd->ihd", torch.softmax((torch.einsum("ihd,jhd->hij", q.double(), k.double().repeat_interleave(heads // kv, 1)) * SC)
                                 .masked_fill(~torch.ones(t, t, dtype=torch.bool, device=DEV).tril(), float("-inf")), -1),
                                 v.double().repeat_interleave(heads // kv, 1))
            plain, _ = _bwd64(q, k, v, out64, lse64, dout, rounded=False)      # the written-out formulas on exact lse / out
            for a, r in zip(plain, ref):
                assert (a - r).abs().max().item() <= 1e-9 * max(1.0, r.abs().max().item())
            route = _route16(q, k, v, dout)
            for i, (name, got, hh) in enumerate((("dq", o.dq, heads), ("dk", o.dk, kv), ("dv", o.dv, kv))):
                own = ((o.seq(got, b, hh).double() - ref[i]).norm() / ref[i].norm()).item()
                r16 = ((route[i] - ref[i]).norm() / ref[i].norm()).item()
                allowed = 2 * r16 + 2.0 ** -10
                assert own <= allowed, f"({heads},{kv}) n_seq {n_seq} t {t} seq {b}: {name} rel L2 {own:.3e} > 2 x {r16:.3e} + 2^-10"
                worst[i] = max(worst[i], own / allowed)
    print(f"[attn_train] vs fp16 torch route ({heads},{kv}): worst rel L2 / allowed  dq {worst[0]:.3f}  dk {worst[1]:.3f}  dv {worst[2]:.3f}")


# ---- 4. invariance, bit for bit
@pytest.mark.parametrize("heads,kv,t", [(64, 8, 200), (32, 32, 129), (40, 8, 65)])
def test_a_sequence_does_not_depend_on_its_batch_or_on_strides(heads, kv, t):
    """One sequence alone, as b = 0 of 3 and as b = 2 of 3, at two sets of strides: out, lse, dq, dk, dv bit for bit."""
    base = _ran(heads, kv, 1, t)
    want = [_bits(x) for x in (base.out, base.lse, base.dq, base.dk, base.dv)]
    for b, pad in ((0, 0), (2, 0), (0, 256), (2, 256)):
        o = _Ops(heads, kv, 3, t, seed=90 + b + pad, pad=pad, like=base, seq_of=(0, b)).fwd().bwd()
        got = [_bits(x[b * t:(b + 1) * t]) for x in (o.out, o.lse, o.dq, o.dk, o.dv)]
        for name, g, w in zip(("out", "lse", "dq", "dk", "dv"), got, want):
            assert torch.equal(g, w), (heads, kv, t, b, pad, name)
    alone = _Ops(heads, kv, 1, t, seed=5, pad=512, like=base, seq_of=(0, 0)).fwd().bwd()
    for name, x, w in zip(("out", "lse", "dq", "dk", "dv"), (alone.out, alone.lse, alone.dq, alone.dk, alone.dv), want):
        assert torch.equal(_bits(x), w), (heads, kv, t, "alone, padded", name)
    print(f"[attn_train] invariance ({heads},{kv}) t {t}: alone = b 0 of 3 = b 2 of 3, two sets of strides, bit for bit")


@pytest.mark.parametrize("heads,kv", [(64, 8), (32, 32)])
def test_prefix_rule(heads, kv):
    """out / lse row i do not depend on t; dq rows [0, i] of a launch of t equal those of a launch of i + 1 whose dout / out /
    lse are the leading rows."""
    t = 257
    whole = _ran(heads, kv, 1, t)
    for n in (256, 200, 129, 128, 65, 1):
        part = _Ops(heads, kv, 1, n, seed=3)
        part.fused.v[:] = whole.fused.v[:n]
        part.dout_b.v[:] = whole.dout_b.v[:n]
        part.fwd()
        assert torch.equal(_bits(part.out), _bits(whole.out[:n])) and torch.equal(_bits(part.lse), _bits(whole.lse[:n])), n
        part.bwd()
        assert torch.equal(_bits(part.dq), _bits(whole.dq[:n])), n
    print(f"[attn_train] prefix ({heads},{kv}): out, lse, dq of rows [0, n) of t = 257 equal a launch of n rows, bit for bit")


# ---- 5. adversarial scores
@pytest.mark.parametrize("case", ["hot_block0", "hot_diagonal", "hot_last_diagonal", "all_equal"])
def test_adversarial_scores(case):
    """(64, 8), t = 200, as test_rescale_adversarial_scores: q[., 0] = 8 on every row, K[., 0] = 0 but on one key about +40 above
    the rest -- in the first block, on a diagonal mid-tile, on the last row's diagonal; and all-equal scores (K = 0).  Gradients
    stay finite and within test 2's bound."""
    heads, kv, t = 64, 8, 200
    o = _Ops(heads, kv, 1, t, seed=77, scale=0.25)
    o.q.view(t, heads, HD)[:, :, 0] = 8.0
    if case == "all_equal":
        o.k[:] = 0
    else:
        hot = {"hot_block0": 5, "hot_diagonal": 150, "hot_last_diagonal": 199}[case]
        o.k.view(t, kv, HD)[:, :, 0] = 0
        o.k.view(t, kv, HD)[hot, :, 0] = 40 * 128 ** 0.5 / 8
    o.fwd().bwd()
    lse64, E = _lse64(o.seq(o.q, 0, heads), o.seq(o.k, 0, kv))
    bound = E + 2.0 ** -23 * (lse64.abs() + 4) + 2.0 ** -20 * 5
    rl = ((o.lse.double() - lse64).abs() / bound).max().item()
    assert rl <= 1.0, (case, rl)
    worst = _check_bwd(o, 0, case)
    print(f"[attn_train] adversarial {case}: worst error / bound  lse {rl:.4f}  dq {worst[0]:.4f}  dk {worst[1]:.4f}  dv {worst[2]:.4f}")


# ---- 6. causal_attention under autograd
def test_causal_attention_autograd_equals_the_entries():
    """.grad of q, k, v through causal_attention equals the direct entry call bit for bit -- contiguous inputs, views of a fused
    buffer, and inputs whose last two dims are not dense; an input that needs no grad gets None; all four variants are seen."""
    from qeft_amd import _lib, causal_attention
    lib = _lib.lib()
    heads, kv, B, T = 8, 2, 2, 70
    base = _Ops(heads, kv, B, T, seed=61).fwd().bwd()
    assert _lib.last_variant() == "attn_train_dq"
    q4, k4, v4 = base.q.view(B, T, heads, HD), base.k.view(B, T, kv, HD), base.v.view(B, T, kv, HD)     # views of the fused rows
    dout = base.dout.reshape(B, T, heads, HD)
    want = [base.out.reshape(B, T, heads, HD), base.dq.reshape(B, T, heads, HD), base.dk.reshape(B, T, kv, HD),
            base.dv.reshape(B, T, kv, HD)]

    def run(q, k, v, need=(True, True, True)):
        q, k, v = (x.detach().requires_grad_(n) for x, n in zip((q, k, v), need))
        out = causal_attention(q, k, v)
        assert _lib.last_variant() == "attn_train_fwd"
        out.backward(dout)           # (on autograd's own thread: the variant name is per thread, the part calls below assert it)
        return out, q.grad, k.grad, v.grad

    for kind in ("fused views", "contiguous", "transposed heads", "odd k stride"):
        if kind == "fused views":
            q, k, v = q4, k4, v4
        elif kind == "contiguous":
            q, k, v = q4.contiguous(), k4.contiguous(), v4.contiguous()
        elif kind == "transposed heads":           # [B, H, T, 128] storage: the last two dims of the [B, T, H, 128] view are not dense
            q, k, v = (x.transpose(1, 2).contiguous().transpose(1, 2) for x in (q4, k4, v4))
            assert not q.is_contiguous()
        else:                                       # k and v at different row strides
            q, k = q4.contiguous(), k4.contiguous()
            v = torch.empty(B, T, kv * HD + 64, dtype=F16, device=DEV)[:, :, :kv * HD].view(B, T, kv, HD)
            v[:] = v4
        got = run(q, k, v)
        for name, g, w in zip(("out", "dq", "dk", "dv"), got, want):
            assert g is not None and g.shape == w.shape and torch.equal(_bits(g), _bits(w)), (kind, name)
    out, gq, gk, gv = run(q4, k4, v4, need=(True, False, True))
    assert gk is None and torch.equal(_bits(gq), _bits(want[1])) and torch.equal(_bits(gv), _bits(want[3]))
    out, gq, gk, gv = run(q4, k4, v4, need=(False, True, False))
    assert gq is None and gv is None and torch.equal(_bits(gk), _bits(want[2]))

    # the three backward launches one by one (qeft_attn_train_bwd_part): each names its kernel and leaves the bits of the whole entry
    need = lib.qeft_attn_train_bwd_workspace_bytes(B, T, heads, kv)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dq, dk, dv = (torch.full_like(x.contiguous(), float("nan")) for x in (base.dq, base.dk, base.dv))
    for part, name in enumerate(("attn_train_delta", "attn_train_dkv", "attn_train_dq")):
        _lib.check(lib.qeft_attn_train_bwd_part(base.q.data_ptr(), base.q.stride(0), base.k.data_ptr(), base.v.data_ptr(), base.k.stride(0),
                                                base.out.data_ptr(), base.out.stride(0), base.dout.data_ptr(), base.dout.stride(0),
                                                base.lse.data_ptr(), dq.data_ptr(), heads * HD, dk.data_ptr(), dv.data_ptr(), kv * HD,
                                                ws.data_ptr(), need, B, T, heads, kv, part, _st()))
        torch.cuda.synchronize()
        assert _lib.last_variant() == name
        if part == 0:
            assert torch.isnan(dq).all() and torch.isnan(dk).all() and torch.isnan(dv).all()
        if part == 1:
            assert torch.isnan(dq).all() and torch.equal(_bits(dk), _bits(base.dk)) and torch.equal(_bits(dv), _bits(base.dv))
    assert torch.equal(_bits(dq), _bits(base.dq))
    with pytest.raises(ValueError):
        causal_attention(q4, k4[:, :, :1].expand(B, T, 3, HD), v4[:, :, :1].expand(B, T, 3, HD))        # 8 % 3
    with pytest.raises(ValueError):
        causal_attention(q4[..., :64], k4[..., :64], v4[..., :64])
    print("[attn_train] causal_attention: grads equal the entries bit for bit on 4 input layouts; None for inputs without grad")


# ---- 7. model
def _dense_pass(model, dense, leaves, tok2, targets, dt):
    """tests/test_gpu_lm_head_nll_grad.py's dense pass (section 4.14), with k / v repeated under grouped queries: causal-LM mean NLL
    of tok2 [B, T] over dense weights; each linear's last n_out columns are leaves[li][name].  dt = F64: all of it in fp64.
    dt = F16: fp16 tensors and plain torch ops, rounded where causal_lm_loss rounds."""
    s = model.shape
    lo = dt == F16
    up = F32 if lo else F64
    B, T = tok2.shape
    rep = s.n_heads // s.n_kv_heads
    cos, sin = model.rope_cos[:T, None, :].to(up), model.rope_sin[:T, None, :].to(up)

    def rms(x, g):
        xf = x.to(up)
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + s.rms_eps) * g.to(up)).to(dt)

    def rope(x):
        a, b = x[..., :64].to(up), x[..., 64:].to(up)
        return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1).to(dt)

    def lin(x, li, name):
        leaf = leaves[li][name]
        W = torch.cat([dense[li][name][:, :-leaf.shape[1]].to(dt), leaf.to(dt)], dim=1)
        return x @ W.t()

    h = model.model.embed_tokens.weight[tok2.reshape(-1)].to(dt)
    for li, L in enumerate(model.model.layers):
        x = rms(h, L.input_layernorm.weight)
        q = rope(lin(x, li, "q_proj").view(B, T, s.n_heads, 128))
        k = rope(lin(x, li, "k_proj").view(B, T, s.n_kv_heads, 128))
        v = lin(x, li, "v_proj").view(B, T, s.n_kv_heads, 128)
        if rep != 1:
            k, v = k.repeat_interleave(rep, 2), v.repeat_interleave(rep, 2)
        a = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True)
        a = a.transpose(1, 2).reshape(B * T, s.hidden)[:, L.self_attn.o_proj.reorder_ids]
        h = h + lin(a, li, "o_proj")
        x = rms(h, L.post_attention_layernorm.weight)
        act = (torch.nn.functional.silu(lin(x, li, "gate_proj").to(up)) * lin(x, li, "up_proj").to(up)).to(dt)
        h = h + lin(act, li, "down_proj")
    hn = rms(h, model.model.norm.weight)
    logits = (hn @ model.lm_head.weight.to(dt).t()).to(up)
    return torch.nn.functional.cross_entropy(logits, targets.long(), ignore_index=IGNORE, reduction="mean")


LOSS_SCALE = 1024.0
T_DOC = 200
_MODELS = {}


def _trainable(which):
    """(model, tokens, labels, params, reference(batch)) of the GQA 4 / 2 model or the tiny model, made once."""
    if which in _MODELS:
        return _MODELS[which]
    from qeft_amd import finetune
    from qeft_amd.llama import LlamaShape, QuantLlama, layer_linears, tiny_shape
    shape = LlamaShape(512, 512, 2, 4, 2, 512, max_seq=256) if which == "gqa" else tiny_shape(max_seq=256)
    model = QuantLlama(shape, DEV, seed=6)
    g = torch.Generator().manual_seed(4)
    tokens = torch.randint(0, shape.vocab, (T_DOC,), generator=g).to(DEV)
    labels = tokens.clone()
    labels[torch.tensor([0, 1, 2, 10, 11, 30, 99, 100, 150, 199])] = IGNORE
    dense = model.dense_weights()                                       # before begin(): oweight is still the fp16 buffer
    ow = [{nm: ql.oweight.detach().clone() for nm, ql in layer_linears(L)} for L in model.model.layers]
    params = finetune.begin(model)
    refs = {}

    def reference(batch):
        if batch not in refs:
            tok2 = tokens.view(batch, -1)
            targets = finetune.shift_labels(tok2, labels.view(batch, -1)).reshape(-1)
            out = []
            for dt in (F64, F16):
                leaves = [{nm: v.to(F64 if dt == F64 else F32).requires_grad_(True) for nm, v in d.items()} for d in ow]
                loss = _dense_pass(model, dense, leaves, tok2, targets, dt)
                (loss * (LOSS_SCALE if dt == F16 else 1.0)).backward()
                grads = [{nm: (v.grad.to(F64) / (LOSS_SCALE if dt == F16 else 1.0)) for nm, v in d.items()} for d in leaves]
                out += [loss.item(), grads]
            refs[batch] = tuple(out)
        return refs[batch]
    _MODELS[which] = (model, tokens, labels, params, reference)
    return _MODELS[which]


@pytest.mark.parametrize("checkpoint", [True, False], ids=["checkpoint", "plain"])
@pytest.mark.parametrize("batch", [1, 2], ids=["T200", "B2xT100"])
@pytest.mark.parametrize("which", ["gqa", "tiny"])
def test_causal_lm_loss_with_own_attention(which, batch, checkpoint):
    """Section 4.14's criterion for attn="own": the loss error from an fp64 dense pass is at most 2 x that of the fp16 plain-torch
    dense pass + 2^-14, the relative L2 error of every d(oweight) at most 2 x that pass's own; and attn="sdpa" in the same
    process still gives the loss it gave before the attn="own" call."""
    from qeft_amd import causal_lm_loss
    from qeft_amd.llama import layer_linears
    model, tokens, labels, params, reference = _trainable(which)
    loss64, g64, loss16, g16 = reference(batch)
    tok = tokens.view(batch, -1) if batch > 1 else tokens
    lab = labels.view(batch, -1) if batch > 1 else labels
    with torch.no_grad():
        before = causal_lm_loss(model, tok, lab, checkpoint=False).item()
    for p in params:
        p.grad = None
    loss = causal_lm_loss(model, tok, lab, checkpoint=checkpoint, attn="own")
    assert loss.dtype == F32 and loss.dim() == 0
    (loss * LOSS_SCALE).backward()
    e_own, e_16 = abs(loss.item() - loss64), abs(loss16 - loss64)
    worst, lines = 0.0, []
    for li, L in enumerate(model.model.layers):
        for nm, ql in layer_linears(L):
            assert ql.oweight.grad is not None and ql.oweight.grad.dtype == F32, (li, nm)
            ref = g64[li][nm]
            own = ((ql.oweight.grad.to(F64) / LOSS_SCALE - ref).norm() / ref.norm()).item()
            t16 = ((g16[li][nm] - ref).norm() / ref.norm()).item()
            worst = max(worst, own / t16)
            lines.append(f"{li}.{nm} {own:.2e}/{t16:.2e}")
    kind = f"{which} {'checkpoint' if checkpoint else 'plain'} batch {batch}"
    print(f"[attn_train] model {kind}: loss {loss.item():.6f} fp64 {loss64:.6f}  |d| own {e_own:.3e}  fp16 torch {e_16:.3e}")
    print(f"[attn_train] model {kind}: rel L2 error of d(oweight), own / fp16 torch: " + "  ".join(lines))
    print(f"[attn_train] model {kind}: largest ratio own / fp16 torch = {worst:.3f} (allowed 2)")
    assert e_own <= 2 * e_16 + 2.0 ** -14, f"{kind}: loss error {e_own:.3e} > 2 x {e_16:.3e} + 2^-14"
    assert worst <= 2.0, f"{kind}: a d(oweight) is {worst:.2f} x the fp16 torch pass's error from fp64"
    with torch.no_grad():
        after = causal_lm_loss(model, tok, lab, checkpoint=False).item()
    assert after == before, (before, after)


def test_own_attention_launches_are_the_ones_that_run(monkeypatch):
    """causal_lm_loss(attn="own") reaches qeft_attn_train_fwd once per layer (twice under checkpointing: the recomputation
    reruns the forward entry) and qeft_attn_train_bwd once per layer; attn="sdpa" reaches neither."""
    from qeft_amd import _lib, causal_lm_loss
    model, tokens, labels, params, _ = _trainable("gqa")
    lib = _lib.lib()
    calls = []
    of, ob = lib.qeft_attn_train_fwd, lib.qeft_attn_train_bwd
    monkeypatch.setattr(lib, "qeft_attn_train_fwd", lambda *a: (calls.append("f"), of(*a))[1])
    monkeypatch.setattr(lib, "qeft_attn_train_bwd", lambda *a: (calls.append("b"), ob(*a))[1])
    n = model.shape.n_layers
    for ckpt, want_f in ((False, n), (True, 2 * n)):
        calls.clear()
        causal_lm_loss(model, tokens, labels, checkpoint=ckpt, attn="own").backward()
        assert calls.count("f") == want_f and calls.count("b") == n, (ckpt, calls)
    calls.clear()
    causal_lm_loss(model, tokens, labels, attn="sdpa").backward()
    assert calls == []
