"""fp64 net under the three device paths `qeft_cuda.single_query_attention` ends in: qeft_single_query_attention_generic
(sqa_generic_kernel, csrc/decode_aux.hip: every head size but 128, optional ALiBi) and qeft_single_query_attention_alibi (the
one-token body of csrc/decode_attn.h with ALIBI, head size 128) through the C ABI, and the shim's host side (per-sample lengths,
the rotations it applies with torch ops, its argument errors).  The plain head-size-128 entry has its net in
tests/test_gpu_attn_long.py, which this file is modelled on.

One launch per case on caches filled directly: rows < pos hold randn * 0.5, every row >= pos of both caches is fp16 NaN (the
row of the token itself included: the kernels take it from the call's k / v) and `out` is NaN.  After the launch the caches equal,
bit for bit, the caches before it with row pos replaced by the call's (rotated) k and its v: rows < pos unchanged, rows > pos still
the poison, no stray store.  The reference is fp64 on the device over the caches as the launch left them, with the kernels' own
roundings and nothing else:
  generic kernel   q scaled by D^-0.5 in fp32 and not rounded; cached keys fp16; ALiBi adds double(float slope) * (p - pos)
  head size 128    q rotated, scaled by 128^-0.5 and rounded to fp16 (the rotation itself in fp64, one rounding)
  shim rotation    q / k rotated and rounded to fp16 (in fp64, one rounding), then the kernel's own step as above
Acceptance per head of width D: |got - ref| <= 2e-3 + 2e-3 max|ref| (tests/test_gpu_verify_shapes.py, _attn_close).  Each test
prints the worst |got - ref| / bound it saw (DESIGN.md section 4.4a-ref records them)."""
import pytest
import torch

import test_gpu_attn_long as AL
from test_gpu_attn_long import DEV, NAN16, _bits, _same_bits, _st

pytestmark = pytest.mark.gpu
GEN_HEAD_SIZES = [8, 16, 24, 40, 64, 80, 96, 112, 160, 192, 248, 256]
GEN_LAYOUTS = [(4, 4), (8, 2), (6, 1)]
SCALE128 = torch.tensor(0.08838834764831845, dtype=torch.float32).item()     # the head-size-128 kernel's fp32 constant, 1 / sqrt(128)


def _lib():
    from qeft_amd import _lib
    return _lib.lib(), _lib.check


def _to_ft(k):              # [..., max_seq, D] -> the FasterTransformer key layout [..., D/8, max_seq, 8]
    return k.view(*k.shape[:-1], k.shape[-1] // 8, 8).transpose(-3, -2).contiguous()


def _from_ft(k):            # [..., D/8, max_seq, 8] -> [..., max_seq, D]
    return k.transpose(-3, -2).reshape(*k.shape[:-3], k.shape[-2], k.shape[-3] * 8)


def _close(got, ref, D, what):
    """_attn_close with the head view taken at width D; returns the worst error in units of the bound."""
    got = got.double().reshape(-1, D)
    ref = ref.reshape(-1, D)
    assert torch.isfinite(got).all(), what
    tol = 2e-3 + 2e-3 * ref.abs().amax(-1, keepdim=True)
    err = (got - ref).abs()
    ratio = (err / tol).max().item()
    assert ratio <= 1.0, (what, err.max().item(), ratio)
    return ratio


def _std_slopes(heads):
    return (2.0 ** (-8.0 * torch.arange(1, heads + 1, dtype=torch.float32) / heads)).to(DEV)


def _attend64(qs, K, V, pos, slopes=None):
    """fp64 softmax(qs . K + slope (p - pos)) V, head by head: qs [H][D] fp64, K / V [n_kv][>= pos + 1][D] fp16."""
    heads, grp = qs.shape[0], qs.shape[0] // K.shape[0]
    K, V = K[:, :pos + 1].double(), V[:, :pos + 1].double()
    rel = torch.arange(pos + 1, device=DEV, dtype=torch.float64) - pos
    out = torch.empty_like(qs)
    for h in range(heads):
        sc = K[h // grp] @ qs[h]
        if slopes is not None:
            sc = sc + slopes[h].double() * rel
        out[h] = sc.softmax(0) @ V[h // grp]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a. the generic entry through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
class _Gen:
    """Caches [n_kv][max_seq][D] of random content (k0 / v0) and the launches of qeft_single_query_attention_generic on poisoned
    copies of them.  ramp: the values carry a ramp over the positions, so a dropped or double-counted position moves the result."""

    def __init__(self, kv, max_seq, D, seed, ramp=False):
        self.lib, self.ck = _lib()
        self.kv, self.max_seq, self.D = kv, max_seq, D
        self.g = torch.Generator(device=DEV).manual_seed(seed)
        self.k0 = (torch.randn(kv, max_seq, D, generator=self.g, device=DEV) * 0.5).half()
        v0 = torch.randn(kv, max_seq, D, generator=self.g, device=DEV) * 0.5
        if ramp:
            v0 += (torch.arange(max_seq, device=DEV, dtype=torch.float32) * (4.0 / max_seq))[None, :, None]
        self.v0 = v0.half()
        self._keep = []

    def qkv(self, heads):
        D = self.D
        return (torch.randn(heads, D, generator=self.g, device=DEV).half(), torch.randn(self.kv, D, generator=self.g, device=DEV).half(),
                torch.randn(self.kv, D, generator=self.g, device=DEV).half())

    def poisoned(self, ctx):
        """Copies of k0 / v0 with NaN on every row >= ctx."""
        kn, vc = self.k0.clone(), self.v0.clone()
        _bits(kn[:, ctx:]).fill_(NAN16)
        _bits(vc[:, ctx:]).fill_(NAN16)
        assert torch.isnan(kn[:, ctx:]).all() and torch.isnan(vc[:, ctx:]).all()
        return kn, vc

    def launch(self, q, k, v, pos, kft, vc, slopes=None):
        heads = q.shape[0]
        out = torch.full((heads, self.D), float("nan"), dtype=torch.float16, device=DEV)
        pos_t = torch.tensor([pos], dtype=torch.int32, device=DEV)
        self._keep += [pos_t, slopes]
        self.ck(self.lib.qeft_single_query_attention_generic(q.data_ptr(), k.data_ptr(), v.data_ptr(), kft.data_ptr(), vc.data_ptr(),
                                                             pos_t.data_ptr(), out.data_ptr(), heads, self.kv, self.max_seq, self.D,
                                                             slopes.data_ptr() if slopes is not None else None, _st()))
        return out

    def run(self, q, k, v, pos, slopes=None, kn=None, vb=None):
        """One launch at pos over freshly poisoned caches (or kn / vb), the cache checks and the fp64 comparison.
        Returns (out, kft, vc, worst error / bound)."""
        if kn is None:
            kn, vb = self.poisoned(pos)
        kft, vc = _to_ft(kn), vb.clone()
        out = self.launch(q, k, v, pos, kft, vc, slopes)
        torch.cuda.synchronize()
        self._keep.clear()
        what = (q.shape[0], self.kv, self.D, self.max_seq, pos)
        # row pos: the call's k (no rotary in this entry) and v bit for bit; every other element as before the launch
        kn[:, pos], vb[:, pos] = k, v
        assert _same_bits(_from_ft(kft), kn), what
        assert _same_bits(vc, vb), what
        return out, kft, vc, _close(out, self.reference(q, kft, vc, pos, slopes), self.D, what)

    def reference(self, q, kft, vc, pos, slopes=None):
        scale = torch.tensor(float(self.D), dtype=torch.float32, device=DEV).rsqrt()    # D^-0.5 in fp32
        return _attend64((q.float() * scale).double(), _from_ft(kft), vc, pos, slopes)


def _gen_positions(D, max_seq=4096):
    ng = max(256 // D, 1)
    cand = [0, 1, ng - 1, ng, ng + 1, 255, 256, 257, 511, 512, 513, 1000, 4095]
    return sorted({p for p in cand if 0 <= p < max_seq})


@pytest.mark.parametrize("heads,kv", GEN_LAYOUTS)
@pytest.mark.parametrize("D", GEN_HEAD_SIZES)
def test_generic_fp64_head_sizes_layouts_positions(D, heads, kv):
    """Every head size class of the P.V dealing (NG = 256 / D position classes, 256 - NG D idle threads) x the head layouts at the
    positions where a thread takes its first, second and third trip through the 256-strided loops, where the classes first hold
    one position each (NG - 1, NG, NG + 1) and the last row of the cache."""
    A = _Gen(kv, 4096, D, seed=D * 7 + heads)
    worst = {}
    for pos in _gen_positions(D):
        worst[pos] = A.run(*A.qkv(heads), pos)[3]
    at = max(worst, key=worst.get)
    print(f"[sqa-gen] D={D:<3} heads={heads} kv={kv} max_seq=4096 positions={len(worst)} worst err/bound={worst[at]:.3f} (pos {at})")


@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("max_seq", [16, 15360, 15376, 32768])
def test_generic_fp64_cache_lengths(max_seq, D):
    """The smallest cache the shim accepts; 15360 rows, exactly 64 KiB of LDS and no hipFuncSetAttribute call; 15376, the first
    length whose launch raises the kernel's dynamic-LDS limit; 32768, the ceiling (135 168 bytes).  Last row and the middle."""
    A = _Gen(2, max_seq, D, seed=max_seq + D)
    worst = {}
    for pos in (max_seq - 1, max_seq // 2):
        worst[pos] = A.run(*A.qkv(8), pos)[3]
    at = max(worst, key=worst.get)
    print(f"[sqa-gen-len] D={D:<3} heads=8 kv=2 max_seq={max_seq} positions={max_seq - 1},{max_seq // 2} "
          f"worst err/bound={worst[at]:.3f} (pos {at})")


@pytest.mark.parametrize("D", [24, 64, 160, 256])
def test_generic_alibi_fp64_and_zero_slopes(D):
    """The 2^(-8 i / H) slopes against fp64 (the low-slope heads are the ones a mis-scaled slope would pass a loose bound on),
    and all-zero slopes against the launch without slopes, bit for bit."""
    heads, kv = 8, 2
    A = _Gen(kv, 4096, D, seed=D + 31)
    slopes, zeros = _std_slopes(heads), torch.zeros(heads, device=DEV)
    worst = {}
    for pos in (0, 1, 257, 1000, 4095):
        q, k, v = A.qkv(heads)
        out, kft, vc, worst[pos] = A.run(q, k, v, pos, slopes)
        oz, kz, vz, _ = A.run(q, k, v, pos, zeros)
        on, kn, vn, _ = A.run(q, k, v, pos, None)
        assert _same_bits(oz, on) and _same_bits(kz, kn) and _same_bits(vz, vn), (D, pos)
        if pos >= 257:      # the bias is what shapes the result here: without it the output is another one
            assert not torch.equal(out, on), (D, pos)
    at = max(worst, key=worst.get)
    print(f"[sqa-gen-alibi] D={D:<3} heads=8 kv=2 max_seq=4096 positions=0,1,257,1000,4095 worst err/bound={worst[at]:.3f} (pos {at})")


def test_generic_alibi_slope_one_at_32768():
    """One head with slope 1.0 at the last row of a 32768-row cache: the far scores are -3e4 and their weights underflow to zero
    in the kernel's fp32 and in fp64 alike."""
    heads, kv, D, pos = 4, 2, 64, 32767
    A = _Gen(kv, 32768, D, seed=5, ramp=True)
    slopes = _std_slopes(heads)
    slopes[0] = 1.0
    worst = A.run(*A.qkv(heads), pos, slopes)[3]
    print(f"[sqa-gen-alibi] D=64  heads=4 kv=2 max_seq=32768 pos=32767 slope 1.0 on head 0 worst err/bound={worst:.3f}")


@pytest.mark.parametrize("D", [64, 160])
@pytest.mark.parametrize("max_seq", [4096, 32768])
@pytest.mark.parametrize("case", ["q_zero", "sink_0", "sink_255", "sink_256", "sink_before", "sink_self", "equal"])
def test_generic_adversarial_scores(case, max_seq, D):
    """q = 0: uniform weights, the mean of the values; a sink key 24 score units above the rest at position 0, 255, 256 (the last
    position of a thread's first trip and the first of its second), pos - 1 and pos itself (scored from the call's k); all keys
    equal.  The values carry a ramp over the positions."""
    heads, kv, pos = 8, 2, max_seq - 7
    A = _Gen(kv, max_seq, D, seed=max_seq + D + len(case), ramp=True)
    q, k, v = A.qkv(heads)
    big = 3.0 * D ** 0.5                # with q[0] = 8: 8 * big / sqrt(D) = 24
    if case == "q_zero":
        q.zero_()
    elif case == "equal":
        A.k0.copy_(A.k0[:, :1].clone().expand_as(A.k0))
        k = A.k0[:, 0].clone()
    else:
        q[:, 0] = 8.0
        if case == "sink_self":
            k[:, 0] = big
        else:
            A.k0[:, {"sink_0": 0, "sink_255": 255, "sink_256": 256, "sink_before": pos - 1}[case], 0] = big
    out, kft, vc, worst = A.run(q, k, v, pos)
    if case in ("q_zero", "equal"):     # the reference itself against the closed form
        mean = vc[:, :pos + 1].double().mean(1).repeat_interleave(heads // kv, 0)
        assert (A.reference(q, kft, vc, pos) - mean).abs().max().item() < 1e-9
    print(f"[sqa-gen-adv] {case:<11} D={D:<3} heads=8 kv=2 max_seq={max_seq} pos={pos} worst err/bound={worst:.3f}")


def test_generic_invariance():
    """Heads of one kv group with equal q rows give equal bits; a head's bits depend neither on n_heads, nor on the other heads'
    content, nor on what its group's first head (the block that appends) holds; an identical second launch is bit-identical."""
    kv, D, pos = 2, 80, 777
    A = _Gen(kv, 1024, D, seed=9)
    q, k, v = A.qkv(8)
    q[2], q[3], q[5] = q[1], q[1], q[1]                     # heads 1..3 of group 0, head 5 of group 1
    o1, k1, v1, _ = A.run(q, k, v, pos)
    assert _same_bits(o1[1], o1[2]) and _same_bits(o1[1], o1[3]) and not torch.equal(o1[1], o1[5])
    o2, k2, v2, _ = A.run(q, k, v, pos)                     # caches poisoned anew
    assert _same_bits(o1, o2) and _same_bits(k1, k2) and _same_bits(v1, v2)
    qb = q.clone()                                          # the group's first heads and two more heads hold other content
    qb[[0, 4, 2, 7]] = torch.randn(4, D, generator=A.g, device=DEV).half()
    ob = A.run(qb, k, v, pos)[0]
    for h in (1, 3, 5, 6):
        assert _same_bits(ob[h], o1[h]), h
    assert not torch.equal(ob[0], o1[0])
    qc = torch.stack([q[1], qb[2], q[6], q[7]])             # 4 heads on the same 2 kv heads: groups of 2
    oc = A.run(qc, k, v, pos)[0]
    assert _same_bits(oc[0], o1[1]) and _same_bits(oc[2], o1[6]) and _same_bits(oc[3], o1[7]) and _same_bits(oc[1], ob[2])


@pytest.mark.parametrize("pos", [-1, 1024])
def test_generic_position_guard_touches_nothing(pos):
    """sqa_generic_kernel returns before any access when *pos is outside [0, max_seq): out stays NaN and both caches keep their
    bits, poisoned rows and valid rows alike."""
    A = _Gen(2, 1024, 64, seed=3)
    q, k, v = A.qkv(8)
    kn, vb = A.poisoned(512)
    kft, vc = _to_ft(kn), vb.clone()
    out = A.launch(q, k, v, pos, kft, vc, _std_slopes(8))
    torch.cuda.synchronize()
    assert (_bits(out) == NAN16).all()
    assert _same_bits(_from_ft(kft), kn) and _same_bits(vc, vb)


# ---------------------------------------------------------------------------------------------------------------------
# b. the ALiBi entry at head size 128 through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
ALIBI_POSITIONS = (0, 255, 256, 4095)       # those of test_gpu_attn_long.py::test_single_query_attention_ft_layout_long


def _rot64(x, c, s):        # AL._rot in fp64: x [..., 128], c / s [64]
    a, b = x[..., :64], x[..., 64:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


@pytest.mark.parametrize("max_seq", [4096, 32768])
@pytest.mark.parametrize("heads,kv", [(32, 32), (64, 8), (40, 8)])
def test_alibi_128_fp64(heads, kv, max_seq):
    """qeft_single_query_attention_alibi with the 2^(-8 i / H) slopes against fp64, with the whole rotary table (tab_rows ==
    max_seq) and with the selected row (tab_rows == 1), bit-equal to each other; with all-zero slopes bit-equal to
    qeft_single_query_attention, output and caches."""
    HD = AL.HD
    A = AL._Slots(heads, kv, max_seq, seed=heads * 5 + kv + max_seq)
    slopes, zeros = _std_slopes(heads), torch.zeros(heads, device=DEV)
    worst = {}

    def launch(qkv, pos, kft, vc, sl, rows):
        qp, pos_t = qkv.data_ptr(), torch.tensor([pos], dtype=torch.int32, device=DEV)
        cs, sn = (A.cos, A.sin) if rows != 1 else (A.cos[pos].clone(), A.sin[pos].clone())
        o = A.out()
        A._keep += [pos_t, cs, sn]
        A.ck(A.lib.qeft_single_query_attention_alibi(qp, qp + heads * HD * 2, qp + (heads + kv) * HD * 2, cs.data_ptr(), sn.data_ptr(), rows,
                                                     kft.data_ptr(), vc.data_ptr(), pos_t.data_ptr(), o.data_ptr(), heads, kv, max_seq,
                                                     sl.data_ptr(), _st()))
        return o

    for pos in ALIBI_POSITIONS:
        qkv = A.qkv(1)
        A.poison([pos])
        k_before, v_before = A.kc[0], A.vc[0]
        kft, vc = _to_ft(k_before), v_before.clone()
        out = launch(qkv, pos, kft, vc, slopes, max_seq)
        A.sync()
        kc = _from_ft(kft)
        A.check_append(qkv, 1, pos, k_before, v_before, kc, vc)
        qr = _rot64(qkv[0, :heads * HD].double().view(heads, HD), A.cos[pos].double(), A.sin[pos].double())
        qs = (qr * SCALE128).half().double()
        worst[pos] = _close(out, _attend64(qs, kc, vc, pos, slopes), HD, (heads, kv, max_seq, pos))
        del kc
        # the selected-row form
        kft2, vc2 = _to_ft(k_before), v_before.clone()
        o2 = launch(qkv, pos, kft2, vc2, slopes, 1)
        A.sync()
        assert torch.equal(out, o2) and _same_bits(kft, kft2) and _same_bits(vc, vc2), (heads, kv, max_seq, pos)
        # zero slopes (row pos NaN again) against the plain entry
        _bits(kft2[:, :, pos]).fill_(NAN16)
        _bits(vc2[:, pos]).fill_(NAN16)
        oz = launch(qkv, pos, kft2, vc2, zeros, max_seq)
        kft3, vc3, op = _to_ft(k_before), v_before.clone(), A.out()
        A.one(qkv, pos, 1, op, "pos", kc=kft3, vc=vc3, ft=True)
        A.sync()
        assert torch.equal(oz, op) and _same_bits(kft2, kft3) and _same_bits(vc2, vc3), (heads, kv, max_seq, pos)
        if pos:
            assert not torch.equal(out, op), (heads, kv, max_seq, pos)
        del kft, vc, kft2, vc2, kft3, vc3
    at = max(worst, key=worst.get)
    print(f"[sqa-alibi128] heads={heads:<2} kv={kv:<2} max_seq={max_seq} positions=0,255,256,4095 tab_rows=max_seq,1 "
          f"worst err/bound={worst[at]:.3f} (pos {at})")
    del A
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# c. the shim: per-sample lengths, host rotation, argument errors
# ---------------------------------------------------------------------------------------------------------------------
BASE = 10000.0


def _rotate64(x, p, rot, neox):
    """The shim's rotation of the first `rot` dims at position p, in fp64: pairs (i, i + rot/2) (neox) or (2i, 2i + 1) (GPT-J),
    angle p * base^(-2i / rot)."""
    x = x.double()
    if rot == 0:
        return x
    half = rot // 2
    ang = float(p) * (1.0 / (BASE ** (torch.arange(0, half, dtype=torch.float64, device=DEV) * 2.0 / rot)))
    c, s = ang.cos(), ang.sin()
    o = x.clone()
    if neox:
        a, b = x[..., :half], x[..., half:rot]
        o[..., :half], o[..., half:rot] = a * c - b * s, b * c + a * s
    else:
        a, b = x[..., 0:rot:2], x[..., 1:rot:2]
        o[..., 0:rot:2], o[..., 1:rot:2] = a * c - b * s, b * c + a * s
    return o


def _ulps(a, b):
    """Distance of two fp16 tensors in units of the last place (finite values; -0 and +0 are the same number)."""
    def ordered(t):
        i = _bits(t.contiguous()).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (ordered(a) - ordered(b)).abs()


class _Shim:
    """B sequences with caches in the reference's layouts, poisoned from each sample's own length on."""

    def __init__(self, B, H, Hkv, D, L, lens, rot, neox, alibi, seed):
        self.B, self.H, self.Hkv, self.D, self.L, self.lens, self.rot, self.neox = B, H, Hkv, D, L, lens, rot, neox
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.kn = (torch.randn(B, Hkv, L, D, generator=g, device=DEV) * 0.5).half()
        self.vn = (torch.randn(B, Hkv, L, D, generator=g, device=DEV) * 0.5).half()
        for b, n in enumerate(lens):
            _bits(self.kn[b, :, n:]).fill_(NAN16)
            _bits(self.vn[b, :, n:]).fill_(NAN16)
        self.q = torch.randn(B, H, D, generator=g, device=DEV).half()
        self.k = torch.randn(B, Hkv, D, generator=g, device=DEV).half()
        self.v = torch.randn(B, Hkv, D, generator=g, device=DEV).half()
        self.slopes = _std_slopes(H) if alibi else None
        self.in_kernel = rot == 0 or (D == 128 and rot == D and neox)

    def call(self, rows, lens=None, timestep=0):
        """The shim on samples `rows` (a slice) over fresh copies of their caches: (out, k_cache, v_cache)."""
        import qeft_cuda
        kc, vc = _to_ft(self.kn[rows]), self.vn[rows].clone()
        out = qeft_cuda.single_query_attention(self.q[rows], self.k[rows], self.v[rows], kc, vc, lens, self.slopes, timestep,
                                               self.rot, BASE, self.neox)
        torch.cuda.synchronize()
        return out, kc, vc

    def rotated_k(self, b):
        return _rotate64(self.k[b], self.lens[b], self.rot, self.neox)

    def check_sample(self, b, out, kc, vc):
        """Sample b of a call's results: the caches bit for bit outside row pos, v's row the call's, the rotated k's row within one
        unit of the fp64 rotation and untouched beyond `rot`; the output against fp64.  Returns (error / bound, elements of the key
        row one unit off)."""
        D, p, rot = self.D, self.lens[b], self.rot
        what = (self.D, self.rot, self.neox, b, p)
        assert out.shape == (self.H, D) and out.dtype == torch.float16
        kc = _from_ft(kc)
        kexp, vexp = self.kn[b].clone(), self.vn[b].clone()
        vexp[:, p] = self.v[b]
        kexp[:, p] = kc[:, p]
        assert _same_bits(kc, kexp) and _same_bits(vc, vexp), what
        off = _ulps(kc[:, p], self.rotated_k(b).half())
        assert off.max().item() <= 1, (what, off.max().item())
        assert _same_bits(kc[:, p, rot:], self.k[b, :, rot:]), what
        qr = _rotate64(self.q[b], p, rot, self.neox)
        if self.in_kernel:          # one rounding, after the scale
            qs = (qr * SCALE128).half().double()
        elif D == 128:              # rounded by the shim, then scaled and rounded by the kernel (its rotary is the identity)
            qs = (qr.half().float() * torch.tensor(SCALE128, dtype=torch.float32, device=DEV)).half().double()
        else:                       # rounded by the shim; the generic kernel keeps the scaled q in fp32
            qs = (qr.half().float() * torch.tensor(float(D), dtype=torch.float32, device=DEV).rsqrt()).double()
        return _close(out, _attend64(qs, kc, vc, p, self.slopes), D, what), int((off == 1).sum().item())


@pytest.mark.parametrize("D,rot,neox,alibi", [(128, 128, True, False), (128, 64, True, False), (128, 128, False, False),
                                             (96, 32, False, True)])
def test_shim_ragged_lengths(D, rot, neox, alibi):
    """length_per_sample_ = (0, 300, L - 1): the host loop's pos pointer per sample and the per-sample rotation angles.  Each
    sample's output and caches equal, bit for bit, the B = 1 call with `timestep` set to its length, and meet the fp64 bound."""
    L, lens = 1024, (0, 300, 1023)
    S = _Shim(3, 8, 2, D, L, lens, rot, neox, alibi, seed=D + rot)
    out, kc, vc = S.call(slice(0, 3), torch.tensor(lens, dtype=torch.int32, device=DEV), timestep=17)
    worst, ones = 0.0, 0
    for b, n in enumerate(lens):
        o1, k1, v1 = S.call(slice(b, b + 1), None, timestep=n)
        assert _same_bits(out[b], o1[0]) and _same_bits(kc[b], k1[0]) and _same_bits(vc[b], v1[0]), (D, rot, neox, b)
        r, n1 = S.check_sample(b, out[b], kc[b], vc[b])
        worst, ones = max(worst, r), ones + n1
    print(f"[sqa-shim-ragged] D={D:<3} rot={rot:<3} {'neox ' if neox else 'gpt-j'} alibi={int(alibi)} lengths={lens} "
          f"worst err/bound={worst:.3f}, key elements one unit off {ones}")


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("style", ["neox-partial", "gptj-full", "gptj-partial"])
def test_shim_host_rotation(style, D):
    """The rotations the shim applies with torch ops in front of a launch without rotary: the cached key row at pos is the fp64
    rotation of the call's k rounded to fp16, within one unit per element, the dims >= rot the caller's bits."""
    rot, neox = {"neox-partial": (D // 2, True), "gptj-full": (D, False), "gptj-partial": (D // 2, False)}[style]
    S = _Shim(2, 8, 2, D, 1024, (777, 777), rot, neox, False, seed=D + len(style))
    out, kc, vc = S.call(slice(0, 2), None, timestep=777)
    worst, ones = 0.0, 0
    for b in range(2):
        r, n1 = S.check_sample(b, out[b], kc[b], vc[b])
        worst, ones = max(worst, r), ones + n1
    assert not torch.equal(_from_ft(kc)[:, :, 777, :rot], S.k[:, :, :rot])      # it was rotated at all
    print(f"[sqa-shim-rot] {style:<12} D={D:<3} rot={rot:<3} pos=777 worst err/bound={worst:.3f}, "
          f"key elements one unit off {ones} of {2 * 2 * rot}")


def test_shim_argument_errors():
    """The refusals of the shim that had no test: a head size that is no multiple of 8 or above 256, a cache length that is no
    multiple of 16, n_heads % n_kv_heads, a non-contiguous cache, length_per_sample_ of the wrong dtype or length."""
    import qeft_cuda

    def args(B=1, H=4, Hkv=2, D=64, L=32):
        return [torch.zeros(B, H, D, dtype=torch.float16, device=DEV), torch.zeros(B, Hkv, D, dtype=torch.float16, device=DEV),
                torch.zeros(B, Hkv, D, dtype=torch.float16, device=DEV), torch.zeros(B, Hkv, max(D // 8, 1), L, 8, dtype=torch.float16, device=DEV),
                torch.zeros(B, Hkv, L, D, dtype=torch.float16, device=DEV)]

    qeft_cuda.single_query_attention(*args(), None, None, 0)            # the base call is accepted
    for D in (12, 264):
        with pytest.raises(RuntimeError, match="head_dim"):
            qeft_cuda.single_query_attention(*args(D=D), None, None, 0)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        qeft_cuda.single_query_attention(*args(L=24), None, None, 0)
    with pytest.raises(RuntimeError, match="n_kv_heads"):
        qeft_cuda.single_query_attention(*args(H=4, Hkv=3), None, None, 0)
    a = args()
    a[3] = torch.zeros(1, 2, 8, 32, 16, dtype=torch.float16, device=DEV)[..., ::2]
    with pytest.raises(RuntimeError, match="contiguous"):
        qeft_cuda.single_query_attention(*a, None, None, 0)
    a = args()
    a[4] = torch.zeros(1, 2, 32, 128, dtype=torch.float16, device=DEV)[..., ::2]
    with pytest.raises(RuntimeError, match="contiguous"):
        qeft_cuda.single_query_attention(*a, None, None, 0)
    for lens in (torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV),
                 torch.zeros(1, dtype=torch.int32, device=DEV)):
        with pytest.raises(RuntimeError, match="length_per_sample_"):
            qeft_cuda.single_query_attention(*args(B=2), lens, None, 0)
    torch.cuda.synchronize()
