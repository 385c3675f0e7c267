"""fp64 parity of the one-token attention (csrc/decode_attn.h, qeft_rope_attn_decode), the batched attention
(csrc/decode_batch.hip) and the reference-layout entry (qeft_single_query_attention) at long contexts, through the C ABI: every
boundary position of the one-token kernel's dealing of runs to waves on a 4096-row cache at the five head layouts, caches of
16384 and 32768 rows (the launch's > 64 KiB LDS branch), adversarial score patterns on the wave / split merges, ragged batched
launches whose short rows run with splits that hold no key, and the m-row kernel over a poisoned cache.

Every cache row the attention must not see is fp16 NaN before the launch: the rows past the context, the row of the token
itself (the kernels take it from the call's k / v), and whole slots no row of a batched launch serves.  A leaked row makes the
output NaN (0 x NaN in a P.V sum).  The reference is fp64 on the device over the caches as the launch left them, with the
kernels' own roundings and nothing else (q rotated in fp32, scaled by 128^-0.5 and rounded to fp16; the cached k rotated in fp32
and rounded to fp16); acceptance per head |got - ref| <= 2e-3 + 2e-3 max|ref| (tests/test_gpu_verify_shapes.py, _attn_close).
Each test prints the worst |got - ref| / (2e-3 + 2e-3 max|ref|) it saw (DESIGN.md section 4 records them)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 128
LAYOUTS = [(32, 32), (40, 40), (64, 8), (40, 8), (32, 1)]
SPLITS = (1, 2, 4, 8)
NAN16 = 0x7e00                  # the fp16 quiet NaN the caches are poisoned with


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from qeft_amd import _lib
    return _lib.lib(), _lib.check


def _rot(x, c, s):          # x [..., 128] fp32, c / s [..., 64]: neox-style rotary, as the kernels
    a, b = x[..., :64], x[..., 64:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def _bits(t):
    return t.view(torch.int16)


def _same_bits(a, b):
    """Bit equality (NaN == NaN of the same pattern)."""
    return torch.equal(_bits(a), _bits(b))


def _attn_close(got, ref, what):
    """tests/test_gpu_verify_shapes.py::_attn_close, and the worst error in units of the bound."""
    got = got.double().view(got.shape[0], -1, HD)
    ref = ref.view(got.shape)
    assert torch.isfinite(got).all(), what
    tol = 2e-3 + 2e-3 * ref.abs().amax(-1, keepdim=True)
    bad = (got - ref).abs() > tol
    assert not bad.any(), (what, (got - ref).abs().max().item(), bad.nonzero()[:4].tolist())
    return ((got - ref).abs() / tol).max().item()


def _to_ft(k):              # [..., max_seq, 128] -> the FasterTransformer key layout [..., 16, max_seq, 8]
    return k.view(*k.shape[:-1], 16, 8).transpose(-3, -2).contiguous()


def _from_ft(k):            # [..., 16, max_seq, 8] -> [..., max_seq, 128]
    return k.transpose(-3, -2).reshape(*k.shape[:-3], k.shape[-2], HD)


class _Slots:
    """n_slots caches [n_kv][max_seq][128] of one head layout, the rotary tables and the workspaces of the three kernels.
    k0 / v0 hold the random content; poison() rebuilds kc / vc from it with NaN wherever a launch must not look."""

    def __init__(self, heads, kv, max_seq, seed, n_slots=1):
        self.lib, self.ck = _lib()
        self.heads, self.kv, self.max_seq, self.n_slots = heads, kv, max_seq, n_slots
        self.g = torch.Generator(device=DEV).manual_seed(seed)
        self.nq = (heads + 2 * kv) * HD
        self.k0 = (torch.randn(n_slots, kv, max_seq, HD, generator=self.g, device=DEV) * 0.5).half()
        self.v0 = (torch.randn(n_slots, kv, max_seq, HD, generator=self.g, device=DEV) * 0.5).half()
        self.kc, self.vc = self.k0.clone(), self.v0.clone()
        self.ws1 = torch.zeros(max(self.lib.qeft_attn_workspace_bytes(heads, 8), 16) // 4, device=DEV)
        self.wsm = torch.zeros(max(self.lib.qeft_attn_m_workspace_bytes(heads, 8, 8), 16) // 4, device=DEV)
        self.wsb = torch.zeros(max(self.lib.qeft_attn_batch_workspace_bytes(heads, 8, 8), 16) // 4, device=DEV)
        self.tables(torch.randn(max_seq, 64, generator=self.g, device=DEV))
        self._keep = []

    def tables(self, ang):
        self.cos, self.sin = ang.cos().contiguous(), ang.sin().contiguous()

    def qkv(self, m):
        return torch.randn(m, self.nq, generator=self.g, device=DEV).half()

    def poison(self, ctx):
        """kc / vc <- k0 / v0 with NaN on rows >= ctx[s] of slot s (ctx[s] = 0: the whole slot)."""
        self.kc.copy_(self.k0)
        self.vc.copy_(self.v0)
        for s, p in enumerate(ctx):
            _bits(self.kc[s, :, p:]).fill_(NAN16)
            _bits(self.vc[s, :, p:]).fill_(NAN16)
        assert torch.isnan(self.kc[0, :, ctx[0]:]).all()

    def repoison(self, s, p0, p1):
        _bits(self.kc[s, :, p0:p1]).fill_(NAN16)
        _bits(self.vc[s, :, p0:p1]).fill_(NAN16)

    def out(self, m=1):
        return torch.full((m, self.heads * HD), float("nan"), dtype=torch.float16, device=DEV)

    # ---- launches --------------------------------------------------------------------------------------------------------
    def one(self, qkv, pos, split, out, form="pos", out_pos=None, slot=0, kc=None, vc=None, ft=False):
        """qeft_rope_attn_decode (ft: qeft_single_query_attention, kc in the reference's layout) on one row of qkv."""
        qp, pos_t = qkv.data_ptr(), torch.tensor([pos], dtype=torch.int32, device=DEV)
        kc = self.kc[slot] if kc is None else kc
        vc = self.vc[slot] if vc is None else vc
        if form == "pos":
            cs, sn, rows = self.cos, self.sin, self.max_seq
        else:                       # the engine's form: the row of this position, selected by the caller
            cs, sn, rows = self.cos[pos].clone(), self.sin[pos].clone(), 1
        self._keep += [pos_t, cs, sn]
        args = (qp, qp + self.heads * HD * 2, qp + (self.heads + self.kv) * HD * 2, cs.data_ptr(), sn.data_ptr(), rows,
                kc.data_ptr(), vc.data_ptr(), pos_t.data_ptr())
        if ft:
            self.ck(self.lib.qeft_single_query_attention(*args, out.data_ptr(), self.heads, self.kv, self.max_seq, _st()))
        else:
            self.ck(self.lib.qeft_rope_attn_decode(*args, out_pos.data_ptr() if out_pos is not None else None, out.data_ptr(),
                                                   self.ws1.data_ptr(), split, self.heads, self.kv, self.max_seq, _st()))

    def rows_m(self, qkv, m, pos, split, out, slot=0):
        """qeft_rope_attn_decode_m: m consecutive tokens of one sequence."""
        qp, pos_t = qkv.data_ptr(), torch.tensor([pos], dtype=torch.int32, device=DEV)
        self._keep.append(pos_t)
        self.ck(self.lib.qeft_rope_attn_decode_m(qp, qp + self.heads * HD * 2, qp + (self.heads + self.kv) * HD * 2, self.nq,
                                                 self.cos.data_ptr(), self.sin.data_ptr(), 64, self.max_seq,
                                                 self.kc[slot].data_ptr(), self.vc[slot].data_ptr(), pos_t.data_ptr(), None,
                                                 out.data_ptr(), self.heads * HD, self.wsm.data_ptr(), split, self.heads, self.kv,
                                                 self.max_seq, m, _st()))

    def batch(self, qkv, m, slots_d, pos_d, done_d, split, out, kc=None, vc=None):
        """qeft_rope_attn_decode_batch: m rows, row r in slot slots_d[r] at pos_d[slot]."""
        qp = qkv.data_ptr()
        kc = self.kc if kc is None else kc
        vc = self.vc if vc is None else vc
        self.ck(self.lib.qeft_rope_attn_decode_batch(qp, qp + self.heads * HD * 2, qp + (self.heads + self.kv) * HD * 2, self.nq,
                                                     self.cos.data_ptr(), self.sin.data_ptr(), 64, self.max_seq, kc.data_ptr(),
                                                     vc.data_ptr(), slots_d.data_ptr(), pos_d.data_ptr(),
                                                     done_d.data_ptr() if done_d is not None else None, None, out.data_ptr(),
                                                     self.heads * HD, self.wsb.data_ptr(), split, self.n_slots, self.heads, self.kv,
                                                     self.max_seq, m, _st()))

    def sync(self):
        torch.cuda.synchronize()
        self._keep.clear()

    # ---- references ------------------------------------------------------------------------------------------------------
    def reference(self, qkv, m, pos, kc=None, vc=None, slot=0):
        """fp64 causal attention of m consecutive rows over keys [0, pos + i] of the cache as the launch left it."""
        heads, grp = self.heads, self.heads // self.kv
        kc = self.kc[slot] if kc is None else kc
        vc = self.vc[slot] if vc is None else vc
        q = _rot(qkv[:m, :heads * HD].float().view(m, heads, HD), self.cos[pos:pos + m, None], self.sin[pos:pos + m, None])
        q = (q * HD ** -0.5).half().double()
        Lk = pos + m
        out = torch.empty(m, heads, HD, dtype=torch.float64, device=DEV)
        for h0 in range(0, heads, 8):           # 8 heads at a time: a 32768-key fp64 cache of all heads would be gigabytes
            hs = torch.arange(h0, min(h0 + 8, heads), device=DEV)
            K = kc[hs // grp, :Lk].double()
            V = vc[hs // grp, :Lk].double()
            sc = torch.einsum("mhd,hld->hml", q[:, hs], K)
            mask = torch.arange(Lk, device=DEV)[None, :] > (pos + torch.arange(m, device=DEV))[:, None]
            sc = sc.masked_fill(mask[None], float("-inf"))
            out[:, hs] = torch.einsum("hml,hld->mhd", sc.softmax(-1), V)
        return out.reshape(m, heads * HD)

    def check_append(self, qkv, m, pos, k_before, v_before, kc=None, vc=None, slot=0):
        """Rows pos .. pos + m - 1: v the call's bit for bit, k within one fp16 unit of the fp32 rotary formula; every other
        element of either cache as it was before the launch, bit for bit (NaN included)."""
        heads, kv = self.heads, self.kv
        kc = self.kc[slot] if kc is None else kc
        vc = self.vc[slot] if vc is None else vc
        kn = qkv[:m, heads * HD:(heads + kv) * HD].float().view(m, kv, HD)
        kr = _rot(kn, self.cos[pos:pos + m, None], self.sin[pos:pos + m, None]).transpose(0, 1)
        vn = qkv[:m, (heads + kv) * HD:].view(m, kv, HD).transpose(0, 1)
        assert _same_bits(vc[:, pos:pos + m], vn.contiguous())
        dk = (kc[:, pos:pos + m].float() - kr).abs()
        assert (dk <= kr.abs() * 2.0 ** -10 + 2.0 ** -24).all(), dk.max().item()
        assert _same_bits(kc[:, :pos], k_before[:, :pos]) and _same_bits(kc[:, pos + m:], k_before[:, pos + m:])
        assert _same_bits(vc[:, :pos], v_before[:, :pos]) and _same_bits(vc[:, pos + m:], v_before[:, pos + m:])


# ---------------------------------------------------------------------------------------------------------------------
# a. the one-token kernel
# ---------------------------------------------------------------------------------------------------------------------
# run edges (15, 16); a position that leaves splits without a key (20: two runs); 64 S - 1 / 64 S for S = 1, 2, 4, 8 (the first
# wrap of run r -> wave r % 4S); 255 .. 257 (end of the unconditional prefetch, the engine's first switch); 1535 / 1536 (its
# second); the last row
POSITIONS = [0, 1, 15, 16, 20, 63, 64, 127, 128, 255, 256, 257, 511, 512, 1535, 1536, 4095]


def _one_token_position(A, pos, splits, qkv=None):
    """Every split x both rotary forms at one position over a freshly poisoned cache: against fp64, the forms bit-equal, the
    appended rows and the untouched rest of the cache.  The row at pos is NaN again before every launch."""
    qkv = A.qkv(1) if qkv is None else qkv
    A.poison([pos])
    k_before, v_before = A.kc[0].clone(), A.vc[0].clone()
    outs = {}
    for split in splits:
        for form in ("pos", "rows"):
            A.repoison(0, pos, pos + 1)
            o = A.out()
            A.one(qkv, pos, split, o, form)
            outs[split, form] = o
    perm = torch.randperm(A.heads * HD, generator=A.g, device=DEV).to(torch.int32)
    op = A.out()
    A.repoison(0, pos, pos + 1)
    A.one(qkv, pos, splits[-1], op, "rows", out_pos=perm)
    A.sync()
    A.check_append(qkv, 1, pos, k_before, v_before)
    ref = A.reference(qkv, 1, pos)
    worst = 0.0
    for split in splits:
        worst = max(worst, _attn_close(outs[split, "pos"], ref, (A.heads, A.kv, A.max_seq, pos, split)))
        assert torch.equal(outs[split, "pos"], outs[split, "rows"]), (A.heads, A.kv, pos, split)
    assert torch.equal(op[:, perm.long()], outs[splits[-1], "rows"]), (A.heads, A.kv, pos)
    return worst


@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_one_token_fp64_at_boundary_positions(heads, kv):
    A = _Slots(heads, kv, 4096, seed=heads * 11 + kv)
    worst = {}
    for pos in POSITIONS:
        worst[pos] = _one_token_position(A, pos, SPLITS)
    at = max(worst, key=worst.get)
    print(f"[attn-1] heads={heads:<2} kv={kv:<2} max_seq=4096 splits=1,2,4,8 positions={len(POSITIONS)} "
          f"worst err/bound={worst[at]:.3f} (pos {at})")
    del A
    torch.cuda.empty_cache()


@pytest.mark.parametrize("max_seq", [16384, 32768])
@pytest.mark.parametrize("heads,kv", [(64, 8), (32, 32)])
def test_one_token_fp64_large_cache(heads, kv, max_seq):
    """The upper half of the domain the ABI accepts: LDS of 74 832 / 140 368 bytes, above the 64 KiB a launch gets without
    hipFuncSetAttribute (14064 is the first max_seq of that branch, here a position).  The launch has to return 0 and match."""
    A = _Slots(heads, kv, max_seq, seed=heads + kv + max_seq)
    worst = {}
    for pos in (0, 255, 14064, max_seq - 1):
        worst[pos] = _one_token_position(A, pos, (1, 8))
    at = max(worst, key=worst.get)
    print(f"[attn-1] heads={heads:<2} kv={kv:<2} max_seq={max_seq} splits=1,8 positions=0,255,14064,{max_seq - 1} "
          f"worst err/bound={worst[at]:.3f} (pos {at})")
    del A
    torch.cuda.empty_cache()


def test_one_token_deterministic_at_4000_split_8():
    """Back-to-back launches without a host sync are bit-equal, with launches of other splits on the same workspace between."""
    A = _Slots(32, 32, 4096, seed=77)
    pos, qkv = 4000, A.qkv(1)
    A.poison([pos])
    rep = [A.out() for _ in range(3)]
    for o in rep:
        A.one(qkv, pos, 8, o, "rows")
    o2, o4, o1, last = A.out(), A.out(), A.out(), A.out()
    A.one(qkv, pos, 2, o2, "rows")
    A.one(qkv, pos, 4, o4, "rows")
    A.one(qkv, pos, 1, o1, "rows")
    A.one(qkv, pos, 8, last, "rows")
    A.sync()
    for o in rep[1:] + [last]:
        assert torch.equal(o, rep[0])
    ref = A.reference(qkv, 1, pos)
    for o, what in ((rep[0], 8), (o4, 4), (o2, 2), (o1, 1)):
        _attn_close(o, ref, ("interleaved", what))
    del A
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# b. adversarial scores, one-token and batched kernel
# ---------------------------------------------------------------------------------------------------------------------
ADV_POS = (1000, 4000)


def _sink_row(pos, split):
    """A key row in a wave of another split than the one that owns `pos`, in that wave's second run (run r -> wave r % 4S)."""
    last = pos // 16
    own = (last % (4 * split)) // 4
    js = 4 * split + 4 * ((own + 1) % split) + 1
    assert js < last and ((js % (4 * split)) // 4 != own or split == 1) and js // (4 * split) == 1
    return 16 * js + 7


@pytest.mark.parametrize("heads,kv", LAYOUTS)
@pytest.mark.parametrize("case", ["sink", "new_max", "equal", "first_only"])
@pytest.mark.parametrize("kernel", ["one", "batch"])
def test_adversarial_scores(kernel, case, heads, kv):
    """Score patterns where a wrong rescale or merge shows (the verify kernel's, tests/test_gpu_verify_shapes.py): "sink", a key
    ~35 nats above the rest in the second run of a wave of another split than the query's own; "new_max", the maximum is the
    appended key, scored from LDS; "equal", every visible key identical: the plain mean of the values; "first_only", key 0 is
    the sink, so at position 4000 seven of eight splits and fifteen of sixteen runs carry weights that underflow to zero
    against the head's maximum.  The values carry a ramp over the positions, so a dropped or double-counted run moves the
    result; rotary pair (0, 64) is left unrotated so that dimension 0 lines q and k up.  Slot i serves position ADV_POS[i]:
    the batched kernel takes both in one launch of two rows."""
    A = _Slots(heads, kv, 4096, seed=13 * heads + kv, n_slots=2)
    ramp = (torch.arange(A.max_seq, device=DEV, dtype=torch.float32) / 1024)[None, None, :, None]
    A.v0 = (A.v0.float() + ramp).half()
    ang = torch.randn(A.max_seq, 64, generator=A.g, device=DEV)
    ang[:, 0] = 0.0
    if case == "equal":
        ang.zero_()
        A.k0.copy_(A.k0[:, :, :1].clone().expand_as(A.k0))
    A.tables(ang)
    slots_d = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    pos_d = torch.tensor(ADV_POS, dtype=torch.int32, device=DEV)
    worst = 0.0
    for split in SPLITS:
        qkv = A.qkv(2)
        kq = qkv[:, heads * HD:(heads + kv) * HD].view(2, kv, HD)
        if case == "equal":
            kq.copy_(A.k0[:, :, 0])
        else:
            qkv[:, :heads * HD].view(2, heads, HD)[:, :, 0] = 8.0
            if case == "new_max":
                kq[:, :, 0] = 50.0
        A.poison(ADV_POS)
        for s, pos in enumerate(ADV_POS):
            if case == "sink":
                A.kc[s, :, _sink_row(pos, split), 0] = 50.0
            elif case == "first_only":
                A.kc[s, :, 0, 0] = 50.0
        k_before, v_before = A.kc.clone(), A.vc.clone()
        out = A.out(2)
        if kernel == "batch":
            A.batch(qkv, 2, slots_d, pos_d, None, split, out)
        else:
            for s, pos in enumerate(ADV_POS):
                A.one(qkv[s:s + 1], pos, split, out[s:s + 1], "rows" if split % 4 else "pos", slot=s)
        A.sync()
        for s, pos in enumerate(ADV_POS):
            A.check_append(qkv[s:s + 1], 1, pos, k_before[s], v_before[s], slot=s)
            ref = A.reference(qkv[s:s + 1], 1, pos, slot=s)
            if case == "equal":     # the reference itself against the closed form: the mean of the values
                mean = A.vc[s, :, :pos + 1].double().mean(1).repeat_interleave(heads // kv, 0).reshape(1, -1)
                assert (ref - mean).abs().max().item() < 1e-9
            worst = max(worst, _attn_close(out[s:s + 1], ref, (kernel, case, heads, kv, split, pos)))
    print(f"[attn-adv] {kernel:<5} {case:<10} heads={heads:<2} kv={kv:<2} positions=1000,4000 splits=1,2,4,8 worst err/bound={worst:.3f}")
    del A
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# c. the batched kernel, long and ragged
# ---------------------------------------------------------------------------------------------------------------------
B_MAX_SEQ = 4096
B_POSITIONS = [4095, 0, 1536, 17, 1535, 256, 37, 2047]      # row 6 is done; the split is the longest row's, short rows run with
B_DONE_ROW = 6                                              # splits that hold no key
B_SLOTS = [7, 2, 9, 0, 5, 3, 8, 1]                          # permuted, non-contiguous (slots 4 and 6 unused) of 10


@pytest.mark.parametrize("heads,kv", [(32, 32), (40, 40), (64, 8)])
def test_batched_long_ragged_fp64_and_one_token(heads, kv):
    """m = 1..8 rows x split 1/2/4/8: each row against fp64 over its own slot and against a one-token launch on a copy of that
    slot (V bit-equal, K within one unit, output within 4e-3, the bound of tests/test_gpu_batch.py); the slots no row of the
    launch serves (whole-slot NaN) and the done row's slot unchanged bit for bit; two identical launches bit-equal."""
    n_slots = 10
    A = _Slots(heads, kv, B_MAX_SEQ, seed=heads + 3 * kv, n_slots=n_slots)
    pos_tab = torch.full((n_slots,), 3, dtype=torch.int32)
    done = torch.zeros(n_slots, dtype=torch.int32)
    for r, s in enumerate(B_SLOTS):
        pos_tab[s] = B_POSITIONS[r]
    done[B_SLOTS[B_DONE_ROW]] = 1
    pos_d, done_d = pos_tab.to(DEV), done.to(DEV)
    slots_d = torch.tensor(B_SLOTS, dtype=torch.int32, device=DEV)
    qkv = A.qkv(8)
    refs, ones = {}, {}
    worst = worst1 = 0.0
    for m in range(1, 9):
        served = {B_SLOTS[r]: B_POSITIONS[r] for r in range(m) if r != B_DONE_ROW}
        A.poison([served.get(s, 0) for s in range(n_slots)])
        kb, vb = A.kc.clone(), A.vc.clone()                  # the caches before a launch of these m rows
        for split in SPLITS:
            runs = []
            for _ in range(2):
                kc, vc = kb.clone(), vb.clone()
                out = A.out(m)
                A.batch(qkv, m, slots_d, pos_d, done_d, split, out, kc, vc)
                runs.append((out, kc, vc))
            A.sync()
            (out, kc, vc), (out2, kc2, vc2) = runs
            assert torch.equal(out, out2) and _same_bits(kc, kc2) and _same_bits(vc, vc2), (m, split)
            for s in range(n_slots):
                if s not in served:
                    assert _same_bits(kc[s], kb[s]) and _same_bits(vc[s], vb[s]), (m, split, s)
            for r in range(m):
                s, p = B_SLOTS[r], B_POSITIONS[r]
                if r == B_DONE_ROW:
                    assert (out[r] == 0).all(), (m, split)
                    continue
                A.check_append(qkv[r:r + 1], 1, p, kb[s], vb[s], kc[s], vc[s])
                if r not in refs:
                    refs[r] = A.reference(qkv[r:r + 1], 1, p, kc[s], vc[s])
                worst = max(worst, _attn_close(out[r:r + 1], refs[r], (heads, kv, m, split, r, p)))
                if (r, split) not in ones:      # the one-token launch on a copy of the slot as it was
                    k1, v1, o1 = kb[s].clone(), vb[s].clone(), A.out()
                    A.one(qkv[r:r + 1], p, split, o1, kc=k1, vc=v1)
                    A.sync()
                    ones[r, split] = (k1[:, p].clone(), o1)
                    assert _same_bits(vc[s], v1), (m, split, r)
                    assert _same_bits(kc[s][:, :p], k1[:, :p]) and _same_bits(kc[s][:, p + 1:], k1[:, p + 1:]), (m, split, r)
                k1p, o1 = ones[r, split]
                dk = (kc[s][:, p].float() - k1p.float()).abs()
                assert (dk <= k1p.float().abs() * 2.0 ** -10 + 2.0 ** -24).all(), (m, split, r, dk.max().item())
                d1 = (out[r].float() - o1[0].float()).abs().max().item()
                assert d1 < 4e-3, (m, split, r, d1)
                worst1 = max(worst1, d1)
    print(f"[attn-b] heads={heads:<2} kv={kv:<2} max_seq={B_MAX_SEQ} m=1..8 splits=1,2,4,8 positions={B_POSITIONS} "
          f"worst err/bound={worst:.3f}, max|batched - one-token|={worst1:.2e}")
    del A, kb, vb, runs, kc, vc, kc2, vc2
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# d. the m-row kernel over a poisoned cache
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_m_row_ignores_rows_past_the_context(heads, kv):
    """The verify pass's attention at position 1000 with every cache row >= pos NaN before the launch (its own m rows
    included: they come from the call).  Its other coverage is tests/test_gpu_verify_shapes.py."""
    A = _Slots(heads, kv, 2048, seed=heads * 5 + kv)
    pos, worst = 1000, 0.0
    for m in (1, 5, 8):
        for split in (1, 8):
            qkv = A.qkv(m)
            A.poison([pos])
            k_before, v_before = A.kc[0].clone(), A.vc[0].clone()
            out = A.out(m)
            A.rows_m(qkv, m, pos, split, out)
            A.sync()
            A.check_append(qkv, m, pos, k_before, v_before)
            worst = max(worst, _attn_close(out, A.reference(qkv, m, pos), (heads, kv, m, split)))
    print(f"[attn-m-nan] heads={heads:<2} kv={kv:<2} pos=1000 m=1,5,8 splits=1,8 worst err/bound={worst:.3f}")
    del A
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# e. the reference-layout entry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,kv", [(32, 32), (64, 8)])
def test_single_query_attention_ft_layout_long(heads, kv):
    """qeft_single_query_attention: the one-token body with the key cache laid out [n_kv][16][max_seq][8], one block per head."""
    A = _Slots(heads, kv, 4096, seed=heads * 3 + kv)
    worst = 0.0
    for pos in (0, 255, 256, 4095):
        qkv = A.qkv(1)
        A.poison([pos])
        k_before, v_before = A.kc[0].clone(), A.vc[0].clone()
        outs = {}
        for form in ("pos", "rows"):
            kft, vc = _to_ft(k_before), v_before.clone()
            o = A.out()
            A.one(qkv, pos, 1, o, form, kc=kft, vc=vc, ft=True)
            outs[form] = (o, kft, vc)
        A.sync()
        o, kft, vc = outs["pos"]
        kc = _from_ft(kft)
        A.check_append(qkv, 1, pos, k_before, v_before, kc, vc)
        worst = max(worst, _attn_close(o, A.reference(qkv, 1, pos, kc, vc), (heads, kv, pos)))
        assert torch.equal(o, outs["rows"][0]) and _same_bits(kft, outs["rows"][1]) and _same_bits(vc, outs["rows"][2])
    print(f"[attn-ft] heads={heads:<2} kv={kv:<2} max_seq=4096 positions=0,255,256,4095 worst err/bound={worst:.3f}")
    del A
    torch.cuda.empty_cache()
