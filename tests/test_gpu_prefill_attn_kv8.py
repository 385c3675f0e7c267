"""The prompt attention over an e4m3 cache (csrc/prefill_attn_kv8.hip, qeft_attn_prefill_kv8) through the C ABI, and the paths that
launch it: DecodeEngine.extend, llama.prefill(start=, chunk=) and BatchDecodeEngine.admit(chunk=) on kv_dtype="fp8".

The contract is bit-equality with what the project did before the kernel existed: qeft_attn_prefill over the transient fp16 image
cat(kv8_decode_rows(codes[:, :start], scales[:, :start]), the chunk's rows).  Next to it an fp64 reference that uses no kernel
and no decoder of the package (tests/kv8_ref.py's dequantiser), and the decoder alone seen through the kernel (output rows that
are one decoded V row each).  Every launch is poisoned: the cache rows >= start hold NaN codes under NaN scales, every operand --
q|k|v, the separate K / V rows, both code arrays, both scale arrays, out -- lies between bands of NaN that are checked after the
launch, and out starts as NaN."""
import pytest
import torch

import kv8_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 128
BAND = 4096                      # poison elements in front of and behind every operand

LAYOUTS = [(32, 32), (64, 8), (32, 1), (40, 8)]
SHAPES = [(0, 1), (0, 65), (0, 200), (17, 1), (63, 66), (64, 64), (130, 70), (1000, 56)]
# the decoder's table: two rows that hold all 254 non-NaN codes between them, under a scale that gives fp16 subnormals, an
# ordinary one, the largest a row of fp16 values can have, and 0; and a row of zeros
TABLE_SCALES = [2.0 ** -24 / 448, 0.0371, 65504.0 / 448, 0.0]
N_SPECIAL = 2 * len(TABLE_SCALES) + 1


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from qeft_amd import _lib
    return _lib.lib(), _lib.check


def _bits(t):
    return t.view(torch.int16)


class _Banded:
    """n elements of `dtype` between two bands of poison (NaN, or the e4m3 NaN code); still_poisoned() after a launch."""

    def __init__(self, n, dtype):
        self.raw = torch.empty(n + 2 * BAND, dtype=dtype, device=DEV)
        if dtype == torch.uint8:
            self.raw.fill_(kv8_ref.NAN8)
        else:
            self.raw.fill_(float("nan"))
        self.mid = self.raw[BAND:BAND + n]
        assert self.mid.data_ptr() % 16 == 0

    def still_poisoned(self):
        a, b = self.raw[:BAND], self.raw[-BAND:]
        if self.raw.dtype == torch.uint8:
            return bool((a == kv8_ref.NAN8).all() and (b == kv8_ref.NAN8).all())
        return bool(torch.isnan(a).all() and torch.isnan(b).all())


def _table_rows():
    """(codes uint8 [9][128], scales fp32 [9]) on the CPU."""
    lo = torch.arange(0, 128, dtype=torch.uint8)
    hi = torch.arange(128, 256, dtype=torch.int32).to(torch.uint8)
    lo[0x7f], hi[0x7f] = 0x00, 0x80                                    # the two NaN codes out
    assert len(set(lo.tolist()) | set(hi.tolist())) == 254
    rows = [c for _ in TABLE_SCALES for c in (lo, hi)] + [torch.zeros(128, dtype=torch.uint8)]
    scales = [s for s in TABLE_SCALES for _ in range(2)] + [0.0]
    return torch.stack(rows), torch.tensor(scales, dtype=torch.float32)


def _special_positions(start):
    """Nine distinct rows from the first to the last of the past."""
    return [i * (start - 1) // (N_SPECIAL - 1) for i in range(N_SPECIAL)]


class _Case:
    """One head layout and one (start, t): an e4m3 cache of kv_rows rows whose first `start` rows are quantised random fp16 rows
    (tests/kv8_ref.quant_rows) with the decoder's table rows among them, poison behind; t rows of q|k|v.  new_form "fused" takes
    the K / V rows as views of q|k|v (new_stride (heads + 2 kv) 128), "narrow" from buffers of their own (new_stride kv 128)."""

    def __init__(self, heads, kv, kv_rows, start, t, new_form, seed, specials=True):
        self.lib, self.ck = _lib()
        self.heads, self.kv, self.kv_rows, self.start, self.t = heads, kv, kv_rows, start, t
        g = torch.Generator(device=DEV).manual_seed(seed)
        n = kv * kv_rows
        self.b_kc, self.b_vc = _Banded(n * HD, torch.uint8), _Banded(n * HD, torch.uint8)
        self.b_ks, self.b_vs = _Banded(n, torch.float32), _Banded(n, torch.float32)
        self.kc, self.vc = self.b_kc.mid.view(kv, kv_rows, HD), self.b_vc.mid.view(kv, kv_rows, HD)
        self.ks, self.vs = self.b_ks.mid.view(kv, kv_rows), self.b_vs.mid.view(kv, kv_rows)
        for c, s in ((self.kc, self.ks), (self.vc, self.vs)):
            c.fill_(kv8_ref.NAN8)                                      # rows >= start keep this
            s.fill_(float("nan"))
            if start:
                c[:, :start], s[:, :start] = kv8_ref.quant_rows((torch.randn(kv, start, HD, generator=g, device=DEV) * 0.5).half())
        self.special = []
        if specials and start >= N_SPECIAL:
            codes, scales = _table_rows()
            self.special = _special_positions(start)
            pos = torch.tensor(self.special, device=DEV)
            self.vc[:, pos], self.vs[:, pos] = codes.to(DEV), scales.to(DEV)
            # K: a row of +-65504 takes the whole softmax of every query it meets, so those two stay on kv head 0
            mild = [i for i in range(N_SPECIAL) if scales[i] < 1.0]
            self.kc[:, pos[mild]], self.ks[:, pos[mild]] = codes[mild].to(DEV), scales[mild].to(DEV)
            self.kc[0, pos], self.ks[0, pos] = codes.to(DEV), scales.to(DEV)
        width = (heads + 2 * kv) * HD
        self.b_qkv = _Banded(t * width, torch.float16)
        self.qkv = self.b_qkv.mid.view(t, width)
        self.qkv.copy_(torch.randn(t, width, generator=g, device=DEV).half())
        self.operands = [self.b_kc, self.b_vc, self.b_ks, self.b_vs, self.b_qkv]
        if new_form == "fused":
            self.k_new, self.v_new = self.qkv[:, heads * HD:(heads + kv) * HD], self.qkv[:, (heads + kv) * HD:]
        else:
            self.b_kn, self.b_vn = _Banded(t * kv * HD, torch.float16), _Banded(t * kv * HD, torch.float16)
            self.k_new, self.v_new = self.b_kn.mid.view(t, kv * HD), self.b_vn.mid.view(t, kv * HD)
            self.k_new.copy_(self.qkv[:, heads * HD:(heads + kv) * HD])
            self.v_new.copy_(self.qkv[:, (heads + kv) * HD:])
            self.operands += [self.b_kn, self.b_vn]
        assert self.k_new.stride(0) == (width if new_form == "fused" else kv * HD)
        assert start == kv_rows or ((self.kc[:, start:] == kv8_ref.NAN8).all() and torch.isnan(self.vs[:, start:]).all())

    def _out(self):
        b = _Banded(self.t * self.heads * HD, torch.float16)
        return b, b.mid.view(self.t, self.heads * HD)

    def run(self):
        from qeft_amd import _lib
        b_out, out = self._out()
        assert torch.isnan(out).all()
        q = self.qkv
        self.ck(self.lib.qeft_attn_prefill_kv8(q.data_ptr(), q.stride(0), self.kc.data_ptr(), self.vc.data_ptr(), self.ks.data_ptr(),
                                               self.vs.data_ptr(), self.kv_rows, self.k_new.data_ptr(), self.v_new.data_ptr(),
                                               self.k_new.stride(0), out.data_ptr(), out.stride(0), self.start, self.t, self.heads,
                                               self.kv, _st()))
        torch.cuda.synchronize()
        assert _lib.last_variant() == "attn_prefill_kv8"
        for b in self.operands + [b_out]:
            assert b.still_poisoned()                                 # nothing was written around any operand
        assert torch.isfinite(out).all()
        return out

    def new_rows(self):
        """The chunk's K and V rows as the image holds them: [kv][t][128] fp16."""
        return (x.view(self.t, self.kv, HD).transpose(0, 1) for x in (self.k_new, self.v_new))

    def run_parent_route(self):
        """What llama._own_attention did on an fp8 cache before this kernel: the transient fp16 image and qeft_attn_prefill."""
        from qeft_amd.llama import kv8_decode_rows
        s, L = self.start, self.start + self.t
        kn, vn = self.new_rows()
        kimg = torch.cat([kv8_decode_rows(self.kc[:, :s], self.ks[:, :s]), kn], 1).contiguous()
        vimg = torch.cat([kv8_decode_rows(self.vc[:, :s], self.vs[:, :s]), vn], 1).contiguous()
        b_out, out = self._out()
        q = self.qkv
        self.ck(self.lib.qeft_attn_prefill(q.data_ptr(), q.stride(0), kimg.data_ptr(), vimg.data_ptr(), L, out.data_ptr(),
                                           out.stride(0), s, self.t, self.heads, self.kv, _st()))
        torch.cuda.synchronize()
        return out

    def reference(self):
        """fp64 [t, heads * 128] with the kernel's own roundings and nothing else (tests/test_gpu_prefill_attn.py, _Case.reference)
        over the past as tests/kv8_ref.py decodes it, rounded to fp16, and the chunk's fp16 rows."""
        s, t, L, rep = self.start, self.t, self.start + self.t, self.heads // self.kv
        kn, vn = self.new_rows()
        K = torch.cat([kv8_ref.dequant_rows(self.kc[:, :s], self.ks[:, :s]).half(), kn], 1).double()
        V = torch.cat([kv8_ref.dequant_rows(self.vc[:, :s], self.vs[:, :s]).half(), vn], 1).double()
        q = self.qkv[:, :self.heads * HD].view(t, self.heads, HD).double()
        out = torch.empty(t, self.heads, HD, dtype=torch.float64, device=DEV)
        scale = float(torch.tensor(128 ** -0.5, dtype=torch.float32))
        vis = torch.arange(L, device=DEV)[None, :] <= (s + torch.arange(t, device=DEV))[:, None]           # [t, L]
        for g in range(self.kv):
            sc = torch.einsum("thd,ld->htl", q[:, g * rep:(g + 1) * rep], K[g]) * scale
            sc = sc.masked_fill(~vis[None], float("-inf"))
            p = torch.exp(sc - sc.amax(-1, keepdim=True))
            o = torch.einsum("htl,ld->thd", p.half().double(), V[g]) / p.sum(-1).transpose(0, 1)[..., None]
            out[:, g * rep:(g + 1) * rep] = o
        return out.view(t, self.heads * HD)


def _kv_rows(start, t):
    return 256 if start + t <= 256 else 1056


# ---- 1. bit-equality with the route it replaces
@pytest.mark.parametrize("new_form", ["fused", "narrow"])
@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_bit_equal_to_the_fp16_kernel_over_the_decoded_image(heads, kv, new_form):
    """Every (start, t): no past at all, a past inside the first tile, a tile that straddles start ((17, 1), (63, 66), (130, 70),
    (1000, 56)), start on a tile boundary, one and two Q tiles, the context ending at the cache's last row ((1000, 56) on 1056
    rows).  No tolerance: torch.equal on the bits."""
    for start, t in SHAPES:
        c = _Case(heads, kv, _kv_rows(start, t), start, t, new_form, seed=heads + kv + start + t)
        assert bool(c.special) == (start >= N_SPECIAL)
        got, want = c.run(), c.run_parent_route()
        assert torch.equal(_bits(got), _bits(want)), (heads, kv, start, t, new_form,
                                                      int((_bits(got) != _bits(want)).sum()), "elements differ")


def test_scales_need_4_byte_alignment_only():
    """Scales that start 4 bytes past a 16-byte boundary (a slot's slice of [n_slots][n_kv][max_seq] at an odd row count lands
    there) are taken, and give the same bits."""
    heads, kv, start, t = 64, 8, 130, 70
    c = _Case(heads, kv, 256, start, t, "fused", seed=8)
    want = c.run()
    for name in ("ks", "vs"):
        b = _Banded(kv * 256 + 4, torch.float32)
        moved = b.mid[1:1 + kv * 256].view(kv, 256)
        moved.copy_(getattr(c, name))
        assert moved.data_ptr() % 16 == 4
        setattr(c, name, moved)
        c.operands.append(b)
    assert torch.equal(_bits(c.run()), _bits(want))


# ---- 2. fp64 parity, independent of every kernel and of the package's decoder
def test_parity_fp64():
    """|got - ref| <= 2e-3 + 2e-3 max|ref| per head, the bound of tests/test_gpu_prefill_attn.py and tests/test_gpu_attn_long.py."""
    heads, kv = 64, 8
    for start, t in ((63, 66), (130, 70), (1000, 56)):
        c = _Case(heads, kv, _kv_rows(start, t), start, t, "fused", seed=start, specials=False)
        got, ref = c.run().double().view(t, heads, HD), c.reference().view(t, heads, HD)
        tol = 2e-3 + 2e-3 * ref.abs().amax(-1, keepdim=True)
        err = (got - ref).abs()
        print(f"[prefill-attn-kv8 parity] ({start},{t}): worst error / bound = {(err / tol).max().item():.3f}")
        assert not (err > tol).any(), (start, t, err.max().item())


# ---- 3. the decoder seen through the kernel
@pytest.mark.parametrize("new_form", ["fused", "narrow"])
def test_output_rows_that_are_one_decoded_v_row(new_form):
    """(130, 70) on (64, 8).  Query row i < 9 is 8 on dimension 8 i and 0 elsewhere; K is 0 everywhere but one element per table
    row: K[table row i][8 i] = 40 sqrt(128) / 8, so row i's hot key scores 40 nats above every other key (all 0).  Then every
    other p is exp(-40) = 0 in fp16 and l = 1.0 in fp32 (at most 200 exp(-40) more), and the row's output is the decoded V row of
    table row i -- kv8_ref.dequant_rows(...).half(), not the package's decoder -- bit for bit, in every head, up to the sign of a
    zero.  What the tiles in front of the hot key's left in O is scaled by exp(-40): under 128 x 65504 x 4.3e-18 < 4e-11, a
    thousandth of half the smallest fp16 step, so no non-zero element moves; an element that decodes to +-0 comes out as that
    residue rounded to fp16, a zero of either sign (and without a residue as +0: O starts as +0 and +0 + 1.0 x -0 = +0 in the
    MFMA) -- the same in qeft_attn_prefill, whose output over the image is compared bit for bit at the end.  So: equal as
    numbers everywhere (fp16 == takes -0 for +0, and nothing else for anything else), and the bits wherever the row is not 0."""
    heads, kv, start, t = 64, 8, 130, 70
    c = _Case(heads, kv, 256, start, t, new_form, seed=3)
    pos = c.special
    assert len(pos) == N_SPECIAL and len(set(p // 64 for p in pos)) == 3          # the table rows lie in three tiles
    hot = 40 * 128 ** 0.5 / 8
    c.kc[:, :start] = 0
    c.ks[:, :start] = 1.0
    for i, p in enumerate(pos):
        c.kc[:, p, 8 * i] = 0x7e                                       # 448
        c.ks[:, p] = hot / 448
    c.k_new.zero_()
    q = c.qkv[:, :heads * HD].view(t, heads, HD)
    q.zero_()
    for i in range(N_SPECIAL):
        q[i, :, 8 * i] = 8.0
    if new_form == "fused":
        assert c.qkv[:, heads * HD:(heads + kv) * HD].abs().max().item() == 0
    out = c.run().view(t, heads, HD)
    want = kv8_ref.dequant_rows(c.vc[:, pos], c.vs[:, pos]).half()                 # [kv][9][128]
    assert (want.abs() > 0).any() and (want.abs().max().item() == 65504.0) and (want[want != 0].abs().min().item() < 6.2e-5)
    want = want.repeat_interleave(heads // kv, 0).transpose(0, 1).contiguous()    # [9][heads][128]
    got = out[:N_SPECIAL].contiguous()
    assert bool((got == want).all())
    assert torch.equal(_bits(got)[want != 0], _bits(want)[want != 0]) and int((want != 0).sum()) > 400 * heads
    assert torch.equal(_bits(c.run_parent_route().view(t, heads, HD)), _bits(out))


# ---- 4. the engines
T_PROMPT = 150


@pytest.fixture(scope="module")
def tiny():
    from qeft_amd.llama import QuantLlama, tiny_shape
    shape = tiny_shape(n_layers=2, hidden=256, inter=512, n_heads=2, vocab=384, max_seq=2048)
    model = QuantLlama(shape, DEV, seed=6)
    tokens = torch.randint(0, shape.vocab, (T_PROMPT,), generator=torch.Generator().manual_seed(3)).to(DEV)
    return model, tokens


_ORIG = []


class _Spy:
    """Counts the launches of both prompt attention entries and the calls of kv8_decode_rows, remembers the tensors of the last
    store_kv_rows (the chunk's K / V rows and the cache they went to), and with shim=True serves qeft_attn_prefill_kv8 the way the
    project did before the kernel: the transient fp16 image and qeft_attn_prefill."""

    def __init__(self, monkeypatch, shim=False):
        from qeft_amd import _lib, llama
        lib = _lib.lib()
        self.kv8, self.f16, self.decodes, self.last = [], [], 0, None
        if not _ORIG:                                                 # the first spy of a run finds nothing patched
            _ORIG.extend([lib.qeft_attn_prefill_kv8, lib.qeft_attn_prefill, llama.kv8_decode_rows, llama.store_kv_rows])
        kv8, f16, dec, store = _ORIG                                  # a second spy in one test replaces the first

        def on_store(lib_, k, v, kc, vc, ks, vs, T, start=0):
            self.last = (k, v, kc, vc, ks, vs)
            return store(lib_, k, v, kc, vc, ks, vs, T, start)

        def on_decode(codes, scales):
            self.decodes += 1
            return dec(codes, scales)

        def on_f16(*a):
            self.f16.append(a[7:9])
            return f16(*a)

        def on_kv8(*a):
            self.kv8.append(a[12:14])                                 # (start, t)
            if not shim:
                return kv8(*a)
            q, qs, kcp, vcp, ksp, vsp, kv_rows, knp, vnp, ns, out, os_, start, t, heads, kv, stream = a
            k, v, kc, vc, ks, vs = self.last
            assert (kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), kc.shape[1]) == (kcp, vcp, ksp, vsp, kv_rows)
            assert k.shape == v.shape == (t, kv, HD) and (k.data_ptr() == knp or not k.is_contiguous() or k.stride(0) != ns)
            kimg, vimg = (torch.cat([dec(c[:, :start], sc[:, :start]), x.transpose(0, 1)], 1).contiguous()
                          for c, sc, x in ((kc, ks, k), (vc, vs, v)))
            return on_f16(q, qs, kimg.data_ptr(), vimg.data_ptr(), start + t, out, os_, start, t, heads, kv, stream)
        monkeypatch.setattr(lib, "qeft_attn_prefill_kv8", on_kv8)
        monkeypatch.setattr(lib, "qeft_attn_prefill", on_f16)
        monkeypatch.setattr(llama, "kv8_decode_rows", on_decode)
        monkeypatch.setattr(llama, "store_kv_rows", on_store)


def _fp8_engine(model):
    from qeft_amd.llama import DecodeEngine
    e = DecodeEngine(model, use_graph=False, kv_dtype="fp8")
    for c in e.kc + e.vc:
        c.fill_(kv8_ref.NAN8)
    for s in e.ks + e.vs:
        s.fill_(float("nan"))
    return e


def _state(e, n):
    torch.cuda.synchronize()
    assert e.host_pos == n and int(e.pos.item()) == n
    for li in range(len(e.kc)):                                       # the rows behind keep their poison
        assert (e.kc[li][:, n:] == kv8_ref.NAN8).all() and torch.isnan(e.vs[li][:, n:]).all()
    return [c[:, :n].clone() for c in e.kc + e.vc] + [s[:, :n].contiguous().view(torch.int32).clone() for s in e.ks + e.vs]


def _run(case, model, tokens, e):
    from qeft_amd.llama import prefill
    if case == "extend":
        first = prefill(model, tokens[:90], e)
        assert e.host_pos == 90
        return first, e.extend(tokens[90:])
    return None, prefill(model, tokens, e, chunk={"chunk64": 64, "chunk5": 5}[case])


@pytest.mark.parametrize("case", ["extend", "chunk64", "chunk5"])
def test_engine_launches_the_kernel_and_matches_the_image_route(tiny, case, monkeypatch):
    """prefill(90) + extend(60), and the prompt in pieces of 64 and of 5 (under the 8 rows of the fused GEMM path: K / V rows of
    their own, new_stride n_kv 128), on an fp8 engine: the launch list of tests/test_gpu_prefill_attn.py's fp16 cases on the new
    entry, no image and no fp16 launch; then the same pass with the entry served by the image route: equal logits, codes, scales
    and position, bit for bit."""
    model, tokens = tiny
    L = model.shape.n_layers
    spy = _Spy(monkeypatch)
    e = _fp8_engine(model)
    first, got = _run(case, model, tokens, e)
    state = _state(e, T_PROMPT)
    want = {"extend": [(90, 60)], "chunk64": [(0, 64), (64, 64), (128, 22)], "chunk5": [(a, 5) for a in range(0, 150, 5)]}[case]
    assert spy.kv8 == [c for c in want for _ in range(L)], spy.kv8
    assert spy.f16 == [] and spy.decodes == 0
    assert torch.isfinite(got.float()).all()

    shim = _Spy(monkeypatch, shim=True)
    e2 = _fp8_engine(model)
    first2, got2 = _run(case, model, tokens, e2)
    state2 = _state(e2, T_PROMPT)
    assert shim.kv8 == spy.kv8 and len(shim.f16) == len(spy.kv8) and shim.f16 == shim.kv8
    assert torch.equal(_bits(got), _bits(got2)) and (first is None or torch.equal(_bits(first), _bits(first2)))
    assert len(state) == len(state2) and all(torch.equal(a, b) for a, b in zip(state, state2))


def test_an_fp16_engine_never_launches_it(tiny, monkeypatch):
    from qeft_amd.llama import DecodeEngine, prefill
    model, tokens = tiny
    spy = _Spy(monkeypatch)
    e = DecodeEngine(model, use_graph=False)
    prefill(model, tokens[:90], e)
    e.extend(tokens[90:])
    prefill(model, tokens, e, chunk=64)
    torch.cuda.synchronize()
    L = model.shape.n_layers
    assert spy.kv8 == [] and spy.decodes == 0
    assert spy.f16 == [c for c in [(90, 60), (0, 64), (64, 64), (128, 22)] for _ in range(L)]


def test_extend_allocates_nothing_that_grows_with_the_position(tiny):
    """The peak of extend(64 tokens) above what was allocated before it, at position 64 and at position 1920: equal.  (With the
    transient image the second needed 2 n_kv 1856 128 2 bytes more at the least: K and V rows [64, 1920) in fp16.)  What the
    rows between hold does not matter here: zero codes under zero scales."""
    model, tokens = tiny
    e = _fp8_engine(model)
    for t in e.kc + e.vc + e.ks + e.vs:
        t.zero_()
    from qeft_amd.llama import prefill
    prefill(model, tokens[:64], e)                                    # the first prompt also derives the model's fused operands
    peaks = []
    for pos in (64, 1920, 64, 1920):
        e.set_position(pos)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        logits = e.extend(tokens[64:128])
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        assert e.host_pos == pos + 64 and torch.isfinite(logits.float()).all()
        del logits
    print(f"[prefill-attn-kv8 memory] peak of extend(64) above the base at 64 / 1920 / 64 / 1920: {peaks}")
    assert peaks[0] == peaks[1] == peaks[2] == peaks[3] and peaks[0] > 0


def test_batch_admit_chunked_goes_through_it(tiny, monkeypatch):
    """BatchDecodeEngine on an fp8 engine: admit(chunk=32) of a 100-token prompt launches the new entry per layer and piece on
    the slot's caches (through _SlotView, unchanged), and gives the first token and the slot position of the same admission
    served by the image route; the two slots' rows are equal."""
    from qeft_amd.batch import BatchDecodeEngine
    from qeft_amd.llama import DecodeEngine
    model, _ = tiny
    L = model.shape.n_layers
    prompt = torch.randint(0, 384, (100,), generator=torch.Generator().manual_seed(10))
    be = BatchDecodeEngine(DecodeEngine(model, use_graph=True, kv_dtype="fp8"), max_batch=2, use_graph=False)
    assert be.ks is not None
    spy = _Spy(monkeypatch)
    s_new = be.admit(prompt, 40, chunk=32)
    torch.cuda.synchronize()
    assert spy.kv8 == [c for c in [(0, 32), (32, 32), (64, 32), (96, 4)] for _ in range(L)] and spy.f16 == [] and spy.decodes == 0
    shim = _Spy(monkeypatch, shim=True)
    s_old = be.admit(prompt, 40, chunk=32)
    torch.cuda.synchronize()
    assert s_old != s_new and shim.f16 == spy.kv8
    assert be.tokens(s_new) == be.tokens(s_old) and len(be.tokens(s_new)) == 1
    assert be.table.get(s_new).pos == be.table.get(s_old).pos == 100
    for li in range(L):
        for c in (be.kc[li], be.vc[li], be.ks[li].view(torch.int32), be.vs[li].view(torch.int32)):
            assert torch.equal(c[s_new][:, :100], c[s_old][:, :100])
