"""The one-token attention (csrc/decode_attn.h, qeft_rope_attn_decode) where its K/V prefetch is requested before `pos` is known:
the smallest shapes at which the addressing of those early runs can go wrong.

A wave's early run i starts at row (i * 4 * n_split + wave) * 16 if that is inside the cache, else at row 0.  Caches of 16 and 64
rows put most (16: all but one) of the prefetched runs outside the cache -- the clamp; 512 rows hold them all, and positions 255 /
256 / 300 cross from the prefetched runs into the loop behind them.  Head layouts (2, 2) and (4, 1), n_split 1 / 2 / 4, with and
without an output map, and the three rotary forms of the launcher: the whole table, this position's rows in two buffers, and
this position's rows in one buffer [cos 64 | sin 64] (the decode engine's).  Every operand is a tensor of its own.

Before each launch every cache row at or beyond `pos` is fp16 NaN -- the row of the token itself included, which the kernel takes
from the call's k / v -- so a row the masks let through makes the output NaN.

Check 1: an fp64 reference written here (q and the new k rotated in fp32 and rounded to fp16 as the kernel does, the rest in
fp64), per head |got - ref| <= 2e-3 + 2e-3 max|ref|: the bound tests/test_gpu_attn_long.py applies to this kernel.
Check 2: the output bits equal those of the commit before the early prefetch for the same seeded inputs
(tests/golden/attn_early_prefetch_parent.npz, written once on the GPU by tests/golden/make_golden_attn_early.py with that
commit's library); forms and output maps give those same bits."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 128
NAN16 = 0x7e00
LAYOUTS = [(2, 2), (4, 1)]
MAX_SEQS = [16, 64, 512]
SPLITS = (1, 2, 4)
FORMS = ("table", "rows", "row_buffer")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_early_prefetch_parent.npz")


def positions(max_seq):
    ps = [0, 15, 16, 17, max_seq - 1] + ([255, 256, 300] if max_seq == 512 else [])
    return sorted({p for p in ps if p < max_seq})


def key(heads, kv, max_seq, pos, split):
    return f"h{heads}_kv{kv}_m{max_seq}_p{pos}_s{split}"


class Case:
    """Seeded operands of one (layout, cache size), each in a tensor of its own; numpy's legacy generator, so that the values do
    not depend on the torch build."""

    def __init__(self, heads, kv, max_seq):
        from qeft_amd import _lib
        self.lib, self.ck = _lib.lib(), _lib.check
        self.heads, self.kv, self.max_seq = heads, kv, max_seq
        rs = np.random.RandomState(7000 + heads * 64 + kv * 8 + max_seq)

        def dev(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)

        self.k0 = dev(rs.standard_normal((kv, max_seq, HD)) * 0.5, torch.float16)
        self.v0 = dev(rs.standard_normal((kv, max_seq, HD)) * 0.5, torch.float16)
        ang = rs.standard_normal((max_seq, 64))
        self.cos, self.sin = dev(np.cos(ang), torch.float32), dev(np.sin(ang), torch.float32)
        self.qkv = {p: [dev(rs.standard_normal(n * HD), torch.float16) for n in (heads, kv, kv)] for p in positions(max_seq)}
        self.perm = dev(rs.permutation(heads * HD), torch.int32)
        self.kc, self.vc = self.k0.clone(), self.v0.clone()
        self.ws = torch.zeros(max(self.lib.qeft_attn_workspace_bytes(heads, 8), 16) // 4, device=DEV)
        self._keep = []

    def poison(self, pos):
        self.kc.copy_(self.k0)
        self.vc.copy_(self.v0)
        self.kc[:, pos:].view(torch.int16).fill_(NAN16)
        self.vc[:, pos:].view(torch.int16).fill_(NAN16)

    def launch(self, pos, split, form, mapped):
        """One launch over a freshly poisoned cache; returns the output in natural order."""
        q, k, v = self.qkv[pos]
        self.poison(pos)
        pos_t = torch.tensor([pos], dtype=torch.int32, device=DEV)
        out = torch.full((self.heads * HD,), float("nan"), dtype=torch.float16, device=DEV)
        if form == "table":
            cs, sn, rows = self.cos, self.sin, self.max_seq
        elif form == "rows":
            cs, sn, rows = self.cos[pos].clone(), self.sin[pos].clone(), 1
        else:
            buf = torch.cat([self.cos[pos], self.sin[pos]]).contiguous()
            cs, sn, rows = buf[:64], buf[64:], 1
            assert sn.data_ptr() == cs.data_ptr() + 64 * 4
        self._keep += [pos_t, cs, sn]
        st = torch.cuda.current_stream().cuda_stream
        self.ck(self.lib.qeft_rope_attn_decode(q.data_ptr(), k.data_ptr(), v.data_ptr(), cs.data_ptr(), sn.data_ptr(), rows,
                                               self.kc.data_ptr(), self.vc.data_ptr(), pos_t.data_ptr(),
                                               self.perm.data_ptr() if mapped else None, out.data_ptr(), self.ws.data_ptr(), split,
                                               self.heads, self.kv, self.max_seq, st))
        return out[self.perm.long()] if mapped else out         # element i is stored at out[perm[i]]

    def sync(self):
        torch.cuda.synchronize()
        self._keep.clear()

    def reference(self, pos):
        """fp64 attention of the token at `pos` over rows [0, pos) of the cache and its own k / v."""
        heads, kv, grp = self.heads, self.kv, self.heads // self.kv
        q, k, v = (t.cpu() for t in self.qkv[pos])
        c, s = self.cos[pos].cpu(), self.sin[pos].cpu()

        def rot(x):             # fp32, as the kernel: neox pairs (i, i + 64)
            a, b = x[:, :64], x[:, 64:]
            return torch.cat([a * c - b * s, b * c + a * s], -1)

        qr = (rot(q.float().view(heads, HD)) * HD ** -0.5).half().double()
        kn = rot(k.float().view(kv, HD)).half().double()
        K = torch.cat([self.k0[:, :pos].cpu().double(), kn[:, None]], 1)
        V = torch.cat([self.v0[:, :pos].cpu().double(), v.view(kv, 1, HD).double()], 1)
        hk = torch.arange(heads) // grp
        sc = torch.einsum("hd,hld->hl", qr, K[hk])
        return torch.einsum("hl,hld->hd", sc.softmax(-1), V[hk])


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def golden_entries(heads, kv, max_seq):
    """What tests/golden/make_golden_attn_early.py stores: the output bits of every (position, split), rows form, no output map."""
    C = Case(heads, kv, max_seq)
    out = {}
    for pos in positions(max_seq):
        for split in SPLITS:
            out[key(heads, kv, max_seq, pos, split)] = C.launch(pos, split, "rows", False)
    C.sync()
    return {k_: bits(o) for k_, o in out.items()}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("max_seq", MAX_SEQS)
@pytest.mark.parametrize("heads,kv", LAYOUTS)
def test_early_prefetch_fp64_and_parent_bits(heads, kv, max_seq, golden):
    C = Case(heads, kv, max_seq)
    worst = 0.0
    for pos in positions(max_seq):
        outs = {(split, form, mapped): C.launch(pos, split, form, mapped)
                for split in SPLITS for form in FORMS for mapped in (False, True)}
        C.sync()
        ref = C.reference(pos)
        tol = 2e-3 + 2e-3 * ref.abs().amax(-1, keepdim=True)
        for what, o in outs.items():
            got = o.cpu().double().view(heads, HD)
            assert torch.isfinite(got).all(), (heads, kv, max_seq, pos, what)
            err = ((got - ref).abs() / tol).max().item()
            worst = max(worst, err)
            assert err <= 1.0, (heads, kv, max_seq, pos, what, err)
            want = golden[key(heads, kv, max_seq, pos, what[0])]
            assert np.array_equal(bits(o), want), ("output differs from the parent's", heads, kv, max_seq, pos, what)
    print(f"[attn-early] heads={heads} kv={kv} max_seq={max_seq} splits=1,2,4 positions={positions(max_seq)} "
          f"forms={len(FORMS)} x map: worst err/bound={worst:.3f}")
