"""The one-token attention for long caches (csrc/decode_attn_long.hip, qeft_rope_attn_decode_long; variant "attn_decode_long";
DESIGN.md section 4.4d) through the C ABI, and the decode engine on a model whose max_seq passes 32768.

The harness is tests/test_gpu_attn_long.py's: cache rows at and past pos are fp16 NaN before a launch, the reference is fp64
over the cache as the launch left it with the kernel's own roundings, acceptance per head |got - ref| <= 2e-3 + 2e-3 max|ref|.
_one_token_position checks, per position: every split x both rotary forms against fp64, the forms bit-equal, out_pos, the
appended K row within one fp16 unit, the V row bit-exact, every other cache element untouched bit for bit."""
import pytest
import torch

from test_gpu_attn_long import DEV, HD, _attn_close, _one_token_position, _Slots, _st

pytestmark = pytest.mark.gpu
SPLITS = (1, 2, 64)
# tile edges of a wave (32) and a block step (128); 100: 63 of 64 ranges empty; 20351 .. 20353: around the start of range 53 of
# 64 (ranges of 384 keys there); 32767 / 32768: the old ceiling; the last row is added per cache
POSITIONS = [0, 15, 16, 63, 64, 65, 100, 20351, 20352, 20353, 32767, 32768]


class _Long(_Slots):
    """_Slots whose one-token launch is the long entry, on a workspace sized for 64 splits."""

    def __init__(self, heads, kv, max_seq, seed):
        super().__init__(heads, kv, max_seq, seed)
        self.wsl = torch.zeros(self.lib.qeft_attn_long_workspace_bytes(heads, 64) // 4, device=DEV)

    def one(self, qkv, pos, split, out, form="pos", out_pos=None, slot=0):
        qp, pos_t = qkv.data_ptr(), torch.tensor([pos], dtype=torch.int32, device=DEV)
        cs, sn, rows = (self.cos, self.sin, self.max_seq) if form == "pos" else (self.cos[pos].clone(), self.sin[pos].clone(), 1)
        self._keep += [pos_t, cs, sn]
        self.ck(self.lib.qeft_rope_attn_decode_long(
            qp, qp + self.heads * HD * 2, qp + (self.heads + self.kv) * HD * 2, cs.data_ptr(), sn.data_ptr(), rows,
            self.kc[slot].data_ptr(), self.vc[slot].data_ptr(), pos_t.data_ptr(), out_pos.data_ptr() if out_pos is not None else None,
            out.data_ptr(), self.wsl.data_ptr(), split, self.heads, self.kv, self.max_seq, _st()))


@pytest.mark.parametrize("max_seq", [32784, 65536])
@pytest.mark.parametrize("heads,kv", [(2, 2), (8, 2), (8, 1)])
def test_long_fp64_at_boundary_positions(heads, kv, max_seq):
    A = _Long(heads, kv, max_seq, seed=heads * 7 + kv + max_seq)
    worst = {pos: _one_token_position(A, pos, SPLITS) for pos in POSITIONS + [max_seq - 1]}
    assert A.lib.qeft_last_variant().decode() == "attn_decode_long"
    at = max(worst, key=worst.get)
    print(f"[attn-long] heads={heads} kv={kv} max_seq={max_seq} splits=1,2,64 positions={len(worst)} "
          f"worst err/bound={worst[at]:.3f} (pos {at})")


def test_long_column_tiles_and_determinism():
    """17 query heads per kv head: two column tiles of 16.  Back-to-back launches are bit-equal, with launches of other splits on
    the same workspace between them."""
    A = _Long(34, 2, 32784, seed=5)
    pos, qkv = 32770, A.qkv(1)
    A.poison([pos])
    outs = {}
    for i, split in enumerate((64, 64, 2, 1, 4, 64)):
        outs[i] = A.out()
        A.one(qkv, pos, split, outs[i], "rows")
    A.sync()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[5])
    ref = A.reference(qkv, 1, pos)
    worst = max(_attn_close(o, ref, ("tiles", i)) for i, o in outs.items())
    print(f"[attn-long] heads=34 kv=2 max_seq=32784 pos={pos} splits=64,2,1,4 worst err/bound={worst:.3f}")


@pytest.mark.parametrize("case", ["ramp", "own_split"])
@pytest.mark.parametrize("heads,kv", [(8, 2), (2, 2)])
def test_long_adversarial_scores(case, heads, kv):
    """"ramp": the scores climb ~28 nats with the position, so the running maximum moves in every tile and every earlier
    accumulator is rescaled again and again; "own_split": at the first row of range 53 of 64 the appended key, alone in its
    split and scored from the call's operands, carries all the weight.  The values ramp too; rotary pair (0, 64) is unrotated."""
    A = _Long(heads, kv, 32784, seed=3 * heads + kv)
    pos = 32783 if case == "ramp" else 20352
    idx = torch.arange(A.max_seq, device=DEV, dtype=torch.float32)
    A.v0 = (A.v0.float() + (idx / 8192)[None, None, :, None]).half()
    if case == "ramp":
        A.k0[..., 0] = (idx * (40.0 / A.max_seq)).half()
    ang = torch.randn(A.max_seq, 64, generator=A.g, device=DEV)
    ang[:, 0] = 0.0
    A.tables(ang)
    qkv = A.qkv(1)
    qkv[:, :heads * HD].view(heads, HD)[:, 0] = 8.0
    qkv[:, heads * HD:(heads + kv) * HD].view(kv, HD)[:, 0] = 50.0 if case == "own_split" else 40.0
    worst = _one_token_position(A, pos, SPLITS, qkv)
    print(f"[attn-long-adv] {case} heads={heads} kv={kv} pos={pos} splits=1,2,64 worst err/bound={worst:.3f}")


# ---- the engine on a model of 32832 positions
@pytest.fixture(scope="module")
def long_model():
    from qeft_amd import llama
    return llama.QuantLlama(llama.tiny_shape(n_layers=2, hidden=256, inter=512, n_heads=2, vocab=384, max_seq=32832), DEV, seed=4)


def test_engine_decodes_across_32768(long_model):
    """step() from 32760 over the old ceiling against extend() (qeft_attn_prefill, which has no ceiling and its own fp64 tests),
    with tests/test_gpu_prefill_attn.py's bounds; then run(8) on graphs emits what greedy step() emits."""
    from qeft_amd import llama
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, 384, (32760,), generator=g).to(DEV)
    nxt = torch.randint(0, 384, (16,), generator=g).to(DEV)
    engs = [llama.DecodeEngine(long_model, use_graph=(i == 2)) for i in range(3)]
    llama.prefill(long_model, prompt, engine=engs[0], chunk=4096)
    for e in engs[1:]:      # the same prompt: the caches of the first, copied
        for li in range(2):
            e.kc[li].copy_(engs[0].kc[li])
            e.vc[li].copy_(engs[0].vc[li])
        e.set_position(32760)
    assert all(e.host_pos == 32760 and e.long_ctx for e in engs)
    a, b, c = engs
    got = torch.empty(16, 384, device=DEV)
    for i, t in enumerate(nxt):
        a.tok.fill_(int(t))
        a.step()
        got[i] = a.logits[0].float()
    ref = b.extend(nxt).float()
    assert a.host_pos == b.host_pos == 32776
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    agree = (got.argmax(-1) == ref.argmax(-1)).float().mean().item()
    print(f"[attn-long-engine] step vs extend over 32760..32775: max|dlogit|/max|ref|={rel:.2e} argmax agreement={agree:.2f}")
    assert rel < 2e-2 and agree >= 0.8
    a.set_position(32760)
    a.greedy = c.greedy = True
    a.tok.fill_(int(nxt[0]))
    c.tok.fill_(int(nxt[0]))
    for _ in range(8):
        a.step()
    c.run(8)            # one replay of an 8-token graph: each token feeds the next on the device, so the last one pins the chain
    assert c.host_pos == 32768 and int(c.tok) == int(a.tok) == int(c.logits.argmax())
    c.step()            # ... and the one-token graph at 32768
    a.step()
    assert int(c.tok) == int(a.tok)


def test_paths_that_keep_the_ceiling_refuse_a_long_model(long_model):
    from qeft_amd import batch, llama
    with pytest.raises(ValueError, match="max_seq"):
        llama.DecodeEngine(long_model, kv_dtype="fp8")
    eng = llama.DecodeEngine(long_model, use_graph=False)
    with pytest.raises(ValueError, match="max_seq"):
        batch.BatchDecodeEngine(eng)
    with pytest.raises(ValueError, match="max_seq"):
        eng.verify([1, 2, 3])
