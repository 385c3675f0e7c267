"""CPU checks of the packed (variable-length) training attention's boundary (the varlen launches of csrc/attn_train.hip, DESIGN.md
section 4.18): the entries are declared and exported; they refuse bad arguments in the documented order before any HIP call --
the scalars, then the host prefix itself (NULL), then its contents, then the workspace size, then NULL and alignment of the
device operands; the workspace size is 0 for what they refuse; the host-side enumerations of every address the forward and the
three backward launches form find none outside its operand over the sweep of length lists, head layouts and strides; and the
Python side -- shift_labels(seq_lens=), pack_sequences, causal_lm_loss(seq_lens=) -- keeps its promises without a launch.

As in tests/test_train_rope_cpu.py, no test here hands a launching entry a complete set of valid arguments: where a GPU is
present such a call would launch on made-up addresses."""
import ctypes
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["qeft_attn_train_varlen_fwd", "qeft_attn_train_varlen_bwd", "qeft_attn_train_varlen_bwd_workspace_bytes",
       "qeft_attn_train_varlen_check_extents", "qeft_attn_train_varlen_bwd_check_extents", "qeft_attn_train_varlen_bwd_part"]
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6
P = 1 << 20                       # a 16-byte aligned non-null "pointer": no entry below gets as far as using it
AT_MAX_SEQ = 128


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _prefix(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return (ctypes.c_int * len(cu))(*cu)


def _raw(values):
    return (ctypes.c_int * len(values))(*values)


def test_symbols_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/qeft_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    import qeft_amd
    from qeft_amd import attention
    assert "causal_attention_packed" in qeft_amd.__all__ and callable(qeft_amd.causal_attention_packed)
    assert "pack_sequences" in qeft_amd.__all__ and callable(qeft_amd.pack_sequences)
    header = open(os.path.join(ROOT, "qeft_amd", "csrc", "attn_train.h")).read()
    assert re.search(r"constexpr int AT_MAX_SEQ = (\d+);", header).group(1) == str(AT_MAX_SEQ) == str(attention.MAX_SEQ)


BAD_PREFIXES = [[0, 5, 5, 9], [0, 5, 4, 9], [1, 5, 9], [-1, 5, 9], [0, 0, 9], [0, 5, -2], [0, 5, (1 << 20) + 1]]
GOOD = [0, 5, 16]


def _fwd(lib, q=P, k=P, v=P, out=P, lse=P, q_stride=4096, kv_stride=4096, out_stride=4096, cu=GOOD, n_seq=None, heads=32, kv=32):
    n_seq = len(cu) - 1 if n_seq is None else n_seq
    return lib.qeft_attn_train_varlen_fwd(q, q_stride, k, v, kv_stride, out, out_stride, lse, None if cu is None else _raw(cu), n_seq,
                                          heads, kv, None)


def _bwd(lib, ptr=None, strides=None, ws_bytes=None, cu=GOOD, n_seq=None, heads=32, kv=32, part=None):
    """ptr: overrides of the ten pointers by name; strides: overrides of the six strides by name."""
    p = dict(q=P, k=P, v=P, out=P, dout=P, lse=P, dq=P, dk=P, dv=P, ws=P)
    p.update(ptr or {})
    s = dict(q=heads * 128, kv=kv * 128, out=heads * 128, dout=heads * 128, dq=heads * 128, dkv=kv * 128)
    s.update(strides or {})
    n_seq = len(cu) - 1 if n_seq is None else n_seq
    if ws_bytes is None:
        ws_bytes = 4 * (1 << 20) * max(heads, 1)
    args = [p["q"], s["q"], p["k"], p["v"], s["kv"], p["out"], s["out"], p["dout"], s["dout"], p["lse"], p["dq"], s["dq"], p["dk"],
            p["dv"], s["dkv"], p["ws"], ws_bytes, None if cu is None else _raw(cu), n_seq, heads, kv]
    if part is None:
        return lib.qeft_attn_train_varlen_bwd(*args, None)
    return lib.qeft_attn_train_varlen_bwd_part(*args, part, None)


def test_forward_refuses_in_order_without_a_gpu(lib):
    """QEFT_ERR_SHAPE first, with every device pointer null and misaligned: none is looked at; then NULL; then ALIGN."""
    many = list(range(AT_MAX_SEQ + 2))
    shapes = [dict(n_seq=0), dict(n_seq=-1), dict(cu=many, n_seq=AT_MAX_SEQ + 1), dict(heads=32, kv=5), dict(heads=32, kv=0),
              dict(heads=0, kv=0), dict(q_stride=4100), dict(q_stride=4088), dict(out_stride=4100), dict(out_stride=2048),
              dict(kv_stride=4100), dict(kv_stride=1024)] + [dict(cu=cu) for cu in BAD_PREFIXES]
    for bad in shapes:
        assert _fwd(lib, **bad) == ERR_SHAPE, bad
        assert _fwd(lib, q=None, k=3, v=None, out=5, lse=1, **bad) == ERR_SHAPE, bad
    # the scalars before the prefix is read at all; the prefix itself before its contents and before the device pointers
    assert _fwd(lib, cu=None, n_seq=0) == ERR_SHAPE and _fwd(lib, cu=None, n_seq=2, q_stride=4100) == ERR_SHAPE
    assert _fwd(lib, cu=None, n_seq=2) == ERR_NULL and _fwd(lib, cu=None, n_seq=2, q=3, out=5) == ERR_NULL
    assert _fwd(lib, cu=many[:AT_MAX_SEQ + 1], q=None) == ERR_NULL            # AT_MAX_SEQ sequences are taken
    assert _fwd(lib, cu=[0, 1 << 20], q=None) == ERR_NULL                    # 2^20 rows are taken
    for name in ("q", "k", "v", "out", "lse"):
        assert _fwd(lib, **{name: None}) == ERR_NULL, name
        assert _fwd(lib, **{name: None, "q" if name != "q" else "k": P + 2}) == ERR_NULL, name      # NULL before ALIGN
    for name in ("q", "k", "v", "out"):
        assert _fwd(lib, **{name: P + 8}) == ERR_ALIGN, name
    assert _fwd(lib, lse=P + 2) == ERR_ALIGN and _fwd(lib, lse=P + 1) == ERR_ALIGN


def test_backward_refuses_in_order_without_a_gpu(lib):
    nul = dict(q=None, k=None, v=None, out=None, dout=None, lse=None, dq=None, dk=None, dv=None, ws=None)
    odd = {k_: 3 for k_ in nul}
    many = list(range(AT_MAX_SEQ + 2))
    shapes = [dict(n_seq=0), dict(cu=many, n_seq=AT_MAX_SEQ + 1), dict(heads=32, kv=5), dict(heads=32, kv=0)] + \
        [dict(cu=cu) for cu in BAD_PREFIXES]
    for bad in shapes:
        for ptr in (None, nul, odd):
            assert _bwd(lib, ptr=ptr, **bad) == ERR_SHAPE, (bad, ptr)
            assert _bwd(lib, ptr=ptr, part=1, **bad) == ERR_SHAPE, (bad, ptr)
    for name, width in (("q", 4096), ("kv", 4096), ("out", 4096), ("dout", 4096), ("dq", 4096), ("dkv", 4096)):
        for stride in (width + 4, width - 8):
            for ptr in (None, nul, odd):
                assert _bwd(lib, ptr=ptr, strides={name: stride}) == ERR_SHAPE, (name, stride)
    for ptr in (None, nul, odd):
        assert _bwd(lib, ptr=ptr, cu=None, n_seq=2) == ERR_NULL                  # the host prefix
        assert _bwd(lib, ptr=ptr, cu=None, n_seq=0) == ERR_SHAPE
    need = lib.qeft_attn_train_varlen_bwd_workspace_bytes(_raw(GOOD), 2, 32, 32)
    assert need == 4 * 16 * 32
    for ptr in (None, nul, odd):
        assert _bwd(lib, ptr=ptr, ws_bytes=need - 1) == ERR_SHAPE               # a short workspace is a shape error
    assert _bwd(lib, ptr=nul, ws_bytes=need) == ERR_NULL
    for name in nul:
        assert _bwd(lib, ptr={name: None}) == ERR_NULL, name
        other = "q" if name != "q" else "k"
        assert _bwd(lib, ptr={name: None, other: P + 2}) == ERR_NULL, name      # NULL before ALIGN
    for name in nul:
        assert _bwd(lib, ptr={name: P + (2 if name == "lse" else 8)}) == ERR_ALIGN, name
    for part in (-1, 3):
        for ptr in (None, nul):
            assert _bwd(lib, ptr=ptr, part=part) == ERR_SHAPE
    assert _bwd(lib, ptr={"dk": None}, part=1) == ERR_NULL and _bwd(lib, ptr={"dq": P + 8}, part=2) == ERR_ALIGN


def test_workspace_bytes(lib):
    f = lib.qeft_attn_train_varlen_bwd_workspace_bytes
    assert f(_prefix([200, 7, 257, 64, 3]), 5, 64, 8) == 4 * 531 * 64
    assert f(_prefix([1] * AT_MAX_SEQ), AT_MAX_SEQ, 4, 2) == 4 * AT_MAX_SEQ * 4
    assert f(_raw([0, 1 << 20]), 1, 32, 32) == 4 * 2 ** 20 * 32
    for cu, n_seq, heads, kv in ((GOOD, 0, 32, 32), (GOOD, -1, 32, 32), (list(range(AT_MAX_SEQ + 2)), AT_MAX_SEQ + 1, 32, 32),
                                 (GOOD, 2, 32, 5), (GOOD, 2, 32, 0), (GOOD, 2, 0, 0), (GOOD, 2, -32, -32), (None, 2, 32, 32)) + \
            tuple((cu, len(cu) - 1, 32, 32) for cu in BAD_PREFIXES):
        assert f(None if cu is None else _raw(cu), n_seq, heads, kv) == 0, (cu, n_seq, heads, kv)


LENGTH_LISTS = ([1], [1, 1, 1], [64, 65], [127, 1, 128, 129], [200, 7, 257, 64, 3], [1] * AT_MAX_SEQ, [2048])
LAYOUTS = ((4, 2), (2, 2), (8, 1), (64, 8))


def test_no_address_outside_its_operand(lib):
    """Both enumerations over the sweep, with every stride at its minimum and padded (q, k, v as views of one fused buffer; the
    gradients in padded rows of their own)."""
    fwd, bwd = lib.qeft_attn_train_varlen_check_extents, lib.qeft_attn_train_varlen_bwd_check_extents
    n = 0
    for lens in LENGTH_LISTS:
        cu = _prefix(lens)
        for heads, kv in LAYOUTS:
            hw, kw, fused = heads * 128, kv * 128, (heads + 2 * kv) * 128
            for pad in (False, True):
                qs, ks, os_ = (fused, fused, hw + 64) if pad else (hw, kw, hw)
                assert fwd(qs, ks, os_, cu, len(lens), heads, kv) == 0, (lens, heads, kv, pad)
                ds, dqs, dkvs = (hw + 8, fused, fused) if pad else (hw, hw, kw)
                assert bwd(qs, ks, os_, ds, dqs, dkvs, cu, len(lens), heads, kv) == 0, (lens, heads, kv, pad)
                n += 1
    assert n == len(LENGTH_LISTS) * len(LAYOUTS) * 2


def test_the_enumerations_walk_the_fixed_length_addresses(lib):
    """Equal lengths are the fixed-length launch: both pairs of enumerations agree there (0), so the walkers they share see the
    same operands either way; and the varlen pair refuses what the entries refuse."""
    fwd, bwd = lib.qeft_attn_train_varlen_check_extents, lib.qeft_attn_train_varlen_bwd_check_extents
    for t, n_seq in ((129, 3), (64, 2), (1, 5)):
        cu = _prefix([t] * n_seq)
        assert fwd(1024, 256, 1024, cu, n_seq, 8, 2) == lib.qeft_attn_train_check_extents(1024, 256, 1024, n_seq, t, 8, 2) == 0
        assert bwd(1024, 256, 1024, 1024, 1024, 256, cu, n_seq, 8, 2) == \
            lib.qeft_attn_train_bwd_check_extents(1024, 256, 1024, 1024, 1024, 256, n_seq, t, 8, 2) == 0
    good = _raw(GOOD)
    assert fwd(4096, 4096, 4096, good, 0, 32, 32) == -1 and fwd(4096, 4096, 4096, None, 2, 32, 32) == -1
    assert fwd(4096, 4088, 4096, good, 2, 32, 32) == -1 and fwd(4096, 4096, 4096, good, 2, 32, 5) == -1
    for cu in BAD_PREFIXES:
        assert fwd(4096, 4096, 4096, _raw(cu), len(cu) - 1, 32, 32) == -1, cu
        assert bwd(4096, 4096, 4096, 4096, 4096, 4096, _raw(cu), len(cu) - 1, 32, 32) == -1, cu
    assert bwd(4096, 4096, 4096, 4100, 4096, 4096, good, 2, 32, 32) == -1
    assert bwd(4096, 4096, 4096, 4096, 4096, 1024, good, 2, 32, 32) == -1


def test_shift_labels_ignores_the_last_row_of_every_packed_sequence():
    import torch
    from qeft_amd.finetune import IGNORE_INDEX as I, shift_labels
    tokens = torch.tensor([10, 11, 12, 20, 30, 31, 40, 41, 42, 43])
    assert shift_labels(tokens, seq_lens=[3, 1, 2, 4]).tolist() == [11, 12, I, I, 31, I, 41, 42, 43, I]
    labels = torch.tensor([10, I, 12, 20, 30, 31, 40, 41, I, 43])
    got = shift_labels(tokens, labels, seq_lens=(3, 1, 2, 4))
    assert got.dtype == torch.int32 and got.tolist() == [I, 12, I, I, 31, I, 41, I, 43, I]
    assert shift_labels(tokens, seq_lens=[10]).tolist() == shift_labels(tokens).tolist()             # one sequence: the old rule
    assert shift_labels(tokens).tolist() == [11, 12, 20, 30, 31, 40, 41, 42, 43, I]                  # and that one is unchanged
    assert shift_labels(tokens.view(2, 5)).tolist() == [[11, 12, 20, 30, I], [40, 41, 42, 43, I]]
    for bad in ([3, 1, 2, 3], [3, 1, 2, 5], [3, 0, 3, 4], [11, -1], []):
        with pytest.raises(ValueError):
            shift_labels(tokens, seq_lens=bad)
    with pytest.raises(ValueError, match="1-D"):
        shift_labels(tokens.view(2, 5), seq_lens=[5, 5])


def test_pack_sequences_invariants():
    import torch
    from qeft_amd.finetune import pack_sequences
    g = torch.Generator().manual_seed(3)
    lens = [int(n) for n in torch.randint(1, 700, (60,), generator=g)] + [2048, 1, 1, 1024, 1024]
    seqs = [torch.full((n,), i, dtype=torch.long) for i, n in enumerate(lens)]           # sequence i holds the value i
    labels = [-s - 1 for s in seqs]
    packs = pack_sequences(seqs, labels, budget=2048)
    seen = []
    for tokens, labs, seq_lens in packs:
        assert tokens.dim() == 1 and tokens.shape[0] == sum(seq_lens) <= 2048 and 1 <= len(seq_lens) <= AT_MAX_SEQ
        assert torch.equal(labs, -tokens - 1)
        a = 0
        for n in seq_lens:
            i = int(tokens[a])
            assert lens[i] == n and bool((tokens[a:a + n] == i).all())                 # whole, in one piece
            seen.append(i)
            a += n
    assert sorted(seen) == list(range(len(seqs)))                                        # every sequence exactly once
    assert len(packs) <= 2 * (sum(lens) + 2047) // 2048                                  # first-fit leaves at most one pack half empty
    again = pack_sequences(seqs, labels, budget=2048)
    assert [(t.tolist(), l.tolist(), n) for t, l, n in again] == [(t.tolist(), l.tolist(), n) for t, l, n in packs]
    assert all(l is None for _, l, _ in pack_sequences(seqs))
    # more than AT_MAX_SEQ one-token sequences under one budget: the count splits the packs, not the rows
    ones = pack_sequences([torch.tensor([i]) for i in range(3 * AT_MAX_SEQ + 5)], budget=2048)
    assert [len(n) for _, _, n in ones] == [AT_MAX_SEQ] * 3 + [5]
    assert torch.cat([t for t, _, _ in ones]).tolist() == list(range(3 * AT_MAX_SEQ + 5))
    with pytest.raises(ValueError, match="budget"):
        pack_sequences([torch.zeros(5, dtype=torch.long), torch.zeros(2049, dtype=torch.long)], budget=2048)
    with pytest.raises(ValueError):
        pack_sequences([torch.zeros(0, dtype=torch.long)])
    with pytest.raises(ValueError):
        pack_sequences([torch.zeros(2, 3, dtype=torch.long)])
    with pytest.raises(ValueError):
        pack_sequences(seqs, labels[:-1])
    assert pack_sequences([]) == []


def test_causal_lm_loss_refuses_bad_seq_lens_before_any_launch():
    """Raised before the model's weights or the library are looked at: a bare shape is all the 'model' has."""
    import torch
    from qeft_amd import finetune
    from qeft_amd.llama import LlamaShape
    model = types.SimpleNamespace(shape=LlamaShape(512, 512, 2, 4, 2, 512, max_seq=256))
    tokens = torch.zeros(300, dtype=torch.long)
    for attn in ("own", "sdpa"):
        with pytest.raises(ValueError, match="1-D"):
            finetune.causal_lm_loss(model, tokens.view(3, 100), seq_lens=[100, 100, 100], attn=attn)
        with pytest.raises(ValueError, match="sum"):
            finetune.causal_lm_loss(model, tokens, seq_lens=[100, 100, 99], attn=attn)
        with pytest.raises(ValueError, match="at least one row"):
            finetune.causal_lm_loss(model, tokens, seq_lens=[100, 0, 200], attn=attn)
        with pytest.raises(ValueError, match="at least one row"):
            finetune.causal_lm_loss(model, tokens, seq_lens=[301, -1], attn=attn)
        with pytest.raises(ValueError, match="max_seq"):
            finetune.causal_lm_loss(model, tokens, seq_lens=[257, 43], attn=attn)
        with pytest.raises(ValueError, match="sequences"):
            finetune.causal_lm_loss(model, tokens, seq_lens=[1] * (AT_MAX_SEQ + 1) + [300 - AT_MAX_SEQ - 1], attn=attn)
        with pytest.raises(ValueError, match="sequences"):
            finetune.causal_lm_loss(model, tokens, seq_lens=[], attn=attn)
        with pytest.raises(ValueError, match="ints"):
            finetune.causal_lm_loss(model, tokens, seq_lens=[150.0, 150.0], attn=attn)


def test_causal_attention_packed_refuses_on_the_cpu():
    import torch
    from qeft_amd.attention import causal_attention_packed
    z = lambda *s: torch.zeros(*s, dtype=torch.float16)
    with pytest.raises(ValueError, match="multiple"):
        causal_attention_packed(z(8, 6, 128), z(8, 4, 128), z(8, 4, 128), [8])
    with pytest.raises(ValueError, match="head size"):
        causal_attention_packed(z(8, 6, 64), z(8, 2, 64), z(8, 2, 64), [8])
    with pytest.raises(ValueError, match=r"\[R, H, 128\]"):
        causal_attention_packed(z(1, 8, 6, 128), z(1, 8, 2, 128), z(1, 8, 2, 128), [8])
    with pytest.raises(ValueError, match="sum"):
        causal_attention_packed(z(8, 6, 128), z(8, 2, 128), z(8, 2, 128), [3, 4])
    with pytest.raises(ValueError, match="sequences"):
        causal_attention_packed(z(200, 6, 128), z(200, 2, 128), z(200, 2, 128), [1] * 129 + [71])
    with pytest.raises(ValueError, match="fp16"):
        causal_attention_packed(z(8, 6, 128).float(), z(8, 2, 128), z(8, 2, 128), [8])
    with pytest.raises(RuntimeError, match="GPU"):
        causal_attention_packed(z(8, 6, 128), z(8, 2, 128), z(8, 2, 128), [3, 5])
