"""CPU checks of the fused lm_head + cross-entropy entry (csrc/lm_head_nll.hip) and of scoring.eval_nll's arithmetic: the three
entries are declared, exported and bound; the entry refuses bad arguments before any HIP call, SHAPE before NULL before ALIGN; the
workspace size is positive and monotone; the host-side enumeration of every address the two launches form finds none outside its
operand over the sweep of rows, widths, vocabularies and strides; eval_nll reproduces the reference's perplexity formula
(qeft/main.py:291-305) on logits the test owns."""
import itertools
import math
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["qeft_lm_head_nll_workspace_bytes", "qeft_lm_head_nll", "qeft_lm_head_nll_check_extents"]
ERR_SHAPE, ERR_NULL, ERR_ALIGN = 2, 4, 6


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_symbols_declared_exported_and_bound(lib):
    from qeft_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/qeft_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    assert lib.qeft_abi_version() == 1
    import qeft_amd
    from qeft_amd import scoring
    assert qeft_amd.score is scoring.score and qeft_amd.eval_nll is scoring.eval_nll and qeft_amd.lm_head_nll is scoring.lm_head_nll


def test_entry_refuses_bad_arguments_without_a_gpu(lib):
    """Validation happens before any HIP call: SHAPE before any pointer is looked at, then NULL, then ALIGN."""
    P = 1 << 20
    e = lib.qeft_lm_head_nll
    big = 1 << 40

    def call(x=P, x_stride=256, w=P, targets=P, lse=P, tgt=P, argmax=P, ws=P, ws_bytes=big, t=16, hidden=256, vocab=512):
        return e(x, x_stride, w, targets, lse, tgt, argmax, ws, ws_bytes, t, hidden, vocab, None)
    assert call(t=0) == ERR_SHAPE and call(t=-3) == ERR_SHAPE
    assert call(hidden=96, x_stride=96) == ERR_SHAPE and call(hidden=0, x_stride=0) == ERR_SHAPE and call(hidden=32, x_stride=32) == ERR_SHAPE
    assert call(vocab=0) == ERR_SHAPE
    assert call(x_stride=248) == ERR_SHAPE and call(x_stride=260) == ERR_SHAPE      # narrower than hidden / not a multiple of 8
    need = lib.qeft_lm_head_nll_workspace_bytes(16, 512)
    assert call(x=None, ws_bytes=need) == ERR_NULL                                   # exactly enough passes the shape check
    assert call(ws_bytes=need - 1) == ERR_SHAPE and call(ws_bytes=0) == ERR_SHAPE
    # SHAPE wins over NULL and ALIGN
    assert call(x=None, t=0) == ERR_SHAPE and call(x=P + 2, hidden=96, x_stride=96) == ERR_SHAPE
    assert call(ws=None, ws_bytes=0) == ERR_SHAPE
    # NULL wins over ALIGN
    for kw in ("x", "w", "lse", "ws"):
        assert call(**{kw: None}) == ERR_NULL, kw
    assert call(tgt=None) == ERR_NULL                                                # targets given, nowhere to put their logits
    assert call(x=None, w=P + 2) == ERR_NULL
    for kw in ("x", "w", "ws"):
        assert call(**{kw: P + 8}) == ERR_ALIGN, kw
    for kw in ("targets", "lse", "tgt", "argmax"):
        assert call(**{kw: P + 2}) == ERR_ALIGN, kw


def test_workspace_bytes(lib):
    f = lib.qeft_lm_head_nll_workspace_bytes
    ts, vs = (1, 7, 64, 65, 200, 2048), (1, 9, 127, 128, 129, 4097, 32000)
    for t in ts:
        for v in vs:
            assert f(t, v) >= 12 * t * ((v + 127) // 128) > 0
    for v in vs:
        col = [f(t, v) for t in ts]
        assert col == sorted(col)
    for t in ts:
        row = [f(t, v) for v in vs]
        assert row == sorted(row)
    assert f(2048, 32000) == 12 * 2048 * 250
    assert f(0, 512) == 0 and f(-1, 512) == 0 and f(16, 0) == 0 and f(16, -5) == 0


def test_no_address_outside_its_operand(lib):
    f = lib.qeft_lm_head_nll_check_extents
    n = 0
    for t, hidden, vocab in itertools.product((1, 7, 63, 64, 65, 127, 128, 129, 200, 2048), (64, 256, 4096, 5120, 8192),
                                              (1, 9, 127, 128, 129, 4097, 32000)):
        for x_stride in (hidden, hidden + 8, 3 * hidden):
            assert f(x_stride, t, hidden, vocab) == 0, (t, hidden, vocab, x_stride)
            n += 1
    assert n == 10 * 5 * 7 * 3
    assert f(256, 0, 256, 512) == -1 and f(96, 4, 96, 512) == -1 and f(248, 4, 256, 512) == -1 and f(260, 4, 256, 512) == -1
    assert f(256, 4, 256, 0) == -1


def _reference_ppl(logits, tokens, seqlen):
    """qeft/main.py:291-305 in fp64: CrossEntropyLoss of the shifted window x seqlen, summed, over n * seqlen."""
    n = tokens.numel() // seqlen
    nlls = []
    for i in range(n):
        win = tokens[i * seqlen:(i + 1) * seqlen]
        loss = torch.nn.CrossEntropyLoss()(logits[i][:-1].double(), win[1:])
        nlls.append(loss * seqlen)
    return (torch.stack(nlls).sum() / (n * seqlen)).item()


def test_eval_nll_is_the_reference_formula(monkeypatch):
    from qeft_amd import scoring
    vocab, seqlen, n = 37, 16, 3
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, vocab, (n * seqlen + 5,), generator=g)                 # 5 trailing tokens: a partial window, dropped
    logits = (torch.randn(n, seqlen, vocab, generator=g, dtype=torch.float64) * 3)
    model = types.SimpleNamespace(shape=types.SimpleNamespace(max_seq=64, vocab=vocab))
    calls = []

    def stub(m, toks, engine=None, *, start=0, attn=None, chunk=None, targets=None):
        i = len(calls)
        calls.append((toks.clone(), chunk))
        assert m is model and engine is None and start == 0 and targets is None
        lg = logits[i]
        lse = torch.logsumexp(lg, dim=1)
        lp = torch.zeros(seqlen, dtype=torch.float64)
        lp[:-1] = lg[:-1].gather(1, toks[1:, None])[:, 0] - lse[:-1]
        return scoring.Score(lp, lse, lg.argmax(1).to(torch.int32))
    monkeypatch.setattr(scoring, "score", stub)
    out = scoring.eval_nll(model, tokens, seqlen=seqlen, chunk=8)
    assert len(calls) == n and all(c == 8 for _, c in calls)
    for i, (toks, _) in enumerate(calls):                                             # every window starts at its own position 0
        assert torch.equal(toks, tokens[i * seqlen:(i + 1) * seqlen])
    want = _reference_ppl(logits, tokens, seqlen)
    assert abs(out["nll"] - want) <= 1e-12, (out["nll"], want)
    assert abs(out["ppl"] - math.exp(want)) <= 1e-12 * math.exp(want) * 4
    assert out["windows"] == n and out["tokens"] == n * seqlen
    with pytest.raises(ValueError):
        scoring.eval_nll(model, tokens[:seqlen - 1], seqlen=seqlen)                  # n == 0
    with pytest.raises(ValueError):
        scoring.eval_nll(model, tokens, seqlen=65)                                   # seqlen > max_seq
