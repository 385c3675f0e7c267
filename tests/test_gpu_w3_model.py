"""A 3-bit model through every pass that takes one, whole passes against a float64 dense pass
(tests/dense_ref.py).  test_gpu_w3.py pins the 3-bit kernels one launch at a time and runs the v3 decode engine on a 256-wide toy;
here prefill, score / eval_nll, causal_lm_loss, finetune.begin / end, the checkpoint round trips, the fp8 KV cache and the
refusals run on

    LlamaShape(hidden 512, inter 1536, 2 layers, 4 heads / 2 kv heads, vocab 512, max_seq 1408, bits 3)

whose sizes split the routes of QuantLinear._forward_w3 and of the backward (the predicates are gemm_w4.hip's gemm_w3_native_tile
and gemm_dx_v3_tile; test_the_shape_splits_the_routes asks the library itself):

    rows <= 16                  gemv_3bit on the 3-bit stream (gemv_w3 / gemv_w3_rows)
    17 .. , too few tiles       gemm_3bit_qeft expands to the 4-bit layout per call (every linear at T = 17, 200; N or K = 512 at T = 1280)
    T = 1280, N = 1536          10 x 12 = 120 >= 112 tiles: gate_proj (and up_proj in training) on gemm_v3_128x128_w3, native
    T = 1280, dX with K = 1536  down_proj's dX on dx128v3_w3, native; every other dX expands

(in prefill up_proj runs inside forward_silu_mul, which expands for the SiLU epilogue of the 4-bit GEMM from 8 rows on.)  Bounds:
own error from fp64 <= 2 x the fp16 torch pass's + a floor of the output format, as in tests/test_gpu_engine_round1.py."""
import argparse
import math

import pytest
import torch

from dense_ref import F16, F32, F64, IGNORE, NLL_FLOOR, bounded, check_logits_and_nll, dense_pass, logits_pair, next_token_nll

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_LONG, T_SMALL = 1280, 48
SCALE = 1024.0
HEADS = dict(n_heads=4, n_kv_heads=2)


def _shape():
    from qeft_amd.llama import LlamaShape
    return LlamaShape(hidden=512, inter=1536, n_layers=2, n_heads=4, n_kv_heads=2, vocab=512, max_seq=1408, bits=3, name="w3")


def _new_model():
    from qeft_amd.llama import QuantLlama
    return QuantLlama(_shape(), DEV, seed=12)


def _tokens():
    return torch.randint(0, 512, (T_LONG,), generator=torch.Generator().manual_seed(13)).to(DEV)


_INFER = {}


def _infer():
    """(model, tokens, dense weights) of the inference tests: made once, shared, never written."""
    if not _INFER:
        model = _new_model()
        _INFER["m"] = (model, _tokens(), model.dense_weights())
    return _INFER["m"]


def _refs(T):
    """(ref64, logits16) of the first T tokens, once per T."""
    if T not in _INFER:
        model, tokens, dense = _infer()
        _INFER[T] = logits_pair(model, tokens[:T], dense)
    return _INFER[T]


class Spy:
    """Notes every call of qeft_cuda's 3-bit entries with the variant it dispatched to; a GEMM or dX call is `native` when it did
    not come back through expand_3bit."""

    def __init__(self, monkeypatch):
        from qeft_amd import _lib, qeft_cuda
        self.calls = []
        expands = []

        def wrap(name, fn):
            def call(*a, **kw):
                before = len(expands)
                out = fn(*a, **kw)
                if name == "expand_3bit":
                    expands.append(1)
                rows = a[0].numel() // a[0].shape[-1] if name != "expand_3bit" else 0
                self.calls.append((name, _lib.last_variant(), len(expands) == before, rows))
                return out
            return call
        for name in ("gemv_3bit", "gemm_3bit_qeft", "gemm_3bit_dx", "expand_3bit"):
            monkeypatch.setattr(qeft_cuda, name, wrap(name, getattr(qeft_cuda, name)))

    def of(self, name):
        return [c for c in self.calls if c[0] == name]

    def routes(self):
        out = set()
        for name, variant, native, _ in self.calls:
            if name == "gemv_3bit":
                out.add(variant)
            elif name in ("gemm_3bit_qeft", "gemm_3bit_dx"):
                out.add(variant if native else name + ":expanded")
        return out


def test_the_shape_splits_the_routes():
    """The library's own predicates on the linears of this model: which take the 3-bit stream natively at which row count."""
    from qeft_amd import _lib
    lib, s = _lib.lib(), _shape()
    kv = s.n_kv_heads * 128
    fwd = {"q": (s.hidden, s.hidden), "k": (kv, s.hidden), "gate": (s.inter, s.hidden), "down": (s.hidden, s.inter)}
    for T in (17, 200, T_SMALL):
        assert not any(lib.qeft_gemm_w3_supported(T, n, k, 128, 128) for n, k in fwd.values()), T
        assert not any(lib.qeft_gemm_w3_dx_supported(T, n, k, 128, 128) for n, k in fwd.values()), T
    assert {nm: bool(lib.qeft_gemm_w3_supported(T_LONG, n, k, 128, 128)) for nm, (n, k) in fwd.items()} == \
        {"q": False, "k": False, "gate": True, "down": False}
    assert {nm: bool(lib.qeft_gemm_w3_dx_supported(T_LONG, n, k, 128, 128)) for nm, (n, k) in fwd.items()} == \
        {"q": False, "k": False, "gate": False, "down": True}


def test_prefill_routes_against_fp64(monkeypatch):
    from qeft_amd.llama import prefill
    model, tokens, _ = _infer()
    for T in (5, 16, 17, 200, T_LONG):
        _refs(T)                                    # (dense_weights() expands too: before the spy)
    n_layers, union = model.shape.n_layers, set()
    for T in (5, 16, 17, 200, T_LONG):
        spy = Spy(monkeypatch)
        logits = prefill(model, tokens[:T])
        torch.cuda.synchronize()
        monkeypatch.undo()
        routes = spy.routes()
        union |= routes
        print(f"[w3 model] prefill T={T}: {sorted(routes)}  gemv {len(spy.of('gemv_3bit'))}  gemm {len(spy.of('gemm_3bit_qeft'))}  "
              f"expand {len(spy.of('expand_3bit'))}")
        assert logits.shape == (T, model.shape.vocab) and logits.dtype == F16
        if T <= 16:
            assert not spy.of("gemm_3bit_qeft"), f"T = {T} reached the GEMM"
            assert routes == {"gemv_w3_rows"} and all(c[3] == T for c in spy.of("gemv_3bit"))
            # up_proj leaves the GEMV for forward_silu_mul's GEMM epilogue from 8 rows on
            assert len(spy.of("gemv_3bit")) == (7 if T < 8 else 6) * n_layers
        else:
            assert not spy.of("gemv_3bit") and len(spy.of("gemm_3bit_qeft")) == 6 * n_layers, f"T = {T}"
            native = [c for c in spy.of("gemm_3bit_qeft") if c[2]]
            if T == T_LONG:
                assert [c[1] for c in native] == ["gemm_v3_128x128_w3"] * n_layers         # gate_proj
                assert "gemm_3bit_qeft:expanded" in routes
            else:
                assert not native and routes == {"gemm_3bit_qeft:expanded"}
        check_logits_and_nll(f"w3 prefill T={T}", logits.float(), *_refs(T), tokens[:T])
    assert union >= {"gemv_w3_rows", "gemm_3bit_qeft:expanded", "gemm_v3_128x128_w3"}, union


@pytest.mark.parametrize("chunk", [None, 64])
def test_prefill_on_the_own_attention(chunk):
    from qeft_amd.llama import prefill
    model, tokens, _ = _infer()
    T = 200
    logits = prefill(model, tokens[:T], attn="own", chunk=chunk)
    check_logits_and_nll(f"w3 prefill own attention chunk={chunk} T={T}", logits.float(), *_refs(T), tokens[:T])


def test_score_and_eval_nll_against_fp64():
    from qeft_amd import eval_nll, score
    model, tokens, dense = _infer()
    T = 256
    toks = tokens[:T]
    ref64, l16 = _refs(T)
    n64, n16 = next_token_nll(ref64, toks), next_token_nll(l16.half(), toks)
    sc = score(model, toks)
    assert sc.logprob.shape == (T,) and sc.logprob[-1].item() == 0.0
    bounded("w3 score T=256", abs(-sc.logprob[:-1].double().mean().item() - n64), abs(n16 - n64), NLL_FLOOR, "nll")
    # eval_nll: two windows of 128, each from position 0; the mean of the window means
    tok2 = toks.view(2, 128)
    targets = torch.full((2, 128), IGNORE, dtype=torch.long, device=DEV)
    targets[:, :-1] = tok2[:, 1:]
    with torch.no_grad():
        w64 = dense_pass(model, dense, None, tok2, targets.reshape(-1), F64).item()
        w16 = dense_pass(model, dense, None, tok2, targets.reshape(-1), F16).item()
    ev = eval_nll(model, toks, seqlen=128)
    assert ev["windows"] == 2 and ev["tokens"] == 256 and ev["ppl"] == math.exp(ev["nll"])
    # (the protocol weighs a window's mean over 127 targets by 128 and divides by 256: the mean of the window means)
    bounded("w3 eval_nll 2 x 128", abs(ev["nll"] - w64), abs(w16 - w64), NLL_FLOOR, "nll")


# ---- training: causal_lm_loss and all 14 d(oweight) against fp64 autograd of the dense pass
NAMES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
_TRAIN = {}


def _train():
    """(model, tokens, labels, params, reference(T)) with the model in training mode: made once, shared."""
    if not _TRAIN:
        from qeft_amd import finetune
        from qeft_amd.llama import layer_linears
        model, tokens = _new_model(), _tokens()
        labels = tokens.clone()
        labels[torch.tensor([0, 1, 2, 10, 11, 30, 47, 600, 1279])] = IGNORE
        dense = model.dense_weights()                                   # before begin(): oweight is still the fp16 buffer
        ow = [{nm: ql.oweight.detach().clone() for nm, ql in layer_linears(L)} for L in model.model.layers]
        params = finetune.begin(model)
        assert len(params) == 7 * model.shape.n_layers and all(p.dtype == F32 and p.requires_grad for p in params)
        refs = {}

        def reference(T):
            """(loss64, grads64, loss16, grads16) over the first T tokens, once per T."""
            if T not in refs:
                tok2 = tokens[:T].view(1, -1)
                targets = finetune.shift_labels(tok2, labels[:T].view(1, -1)).reshape(-1)
                out = []
                for dt in (F64, F16):
                    leaves = [{nm: v.to(F64 if dt == F64 else F32).requires_grad_(True) for nm, v in d.items()} for d in ow]
                    loss = dense_pass(model, dense, leaves, tok2, targets, dt)
                    (loss * (SCALE if dt == F16 else 1.0)).backward()
                    grads = [{nm: (v.grad.to(F64) / (SCALE if dt == F16 else 1.0)) for nm, v in d.items()} for d in leaves]
                    out += [loss.item(), grads]
                refs[T] = tuple(out)
            return refs[T]
        _TRAIN["t"] = (model, tokens, labels, params, reference)
    return _TRAIN["t"]


OPTIONS = {"defaults": {}, "own-fused-checkpoint": dict(attn="own", glue="fused", rope="fused", checkpoint=True)}


@pytest.mark.parametrize("T", [T_SMALL, T_LONG])
@pytest.mark.parametrize("kind", list(OPTIONS))
def test_causal_lm_loss_and_d_oweight_against_fp64(kind, T, monkeypatch):
    from qeft_amd import causal_lm_loss
    from qeft_amd.llama import layer_linears
    model, tokens, labels, params, reference = _train()
    loss64, g64, loss16, g16 = reference(T)
    for p in params:
        p.grad = None
    spy = Spy(monkeypatch)
    loss = causal_lm_loss(model, tokens[:T], labels[:T], **OPTIONS[kind])
    assert loss.dtype == F32 and loss.dim() == 0
    (loss * SCALE).backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    fwd, dx = spy.of("gemm_3bit_qeft"), spy.of("gemm_3bit_dx")
    tag = f"w3 train {kind} T={T}"
    print(f"[w3 model] {tag}: forward {sorted({c[1] if c[2] else 'expanded' for c in fwd})}  dX {sorted({c[1] if c[2] else 'expanded' for c in dx})}")
    assert not spy.of("gemv_3bit") and fwd and dx
    if T == T_SMALL:
        assert not any(c[2] for c in fwd) and not any(c[2] for c in dx), "48 rows took a native tier"
    else:
        assert {c[1] for c in fwd if c[2]} == {"gemm_v3_128x128_w3"} and any(not c[2] for c in fwd)
        assert {c[1] for c in dx if c[2]} == {"dx128v3_w3"} and any(not c[2] for c in dx)
    bounded(tag, abs(loss.item() - loss64), abs(loss16 - loss64), NLL_FLOOR, "loss")
    worst, lines = 0.0, []
    for li, L in enumerate(model.model.layers):
        for nm, ql in layer_linears(L):
            assert ql.oweight.grad is not None and ql.oweight.grad.dtype == F32, (li, nm)
            assert torch.isfinite(ql.oweight.grad).all(), (li, nm)
            ref = g64[li][nm]
            own = ((ql.oweight.grad.to(F64) / SCALE - ref).norm() / ref.norm()).item()
            t16 = ((g16[li][nm] - ref).norm() / ref.norm()).item()
            worst = max(worst, own / t16)
            lines.append(f"{li}.{nm} {own:.2e}/{t16:.2e}={own / t16:.2f}")
    print(f"[w3 model] {tag}: rel L2 error of d(oweight), own / fp16 torch: " + "  ".join(lines))
    print(f"[w3 model] {tag}: largest ratio own / fp16 torch = {worst:.3f} (allowed 2)")
    assert len(lines) == 14
    assert worst <= 2.0, f"{tag}: a d(oweight) is {worst:.2f} x the fp16 torch pass's error from fp64"


def _infos(model):
    from qeft_amd.llama import LINEARS
    return {f"model.layers.{li}.{grp}.{nm}": argparse.Namespace(bits=3, sym=False, group_size=128, n_out=128, reorder=True)
            for li in range(model.shape.n_layers) for grp, nm in LINEARS}


BUFFERS = ("qweight", "scales", "scaled_zeros", "oweight", "oweight_interleaved", "outlieridx")


def test_train_then_use(tmp_path, monkeypatch):
    """test_gpu_lm_head_nll_grad.py's test_train_then_use on the 3-bit model: the packed checkpoint round-trips bit for bit; one
    SGD step lowers the loss; after end() an engine built before refuses to run, the interleaved slabs the 3-bit GEMV reads hold the
    trained slices, new engines (v3 and round 1) agree with prefill on the trained weights and with fp64; save_finetuned ->
    from_packed round-trips the trained slices."""
    from qeft_amd import causal_lm_loss, checkpoint, finetune
    from qeft_amd.llama import DecodeEngine, QuantLlama, layer_linears, prefill
    from qeft_amd.qlinear import pack_oweight
    model, tokens = _new_model(), _tokens()[:T_SMALL]
    base = str(tmp_path / "w3" / "model.pth")
    checkpoint.save_packed(model, _infos(model), base)
    packed = QuantLlama.from_packed(base, device=DEV, max_seq=model.shape.max_seq, **HEADS)
    assert packed.shape.bits == 3 and packed.shape.n_out == 128 and packed.shape.n_kv_heads == 2
    for L0, L1 in zip(model.model.layers, packed.model.layers):
        for (nm, a), (_, b) in zip(layer_linears(L0), layer_linears(L1)):
            assert b.bits == 3 and b.qweight.dtype == torch.int32, nm
            for key in BUFFERS + (("reorder_ids",) if nm == "o_proj" else ()):
                assert torch.equal(getattr(a, key), getattr(b, key)), (nm, key)
    for key in ("model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"):
        assert torch.equal(model.state_dict()[key], packed.state_dict()[key]), key
    assert torch.equal(prefill(model, tokens), prefill(packed, tokens))

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
    print(f"[w3 model] train: loss {loss0.item():.6f} -> {loss1:.6f} after one SGD step")
    assert loss1 < loss0.item()
    finetune.end(model)
    assert model._prefill_ops is None
    with pytest.raises(RuntimeError, match="build a new DecodeEngine"):
        stale.step()
    changed = 0
    for L0, L1 in zip(model.model.layers, packed.model.layers):
        for (nm, a), (_, b) in zip(layer_linears(L0), layer_linears(L1)):
            trained = a.oweight.detach().half()
            changed += not torch.equal(trained, b.oweight)
            assert torch.equal(a.oweight_interleaved, pack_oweight(trained)), f"{nm}: the GEMV's slab is not the trained slice"
    assert changed > 0, "the step changed no outlier slice"
    ref64, l16 = logits_pair(model, tokens)                             # dense_weights() dequantises the trained slices
    logits = prefill(model, tokens)
    check_logits_and_nll("w3 trained prefill", logits.float(), ref64, l16, tokens)
    few = prefill(model, tokens[:16])                                   # 16 rows: gemv_3bit, which reads the interleaved slab
    check_logits_and_nll("w3 trained prefill, 16 rows", few.float(), ref64, l16, tokens, slice(0, 16))
    for v2 in (False, True):
        monkeypatch.delenv("QEFT_ENGINE_V2", raising=False)
        if v2:
            monkeypatch.setenv("QEFT_ENGINE_V2", "1")
        fresh = DecodeEngine(model, use_graph=False)
        assert fresh.v3 != v2
        got = fresh.teacher_forced_logits(tokens)
        assert (got - logits.float()).abs().max().item() <= 2e-2 * logits.float().abs().max().item()    # test_train_then_use's
        check_logits_and_nll(f"w3 trained engine {'round 1' if v2 else 'v3'}", got, ref64, l16, tokens)
    monkeypatch.delenv("QEFT_ENGINE_V2", raising=False)
    path = checkpoint.save_finetuned(model, base, str(tmp_path / "ft"))
    again = QuantLlama.from_packed(path, device=DEV, max_seq=model.shape.max_seq, **HEADS)
    for L0, L1 in zip(model.model.layers, again.model.layers):
        for (nm, a), (_, b) in zip(layer_linears(L0), layer_linears(L1)):
            assert b.bits == 3 and b.oweight.dtype == F16 and torch.equal(a.oweight.detach().half(), b.oweight), nm
            assert torch.equal(a.oweight_interleaved, b.oweight_interleaved), nm
    assert torch.equal(prefill(again, tokens), logits)


def test_fp8_kv_cache_on_the_3bit_engine():
    """Eager and captured bit for bit; against the fp16-cache 3-bit engine with the tolerance test_gpu_kv8.py applies to 4 bits
    (test_engine_accuracy_against_fp16_engine: 4 x its measured figures, taken from there)."""
    import test_gpu_kv8 as kv8
    from qeft_amd.llama import DecodeEngine, nll_from_logits
    model, tokens, _ = _infer()
    toks = tokens[:T_SMALL]
    e8 = DecodeEngine(model, use_graph=False, kv_dtype="fp8")
    assert e8.v3 and e8.bits == 3 and e8.kc[0].dtype == torch.uint8
    l8 = e8.teacher_forced_logits(toks)
    l8g = DecodeEngine(model, use_graph=True, kv_dtype="fp8").teacher_forced_logits(toks)
    assert torch.isfinite(l8).all() and torch.equal(l8, l8g)
    l16 = DecodeEngine(model, use_graph=True).teacher_forced_logits(toks)
    dl = (l8 - l16).abs().max().item()
    dn = abs(nll_from_logits(l8, toks) - nll_from_logits(l16, toks))
    print(f"[w3 model] fp8 cache: max|dlogit| = {dl:.6e} (max|logit| {l16.abs().max().item():.3f}, allowed {4 * kv8.MEASURED_DLOGIT:.3e})  "
          f"|dNLL| = {dn:.6e} (allowed {4 * kv8.MEASURED_DNLL:.3e})")
    assert dl <= 4 * kv8.MEASURED_DLOGIT, dl
    assert dn <= 4 * kv8.MEASURED_DNLL, dn


def test_the_4bit_only_passes_refuse_the_3bit_engine():
    from qeft_amd.assisted import PromptLookupDraft, assisted_generate
    from qeft_amd.batch import BatchDecodeEngine
    from qeft_amd.llama import DecodeEngine
    model, tokens, _ = _infer()
    eng = DecodeEngine(model, use_graph=False)
    assert eng.v3 and eng.bits == 3
    with pytest.raises(RuntimeError, match="the verify pass runs on 4-bit weights only"):
        eng.verify([1, 2])
    with pytest.raises(RuntimeError, match="batched decoding runs on 4-bit weights only"):
        BatchDecodeEngine(eng, max_batch=2)
    with pytest.raises(RuntimeError, match="the verify pass runs on 4-bit weights only"):
        assisted_generate(eng, PromptLookupDraft(), int(tokens[0]), 4, 3)
    assert eng.host_pos == 0
