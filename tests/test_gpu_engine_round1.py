"""The round-1 launch sequence of DecodeEngine on one GPU (DecodeEngine._launch_token below the v3 / tp3 early returns; DESIGN.md
section 4.4): token begin, q|k|v grouped GEMV, attention, o_proj GEMV + residual, gate|up grouped GEMV, down_proj GEMV with the
SiLU staging + residual, final norm, torch's lm_head matmul, token end, on an fp16 residual stream.  It runs for a checkpoint
whose n_out is not 0 or 128, whose group size is not 128, and under QEFT_ENGINE_V2=1.  The kernels are pinned one launch at a
time elsewhere (test_gpu_gemm_tiers.py, test_gpu_decode.py, test_gpu_w3.py); here the sequence that strings them together runs as
a whole, eager and captured, against a float64 dense pass (tests/dense_ref.py).

    case       shape                                            why round 1            q|k|v, gate|up     o_proj      down_proj
    n_out64    hidden 256, inter 512, g 128, n_out 64           v3 refuses n_out       gemv_valu_group    gemv_valu   gemv_valu_silu
    n_out256   hidden 512, inter 1024, 4 heads / 2 kv, n_out 256  v3 refuses n_out     gemv_mfma_group    gemv_mfma   gemv_mfma_silu
    group64    hidden 256, inter 512, g 64, n_out 128           v3 refuses the group   gemv_valu_group    gemv_valu   gemv_valu_silu
    v2_w4      hidden 256, inter 512, g 128, n_out 128          QEFT_ENGINE_V2=1       gemv_mfma_group    gemv_mfma   gemv_mfma_silu
    v2_w3      the same, bits 3                                 QEFT_ENGINE_V2=1       gemv_w3_group      gemv_w3     gemv_w3_silu

(the variants are gemv_w4.hip's, at both bit widths: mfma_ok() wants n_out % 128 == 0 and a group of 128 or K.)  The first three
cases are built WITHOUT the environment variable, so that the refusal of the v3 path is the shape's own.

Bounds: own error from fp64 <= 2 x the fp16 torch pass's + one fp16 ulp of the largest logit (the factor is the project's margin
over the fp16 torch pass, test_causal_lm_loss_on_the_tiny_model); the NLL likewise with that test's floor 2^-14; the two V2 cases
also against the v3 engine on the same model, <= 2 x its error + the ulp.  Sampling stays out of this file (_token_end is the v3
engine's too and is covered there)."""
import pytest
import torch

from dense_ref import bounded, check_logits_and_nll, logits_pair, max_err, ulp16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_TOK, T_PROMPT, N_GREEDY = 24, 9, 12

W4 = ("qeft_gemv_w4_group", "qeft_gemv_w4_fused", "qeft_gemv_w4_silu")
W3 = ("qeft_gemv_w3_group", "qeft_gemv_w3", "qeft_gemv_w3_silu")
VALU = ("gemv_valu_group", "gemv_valu", "gemv_valu_silu")
MFMA = ("gemv_mfma_group", "gemv_mfma", "gemv_mfma_silu")


def _shape(hidden=256, inter=512, heads=2, kv=2, **kw):
    from qeft_amd.llama import LlamaShape
    return LlamaShape(hidden, inter, 2, heads, kv, 384, 64, name="round1", **kw)


# case -> (shape arguments, QEFT_ENGINE_V2, entries, variants)
CASES = {
    "n_out64": (dict(n_out=64), False, W4, VALU),
    "n_out256": (dict(hidden=512, inter=1024, heads=4, kv=2, n_out=256), False, W4, MFMA),
    "group64": (dict(n_out=128, group_size=64), False, W4, VALU),
    "v2_w4": (dict(n_out=128), True, W4, MFMA),
    "v2_w3": (dict(n_out=128, bits=3), True, W3, ("gemv_w3_group", "gemv_w3", "gemv_w3_silu")),
}
_MADE = {}


def _case(name):
    """(model, tokens, ref64, logits16) of a case: made once, shared, never written."""
    if name not in _MADE:
        from qeft_amd.llama import QuantLlama
        model = QuantLlama(_shape(**CASES[name][0]), DEV, seed=5)
        tokens = torch.randint(0, model.shape.vocab, (T_TOK,), generator=torch.Generator().manual_seed(7)).to(DEV)
        _MADE[name] = (model, tokens) + logits_pair(model, tokens)
    return _MADE[name]


def _engine(name, monkeypatch, use_graph, v3=False, **kw):
    """The case's engine; the environment variable is read at construction.  v3=True: the v3 engine of the same model."""
    from qeft_amd.llama import DecodeEngine
    monkeypatch.delenv("QEFT_ENGINE_V2", raising=False)
    if CASES[name][1] and not v3:
        monkeypatch.setenv("QEFT_ENGINE_V2", "1")
    eng = DecodeEngine(_case(name)[0], use_graph=use_graph, **kw)
    assert eng.v3 == v3 and not eng.tp and not eng.tp3, f"{name}: v3 = {eng.v3}"
    return eng


class Recorder:
    """A stand-in for eng.lib that notes (entry, variant it dispatched to) after every call."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        from qeft_amd import _lib
        fn = getattr(self._lib, name)

        def call(*a):
            rc = fn(*a)
            self._log.append((name, _lib.last_variant()))
            return rc
        return call


@pytest.mark.parametrize("name", list(CASES))
def test_the_launches_that_run(name, monkeypatch):
    """One eager token reaches exactly the entries _launch_token lists, in its order, and every GEMV entry dispatches to the
    variant of the table (the entries between them set no variant of their own)."""
    eng = _engine(name, monkeypatch, use_graph=False)
    model, tokens = _case(name)[:2]
    group, fused, silu = CASES[name][2]
    vg, vf, vs = CASES[name][3]
    log = []
    eng.lib = Recorder(eng.lib, log)
    eng.reset()
    eng.tok.fill_(int(tokens[0]))
    eng.step()
    torch.cuda.synchronize()
    layer = [(group, vg), ("qeft_rope_attn_decode", None), (fused, vf), (group, vg), (silu, vs)]
    want = [("qeft_token_begin", None)] + layer * model.shape.n_layers + [("qeft_rmsnorm", None), ("qeft_token_end", None)]
    print(f"[round1] {name}: " + " ".join(f"{e[5:]}:{v}" if e in CASES[name][2] else e[5:] for e, v in log))
    assert [e for e, _ in log] == [e for e, _ in want]
    assert [(e, v) for e, v in log if e in CASES[name][2]] == [(e, v) for e, v in want if v is not None]


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_teacher_forced_logits_against_fp64(name, use_graph, monkeypatch):
    model, tokens, ref64, l16 = _case(name)
    eng = _engine(name, monkeypatch, use_graph)
    got = eng.teacher_forced_logits(tokens)
    tag = f"round1 {name} {'graph' if use_graph else 'eager'}"
    e_own, e_16 = check_logits_and_nll(tag, got, ref64, l16, tokens)
    if CASES[name][1]:
        e_v3 = max_err(_engine(name, monkeypatch, use_graph, v3=True).teacher_forced_logits(tokens), ref64)
        bounded(tag + " vs the v3 engine", e_own, e_v3, ulp16(ref64.abs().max().item()))


@pytest.mark.parametrize("name", list(CASES))
def test_graph_equals_eager_bit_for_bit(name, monkeypatch):
    """Teacher-forced logits, twelve greedy tokens one run(1) at a time, and run(12) (on the graph engine: one captured graph of
    MULTI tokens, then single steps) end in the same tokens and the same logits."""
    model, tokens = _case(name)[:2]
    ea, gr = _engine(name, monkeypatch, False), _engine(name, monkeypatch, True)
    assert torch.equal(ea.teacher_forced_logits(tokens), gr.teacher_forced_logits(tokens))
    seqs = []
    for eng in (ea, gr):
        eng.reset()
        eng.greedy = True
        eng.tok.fill_(int(tokens[0]))
        seq = []
        for _ in range(N_GREEDY):
            eng.run(1)
            seq.append(int(eng.tok.item()))
        seqs.append(seq)
    assert seqs[0] == seqs[1], (name, seqs)
    last = ea.logits.clone()
    for eng in (ea, gr):
        eng.reset()
        eng.tok.fill_(int(tokens[0]))
        eng.run(N_GREEDY)
        assert eng.host_pos == N_GREEDY and int(eng.pos.item()) == N_GREEDY
        assert int(eng.tok.item()) == seqs[0][-1] and torch.equal(eng.logits, last), f"{name}: run({N_GREEDY}) ends elsewhere"
    assert any(len(k) == 3 for k in gr.graphs), "run(12) captured no multi-token graph"


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_prefill_hands_over_to_the_round1_engine(name, use_graph, monkeypatch):
    """prefill() of 9 tokens into the engine's caches, the rest stepped: the teacher-forced rows >= 9 within the same bound."""
    from qeft_amd.llama import prefill
    model, tokens, ref64, l16 = _case(name)
    eng = _engine(name, monkeypatch, use_graph)
    prefill(model, tokens[:T_PROMPT], engine=eng)
    assert eng.host_pos == T_PROMPT and int(eng.pos.item()) == T_PROMPT
    rows = []
    for t in tokens[T_PROMPT:].tolist():
        eng.tok.fill_(t)
        eng.step()
        rows.append(eng.logits[0].float().clone())
    tag = f"round1 {name} {'graph' if use_graph else 'eager'} hand-over"
    check_logits_and_nll(tag, torch.stack(rows), ref64, l16, tokens, slice(T_PROMPT, T_TOK))
