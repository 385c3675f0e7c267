"""GPU checks of sampled assisted decoding (qeft_verify_sample in csrc/decode_sample.hip, DecodeEngine.verify_sample,
assisted_generate(..., sampling=)).

Kernel level, all exact: the draws implied by the outputs equal qeft_sample on the same rows at p0 + i + 1 and the outputs equal
accepted_prefix on them for every n; T = 0 equals qeft_verify_greedy bit for bit; graph replays equal eager calls (the ticket
re-arms); the smallest shapes run with every operand in an allocation of its own.

Engine level (2-layer 7B and 70B shapes): every token verify_sample emits is qeft_sample's draw on its logits_m row; the stream of
assisted_generate(sampling=) is the stream of the one-row sampled engine with the same record, for every draft and k, except
where rounding between the m-row and the one-row launch explains a difference.  The bound is derived, not tuned: with P1, Pm the
fp64 reference distributions of the one-row and the m-row logits of a position, every index-order CDF value differs by at most
TV(P1, Pm); the one-row engine draws d where u lies in d's interval under P1, so a different token under Pm needs u within
TV(P1, Pm) (+ 1e-6 for the kernels' fixed-point weights, the tolerance of the existing sampled-run check) of an edge of that
interval.  Any other mismatch fails; and the share of positions whose u lies in such an edge zone must be <= 1/4 per case."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sampling_ref import cdf_interval, draw_u, filter_probs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from qeft_amd import _lib
    return _lib.lib(), _lib.check


def _f32(x):
    return float(np.float32(x))


def _rec(T, k, p, seed):
    from qeft_amd.sampling import SamplingParams
    return SamplingParams(T, k, p, seed).record()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _draws(lgd, rec, positions):
    """qeft_sample on device rows lgd [m][vocab] with one record at the given positions -> list of m tokens."""
    lib, ck = _lib()
    m, vocab = lgd.shape
    recs, pos = _i32([rec] * m), _i32(list(positions))
    out = torch.full((m,), -7, dtype=torch.long, device=DEV)
    ck(lib.qeft_sample(lgd.data_ptr(), vocab, m, recs.data_ptr(), pos.data_ptr(), out.data_ptr(), _st()))
    torch.cuda.synchronize()
    return out.tolist()


class _Call:
    """Operands of one qeft_verify_sample call (out_tokens pre-filled with -1)."""

    def __init__(self, lgd, tokens, rec, p0, work=None):
        self.lgd, self.m = lgd, len(tokens)
        self.toks = torch.tensor(tokens, dtype=torch.long, device=DEV)
        self.rec = _i32(rec)
        self.work = work if work is not None else torch.zeros(16, dtype=torch.int32, device=DEV)
        self.out = torch.full((8,), -1, dtype=torch.long, device=DEV)
        self.n, self.tok, self.pos = _i32([-3]), torch.full((1,), -5, dtype=torch.long, device=DEV), _i32([p0])

    def launch(self):
        lib, ck = _lib()
        ck(lib.qeft_verify_sample(self.lgd.data_ptr(), self.toks.data_ptr(), self.m, self.lgd.shape[1], self.rec.data_ptr(),
                                  self.work.data_ptr(), self.out.data_ptr(), self.n.data_ptr(), self.tok.data_ptr(),
                                  self.pos.data_ptr(), _st()))

    def result(self):
        torch.cuda.synchronize()
        return int(self.n.item()), self.out.tolist(), int(self.tok.item()), int(self.pos.item())


def _rows8(vocab, g):
    """8 fp16 rows: random, ties on three values, a dominant logit, all equal, NaN / -inf / -0 entries, random again"""
    rows = [torch.randn(vocab, generator=g) * 2, torch.randint(0, 3, (vocab,), generator=g).float() * -0.5,
            torch.randn(vocab, generator=g) * 0.5, torch.full((vocab,), 0.25), torch.randn(vocab, generator=g) * 1.5,
            torch.randn(vocab, generator=g) * 2, torch.randn(vocab, generator=g), torch.randn(vocab, generator=g) * 3]
    rows[2][vocab // 3] = 12.0
    rows[4][torch.randint(0, vocab, (max(1, vocab // 50),), generator=g)] = float("nan")
    rows[4][torch.randint(0, vocab, (max(1, vocab // 50),), generator=g)] = float("-inf")
    rows[4][torch.randint(0, vocab, (max(1, vocab // 100),), generator=g)] = -0.0
    return torch.stack(rows).half()


RECORDS = [(1.0, 0, 1.0), (0.8, 40, 1.0), (1.3, 0, 0.9), (0.7, 50, 0.95), (0.0, 0, 1.0)]


@pytest.mark.parametrize("vocab", [32000, 32001, 511, 128256])
def test_kernel_equals_sample_and_accepted_prefix(vocab):
    from qeft_amd.assisted import accepted_prefix
    g = torch.Generator().manual_seed(vocab + 1)
    base = _rows8(vocab, g)
    work = torch.zeros(16, dtype=torch.int32, device=DEV)        # one buffer through every call: the ticket re-arms
    n_calls = 0
    for ri, (T, k, p) in enumerate(RECORDS):
        rec = _rec(T, k, p, 0xabc0_0000_0000_0000 + 7919 * ri + vocab)
        for p0 in (0, 57 + ri, 4000):
            perm = torch.randperm(8, generator=g).tolist()
            lgd = base[perm].to(DEV)
            a = _draws(lgd, rec, [p0 + i + 1 for i in range(8)])
            for m in range(1, 9):
                for n_want in range(m):
                    # drafts from the draws: right up to n_want, wrong there, right again behind it (must not be accepted)
                    toks = [3] + a[:m - 1]
                    if n_want < m - 1:
                        toks[n_want + 1] = (a[n_want] + 1) % vocab
                    c = _Call(lgd[:m], toks, rec, p0, work)
                    c.launch()
                    n, out, tok, pos = c.result()
                    n_calls += 1
                    rn, racc = accepted_prefix(a[:m], toks)
                    assert rn == n_want
                    assert (n, out[:n + 1], tok, pos) == (rn, racc, racc[-1], p0 + rn + 1), (vocab, T, k, p, p0, m, n_want)
                    assert out[n + 1:] == [-1] * (7 - n)
                    w = work.tolist()
                    assert w[:m] == a[:m] and w[8:] == [0] * 8, (vocab, m, w)      # the header's contract for `work`
    assert n_calls == len(RECORDS) * 3 * 36


@pytest.mark.parametrize("vocab", [1000, 32000, 1003, 128256])
def test_zero_temperature_equals_verify_greedy_bit_for_bit(vocab):
    lib, ck = _lib()
    g = torch.Generator().manual_seed(vocab + 2)
    rec = _rec(0.0, 40, 0.5, 77)
    for m in range(1, 9):
        lg = (torch.randn(m, vocab, generator=g) * 2).half()
        lg[: m // 2, 17] = 30.0                         # a tie between 17 and 900: the lower index wins
        lg[: m // 2, 900] = 30.0
        if m > 2:
            lg[2, 5] = float("nan")
        if m > 5:
            lg[5] = float("-inf")                       # no value above -inf: token 0
        lgd = lg.to(DEV)
        am = _draws(lgd, rec, list(range(m)))
        for case in ("all", "none", "partial"):
            toks = [3] + am[:m - 1]
            if case == "none":
                toks = [3] + [(t + 1) % vocab for t in am[:m - 1]]
            elif case == "partial" and m > 2:
                toks[m // 2 + 1] = (toks[m // 2 + 1] + 5) % vocab
            c = _Call(lgd, toks, rec, 10)
            c.launch()
            got = c.result()
            out = torch.full((8,), -1, dtype=torch.long, device=DEV)
            n, tok, pos = _i32([-3]), torch.full((1,), -5, dtype=torch.long, device=DEV), _i32([10])
            ck(lib.qeft_verify_greedy(lgd.data_ptr(), c.toks.data_ptr(), m, vocab, 1, out.data_ptr(), n.data_ptr(), tok.data_ptr(),
                                      pos.data_ptr(), _st()))
            torch.cuda.synchronize()
            assert got == (int(n.item()), out.tolist(), int(tok.item()), int(pos.item())), (vocab, m, case)


def test_graph_replays_equal_eager_calls():
    """4 calls in one captured graph (m = 8, 3, 5, 1 on one `work` buffer and one position word), replayed 10 times, against the
    same 40 calls made eagerly: the position advances by n + 1 per call, so every call draws at new positions."""
    vocab = 32000
    g = torch.Generator().manual_seed(9)
    lgd = (torch.randn(8, vocab, generator=g) * 0.7).half().to(DEV)
    rec = _rec(0.6, 3, 1.0, 31337)
    first = _draws(lgd, rec, list(range(1, 9)))
    ms = (8, 3, 5, 1)

    def calls():
        work = torch.zeros(16, dtype=torch.int32, device=DEV)
        cs = [_Call(lgd[:m], [3] + first[:m - 1], rec, 0, work) for m in ms]
        for c in cs[1:]:
            c.pos, c.tok = cs[0].pos, cs[0].tok         # one sequence: a shared position and token word
        return cs, work
    (ea, wa), (gr, wg) = calls(), calls()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):                      # warm-up launches outside the capture
        for c in gr:
            c.launch()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    gr[0].pos.fill_(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for c in gr:
            c.launch()
    ns = set()
    for rep in range(10):
        for c in ea:
            c.launch()
        graph.replay()
        torch.cuda.synchronize()
        for c, d in zip(ea, gr):
            assert c.result() == d.result(), rep
            ns.add(c.result()[0])
        assert wa.tolist() == wg.tolist() and wg.tolist()[8:] == [0] * 8
    assert ea[0].pos.item() > 40 and len(ns) > 1       # (the drafts are right at position 0 only: n varies over the calls)


# The smallest shapes with every operand in an exact-size allocation of its own (a child process with
# PYTORCH_NO_CUDA_MEMORY_CACHING=1, as tests/test_gpu_zz_alloc_guard.py): a read or write past the rows, the tokens, the record,
# `work` or an output would reach the end of its mapping.  vocab 1 and 7 (register-held keys, the scalar tail path), 8 (one
# vector load) and 32769 (the re-reading form, odd length); m = 1, 2 and 8; everything accepted and nothing accepted.
ALLOC_CHILD = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import torch
from qeft_amd import _lib
from qeft_amd.assisted import accepted_prefix
from qeft_amd.sampling import SamplingParams
lib, ck = _lib.lib(), _lib.check
DEV = "cuda:0"
st = lambda: torch.cuda.current_stream().cuda_stream
i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
g = torch.Generator().manual_seed(78)
for vocab in (1, 7, 8, 32769):
    for m in (1, 2, 8):
        for T, k, p in ((0.0, 0, 1.0), (1.0, 3, 0.8), (0.5, 0, 1.0)):
            lg = (torch.randn(m, vocab, generator=g) * 2).half().to(DEV)
            rec = i32(SamplingParams(T, k, p, seed=99).record())
            recs, pos_m = i32([SamplingParams(T, k, p, seed=99).record()] * m), i32([5 + i for i in range(m)])
            a_d = torch.full((m,), -7, dtype=torch.long, device=DEV)
            ck(lib.qeft_sample(lg.data_ptr(), vocab, m, recs.data_ptr(), pos_m.data_ptr(), a_d.data_ptr(), st()))
            torch.cuda.synchronize()
            a = a_d.tolist()
            for wrong in (False, True):
                toks = [0] + [(t + 1) %% max(vocab, 2) if wrong else t for t in a[:m - 1]]
                tk = torch.tensor(toks, dtype=torch.long, device=DEV)
                work, out = i32([0] * 16), torch.full((m,), -1, dtype=torch.long, device=DEV)
                n, tok, pos = i32([-3]), torch.full((1,), -5, dtype=torch.long, device=DEV), i32([4])
                ck(lib.qeft_verify_sample(lg.data_ptr(), tk.data_ptr(), m, vocab, rec.data_ptr(), work.data_ptr(), out.data_ptr(),
                                          n.data_ptr(), tok.data_ptr(), pos.data_ptr(), st()))
                torch.cuda.synchronize()
                rn, racc = accepted_prefix(a, toks)
                assert (n.item(), out.tolist()[:rn + 1], tok.item(), pos.item()) == (rn, racc, racc[-1], 5 + rn), (vocab, m, T, wrong)
                assert work.tolist()[:m] == a and work.tolist()[8] == 0
print("VERIFY-SAMPLE-GUARD-OK")
'''


def test_smallest_shapes_in_own_allocations():
    env = dict(os.environ, PYTORCH_NO_CUDA_MEMORY_CACHING="1")
    out = subprocess.run([sys.executable, "-c", ALLOC_CHILD % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "VERIFY-SAMPLE-GUARD-OK" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])


# ---- the engine ------------------------------------------------------------------------------------------------------------------
PROMPT = [11, 4021, 977, 15002, 31000, 8, 2600, 19999, 123]
T0, FIRST, N = len(PROMPT), 5150, 56
# The record of the engine cases.  The edge-zone condition is on the inputs: with (T 0.8, top-k 40, top-p 0.95) the share was
# 0.11-0.21 on the 7B shapes but 0.29 on the 70B shapes (lookup, k = 1), above the 1/4 the cases must stay under.  Fewer kept
# tokens mean fewer CDF edges for u to fall next to, so the cases run with top-k 12 at T 0.7, top-p 0.9.
SP = dict(temperature=0.7, top_k=12, top_p=0.9, seed=20261016)


@pytest.fixture(scope="module", params=["7b", "70b"])
def model2(request):
    from qeft_amd.llama import LLAMA2_7B, LLAMA2_70B, QuantLlama
    base = {"7b": LLAMA2_7B, "70b": LLAMA2_70B}[request.param]
    shape = dataclasses.replace(base, n_layers=2, max_seq=256, name=base.name + "-2layers")
    model = QuantLlama(shape, DEV, seed=3, fast_init=True)
    yield request.param, model
    del model
    torch.cuda.empty_cache()


def _engine_with_prompt(model):
    """A graph engine whose cache holds PROMPT, fed by one-row steps (the way a draft engine feeds its context)."""
    from qeft_amd.llama import DecodeEngine
    eng = DecodeEngine(model, use_graph=True)
    eng.reset()
    eng.set_sampling(None)
    eng.greedy = False
    for t in PROMPT:
        eng.tok.fill_(t)
        eng.step()
    return eng


def _record_passes(eng):
    """Wrap eng.verify_sample: per pass (host_pos before, tokens, n, accepted, logits_m rows 0..n)."""
    passes, inner = [], eng.verify_sample

    def wrapped(tokens):
        p = eng.host_pos
        n, acc = inner(tokens)
        passes.append((p, [int(t) for t in tokens], n, acc, eng.logits_m[:n + 1].clone()))
        return n, acc
    eng.verify_sample = wrapped
    return passes


def _one_row_along(eng1, sp, stream):
    """Teacher-force the one-row engine along FIRST + stream with the record set: per position its draw and its logits row."""
    eng1.set_position(T0)
    eng1.greedy = False
    eng1.set_sampling(sp)
    draws, rows = [], []
    for x in [FIRST] + stream[:-1]:
        eng1.tok.fill_(x)
        eng1.step()
        draws.append(int(eng1.tok.item()))
        rows.append(eng1.logits[0].clone())
    eng1.set_sampling(None)
    return draws, rows


def _check_stream(label, sp, stream, rows_m, draws, rows_1):
    """The rule of the module docstring over one emitted stream.  Returns the positions that mismatched (all admissible)."""
    T, k, p = _f32(sp.temperature), sp.top_k, _f32(sp.top_p)
    u, _ = draw_u(sp.seed, [T0 + j + 1 for j in range(len(stream))])
    zone, mism, bad = 0, [], []
    for j, t in enumerate(stream):
        _, p1, _ = filter_probs(rows_1[j].cpu().double().numpy(), T, k, p)
        _, pm, _ = filter_probs(rows_m[j].cpu().double().numpy(), T, k, p)
        tol = 0.5 * np.abs(p1 - pm).sum() + 1e-6
        cdf = np.cumsum(p1)
        d_ref = int(min(np.searchsorted(cdf, u[j], side="right"), np.nonzero(p1)[0][-1]))
        lo, hi = cdf_interval(p1, d_ref)
        zone += min(u[j] - lo, hi - u[j]) <= tol
        if draws[j] != t:
            lo, hi = cdf_interval(p1, draws[j])
            near = min(abs(u[j] - lo), abs(u[j] - hi))
            mism.append(j)
            if near > tol:
                bad.append((j, t, draws[j], float(u[j]), float(lo), float(hi), float(tol)))
    share = zone / len(stream)
    print(f"[verify_sample {label}] edge-zone share {share:.3f} ({zone}/{len(stream)}), mismatches at {mism}")
    assert not bad, (label, bad[:4])
    assert share <= 0.25, (label, share)
    return mism


def test_verify_sample_tokens_are_the_kernels_draws(model2):
    """Every token a pass emits is qeft_sample's draw on the matching logits_m row at its position (exact), lies in the fp64
    reference's kept set and has u inside its CDF interval +- 1e-6.  Drafts: the one-row sampled stream with every third one
    spoiled, so that n takes many values; m = 1..8; eager and graph give the same."""
    from qeft_amd.assisted import accepted_prefix
    from qeft_amd.sampling import SamplingParams
    name, model = model2
    sp = SamplingParams(**SP)
    eng = _engine_with_prompt(model)
    with pytest.raises(RuntimeError, match="set_sampling"):
        eng.verify_sample([FIRST])
    eng.set_sampling(sp)
    eng.set_position(T0)
    eng.tok.fill_(FIRST)
    one_row = []
    for _ in range(N):                                   # the one-row sampled stream: the source of the drafts
        eng.step()
        one_row.append(int(eng.tok.item()))
    streams = []
    ms = [1, 8, 4, 8, 2, 7, 3, 8, 5, 6, 8, 8]
    for use_graph in (True, False):
        eng.use_graph = use_graph
        eng.set_position(T0)
        ctx, out, sizes = [FIRST], [], []
        for pi, m in enumerate(ms):
            drafts = []
            for i in range(m - 1):
                j = len(out) + i
                t = one_row[j] if j < N else 0
                drafts.append((t + 1) % model.shape.vocab if j % 6 == 5 else t)      # every sixth one spoiled
            p0 = eng.host_pos
            toks = [ctx[-1]] + drafts
            n, acc = eng.verify_sample(toks)
            rows = eng.logits_m[:m].clone()
            assert eng.host_pos == p0 + n + 1 == int(eng.pos.item()) and int(eng.tok.item()) == acc[-1]
            a = _draws(rows, sp.record(), [p0 + i + 1 for i in range(m)])
            assert (n, acc) == accepted_prefix(a, toks), (name, pi, m)
            u, _ = draw_u(sp.seed, [p0 + i + 1 for i in range(n + 1)])
            for i, t in enumerate(acc):
                kept, pr, _ = filter_probs(rows[i].cpu().double().numpy(), _f32(sp.temperature), sp.top_k, _f32(sp.top_p))
                lo, hi = cdf_interval(pr, t)
                assert kept[t] and lo - 1e-6 <= u[i] <= hi + 1e-6, (name, pi, i)
            sizes.append(n)
            out += acc
            ctx += acc
        streams.append(out)
        if use_graph:
            assert {kk for kk in eng.graphs if kk[0] == "verify"} == {("verify", m, 1, "sample") for m in set(ms)}
        print(f"[verify_sample {name}] graph={use_graph}: accepted per pass {sizes}")
    assert streams[0] == streams[1]
    eng.use_graph = True
    eng.set_sampling(None)


class _Replay:
    def __init__(self, stream, wrong=False, vocab=32000):
        self.s, self.wrong, self.vocab = stream, wrong, vocab

    def propose(self, ctx, k):
        j = len(ctx) - 1 - T0                            # index into the stream of the token after ctx[-1]
        return [(t + 1) % self.vocab if self.wrong else t for t in self.s[j:j + k]]


def test_stream_identity_and_coupling(model2):
    from qeft_amd.assisted import EngineDraft, PromptLookupDraft, assisted_generate
    from qeft_amd.llama import DecodeEngine
    from qeft_amd.sampling import SamplingParams
    name, model = model2
    vocab = model.shape.vocab
    sp = SamplingParams(**SP)
    eng, eng1 = _engine_with_prompt(model), _engine_with_prompt(model)
    passes = _record_passes(eng)

    def generate(draft, k):
        del passes[:]
        eng.set_position(T0)
        out, acc = assisted_generate(eng, draft, FIRST, N, k, context=PROMPT, sampling=sp)
        torch.cuda.synchronize()
        assert len(out) == N and eng.sampling is None
        assert acc == [ps[2] for ps in passes]
        rows_m = [r for ps in passes for r in ps[4]][:N]
        return out, acc, rows_m

    # the one-row sampled stream: the replay draft's first recording
    eng1.set_position(T0)
    eng1.set_sampling(sp)
    eng1.tok.fill_(FIRST)
    one_row = []
    for _ in range(N):
        eng1.step()
        one_row.append(int(eng1.tok.item()))
    eng1.set_sampling(None)

    draft_eng = DecodeEngine(model, use_graph=True)
    rates = {}
    for k in (1, 4, 7):
        for kind in ("lookup", "replay", "wrong", "coupled"):
            label = f"{name} {kind} k={k}"
            if kind == "lookup":
                out, acc, rows_m = generate(PromptLookupDraft(), k)
            elif kind in ("wrong", "replay"):
                # the recorded stream is the one this very pass structure emits: start from the one-row stream and, where an
                # m-row rounding changed a token, record the emitted stream and replay that (each run fixes the stream up to its next such position).
                # At the fixed point every replayed draft is the token the target draws, and every spoiled one is not.
                rec_stream = one_row
                for _ in range(12):
                    out, acc, rows_m = generate(_Replay(rec_stream, wrong=kind == "wrong", vocab=vocab), k)
                    if out == rec_stream:
                        break
                    rec_stream = out
                assert out == rec_stream, label
                offered = [len(ps[1]) - 1 for ps in passes]
                assert max(offered) == k and acc == (offered if kind == "replay" else [0] * N), (label, acc, offered)
            else:
                d = EngineDraft(draft_eng)
                out, acc, rows_m = generate(d, k)
                assert d.sampling is None
            draws, rows_1 = _one_row_along(eng1, sp, out)
            mism = _check_stream(label, sp, out, rows_m, draws, rows_1)
            if kind == "coupled":
                # a rejected draft is the one-row engine's draw at that position (same model, same record, same history), so
                # each rejection is a mismatch position of the check above: admissible by the rounding rule, or it has failed
                rejected = [(ps[0] + ps[2] + 1 - T0 - 1, ps[1][ps[2] + 1]) for ps in passes if ps[2] < len(ps[1]) - 1]
                for j, q in rejected:
                    assert q == draws[j] and j in mism, (label, j, q, draws[j])
                offered = sum(len(ps[1]) - 1 for ps in passes)
                rates[k] = (sum(acc) / offered, len(rejected))
    # the control: the same draft engine with a seed of its own
    class Independent(EngineDraft):
        def set_sampling(self, params):
            super().set_sampling(dataclasses.replace(params, seed=params.seed ^ 0x5555_5555) if params is not None else None)
    for k in (4, 7):
        out, acc, rows_m = generate(Independent(draft_eng), k)
        offered = sum(len(ps[1]) - 1 for ps in passes)
        indep = sum(acc) / offered
        print(f"[verify_sample {name}] k={k}: acceptance coupled {rates[k][0]:.3f} ({rates[k][1]} rejected), independent seed {indep:.3f}")
        assert indep < rates[k][0], (name, k, indep, rates[k])
        draws, rows_1 = _one_row_along(eng1, sp, out)
        _check_stream(f"{name} independent k={k}", sp, out, rows_m, draws, rows_1)


def test_greedy_verify_is_untouched_by_a_sampled_run(model2):
    from qeft_amd.assisted import PromptLookupDraft, assisted_generate
    from qeft_amd.sampling import SamplingParams
    name, model = model2
    eng = _engine_with_prompt(model)

    def greedy():
        eng.set_position(T0)
        out, acc = assisted_generate(eng, PromptLookupDraft(), FIRST, 24, 4, context=PROMPT)
        lg_a = eng.logits_m[:1].clone()                  # (row 0 is written by every pass; later rows may be an earlier pass's)
        eng.set_position(T0)
        eng.greedy = True
        res = eng.verify([FIRST] + out[:7])
        torch.cuda.synchronize()
        return out, acc, lg_a, res, eng.logits_m.clone(), int(eng.tok.item())
    before = greedy()
    keys = set(eng.graphs)
    assert all(kk[0] != "verify" or kk[3] is True for kk in keys) and ("verify", 8, 1, True) in keys
    eng.set_position(T0)
    out, _ = assisted_generate(eng, PromptLookupDraft(), FIRST, 24, 4, context=PROMPT, sampling=SamplingParams(**SP))
    assert eng.sampling is None and out != before[0]
    new = set(eng.graphs) - keys
    assert new and all(kk[0] == "verify" and kk[3] == "sample" for kk in new), new
    # verify() with sampling set is still the greedy pass, on the greedy graph
    eng.set_sampling(SamplingParams(**SP))
    eng.set_position(T0)
    eng.greedy = True
    assert eng.verify([FIRST] + before[0][:7]) == before[3]
    eng.set_sampling(None)
    after = greedy()
    assert set(eng.graphs) - new == keys
    assert before[0] == after[0] and before[1] == after[1] and before[3] == after[3] and before[5] == after[5]
    assert torch.equal(before[2], after[2]) and torch.equal(before[4], after[4])
