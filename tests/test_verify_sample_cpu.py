"""CPU-only checks of sampled assisted decoding: qeft_verify_sample is declared, exported and bound as declared, rejects bad
arguments without a device, compiles without scratch; assisted_generate(..., sampling=) on a host-side engine that implements
verify_sample from the fp64 / Philox references emits the reference's token stream for any draft and any k, restores the engine's
sampling state, and stays greedy-only without the keyword."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from sampling_ref import draw_u, filter_probs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qeft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ERR_BATCH, ERR_SHAPE, ERR_NULL, ERR_ALIGN = 1, 2, 4, 6


@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_symbol_declared_exported_and_bound(lib):
    from qeft_amd import _lib
    text = open(os.path.join(ROOT, "include", "qeft_hip.h")).read()
    assert re.search(r"#define\s+QEFT_VERIFY_SAMPLE_WORK\s+16\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bqeft_verify_sample\s*\(([^)]*)\)", text)
    assert m and hasattr(lib, "qeft_verify_sample")
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES["qeft_verify_sample"]) == 11


def test_bad_arguments_rejected_before_the_device(lib):
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    v = lib.qeft_verify_sample
    for m in (0, 9, -1):
        assert v(None, None, m, 1000, None, None, None, None, None, None, None) == ERR_BATCH
        assert v(p, p, m, 1000, p, p, p, p, p, p, None) == ERR_BATCH
    assert v(p, p, 4, 0, p, p, p, p, p, p, None) == ERR_SHAPE
    ptrs = [0, 1, 4, 5, 6, 7, 8, 9]                  # logits, tokens, params, work, out_tokens, n_accepted, tok, pos
    for i in ptrs:
        a = [p, p, 4, 1000, p, p, p, p, p, p, None]
        a[i] = None
        assert v(*a) == ERR_NULL, i
    assert v(p + 2, p, 4, 1000, p, p, p, p, p, p, None) == ERR_ALIGN
    assert v(p, p, 4, 1000, p + 4, p, p, p, p, p, None) == ERR_ALIGN


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_verify_sample_kernels_have_no_scratch(tmp_path):
    out = tmp_path / "decode_sample.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-kernarg-preload-count=16",
                    "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "decode_sample.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    found = 0
    for blk in open(out).read().split(".name:")[1:]:
        if "verify_sample_kernel" not in blk.split()[0]:
            continue
        vals = {k: int(x) for k, x in re.findall(r"\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", blk[:1500])}
        if vals:
            found += 1
            assert not any(vals.values()), (blk.split()[0], vals)
    assert found == 2               # the register-resident and the re-reading form


# ---- a host-side engine: logits are a fixed function of (position, token at that position), the draw is the reference's ---------
VOCAB = 48


def _row(p, t):
    return np.random.default_rng(1000 * p + t).standard_normal(VOCAB).astype(np.float16).astype(np.float64) * 2


def _ref_draw(row, sp, p):
    """The reference's token: index-order inverse CDF of the fp64 filter at the Philox uniform of (seed, p)."""
    kept, pr, _ = filter_probs(row, float(np.float32(sp.temperature)), sp.top_k, float(np.float32(sp.top_p)))
    if sp.temperature == 0:
        return int(np.nonzero(kept)[0][0])
    u, _ = draw_u(sp.seed, [p])
    return int(min(np.searchsorted(np.cumsum(pr), u[0], side="right"), np.nonzero(kept)[0][-1]))


class FakeEngine:
    VERIFY_MAX = 8

    def __init__(self, max_seq=512):
        import types
        self.m = types.SimpleNamespace(shape=types.SimpleNamespace(max_seq=max_seq))
        self.host_pos, self.sampling, self.greedy, self.calls = 0, None, False, []

    def set_sampling(self, params):
        self.sampling = params.resolved() if params is not None else None

    def verify_sample(self, tokens):
        from qeft_amd.assisted import accepted_prefix
        assert self.sampling is not None and 1 <= len(tokens) <= self.VERIFY_MAX
        a = [_ref_draw(_row(self.host_pos + i, t), self.sampling, self.host_pos + i + 1) for i, t in enumerate(tokens)]
        n, acc = accepted_prefix(a, tokens)
        self.calls.append(len(tokens))
        self.host_pos += n + 1
        return n, acc

    def verify(self, tokens):
        raise AssertionError("the sampled loop must not run the greedy verify pass")


def _ref_stream(sp, first, p0, n):
    out, t = [], first
    for p in range(p0, p0 + n):
        t = _ref_draw(_row(p, t), sp, p + 1)
        out.append(t)
    return out


class Replay:
    def __init__(self, stream, p0, wrong=False):
        self.s, self.p0, self.wrong = stream, p0, wrong

    def propose(self, ctx, k):
        j = len(ctx) - 1 - self.p0                        # index into the stream of the token after ctx[-1]
        return [(t + 1) % VOCAB if self.wrong else t for t in self.s[j:j + k]]


class Noise:
    def __init__(self, stream, p0, seed):
        self.s, self.p0, self.rng = stream, p0, random.Random(seed)

    def propose(self, ctx, k):
        j = len(ctx) - 1 - self.p0
        return [t if self.rng.random() < 0.7 else self.rng.randrange(VOCAB) for t in self.s[j:j + self.rng.randrange(0, k + 1)]]


@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 0, 1.0), (0.8, 10, 0.9), (1.3, 0, 0.7), (0.0, 5, 0.5)])
def test_sampled_assisted_stream_is_the_reference_stream_for_any_draft(T, top_k, top_p):
    from qeft_amd.assisted import PromptLookupDraft, assisted_generate
    from qeft_amd.sampling import SamplingParams
    sp = SamplingParams(T, top_k, top_p, seed=0x1234_5678_9abc_def0)
    first, p0, N = 5, 9, 64
    context = list(range(p0))
    ref = _ref_stream(sp, first, p0, N)
    for k in (0, 1, 4, 7, 12):
        for name, draft in (("replay", Replay(ref, p0)), ("wrong", Replay(ref, p0, wrong=True)), ("noise", Noise(ref, p0, k)),
                            ("lookup", PromptLookupDraft())):
            eng = FakeEngine()
            eng.host_pos = p0
            out, acc = assisted_generate(eng, draft, first, N, k, context=context, sampling=sp)
            assert out == ref, (k, name)
            assert len(acc) == len(eng.calls) and sum(acc) + len(acc) >= N and max(eng.calls) <= min(k, 7) + 1
            if name == "wrong":
                assert acc == [0] * N
            if name == "replay":
                assert all(a == c - 1 for a, c in zip(acc, eng.calls)), (k, acc)
            assert eng.sampling is None


def test_engine_and_draft_sampling_state_is_restored():
    from qeft_amd.assisted import assisted_generate
    from qeft_amd.sampling import SamplingParams
    import torch
    prev = SamplingParams(0.5, 3, 1.0, seed=1)
    seen = []

    class Draft:
        sampling = "before"

        def set_sampling(self, params):
            self.sampling = params
            seen.append(params)

        def propose(self, ctx, k):
            return []
    eng, d = FakeEngine(), Draft()
    eng.set_sampling(prev)
    torch.manual_seed(7)
    out, _ = assisted_generate(eng, d, 3, 10, 4, sampling=SamplingParams(0.9, 0, 1.0))      # seed=None: drawn once
    assert eng.sampling == prev and d.sampling == "before"
    assert seen[0].seed is not None and out == _ref_stream(seen[0], 3, 0, 10)        # the draft got the resolved record

    class Boom:
        def propose(self, ctx, k):
            raise KeyError("draft failed")
    eng = FakeEngine()
    eng.set_sampling(prev)
    with pytest.raises(KeyError):
        assisted_generate(eng, Boom(), 3, 10, 4, sampling=SamplingParams(0.9, seed=2))
    assert eng.sampling == prev


def test_without_the_keyword_it_is_greedy_only():
    from qeft_amd.assisted import assisted_generate
    from qeft_amd.sampling import SamplingParams
    eng = FakeEngine()
    eng.set_sampling(SamplingParams(0.9, seed=2))
    with pytest.raises(ValueError):
        assisted_generate(eng, Replay([], 0), 3, 4, 3)
    with pytest.raises(ValueError):
        assisted_generate(eng, Replay([], 0), 3, 4, 3, sampling=None)


def test_engine_draft_draws_with_its_record_and_feeds_teacher_forced():
    """EngineDraft on a host-side engine: the context is fed with sampling off, the proposals are stepped with the record set."""
    from qeft_amd.assisted import EngineDraft
    from qeft_amd.sampling import SamplingParams
    import types

    class Tok:
        v = 0

        def fill_(self, t):
            self.v = t

        def item(self):
            return self.v

    class Eng:
        def __init__(self):
            self.m = types.SimpleNamespace(shape=types.SimpleNamespace(max_seq=64))
            self.tok, self.pos, self.sampling, self.greedy, self.log = Tok(), 0, None, False, []

        def reset(self):
            self.pos = 0

        def set_position(self, p):
            self.pos = p

        def set_sampling(self, params):
            self.sampling = params

        def step(self):
            self.log.append((self.pos, self.tok.v, self.sampling, self.greedy))
            if self.sampling is not None:
                self.tok.v = _ref_draw(_row(self.pos, self.tok.v), self.sampling, self.pos + 1)
            self.pos += 1
    sp = SamplingParams(0.9, 12, 0.95, seed=77)
    d = EngineDraft(Eng())
    d.set_sampling(sp)
    ctx = [4, 8, 15, 16]
    got = d.propose(ctx, 3)
    assert got == _ref_stream(sp, 16, 3, 3)                  # the draws a target with the same logits would make at 4, 5, 6
    assert [(p, t, s) for p, t, s, _ in d.eng.log[:3]] == [(0, 4, None), (1, 8, None), (2, 15, None)]
    assert all(s == sp for _, _, s, _ in d.eng.log[3:]) and len(d.eng.log) == 6
    d.set_sampling(None)
    d.propose(ctx + got[:1], 2)
    assert all(s is None for _, _, s, _ in d.eng.log[6:]) and d.eng.log[-1][3] is True
