"""CPU checks of sampled decoding: the Philox reference against Random123's known answers, the fp64 filter on hand-built rows,
SamplingParams, and the C entries' argument validation (before any device work)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from sampling_ref import cdf_interval, draw_u, filter_probs, philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_philox_known_answers(ctr, key, want):
    got = [int(x) for x in philox4x32_10(ctr, key)]
    assert got == want, [hex(x) for x in got]


def test_draw_u_uses_seed_halves_and_position():
    u, x0 = draw_u(0x0123456789abcdef, [0, 1, 2])
    for p in range(3):
        ref = philox4x32_10([p, 0, 0, 0], [0x89abcdef, 0x01234567])[0]
        assert int(x0[p]) == int(ref) and u[p] == int(ref) / 2 ** 32


# ---- the fp64 filter -------------------------------------------------------------------------------------------------------------
def test_top_k_keeps_every_tie_at_the_kth_value():
    l = np.array([1.0, 3.0, 2.0, 2.0, 2.0, 0.5])
    kept, pr, _ = filter_probs(l, 1.0, 2, 1.0)
    assert kept.tolist() == [False, True, True, True, True, False]
    assert abs(pr.sum() - 1) < 1e-12


def test_top_p_keeps_the_token_that_crosses():
    l = np.log(np.array([0.5, 0.3, 0.2]))
    kept, _, _ = filter_probs(l, 1.0, 0, 0.6)       # W(> 0.3) = 0.5 < 0.6: kept; W(> 0.2) = 0.8: cut
    assert kept.tolist() == [True, True, False]
    kept, _, _ = filter_probs(l, 1.0, 0, 0.5)       # W(> 0.3) = 0.5 is not below 0.5
    assert kept.tolist() == [True, False, False]


def test_tiny_top_p_keeps_the_maximum_and_its_ties():
    l = np.array([0.0, 2.0, 1.0, 2.0, -1.0])
    kept, pr, _ = filter_probs(l, 0.7, 0, 1e-6)
    assert kept.tolist() == [False, True, False, True, False]
    assert pr[1] == pr[3] == 0.5


def test_zero_temperature_is_the_argmax():
    l = np.array([0.0, 5.0, np.nan, 5.0, 1.0])
    kept, pr, _ = filter_probs(l, 0.0, 3, 0.5)
    assert kept.tolist() == [False, True, False, False, False] and pr[1] == 1
    assert filter_probs(np.array([np.nan, -np.inf]), 0.0, 0, 1.0)[0].tolist() == [True, False]     # as token_end: 0


def test_nan_is_never_kept():
    l = np.array([np.nan, 1.0, np.nan, 0.5, -np.inf])
    for T, k, p in [(1.0, 0, 1.0), (0.3, 2, 1.0), (1.7, 0, 0.95), (1.0, 4, 0.5)]:
        kept, pr, _ = filter_probs(l, T, k, p)
        assert not kept[0] and not kept[2] and pr[0] == pr[2] == 0
        assert pr[4] == 0 and abs(pr.sum() - 1) < 1e-12


def test_minus_zero_equals_plus_zero():
    l = np.array([-0.0, 0.0, -1.0])
    kept, pr, _ = filter_probs(l, 1.0, 1, 1.0)         # both zeros are the top value
    assert kept.tolist() == [True, True, False] and pr[0] == pr[1]


def test_cdf_interval():
    lo, hi = cdf_interval(np.array([0.25, 0.5, 0.25]), 1)
    assert (lo, hi) == (0.25, 0.75)


# ---- SamplingParams --------------------------------------------------------------------------------------------------------------
def test_sampling_params_validation():
    from qeft_amd.sampling import SamplingParams
    SamplingParams()
    SamplingParams(temperature=0, top_k=0, top_p=1.0, seed=0)
    SamplingParams(temperature=0.7, top_k=50, top_p=0.9, seed=2 ** 64 - 1)
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_k=-1),
                dict(top_p=0.0), dict(top_p=1.01), dict(top_p=-0.5), dict(top_p=float("nan")), dict(seed=-1), dict(seed=2 ** 64),
                dict(temperature=np.float32(-1)), dict(top_k=np.int64(-3))):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    for bad in (dict(top_k=1.5), dict(seed=1.0), dict(temperature="1"), dict(top_p=None), dict(top_k=True)):
        with pytest.raises(TypeError):
            SamplingParams(**bad)


def test_sampling_params_accept_numpy_scalars():
    from qeft_amd.sampling import SamplingParams
    p = SamplingParams(np.float32(0.7), np.int64(50), np.float64(0.9), np.uint64(2 ** 63 + 5))
    assert (p.temperature, p.top_k, p.top_p, p.seed) == (float(np.float32(0.7)), 50, 0.9, 2 ** 63 + 5)
    assert type(p.temperature) is float and type(p.top_k) is int and type(p.seed) is int
    assert p.record() == SamplingParams(float(np.float32(0.7)), 50, 0.9, 2 ** 63 + 5).record()


def test_tensor_parallel_engine_needs_an_explicit_seed():
    """Each rank would draw seed=None from its own generator: a tensor-parallel engine refuses it (before any device work)."""
    import types
    from qeft_amd.llama import DecodeEngine
    from qeft_amd.sampling import SamplingParams
    with pytest.raises(ValueError, match="explicit sampling seed"):
        DecodeEngine.set_sampling(types.SimpleNamespace(tp=True), SamplingParams(0.7))


def test_from_generation_config():
    from qeft_amd.sampling import SamplingParams
    g = SamplingParams.from_generation_config(False, 0.7, 50, 0.9)
    assert g.temperature == 0 and g.greedy
    s = SamplingParams.from_generation_config(True, 0.7, 50, 0.9, seed=5)
    assert (s.temperature, s.top_k, s.top_p, s.seed) == (0.7, 50, 0.9, 5)
    assert SamplingParams.from_generation_config(True, None, None, None) == SamplingParams()
    with pytest.raises(TypeError):
        SamplingParams.from_generation_config(True, 0.7)          # top_k must be given
    with pytest.raises(ValueError):
        SamplingParams.from_generation_config(True, -1.0, 0, 1.0)


def test_record_layout_and_seed_from_torch_generator():
    import struct
    from qeft_amd.sampling import SamplingParams
    r = SamplingParams(0.5, 40, 0.25, seed=0xfedcba9876543210).record()
    assert r[0] == struct.unpack("<i", struct.pack("<f", 0.5))[0] and r[1] == 40
    assert r[2] == struct.unpack("<i", struct.pack("<f", 0.25))[0]
    assert r[3] & 0xffffffff == 0x76543210 and r[4] & 0xffffffff == 0xfedcba98 and r[5:] == [0, 0, 0]
    assert SamplingParams(top_k=2 ** 40, seed=1).record()[1] == 2 ** 31 - 1
    with pytest.raises(ValueError):
        SamplingParams().record()
    torch.manual_seed(123)
    a = SamplingParams().resolved().seed
    torch.manual_seed(123)
    assert SamplingParams().resolved().seed == a and 0 <= a < 2 ** 64
    assert SamplingParams(seed=7).resolved().seed == 7


# ---- C entries -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from qeft_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_declares_the_sampling_entries_as_bound():
    from qeft_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeft_hip.h")).read(), flags=re.S)
    for name in ("qeft_sample", "qeft_token_end_sample", "qeft_token_end_sample_batch"):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name


def test_sampling_entries_reject_bad_arguments_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    s = lib.qeft_sample
    assert s(p, 32000, 0, p, p, p, None) == 1                   # m
    assert s(p, 0, 1, p, p, p, None) == 2                       # vocab
    assert s(None, 32000, 1, p, p, p, None) == 4
    assert s(p, 32000, 1, None, p, p, None) == 4
    assert s(p, 32000, 1, p, None, p, None) == 4
    assert s(p, 32000, 1, p, p, None, None) == 4
    assert s(p + 2, 32000, 1, p, p, p, None) == 6               # alignment of logits / params
    assert s(p, 32000, 1, p + 4, p, p, None) == 6
    e = lib.qeft_token_end_sample
    assert e(p, p, p, 0, p, None) == 2
    assert e(None, p, p, 100, p, None) == 4 and e(p, None, p, 100, p, None) == 4
    assert e(p, p, None, 100, p, None) == 4 and e(p, p, p, 100, None, None) == 4
    assert e(p + 8, p, p, 100, p, None) == 6 and e(p, p, p, 100, p + 8, None) == 6
    b = lib.qeft_token_end_sample_batch
    args = [p, p, p, p, p, p, p, p, p, p]
    assert b(*args, 100, 16, 8, 0, None) == 1 and b(*args, 100, 16, 8, 9, None) == 1
    assert b(*args, 0, 16, 8, 1, None) == 2 and b(*args, 100, 0, 8, 1, None) == 2 and b(*args, 100, 16, 0, 1, None) == 2
    for i in range(10):
        a = list(args)
        a[i] = None
        assert b(*a, 100, 16, 8, 1, None) == 4, i
    a = list(args)
    a[9] = p + 4
    assert b(*a, 100, 16, 8, 1, None) == 6
    a = list(args)
    a[0] = p + 2
    assert b(*a, 100, 16, 8, 1, None) == 6


def test_sample_wrapper_refuses_host_tensors():
    from qeft_amd.sampling import SamplingParams, sample
    with pytest.raises(ValueError):
        sample(torch.zeros(10, dtype=torch.float16), SamplingParams(seed=1), 0)
