"""Sampled decoding: temperature, top-k and top-p with a counter-based RNG, drawn on the device.

A sequence's `SamplingParams` become a parameter record of 8 int32 words in device memory (csrc/decode_sample.hip): temperature
(fp32 bits), top_k, top_p (fp32 bits), seed lo, seed hi and 3 reserved zeros.  The kernel applies HF's warpers in their order
(temperature, top-k, top-p; ties at either boundary kept by value) and draws with Philox4x32-10 keyed by the seed at counter
(p, 0, 0, 0), p being the position the drawn token will occupy.  So a token depends on its logits, its record and its position
only: it is reproducible, independent of the other rows of a batch, and the same inside or outside a captured graph.
Temperature 0 is greedy decoding, bit-identical to the argmax token end.
"""
import dataclasses
import math
import numbers
import struct

import torch

from . import _lib

RECORD_WORDS = 8


def _f32_bits(x):
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


@dataclasses.dataclass(frozen=True)
class SamplingParams:
    """temperature: finite, >= 0 (0: greedy); top_k: >= 0 (0 or >= vocab: off); top_p: in (0, 1] (1: off); seed: an integer in
    [0, 2^64) or None (drawn from torch's default generator when a sequence is admitted or the parameters are set)."""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = None

    def __post_init__(self):
        # any real / integral number (numpy scalars included) is accepted and stored as a Python float / int
        t, k, p, s = self.temperature, self.top_k, self.top_p, self.seed
        if isinstance(t, bool) or not isinstance(t, numbers.Real):
            raise TypeError(f"temperature must be a real number, got {type(t).__name__}")
        if isinstance(k, bool) or not isinstance(k, numbers.Integral):
            raise TypeError(f"top_k must be an integer, got {type(k).__name__}")
        if isinstance(p, bool) or not isinstance(p, numbers.Real):
            raise TypeError(f"top_p must be a real number, got {type(p).__name__}")
        if s is not None and (isinstance(s, bool) or not isinstance(s, numbers.Integral)):
            raise TypeError(f"seed must be an integer or None, got {type(s).__name__}")
        t, k, p, s = float(t), int(k), float(p), (int(s) if s is not None else None)
        if not math.isfinite(t) or t < 0:
            raise ValueError(f"temperature must be finite and >= 0, got {t!r}")
        if k < 0:
            raise ValueError(f"top_k must be >= 0, got {k!r}")
        if not 0 < p <= 1:
            raise ValueError(f"top_p must lie in (0, 1], got {p!r}")
        if s is not None and not 0 <= s < 2 ** 64:
            raise ValueError(f"seed must lie in [0, 2^64), got {s!r}")
        for name, v in (("temperature", t), ("top_k", k), ("top_p", p), ("seed", s)):
            object.__setattr__(self, name, v)

    @property
    def greedy(self):
        return self.temperature == 0

    @classmethod
    def from_generation_config(cls, do_sample, temperature, top_k, top_p, seed=None):
        """HF's generation settings (do_sample, temperature, top_k, top_p).  do_sample=False is greedy (temperature 0).  top_k
        has no default here: HF's default of 50 is not this project's (0, off), so callers say which one they mean.  None for
        temperature / top_k / top_p means off (1.0 / 0 / 1.0)."""
        if not do_sample:
            return cls(temperature=0.0, top_k=0, top_p=1.0, seed=seed)
        return cls(temperature=1.0 if temperature is None else float(temperature), top_k=0 if top_k is None else int(top_k),
                   top_p=1.0 if top_p is None else float(top_p), seed=seed)

    def resolved(self):
        """These parameters with a seed: a None seed is drawn (64 bits) from torch's default generator."""
        if self.seed is not None:
            return self
        lo, hi = (int(x) for x in torch.randint(0, 2 ** 32, (2,), dtype=torch.int64))
        return dataclasses.replace(self, seed=lo | hi << 32)

    def record(self):
        """The 8-word parameter record (Python ints, int32 range) of these parameters; the seed must be set (resolved())."""
        if self.seed is None:
            raise ValueError("the record needs a seed: call resolved() first")
        lo, hi = self.seed & 0xffffffff, self.seed >> 32
        as_i32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v       # noqa: E731
        return [_f32_bits(self.temperature), min(self.top_k, 2 ** 31 - 1), _f32_bits(self.top_p), as_i32(lo), as_i32(hi), 0, 0, 0]


GREEDY_RECORD = [0] * RECORD_WORDS          # temperature 0: the argmax


def records(params, m):
    """int32 [m][8] host tensor of m rows' records; params: one SamplingParams (every row) or a list of m (None: greedy)."""
    ps = list(params) if isinstance(params, (list, tuple)) else [params] * m
    if len(ps) != m:
        raise ValueError(f"{len(ps)} parameter sets for {m} rows")
    return torch.tensor([p.resolved().record() if p is not None else GREEDY_RECORD for p in ps], dtype=torch.int32)


@torch.no_grad()
def sample(logits, params, positions):
    """Tokens (int64 [m], on the logits' device) drawn from fp16 logits [m][vocab] (or one row [vocab]) on the GPU with
    qeft_sample.  params: a SamplingParams or a list of m; positions: an int or m ints, the positions the drawn tokens will
    occupy.  A row that is not 16-byte aligned (or not contiguous) is copied into an aligned buffer first."""
    if not logits.is_cuda:
        raise ValueError("sample() runs on the GPU: logits must be a CUDA tensor")
    if logits.dtype != torch.float16:
        raise ValueError(f"sample() takes fp16 logits, got {logits.dtype}")
    x = logits.unsqueeze(0) if logits.dim() == 1 else logits
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"logits must be [vocab] or [m][vocab], got {tuple(logits.shape)}")
    m, vocab = x.shape
    if not x.is_contiguous() or x.data_ptr() % 16:
        x = x.clone(memory_format=torch.contiguous_format)       # the caching allocator's blocks are 512-byte aligned
    pos = [int(positions)] * m if isinstance(positions, int) else [int(p) for p in torch.as_tensor(positions).flatten().tolist()]
    if len(pos) != m:
        raise ValueError(f"{len(pos)} positions for {m} rows")
    dev = x.device
    rec = records(params, m).to(dev)
    pos_d = torch.tensor(pos, dtype=torch.int32).to(dev)
    out = torch.empty(m, dtype=torch.long, device=dev)
    lib = _lib.lib()
    _lib.check(lib.qeft_sample(x.data_ptr(), vocab, m, rec.data_ptr(), pos_d.data_ptr(), out.data_ptr(),
                               torch.cuda.current_stream(dev).cuda_stream))
    return out
