"""Write tests/golden/attn_early_prefetch_parent.npz: the output bits of qeft_rope_attn_decode for every (layout, cache size,
position, split) of tests/test_gpu_attn_early_prefetch.py (same seeded operands), from the library that is loaded.

Run once, on the GPU, with the library of the commit whose bits are to be pinned (the one before the early prefetch):

    QEFT_HIP_LIB=/path/to/that/libqeft_hip.so python tests/golden/make_golden_attn_early.py [OUT.npz]

The test then holds every later build to those bits."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import numpy as np

import test_gpu_attn_early_prefetch as T

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
entries = {}
for heads, kv in T.LAYOUTS:
    for max_seq in T.MAX_SEQS:
        entries.update(T.golden_entries(heads, kv, max_seq))
np.savez_compressed(out, **entries)
from qeft_amd import _lib
print(f"{len(entries)} arrays from {_lib.LIB_PATH} -> {out} ({os.path.getsize(out)} bytes)")
