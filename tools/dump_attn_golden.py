"""Write tests/golden/attn_decode_parent.npz: output bits and appended k / v rows of qeft_rope_attn_decode for every case of
tests/test_gpu_attn_overlap.py (same fixture, same seeds), from the library that is loaded.

Run once, on the GPU, with the library of the commit whose bits are to be pinned:

    QEFT_HIP_LIB=/path/to/that/libqeft_hip.so python tools/dump_attn_golden.py [OUT.npz]

The test then holds every later build to those bits."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import test_gpu_attn_overlap as T

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
entries = {}
for heads, kv in T.LAYOUTS:
    entries.update(T.golden_entries(heads, kv))
np.savez_compressed(out, **entries)
from qeft_amd import _lib
print(f"{len(entries)} arrays from {_lib.LIB_PATH} -> {out} ({os.path.getsize(out)} bytes)")
