"""The long one-token attention (qeft_rope_attn_decode_long) per split: one GPU, one process, HIP events, a
warm-up before every measurement, medians of --reps windows of back-to-back launches.

    python tools/bench_attn_decode_long.py [--reps 7] > profiles/attn_decode_long_bench.json.log

Head layouts (32, 32) and (64, 8), cache of 131072 rows, positions 2048 / 8192 (a long engine's early tokens) and 32768 / 65536 /
131071, every n_split 1 .. 64: microseconds
per launch and the fraction of 8 TB/s the K + V bytes of the context (2 x (pos + 1) x 256 bytes per kv head) come to.  The
table behind DecodeEngine._split_for's long route.  For information, with no pass mark: qeft_rope_attn_decode at max_seq 32768,
position 32767, 8 splits, against this kernel at max_seq 32784, same position.
Every point runs under its own time limit (a watchdog ends the process when a point overruns it) and the first failure ends the
run.  One JSON line per point; no threshold."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
HD = 128
PEAK = 8.0e12           # bytes / s of HBM3E on an MI355X


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner       # us per call


def median_us(fn, reps, inner, warm=2):
    for _ in range(warm):
        timed(fn, 1)
    return statistics.median(timed(fn, inner) for _ in range(reps))


class Case:
    def __init__(self, heads, kv, max_seq):
        from qeft_amd import _lib
        self.lib, self.ck = _lib.lib(), _lib.check
        self.heads, self.kv, self.max_seq = heads, kv, max_seq
        g = torch.Generator(device=DEV).manual_seed(heads + kv)
        self.qkv = torch.randn((heads + 2 * kv) * HD, generator=g, device=DEV).half()
        self.kc = torch.empty(kv, max_seq, HD, dtype=torch.float16, device=DEV).normal_(0, 0.5, generator=g)
        self.vc = torch.empty(kv, max_seq, HD, dtype=torch.float16, device=DEV).normal_(0, 0.5, generator=g)
        self.rope = torch.randn(1, 64, generator=g, device=DEV).repeat(1, 2)
        self.rope[:, :64].cos_()
        self.rope[:, 64:].sin_()
        self.out = torch.empty(heads * HD, dtype=torch.float16, device=DEV)
        self.ws = torch.zeros(max(self.lib.qeft_attn_long_workspace_bytes(heads, 64), self.lib.qeft_attn_workspace_bytes(heads, 8)) // 4,
                              device=DEV)
        self.pos = torch.zeros(1, dtype=torch.int32, device=DEV)

    def launch(self, entry, split):
        qp, st = self.qkv.data_ptr(), torch.cuda.current_stream().cuda_stream
        self.ck(entry(qp, qp + self.heads * HD * 2, qp + (self.heads + self.kv) * HD * 2, self.rope.data_ptr(),
                      self.rope.data_ptr() + 256, 1, self.kc.data_ptr(), self.vc.data_ptr(), self.pos.data_ptr(), None,
                      self.out.data_ptr(), self.ws.data_ptr(), split, self.heads, self.kv, self.max_seq, st))

    def point(self, entry, name, pos, split, reps):
        self.pos.fill_(pos)
        faulthandler.dump_traceback_later(120, exit=True)
        us = median_us(lambda: self.launch(entry, split), reps, inner=8)
        faulthandler.cancel_dump_traceback_later()
        nbytes = 2.0 * (pos + 1) * HD * 2 * self.kv
        print(json.dumps(dict(bench=name, heads=self.heads, kv=self.kv, max_seq=self.max_seq, pos=pos, n_split=split, reps=reps,
                              us=round(us, 1), kv_MB=round(nbytes / 1e6, 1), frac_of_8TBs=round(nbytes / (us * 1e-6) / PEAK, 3))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    print(json.dumps(dict(bench="attn_decode_long", device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    for heads, kv in ((32, 32), (64, 8)):
        c = Case(heads, kv, 131072)
        for pos in (2048, 8192, 32768, 65536, 131071):
            for split in (1, 2, 4, 8, 16, 32, 64):
                c.point(c.lib.qeft_rope_attn_decode_long, "attn_decode_long", pos, split, a.reps)
        del c
        torch.cuda.empty_cache()
        old, new = Case(heads, kv, 32768), Case(heads, kv, 32784)
        old.point(old.lib.qeft_rope_attn_decode, "attn_decode_at_the_ceiling", 32767, 8, a.reps)
        for split in (8, 16, 32, 64):
            new.point(new.lib.qeft_rope_attn_decode_long, "attn_decode_long_at_the_ceiling", 32767, split, a.reps)
        del old, new
        torch.cuda.empty_cache()
