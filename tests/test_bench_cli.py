"""bench.py's command line and its --dump-outputs writer (host only; the timed path itself runs in the GPU suite's engine tests)."""
import types

import numpy as np
import torch

import bench


def test_plain_run_is_the_default_and_takes_steps_as_given():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.full, a.dump_outputs, a.gpus, a.steps, a.warmup) == (False, None, 1, 7, 3)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_writes_the_last_steps_logits_and_token(tmp_path):
    eng = types.SimpleNamespace(logits=torch.randn(1, 1000, generator=torch.Generator().manual_seed(0)).half(),
                                tok=torch.tensor([31999]))
    bench.dump_outputs(str(tmp_path / "out"), eng)
    logits = np.load(tmp_path / "out" / "logits.npy")
    tok = np.load(tmp_path / "out" / "next_token.npy")
    assert logits.dtype == np.float32 and logits.shape == (1, 1000)
    assert np.array_equal(logits, eng.logits.float().numpy())
    assert tok.dtype == np.float64 and tok.tolist() == [31999.0]
