"""QEFT on AMD: packed QuantLinear, the decode engines, prefill and scoring over hand-written gfx950 kernels.

The scoring entry points are exported here; they resolve on first use, so that `import qeft_amd` (and `qeft_amd.build`, which
runs before the library exists) stays free of torch and of the HIP library.
"""
__all__ = ["score", "eval_nll", "lm_head_nll"]


def __getattr__(name):
    if name in __all__:
        from . import scoring
        return getattr(scoring, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
