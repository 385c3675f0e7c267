"""QEFT on AMD: packed QuantLinear, the decode engines, prefill, scoring, the training loss and the per-linear calibration over
hand-written gfx950 kernels.

The scoring, fine-tuning and calibration entry points are exported here; they resolve on first use, so that `import qeft_amd` (and
`qeft_amd.build`, which runs before the library exists) stays free of torch and of the HIP library.
"""
_SCORING = ("score", "eval_nll", "lm_head_nll", "lm_head_nll_loss")
_FINETUNE = ("causal_lm_loss", "shift_labels", "pack_sequences", "train_step", "warmup_constant_lr")     # qeft_amd.finetune also has begin(model) / end(model)
_ATTENTION = ("causal_attention", "causal_attention_packed")
_GLUE = ("add_rmsnorm", "swiglu", "rope_qk")
_OPTIM = ("OWeightAdamW",)
_CALIBRATE = ("HessianAccumulator", "frob_norm_error", "select_outliers", "gptq_reorder", "calibrate_linear")
__all__ = [*_SCORING, *_FINETUNE, *_ATTENTION, *_GLUE, *_OPTIM, *_CALIBRATE]


def __getattr__(name):
    if name in _SCORING:
        from . import scoring
        return getattr(scoring, name)
    if name in _FINETUNE:
        from . import finetune
        return getattr(finetune, name)
    if name in _ATTENTION:
        from . import attention
        return getattr(attention, name)
    if name in _GLUE:
        from . import glue
        return getattr(glue, name)
    if name in _OPTIM:
        from . import optim
        return getattr(optim, name)
    if name in _CALIBRATE:
        from . import calibrate
        return getattr(calibrate, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
