"""The whole-pass reference of tests/dense_ref.py against the model's own fp32 dense pass (QuantLlama.forward_dense_reference):
a sanity check of the helper, not of a kernel.  Both run over the same dense weights, so they differ by the fp32 pass's rounding
alone.  A loose first-order bound on that: every fp32 dot product of length K is off by at most K 2^-24 of its magnitude, and
along one path through the network the contraction lengths add up to

    C = n_layers (hidden [q|k|v] + T [softmax . v] + hidden [o_proj] + hidden [gate|up] + inter [down_proj]) + hidden [lm_head]

so |fp32 - fp64| <= C 2^-24 max|logit|, the gains of the layers taken as one (a wrong helper -- a missing o_proj gather, the
wrong rotary pairing, k / v heads not repeated -- is off by the size of the logits themselves)."""
import dataclasses

import pytest
import torch

from dense_ref import logits_pair, max_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("bits,gqa", [(4, False), (3, False), (4, True)])
def test_fp64_logits_agree_with_the_models_fp32_pass(bits, gqa):
    from qeft_amd.llama import LlamaShape, QuantLlama, tiny_shape
    if gqa:
        shape = LlamaShape(512, 512, 2, 4, 2, 384, 64, n_out=128, bits=bits, name="tiny-gqa")
    else:
        shape = dataclasses.replace(tiny_shape(n_layers=2, vocab=384), bits=bits)
    model = QuantLlama(shape, DEV, seed=11)
    T = 24
    tokens = torch.randint(0, shape.vocab, (T,), generator=torch.Generator().manual_seed(3)).to(DEV)
    dense = model.dense_weights()
    ref64, l16 = logits_pair(model, tokens, dense)
    ref32 = model.forward_dense_reference(tokens, dense)
    assert ref64.dtype == torch.float64 and ref64.shape == (T, shape.vocab) and torch.isfinite(ref64).all()
    C = shape.n_layers * (3 * shape.hidden + T + shape.inter) + shape.hidden
    top = ref64.abs().max().item()
    bound = C * 2.0 ** -24 * top
    e32, e16 = max_err(ref32, ref64), max_err(l16, ref64)
    print(f"[dense_ref] helper bits={bits} gqa={gqa}: max|fp32 - fp64| {e32:.3e} (bound {bound:.3e} = {C} 2^-24 x {top:.3f}); "
          f"fp16 torch pass {e16:.3e}")
    assert e32 <= bound
    assert e32 < e16                        # the fp16 mode rounds more coarsely than the fp32 pass
