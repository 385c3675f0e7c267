"""Golden vector for the calibrator: the REFERENCE's own GPTQ_OWQ run on the CPU on one small layer.

    PYTHONPATH=/root/reference python tests/golden/make_golden_calib.py       (build container only)

add_batch per sample, hessian_sorting with the Frobenius term of main.py:132-138, fasterquant_reorder(percdamp=.01,
groupsize=128) with Quantizer(4, perchannel=True, mse=False, group_size=128)  (recon.py:35-100, 488-573).  The reference calls
torch.cuda.synchronize() inside the loop; it is replaced by a no-op here so that the run needs no GPU.  The layer is
tests/calib_ref.make_case(0): N = 32, K = 256, r = 64 (192 live columns: one full and one half block), 4 samples x 96 tokens.
The fixture holds data only: W, X, H, the Frobenius term, out_ids, the reference's ids, Q, scale_group, zero_group -- and, for
the record, the reference's proxy loss over round-to-nearest on this recipe's other seeds is printed, not stored.
calib_mse0.npz: one group's rows and what the reference's MSE parameter search returns for them at 4 and 3 bits.
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
torch.cuda.synchronize = lambda *a, **k: None
from qeft.quant import Quantizer  # noqa: E402
from qeft.recon import GPTQ_OWQ  # noqa: E402

import calib_ref as R  # noqa: E402


def run_reference(W, X, r):
    n, k = W.shape
    lin = nn.Linear(k, n, bias=False)
    lin.weight.data = W.float().clone()
    g = GPTQ_OWQ(lin, n_out=r)
    g.quantizer = Quantizer(4, perchannel=True, sym=False, mse=False, group_size=128)
    for j in range(X.shape[0]):
        g.add_batch(X[j].unsqueeze(0), None)
    H = g.H.clone()
    tq = Quantizer(4, perchannel=True, sym=False, mse=False, group_size=128)
    W0 = W.float()
    tq.find_params(W0, weight=True, num=40)
    frob = (W0 - tq.quantize(W0)).pow(2).sum(dim=0)
    out_ids = g.hessian_sorting(actorder=False, frob_norm=frob, outidx=None)
    ids = g.ids.clone()
    g.fasterquant_reorder(percdamp=.01, groupsize=128, actorder=False)
    return dict(H=H, frob=frob, out_ids=out_ids, ids=ids, Q=lin.weight.data.clone(), scale_group=g.quantizer.scale_group.clone(),
                zero_group=g.quantizer.zero_group.clone())


def main():
    for seed, shape in [(0, {}), (1, {}), (2, {}), (3, {}), (4, dict(N=72, K=384, r=128))]:
        W, X, hot = R.make_case(seed, **shape)
        k, r = W.shape[1], len(hot)
        ref = run_reference(W, X, r)
        H64 = R.hessian64(X)
        ids = R.dense_ids(ref["out_ids"], k)
        ratio = R.proxy_loss(W, ref["Q"], H64) / R.proxy_loss(W[:, ids], R.rtn(W[:, ids], k - r), H64[ids][:, ids])
        print(f"seed {seed}: reference picked the scaled channels: {bool((ref['out_ids'].long() == hot).all())}; "
              f"reference proxy loss / RTN = {ratio:.3f}")
        if seed == 0:
            np.savez_compressed(os.path.join(HERE, "calib_case0.npz"), W=W.numpy(), X=X.numpy(), H=ref["H"].numpy(),
                                frob=ref["frob"].numpy(), out_ids=ref["out_ids"].numpy(), ids=ref["ids"].numpy(),
                                Q=ref["Q"].numpy(), scale_group=ref["scale_group"].numpy(), zero_group=ref["zero_group"].numpy(),
                                hot=hot.numpy())
            print("wrote calib_case0.npz")


def main_mse():
    """The reference's MSE parameter search (Quantizer.find_params(mse=True, num=40), quant.py:87-141) on one group of 128
    columns, 4 and 3 bits: the rows of make_case(0)'s first group, one of them zeroed and one made one-sided."""
    W, _, _ = R.make_case(0)
    x = W[:16, :128].float().clone()
    x[3] = 0
    x[5] = x[5].abs()
    out = dict(x=x.numpy())
    for bits in (4, 3):
        q = Quantizer(bits, perchannel=True, sym=False, mse=True, group_size=128)
        q.find_params(x, weight=True, num=40)
        out[f"scale{bits}"], out[f"zero{bits}"] = q.scale.numpy(), q.zero.numpy()
    np.savez_compressed(os.path.join(HERE, "calib_mse0.npz"), **out)
    print("wrote calib_mse0.npz")


if __name__ == "__main__":
    main()
    main_mse()
