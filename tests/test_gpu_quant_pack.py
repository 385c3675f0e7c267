"""Tests of the device quantise-and-pack kernel (qeft_quant_pack, csrc/quant_pack.hip; qeft_cuda.quant_pack,
QuantLinear.pack_device, calibrate_linear(pack="device"), rtn_linear).

The oracle of the packed buffers is QuantLinear.pack on the CPU, compared with torch.equal; the one of the found parameters is
quant.minmax_params over each group's live columns, compared as bits.  Weights are fp16 N(0, 0.02^2).  Shapes (N, K, n_out):
one and three row sets, one live group and several, a group without a live column, a short last group (n_out = 32, 4 bits only).

The last test is the CPU's: refusals only -- no call hands the launching entry a complete set of valid arguments."""
import functools
import types

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(16, 256, 0), (16, 256, 128), (48, 384, 32), (32, 384, 128)]
CASES = [(4, *s) for s in SHAPES] + [(3, *s) for s in SHAPES if s[2] % 128 == 0]
BUFFERS = ("qweight", "scales", "scaled_zeros", "oweight", "oweight_interleaved")


@functools.lru_cache(maxsize=None)
def layer(bits, N, K, n_out):
    """CPU: (raw fp16 W with an all-zero and an all-positive group, the min-max (scale, zero) fp32 [N, K / 128] of each group's
    live columns -- a group without one repeats the last -- and W fake-quantised with them, the last n_out columns raw)."""
    from qeft_amd.quant import minmax_params, quantize
    W = (torch.randn(N, K, generator=torch.Generator().manual_seed(N + K + n_out)) * 0.02).half()
    W[0, :128] = 0
    W[1, :128] = W[1, :128].abs() + 0.001
    live = K - n_out
    par = [minmax_params(W[:, c:min(c + 128, live)], min(c + 128, live) - c, bits) for c in range(0, live, 128)]
    par += [par[-1]] * (K // 128 - len(par))
    scale, zero = (torch.cat([p[i] for p in par], 1) for i in range(2))
    s, z = (torch.repeat_interleave(t, 128, dim=1)[:, :live] for t in (scale, zero))
    fq = W.clone()
    fq[:, :live] = quantize(W[:, :live].float(), s, z, 0, 2 ** bits - 1).half()
    return W, scale, zero, fq


def packed(bits, W, scale, zero, n_out, device, **kw):
    from qeft_amd.qlinear import QuantLinear
    N, K = W.shape
    m = QuantLinear(bits, K, N, False, torch.float16, n_out, 128, True, "q_proj")
    holder = types.SimpleNamespace(weight=types.SimpleNamespace(data=W.to(device)), bias=None)
    ids = torch.arange(K - n_out, K, dtype=torch.int32)
    if device == "cpu":
        m.pack(holder, scale, zero, ids)
    else:
        to = lambda t: None if t is None else t.to(device)
        m.found = m.to(device).pack_device(holder, to(scale), to(zero), ids, **kw)
    return m


def assert_same_buffers(dev_module, host_module, n_out):
    for name in BUFFERS[:3 if n_out == 0 else 5]:
        a, b = getattr(dev_module, name).cpu(), getattr(host_module, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name


@gpu
@pytest.mark.parametrize("bits,N,K,n_out", CASES)
def test_given_mode_equals_the_host_pack(bits, N, K, n_out):
    _, scale, zero, fq = layer(bits, N, K, n_out)
    assert_same_buffers(packed(bits, fq, scale, zero, n_out, DEV), packed(bits, fq, scale, zero, n_out, "cpu"), n_out)


@gpu
@pytest.mark.parametrize("bits,N,K,n_out", CASES)
def test_find_mode_equals_minmax_and_the_host_pack(bits, N, K, n_out):
    W, scale, zero, fq = layer(bits, N, K, n_out)
    m = packed(bits, W, None, None, n_out, DEV)
    for found, want in zip(m.found, (scale, zero)):
        assert torch.equal(found.cpu().view(torch.int32), want.view(torch.int32))
    assert_same_buffers(m, packed(bits, fq, scale, zero, n_out, "cpu"), n_out)


@gpu
@pytest.mark.parametrize("bits,N,K,n_out", [(4, 48, 384, 32), (3, 32, 384, 128)])
def test_col_ids_equals_the_gathered_matrix(bits, N, K, n_out):
    from qeft_amd import qeft_cuda
    from qeft_amd.reorder import sparse_to_dense_ids
    W = layer(bits, N, K, n_out)[0].to(DEV)
    out_ids = torch.sort(torch.randperm(K, generator=torch.Generator().manual_seed(K))[:n_out])[0].to(torch.int32)
    ids = sparse_to_dense_ids(out_ids, K).to(DEV)
    plain = qeft_cuda.quant_pack(W[:, ids].contiguous(), n_out=n_out, bits=bits)
    gathered = qeft_cuda.quant_pack(W, n_out=n_out, bits=bits, col_ids=ids.to(torch.int32))
    for a, b in zip(gathered, plain):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@gpu
def test_calibrate_linear_packs_the_same_on_the_device():
    from qeft_amd.calibrate import HessianAccumulator, calibrate_linear
    N, K, n_out = 64, 256, 32
    lin = torch.nn.Linear(K, N, bias=True).half().to(DEV)
    acc = HessianAccumulator(K, DEV).add_batch(torch.randn(2, 300, K, generator=torch.Generator().manual_seed(1)).half().to(DEV))
    host, dev = (calibrate_linear(lin, acc.H, n_out, "q_proj", pack=p)[0].state_dict() for p in ("host", "device"))
    assert list(host) == list(dev)
    for key in host:
        assert host[key].device == dev[key].device and host[key].dtype == dev[key].dtype and torch.equal(host[key], dev[key]), key


@gpu
@pytest.mark.parametrize("n_out", [0, 32])
def test_rtn_linear_forward_against_fp64(n_out):
    """m = 1 against x . Wfq^T in fp64, Wfq the fake-quantised weights in `ids` order as the math oracle of SURVEY section 8-c
    states them (q s16 + sz16, the fp16 pair a packed layer holds; the codes q recomputed here from the returned fp32
    parameters); 1e-3 of the largest output, that section's kernel-vs-oracle bound."""
    from qeft_amd import rtn_linear
    N, K, maxq = 64, 256, 15
    g = torch.Generator().manual_seed(7 + n_out)
    lin = torch.nn.Linear(K, N, bias=False).half()
    lin.weight.data = (torch.randn(N, K, generator=g) * 0.02).half()
    H = torch.diag(torch.rand(K, generator=g) + 0.1)
    module, info = rtn_linear(lin.to(DEV), n_out, "q_proj", H=H.to(DEV))
    ids = info.ids.cpu()
    Wp = lin.weight.data.cpu()[:, ids].float()
    live = K - n_out
    assert info.out_ids.numel() == n_out and info.scale_group.shape == (N, K // 128) and module.qweight.is_cuda
    s, z = (torch.repeat_interleave(t.cpu(), 128, dim=1)[:, :live] for t in (info.scale_group, info.zero_group))
    q = torch.clamp(torch.round(Wp[:, :live] / s) + z, 0, maxq)
    Wp[:, :live] = q * s.half().float() + (-(z * s)).half().float()
    x = torch.randn(1, K, generator=g).half()
    y = module(x[:, ids].to(DEV)).cpu().double()
    ref = x[:, ids].double() @ Wp.double().t()
    err = ((y - ref).abs().max() / ref.abs().max()).item()
    print(f"rtn_linear n_out = {n_out}: relative error {err:.3g} (bound 1e-3)")
    assert err < 1e-3
    with pytest.raises(ValueError, match="tuning"):
        rtn_linear(lin, n_out, "q_proj", H=H.to(DEV), tuning="mse")


def test_refusals_without_a_gpu():
    """SHAPE, then GROUP, then NULL, then ALIGN; every call below has something wrong."""
    import qeft_amd
    from qeft_amd import _lib, build, qeft_cuda
    build.build(verbose=False)
    lib = _lib.lib()
    ERR_SHAPE, ERR_GROUP, ERR_NULL, ERR_ALIGN, P = 2, 3, 4, 6, 1 << 20
    def call(w=P, ids=None, s=None, z=None, q=2 * P, sc=3 * P, sz=4 * P, so=None, zo=None, n=32, k=256, ld=256, n_out=0, bits=4, g=128):
        return lib.qeft_quant_pack(w, ld, ids, s, z, q, sc, sz, so, zo, n, k, n_out, bits, g, None)
    for bad in (dict(bits=2), dict(bits=8), dict(n=24), dict(n=0), dict(k=192, ld=192), dict(ld=248), dict(ld=260), dict(n_out=33),
                dict(n_out=256), dict(n_out=-2), dict(bits=3, n_out=32), dict(n=(1 << 20) + 16)):
        assert call(**bad) == ERR_SHAPE and call(**bad, w=None, q=None) == ERR_SHAPE, bad
    assert call(g=64) == ERR_GROUP and call(g=256) == ERR_GROUP and call(g=64, w=None) == ERR_GROUP
    for name in ("w", "q", "sc", "sz"):
        assert call(**{name: None}) == ERR_NULL, name
    assert call(s=P) == ERR_NULL and call(z=P) == ERR_NULL                # the given parameters come as a pair
    assert call(w=P + 8) == ERR_ALIGN and call(q=2 * P + 8) == ERR_ALIGN and call(sc=3 * P + 1) == ERR_ALIGN
    assert call(so=5 * P + 2) == ERR_ALIGN and call(ids=6 * P + 2, ld=260) == ERR_ALIGN
    assert "rtn_linear" in qeft_amd.__all__ and "quant_pack.hip" in build.SOURCES and "quant_pack.h" in build.HEADERS
    with pytest.raises(RuntimeError, match="GPU"):                        # no CPU path and no torch fallback
        qeft_cuda.quant_pack(torch.zeros(16, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="GPU"):
        qeft_amd.rtn_linear(torch.nn.Linear(128, 16).half(), 0, "q_proj")
