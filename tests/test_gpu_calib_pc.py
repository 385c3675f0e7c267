"""Per-channel grids (group_size=-1): qeft_gptq_rows_pc / _pc_mse (csrc/calib_rows.hip), qeft_quant_pack_pc
(csrc/quant_pack.hip) and gptq_reorder / calibrate_linear / rtn_linear(group_size=-1).  Layers, the identity's derived bound and the
search's criteria with G = 1e-4 are test_gpu_gptq_rows' and test_gpu_mse_search's (G needs gamma(n_nonout) + 1e-6 < G / 2: up to
640 columns); the oracle of the packed buffers is QuantLinear.pack on the CPU with scales [N, 1], compared with torch.equal."""
import types

import pytest
import torch

import calib_ref as R
from test_gpu_gptq_rows import _placed, assert_identity, golden, layer  # noqa: F401  (golden is a fixture)
from test_gpu_mse_search import G, bits_of, candidates
from test_gpu_quant_pack import assert_same_buffers

gpu = pytest.mark.gpu
DEV = "cuda:0"


def run_rows_pc(W0, U, nn, maxq, num=None):
    """One launch through the C entry, placed as run_rows places it: NaN around W0, a NaN guard row under every output."""
    from qeft_amd import _lib
    n, k = W0.shape
    (wi, wo), u = _placed(W0, n + 2, k + 8, 1, 4), U.contiguous().to(DEV)
    w = wi.to(DEV)
    q, err, s, z = (torch.full((n + 1, cols), float("nan"), device=DEV) for cols in (k, nn, 1, 1))
    args = (w.data_ptr() + 4 * wo, k + 8, u.data_ptr(), k, q.data_ptr(), err.data_ptr(), s.data_ptr(), z.data_ptr(), n, k, nn, maxq)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().qeft_gptq_rows_pc(*args, st) if num is None else _lib.lib().qeft_gptq_rows_pc_mse(*args, num, st))
    torch.cuda.synchronize()
    assert _lib.last_variant() == ("gptq_rows_pc" if num is None else "gptq_rows_pc_mse_w4" if maxq == 15 else "gptq_rows_pc_mse_w3")
    assert torch.equal(bits_of(w.cpu()), bits_of(wi)) and torch.equal(bits_of(u.cpu()), bits_of(U))
    out = [t.cpu() for t in (q, err, s, z)]
    assert all(torch.isnan(t[n]).all() for t in out)
    return tuple(t[:n].contiguous() for t in out)


def assert_grid_and_identity(W0, U, outs, nn, maxq, what):
    q, err, s, z = outs
    assert s.shape == z.shape == (W0.shape[0], 1) and all(torch.isfinite(t).all() for t in outs) and s.min() >= 1e-8
    assert torch.equal(z, z.round()) and z.min() >= 0 and z.max() <= maxq
    codes = torch.round(q[:, :nn] / s + z)
    assert codes.min() >= 0 and codes.max() <= maxq and torch.equal(bits_of(s * (codes - z)), bits_of(q[:, :nn]))
    assert_identity(W0, q, err, U, nn, what)


@gpu
@pytest.mark.parametrize("N,K,r,bits", [(8, 256, 64, 4), (72, 384, 128, 4), (16, 640, 0, 4), (24, 256, 2, 4), (24, 384, 130, 3)])
def test_defining_identity_and_the_minmax_pair(N, K, r, bits):
    from qeft_amd.quant import minmax_params
    _, _, _, _, W0, U = layer(N, K, r)
    nn, maxq = K - r, 2 ** bits - 1
    full = run_rows_pc(W0, U, nn, maxq)
    want = minmax_params(W0[:, :nn].to(DEV), nn, bits)                     # as torch runs it on the device
    assert all(torch.equal(bits_of(a), bits_of(b.cpu())) for a, b in zip(full[2:], want))
    assert_grid_and_identity(W0, U, full, nn, maxq, f"per-channel, {N} x {K}, r = {r}, {bits} bits")
    if N == 72:                                                           # a rerun, and rows 16 .. 31 alone: the same bits
        for a, b, c in zip(full, run_rows_pc(W0, U, nn, maxq), run_rows_pc(W0[16:32], U, nn, maxq)):
            assert torch.equal(bits_of(a), bits_of(b)) and torch.equal(bits_of(a[16:32]), bits_of(c))


@gpu
@pytest.mark.parametrize("bits", [4, 3])
def test_the_sweep_has_the_bits_of_the_block_lines(bits):
    """U zeroed outside its diagonal blocks: every live block starts from W0's own columns and is swept with the row's pair."""
    _, _, _, _, W0, U = layer(24, 384, 130)
    Ub, maxq = torch.block_diag(*(U[i:i + 128, i:i + 128] for i in range(0, 384, 128))).contiguous(), 2 ** bits - 1
    q, err, s, z = run_rows_pc(W0, Ub, 254, maxq)
    for i1, i2 in ((0, 128), (128, 254)):
        Q1, E1, _ = R.block_lines(W0[:, i1:i2], Ub[i1:i2, i1:i2], s[:, 0], z[:, 0], maxq)
        assert torch.equal(bits_of(q[:, i1:i2]), bits_of(Q1)) and torch.equal(bits_of(err[:, i1:i2]), bits_of(E1))


@gpu
@pytest.mark.parametrize("N,K,r,bits", [(24, 384, 130, 4), (24, 384, 130, 3), (24, 640, 130, 4)])
def test_the_pair_is_the_whole_rows_search(N, K, r, bits, num=40):
    _, _, _, _, W0, U = layer(N, K, r)
    nn, maxq = K - r, 2 ** bits - 1
    outs = run_rows_pc(W0, U, nn, maxq, num=num)
    sg, zg = outs[2][:, 0], outs[3][:, 0]
    scores, pairs = candidates(W0[:, :nn], bits, num)
    best, first, inf = scores.min(0)[0], scores.argmin(0), torch.full_like(scores, float("inf"))
    member = (bits_of(pairs[:, 0]) == bits_of(sg)) & (bits_of(pairs[:, 1]) == bits_of(zg))
    mine, nxt = torch.where(member, scores, inf).min(0)[0], torch.where(scores > best, scores, inf).min(0)[0]
    clear = (best == 0) | (nxt - best >= G * best)
    ref = pairs[first, :, torch.arange(N)]
    same = (bits_of(ref[:, 0]) == bits_of(sg)) & (bits_of(ref[:, 1]) == bits_of(zg))
    print(f"{bits} bits, {nn} columns: largest score excess {(mine / best.clamp_min(1e-300) - 1).max().item():.3g}, rows left out of "
          f"(3) {(~clear).sum().item()} / {N}, rows with another pair than the reference's {(~same).sum().item()}")
    assert R.gamma(nn) + 1e-6 < G / 2 and member.any(0).all()                                                        # (1)
    assert (mine <= (1 + G) * best).all() and (~clear).sum().item() <= 0.1 * N and same[clear].all()                 # (2), (3)
    assert_grid_and_identity(W0, U, outs, nn, maxq, f"per-channel mse, {N} x {K}, r = {r}, {bits} bits")


@gpu
@pytest.mark.parametrize("N,K,r", [(40, 256, 128), (40, 256, 192)])
def test_one_block_has_the_bits_of_the_block_route(N, K, r):
    from qeft_amd.calibrate import gptq_reorder
    W, _, H, ids, _, U = layer(N, K, r)
    a, b = (gptq_reorder(W.to(DEV), H.float().to(DEV), ids.to(DEV), r, group_size=-1, hinv=U, loop=loop) for loop in ("rows", "blocks"))
    assert a.scale_group.shape == a.zero_group.shape == b.scale_group.shape == (N, 1) and a.group_size == -1
    assert torch.equal(a.weight[:, :K - r], b.weight[:, :K - r])
    assert torch.equal(bits_of(a.scale_group), bits_of(b.scale_group)) and torch.equal(bits_of(a.zero_group), bits_of(b.zero_group))


@gpu
@pytest.mark.parametrize("seed,shape", [R.CASES[1], R.CASES[4]])
def test_gptq_reorder_per_channel_end_to_end(seed, shape):
    """Against recon.py:504-554 restated in fp64 (the pair found once over the live columns, then the blocked loop) and RTN."""
    from qeft_amd.calibrate import HessianAccumulator, gptq_reorder, select_outliers
    W, X, hot = R.make_case(seed, **shape)
    K, r = W.shape[1], len(hot)
    H = HessianAccumulator(K, DEV).add_batch(X.to(DEV)).H
    _, ids = select_outliers(H, r)
    nn, idc = K - r, ids.cpu()
    Wp, Hp = W.float()[:, idc], H.cpu()[idc][:, idc]
    Wk, hinv = Wp.double().clone(), R.factor(Hp, torch.float64)[0]
    s, z = R.minmax(Wk[:, :nn], 15)
    Q64, Qr = Wk.clone(), Wk.clone()
    Qr[:, :nn] = s * (torch.clamp(torch.round(Wk[:, :nn] / s) + z, 0, 15) - z)
    for i1 in range(0, nn, 128):
        i2 = min(i1 + 128, nn)
        Q64[:, i1:i2], E1, _ = R.block_lines(Wk[:, i1:i2], hinv[i1:i2, i1:i2], s[:, 0], z[:, 0], 15)
        Wk[:, i2:] -= E1 @ hinv[i1:i2, i2:]
    Q64[:, nn:] = Wk[:, nn:]
    l64, l_rtn = R.proxy_loss(Wp, Q64, Hp), R.proxy_loss(Wp, Qr, Hp)
    res = gptq_reorder(W.to(DEV), H, ids, r, group_size=-1, factor="own", loop="rows")
    print(f"seed {seed}, per-channel rows: proxy loss {res.proxy_loss:.9g}, fp64 restatement {l64:.9g} (relative "
          f"{(res.proxy_loss - l64) / l64:+.3g}, margin {R.REL_MARGIN:.3g}), / per-channel RTN {res.proxy_loss / l_rtn:.3f}")
    assert res.scale_group.shape == (W.shape[0], 1) and res.weight.dtype == torch.float16
    assert res.proxy_loss <= (1 + R.REL_MARGIN) * l64 and res.proxy_loss < l_rtn


@gpu
def test_calibrate_linear_per_channel_through_the_packed_kernels(golden):
    from qeft_amd.calibrate import calibrate_linear
    W, X, (N, K) = golden["W"], golden["X"], golden["W"].shape
    lin = torch.nn.Linear(K, N, bias=False).half().to(DEV)
    lin.weight.data = W.to(DEV)
    (module, info), (host, _) = (calibrate_linear(lin, golden["H"].to(DEV), 64, "layers.0.self_attn.o_proj", group_size=-1, loop="rows",
                                                  pack=pack, factor="own") for pack in ("device", "host"))
    assert module.scales.shape == (1, N) and info.group_size == -1 and info.scale_group.shape == (N, 1)
    Qu = info.weight.cpu().double()[:, torch.argsort(info.ids.cpu())]
    for m in (1, 16):
        x = X.reshape(-1, K)[40:40 + m].contiguous()
        y, yq = module(x.to(DEV)).cpu().double(), x.double() @ Qu.T
        err = (y - yq).abs().max().item() / yq.abs().max().item()
        print(f"per-channel, m = {m}: module vs x Q^T {err:.3g}")
        assert y.shape == (m, N) and err < 1e-3
    a, b = module.state_dict(), host.state_dict()
    assert list(a) == list(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)


PACK = [(4, 32, 256, 0), (4, 32, 256, 64), (3, 32, 384, 128)]


def packed(bits, W, scale, zero, n_out, device, col_ids=None):
    from qeft_amd import _lib
    from qeft_amd.qlinear import QuantLinear
    m = QuantLinear(bits, W.shape[1], W.shape[0], False, torch.float16, n_out, -1, True, "q_proj")
    holder = types.SimpleNamespace(weight=types.SimpleNamespace(data=W.to(device)), bias=None)
    ids = torch.arange(W.shape[1] - n_out, W.shape[1], dtype=torch.int32)
    if device == "cpu":
        m.pack(holder, scale, zero, ids)
        return m
    to = lambda t: None if t is None else t.to(device)
    m.found = m.to(device).pack_device(holder, to(scale), to(zero), ids, col_ids=to(col_ids))
    assert _lib.last_variant() == ("quant_pack_pc_w4" if bits == 4 else "quant_pack_pc_w3") and m.scales.shape == (1, W.shape[0])
    return m


@gpu
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("bits,N,K,n_out", PACK)
def test_pack_find_mode_equals_minmax_and_the_host_pack(bits, N, K, n_out, gather):
    from qeft_amd.quant import minmax_params, quantize
    live = K - n_out
    W = (torch.randn(N, K, generator=torch.Generator().manual_seed(N + K + n_out)) * 0.02).half()
    W[0, :live], W[1, :live] = 0, W[1, :live].abs() + 0.001               # an all-zero and an all-positive row
    scale, zero = minmax_params(W[:, :live], live, bits)
    fq = W.clone()
    fq[:, :live] = quantize(W[:, :live].float(), scale, zero, 0, 2 ** bits - 1).half()
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K)) if gather else torch.arange(K)
    raw = torch.empty_like(W)
    raw[:, perm] = W                                                      # raw[:, perm[j]] is column j of the operand
    m = packed(bits, raw, None, None, n_out, DEV, col_ids=perm.to(torch.int32) if gather else None)
    assert all(f.shape == (N, 1) and torch.equal(bits_of(f.cpu()), bits_of(want)) for f, want in zip(m.found, (scale, zero)))
    assert_same_buffers(m, packed(bits, fq, scale, zero, n_out, "cpu"), n_out)


@gpu
@pytest.mark.parametrize("bits,N,K,n_out", PACK)
def test_pack_given_mode_with_a_gptq_result_equals_the_host_pack(bits, N, K, n_out):
    from qeft_amd.calibrate import gptq_reorder
    W, _, H, ids, _, U = layer(N, K, n_out)
    res = gptq_reorder(W.to(DEV), H.float().to(DEV), ids.to(DEV), n_out, bits=bits, group_size=-1, hinv=U, loop="rows")
    Q, s, z = res.weight.cpu(), res.scale_group.cpu(), res.zero_group.cpu()
    assert_same_buffers(packed(bits, Q, s, z, n_out, DEV), packed(bits, Q, s, z, n_out, "cpu"), n_out)


@gpu
@pytest.mark.parametrize("n_out", [0, 32])
def test_rtn_linear_per_channel_forward_against_fp64(n_out):
    """As test_gpu_quant_pack.test_rtn_linear_forward_against_fp64: m = 1 against x . Wfq^T in fp64, Wfq = q s16 + sz16."""
    from qeft_amd import rtn_linear
    N, K, g = 64, 256, torch.Generator().manual_seed(17 + n_out)
    lin = torch.nn.Linear(K, N, bias=False).half()
    lin.weight.data = (torch.randn(N, K, generator=g) * 0.02).half()
    H = torch.diag(torch.rand(K, generator=g) + 0.1)
    module, info = rtn_linear(lin.to(DEV), n_out, "q_proj", H=H.to(DEV), group_size=-1)
    ids, live, s, z = info.ids.cpu(), K - n_out, info.scale_group.cpu(), info.zero_group.cpu()
    assert info.group_size == -1 and s.shape == (N, 1) and module.scales.shape == (1, N)
    Wp = lin.weight.data.cpu()[:, ids].float()
    Wp[:, :live] = torch.clamp(torch.round(Wp[:, :live] / s) + z, 0, 15) * s.half().float() + (-(z * s)).half().float()
    x = torch.randn(1, K, generator=g).half()[:, ids]
    y, ref = module(x.to(DEV)).cpu().double(), x.double() @ Wp.double().t()
    print(f"rtn_linear per-channel, n_out = {n_out}: relative error {((y - ref).abs().max() / ref.abs().max()).item():.3g}")
    assert (y - ref).abs().max() < 1e-3 * ref.abs().max()


def test_refusals_without_a_gpu():
    """SHAPE (num among it), then NULL, then ALIGN -- no GROUP step; every call below has something wrong."""
    from qeft_amd import _lib, build, qeft_cuda
    from qeft_amd.calibrate import gptq_reorder, rtn_linear
    build.build(verbose=False)
    lib = _lib.lib()
    ERR_SHAPE, ERR_NULL, ERR_ALIGN, P = 2, 4, 6, 1 << 20
    def rows(w=P, h=2 * P, q=3 * P, e=4 * P, s=5 * P, z=6 * P, n=32, k=256, ld_w=256, ld_h=256, nn=192, maxq=15, num=None):
        args = (w, ld_w, h, ld_h, q, e, s, z, n, k, nn, maxq)
        return lib.qeft_gptq_rows_pc(*args, None) if num is None else lib.qeft_gptq_rows_pc_mse(*args, num, None)
    for num in (None, 40):
        for bad in (dict(n=0), dict(k=192, ld_w=192, ld_h=192, nn=128), dict(ld_w=252), dict(ld_h=262), dict(nn=0), dict(nn=191), dict(maxq=3)):
            assert rows(**bad, num=num) == ERR_SHAPE and rows(**bad, num=num, w=None, q=3 * P + 8) == ERR_SHAPE, bad
        assert all(rows(**{p: None}, num=num) == ERR_NULL for p in "whqesz") and rows(w=None, num=num, e=4 * P + 8) == ERR_NULL
        assert all(rows(**{p: v}, num=num) == ERR_ALIGN for p, v in dict(w=P + 8, h=P + 8, q=P + 8, e=P + 8, s=P + 2, z=P + 1).items())
    assert rows(num=0) == ERR_SHAPE and rows(num=41, w=None) == ERR_SHAPE
    def pack(w=P, ids=None, s=None, z=None, q=2 * P, sc=3 * P, sz=4 * P, so=None, zo=None, n=32, k=256, ld=256, n_out=0, bits=4):
        return lib.qeft_quant_pack_pc(w, ld, ids, s, z, q, sc, sz, so, zo, n, k, n_out, bits, None)
    for bad in (dict(bits=2), dict(n=24), dict(k=192, ld=192), dict(ld=248), dict(ld=260), dict(n_out=33), dict(n_out=256), dict(bits=3, n_out=32)):
        assert pack(**bad) == ERR_SHAPE and pack(**bad, w=None, q=2 * P + 8) == ERR_SHAPE, bad
    assert all(pack(**{p: None}) == ERR_NULL and pack(**{p: None}, so=P + 2) == ERR_NULL for p in ("w", "q", "sc", "sz"))
    assert pack(s=P) == ERR_NULL and pack(z=P) == ERR_NULL                # the given parameters come as a pair
    assert all(pack(**bad) == ERR_ALIGN for bad in (dict(w=P + 8), dict(q=P + 8), dict(sc=P + 1), dict(so=P + 2), dict(ids=P + 2, ld=260), dict(s=P, z=P + 2)))
    W, H, ids, lin = torch.zeros(16, 128), torch.eye(128), torch.arange(128), torch.nn.Linear(128, 16).half()
    for err, match, fn in ((ValueError, "GPU", lambda: gptq_reorder(W, H, ids, 0, group_size=-1)),      # no CPU path, no fallback
                           (ValueError, "GPU", lambda: gptq_reorder(W, H, ids, 0, group_size=-1, loop="rows", tuning="mse_fused")),
                           (RuntimeError, "GPU", lambda: qeft_cuda.quant_pack(W.half(), group_size=-1)),
                           (ValueError, "GPU", lambda: rtn_linear(lin, 0, "q_proj", group_size=-1)),
                           (ValueError, "128", lambda: gptq_reorder(W, H, ids, 0, group_size=64)),
                           (ValueError, "128", lambda: rtn_linear(lin, 0, "q_proj", group_size=64))):
        with pytest.raises(err, match=match):
            fn()
