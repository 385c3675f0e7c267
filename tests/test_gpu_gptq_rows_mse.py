"""Tests of the row-owned GPTQ loop with the MSE search inside the launch (qeft_gptq_rows_mse, csrc/calib_rows.hip;
tuning="mse_fused", loop="rows").  The oracle: test_gpu_mse_search.candidates, its three criteria and G = 1e-4,
a condition on the inputs (the score error is gamma(128) = 7.6e-6 for 128 terms in any order plus ~1e-6 of the hardware log2 / exp2,
below G / 2).  The CPU test holds refusals only: no call hands the launching entry a complete set of valid arguments."""
import pytest
import torch

import calib_ref as R
from test_gpu_gptq_rows import assert_identity, golden, layer, run_rows  # noqa: F401  (golden is a fixture)
from test_gpu_mse_search import G, bits_of, candidates

gpu = pytest.mark.gpu
DEV = "cuda:0"


def run_rows_mse(W0, U, nn, maxq, num=40, ld_w=None, ld_h=None):
    return run_rows(W0, U, nn, maxq, ld_w=ld_w, ld_h=ld_h, num=num)


def assert_the_pairs_are_the_searchs(W0, Ub, outs, groups, bits, num=40):
    """Criteria (1) to (3) of test_gpu_mse_search for every live group (i1, i2) of a run on a block-diagonal factor, the sweep of
    the block with the kernel's own pair bit for bit, and the last pair repeated in the groups after the last live one.  An exact
    tie for the minimum leaves a row in (3): `nxt` is the next DISTINCT score, and the reference's pair is the first candidate's."""
    q, err, s, z = outs
    N, maxq = W0.shape[0], 2 ** bits - 1
    for g, (i1, i2) in enumerate(groups):
        x, sg, zg = W0[:, i1:i2], s[:, g], z[:, g]
        scores, pairs = candidates(x, bits, num)
        best, first, inf = scores.min(0)[0], scores.argmin(0), torch.full_like(scores, float("inf"))
        member = (bits_of(pairs[:, 0]) == bits_of(sg)) & (bits_of(pairs[:, 1]) == bits_of(zg))
        mine, nxt = torch.where(member, scores, inf).min(0)[0], torch.where(scores > best, scores, inf).min(0)[0]
        clear = (best == 0) | (nxt - best >= G * best)
        ref = pairs[first, :, torch.arange(N)]
        same = (bits_of(ref[:, 0]) == bits_of(sg)) & (bits_of(ref[:, 1]) == bits_of(zg))
        excess = torch.where(best > 0, mine / best.clamp_min(1e-300) - 1, mine)
        print(f"{bits} bits, num {num}, group {g} ({i2 - i1} columns): largest score excess {excess.max().item():.3g}, rows left out "
              f"of (3) {(~clear).sum().item()} / {N}, rows with another pair than the reference's {(~same).sum().item()}")
        assert member.any(0).all() and torch.equal(zg, zg.round()) and zg.min() >= 0 and zg.max() <= maxq and sg.min() >= 1e-8   # (1)
        assert (mine <= (1 + G) * best).all() and (~clear).sum().item() <= 0.1 * N and same[clear].all()                        # (2), (3)
        Q1, E1, _ = R.block_lines(x, Ub[i1:i2, i1:i2], sg, zg, maxq)        # the sweep, with the kernel's own pair
        assert torch.equal(q[:, i1:i2], Q1) and torch.equal(err[:, i1:i2], E1)
    for g in range(len(groups), s.shape[1]):
        assert torch.equal(bits_of(s[:, g]), bits_of(s[:, len(groups) - 1])) and torch.equal(bits_of(z[:, g]), bits_of(z[:, len(groups) - 1]))


@gpu
@pytest.mark.parametrize("bits", [4, 3])
def test_the_pair_is_the_searchs_in_every_group(bits):
    """U zeroed outside its diagonal blocks: every tile starts from W0's own columns.  Full | 126 live + 2 outlier | outlier-only."""
    N, K, nn, maxq = 24, 384, 254, 2 ** bits - 1
    _, _, _, _, W0, U = layer(N, K, 130)
    Ub = torch.block_diag(*(U[i:i + 128, i:i + 128] for i in range(0, K, 128))).contiguous()
    assert_the_pairs_are_the_searchs(W0, Ub, run_rows_mse(W0, Ub, nn, maxq), [(0, 128), (128, nn)], bits)


@gpu
@pytest.mark.parametrize("N,K,r,bits", [(8, 256, 64, 4), (72, 384, 128, 4), (24, 256, 2, 4), (24, 384, 130, 3)])
def test_defining_identity(N, K, r, bits):
    _, _, _, _, W0, U = layer(N, K, r)
    nn, maxq, ng, ngl = K - r, 2 ** bits - 1, K // 128, -(-(K - r) // 128)
    q, err, s, z = full = run_rows_mse(W0, U, nn, maxq)
    assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in full) and s.min() >= 1e-8
    assert torch.equal(z, z.round()) and z.min() >= 0 and z.max() <= maxq
    assert all(torch.equal(s[:, j], s[:, ngl - 1]) and torch.equal(z[:, j], z[:, ngl - 1]) for j in range(ngl, ng))
    sf, zf = (torch.repeat_interleave(t, 128, 1)[:, :nn] for t in (s, z))
    codes = torch.round(q[:, :nn] / sf + zf)
    assert codes.min() >= 0 and codes.max() <= maxq and torch.equal(bits_of(sf * (codes - zf)), bits_of(q[:, :nn]))
    assert_identity(W0, q, err, U, nn, f"mse_fused, {N} x {K}, r = {r}, {bits} bits")
    if N == 72:                                                           # a rerun, and rows 16 .. 31 alone: the same bits
        again, part = run_rows_mse(W0, U, nn, maxq), run_rows_mse(W0[16:32], U, nn, maxq)
        for a, b, c in zip(full, again, part):
            assert torch.equal(bits_of(a), bits_of(b)) and torch.equal(bits_of(a[16:32]), bits_of(c))


@gpu
@pytest.mark.parametrize("seed,shape,bits", [(*R.CASES[4], 4), (*R.CASES_W3[1], 3)])
def test_gptq_reorder_mse_fused_end_to_end(seed, shape, bits):
    from qeft_amd.calibrate import HessianAccumulator, frob_norm_error, gptq_reorder, select_outliers
    W, X, hot = R.make_case(seed, **shape)
    K, r = W.shape[1], len(hot)
    H = HessianAccumulator(K, DEV).add_batch(X.to(DEV)).H
    _, ids = select_outliers(H, r, frob_norm=frob_norm_error(W.to(DEV), bits, 128, "mse_fused"))
    Wp, Hp = W.float()[:, ids.cpu()], H.cpu()[ids.cpu()][:, ids.cpu()]
    l_rtn = R.proxy_loss(Wp, R.rtn(Wp, K - r, bits=bits), Hp)
    res, ref = (gptq_reorder(W.to(DEV), H, ids, r, bits=bits, factor="own", loop=loop, tuning=tuning)
                for loop, tuning in (("rows", "mse_fused"), ("blocks", "mse")))
    print(f"seed {seed}, {bits} bits, mse_fused: proxy loss {res.proxy_loss:.9g}, / RTN {res.proxy_loss / l_rtn:.3f}, "
          f"/ loop='blocks' tuning='mse' {res.proxy_loss / ref.proxy_loss:.5f}")
    assert res.weight.dtype == torch.float16 and res.proxy_loss < 0.6 * l_rtn


@gpu
def test_calibrate_linear_mse_fused_through_the_packed_kernels(golden):
    from qeft_amd.calibrate import calibrate_linear
    W, X, (N, K) = golden["W"], golden["X"], golden["W"].shape
    lin = torch.nn.Linear(K, N, bias=False).half().to(DEV)
    lin.weight.data = W.to(DEV)
    module, info = calibrate_linear(lin, golden["H"].to(DEV), 64, "layers.0.self_attn.o_proj", loop="rows", tuning="mse_fused",
                                    pack="device", factor="own")
    x = X.reshape(-1, K)[40:41].contiguous()
    y, yq = module(x.to(DEV)).cpu().double(), x.double() @ info.weight.cpu().double()[:, torch.argsort(info.ids.cpu())].T
    err = (y - yq).abs().max().item() / yq.abs().max().item()
    print(f"mse_fused, m = 1: module vs x Q^T {err:.3g}")
    assert y.shape == (1, N) and err < 1e-3


def test_refusals_without_a_gpu():
    """SHAPE (num among it), then GROUP, then NULL, then ALIGN; every call below has something wrong."""
    from qeft_amd import _lib, build
    from qeft_amd.calibrate import calibrate_linear, gptq_reorder, rtn_linear
    build.build(verbose=False)
    lib = _lib.lib()
    ERR_SHAPE, ERR_GROUP, ERR_NULL, ERR_ALIGN, P = 2, 3, 4, 6, 1 << 20
    def call(w=P, h=2 * P, q=3 * P, e=4 * P, s=5 * P, z=6 * P, n=32, k=256, ld_w=256, ld_h=256, nn=192, maxq=15, g=128, num=40):
        return lib.qeft_gptq_rows_mse(w, ld_w, h, ld_h, q, e, s, z, n, k, nn, maxq, g, num, None)
    for bad in (dict(num=0), dict(num=41), dict(n=0), dict(k=192, ld_w=192, ld_h=192, nn=128), dict(ld_w=252), dict(ld_h=262),
                dict(nn=0), dict(nn=258), dict(nn=191), dict(maxq=3)):
        assert call(**bad) == ERR_SHAPE and call(**bad, w=None, g=64) == ERR_SHAPE, bad
    assert call(g=64) == ERR_GROUP and call(g=256, w=None) == ERR_GROUP and all(call(**{p: None}) == ERR_NULL for p in "whqesz")
    assert all(call(**bad) == ERR_ALIGN for bad in (dict(w=P + 8), dict(h=P + 8), dict(q=P + 8), dict(e=P + 8), dict(s=5 * P + 2), dict(z=6 * P + 1)))
    W, H, ids, lin = torch.zeros(16, 128), torch.eye(128), torch.arange(128), torch.nn.Linear(128, 16, bias=False).half()
    for match, fn in (("loop='rows'", lambda: gptq_reorder(W, H, ids, 0, tuning="mse_fused")),           # "blocks" is the default
                      ("GPU", lambda: gptq_reorder(W, H, ids, 0, tuning="mse_fused", loop="rows")),      # no CPU path, no fallback
                      ("GPU", lambda: calibrate_linear(lin, H, 0, "q_proj", tuning="mse_fused", loop="rows")),
                      ("min-max", lambda: rtn_linear(lin, 0, "q_proj", tuning="mse_fused"))):
        with pytest.raises(ValueError, match=match):
            fn()
