"""An independent net under the calibration kernels (qeft_gptq_rows, qeft_gptq_rows_mse, qeft_hinv_factor and the routes of
gptq_reorder; DESIGN.md sections 4.20 - 4.25) at the clauses of their contracts that no other GPU test reaches: leading dimensions
other than k, the masked triangle of the factor, dead columns (diag(H) == 0), the nearest-point rounding of the row-owned sweep,
the search inside the launch with other `num` and a two-column block, and qeft_hinv_factor element by element.

Every reference runs on the CPU in fp32 / fp64 torch.  What is cached at module level stays on the CPU and no GPU tensor outlives
its test.  Shapes are the smallest at which each path exists (two live blocks of 128 + 126 with an outlier-only tile; a block of 2
live columns; three blocks of the factor)."""
import functools

import pytest
import torch

import calib_ref as R
from test_gpu_calibrate import grid_properties
from test_gpu_gptq_rows import IDENTITY, layer, run_rows
from test_gpu_gptq_rows_mse import assert_the_pairs_are_the_searchs, run_rows_mse
from test_gpu_hinv_factor import case
from test_gpu_mse_search import bits_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def leave_no_garbage():
    """A pytest.raises context keeps the raising frames -- and the GPU tensors in them -- alive in a reference cycle.  Collect once
    when the file is done: the peak-memory tests of later files compare readings that garbage freed mid-window would lower."""
    yield
    import gc
    gc.collect()


def run(mode, W0, U, nn, bits, **kw):
    """mode "minmax": qeft_gptq_rows; "mse": qeft_gptq_rows_mse with 40 ranges."""
    return run_rows(W0, U, nn, 2 ** bits - 1, **kw) if mode == "minmax" else run_rows_mse(W0, U, nn, 2 ** bits - 1, **kw)


# ------------------------------------------------------------------------------ A. the row-owned loop
@pytest.mark.parametrize("mode,bits,variant", [("minmax", 4, "gptq_rows_16"), ("mse", 4, "gptq_rows_mse_w4"), ("mse", 3, "gptq_rows_mse_w3")])
@pytest.mark.parametrize("N,K,r", [(24, 384, 130), (8, 256, 64)])
def test_strides_and_the_masked_triangle_leave_the_bits(N, K, r, mode, bits, variant):
    """A1.  ld_w = K + 12 (W0 a view into a NaN-filled [N + 2, K + 12] buffer), ld_h = K + 20 (U a view into a NaN-filled
    [K + 3, K + 20] buffer, NaN below the diagonal inside the view), each alone and both: the kernel promises one fixed order, so
    q, err, scale and zero must carry the bits of the contiguous run.  (What lies below the diagonal must not reach a result;
    whether by tri_store's mask or because gr_sweep reads the triangle's rows from the diagonal on is not observable.)  run_rows asserts that both input buffers come back
    unchanged, padding included, and that the NaN guard row behind every dense output is untouched."""
    from qeft_amd import _lib
    _, _, _, _, W0, U = layer(N, K, r)
    nn = K - r
    ref = run(mode, W0, U, nn, bits)
    assert _lib.last_variant() == variant
    assert all(torch.isfinite(t).all() for t in ref)
    for kw in (dict(ld_w=K + 12), dict(ld_h=K + 20), dict(ld_w=K + 12, ld_h=K + 20)):
        out = run(mode, W0, U, nn, bits, **kw)
        assert _lib.last_variant() == variant
        for name, a, b in zip(("q", "err", "scale", "zero"), ref, out):
            assert torch.equal(bits_of(a), bits_of(b)), (name, kw)


@pytest.mark.parametrize("N,K,r,bits,mode", [(*c, "minmax") for c in IDENTITY + [(16, 256, 126, 4)]] +
                         [(*c, "mse") for c in [(8, 256, 64, 4), (72, 384, 128, 4), (24, 256, 2, 4), (24, 384, 130, 3), (16, 256, 126, 4)]])
def test_the_sweep_rounds_to_the_nearest_grid_point(N, K, r, bits, mode):
    """A2.  assert_identity checks the feedback, which holds for any q on the grid; this checks q itself.  With d = U[i][i], w the
    value step i saw, (s, z) the column's pair and u = 2^-24, the pinned lines are  x = fl(w / s);  c = clamp(rint(x) + z);
    q = fl(s (c - z));  e = fl(fl(w - q) / d).  Where c is strictly inside 0..maxq nothing clamps and
      |w - s (c - z)| <= s |x - rint(x)| + s |w / s - x| <= s / 2 + u |w|,   |w| <= |q| + s / 2 + ..,
    q rounds s (c - z) once (u |q|), w - q rounds once, the quotient once, and the product e d taken back in fp64 from the fp32
    e and d at most once more: (w - q)(1 + u)^3.  Together
      |e d| <= B = (s / 2 + 2u (|q| + s)) (1 + 4u),
    derived, not measured.  On code 0 the value may lie any distance BELOW the grid's end (w - q <= B), on code maxq any
    distance above (w - q >= -B).  A floor or a truncation in place of rint doubles the inner error and fails here while
    assert_identity still passes.  At most 10 % of the live elements may sit on an end code (the fp32 restatement on the CPU
    gives 2.2 - 4.2 % with min-max pairs and 3.2 - 8.0 % with the search's winning pairs on these shapes)."""
    _, _, _, _, W0, U = layer(N, K, r)
    nn, maxq, u = K - r, 2 ** bits - 1, R.U
    q, err, s, z = run(mode, W0, U, nn, bits)
    sf, zf = (torch.repeat_interleave(t, 128, 1)[:, :nn] for t in (s, z))
    codes = torch.round(q[:, :nn] / sf + zf)
    ed = err.double() * torch.diag(U).double()[:nn]
    B = (sf.double() / 2 + 2 * u * (q[:, :nn].double().abs() + sf.double())) * (1 + 4 * u)
    low, high = codes == 0, codes == maxq
    inner = ~low & ~high
    end = (low | high).float().mean().item()
    top = lambda t: t.max().item() if t.numel() else 0.0
    print(f"{mode}, {N} x {K}, r = {r}, {bits} bits: largest |e d| / B inside the grid {top((ed.abs() / B)[inner]):.4f}, "
          f"at the ends {max(top((ed / B)[low]), top((-ed / B)[high])):.4f}; {100 * end:.1f} % on an end code")
    assert codes.min() >= 0 and codes.max() <= maxq and end <= 0.1
    assert (ed.abs() <= B)[inner].all() and (ed <= B)[low].all() and (ed >= -B)[high].all()


@functools.lru_cache(maxsize=None)
def degenerate(N, K, r):
    """The layer's W0 with five rows overwritten -- all zero, all positive, all negative, constant, one 0.5 per block among the
    0.02-scale values -- and its factor zeroed outside the diagonal blocks, so that every tile starts from W0's own columns."""
    _, _, _, _, W0, U = layer(N, K, r)
    W0 = W0.clone()
    W0[0] = 0
    W0[1], W0[2] = W0[1].abs(), -W0[2].abs()
    W0[3] = W0[3, 0]
    W0[4, 1::128] = 0.5                                                    # columns 1, 129, ..: inside the 2-column block too
    return W0, torch.block_diag(*(U[i:i + 128, i:i + 128] for i in range(0, K, 128))).contiguous()


@pytest.mark.parametrize("num", [1, 7])
@pytest.mark.parametrize("bits", [4, 3])
@pytest.mark.parametrize("N,K,r", [(24, 384, 130), (24, 256, 126)])
def test_the_search_with_other_num_a_short_block_and_degenerate_rows(N, K, r, bits, num):
    """A3.  (24, 256, 126): the second block has 2 live columns, so 15 of a row's 16 lanes carry padding zeros alone into the
    reduce-scatter.  With num = 1 there are only 2^bits candidates and exact ties for the minimum are likely: the first in the
    reference's order is the winner on both sides.  On the CPU the reference leaves no row of these cases out of (3)."""
    W0, Ub = degenerate(N, K, r)
    nn = K - r
    outs = q, err, s, z = run_rows_mse(W0, Ub, nn, 2 ** bits - 1, num=num)
    assert all(torch.isfinite(t).all() for t in outs)
    assert_the_pairs_are_the_searchs(W0, Ub, outs, [(0, 128), (128, nn)], bits, num)
    assert (q[0] == 0).all() and (err[0] == 0).all() and (s[0] > 0).all() and torch.isfinite(s[0]).all()


# ------------------------------------------------------------------------------ B. qeft_hinv_factor
def factor_raw(Hd, ld=None):
    """The C entry on a in a [K, ld] buffer (NaN padding) and u at the head of a NaN-filled buffer of K * ld floats.  Returns
    (the first K * K floats of u as [K, K], what lies behind them, the status, a's padding afterwards), on the CPU."""
    from qeft_amd import _lib
    K = Hd.shape[0]
    ld = ld or K
    a = torch.full((K, ld), NAN, device=DEV)
    a[:, :K] = Hd.to(DEV)
    u = torch.full((K * ld + 4,), NAN, device=DEV)
    info = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().qeft_hinv_factor(a.data_ptr(), ld, u.data_ptr(), info.data_ptr(), K, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _lib.last_variant() == "hinv_factor_b128"
    u = u.cpu()
    return u[:K * K].view(K, K), u[K * K:], info.item(), a.cpu()[:, K:]


@pytest.mark.parametrize("K", [256, 384])
def test_the_factor_with_a_leading_dimension(K):
    """B1.  ld = K + 12 is a's leading dimension; u is dense [K][K] by the contract (calib_factor.h: only A carries ld), so the
    result must be the ld == K bits in the first K * K floats of u's buffer, with the 12 K floats behind them -- where a kernel
    that strode u by ld would write -- still NaN, as a's padding is."""
    Hd = case(K)[0]
    ref, tail0, info0, _ = factor_raw(Hd)
    u, tail, info, pad = factor_raw(Hd, K + 12)
    assert info0 == 0 and info == 0 and torch.isfinite(ref).all()
    assert torch.equal(bits_of(u), bits_of(ref))
    assert pad.shape == (K, 12) and torch.isnan(pad).all() and torch.isnan(tail).all() and torch.isnan(tail0).all()


@functools.lru_cache(maxsize=None)
def spd(K, seed):
    """test_gpu_hinv_factor.case's recipe with a seed of its own."""
    _, X, _ = R.make_case(seed, N=8, K=K, r=K // 4, S=2, T=K // 2 + 40)
    H = R.hessian64(X).float()
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(seed))
    Hd = H[perm][:, perm].contiguous()
    Hd[range(K), range(K)] += 0.01 * torch.mean(torch.diag(Hd))
    return Hd


def test_a_block_diagonal_matrix_gives_the_blocks_own_factors():
    """B2.  Hd = block_diag(A0, A1, A2): every panel V[i][j] = A[i][j] D_j^T is a sum of products with exact zeros, so every
    trailing update adds -0 or +0 to A[i][l] (its bits stay) and every T[i][l], hence every U[j][l != j], is a zero.  The reduced
    diagonal block the diag kernel sees is then Ai itself and the kernel is the one that factors Ai alone: the same bits.  Exact
    on reading calib_factor.hip (alpha * acc + *c with acc == 0; no value-dependent path); a block stored, read or accumulated
    in the wrong place breaks it."""
    from qeft_amd import hinv_factor
    blocks = [spd(128, s) for s in (301, 302, 303)]
    u, _, info, _ = factor_raw(torch.block_diag(*blocks).contiguous())   # into a NaN-filled u: every element is written
    assert info == 0
    own =[hinv_factor(Ai.to(DEV)).cpu() for Ai in blocks]
    assert not any(torch.equal(own[i], own[j]) for i, j in ((0, 1), (0, 2), (1, 2)))                      # the blocks do differ
    for i in range(3):
        for j in range(3):
            got = u[128 * i:128 * i + 128, 128 * j:128 * j + 128]
            if i == j:
                assert torch.equal(bits_of(got), bits_of(own[i])), i
            else:
                assert torch.equal(got, torch.zeros(128, 128)), (i, j)


@functools.lru_cache(maxsize=None)
def dead_matrix():
    """(Hd fp32 [256, 256], the dead positions): a make_case Hessian with three channels of X zeroed, under a permutation that
    puts them first, in the middle and last, prepared as gptq_reorder does (1 on the dead diagonal, then the damping)."""
    K = 256
    _, X, hot = R.make_case(77, N=8, K=K, r=64, S=2, T=200, dead=(3, 90, 150))
    H = R.hessian64(X).float()
    gone = torch.nonzero(torch.diag(H) == 0)[:, 0]
    assert len(gone) == 3
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(7))
    perm = perm[~torch.isin(perm, gone)]
    perm = torch.cat([gone[:1], perm[:130], gone[1:2], perm[130:], gone[2:]])
    Hd = H[perm][:, perm].contiguous()
    dead = torch.diag(Hd) == 0
    assert torch.nonzero(dead)[:, 0].tolist() == [0, 131, 255]
    Hd[dead, dead] = 1
    Hd[range(K), range(K)] += 0.01 * torch.mean(torch.diag(Hd))
    return Hd, [0, 131, 255]


def ulps(a, b):
    """|a - b| in units of the last place of the fp32 b."""
    b32 = torch.tensor(b, dtype=torch.float32)
    return abs(a - b) / (torch.nextafter(b32, b32 * 2) - b32).item()


def test_the_factor_with_dead_columns():
    """B3.  A dead column is a unit row and column of Hd (1 + damping on the diagonal, exact zeros off it).  The exact factor has
    1 / sqrt(Hd[c][c]) there and zeros in the rest of row and column c; in the kernel every product that could reach them has an
    exact zero factor, so the zeros must be exact and the diagonal entry is one fp32 sqrt and one division away (4 ulp)."""
    from qeft_amd import hinv_factor
    Hd, dead = dead_matrix()
    ref = torch.linalg.cholesky(torch.linalg.inv(Hd.double()), upper=True)
    u = hinv_factor(Hd.to(DEV)).cpu()
    for c in dead:
        off = torch.arange(256) != c
        assert (ref[c][off] == 0).all() and (ref[:, c][off] == 0).all()                                   # the oracle has them too
        assert (u[c][off] == 0).all() and (u[:, c][off] == 0).all(), c
        want = 1 / Hd[c, c].double().sqrt().item()
        print(f"dead column {c}: U[c][c] {u[c, c].item():.9g}, 1 / sqrt(Hd[c][c]) {want:.9g}, {ulps(u[c, c].item(), want):.2f} ulp")
        assert ulps(u[c, c].item(), want) <= 4


def identity_error(u, Hd):
    """max |U Hd U^T - I| in fp64 and its position: the defining identity of Hd^-1 = U^T U, element by element."""
    E = (u.double() @ Hd.double() @ u.double().T - torch.eye(Hd.shape[0], dtype=torch.float64)).abs()
    i = E.argmax().item()
    return E.max().item(), divmod(i, Hd.shape[0])


@pytest.mark.parametrize("K", [128, 256, 384, 1152, "dead"])
def test_the_factor_element_by_element(K):
    """B4.  A largest-entry measure cannot average a wrong element away as the Frobenius one of test_parity_with_the_fp64_factor
    can.  The reference measure is that of torch's three fp32 calls on the same device and input; the factor 2 is the one the
    project already grants the own route over them."""
    from qeft_amd import hinv_factor
    Hd = dead_matrix()[0] if K == "dead" else case(K)[0]
    g = Hd.to(DEV)
    own = hinv_factor(g).cpu()
    three = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(g)), upper=True).cpu()
    (e_own, (i, j)), (e_torch, _) = identity_error(own, Hd), identity_error(three, Hd)
    print(f"K = {K}: max |U Hd U^T - I|: own {e_own:.3g} at ({i}, {j}), block ({i // 128}, {j // 128}); three torch calls "
          f"{e_torch:.3g} (ratio {e_own / e_torch:.3f})")
    assert e_own <= 2 * e_torch


@pytest.mark.parametrize("c", [383, 256, 255, 77, 0])
def test_the_status_names_the_column(c):
    """B5.  The sweep runs from the bottom-right corner, so the pivot of column c depends on rows and columns >= c alone and no
    column the sweep reaches earlier sees Hd[c][c].  With Hd[c][c] < 2 mean(diag) (asserted: the columns are not scaled channels)
    the entry goes negative, the pivot is that entry minus a sum of squares, and exactly column c fails: info == c + 1.  Bottom
    and top of the last block (the first the sweep takes), bottom of the middle block, an interior column and the top of block 0.
    A NaN and a +inf on the diagonal fail the same test `p > 0 && p <= FLT_MAX` at the same column.  The failing path writes
    `info` and skips nothing: every address is a function of the geometry alone, the non-finite values only flow through
    arithmetic, so these are a status and cannot fault."""
    Hd = case(384)[0]
    mean = torch.mean(torch.diag(Hd))
    assert Hd[c, c] < 2 * mean
    for name, value in (("negative", Hd[c, c] - 2 * mean), ("NaN", NAN), ("+inf", float("inf"))):
        bad = Hd.clone()
        bad[c, c] = value
        info = factor_raw(bad)[2]
        print(f"column {c}, {name}: info = {info}")
        assert info == c + 1, name
    from qeft_amd import hinv_factor
    with pytest.raises(torch.linalg.LinAlgError, match=f"column {c} ") as e:
        hinv_factor(bad.to(DEV))
    assert e.value.info == c + 1


# ------------------------------------------------------------------------------ C. dead columns end to end
ROUTES = [("blocks", "minmax"), ("blocks", "mse"), ("rows", "minmax"), ("rows", "mse_fused")]
# (seed, make_case keywords, bits, dead positions in ids order): first block | a block boundary | the end of the live columns
DEAD = [(21, dict(N=72, K=384, r=128), 4, (5, 127, 255)), (22, dict(N=24, K=384, r=130), 3, (5, 128, 253))]


def dead_layer(seed, shape, bits, dead):
    """(W, X, H on the GPU, ids on the GPU, the dead channels, their positions in ids).  H from HessianAccumulator: the dead rows
    and columns of it are exact zeros, and select_outliers keeps every dead channel out of the fp16 columns."""
    from qeft_amd.calibrate import HessianAccumulator, frob_norm_error, select_outliers
    W, X, hot = R.make_case(seed, **shape, dead=dead)
    K = W.shape[1]
    ch = R.dense_ids(hot, K)[list(dead)]
    assert (X[..., ch] == 0).all() and not torch.isin(ch, hot).any()
    acc = HessianAccumulator(K, DEV)
    for j in range(X.shape[0]):
        acc.add_batch(X[j].to(DEV))
    H = acc.H
    Hc = H.cpu()
    assert (torch.diag(Hc)[ch] == 0).all() and (Hc[ch] == 0).all() and (Hc[:, ch] == 0).all()
    assert (torch.diag(Hc) == 0).sum().item() == len(dead)
    out_ids, ids = select_outliers(H, len(hot), frob_norm=frob_norm_error(W.to(DEV), bits, 128, "minmax"))
    assert not torch.isin(out_ids.cpu().long(), ch).any()
    pos = torch.nonzero(torch.isin(ids.cpu(), ch))[:, 0]
    return W, X, H, ids, ch, pos


@pytest.mark.parametrize("seed,shape,bits,dead", DEAD)
def test_dead_columns_on_every_route(seed, shape, bits, dead):
    """C.  Three non-outlier channels never fire.  On every route and with both factors: the grid properties, exact zeros in the
    dead columns, the proxy loss under 0.6 x RTN, and on the min-max routes within REL_MARGIN of calib_ref.gptq_reorder in fp64
    (which zeroes the column and puts 1 on the diagonal as the reference does)."""
    from qeft_amd.calibrate import gptq_reorder
    W, X, H, ids, ch, pos = dead_layer(seed, shape, bits, dead)
    (N, K), r = W.shape, shape["r"]
    nn = K - r
    assert pos.tolist() == list(dead) and pos.max() < nn
    idc = ids.cpu()
    Wp, Hp = W.float()[:, idc], H.cpu()[idc][:, idc]
    l64 = R.proxy_loss(Wp, R.gptq_reorder(Wp, Hp, nn, torch.float64, bits=bits)[0], Hp)
    l_rtn = R.proxy_loss(Wp, R.rtn(Wp, nn, bits=bits), Hp)
    print(f"seed {seed}, {bits} bits, dead at {list(dead)}: fp64 restatement {l64:.9g} = {l64 / l_rtn:.3f} x RTN")
    for factor in ("torch", "own"):
        for loop, tuning in ROUTES:
            res = gptq_reorder(W.to(DEV), H, ids, r, bits=bits, factor=factor, loop=loop, tuning=tuning)
            print(f"  factor {factor:5s} loop {loop:6s} tuning {tuning:9s}: proxy loss {res.proxy_loss:.9g} (relative to fp64 "
                  f"{(res.proxy_loss - l64) / l64:+.3g}), / RTN {res.proxy_loss / l_rtn:.3f}")
            grid_properties(res, N, K, r, 2 ** bits - 1)
            assert (res.weight[:, pos.to(DEV)] == 0).all(), (factor, loop, tuning)
            assert res.proxy_loss < 0.6 * l_rtn, (factor, loop, tuning)
            if tuning == "minmax":
                assert res.proxy_loss <= (1 + R.REL_MARGIN) * l64, (factor, loop)


def test_calibrate_linear_with_dead_input_channels():
    """The first layer through loop="rows", pack="device", factor="own", as an o_proj (the module gathers its own input).  The
    device pack takes multiples of 16 rows, so the layer's first 64 rows (GPTQ's rows are independent).  A dead input channel may
    carry any finite x: its column of Q is zero, and the packed column's dequantised value is the fp16 rounding of s z - s z."""
    from qeft_amd.calibrate import calibrate_linear
    seed, shape, bits, dead = DEAD[0]
    W, X, H, _, ch, _ = dead_layer(seed, shape, bits, dead)
    W, K, r = W[:64].contiguous(), shape["K"], shape["r"]
    lin = torch.nn.Linear(K, 64, bias=False).half().to(DEV)
    lin.weight.data = W.to(DEV)
    module, info = calibrate_linear(lin, H, r, "layers.0.self_attn.o_proj", bits=bits, loop="rows", pack="device", factor="own")
    assert not torch.isin(info.out_ids.cpu().long(), ch).any()
    Qu = info.weight.cpu().double()[:, torch.argsort(info.ids.cpu())]
    assert (Qu[:, ch] == 0).all()
    for m in (1, 16):
        x = X.reshape(-1, K)[40:40 + m].clone()
        x[:, ch] = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float16)
        y, yq = module(x.to(DEV)).cpu().double(), x.double() @ Qu.T
        err = (y - yq).abs().max().item() / yq.abs().max().item()
        print(f"dead channels, m = {m}: module vs x Q^T {err:.3g}")
        assert y.shape == (m, 64) and err < 1e-3
