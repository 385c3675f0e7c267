"""fp64 net under the fused lm_head + cross-entropy entry (csrc/lm_head_nll.hip, variant "lm_head_nll") and under the scoring
path built on it (qeft_amd/scoring.py: lm_head_nll, score, eval_nll).

The reference is fp64 from the kernel's own fp16 inputs (a float64 matmul), never another kernel's output.  With
mag_ij = sum_k |x_ik w_jk| (fp64), the bounds are derived, not measured:

  logit   fp16 x fp16 products are exact in fp32; a chain of K / 16 MFMA accumulation steps, each faithful to 2^-23 of a partial
          sum that never exceeds mag, gives E_ij = (K / 16 + 8) * 2^-23 * mag_ij (truncation allowed for).
  tgt     |tgt_logit - ref| <= E_i,target; an ignored target gives exactly 0.0.
  lse     |lse - ref| <= max_j E_ij + 2^-14: the constant covers the fp32 exp, the <= (128 + ceil(vocab / 128))-term sums and the log.
  argmax  an index whose fp64 logit is within E_i,argmax + E_i,best (<= 2 E) of the fp64 maximum; the exact lowest index in the
          constructed ties.

x is a view inside a wider NaN buffer (NaN rows before and after, NaN bands on both sides), the weight sits inside a NaN buffer,
outputs and workspace start as NaN between guard margins of one byte pattern that must come back intact.  Every test prints its
worst error / bound ratio ([lm_head_nll] ...)."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 64
FILL = 0xA5
NAN = float("nan")
F16, F32, F64, I32 = torch.float16, torch.float32, torch.float64, torch.int32
IGNORE = -100


def _L():
    from qeft_amd import _lib
    return _lib, _lib.lib()


class Guarded:
    """`n` elements of `dtype` between two margins of FILL bytes; the elements start as NaN (float) or as FILL bytes (int)."""

    def __init__(self, n, dtype):
        es = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((n + 2 * MARGIN) * es,), FILL, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = MARGIN * es, (MARGIN + n) * es
        self.t = self.raw[self.lo:self.hi].view(dtype)
        if dtype.is_floating_point:
            self.t.fill_(NAN)

    def margins_intact(self):
        return bool((self.raw[:self.lo] == FILL).all().item() and (self.raw[self.hi:] == FILL).all().item())


def _poisoned_x(x, pad=8, stride=None):
    """x [t, hidden] as a view of a NaN buffer: one NaN row before, two after, `pad` NaN elements left of every row, the rest of
    the stride right of it."""
    t, hidden = x.shape
    stride = stride or hidden + 2 * pad
    buf = torch.full((t + 3, stride), NAN, dtype=F16, device=DEV)
    view = buf[1:1 + t, pad:pad + hidden]
    view.copy_(x)
    return view


def _poisoned_w(w):
    vocab, hidden = w.shape
    buf = torch.full((vocab * hidden + 2 * MARGIN,), NAN, dtype=F16, device=DEV)
    view = buf[MARGIN:MARGIN + vocab * hidden].view(vocab, hidden)
    view.copy_(w)
    return view


def _launch(x, w, targets, want_tgt=True, want_argmax=True):
    """One call of the C entry on guarded outputs and a guarded, exactly sized workspace.  Returns (lse, tgt_logit, argmax)."""
    _lib, lib = _L()
    t, hidden = x.shape
    vocab = w.shape[0]
    assert x.stride(1) == 1 and w.is_contiguous()
    need = lib.qeft_lm_head_nll_workspace_bytes(t, vocab)
    assert need == 12 * t * ((vocab + 127) // 128)
    ws = Guarded(need // 4, F32)
    lse, tgt, am = Guarded(t, F32), Guarded(t, F32), Guarded(t, I32)
    tg = None if targets is None else targets.to(device=DEV, dtype=I32).contiguous()
    _lib.check(lib.qeft_lm_head_nll(x.data_ptr(), x.stride(0), w.data_ptr(), None if tg is None else tg.data_ptr(), lse.t.data_ptr(),
                                    tgt.t.data_ptr() if (tg is not None and want_tgt) else None,
                                    am.t.data_ptr() if want_argmax else None, ws.t.data_ptr(), need, t, hidden, vocab,
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _lib.last_variant() == "lm_head_nll"
    for name, g in (("workspace", ws), ("lse", lse), ("tgt_logit", tgt), ("argmax", am)):
        assert g.margins_intact(), f"{name}: a guard margin was written"
    if tg is None or not want_tgt:
        assert torch.isnan(tgt.t).all(), "tgt_logit was touched without targets"
    if not want_argmax:
        assert (am.raw == FILL).all(), "argmax was touched"
    return lse.t.clone(), tgt.t.clone(), am.t.clone()


def _ref64(x, w):
    """fp64 logits and mag [t, vocab] of fp16 operands, the vocabulary in pieces (a 32000 x 8192 head is 2 GB as float64)."""
    xd = x.to(F64)
    xa = xd.abs()
    t, vocab = x.shape[0], w.shape[0]
    logits, mag = torch.empty(t, vocab, dtype=F64, device=DEV), torch.empty(t, vocab, dtype=F64, device=DEV)
    for c0 in range(0, vocab, 4096):
        wd = w[c0:c0 + 4096].to(F64)
        logits[:, c0:c0 + 4096] = xd @ wd.t()
        mag[:, c0:c0 + 4096] = xa @ wd.abs_().t()
    return logits, mag


WORST = {}


def _check(tag, got, targets, logits, mag, hidden):
    """The three outputs of rows [0, t) against the fp64 reference rows; returns nothing, asserts the bounds, records the ratios."""
    lse, tgt, am = got
    t, vocab = lse.numel(), logits.shape[1]
    logits, mag = logits[:t], mag[:t]
    E = (hidden / 16 + 8) * 2.0 ** -23 * mag
    assert torch.isfinite(lse).all(), f"{tag}: non-finite lse"
    r_lse = ((lse.to(F64) - torch.logsumexp(logits, dim=1)).abs() / (E.max(dim=1).values + 2.0 ** -14)).max().item()
    best_v, best_i = logits.max(dim=1)
    assert ((am >= 0) & (am < vocab)).all(), f"{tag}: argmax outside the vocabulary"
    ami = am.long()[:, None]
    slack = E.gather(1, ami)[:, 0] + E.gather(1, best_i[:, None])[:, 0]
    gap = best_v - logits.gather(1, ami)[:, 0]
    r_am = (gap / slack.clamp_min(1e-300)).max().item() if bool((gap > 0).any()) else 0.0
    r_tgt = 0.0
    if targets is not None:
        tg = targets.to(DEV).long()
        ok = (tg >= 0) & (tg < vocab)
        assert torch.isfinite(tgt).all(), f"{tag}: non-finite tgt_logit"
        assert (tgt[~ok] == 0).all(), f"{tag}: an ignored target's tgt_logit is not 0.0"
        if bool(ok.any()):
            rows = ok.nonzero()[:, 0]
            want, e = logits[rows, tg[rows]], E[rows, tg[rows]]
            r_tgt = ((tgt[rows].to(F64) - want).abs() / e.clamp_min(1e-300)).max().item()
    key = tag.split(" ")[0]
    for k, v in (("lse", r_lse), ("tgt", r_tgt), ("argmax", r_am)):
        WORST[(key, k)] = max(WORST.get((key, k), 0.0), v)
    print(f"[lm_head_nll] {tag}: err / bound  lse {r_lse:.4f}  tgt {r_tgt:.4f}  argmax gap {r_am:.4f}")
    assert r_lse <= 1.0 and r_tgt <= 1.0 and r_am <= 1.0, f"{tag}: lse {r_lse:.3f}, tgt {r_tgt:.3f}, argmax {r_am:.3f} of the bound"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\n[lm_head_nll] {k[0]} {k[1]}: largest err / bound over all cases = {WORST[k]:.4f}", end="")


_OPERANDS = {}


def _operands(hidden, vocab, rows):
    """Random operands of one shape with their fp64 reference: made once, shared, never written.  x [rows, hidden] ~ N(0, 1),
    w ~ N(0, 0.02^2) inside a NaN buffer, targets with every kind of row."""
    key = (hidden, vocab)
    if key not in _OPERANDS or _OPERANDS[key][0].shape[0] < rows:
        g = torch.Generator(device=DEV).manual_seed(hidden * 7 + vocab)
        x = torch.randn(rows, hidden, generator=g, device=DEV).half()
        w = _poisoned_w((torch.randn(vocab, hidden, generator=g, device=DEV) * 0.02).half())
        targets = torch.randint(0, vocab, (rows,), generator=g, device=DEV).to(I32)
        special = torch.tensor([IGNORE, -1, vocab, vocab + 5, vocab - 1, 0], dtype=I32, device=DEV)
        every5 = torch.arange(0, rows, 5, device=DEV)
        targets[every5] = special[torch.arange(every5.numel(), device=DEV) % 6]        # ignored rows and both ends of the vocabulary
        logits, mag = _ref64(x, w)
        _OPERANDS[key] = (x, w, targets, logits, mag)
    return _OPERANDS[key]


SMALL = [(256, 512), (512, 9), (512, 127), (512, 129), (1024, 4097)]
CASES = [(h, v, t) for h, v in SMALL for t in (1, 7, 64, 65, 129, 200)] + \
        [(4096, 32000, t) for t in (1, 65, 200)] + [(5120, 32000, 7), (8192, 32000, 65)]
ROWS = {(4096, 32000): 200, (5120, 32000): 7, (8192, 32000): 65}


@pytest.mark.parametrize("hidden,vocab,t", CASES)
def test_parity_fp64_poisoned(hidden, vocab, t):
    x, w, targets, logits, mag = _operands(hidden, vocab, ROWS.get((hidden, vocab), 200))
    got = _launch(_poisoned_x(x[:t]), w, targets[:t])
    _check(f"parity hidden={hidden} vocab={vocab} t={t}", got, targets[:t], logits, mag, hidden)


def test_logits_are_not_rounded_to_fp16():
    """All-positive operands: mag = logit.  Logits of about 12, so the bound is 2^-15 * logit ~ 4e-4, a tenth of fp16's half-ulp
    there (2^-8): a rounding of a logit to fp16 anywhere on the path fails the tgt_logit bound."""
    hidden, vocab, t = 4096, 4097, 65
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.rand(t, hidden, generator=g, device=DEV).half()
    w = _poisoned_w((torch.rand(vocab, hidden, generator=g, device=DEV) * (12.0 / 1024)).half())
    targets = torch.randint(0, vocab, (t,), generator=g, device=DEV).to(I32)
    logits, mag = _ref64(x, w)
    assert 8 < logits.min().item() and logits.max().item() < 16
    bound = (hidden / 16 + 8) * 2.0 ** -23 * mag.max().item()
    assert bound < 2.0 ** -8 / 8, bound
    _check("no-fp16 hidden=4096 vocab=4097 t=65", _launch(_poisoned_x(x), w, targets), targets, logits, mag, hidden)


def test_targets_and_ties():
    hidden, vocab = 256, 512
    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn(8, hidden, generator=g, device=DEV).abs().half()              # all-positive rows: a constant weight row wins
    w0 = (torch.randn(vocab, hidden, generator=g, device=DEV) * 0.02).half()
    targets = torch.tensor([0, 127, 128, vocab - 1, IGNORE, -1, vocab, vocab + 5], dtype=I32)
    logits, mag = _ref64(x, w0)
    w = _poisoned_w(w0)
    xv = _poisoned_x(x)
    got = _launch(xv, w, targets)
    _check("targets hidden=256 vocab=512 t=8", got, targets, logits, mag, hidden)
    assert (got[1][4:] == 0).all() and (got[1][:4] != 0).all()
    # NULL targets with NULL tgt_logit, and a NULL argmax: lse (and argmax) as before, bit for bit
    no_t = _launch(xv, w, None)
    assert torch.equal(no_t[0].view(I32), got[0].view(I32)) and torch.equal(no_t[2], got[2])
    no_a = _launch(xv, w, targets, want_argmax=False)
    assert torch.equal(no_a[0].view(I32), got[0].view(I32)) and torch.equal(no_a[1].view(I32), got[1].view(I32))
    # duplicate weight rows that are every row's maximum: inside one tile (5, 133 sits in the next) and across a tile edge (127, 128)
    for lo, hi in ((5, 133), (127, 128)):
        wd = w0.clone()
        wd[lo] = 0.5
        wd[hi] = 0.5
        lg, mg = _ref64(x, wd)
        assert (lg.max(1).values == lg[:, lo]).all() and (lg[:, lo] == lg[:, hi]).all()
        got = _launch(xv, _poisoned_w(wd), targets)
        _check(f"ties({lo},{hi}) hidden=256 vocab=512 t=8", got, targets, lg, mg, hidden)
        assert (got[2] == lo).all(), (lo, hi, got[2].tolist())


def test_range():
    """A zero row: lse = log(vocab), argmax 0.  Rows whose logits are about +-3e4 (25600 .. 38400 in magnitude, 25 apart): a finite
    lse equal to the row maximum within the bound."""
    hidden, vocab = 256, 512
    x = torch.zeros(3, hidden, dtype=F16, device=DEV)
    x[1], x[2] = 100.0, -100.0
    j = torch.arange(vocab, device=DEV)
    col = (1.0 + j.double() / 1024) * torch.where(j % 2 == 0, 1.0, -1.0).double()
    w0 = col[:, None].expand(vocab, hidden).half().contiguous()
    logits, mag = _ref64(x, w0)
    assert 3.8e4 < logits[1:].max().item() < 3.9e4 and -3.9e4 < logits[1:].min().item() < -3.8e4
    got = _launch(_poisoned_x(x), _poisoned_w(w0), None)
    lse, _, am = got
    _check("range hidden=256 vocab=512 t=3", got, None, logits, mag, hidden)
    assert torch.isfinite(lse).all()
    assert abs(lse[0].item() - math.log(vocab)) <= 2.0 ** -14 and am[0].item() == 0
    E = (hidden / 16 + 8) * 2.0 ** -23 * mag.max(dim=1).values
    for r in (1, 2):
        assert abs(lse[r].item() - logits[r].max().item()) <= E[r].item() + 2.0 ** -14
        assert am[r].item() == logits[r].argmax().item()


@pytest.mark.parametrize("hidden,vocab", [(256, 512), (4096, 32000)])
def test_row_invariance_bit_for_bit(hidden, vocab):
    """A row's results do not depend on t, on the row's index in the launch (64- and 128-row tiles, every wave) or on x_stride."""
    x, w, targets, _, _ = _operands(hidden, vocab, 200)
    full = _launch(_poisoned_x(x), w, targets)
    bits = lambda o: [o[0].view(I32), o[1].view(I32), o[2]]      # noqa: E731
    for a, b in ((0, 64), (64, 65), (65, 200)):
        part = _launch(_poisoned_x(x[a:b]), w, targets[a:b])
        for f, p, name in zip(bits(full), bits(part), ("lse", "tgt_logit", "argmax")):
            assert torch.equal(f[a:b], p), f"rows [{a}, {b}) launched alone: {name} differs"
    other = _launch(_poisoned_x(x, pad=0, stride=3 * hidden), w, targets)
    for f, p, name in zip(bits(full), bits(other), ("lse", "tgt_logit", "argmax")):
        assert torch.equal(f, p), f"x_stride = 3 * hidden: {name} differs"
    print(f"[lm_head_nll] invariance hidden={hidden} vocab={vocab}: 3 sub-launches and a second stride, bit for bit")


def test_no_logits_in_memory():
    """lm_head_nll on hn [2048, 512], W [32000, 512]: the peak rises by less than 16 MB over the operands (the workspace is 6 MB; the
    fp16 logits alone would be 131 MB)."""
    from qeft_amd import scoring
    g = torch.Generator(device=DEV).manual_seed(13)
    hn = torch.randn(2048, 512, generator=g, device=DEV).half()
    w = (torch.randn(32000, 512, generator=g, device=DEV) * 0.02).half()
    targets = torch.randint(0, 32000, (2048,), generator=g, device=DEV)
    scoring._workspace.clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lse, tgt, am = scoring.lm_head_nll(hn, w, targets)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"[lm_head_nll] memory: peak rise {rise / 2 ** 20:.2f} MB at T = 2048, vocab = 32000")
    assert _L()[0].last_variant() == "lm_head_nll" and rise < 16 * 2 ** 20
    assert torch.isfinite(lse).all() and torch.isfinite(tgt).all() and lse.dtype == F32 and am.dtype == I32


# ---- end to end on the tiny model: score / eval_nll against prefill() + fp32 log-softmax
T_DOC = 48


@pytest.fixture(scope="module")
def tiny():
    from qeft_amd.llama import QuantLlama, prefill, tiny_shape
    model = QuantLlama(tiny_shape(), DEV, seed=6)
    tokens = torch.randint(0, model.shape.vocab, (T_DOC,), generator=torch.Generator().manual_seed(3)).to(DEV)
    logits = prefill(model, tokens)                                    # fp16 [T, vocab]: the parent's route
    hn = prefill(model, tokens, _head=False)
    _, mag = _ref64(hn, model.lm_head.weight)
    torch.cuda.synchronize()
    return model, tokens, logits, hn, mag


def _ulp16(v):
    return 2.0 ** (math.floor(math.log2(v)) - 10)


def _tol(model, logits, mag):
    """ulp16(max |logit|) for the fp16 rounding of the old route's logits, plus the kernel's bound on tgt_logit - lse."""
    E = (model.shape.hidden / 16 + 8) * 2.0 ** -23 * mag.max().item()
    return _ulp16(logits.float().abs().max().item()) + 2 * E + 2.0 ** -14


def test_score_matches_prefill_log_softmax(tiny):
    from qeft_amd import score
    model, tokens, logits, hn, mag = tiny
    assert hn.shape == (T_DOC, model.shape.hidden) and hn.dtype == F16
    sc = score(model, tokens)
    assert _L()[0].last_variant() == "lm_head_nll"
    lp_old = torch.log_softmax(logits.float(), dim=1)
    want = lp_old[torch.arange(T_DOC - 1), tokens[1:]]
    tol = _tol(model, logits, mag)
    err = (sc.logprob[:-1] - want).abs().max().item()
    err_lse = (sc.lse - torch.logsumexp(logits.float(), dim=1)).abs().max().item()
    print(f"[lm_head_nll] score vs prefill + log_softmax: max |d logprob| / tol = {err / tol:.4f}, |d lse| / tol = {err_lse / tol:.4f} (tol {tol:.3e})")
    assert sc.logprob.dtype == F32 and sc.lse.dtype == F32 and sc.argmax.dtype == I32 and sc.logprob.shape == (T_DOC,)
    assert err <= tol and err_lse <= tol and sc.logprob[-1].item() == 0.0
    top2 = logits.float().topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > tol
    assert bool(clear.any()) and torch.equal(sc.argmax[clear].long(), logits.float().argmax(1)[clear])
    # labels: -100 excludes a row, any other row is scored against its label
    labels = torch.cat([tokens[1:], tokens[:1]]).to(I32)
    labels[::3] = IGNORE
    sl = score(model, tokens, targets=labels)
    keep = labels >= 0
    assert (sl.logprob[~keep] == 0).all() and torch.equal(sl.lse.view(I32), sc.lse.view(I32))
    want_l = lp_old[torch.arange(T_DOC, device=DEV)[keep], labels[keep].long()]
    assert (sl.logprob[keep] - want_l).abs().max().item() <= tol


def _cache_state(eng, T):
    """(the raw cache rows [0, T) of every layer, their values as fp32, device position, host position)"""
    from qeft_amd.llama import kv8_decode_rows
    raw = [c[:, :T].clone() for c in eng.kc + eng.vc]
    if eng.ks is None:
        return raw, [r.float() for r in raw], int(eng.pos.item()), eng.host_pos
    scales = [s[:, :T].clone() for s in eng.ks + eng.vs]
    return raw + scales, [kv8_decode_rows(c, s).float() for c, s in zip(raw, scales)], int(eng.pos.item()), eng.host_pos


@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8"])
def test_score_on_an_engine_whole_chunked_continued(tiny, kv_dtype):
    """score(engine=e), score(engine=e, chunk=16) and score(tokens[:24]) + score(tokens[24:], start=24): each leaves the engine as
    prefill() with the same arguments does (bit for bit: the same launches up to the head), the three agree in logprob within twice
    the tolerance and in position; their cache rows agree within the project's bound between two routes of one pass (2e-2 of the
    largest entry, tests/test_gpu_prefill_attn.py).  fp8: chunked against continued only (both on the own e4m3 attention)."""
    from qeft_amd import score
    from qeft_amd.llama import DecodeEngine, prefill
    model, tokens, logits, hn, mag = tiny
    tol = _tol(model, logits, mag)

    def run(kind, fn):
        e = DecodeEngine(model, use_graph=False, kv_dtype=kv_dtype)
        if kind == "whole":
            out = [fn(model, tokens, e)]
        elif kind == "chunk":
            out = [fn(model, tokens, e, chunk=16)]
        else:
            out = [fn(model, tokens[:24], e), fn(model, tokens[24:], e, start=24)]
        torch.cuda.synchronize()
        return out, e

    kinds = ("whole", "chunk", "continued") if kv_dtype == "fp16" else ("chunk", "continued")
    lps, states = {}, {}
    for kind in kinds:
        out, e = run(kind, score)
        lp = torch.cat([o.logprob for o in out])
        if kind == "continued":
            assert out[0].logprob[-1].item() == 0.0                    # the first piece's last row has no next token of its own
            lp = lp.clone()
            lp[23] = NAN
        lps[kind], states[kind] = lp, _cache_state(e, T_DOC)
        _, e2 = run(kind, lambda *a, **k: prefill(*a, **k))
        s2 = _cache_state(e2, T_DOC)
        assert states[kind][2:] == s2[2:] == (T_DOC, T_DOC)
        assert all(torch.equal(a, b) for a, b in zip(states[kind][0], s2[0])), f"{kind}: caches differ from prefill()'s"
    first = kinds[0]
    # between two routes a cache entry may move by the project's route-to-route bound; on e4m3 a code may flip besides (2^-3)
    cache_bound = 2e-2 if kv_dtype == "fp16" else 2e-2 + 2.0 ** -3
    for kind in kinds[1:]:
        ok = ~torch.isnan(lps[kind])
        d = (lps[kind][ok] - lps[first][ok]).abs().max().item()
        dc = max(((a - b).abs().max() / a.abs().max()).item() for a, b in zip(states[kind][1], states[first][1]))
        print(f"[lm_head_nll] {kv_dtype} {kind} vs {first}: max |d logprob| / (2 tol) = {d / (2 * tol):.4f}, cache rel diff {dc:.3e}")
        assert states[kind][2:] == states[first][2:] and dc < cache_bound
        assert d <= 2 * tol, f"{kv_dtype} {kind} vs {first}: max |d logprob| {d:.3e} > 2 tol {2 * tol:.3e}"


def test_eval_nll_on_the_tiny_model(tiny):
    from qeft_amd import eval_nll
    from qeft_amd.llama import prefill
    model, tokens, _, _, mag = tiny
    seqlen, n = 32, T_DOC // 32
    out = eval_nll(model, tokens, seqlen=seqlen)
    nlls, worst = [], 0.0
    for i in range(n):
        win = tokens[i * seqlen:(i + 1) * seqlen]
        lg = prefill(model, win)
        worst = max(worst, lg.float().abs().max().item())
        nlls.append(torch.nn.CrossEntropyLoss()(lg[:-1].double(), win[1:]) * seqlen)
    want = (torch.stack(nlls).sum() / (n * seqlen)).item()
    tol = _ulp16(worst) + 2 * (model.shape.hidden / 16 + 8) * 2.0 ** -23 * mag.max().item() + 2.0 ** -14
    print(f"[lm_head_nll] eval_nll {out['nll']:.6f} vs reference formula on prefill logits {want:.6f} (tol {tol:.3e})")
    assert out["windows"] == n and out["tokens"] == n * seqlen and abs(out["nll"] - want) <= tol
    assert abs(out["ppl"] - math.exp(out["nll"])) < 1e-9
    chunked = eval_nll(model, tokens, seqlen=seqlen, chunk=16)
    assert abs(chunked["nll"] - out["nll"]) <= 2 * tol
    with pytest.raises(ValueError):
        eval_nll(model, tokens[:seqlen - 1], seqlen=seqlen)
    with pytest.raises(ValueError):
        eval_nll(model, tokens, seqlen=model.shape.max_seq + 1)


def test_torch_route_for_a_width_the_entry_refuses(monkeypatch):
    """hn [5, 96]: hidden % 64 != 0, so lm_head_nll computes the three tensors with torch in fp32 -- within the same bounds."""
    from qeft_amd import lm_head_nll
    _lib, lib = _L()
    hidden, vocab = 96, 300
    g = torch.Generator(device=DEV).manual_seed(14)
    hn = torch.randn(5, hidden, generator=g, device=DEV).half()
    w = (torch.randn(vocab, hidden, generator=g, device=DEV) * 0.05).half()
    targets = torch.tensor([0, 299, IGNORE, 128, vocab], dtype=I32)
    assert lib.qeft_lm_head_nll(1 << 20, hidden, 1 << 20, None, 1 << 20, None, None, 1 << 20, 1 << 30, 5, hidden, vocab, None) == 2
    hn2 = torch.randn(8, 256, generator=g, device=DEV).half()
    lm_head_nll(hn2, (torch.randn(64, 256, generator=g, device=DEV) * 0.05).half())
    assert _lib.last_variant() == "lm_head_nll"
    calls = []
    orig = lib.qeft_lm_head_nll
    monkeypatch.setattr(lib, "qeft_lm_head_nll", lambda *a: (calls.append(a), orig(*a))[1])
    got = lm_head_nll(hn, w, targets)
    assert calls == [], "the refused width was launched"
    logits, mag = _ref64(hn, w)
    _check("torch-route hidden=96 vocab=300 t=5", got, targets, logits, mag, hidden)
    assert got[0].dtype == F32 and got[1].dtype == F32 and got[2].dtype == I32
