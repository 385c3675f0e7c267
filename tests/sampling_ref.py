"""Host references of sampled decoding (qeft_amd/sampling.py, csrc/decode_sample.hip): Philox4x32-10 in numpy and the filter of
temperature / top-k / top-p in fp64, written from the semantics, not from the kernel."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Random123 Philox4x32-10 of counter words ctr[4] under key words key[2] (uint32 arrays broadcast together)."""
    c = [np.asarray(x, dtype=np.uint64) for x in ctr]
    k0, k1 = np.asarray(key[0], dtype=np.uint64), np.asarray(key[1], dtype=np.uint64)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(W0)) & np.uint64(MASK), (k1 + np.uint64(W1)) & np.uint64(MASK)
    return [x.astype(np.uint32) for x in c]


def draw_u(seed, positions):
    """u = x0 / 2^32 of counter (p, 0, 0, 0), key (seed lo, seed hi), and x0 itself."""
    p = np.asarray(positions, dtype=np.uint64)
    z = np.zeros_like(p)
    x0 = philox4x32_10([p, z, z, z], [seed & MASK, seed >> 32])[0]
    return x0.astype(np.float64) / 2.0 ** 32, x0


def filter_probs(logits, temperature, top_k, top_p):
    """fp64 reference: (kept bool [V], probabilities [V] over the kept set, margin [V]).  margin[j] = |W(> l_j) - p Z| / Z for
    the top-p decision of each top-k survivor (inf where top-p is off or the token was cut by top-k).  temperature 0: the argmax
    (lowest index; NaN never; no value above -inf -> 0) alone."""
    l = np.asarray(logits, dtype=np.float64)
    V = l.size
    ok = ~np.isnan(l)
    margin = np.full(V, np.inf)
    if temperature == 0 or not ok.any():
        vals = np.where(ok, l, -np.inf)
        a = int(np.argmax(vals)) if (vals > -np.inf).any() else 0
        kept = np.zeros(V, bool)
        kept[a] = True
        return kept, kept.astype(np.float64), margin
    lmax = l[ok].max()
    with np.errstate(invalid="ignore", over="ignore"):
        # the exponent as the semantics compute it: fp32 (l - max) / T (exact differences of fp16 values, one fp32 division)
        q = (np.float32(1) * (l - lmax).astype(np.float32) / np.float32(temperature)).astype(np.float64)
        w = np.where(l == lmax, 1.0, np.exp(q))
    w = np.where(ok, w, 0.0)
    surv = ok.copy()
    if 0 < top_k < V and ok.sum() > top_k:
        kth = np.sort(l[ok])[::-1][top_k - 1]
        surv &= l >= kth
    kept = surv.copy()
    if top_p < 1:
        idx = np.nonzero(surv)[0]
        Z = w[idx].sum()
        uniq, inv = np.unique(l[idx], return_inverse=True)             # (-0 and +0 are one value)
        per = np.bincount(inv, weights=w[idx], minlength=uniq.size)
        above = (np.cumsum(per[::-1])[::-1] - per)[inv]                   # weight of strictly greater survivors
        kept[idx] = above < top_p * Z
        margin[idx] = np.abs(above - top_p * Z) / Z
        if not kept.any():
            kept = surv & (l == lmax)
    pr = np.where(kept, w, 0.0)
    return kept, pr / pr.sum(), margin


def cdf_interval(probs, token):
    """[lo, hi) of `token` in the inclusive CDF of probs in index order."""
    c = np.cumsum(probs)
    hi = c[token]
    return hi - probs[token], hi
