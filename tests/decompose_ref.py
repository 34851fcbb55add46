"""numpy restatement of the signature decomposition of include/mmmusig.h (mmm_decompose_search, mmm_signature_decompose; DESIGN.md section
4.16) and the seeded cases its tests share.  `search` takes every subset of a size at once through elementwise float64 operations -- each a
single IEEE rounding, in the order the header gives -- so the device's outputs are compared with it bit for bit.  It knows nothing of ranks,
prefixes or lanes: subsets come from itertools.combinations in lexicographic order."""
import itertools
import math

import numpy as np

PIVOT = 2.0 ** -26


def _solve(g, beta):
    """g [N, s, s], beta [N, s] -> (admissible [N], gain [N], w [N, s], ratio [N] = min_i d_i / g_ii) by the row steps of the header"""
    N, s = beta.shape
    l = np.zeros((N, s, s)); r = np.zeros((N, s)); y = np.zeros((N, s)); z = np.zeros((N, s)); w = np.zeros((N, s))
    ok = np.ones(N, dtype=bool); ratio = np.full(N, np.inf)
    with np.errstate(all="ignore"):
        for i in range(s):
            u = np.zeros((N, i + 1))
            for j in range(i):
                t = g[:, i, j].copy()
                for p in range(j):
                    t = t - u[:, p] * l[:, j, p]
                u[:, j] = t
                l[:, i, j] = t * r[:, j]
            d = g[:, i, i].copy()
            for p in range(i):
                d = d - u[:, p] * l[:, i, p]
            ok &= d > PIVOT * g[:, i, i]
            ratio = np.minimum(ratio, np.where(g[:, i, i] > 0, d / np.where(g[:, i, i] > 0, g[:, i, i], 1.0), -np.inf))
            r[:, i] = 1.0 / d
            t = beta[:, i].copy()
            for p in range(i):
                t = t - l[:, i, p] * y[:, p]
            y[:, i] = t
            z[:, i] = t * r[:, i]
        gain = y[:, 0] * z[:, 0]
        for i in range(1, s):
            gain = gain + y[:, i] * z[:, i]
        for i in range(s - 1, -1, -1):
            t = z[:, i].copy()
            for p in range(i + 1, s):
                t = t - l[:, p, i] * w[:, p]
            w[:, i] = t
        ok &= (w > 0).all(axis=1)
    return ok, gain, w, ratio


def evaluate(G, b, subset):
    """one subset (ascending rows) of one signature (b [C]) -> (admissible, gain, w [s])"""
    c = np.asarray(subset, dtype=np.int64)
    G = np.asarray(G, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    ok, gain, w, _ = _solve(G[np.ix_(c, c)][None], b[c][None])
    return bool(ok[0]), gain[0], w[0]


def search(G, b, ss, S, stats=None):
    """(subset [n, S, S], weight [n, S, S], gain [n, S], cosine [n, S]) of the header.  stats (a dict): 'ratio' <- the smallest d_i / g_ii
    over all admissible subsets met, 'sizes_found' <- [n, S] bool."""
    G = np.asarray(G, dtype=np.float64); b = np.asarray(b, dtype=np.float64); ss = np.asarray(ss, dtype=np.float64)
    C = G.shape[0]; n = b.shape[0]
    subset = np.full((n, S, S), -1, dtype=np.int32); weight = np.zeros((n, S, S)); gain = np.zeros((n, S)); cosine = np.zeros((n, S))
    worst = np.inf
    for s in range(1, min(S, C) + 1):
        combos = np.array(list(itertools.combinations(range(C), s)), dtype=np.int64)          # lexicographic
        g = G[combos[:, :, None], combos[:, None, :]]
        for i in range(n):
            if ss[i] == 0.0:
                continue
            ok, gn, w, ratio = _solve(g, b[i][combos])
            if not ok.any():
                continue
            worst = min(worst, float(ratio[ok].min()))
            k = int(np.argmax(np.where(ok, gn, -1.0)))                                     # the first maximum: the lexicographically smallest
            subset[i, s - 1, :s] = combos[k]; weight[i, s - 1, :s] = w[k]; gain[i, s - 1] = gn[k]
            cosine[i, s - 1] = np.sqrt(min(gn[k] / ss[i], 1.0))
    if stats is not None:
        stats["ratio"] = worst
        stats["sizes_found"] = subset[:, :, 0] >= 0
    return subset, weight, gain, cosine


def moments(sig, cat):
    """(G, b, ss) with numpy's sums: data for the search, not a statement about the device's rounding"""
    sig = np.asarray(sig, dtype=np.float64); cat = np.asarray(cat, dtype=np.float64)
    # (products first, then one sum per entry: symmetric, and equal rows give equal entries -- a BLAS product promises neither)
    return (cat[:, None, :] * cat[None, :, :]).sum(axis=-1), (sig[:, None, :] * cat[None, :, :]).sum(axis=-1), (sig * sig).sum(axis=1)


def moments_exact(sig, cat):
    """(G, b, ss) with every sum taken exactly (math.fsum over the singly rounded products): one more rounding per entry.  All terms are
    >= 0, so an entry is also its own sum of |terms|."""
    sig = np.asarray(sig, dtype=np.float64); cat = np.asarray(cat, dtype=np.float64)
    C, n = cat.shape[0], sig.shape[0]
    G = np.zeros((C, C)); b = np.zeros((n, C)); ss = np.zeros(n)
    for c in range(C):
        for e in range(c, C):
            G[c, e] = G[e, c] = math.fsum((cat[c] * cat[e]).tolist())
    for i in range(n):
        ss[i] = math.fsum((sig[i] * sig[i]).tolist())
        for c in range(C):
            b[i, c] = math.fsum((sig[i] * cat[c]).tolist())
    return G, b, ss


# ---- the seeded cases ------------------------------------------------------------------------------------------------------------------------
SEARCH_SHAPES = [(1, 1), (2, 3), (6, 6), (12, 6), (20, 4), (63, 2), (64, 3), (65, 3), (86, 3), (130, 2), (256, 2)]      # (C, S)
SEARCH_N = [1, 7, 70]
MOMENT_V = [1, 63, 64, 65, 96, 130]


def catalogue(rng, C, V, degenerate=True):
    """C unnormalised non-negative rows (scales 0.1 .. 100).  degenerate: row C - 2 is 2.5 x row 1 (a scaled duplicate), row C // 2 equals row
    0 (an exact duplicate) and row 3 is an exact blend of rows 4 and 5 -- each where C leaves room."""
    cat = (rng.dirichlet(np.full(V, 0.3), size=C) if V > 1 else rng.random((C, 1)) + 0.1) * 10.0 ** rng.uniform(-1, 2, size=(C, 1))
    if degenerate:
        if C >= 8:
            cat[3] = 0.25 * cat[4] + 0.75 * cat[5]
        if C >= 6:
            cat[C // 2] = cat[0]
        if C >= 4:
            cat[C - 2] = 2.5 * cat[1]
    return cat


def signatures(rng, cat, n):
    """n signatures over the catalogue, by i % 5: 0 a noisy planted mixture of 1-3 rows; 1 an exact one (its spare weights are rounding noise
    whose sign decides admissibility); 2 a noisy mixture of the LAST rows (the highest ranks); 3 exactly row 0 (which row C // 2 duplicates);
    4 a zero row (ss = 0)."""
    C, V = cat.shape
    sig = np.zeros((n, V))
    for i in range(n):
        kind = i % 5
        m = int(rng.integers(1, min(3, C) + 1))
        if kind == 4:
            continue
        if kind == 3:
            sig[i] = cat[0]
            continue
        rows = np.arange(C - m, C) if kind == 2 else np.sort(rng.choice(C, size=m, replace=False))
        sig[i] = rng.uniform(0.2, 1.0, size=m) @ cat[rows]
        if kind != 1:
            sig[i] *= rng.gamma(2500.0, 1.0 / 2500.0, size=V)          # 2 % noise
    return sig


def search_case(C, S, n):
    """(G, b, ss) of the seeded case (C, S, n), V = 40"""
    rng = np.random.default_rng(1000003 * C + 1009 * S + n)
    cat = catalogue(rng, C, 40)
    return moments(signatures(rng, cat, n), cat)
