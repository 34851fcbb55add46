"""numpy restatement of mmm_cluster_samples (include/mmmusig.h) and the cases its tests share.

`cluster` follows the header literally in float64.  Wherever the header gives a sum an order, the sum is an explicit Python loop from 0.0 (the
distance over p, cum over the members, a stripe's members in ascending d, the 16 stripe sums); the vector operations inside a loop step act
on independent elements.  The pair counts and PAC are integers.  Only +, -, x, /, comparisons and integers decide every output, so a device
that keeps the same order gives the same bits.  Besides the outputs it returns the final centres and which branches of the definition every
pair took.  `upgma` is the average linkage written from its definition (the mean distance between two groups, recomputed from the original
matrix at every step): it shares nothing with the Lance-Williams update of the package."""
import functools
from collections import namedtuple

import numpy as np

from bootstrap_ref import philox4x32_10

STRIPES = 16
BITS = 0xC0000000

ClOut = namedtuple("ClOut", "labels iters inertia together same ambiguous valid centres flags")
ClOut.__doc__ = """labels [nk, B, D] int8; iters [nk, B] int32; inertia [nk, B]; together, same [nk, D, D] uint32; ambiguous, valid [nk] int64;
centres: {(ki, b): [k, P]} of the pairs that ran; flags: {(ki, b): set of "skipped", "s0", "empty", "maxiter", "settled"}."""


def words(c0, c1, c2, c3, seed):
    """the four output words of one block, as Python ints"""
    w = philox4x32_10(np.array([c0], np.uint64), np.array([c1], np.uint64), np.array([c2], np.uint64), np.array([c3], np.uint64),
                      int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return [int(v[0]) for v in w]


def members(D, bg, keep, seed, stream):
    """the members of the replicate with GLOBAL index bg, ascending"""
    if keep == 0:
        return np.arange(D)
    nb = (D + 3) // 4
    z = np.zeros(nb, np.uint64)
    w = philox4x32_10(np.arange(nb, dtype=np.uint64), z + np.uint64(BITS), z + np.uint64(bg), z + np.uint64(stream), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    u = np.stack(w, axis=1).ravel()[:D]
    return np.flatnonzero(u < np.uint64(keep))


def dist(X, m):
    """[n]: sum_p (x_p - m_p)^2, p ascending from 0.0"""
    s = np.zeros(X.shape[0])
    for p in range(X.shape[1]):
        t = X[:, p] - m[p]
        s = s + t * t
    return s


def start(X, k, bg, seed, stream):
    """the k members (positions a) taken as centres, and whether the S = 0 branch was taken"""
    n = X.shape[0]
    u = []
    for blk in range((k + 3) // 4):
        u += words(blk, BITS | k, bg, stream, seed)
    chosen = [(u[0] * n) >> 32]
    md = dist(X, X[chosen[0]])
    s0 = False
    for i in range(1, k):
        cum = np.zeros(n)
        c = 0.0
        for a in range(n):
            c = c + md[a]
            cum[a] = c
        S = cum[n - 1]
        if S > 0.0:
            T = np.floor((cum / S) * 4294967296.0)
            pick = int(np.flatnonzero(T > float(u[i]))[0])
        else:
            s0 = True
            pick = min(a for a in range(n) if a not in chosen)
        chosen.append(pick)
        md = np.minimum(md, dist(X, X[pick]))
    return chosen, s0


def stripe_sum_rows(rows, d, k, lab):
    """[k, P] sums of `rows` per label and [k] counts: a stripe's members in ascending d from 0.0, then the 16 stripe sums in stripe order from 0.0"""
    P = rows.shape[1]
    slab = np.zeros((STRIPES, k, P))
    cnt = np.zeros(k, dtype=np.int64)
    for a in range(rows.shape[0]):                       # ascending d: ascending inside every stripe
        st = int(d[a]) % STRIPES
        slab[st, lab[a]] = slab[st, lab[a]] + rows[a]
        cnt[lab[a]] += 1
    s = np.zeros((k, P))
    for st in range(STRIPES):
        s = s + slab[st]
    return s, cnt


def kmeans(X, d, k, bg, seed, stream, maxiter):
    """one pair -> (labels [n], iters, inertia, centres [k, P], flags)"""
    n = X.shape[0]
    chosen, s0 = start(X, k, bg, seed, stream)
    flags = {"s0"} if s0 else set()
    cent = X[chosen].copy()
    lab = np.full(n, -1)
    it = 0
    while it < maxiter:
        it += 1
        dd = np.stack([dist(X, cent[c]) for c in range(k)], axis=1)
        new = np.argmin(dd, axis=1)                      # the first minimum: ties to the lowest centre
        md = dd[np.arange(n), new]
        changed = bool((new != lab).any())
        lab = new
        if not changed:
            flags.add("settled")
            break
        s, cnt = stripe_sum_rows(X, d, k, lab)
        if (cnt == 0).any():
            flags.add("empty")
        for c in range(k):
            if cnt[c] > 0:
                cent[c] = s[c] / float(cnt[c])
    if it == maxiter:
        flags.add("maxiter")
    tot, _ = stripe_sum_rows(md[:, None], d, 1, np.zeros(n, dtype=np.int64))
    return lab, it, float(tot[0, 0]), cent, flags


def pair_counts(labels):
    """labels [nk, B, D] -> together, same [nk, D, D] uint32"""
    nk, B, D = labels.shape
    tog = np.zeros((nk, D, D), dtype=np.uint32); same = np.zeros((nk, D, D), dtype=np.uint32)
    for ki in range(nk):
        for b in range(B):
            l = labels[ki, b].astype(np.int64)
            m = l >= 0
            both = m[:, None] & m[None, :]
            tog[ki] += both.astype(np.uint32)
            same[ki] += (both & (l[:, None] == l[None, :])).astype(np.uint32)
    return tog, same


def pac_counts(tog, same, pac_lo, pac_hi):
    """-> ambiguous, valid [nk] int64 over the pairs i < j, in integers"""
    nk, D, _ = tog.shape
    up = np.triu(np.ones((D, D), dtype=bool), 1)
    amb = np.zeros(nk, dtype=np.int64); val = np.zeros(nk, dtype=np.int64)
    for ki in range(nk):
        t = tog[ki].astype(np.int64); s = same[ki].astype(np.int64)
        v = up & (t > 0)
        val[ki] = int(v.sum())
        amb[ki] = int((v & (1000 * s > pac_lo * t) & (1000 * s < pac_hi * t)).sum())
    return amb, val


def cluster(x, ks, B, b0=0, keep=0, seed=0, stream=0, maxiter=100, pac_lo=100, pac_hi=900):
    x = np.ascontiguousarray(x, dtype=np.float64)
    D = x.shape[0]
    nk = len(ks)
    labels = np.full((nk, B, D), -1, dtype=np.int8)
    iters = np.zeros((nk, B), dtype=np.int32); inertia = np.zeros((nk, B))
    centres, flags = {}, {}
    for b in range(B):
        mem = members(D, b0 + b, keep, seed, stream)
        for ki, k in enumerate(ks):
            if mem.size < k:
                flags[(ki, b)] = {"skipped"}
                continue
            lab, it, ine, cent, fl = kmeans(x[mem], mem, int(k), b0 + b, seed, stream, maxiter)
            labels[ki, b, mem] = lab
            iters[ki, b] = it; inertia[ki, b] = ine
            centres[(ki, b)] = cent; flags[(ki, b)] = fl
    tog, same = pair_counts(labels)
    amb, val = pac_counts(tog, same, pac_lo, pac_hi)
    return ClOut(labels, iters, inertia, tog, same, amb, val, centres, flags)


def consensus(tog, same):
    return np.where(tog > 0, same / np.maximum(tog, 1).astype(np.float64), 0.0)


def upgma(dm, k):
    """average linkage from its definition: the two groups with the smallest MEAN pairwise distance (over the original matrix) merge, the first
    such pair in the order of (smallest member of the one, smallest member of the other); groups numbered by their smallest member"""
    dm = np.asarray(dm, dtype=np.float64)
    D = dm.shape[0]
    groups = [[i] for i in range(D)]
    while len(groups) > k:
        Z = np.zeros((len(groups), D))
        for g, idx in enumerate(groups):
            Z[g, idx] = 1.0
        size = Z.sum(axis=1)
        avg = (Z @ dm @ Z.T) / np.outer(size, size)
        np.fill_diagonal(avg, np.inf)
        g, h = divmod(int(np.argmin(avg)), len(groups))  # groups stay sorted by their smallest member
        groups[g] = sorted(groups[g] + groups[h])
        del groups[h]
    lab = np.zeros(D, dtype=np.int64)
    for g, idx in enumerate(groups):
        lab[idx] = g
    return lab


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name x ks B b0 keep seed maxiter pac_lo pac_hi")


def keep_of(f):
    return int(np.floor(f * 4294967296.0))


def blobs(D, P, G, seed, spread=0.08):
    """D rows round G random centres in [0, 1]^P, continuous: no two distances tie"""
    rng = np.random.default_rng([D, P, G, seed])
    c = rng.uniform(0.0, 1.0, size=(G, P))
    return c[rng.integers(0, G, size=D)] + spread * rng.standard_normal((D, P))


# LDS placement of the per-block arrays: 8 (kmax P + 16) + 2328 + 8 (2 D + 16 kmax P + D (P | 1)) + 12 D <= 160 KiB; with P = 3, kmax = 2 that is
# 3272 + 52 D: D = 3087 is the largest that fits, D = 3088 the smallest that goes to memory
LDS_EDGE = 3087


@functools.lru_cache(maxsize=None)
def cases():
    two = np.zeros((12, 2)); two[1::2] = [1.0, 2.0]; two[::2] = [0.25, -0.5]          # two distinct rows: S = 0 at the third centre, which stays empty
    out = [
        Case("D1P1", np.array([[0.5]]), (1,), 3, 0, 0, 11, 10, 100, 900),
        Case("D3P1", np.array([[0.0], [1.0], [5.0]]), (1, 2, 3), 4, 0, 0, 12, 10, 100, 900),                      # k = n
        Case("D5P2keep", blobs(5, 2, 2, 1), (1, 2, 3), 12, 0, keep_of(0.35), 13, 10, 100, 900),                    # some n < k, some n = 0
        Case("D12two", two, (3,), 6, 0, 0, 14, 10, 100, 900),
        Case("D12twokeep", two, (2, 3), 6, 0, keep_of(0.7), 15, 10, 100, 900),
        Case("D65P3", blobs(65, 3, 3, 2), (2, 3, 4), 5, 0, keep_of(0.8), 16, 50, 100, 900),                         # past one wave
        Case("D130P33", blobs(130, 33, 4, 3), (3, 5), 4, 0, keep_of(0.8), 17, 50, 100, 900),
        Case("D257P1", blobs(257, 1, 3, 4), (2, 4), 4, 0, keep_of(0.8), 18, 50, 50, 950),
        Case("D40k32", blobs(40, 4, 6, 5), (32,), 3, 0, 0, 19, 50, 100, 900),
        Case("maxiter1", blobs(65, 3, 3, 6, 0.3), (3,), 4, 0, keep_of(0.8), 20, 1, 100, 900),
        Case("maxiter2", blobs(90, 5, 3, 7, 0.4), (4,), 4, 0, keep_of(0.8), 21, 2, 100, 900),                      # a stop at maxiter with centres moved
        Case("nk16", blobs(24, 2, 4, 8), tuple(range(1, 17)), 3, 0, keep_of(0.9), 22, 30, 100, 900),
        Case("b0", blobs(65, 3, 3, 2), (2, 3), 6, 0, keep_of(0.8), 16, 50, 100, 900),                              # sliced and added from b0 > 0
        Case("ldsfits", blobs(LDS_EDGE, 3, 2, 9, 0.2), (2,), 2, 0, keep_of(0.999), 23, 3, 100, 900),
        Case("ldsover", blobs(LDS_EDGE + 1, 3, 2, 9, 0.2), (2,), 2, 0, keep_of(0.999), 23, 3, 100, 900),
    ]
    return out


_REF = {}


def reference(c, b0=None, B=None):
    key = (c.name, b0, B)
    if key not in _REF:
        _REF[key] = cluster(c.x, c.ks, c.B if B is None else B, c.b0 if b0 is None else b0, c.keep, c.seed, 0, c.maxiter, c.pac_lo, c.pac_hi)
    return _REF[key]


def planted(D, P, G, conc, seed):
    """G Dirichlet(1) centres, D samples Dirichlet(conc centre) round them, Hellinger features -> (x [D, P], truth [D])"""
    rng = np.random.default_rng([D, P, G, seed])
    c = rng.dirichlet(np.ones(P), size=G)
    truth = np.arange(D) % G
    E = np.stack([rng.dirichlet(conc * c[g] + 1e-3) for g in truth])
    return np.sqrt(E / E.sum(axis=1, keepdims=True)), truth


# (D, P, G, concentration, seed): seeds at which the restatement finds the planted groups with the PAC margin tests/test_cluster_cpu.py asserts
PLANTED = [(96, 8, 4, 60.0, 8), (130, 10, 5, 80.0, 8)]
_PLANTED = {}


def planted_reference(D, P, G, conc, seed):
    """the restatement on a planted case: ks = 2 .. G + 2, B = 100, subsample 0.8"""
    key = (D, P, G, conc, seed)
    if key not in _PLANTED:
        x, _ = planted(D, P, G, conc, seed)
        _PLANTED[key] = cluster(x, tuple(range(2, G + 3)), 100, 0, keep_of(0.8), 1000 + seed, 0, 100, 100, 900)
    return _PLANTED[key]
