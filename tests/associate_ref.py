"""numpy restatement of mmm_associate_exposures (include/mmmusig.h) and the cases its tests share.

Written from the header text: its own Philox4x32-10, doubled midranks by counting, np.lexsort for the two orders that make pi, the statistic as
an integer matrix product in int64 and t in float64 in the written order (the columns of a covariate in an explicit loop from 0.0, every
product, division and sum a separate numpy operation).  It shares no code with the package."""
import functools
from collections import namedtuple

import numpy as np

BITS = 0xE0000000
M32 = np.uint64(0xFFFFFFFF)

AsOut = namedtuple("AsOut", "obs zc_obs ge ge_max maxstat")
AsOut.__doc__ = "obs [P, C] float64; zc_obs [P, Q] int64; ge, ge_max [P, C] uint32; maxstat [B, C] float64"


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def keys(D, bg, seed, stream):
    """key_d, d < D, of the replicate with GLOBAL index bg"""
    nb = (D + 3) // 4
    z = np.zeros(nb, np.uint64)
    w = philox4x32_10(np.arange(nb, dtype=np.uint64), z + np.uint64(BITS), z + np.uint64(bg), z + np.uint64(stream), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return np.stack(w, axis=1).ravel()[:D]


def permutation(D, strata, bg, seed, stream=0):
    """pi [D]: pi(slot_j) = e_j"""
    s = np.zeros(D, np.int64) if strata is None else np.asarray(strata, np.int64)
    d = np.arange(D)
    slot = np.lexsort((d, s))                            # the last key is the primary one
    e = np.lexsort((d, keys(D, bg, seed, stream), s))
    pi = np.empty(D, np.int64)
    pi[slot] = e
    return pi


def r2(v):
    """doubled midranks: 2 #{less} + #{equal} + 1, IEEE comparisons"""
    v = np.asarray(v, np.float64)
    return (2 * (v[None, :] < v[:, None]).sum(axis=1) + (v[None, :] == v[:, None]).sum(axis=1) + 1).astype(np.int64)


def columns(levels, y):
    """-> Y [D, Q] int64, w [Q] int64, col0 [C + 1]"""
    y = np.asarray(y, np.float64)
    D = y.shape[0]
    cols, w, col0 = [], [], [0]
    for c, G in enumerate(levels):
        if G == 0:
            r = r2(y[:, c])
            cols.append(r); w.append(int(((r - (D + 1)) ** 2).sum()))
        else:
            for g in range(G):
                ind = (y[:, c] == g).astype(np.int64)
                cols.append(ind); w.append(int(ind.sum()))
        col0.append(len(cols))
    return np.stack(cols, axis=1), np.array(w, np.int64), col0


def statistic(Rx, Y, pi, w, ssx, col0):
    """-> t [P, C] float64, Zc [P, Q] int64"""
    D = Rx.shape[0]
    Z = Rx.T @ Y[pi]                                     # int64: sample i keeps its features and receives the row of pi(i)
    Zc = Z - (D + 1) * Y.sum(axis=0)[None, :]
    P, C = Rx.shape[1], len(col0) - 1
    t = np.zeros((P, C))
    for c in range(C):
        acc = np.zeros(P)
        for q in range(col0[c], col0[c + 1]):
            if w[q] == 0:
                continue
            zc = Zc[:, q].astype(np.float64)
            sq = zc * zc
            acc = acc + sq / np.float64(w[q])
        with np.errstate(invalid="ignore", divide="ignore"):
            t[:, c] = np.where(ssx != 0, acc / ssx.astype(np.float64), 0.0)
    return t, Zc


def associate(x, levels, y, strata, B, b0, seed, stream=0):
    x = np.asarray(x, np.float64)
    D, P = x.shape
    Rx = np.stack([r2(x[:, p]) for p in range(P)], axis=1)
    ssx = ((Rx - (D + 1)) ** 2).sum(axis=0)
    Y, w, col0 = columns(levels, y)
    C = len(levels)
    obs, zc = statistic(Rx, Y, np.arange(D), w, ssx, col0)
    ge, gm, ms = np.zeros((P, C), np.uint32), np.zeros((P, C), np.uint32), np.zeros((B, C))
    for b in range(B):
        t, _ = statistic(Rx, Y, permutation(D, strata, b0 + b, seed, stream), w, ssx, col0)
        M = t.max(axis=0)
        ge += (t >= obs).astype(np.uint32)
        gm += (M[None, :] >= obs).astype(np.uint32)
        ms[b] = M
    return AsOut(obs, zc, ge, gm, ms)


def bh(p):
    """Benjamini-Hochberg adjusted p-values of a flat list, written from the definition: q_(i) = min over j >= i of p_(j) m / j"""
    p = [float(v) for v in p]
    m = len(p)
    order = sorted(range(m), key=lambda i: p[i])
    q = [0.0] * m
    for rank, i in enumerate(order, start=1):
        q[i] = min(min(p[order[j - 1]] * m / j for j in range(rank, m + 1)), 1.0)
    return np.array(q)


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name x levels y strata B b0 seed")


def draw(D, P, levels, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((D, P))
    y = np.stack([rng.standard_normal(D) if G == 0 else rng.integers(0, G, size=D).astype(np.float64) for G in levels], axis=1)
    return x, y


def cases():
    out = []

    def add(name, D, P, levels, B, strata=None, b0=0, seed=None, xy=None):
        x, y = xy if xy is not None else draw(D, P, levels, 100 + len(out))
        out.append(Case(name, x, tuple(levels), y, None if strata is None else np.asarray(strata, np.int32), B, b0, 7 + len(out) if seed is None else seed))

    add("D1", 1, 2, [0, 2], 3)
    for D in (2, 5, 63, 64, 65, 257):
        add("D%d" % D, D, 3, [0, 3, 2], 5, b0=D)
    add("D4096", 4096, 2, [0, 2], 4)
    add("P1", 20, 1, [0, 2], 6)
    add("P33", 20, 33, [0, 2], 6)
    add("P256", 9, 256, [2, 0], 4)
    add("PC4097", 9, 241, [0] * 16 + [2], 4)                 # many counts per permutation
    add("Q1", 12, 2, [0], 8)
    add("Q256", 70, 3, [32] * 8, 3)
    # contents: 80 % zeros, a constant feature, -0.0 beside 0.0, a level without members, a constant numeric covariate, a tied numeric one
    rng = np.random.default_rng(55)
    D = 40
    x = rng.random((D, 4))
    x[rng.permutation(D)[:32], 0] = 0.0
    x[:, 1] = 3.25
    x[:, 2] = rng.choice([-0.0, 0.0, 1.0], size=D)
    y = np.stack([rng.choice([0.0, 1.0, 2.0, 4.0], size=D), np.full(D, -1.5), rng.choice([-0.0, 0.0, 2.0, 2.0, 7.5], size=D)], axis=1)
    add("contents", D, 4, [5, 0, 0], 40, xy=(x, y))
    add("onestratum", 30, 3, [0, 3], 10, strata=np.full(30, 5))
    add("allalone", 30, 3, [0, 3], 10, strata=np.arange(30)[::-1])
    add("sizes", 64, 3, [0, 3], 12, strata=[2] + [0, 0] + [1] * 61)
    add("unordered", 41, 3, [0, 2, 0], 12, strata=np.random.default_rng(9).integers(0, 4, size=41)[::-1] * 10)
    add("many", 5, 2, [0, 2], 3000)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, b0, B):
    c = next(v for v in cases() if v.name == name)
    return associate(c.x, c.levels, c.y, c.strata, B, b0, c.seed)


def reference(c, b0=None, B=None):
    """computed once per (case, b0, B) and shared; do not modify the result"""
    return _reference(c.name, c.b0 if b0 is None else b0, c.B if B is None else B)


# ---- planted and confounded inputs ---------------------------------------------------------------------------------------------------------------
PLANTED_SEED, PLANTED_B = 4, 999
CONFOUNDED_SEED = 5


def planted(seed=PLANTED_SEED):
    """D = 120, P = 6, C = 3: feature 0 is shifted between the two groups of covariate 0, feature 1 goes with the numeric covariate 1, covariate 2
    (three levels) and the features 2 .. 5 are noise -> x, y, levels, the planted (feature, covariate) pairs"""
    rng = np.random.default_rng(seed)
    D = 120
    grp = rng.integers(0, 2, size=D).astype(np.float64)
    num = rng.standard_normal(D)
    x = rng.standard_normal((D, 6))
    x[:, 0] += 1.6 * grp
    x[:, 1] += 1.2 * num
    y = np.stack([grp, num, rng.integers(0, 3, size=D).astype(np.float64)], axis=1)
    return x, y, (2, 0, 3), [(0, 0), (1, 1)]


@functools.lru_cache(maxsize=None)
def planted_reference():
    x, y, levels, _ = planted()
    return associate(x, levels, y, None, PLANTED_B, 0, 1000 + PLANTED_SEED)


def confounded(seed=CONFOUNDED_SEED):
    """D = 90 in three strata of 30 that drive both the feature and the numeric covariate; inside a stratum they are independent"""
    rng = np.random.default_rng(seed)
    s = np.repeat(np.arange(3), 30)
    x = (2.0 * s + rng.standard_normal(90))[:, None]
    y = (2.0 * s + rng.standard_normal(90))[:, None]
    return x, y, (0,), s.astype(np.int32)
