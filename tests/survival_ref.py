"""numpy restatement of mmm_survival_association (include/mmmusig.h) and the cases its tests share.

Written from the header text: its own Philox4x32-10, doubled midranks by counting, np.lexsort for every order, the scores by a loop over the
distinct event times of a stratum, the 128-bit quantities as Python ints, T as integer sums in int64 and every statistic in float64 in the
written order (the strata and the levels in explicit loops from 0.0, every product, division and sum a separate numpy operation).  The
per-cut moments are vectors over the cuts, one numpy operation per stratum and step.  It shares no code with the package."""
import functools
from collections import namedtuple

import numpy as np

BITS = 0xA0000000
SCALE = 16777216.0
M32 = np.uint64(0xFFFFFFFF)

SvOut = namedtuple("SvOut", "obs_trend z_trend obs_group u_group obs_cut cut_at ge_trend gemax_trend ge_cut gemax_cut ge_group maxstat")
SvOut.__doc__ = """obs_trend, obs_cut [P] float64; z_trend [P], u_group [Q] int64; obs_group [C] float64; cut_at [P] int32; ge_trend, gemax_trend,
ge_cut, gemax_cut [P], ge_group [C] uint32; maxstat [B, 2] float64.  With the cuts off obs_cut, cut_at, ge_cut and gemax_cut are zeros."""


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
    if v.size > 1024:                                    # the same counts from a sorted copy
        u = np.sort(v + 0.0)
        less, upto = np.searchsorted(u, v + 0.0, side="left"), np.searchsorted(u, v + 0.0, side="right")
        return (2 * less + (upto - less) + 1).astype(np.int64)
    return (2 * (v[None, :] < v[:, None]).sum(axis=1) + (v[None, :] == v[:, None]).sum(axis=1) + 1).astype(np.int64)


def scores(time, event, strata=None):
    """-> a [D] float64 (event - H, H the Nelson-Aalen sum of the sample's stratum at its time), A [D] int64 = rint(a 2^24)"""
    time = np.asarray(time, np.float64)
    event = np.asarray(event).astype(np.int64)
    D = time.size
    s = np.zeros(D, np.int64) if strata is None else np.asarray(strata, np.int64)
    a = np.zeros(D)
    for code in sorted(set(s.tolist())):
        mem = np.flatnonzero(s == code)
        t, ev = time[mem], event[mem]
        H = np.zeros(mem.size)
        for u in sorted(set(t[ev == 1].tolist())):       # ascending; every quotient and every sum rounded on its own
            dj, nj = int(((t == u) & (ev == 1)).sum()), int((t >= u).sum())
            H = np.where(t >= u, H + np.float64(dj) / np.float64(nj), H)
        a[mem] = ev.astype(np.float64) - H
    return a, np.rint(a * SCALE).astype(np.int64)


class Moments:
    """E and V of integer columns under the within-stratum permutation, as the header writes them"""

    def __init__(self, A, strata):
        D = A.size
        self.s = np.zeros(D, np.int64) if strata is None else np.asarray(strata, np.int64)
        self.codes = sorted(set(self.s.tolist()))
        self.n, self.SA, self.NA = {}, {}, {}
        for c in self.codes:
            Ai = [int(v) for v in A[self.s == c]]
            n, sa = len(Ai), sum(Ai)
            self.n[c], self.SA[c] = n, sa
            self.NA[c] = float(n * sum(v * v for v in Ai) - sa * sa)      # a Python int: exact, then rounded to nearest even

    def of(self, Fs, F2s):
        """Fs, F2s: per stratum code the sums of f and f^2 as int64 arrays of one shape (one entry per column) -> E, V float64 arrays"""
        shape = np.shape(Fs[self.codes[0]])
        E, V = np.zeros(shape), np.zeros(shape)
        for c in self.codes:
            n = self.n[c]
            F, F2 = np.asarray(Fs[c], np.int64), np.asarray(F2s[c], np.int64)
            E = E + (F.astype(np.float64) * np.float64(self.SA[c])) / np.float64(n)
            if n >= 2:
                NF = n * F2 - F * F
                V = V + (NF.astype(np.float64) * np.float64(self.NA[c])) / ((np.float64(n) * np.float64(n)) * np.float64(n - 1))
        return E, V

    def columns(self, f):
        """f [D, ncol] int64 -> E, V [ncol]"""
        f = np.asarray(f, np.int64)
        return self.of({c: f[self.s == c].sum(axis=0) for c in self.codes}, {c: (f[self.s == c] ** 2).sum(axis=0) for c in self.codes})


def stat(T, E, V):
    """t of integer T (any shape) against E, V: 0 where V is not > 0"""
    dz = np.asarray(T, np.int64).astype(np.float64) - E
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(V > 0, (dz * dz) / V, 0.0)


class Plan:
    """everything that does not depend on the permutation"""

    def __init__(self, x, levels, groups, time, event, strata, m_lo):
        x = np.asarray(x, np.float64)
        self.D, self.P = D, P = x.shape
        self.levels = tuple(int(g) for g in levels)
        self.C, self.Q = len(self.levels), sum(self.levels)
        self.strata, self.cuts = strata, m_lo >= 1
        self.a, self.A = scores(time, event, strata)
        mom = Moments(self.A, strata)
        self.Rx = np.stack([r2(x[:, p]) for p in range(P)], axis=1)
        self.Et, self.Vt = mom.columns(self.Rx)
        g = np.zeros((D, 0), np.int64) if self.C == 0 else np.asarray(groups, np.int64).reshape(D, self.C)
        self.ind = np.zeros((D, self.Q), np.int64)
        self.col0 = [0]
        for c, G in enumerate(self.levels):
            for lv in range(G):
                self.ind[:, self.col0[-1] + lv] = g[:, c] == lv
            self.col0.append(self.col0[-1] + G)
        self.Eg, self.Vg = mom.columns(self.ind) if self.Q else (np.zeros(0), np.zeros(0))
        d = np.arange(D)
        self.order = [np.lexsort((d, x[:, p] + 0.0)) for p in range(P)]              # -0.0 + 0.0 = 0.0
        self.Ec, self.Vc = np.zeros((P, max(D - 1, 0))), np.zeros((P, max(D - 1, 0)))
        if self.cuts and D > 1:
            j = np.arange(1, D)
            for p in range(P):
                o = self.order[p]
                Fs = {c: np.cumsum(mom.s[o] == c)[:D - 1].astype(np.int64) for c in mom.codes}
                E, V = mom.of(Fs, Fs)                                                # an indicator: f^2 = f
                allowed = (x[o[:-1], p] < x[o[1:], p]) & (m_lo <= j) & (j <= D - m_lo)
                self.Ec[p], self.Vc[p] = E, np.where(allowed, V, 0.0)                # V = 0 takes a cut out

    def statistics(self, pi):
        """-> t_trend [P], T_trend [P], t_group [C], T_group [Q], t_cut [P], cut_at [P]"""
        Api = self.A[pi]
        Tt = self.Rx.T @ Api
        tt = stat(Tt, self.Et, self.Vt)
        Tg = self.ind.T @ Api
        tq = stat(Tg, self.Eg, self.Vg)
        tg = np.zeros(self.C)
        for c in range(self.C):
            acc = np.float64(0.0)
            for q in range(self.col0[c], self.col0[c + 1]):
                if self.Vg[q] > 0:
                    acc = acc + tq[q]
            tg[c] = acc
        tc, at = np.zeros(self.P), np.zeros(self.P, np.int32)
        if self.cuts and self.D > 1:
            for p in range(self.P):
                ok = self.Vc[p] > 0
                if ok.any():
                    t = stat(np.cumsum(Api[self.order[p]])[:self.D - 1], self.Ec[p], self.Vc[p])
                    tc[p] = t[ok].max()
                    at[p] = 1 + int(np.flatnonzero(ok & (t == tc[p]))[0])
        return tt, Tt, tg, Tg, tc, at


def survival(x, levels, groups, time, event, strata, m_lo, B, b0, seed, stream=0):
    pl = Plan(x, levels, groups, time, event, strata, m_lo)
    P, C = pl.P, pl.C
    ot, zt, og, ug, oc, at = pl.statistics(np.arange(pl.D))
    ge_t, gm_t, ge_c, gm_c, ge_g = (np.zeros(n, np.uint32) for n in (P, P, P, P, C))
    ms = np.zeros((B, 2))
    for b in range(B):
        tt, _, tg, _, tc, _ = pl.statistics(permutation(pl.D, strata, b0 + b, seed, stream))
        Mt, Mc = max(0.0, tt.max()), max(0.0, tc.max())
        ge_t += (tt >= ot).astype(np.uint32)
        gm_t += (Mt >= ot).astype(np.uint32)
        ge_g += (tg >= og).astype(np.uint32)
        if pl.cuts:
            ge_c += (tc >= oc).astype(np.uint32)
            gm_c += (Mc >= oc).astype(np.uint32)
        ms[b] = (Mt, Mc)
    return SvOut(ot, zt.astype(np.int64), og, ug.astype(np.int64), oc, at, ge_t, gm_t, ge_c, gm_c, ge_g, ms)


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
Case = namedtuple("Case", "name x levels groups time event strata m_lo B b0 seed")


def draw(D, P, levels, seed, ties=False):
    rng = np.random.default_rng(seed)
    x = rng.random((D, P))
    groups = np.stack([rng.integers(0, G, size=D) for G in levels], axis=1).astype(np.int32) if levels else None
    time = rng.exponential(1.0, size=D)
    if ties:
        time = np.round(time, 1)
    event = (rng.random(D) < 0.6).astype(np.uint8)
    return x, groups, time, event


def cases():
    out = []

    def add(name, D, P, levels, B, m_lo=1, strata=None, b0=0, seed=None, data=None, ties=False):
        x, groups, time, event = data if data is not None else draw(D, P, levels, 200 + len(out), ties)
        out.append(Case(name, x, tuple(levels), groups, time, event, None if strata is None else np.asarray(strata, np.int32), m_lo, B, b0,
                        17 + len(out) if seed is None else seed))

    for D in (1, 2, 5, 63, 64, 65, 257):
        add("D%d" % D, D, 3, [2, 3], 5, b0=D, ties=D == 65)
    add("D4096", 4096, 2, [2], 4, m_lo=0)
    add("D300", 300, 2, [2], 4, m_lo=30, ties=True)
    add("P1", 20, 1, [2], 6)
    add("P33", 13, 33, [2], 6)
    add("P256", 9, 256, [3], 4)
    add("C0", 24, 3, [], 6)
    add("Q256", 70, 3, [32] * 8, 3)
    # contents: 80 % zeros, a constant feature, -0.0 beside 0.0, times tied at one decimal with events and censorings at one time, a level
    # without members
    rng = np.random.default_rng(56)
    D = 40
    x = rng.random((D, 4))
    x[rng.permutation(D)[:32], 0] = 0.0
    x[:, 1] = 3.25
    x[:, 2] = rng.choice([-0.0, 0.0, 1.0], size=D)
    groups = np.stack([rng.choice([0, 1, 2, 4], size=D), rng.integers(0, 2, size=D)], axis=1).astype(np.int32)
    time = np.round(rng.exponential(1.0, size=D), 1)
    event = (rng.random(D) < 0.6).astype(np.uint8)
    data = (x, groups, time, event)
    add("contents", D, 4, [5, 2], 40, data=data)
    add("censored", D, 4, [5, 2], 6, data=(x, groups, time, np.zeros(D, np.uint8)))
    add("onetime", D, 4, [5, 2], 6, data=(x, groups, np.where(event == 1, 0.7, time), event))
    add("onecut", D, 4, [5, 2], 6, m_lo=D // 2, data=data)
    add("nocut", D, 4, [5, 2], 6, m_lo=9, data=data)        # feature 0: 32 zeros, then 8 values: its cuts 32 .. 39 lie beyond D - m_lo = 31
    add("onestratum", 30, 3, [3], 10, strata=np.full(30, 5))
    add("allalone", 30, 3, [3], 10, strata=np.arange(30)[::-1])
    add("sizes", 64, 3, [3], 12, strata=[2] + [0, 0] + [1] * 61)
    add("unordered", 41, 3, [2, 2], 12, strata=np.random.default_rng(9).integers(0, 4, size=41)[::-1] * 10)
    add("strata64", 150, 2, [2], 4, strata=np.random.default_rng(10).permutation(np.arange(150) % 64) * 2, ties=True)
    add("many", 5, 2, [2], 3000)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, b0, B):
    c = next(v for v in cases() if v.name == name)
    return survival(c.x, c.levels, c.groups, c.time, c.event, c.strata, c.m_lo, B, b0, c.seed)


def reference(c, b0=None, B=None):
    """computed once per (case, b0, B) and shared; do not modify the result"""
    return _reference(c.name, c.b0 if b0 is None else b0, c.B if B is None else B)


# ---- planted and confounded inputs ---------------------------------------------------------------------------------------------------------------
PLANTED_SEED, PLANTED_B, PLANTED_MLO = 5, 999, 12
CONFOUNDED_SEED = 5


def planted(seed=PLANTED_SEED):
    """D = 120, P = 5: the hazard is exp(0.9 x_0 + 1.6 [x_1 > 0.5] + 1.2 grp); exponential censoring with mean 1.5; times rounded to 0.01; the
    features 2 .. 4 and the second group column are noise -> x, groups [D, 2], levels, time, event"""
    rng = np.random.default_rng(seed)
    D = 120
    x = rng.random((D, 5))
    x[:, 0] = rng.standard_normal(D)
    grp = rng.integers(0, 2, size=D)
    noise = rng.integers(0, 3, size=D)
    hazard = np.exp(0.9 * x[:, 0] + 1.6 * (x[:, 1] > 0.5) + 1.2 * grp)
    t_event = rng.exponential(1.0, size=D) / hazard
    t_cens = rng.exponential(1.5, size=D)
    time = np.round(np.minimum(t_event, t_cens), 2)
    event = (t_event <= t_cens).astype(np.uint8)
    return x, np.stack([grp, noise], axis=1).astype(np.int32), (2, 3), time, event


@functools.lru_cache(maxsize=None)
def planted_reference():
    x, groups, levels, time, event = planted()
    return survival(x, levels, groups, time, event, None, PLANTED_MLO, PLANTED_B, 0, 1000 + PLANTED_SEED)


def confounded(seed=CONFOUNDED_SEED):
    """D = 90 in three strata of 30 that drive both the hazard and the feature; inside a stratum they are independent -> x, time, event, strata"""
    rng = np.random.default_rng(seed)
    s = np.repeat(np.arange(3), 30)
    x = (2.0 * s + rng.standard_normal(90))[:, None]
    t_event = rng.exponential(1.0, size=90) / np.exp(1.5 * s)
    t_cens = rng.exponential(2.0, size=90)
    return x, np.round(np.minimum(t_event, t_cens), 2), (t_event <= t_cens).astype(np.uint8), s.astype(np.int32)
