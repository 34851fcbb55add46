"""numpy restatement of mmm_classify_exposures (include/mmmusig.h) and the cases its tests share.

Written from the header text: its own Philox4x32-10, np.lexsort for the permutation, and every fit in float64 in the written order -- eta as a
loop over the coefficients from w_0, the stripe sums as np.cumsum (strictly sequential) over a stripe's members from 0.0 and then over the 16
stripes from 0.0, the Cholesky factor and both substitutions as loops over single subtractions, every product, quotient and sum a separate
numpy operation.  Many fits run side by side along a leading axis; a fit that has ended is taken out.  A sample outside the training set
enters its stripe as +0.0, which changes no bit: a sum that starts at +0.0 is never -0.0.  ar_exp is the host build of csrc/mmm_arith.h that
the checker library exposes (orc_ar_exp_vec).  It shares no code with the package."""
import functools
from collections import namedtuple

import numpy as np

BITS = 0x90000000
M32 = np.uint64(0xFFFFFFFF)
LDS_ROWS = 64 * 1024

ClOut = namedtuple("ClOut", "scores u2_obs s_obs coef full_iters ge gemax maxstat events")
ClOut.__doc__ = """scores [R, L, D] float64; u2_obs [R, L], s_obs [L] int64; coef [L, Q] float64; full_iters [L, 2] int32; ge, gemax [L] uint32;
maxstat [B] int64; events [4] uint32"""


def ar_exp(v):
    from oracle import oracle as orc
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.empty_like(v)
    orc.lib().orc_ar_exp_vec(v.size, v.reshape(-1), out.reshape(-1))
    return out


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


def eta_of(w, z):
    """w [n, Q], z [n, D, Q] (column 0 is the 1) -> eta [n, D]: from w_0, ascending j"""
    e = np.repeat(w[:, 0:1], z.shape[1], axis=1)
    for j in range(1, w.shape[1]):
        e = e + z[:, :, j] * w[:, j:j + 1]
    return e


def stripe_sum(t):
    """t [n, D, E], +0.0 where a sample does not take part -> [n, E]: stripe i mod 16 in ascending i from 0.0, then the stripes from 0.0"""
    n, D, E = t.shape
    rows = (D + 15) // 16
    pad = np.zeros((n, 1 + rows, 16, E))
    pad.reshape(n, -1, E)[:, 16:16 + D] = t                  # row 0 is the 0.0 every stripe starts from
    per = np.cumsum(pad, axis=1)[:, -1]                      # [n, 16, E]
    return np.cumsum(np.concatenate([np.zeros((n, 1, E)), per], axis=1), axis=1)[:, -1]


def tri(Q):
    jj, kk = np.tril_indices(Q)                              # row-major over the lower triangle: entry j (j + 1) / 2 + k
    return jj, kk


def newton_step(g, H):
    """g [n, Q], H [n, Q, Q] (lower triangle) -> d [n, Q], failed [n] (a radicand not > 0 or not finite)"""
    n, Q = g.shape
    C = np.zeros((n, Q, Q))
    failed = np.zeros(n, bool)
    for k in range(Q):
        s = H[:, k, k].copy()
        for m in range(k):
            s = s - C[:, k, m] * C[:, k, m]
        failed |= ~((s > 0) & np.isfinite(s))
        ckk = np.sqrt(np.where(failed, 1.0, s))
        C[:, k, k] = ckk
        if k + 1 < Q:
            s2 = H[:, k + 1:, k].copy()
            for m in range(k):
                s2 = s2 - C[:, k + 1:, m] * C[:, k:k + 1, m]
            C[:, k + 1:, k] = s2 / ckk[:, None]
    u = np.zeros((n, Q))
    for k in range(Q):
        s = g[:, k].copy()
        for m in range(k):
            s = s - C[:, k, m] * u[:, m]
        u[:, k] = s / C[:, k, k]
    d = np.zeros((n, Q))
    for k in range(Q - 1, -1, -1):
        s = u[:, k].copy()
        for m in range(Q - 1, k, -1):
            s = s - C[:, m, k] * d[:, m]
        d[:, k] = s / C[:, k, k]
    return d, failed


def fit_batch(zp, pid, y, member, lam, maxiter, tol):
    """zp [nb, D, P]: the permuted rows of nb replicates; fit n uses zp[pid[n]], the training set member[n] [D] (bool) and the penalty lam[n]
    -> w [N, Q], iterations [N], status [N]"""
    N, D = member.shape
    P = zp.shape[2]
    Q = P + 1
    zq = np.concatenate([np.ones((zp.shape[0], D, 1)), zp], axis=2)
    jj, kk = tri(Q)
    diag = np.flatnonzero(jj == kk)
    w, its, status = np.zeros((N, Q)), np.zeros(N, np.int32), np.full(N, -1, np.int32)
    yv = np.asarray(y, np.float64)
    step = max(1, (48 << 20) // (8 * D * jj.size))           # fits side by side
    with np.errstate(all="ignore"):
        for it in range(1, maxiter + 1):
            live = np.flatnonzero(status < 0)
            if live.size == 0:
                break
            for lo in range(0, live.size, step):
                a = live[lo:lo + step]
                z, wa, m = zq[pid[a]], w[a], member[a][:, :, None]
                eta = eta_of(wa, z)
                ec = np.where(eta < -700.0, -700.0, np.where(eta > 700.0, 700.0, eta))
                p = 1.0 / (1.0 + ar_exp(-ec))
                om, r = p * (1.0 - p), p - yv[None, :]
                pen = np.zeros((a.size, Q))
                pen[:, 1:] = lam[a][:, None]
                g = stripe_sum(np.where(m, r[:, :, None] * z, 0.0)) + pen * wa
                Hl = stripe_sum(np.where(m, z[:, :, jj] * (om[:, :, None] * z[:, :, kk]), 0.0))
                Hl[:, diag] = Hl[:, diag] + pen
                H = np.zeros((a.size, Q, Q))
                H[:, jj, kk] = Hl
                d, failed = newton_step(g, H)
                wn = wa - d
                bad = ~np.isfinite(wn).all(axis=1)
                near = ~(np.abs(d) > tol).any(axis=1)
                st = np.where(failed | bad, 2, np.where(near, 0, 1 if it == maxiter else -1))
                w[a] = np.where(failed[:, None], wa, wn)
                its[a], status[a] = it, st
    return w, its, status


def u2(s, y):
    """the doubled pair count of scores s [D]: a NaN compares false"""
    sp, sn = s[np.asarray(y) == 1][:, None], s[np.asarray(y) == 0][None, :]
    with np.errstate(invalid="ignore"):
        return int((2 * (sp > sn).astype(np.int64) + (sp == sn).astype(np.int64)).sum())


def classify(x, y, strata, fold, F, lambdas, maxiter, tol, B, b0, seed, stream=0):
    x = np.asarray(x, np.float64)
    y = np.asarray(y).astype(np.int64)
    fold = np.asarray(fold).astype(np.int64)
    lambdas = np.asarray(lambdas, np.float64)
    D, P = x.shape
    R, L = fold.shape[0], lambdas.size
    # the fits of one replicate, (r, l, f) in this order
    rr, ll, ff = (v.ravel() for v in np.meshgrid(np.arange(R), np.arange(L), np.arange(F), indexing="ij"))
    member = fold[rr] != ff[:, None]                                             # [R L F, D]
    nf = rr.size

    def replicate_stats(pis):
        """pis [nb, D] -> S [nb, L], u2 [nb, R, L], scores [nb, R, L, D], events [nb, 2]"""
        nb = pis.shape[0]
        zp = x[pis]                                                              # sample i receives x[pi(i)]
        pid = np.repeat(np.arange(nb), nf)
        w, _, status = fit_batch(zp, pid, y, np.tile(member, (nb, 1)), np.tile(lambdas[ll], nb), maxiter, tol)
        zq = np.concatenate([np.ones((nb, D, 1)), zp], axis=2)
        with np.errstate(all="ignore"):
            eta = eta_of(w, zq[pid]).reshape(nb, R, L, F, D)
        held = (fold[:, None, :] == np.arange(F)[None, :, None])                 # [R, F, D]
        sc = np.zeros((nb, R, L, D))
        for f in range(F):
            sc = np.where(held[None, :, None, f, :], eta[:, :, :, f, :], sc)
        U = np.array([[[u2(sc[b, r, l], y) for l in range(L)] for r in range(R)] for b in range(nb)], np.int64).reshape(nb, R, L)
        st = status.reshape(nb, nf)
        return U.sum(axis=1), U, sc, np.stack([(st == 1).sum(axis=1), (st == 2).sum(axis=1)], axis=1)

    ident = np.arange(D)[None, :]
    S0, U0, sc0, ev0 = replicate_stats(ident)
    wf, itf, stf = fit_batch(x[ident], np.zeros(L, np.int64), y, np.ones((L, D), bool), lambdas, maxiter, tol)
    events = np.zeros(4, np.uint32)
    events[0], events[1] = ev0[0, 0] + (stf == 1).sum(), ev0[0, 1] + (stf == 2).sum()
    ge, gemax, maxstat = np.zeros(L, np.uint32), np.zeros(L, np.uint32), np.zeros(B, np.int64)
    chunk = max(1, 4096 // nf)
    for lo in range(0, B, chunk):
        bs = range(lo, min(B, lo + chunk))
        Sb, _, _, ev = replicate_stats(np.stack([permutation(D, strata, b0 + b, seed, stream) for b in bs]))
        M = Sb.max(axis=1)
        maxstat[lo:lo + len(bs)] = M
        ge += (Sb >= S0[0][None, :]).sum(axis=0).astype(np.uint32)
        gemax += (M[:, None] >= S0[0][None, :]).sum(axis=0).astype(np.uint32)
        events[2] += ev[:, 0].sum()
        events[3] += ev[:, 1].sum()
    return ClOut(sc0[0], U0[0], S0[0], wf, np.stack([itf, stf], axis=1).astype(np.int32), ge, gemax, maxstat, events)


def rows_in_lds(D, P):
    """whether the kernel holds the permuted rows in LDS: the block's layout (csrc/classify.hip, cf_layout) with the rows within 64 KiB"""
    n2, Q = 1, P + 1
    while n2 < D:
        n2 *= 2
    om = (8 * n2 + 2 * D + D + 7) & ~7
    return om + 16 * D + 16 * Q + 8 * (Q * (Q + 1) // 2) + 8 * 33 + 16 + 8 * D * P <= LDS_ROWS


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name x y strata fold F lambdas maxiter tol B b0 seed")


def deal(y, strata, F, R, seed):
    """folds for the cases: per repeat a shuffled round-robin deal inside every (stratum, class) cell, continued from cell to cell"""
    y = np.asarray(y)
    s = np.zeros(y.size, np.int64) if strata is None else np.asarray(strata)
    rng = np.random.default_rng(seed)
    out = np.zeros((R, y.size), np.uint8)
    for r in range(R):
        nxt = 0
        for code in np.unique(s):
            for c in (0, 1):
                mem = rng.permutation(np.flatnonzero((s == code) & (y == c)))
                out[r, mem] = (nxt + np.arange(mem.size)) % F
                nxt += mem.size
    return out


def cases():
    out = []

    def add(name, D, P, R, F, L, B, strata=None, b0=0, maxiter=30, tol=1e-8, x=None, y=None, lambdas=None, fold=None, frac=0.4):
        rng = np.random.default_rng(300 + len(out))
        if x is None:
            x = rng.standard_normal((D, P))
        if y is None:
            y = np.zeros(D, np.uint8)
            y[rng.permutation(D)[:max(F if fold is None else 2, int(round(frac * D)))]] = 1
            x = x + 0.8 * y[:, None] * (np.arange(P) == 0)
        if lambdas is None:
            lambdas = np.array([1.0]) if L == 1 else 10.0 ** np.linspace(-2, 2, L)
        st = None if strata is None else np.asarray(strata, np.int32)
        if fold is None:
            fold = deal(y, st, F, R, 900 + len(out))
        out.append(Case(name, np.ascontiguousarray(x, dtype=np.float64), np.asarray(y, np.uint8), st, np.asarray(fold, np.uint8), F, np.asarray(lambdas, np.float64),
                        maxiter, tol, B, b0, 41 + len(out)))

    add("D4", 4, 1, 1, 2, 1, 5, y=[0, 1, 0, 1], fold=[[0, 0, 1, 1]], x=np.array([[0.1], [0.9], [-0.4], [0.3]]))
    add("D5", 5, 2, 1, 2, 2, 5, b0=5)                            # fewer samples than stripes: eleven stripes stay empty
    add("D17", 17, 3, 3, 2, 1, 6, b0=17)
    add("D65", 65, 4, 1, 5, 8, 8, b0=65)
    add("D257", 257, 6, 3, 5, 2, 6)
    add("D300", 300, 5, 1, 5, 2, 4)
    add("P1", 20, 1, 1, 2, 2, 6)
    add("P33", 40, 33, 1, 2, 1, 2)
    add("P63", 70, 63, 1, 2, 1, 2)
    add("Fmin", 24, 3, 1, 6, 2, 6, frac=0.25)                    # six positive samples: F = min(n_1, n_0), one per fold
    add("sizes", 64, 3, 1, 3, 2, 8, strata=[2] + [0, 0] + [1] * 61)
    add("unordered", 41, 3, 3, 2, 1, 8, strata=np.random.default_rng(9).integers(0, 4, size=41)[::-1] * 10)
    # duplicated rows with unlike labels: tied scores within and between the classes
    rng = np.random.default_rng(77)
    half = rng.standard_normal((12, 2))
    add("ties", 36, 2, 1, 3, 2, 10, x=np.concatenate([half, half, half]), y=(np.arange(36) % 5 < 2).astype(np.uint8))
    # a separable label, a tiny penalty, three iterations: every fit stops at maxiter (status 1)
    xs = rng.standard_normal((30, 2))
    add("separable", 30, 2, 1, 3, 1, 6, x=xs, y=(xs[:, 0] > np.median(xs[:, 0])).astype(np.uint8), lambdas=[1e-6], maxiter=3)
    # a column scaled by 1e200: its Hessian entries overflow, the first pivot of that column is not finite (status 2)
    xb = rng.standard_normal((30, 3))
    xb[:, 1] *= 1e200
    add("scaled", 30, 3, 1, 3, 2, 6, x=xb)
    add("rows_lds", 300, 22, 1, 2, 1, 2)                         # the last P at D = 300 whose rows fit the 64 KiB
    add("rows_mem", 300, 24, 1, 2, 1, 2)                         # read through pi from memory
    add("many", 4, 1, 1, 2, 1, 1100, y=[0, 1, 0, 1], fold=[[0, 0, 1, 1]], x=np.array([[0.1], [0.9], [-0.4], [0.3]]), strata=[0, 0, 0, 0])
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, b0, B):
    c = next(v for v in cases() if v.name == name)
    return classify(c.x, c.y, c.strata, c.fold, c.F, c.lambdas, c.maxiter, c.tol, B, b0, c.seed)


def reference(c, b0=None, B=None):
    """computed once per (case, b0, B) and shared; do not modify the result"""
    return _reference(c.name, c.b0 if b0 is None else b0, c.B if B is None else B)


# ---- the planted effect ---------------------------------------------------------------------------------------------------------------------------
PLANTED_SEED, PLANTED_B, PLANTED_R, PLANTED_F = 1, 199, 2, 4
PLANTED_PENALTIES = (0.1, 1.0, 10.0, 100.0)


def planted(seed=PLANTED_SEED, effect=0.25):
    """D = 96, P = 6 uniform features, 30 % positive labels, `effect` added to feature 2 of the positive samples -> E, labels"""
    rng = np.random.default_rng(seed)
    D = 96
    labels = np.zeros(D, np.int64)
    labels[rng.permutation(D)[:29]] = 1
    E = rng.random((D, 6))
    E[:, 2] += effect * labels
    return E, labels
