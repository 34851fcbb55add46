"""numpy restatement of mmm_cox_exposures (include/mmmusig.h) and the cases its tests share.

Written from the header text: its own Philox4x32-10, np.lexsort for the permutation, the time order and the tie groups, and every fit in
float64 in the written order -- eta as a loop over the coefficients from 0.0, the two scans chunk by chunk as np.cumsum (strictly sequential)
from 0.0 with the chunk offsets carried in a loop, the stripe sums as np.cumsum over a stripe's members from 0.0 and then over the 16 stripes
from 0.0, the Cholesky factor and both substitutions as loops over single subtractions, every product, quotient and sum a separate numpy
operation.  Many fits run side by side along a leading axis; a fit that has ended is taken out.  A sample outside the training set and a
group without a training event enter their sums as +0.0, which changes no bit: a sum that starts at +0.0 is never -0.0.  The pair count
compares every event sample with every sample through a [D, D] table of the comparable pairs, not through the contiguous ranges the library
forms.  ar_exp is the host build of csrc/mmm_arith.h that the checker library exposes (orc_ar_exp_vec).  It shares no code with the
package."""
import functools
from collections import namedtuple

import numpy as np

BITS = 0xB0000000
M32 = np.uint64(0xFFFFFFFF)
LDS_ROWS = 64 * 1024

CxOut = namedtuple("CxOut", "scores u2_obs s_obs n_pairs coef full_iters ge gemax maxstat events")
CxOut.__doc__ = """scores [R, L, D] float64; u2_obs [R, L], s_obs [L], n_pairs [1] int64; coef [L, P] float64; full_iters [L, 2] int32; ge, gemax [L]
uint32; maxstat [B] int64; events [4] uint32"""
Tables = namedtuple("Tables", "ord gstart gend cst cfirst clast NG NC comparable n_pairs")


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


def tables(time, event, strata):
    """what every replicate shares: the time order, the tie groups, the chunks, the comparable pairs"""
    t = np.asarray(time, np.float64) + 0.0
    ev = np.asarray(event).astype(bool)
    D = t.size
    s = np.zeros(D, np.int64) if strata is None else np.asarray(strata, np.int64)
    d = np.arange(D)
    order = np.lexsort((d, -t, s))                       # ascending (stratum, -time, index)
    so, to = s[order], t[order]
    news = np.r_[True, so[1:] != so[:-1]]
    newg = news | np.r_[True, to[1:] != to[:-1]]
    gstart = np.flatnonzero(newg)
    gend = np.r_[gstart[1:] - 1, D - 1]
    first = np.maximum.accumulate(np.where(news, d, 0))  # the first position of the stratum
    newc = (d - first) % 16 == 0
    cst = np.r_[np.flatnonzero(newc), D]
    cfirst = news[cst[:-1]]
    clast = np.r_[cfirst[1:], True]
    comparable = ev[:, None] & (s[:, None] == s[None, :]) & ((t[None, :] > t[:, None]) | ((t[None, :] == t[:, None]) & ~ev[None, :]))
    return Tables(order, gstart, gend, cst, cfirst, clast, gstart.size, cst.size - 1, comparable, int(comparable.sum()))


def eta_of(w, z):
    """w [n, P], z [n, D, P] -> eta [n, D]: from 0.0, ascending j"""
    e = np.zeros(z.shape[:2])
    for j in range(w.shape[1]):
        e = e + z[:, :, j] * w[:, j:j + 1]
    return e


def seq_cumsum(a):
    """a [n, m, ..] -> the sequential partial sums along axis 1, from 0.0"""
    return np.cumsum(np.concatenate([np.zeros_like(a[:, :1]), a], axis=1), axis=1)[:, 1:]


def scan_down(v, tb):
    """v [n, D, E] by position -> S [n, D, E]: offset of the chunk + partial inside it"""
    S = np.empty_like(v)
    run = None
    for c in range(tb.NC):
        lo, hi = tb.cst[c], tb.cst[c + 1]
        part = seq_cumsum(v[:, lo:hi])
        if tb.cfirst[c]:
            run = np.zeros((v.shape[0], v.shape[2]))
        S[:, lo:hi] = run[:, None, :] + part
        run = run + part[:, -1]
    return S


def scan_up(rho, tb):
    """rho [n, D] by position -> Hhat [n, D]: the same chunks, backwards"""
    H = np.empty_like(rho)
    run = None
    for c in range(tb.NC - 1, -1, -1):
        lo, hi = tb.cst[c], tb.cst[c + 1]
        part = seq_cumsum(rho[:, lo:hi][:, ::-1])[:, ::-1]
        if tb.clast[c]:
            run = np.zeros(rho.shape[0])
        H[:, lo:hi] = run[:, None] + part
        run = run + part[:, 0]
    return H


def stripe_sum(t):
    """t [n, D, E], +0.0 where a member does not take part -> [n, E]: stripe i mod 16 in ascending i from 0.0, then the stripes from 0.0"""
    n, D, E = t.shape
    rows = (D + 15) // 16
    pad = np.zeros((n, 1 + rows, 16, E))
    pad.reshape(n, -1, E)[:, 16:16 + D] = t                  # row 0 is the 0.0 every stripe starts from
    per = np.cumsum(pad, axis=1)[:, -1]                      # [n, 16, E]
    return np.cumsum(np.concatenate([np.zeros((n, 1, E)), per], axis=1), axis=1)[:, -1]


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


def iteration_terms(z, w, m, evq, tb):
    """one iteration's pieces, everything by position: z [n, D, P], w [n, P], m [n, D] (bool: in T), evq [D] -> u, Hhat, uh, M [n, D], dG
    [n, NG] (float), zbar [n, NG, P] (0.0 where dG = 0)"""
    eta = eta_of(w, z)
    ec = np.where(eta < -700.0, -700.0, np.where(eta > 700.0, 700.0, eta))
    u = np.where(m, ar_exp(ec), 0.0)
    S = scan_down(np.concatenate([u[:, :, None], u[:, :, None] * z], axis=2), tb)
    dG = np.add.reduceat((m & evq[None, :].astype(bool)).astype(np.int64), tb.gstart, axis=1).astype(np.float64)
    on = dG > 0
    S0 = np.where(on, S[:, tb.gend, 0], 1.0)
    r = np.where(on, dG / S0, 0.0)
    zbar = np.where(on[:, :, None], S[:, tb.gend, 1:] / S0[:, :, None], 0.0)
    rho = np.zeros_like(u)
    rho[:, tb.gend] = r
    Hhat = scan_up(rho, tb)
    uh = u * Hhat
    return u, Hhat, uh, evq[None, :].astype(np.float64) - uh, dG, zbar


def fit_batch(zp, pid, event, member, lam, tb, maxiter, tol):
    """zp [nb, D, P]: the permuted rows of nb replicates, by sample; fit n uses zp[pid[n]], the training set member[n] [D] (bool, by sample)
    and the penalty lam[n] -> w [N, P], iterations [N], status [N]"""
    N, D = member.shape
    P = zp.shape[2]
    zq, mq, evq = zp[:, tb.ord, :], member[:, tb.ord], np.asarray(event)[tb.ord]
    jj, kk = np.tril_indices(P)                              # row-major over the lower triangle: entry j (j + 1) / 2 + k
    diag = np.flatnonzero(jj == kk)
    w, its, status = np.zeros((N, P)), np.zeros(N, np.int32), np.full(N, -1, np.int32)
    step = max(1, (48 << 20) // (8 * D * max(jj.size, 1)))   # fits side by side
    with np.errstate(all="ignore"):
        for it in range(1, maxiter + 1):
            live = np.flatnonzero(status < 0)
            if live.size == 0:
                break
            for lo in range(0, live.size, step):
                a = live[lo:lo + step]
                z, wa, m = zq[pid[a]], w[a], mq[a]
                _, _, uh, M, dG, zbar = iteration_terms(z, wa, m, evq, tb)
                on = dG > 0
                pen = lam[a][:, None]
                g = pen * wa - stripe_sum(np.where(m[:, :, None], M[:, :, None] * z, 0.0))
                A = stripe_sum(np.where(m[:, :, None], z[:, :, jj] * (uh[:, :, None] * z[:, :, kk]), 0.0))
                Bg = stripe_sum(np.where(on[:, :, None], zbar[:, :, jj] * (dG[:, :, None] * zbar[:, :, kk]), 0.0))
                Hl = A - Bg
                Hl[:, diag] = Hl[:, diag] + pen
                H = np.zeros((a.size, P, P))
                H[:, jj, kk] = Hl
                d, failed = newton_step(g, H)
                wn = wa - d
                bad = ~np.isfinite(wn).all(axis=1)
                near = ~(np.abs(d) > tol).any(axis=1)
                st = np.where(failed | bad, 2, np.where(near, 0, 1 if it == maxiter else -1))
                w[a] = np.where(failed[:, None], wa, wn)
                its[a], status[a] = it, st
    return w, its, status


def u2(s, comparable):
    """the doubled pair count of scores s [D] over the comparable pairs: a NaN compares false"""
    with np.errstate(invalid="ignore"):
        gt, eq = s[:, None] > s[None, :], s[:, None] == s[None, :]
    return int(2 * (gt & comparable).sum() + (eq & comparable).sum())


def cox(x, time, event, strata, fold, F, lambdas, maxiter, tol, B, b0, seed, stream=0):
    x = np.asarray(x, np.float64)
    event = np.asarray(event).astype(np.int64)
    fold = np.asarray(fold).astype(np.int64)
    lambdas = np.asarray(lambdas, np.float64)
    D, P = x.shape
    R, L = fold.shape[0], lambdas.size
    tb = tables(time, event, strata)
    # the fits of one replicate, (r, l, f) in this order
    rr, ll, ff = (v.ravel() for v in np.meshgrid(np.arange(R), np.arange(L), np.arange(F), indexing="ij"))
    member = fold[rr] != ff[:, None]                                             # [R L F, D]
    assert (member & (event == 1)[None, :]).any(axis=1).all() and tb.n_pairs > 0
    nf = rr.size

    def replicate_stats(pis):
        """pis [nb, D] -> S [nb, L], u2 [nb, R, L], scores [nb, R, L, D], events [nb, 2]"""
        nb = pis.shape[0]
        zp = x[pis]                                                              # sample i receives x[pi(i)]
        pid = np.repeat(np.arange(nb), nf)
        w, _, status = fit_batch(zp, pid, event, np.tile(member, (nb, 1)), np.tile(lambdas[ll], nb), tb, maxiter, tol)
        with np.errstate(all="ignore"):
            eta = eta_of(w, zp[pid]).reshape(nb, R, L, F, D)
        held = (fold[:, None, :] == np.arange(F)[None, :, None])                 # [R, F, D]
        sc = np.zeros((nb, R, L, D))
        for f in range(F):
            sc = np.where(held[None, :, None, f, :], eta[:, :, :, f, :], sc)
        U = np.array([[[u2(sc[b, r, l], tb.comparable) for l in range(L)] for r in range(R)] for b in range(nb)], np.int64).reshape(nb, R, L)
        st = status.reshape(nb, nf)
        return U.sum(axis=1), U, sc, np.stack([(st == 1).sum(axis=1), (st == 2).sum(axis=1)], axis=1)

    ident = np.arange(D)[None, :]
    S0, U0, sc0, ev0 = replicate_stats(ident)
    wf, itf, stf = fit_batch(x[ident], np.zeros(L, np.int64), event, np.ones((L, D), bool), lambdas, tb, maxiter, tol)
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
    return CxOut(sc0[0], U0[0], S0[0], np.array([tb.n_pairs], np.int64), wf, np.stack([itf, stf], axis=1).astype(np.int32), ge, gemax, maxstat, events)


def placement(D, P, NG, NC):
    """-> (rows in LDS, zbar in LDS): the block's layout (csrc/cox.hip, cx_layout) held to 64 KiB, zbar first, then the rows beside it"""
    n2 = 1
    while n2 < D:
        n2 *= 2
    dg = (8 * n2 + 2 * D + D + 1) & ~1
    u = (dg + 2 * NG + 7) & ~7
    base = u + 16 * D + 16 * P + 8 * (P * (P + 1) // 2) + 8 * 33 + 8 * 32 + 16
    zbytes = 8 * (NG * (P + 1) + NC * (P + 2))
    zb = base + zbytes <= LDS_ROWS
    rows = base + (zbytes if zb else 0) + 8 * D * P <= LDS_ROWS
    return bool(rows), bool(zb)


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name x time event strata fold F lambdas maxiter tol B b0 seed")


def deal(event, strata, F, R, seed):
    """folds for the cases: per repeat a shuffled round-robin deal inside every (stratum, event) cell, continued from cell to cell"""
    event = np.asarray(event)
    s = np.zeros(event.size, np.int64) if strata is None else np.asarray(strata)
    rng = np.random.default_rng(seed)
    out = np.zeros((R, event.size), np.uint8)
    for r in range(R):
        nxt = 0
        for code in np.unique(s):
            for c in (0, 1):
                mem = rng.permutation(np.flatnonzero((s == code) & (event == c)))
                out[r, mem] = (nxt + np.arange(mem.size)) % F
                nxt += mem.size
    return out


def outcome(rng, x, effect=0.8, censor=1.5, decimals=2):
    """times whose hazard rises with feature 0, exponential censoring, rounded so that ties occur -> time, event"""
    te = rng.exponential(size=x.shape[0]) / np.exp(effect * x[:, 0])
    tc = rng.exponential(size=x.shape[0]) * censor
    t = np.minimum(te, tc)
    return (np.round(t, decimals) if decimals is not None else t), (te <= tc).astype(np.uint8)


def cases():
    out = []

    def add(name, D, P, R, F, L, B, strata=None, b0=0, maxiter=30, tol=1e-8, x=None, time=None, event=None, lambdas=None, fold=None, decimals=2):
        rng = np.random.default_rng(500 + len(out))
        if x is None:
            x = rng.standard_normal((D, P))
        if time is None:
            time, ev = outcome(rng, x, decimals=decimals)
            event = ev if event is None else event
        if lambdas is None:
            lambdas = np.array([1.0]) if L == 1 else 10.0 ** np.linspace(-2, 2, L)
        st = None if strata is None else np.asarray(strata, np.int32)
        if fold is None:
            fold = deal(event, st, F, R, 900 + len(out))
        out.append(Case(name, np.ascontiguousarray(x, dtype=np.float64), np.asarray(time, np.float64), np.asarray(event, np.uint8), st, np.asarray(fold, np.uint8), F,
                        np.asarray(lambdas, np.float64), maxiter, tol, B, b0, 41 + len(out)))

    tiny = dict(x=np.array([[0.1], [0.9], [-0.4], [0.3]]), time=[1.0, 2.0, 3.0, 4.0], event=[1, 0, 1, 0], fold=[[0, 0, 1, 1]])
    add("D4", 4, 1, 1, 2, 1, 5, **tiny)                          # two events, one in either training set
    add("D5", 5, 2, 1, 2, 2, 5, b0=5, event=[1, 0, 1, 1, 0])     # less than one chunk, eleven stripes stay empty
    add("D17", 17, 3, 3, 2, 1, 6, b0=17)                         # the chunk edge
    add("D33", 33, 2, 1, 3, 2, 6)
    add("D65", 65, 4, 1, 5, 8, 8, b0=65)
    add("D257", 257, 6, 3, 5, 2, 6)                              # 17 chunks: the prefix over the chunk totals is longer than a chunk
    add("D300", 300, 5, 1, 5, 2, 4)
    add("P1", 20, 1, 1, 2, 2, 6)
    add("P33", 40, 33, 1, 2, 1, 2)                               # beyond 32 lanes in the solve
    add("P64", 70, 64, 1, 2, 1, 2, lambdas=[20.0])                               # the limit: every lane of the wave owns a row
    ev = np.zeros(24, np.uint8)
    ev[[1, 5, 9, 14, 18, 22]] = 1
    add("Fmin", 24, 3, 1, 6, 2, 6, event=ev)                     # six events, F = 6: one per fold
    # position q = sample q (descending times); positions 13 .. 18 share a time across the chunk edge at 16, events and censored mixed
    tt = 40.0 - np.arange(40)
    tt[13:19] = 27.0
    tt[30:33] = 9.0
    add("tied_times", 40, 3, 1, 3, 2, 8, time=tt, event=(np.arange(40) % 3 != 1).astype(np.uint8))
    rng = np.random.default_rng(70)
    xa = rng.standard_normal((30, 2))
    add("all_events", 30, 2, 1, 3, 2, 6, x=xa, time=np.round(rng.exponential(size=30) / np.exp(0.7 * xa[:, 0]), 1), event=np.ones(30, np.uint8))
    # stratum 1 holds one event, stratum 2 none at all
    e1 = (np.arange(48) % 2 == 0).astype(np.uint8)
    e1[20:] = 0
    e1[25] = 1
    add("one_event_stratum", 48, 3, 1, 3, 2, 8, strata=[0] * 20 + [1] * 14 + [2] * 14, time=np.round(rng.exponential(size=48), 2), event=e1)
    add("sizes", 64, 3, 1, 3, 2, 8, strata=[2] + [0, 0] + [1] * 61)      # strata of 2, 61 and 1: the chunks start again at positions 2 and 63
    add("unordered", 41, 3, 3, 2, 1, 8, strata=np.random.default_rng(9).integers(0, 4, size=41)[::-1] * 10)
    # duplicated rows: tied scores among comparable samples
    half = rng.standard_normal((12, 2))
    add("ties", 36, 2, 1, 3, 2, 10, x=np.concatenate([half, half, half]), time=np.round(rng.exponential(size=36), 1), event=(np.arange(36) % 5 < 3).astype(np.uint8))
    # the risk order is the time order, no censoring, a tiny penalty, three iterations: every fit stops at maxiter (status 1)
    tm = np.arange(1.0, 31.0)
    add("monotone", 30, 2, 1, 3, 1, 6, x=np.stack([-tm / 10.0, rng.standard_normal(30)], axis=1), time=tm, event=np.ones(30, np.uint8), lambdas=[1e-6], maxiter=3)
    # a column scaled by 1e200: its Hessian entries overflow, the first pivot of that column is not finite (status 2)
    xb = rng.standard_normal((30, 3))
    xb[:, 1] *= 1e200
    add("scaled", 30, 3, 1, 3, 2, 6, x=xb)
    # D = 300 with distinct times (NG = 300, NC = 19): the last P whose rows fit the 64 KiB beside zbar and the first that does not; the
    # last P whose zbar fits and the first that does not (its rows then fit again); and a P at which neither fits
    add("rows_lds", 300, 10, 1, 2, 1, 2, decimals=None)
    add("rows_mem", 300, 11, 1, 2, 1, 2, decimals=None)
    add("zbar_lds", 300, 19, 1, 2, 1, 2, decimals=None)
    add("zbar_mem", 300, 20, 1, 2, 1, 2, decimals=None)
    add("both_mem", 300, 22, 1, 2, 1, 2, decimals=None)
    add("many", 4, 1, 1, 2, 1, 1100, strata=[0, 0, 0, 0], **tiny)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, b0, B):
    c = next(v for v in cases() if v.name == name)
    return cox(c.x, c.time, c.event, c.strata, c.fold, c.F, c.lambdas, c.maxiter, c.tol, B, b0, c.seed)


def reference(c, b0=None, B=None):
    """computed once per (case, b0, B) and shared; do not modify the result"""
    return _reference(c.name, c.b0 if b0 is None else b0, c.B if B is None else B)


# ---- the planted effect ---------------------------------------------------------------------------------------------------------------------------
PLANTED_SEED, PLANTED_B, PLANTED_R, PLANTED_F = 1, 199, 2, 4
PLANTED_PENALTIES = (0.1, 1.0, 10.0, 100.0)


def planted(seed=PLANTED_SEED, effect=2.5):
    """D = 96, P = 6 uniform features, hazard exp(effect * feature 2), exponential censoring, times rounded to 0.01 -> E, time, event"""
    rng = np.random.default_rng(seed)
    D = 96
    E = rng.random((D, 6))
    te = rng.exponential(size=D) / np.exp(effect * E[:, 2])
    tc = rng.exponential(size=D) * 0.5
    return E, np.round(np.minimum(te, tc), 2), (te <= tc).astype(np.uint8)
