"""numpy restatement of mmm_exposure_trajectory (include/mmmusig.h) and the case table its tests share.

Built only from the restatements that already exist: `refit_ref.fit` / `normalise` / `ll_longdouble` for the fits and `compare_ref.deal_doc` /
`deal_members` for the dealing; the optimal partitioning is a plain-Python dynamic program.  It imports nothing from the product.  Besides
every output it returns, for each value that passes through a log, the np.longdouble value on the same mixtures with the project's bound
((V + 2) 2^-52 sum n_v |log q_v| per log-likelihood, summed over the log-likelihoods that enter), and the list of every comparison that
decides an integer output: (sample, kind, a, bound_a, provenance_a, b, bound_b, provenance_b).  The provenance of a value is the sequence of
count vectors whose log-likelihoods were added, in the order of the additions: two values of equal provenance are equal bit for bit in any
deterministic implementation (a replicate that deals the observed partition again; an empty bin between two cuts); every other comparison
is comparable across two implementations of log only where it is separated by far more than the bounds (tests/test_trajectory_cpu.py)."""
import functools
import itertools
from collections import namedtuple

import numpy as np

import compare_ref as CR
import refit_ref as R

MAX_BINS = 128

TCase = namedtuple("TCase", "name C V bins cat allowed L M penalty maxiter tol B seed stream")
TCase.__doc__ = """bins: per sample the list of its bins, each (term, count) arrays (0-based terms; duplicate terms, zero counts and any order are
allowed); allowed [D, C] uint8 or None; penalty [D]."""

Fit = namedtuple("Fit", "w ll u it ld bd key")


def csr(c):
    """-> (D, nbins, doc_ptr, term, count, bin_ptr)"""
    flat = [b for s in c.bins for b in s]
    dp, term, count = R._csr(flat)
    bin_ptr = np.concatenate([[0], np.cumsum([len(s) for s in c.bins])]).astype(np.int64)
    return len(c.bins), len(flat), dp, term, count, bin_ptr


def dense_bins(c, d):
    """[T, V] int64: the dense count vectors of the bins of sample d"""
    out = np.zeros((len(c.bins[d]), c.V), dtype=np.int64)
    for t, (tm, ct) in enumerate(c.bins[d]):
        np.add.at(out[t], np.asarray(tm, dtype=np.int64), np.asarray(ct, dtype=np.int64))
    return out


def fit_vector(PA, x, maxiter, tol):
    """fit(A) on the integer vector x; a vector without mutations: w = 0, ll = 0, no iteration"""
    key = x.tobytes()
    if int(x.sum()) == 0:
        return Fit(np.zeros(PA.shape[0]), 0.0, 0.0, 0, np.longdouble(0), 0.0, key)
    xf = x.astype(np.float64)
    w, ll, u, it, q = R.fit(PA, xf, xf / xf.sum(), maxiter, tol)
    ld, bd = R.ll_longdouble(xf, q)
    return Fit(w, ll, u, it, ld, bd, key)


def seg_index(T, i, j):
    return i * T - i * (i - 1) // 2 + (j - i - 1)


def defined(T, L, i, j):
    return j - i >= L or (i == 0 and j == T)


def _canon(p):
    return tuple(sorted(p)) if len(p) <= 2 else tuple(p)        # a + b = b + a bit for bit; longer sums depend on their order


def partition(tab, T, L, M, pen, bd=None, key=None, log=None, d=0):
    """Optimal partitioning on a sample's block `tab` of the segment table -> (best [M + 1], n_cp, cp [M]).  Plain Python floats: the C entry's
    arithmetic.  bd, key (blocks like tab) and log: the bounds and provenances, and the list the comparisons are appended to."""
    nan = float("nan")
    ll = lambda i, j: float(tab[seg_index(T, i, j)])
    Mx = min(M, max(T // L - 1, 0))
    F = [[nan] * (T + 1) for _ in range(Mx + 1)]
    arg = [[-1] * (T + 1) for _ in range(Mx + 1)]
    FB = [[0.0] * (T + 1) for _ in range(Mx + 1)]
    FK = [[()] * (T + 1) for _ in range(Mx + 1)]
    for j in range(1, T + 1):
        if defined(T, L, 0, j):
            F[0][j] = ll(0, j)
            if log is not None:
                FB[0][j] = bd[seg_index(T, 0, j)]; FK[0][j] = (key[seg_index(T, 0, j)],)
    cand = {}                                                  # (m, j) -> {i: (value, bound, provenance)}
    for m in range(1, Mx + 1):
        for j in range(T + 1):
            bi, bv = -1, nan
            for i in range(1, j):
                f = F[m - 1][i]
                if f != f or not defined(T, L, i, j):
                    continue
                v = f + ll(i, j)
                if log is not None:
                    s = seg_index(T, i, j)
                    cand.setdefault((m, j), {})[i] = (v, FB[m - 1][i] + bd[s], FK[m - 1][i] + (key[s],))
                if bi < 0 or v > bv:
                    bi, bv = i, v
            F[m][j], arg[m][j] = bv, bi
            if log is not None and bi >= 0:
                FB[m][j], FK[m][j] = cand[(m, j)][bi][1:]
    best = np.full(M + 1, np.nan)
    mb, vbest = 0, nan
    vals = {}
    for m in range(Mx + 1):
        f = F[m][T]
        best[m] = f
        if f != f:
            continue
        v = f - float(m) * float(pen)
        vals[m] = v
        if vbest != vbest or v > vbest:
            mb, vbest = m, v
    cp = np.full(M, -1, dtype=np.int32)
    j = T
    for m in range(mb, 0, -1):
        if log is not None:                                    # the winner of every state on the path against each of its rivals
            win = cand[(m, j)][arg[m][j]]
            log.extend((d, "cp", win[0], win[1], _canon(win[2]), v, b, _canon(k)) for i, (v, b, k) in cand[(m, j)].items() if i != arg[m][j])
        cp[m - 1] = arg[m][j]
        j = arg[m][j]
    if log is not None:
        log.extend((d, "n_cp", vals[mb], FB[mb][T], ("m", mb), v, FB[m][T], ("m", m)) for m, v in vals.items() if m != mb)
    return best, mb, cp


def brute_force(tab, T, L, M):
    """best [M + 1] over ALL partitions into m + 1 segments of at least L bins, each sum from the left"""
    best = np.full(M + 1, np.nan)
    for m in range(0, min(M, max(T // L - 1, 0)) + 1):
        for cuts in itertools.combinations(range(1, T), m):
            b = (0,) + cuts + (T,)
            if not all(defined(T, L, b[k], b[k + 1]) for k in range(m + 1)):
                continue
            v = float(tab[seg_index(T, b[0], b[1])])
            for k in range(1, m + 1):
                v = v + float(tab[seg_index(T, b[k], b[k + 1])])
            if best[m] != best[m] or v > best[m]:
                best[m] = v
    return best


Out = namedtuple("Out", "seg_ll seg_ld seg_bd best n_cp cp w_seg w_bin gain_cut gain_ld gain_bd cut stat stat_ld stat_bd count_ge count_cut status unexplained iters "
                 "rep rep_ld rep_bd prefixes checks n_allowed seg0 bin_ptr C_t")
Out.__doc__ = """Every output of the C entry in its layout; *_ld / *_bd: the longdouble value and the bound of seg_ll, gain_cut, stat and rep; prefixes:
{(d, b): [T + 1, V]} the replicate's prefix vectors c^{t,b} for the cuts (rows of other t are -1); checks: the comparisons (module docstring);
n_allowed [D] = |A|; seg0 [D + 1]: the blocks of the table; C_t: per sample the totals of the prefixes."""


_OBS = {}


def _observed(c):
    """the table of every sample: {d: (cpre [T + 1, V], A, {(i, j): Fit})}; kept per case, whatever B and key_bits"""
    k = (c.name, c.L, c.maxiter, c.tol, len(c.bins))
    if k not in _OBS:
        _OBS[k] = _observe(c)
    return _OBS[k]


def _observe(c):
    P = R.normalise(c.cat)
    out = {}
    for d in range(len(c.bins)):
        nb = dense_bins(c, d)
        T = nb.shape[0]
        cpre = np.concatenate([np.zeros((1, c.V), np.int64), np.cumsum(nb, axis=0)]) if T else np.zeros((1, c.V), np.int64)
        A = np.flatnonzero(c.allowed[d]) if c.allowed is not None else np.arange(c.C)
        fits = {}
        if T and cpre[T].sum() > 0 and A.size:
            memo = {}
            for i in range(T):
                for j in range(i + 1, T + 1):
                    if defined(T, c.L, i, j):
                        x = cpre[j] - cpre[i]
                        k = x.tobytes()
                        if k not in memo:                      # equal vectors give equal fits: the count of fits is kept by the caller
                            memo[k] = fit_vector(P[A], x, c.maxiter, c.tol)
                        fits[(i, j)] = memo[k]
            for t in range(T):
                x = nb[t]
                k = x.tobytes()
                if k not in memo:
                    memo[k] = fit_vector(P[A], x, c.maxiter, c.tol)
                fits[("bin", t)] = memo[k]
        out[d] = (cpre, A, fits)
    return out


def trajectory(c, B=None, b0=0, key_bits=32):
    B = c.B if B is None else B
    P = R.normalise(c.cat)
    D, C, V, L, M = len(c.bins), c.C, c.V, c.L, c.M
    Ts = [len(s) for s in c.bins]
    bin_ptr = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    seg0 = np.concatenate([[0], np.cumsum([T * (T + 1) // 2 for T in Ts])]).astype(np.int64)
    nb, S = int(bin_ptr[-1]), int(seg0[-1])
    nan = np.nan
    o = Out(np.full(S, nan), np.full(S, nan, dtype=np.longdouble), np.zeros(S), np.full((D, M + 1), nan), np.zeros(D, np.int32), np.full((D, M), -1, np.int32),
            np.zeros((D, M + 1, C)), np.zeros((nb, C)), np.full(nb, nan), np.full(nb, nan, dtype=np.longdouble), np.zeros(nb), np.full(D, -1, np.int32), np.zeros(D),
            np.zeros(D), np.zeros(D), np.zeros(D, np.int32), np.zeros(nb, np.int32), np.zeros(D, np.int8), np.zeros(D), np.zeros(D, np.int64),
            np.full((B, D), nan), np.full((B, D), nan), np.zeros((B, D)), {}, [], np.zeros(D, np.int64), seg0, bin_ptr, {})
    obs = _observed(c)
    for d in range(D):
        T = Ts[d]
        cpre, A, fits = obs[d]
        o.n_allowed[d] = A.size
        o.C_t[d] = cpre.sum(axis=1)
        if not fits:
            o.status[d] = 3
            continue
        blk = slice(int(seg0[d]), int(seg0[d + 1]))
        keys = [None] * (T * (T + 1) // 2)
        for (i, j), f in fits.items():
            if i == "bin":
                o.w_bin[bin_ptr[d] + j, A] = f.w
                continue
            s = int(seg0[d]) + seg_index(T, i, j)
            o.seg_ll[s], o.seg_ld[s], o.seg_bd[s] = f.ll, f.ld, f.bd
            keys[seg_index(T, i, j)] = f.key
            o.iters[d] += f.it
        o.unexplained[d] = fits[(0, T)].u
        best, ncp, cp = partition(o.seg_ll[blk], T, L, M, c.penalty[d], o.seg_bd[blk], keys, o.checks, d)
        o.best[d], o.n_cp[d], o.cp[d] = best, ncp, cp
        bounds = [0] + [int(t) for t in cp[:ncp]] + [T]
        for k in range(ncp + 1):
            o.w_seg[d, k, A] = fits[(bounds[k], bounds[k + 1])].w
        if T < 2 * L:
            o.status[d] = 1
            continue
        f0 = fits[(0, T)]
        cuts = list(range(L, T - L + 1))
        G, Gld, Gbd, Gkey = {}, {}, {}, {}
        gmax, tb = nan, -1
        for t in cuts:
            fa, fb = fits[(0, t)], fits[(t, T)]
            G[t], Gld[t], Gbd[t], Gkey[t] = fa.ll + fb.ll, fa.ld + fb.ld, fa.bd + fb.bd, _canon((fa.key, fb.key))
            o.gain_cut[bin_ptr[d] + t] = G[t] - f0.ll
            o.gain_ld[bin_ptr[d] + t] = Gld[t] - f0.ld
            o.gain_bd[bin_ptr[d] + t] = Gbd[t] + f0.bd
            if tb < 0 or G[t] > gmax:
                gmax, tb = G[t], t
        o.cut[d] = tb
        o.checks.extend((d, "cut", gmax, Gbd[tb], Gkey[tb], G[t], Gbd[t], Gkey[t]) for t in cuts if t != tb)
        o.stat[d] = max(2.0 * (gmax - f0.ll), 0.0)
        o.stat_ld[d] = max(float(2 * (max(Gld.values()) - f0.ld)), 0.0)
        o.stat_bd[d] = 2.0 * (max(Gbd.values()) + f0.bd)
        if B == 0:
            continue
        n = cpre[T]
        N = int(n.sum())
        gb = b0 + np.arange(B)
        dealt = {t: (CR.deal_doc(n, int(o.C_t[d][t]), d, gb, c.seed, c.stream, key_bits) if o.C_t[d][t] else np.zeros((B, V), np.int64)) for t in cuts}
        memo = {}
        for b in range(B):
            pre = np.full((T + 1, V), -1, dtype=np.int64)
            vals = []
            for t in cuts:
                x = dealt[t][b]
                pre[t] = x
                pair = []
                for z in (x, n - x):
                    k = z.tobytes()
                    if k not in memo:
                        memo[k] = fit_vector(P[A], z, c.maxiter, c.tol)
                    pair.append(memo[k])
                    o.iters[d] += memo[k].it
                fa, fb = pair
                vals.append((fa.ll + fb.ll, fa.ld + fb.ld, fa.bd + fb.bd, _canon((fa.key, fb.key))))
            o.prefixes[(d, b)] = pre
            # the maximum: in any implementation its value is within the largest bound of its operands, and it is at least every operand
            gm = max(v[0] for v in vals)
            gm_bd = max(v[2] for v in vals)
            gm_keys = {v[3] for v in vals}
            o.rep[b, d] = 2.0 * (gm - f0.ll)
            o.rep_ld[b, d] = float(2 * (max(v[1] for v in vals) - f0.ld))
            o.rep_bd[b, d] = 2.0 * (gm_bd + f0.bd)
            o.count_ge[d] += gm >= gmax
            o.checks.append((d, "count_ge", gm, gm_bd, gm_keys, gmax, Gbd[tb], Gkey[tb]))
            for t in cuts:
                o.count_cut[bin_ptr[d] + t] += gm >= G[t]
                o.checks.append((d, "count_cut", gm, gm_bd, gm_keys, G[t], Gbd[t], Gkey[t]))
    return o


def decided(chk):
    """is the comparison the same in every implementation: equal provenance (for a replicate's maximum: one of its operands IS the observed
    value bit for bit, so the maximum is at least that), or apart by more than 10^3 times the two bounds"""
    _, kind, a, ba, ka, b, bb, kb = chk
    if (kb in ka) if isinstance(ka, set) else (ka == kb):
        return True
    return abs(a - b) > 1e3 * (ba + bb)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
def _ordered(n):
    v = np.flatnonzero(n)
    return v.astype(np.int32), n[v].astype(np.int32)


_EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def _cat(rng, C, V, private_last=True):
    cat = np.maximum(rng.dirichlet(np.full(V, 0.3 if V > 5 else 1.0), size=C) * rng.uniform(0.5, 2.0, size=(C, 1)), 1e-12) if V > 1 else rng.uniform(0.5, 2.0, size=(C, 1))
    if C >= 2 and V >= 2 and private_last:
        cat[:-1, V - 1] = 0.0                           # only the last signature produces the last term
    return cat


def _sample(rng, P, al, sizes, plant=(), shuffled=True):
    """a timeline: bin t holds sizes[t] mutations of a mixture of up to three allowed signatures; plant: the bins a new segment (another mixture)
    starts with"""
    on = np.flatnonzero(al)
    bins = []
    p = None
    for t, N in enumerate(sizes):
        if p is None or t in plant:
            rows = rng.choice(on, size=min(on.size, 2), replace=False)
            wt = rng.dirichlet(np.full(rows.size, 1.0))
            p = wt @ P[rows]; p = p / p.sum()
        n = rng.multinomial(N, p) if N else np.zeros(P.shape[1], np.int64)
        bins.append(_EMPTY if N == 0 else (R._rows(rng, n) if shuffled and t % 2 else _ordered(n)))
    return bins


def _bic(al, sizes):
    return 0.5 * (float(np.count_nonzero(al)) + 1.0) * np.log(max(float(sum(sizes)), 2.0))


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng([sum(map(ord, name)), 424])
    B, maxiter, tol, M = 24, 40, 1e-9, 3
    if name == "V1":                  # one term, one signature: the |A| = 1 sample of the table
        C, V, L = 1, 1, 1
        cat = _cat(rng, C, V)
        al = [np.ones(C, np.uint8)]
        sizes = [[5, 0, 9]]
        bins = [[(np.zeros(1, np.int32), np.asarray([N], np.int32)) if N else _EMPTY for N in sizes[0]]]
    elif name == "V7":                # allowed = NULL, |A| = 2; T = 1, 2, 3, 5, 17 in one call; empty first, middle and last bins; all in one bin; N = 0
        C, V, L = 2, 7, 1
        cat = _cat(rng, C, V, private_last=False)
        P = R.normalise(cat)
        one = np.ones(C, np.uint8)
        sizes = [[40], [30, 50], [0, 0, 90], [0, 60, 0, 80, 0], [25] * 17, [0, 0, 0], [2]]
        plants = [(), (1,), (), (3,), (6, 12), (), ()]
        al = None
        bins = [_sample(rng, P, one, s, p) for s, p in zip(sizes, plants)]
    elif name == "V64":               # |A| = 5, 2, 0; L = 2 with T < 2 L; a term no allowed signature produces
        C, V, L = 5, 64, 2
        cat = _cat(rng, C, V)
        P = R.normalise(cat)
        one = np.ones(C, np.uint8)
        two = np.zeros(C, np.uint8); two[[0, 3]] = 1
        no_last = one.copy(); no_last[C - 1] = 0
        al = [one, one, two, one, np.zeros(C, np.uint8), no_last]
        sizes = [[50, 60, 70], [40] * 5, [30] * 17, [80, 90], [20, 20, 20, 20], [60, 50, 70, 40, 80]]
        plants = [(), (2,), (5, 11), (), (), (3,)]
        bins = [_sample(rng, P, a if a.any() else one, s, p) for a, s, p in zip(al, sizes, plants)]
        t, n = bins[5][1]
        bins[5][1] = (np.concatenate([t, [V - 1]]).astype(np.int32), np.concatenate([n, [4]]).astype(np.int32))     # unexplained > 0
        al = np.stack(al)
    elif name == "V65":               # |A| = 33 (allowed = NULL), L = 3; a bin over 1024 mutations; two planted changes
        C, V, L = 33, 65, 3
        cat = _cat(rng, C, V)
        P = R.normalise(cat)
        one = np.ones(C, np.uint8)
        sizes = [[40] * 5, [150] * 17, [1100, 90, 80, 70, 60, 50]]
        plants = [(), (6, 12), (3,)]
        al = None
        bins = [_sample(rng, P, one, s, p) for s, p in zip(sizes, plants)]
    elif name == "V129":              # |A| = 70 and |A| = 1
        C, V, L = 70, 129, 1
        cat = _cat(rng, C, V)
        P = R.normalise(cat)
        one = np.ones(C, np.uint8)
        single = np.zeros(C, np.uint8); single[7] = 1
        al = np.stack([one, single])
        sizes = [[400, 500], [60, 70, 50, 40, 80]]
        bins = [_sample(rng, P, one, sizes[0], (1,)), _sample(rng, P, single, sizes[1])]
    elif name == "V200":
        C, V, L = 5, 200, 2
        cat = _cat(rng, C, V)
        P = R.normalise(cat)
        one = np.ones(C, np.uint8)
        al = np.stack([one, one])
        sizes = [[60] * 17, [90, 80, 70, 100]]
        bins = [_sample(rng, P, one, sizes[0], (8,)), _sample(rng, P, one, sizes[1], (2,))]
    elif name == "V4096":             # a dozen non-zero terms
        C, V, L = 2, 4096, 1
        hot = np.sort(rng.choice(V, size=12, replace=False))
        cat = np.zeros((C, V)); cat[:, hot] = rng.dirichlet(np.full(12, 0.5), size=C)
        P = R.normalise(cat)
        one = np.ones(C, np.uint8)
        al = None
        sizes = [[70, 60, 80]]
        bins = [_sample(rng, P, one, sizes[0], (2,))]
    elif name == "T128":              # 8,256 segments
        C, V, L, M, B, maxiter = 3, 7, 1, 2, 2, 50
        cat = _cat(rng, C, V, private_last=False)
        P = R.normalise(cat)
        one = np.ones(C, np.uint8)
        al = None
        sizes = [list(rng.integers(1, 4, size=128))]
        bins = [_sample(rng, P, one, sizes[0], (64,), shuffled=False)]
    else:
        raise KeyError(name)
    D = len(bins)
    al = None if al is None else np.stack(list(al))
    pen =np.array([_bic(np.ones(C) if al is None else al[d], sizes[d]) for d in range(D)])
    return TCase(name, C, V, tuple(tuple(s) for s in bins), cat, al, L, M, pen, maxiter, tol, B, 4240 + C, V % 5)


SHAPES = ("V1", "V7", "V64", "V65", "V129", "V200", "V4096", "T128")
KEY_BITS = (32, 3)             # the contract's, and the hook that puts ties at the threshold in essentially every replicate
RUNS = tuple((n, k) for n in SHAPES for k in KEY_BITS if n != "T128" or k == 32)         # the 8,256-segment case has B = 2: once
_REF = {}


def reference(name, key_bits=32):
    if (name, key_bits) not in _REF:
        _REF[(name, key_bits)] = trajectory(case(name), key_bits=key_bits)
    return _REF[(name, key_bits)]
