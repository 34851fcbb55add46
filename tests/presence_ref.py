"""numpy restatement of mmm_presence_test (include/mmmusig.h) and the corpora its tests share.

Built only from the restatements that already exist: `refit_ref.fit` / `normalise` / `partials` / `butterfly` / `ll_longdouble` for the two
fits and the score, `simulate_ref.mixture` / `thresholds` / `simulate_doc` for the replicates.  It shares nothing with the kernel.  Per item
and per replicate it returns the statistic Λ, its longdouble value on the same mixtures with the rounding bound 2 (bound(ll0) + bound(ll1)),
the branch taken (did fit(A1) run?), the score s and the raw difference 2 (ll1 - ll0) before the clamp at 0 -- the margins that make the
integer outputs of two implementations comparable (tests/test_presence_cpu.py asserts them for every corpus the GPU tests use)."""
import functools
from collections import namedtuple

import numpy as np

import refit_ref as R
import simulate_ref as S

Stat = namedtuple("Stat", "lam lam_ld bound s alt raw w0 w1t iters")
Stat.__doc__ = """lam: Λ; lam_ld, bound: its longdouble value on the same q and 2 (bound(ll0) + bound(ll1)) (0, 0 where fit(A1) did not run; lam_ld
= +inf with Λ); s: the score; alt: fit(A1) ran; raw: 2 (ll1 - ll0) in float64 (NaN where it did not run); w0: [|A0|] null weights; w1t: the
target's weight under A1 (0 where not fitted); iters: EM iterations of the fits that ran."""


def statistic(P, A0, A1, t, n, maxiter, tol, always_alt=False):
    """the statistic of the count vector n [V] for the sets A0, A1 (ascending catalogue rows) and the target t.  always_alt: run fit(A1) where
    the definition skips it too and report its raw difference and weight (lam, alt and iters stay those of the definition)."""
    n = np.asarray(n, dtype=np.float64)
    N = n.sum()
    f = n / N
    w0, ll0, u0, it0, q0 = R.fit(P[A0], n, f, maxiter, tol)
    r = np.zeros_like(q0)
    m = (n > 0) & (q0 > 0)
    r[m] = f[m] / q0[m]
    s = float(R.butterfly(R.partials(r * P[t])))
    alt = bool(u0 > 0 or s > 1)
    if not (alt or always_alt):
        return Stat(0.0, 0.0, 0.0, s, False, np.nan, w0, 0.0, it0)
    w1, ll1, u1, it1, q1 = R.fit(P[A1], n, f, maxiter, tol)
    raw = 2.0 * (ll1 - ll0)
    w1t = float(w1[list(A1).index(t)])
    if not alt:
        return Stat(0.0, 0.0, 0.0, s, False, raw, w0, w1t, it0)
    if u0 > 0 and u1 < u0:
        return Stat(np.inf, np.inf, 0.0, s, True, np.inf, w0, w1t, it0 + it1)
    (L0, b0), (L1, b1) = R.ll_longdouble(n, q0), R.ll_longdouble(n, q1)
    return Stat(max(raw, 0.0), max(float(2 * (L1 - L0)), 0.0), 2.0 * (b0 + b1), s, True, raw, w0, w1t, it0 + it1)


PCorpus = namedtuple("PCorpus", "name D C V doc_ptr term count cat allowed targets maxiter tol B seed stream")

RefOut = namedtuple("RefOut", "w_null stat stat_ld bound score w_alt status count_ge count_zero iters obs_raw rep rep_ld rep_bound rep_alt rep_s rep_raw rep_w1t N")
RefOut.__doc__ = """item-major, j = t_idx D + d: w_null [TD, C]; stat, stat_ld, bound, score, w_alt, obs_raw [TD]; status int8, count_ge, count_zero
int32, iters int64 [TD]; rep, rep_ld, rep_bound, rep_s, rep_raw, rep_w1t [B, TD] (NaN for items without replicates), rep_alt [B, TD] bool;
N [D]."""


def dense(c, d):
    n = np.zeros(c.V)
    np.add.at(n, c.term[c.doc_ptr[d]:c.doc_ptr[d + 1]], c.count[c.doc_ptr[d]:c.doc_ptr[d + 1]].astype(np.float64))
    return n


def sets(c, j):
    """-> (d, t, A0, A1) of item j"""
    d, t = j % c.D, int(c.targets[j // c.D])
    al = np.ones(c.C, dtype=bool) if c.allowed is None else c.allowed[d] != 0
    a1 = al.copy(); a1[t] = True
    a0 = al.copy(); a0[t] = False
    return d, t, np.flatnonzero(a0), np.flatnonzero(a1)


def presence(c, B=None, b0=0, always_alt=False):
    B = c.B if B is None else B
    P = R.normalise(c.cat)
    T = len(c.targets)
    TD = T * c.D
    o = RefOut(np.zeros((TD, c.C)), np.zeros(TD), np.zeros(TD), np.zeros(TD), np.zeros(TD), np.zeros(TD), np.zeros(TD, np.int8), np.zeros(TD, np.int32),
               np.zeros(TD, np.int32), np.zeros(TD, np.int64), np.full(TD, np.nan), *[np.full((B, TD), np.nan) for _ in range(3)], np.zeros((B, TD), bool),
               *[np.full((B, TD), np.nan) for _ in range(3)], np.zeros(c.D, np.int64))
    for j in range(TD):
        d, t, A0, A1 = sets(c, j)
        n = dense(c, d)
        N = int(n.sum())
        o.N[d] = N
        if N == 0 or A0.size == 0:
            o.status[j] = 3
            continue
        st = statistic(P, A0, A1, t, n, c.maxiter, c.tol)
        o.w_null[j, A0] = st.w0
        o.stat[j], o.stat_ld[j], o.bound[j], o.score[j], o.w_alt[j], o.iters[j], o.obs_raw[j] = st.lam, st.lam_ld, st.bound, st.s, st.w1t, st.iters, st.raw
        o.status[j] = 1 if st.lam == 0 else (2 if np.isinf(st.lam) else 0)
        if o.status[j] == 1:
            o.count_ge[j] = B
        if o.status[j] != 0 or B == 0:
            continue
        _, Tv, _ = S.thresholds(S.mixture(o.w_null[j], P))
        draws = S.simulate_doc(Tv, N, j, b0 + np.arange(B), c.seed, c.stream)
        for b in range(B):
            rs = statistic(P, A0, A1, t, draws[b], c.maxiter, c.tol, always_alt)
            o.rep[b, j], o.rep_ld[b, j], o.rep_bound[b, j], o.rep_alt[b, j], o.rep_s[b, j], o.rep_raw[b, j], o.rep_w1t[b, j] = (
                rs.lam, rs.lam_ld, rs.bound, rs.alt, rs.s, rs.raw, rs.w1t)
            o.iters[j] += rs.iters
        o.count_ge[j] = int((o.rep[:, j] >= st.lam).sum())
        o.count_zero[j] = int((o.rep[:, j] == 0).sum())
    return o


# ---- corpora -----------------------------------------------------------------------------------------------------------------------------------
# (C, V): sizes of the documents' allowed sets, replicates -- the smallest shapes at which each mechanism can go wrong: fewer terms than lanes;
# the workload's shape (second slot of 64 terms half empty); more than one 32-wide reduction chunk and every width 4 / 8 / 16 / 32 of it; four
# slots with a ragged last one; a long threshold search whose rows fit LDS only for the small sets
SHAPES = {(4, 5): ((3, 2, 4), 24), (12, 96): ((5, 3, 8), 24), (40, 96): ((40, 3, 7, 13, 20), 12), (8, 200): ((4, 6), 24), (6, 1536): ((1, 3, 5), 12)}
SEEDS = {(4, 5): 0, (12, 96): 0, (40, 96): 0, (8, 200): 0, (6, 1536): 0}


@functools.lru_cache(maxsize=None)
def corpus(C, V):
    """one document per entry of the shape's sizes: `size` allowed signatures of which up to 3 are planted; two targets, the first planted in
    the first document (present), the second wherever the draw puts it"""
    sizes, B = SHAPES[(C, V)]
    rng = np.random.default_rng([C, V, SEEDS[(C, V)], 415])
    cat = np.maximum(rng.dirichlet(np.full(V, 0.3 if V > 5 else 1.0), size=C) * rng.uniform(0.5, 2.0, size=(C, 1)), 1e-12)
    P = R.normalise(cat)
    targets = np.sort(rng.choice(C, size=2, replace=False)).astype(np.int32)
    docs, allowed = [], []
    for i, size in enumerate(sizes):
        al = np.zeros(C, dtype=np.uint8)
        al[rng.choice(C, size=size, replace=False)] = 1
        if i == 0:
            al[targets[0]] = 1
        on = np.flatnonzero(al)
        k = min(on.size, 3)
        planted = rng.choice(on, size=k, replace=False)
        if i == 0 and targets[0] not in planted:
            planted[0] = targets[0]
        wt = rng.dirichlet(np.full(k, 2.0))
        p = wt @ P[planted]
        n = rng.multinomial(int(rng.integers(300, 3000)), p / p.sum())
        docs.append(R._rows(rng, n)); allowed.append(al)
    dp, term, count = R._csr(docs)
    return PCorpus("C%dV%d" % (C, V), len(docs), C, V, dp, term, count, cat, np.stack(allowed), targets, 150, 1e-9, B, 20260 + C, V % 7)


EDGE_SEED = 0


@functools.lru_cache(maxsize=None)
def edge_corpus():
    """C = 6, V = 40.  Only signature 5 produces the last term; signature 2 produces the first five terms only and no document allows it.
    Targets (5, 1, 2).  Documents: 0 regular (all but 2 allowed); 1 empty; 2 one mutation; 3 with target 5 outside its allowed set; 4 allowing
    signature 5 alone (A0 empty for target 5); 5 with a mutation in the last term and 5 allowed (target 5: +inf; target 1: plain); 6 the
    same counts with 5 NOT allowed (targets 1 and 2: the null leaves the last term unexplained and so does the alternative); 7 with no
    mutation in the first five terms (target 2 cannot improve it: score 0)."""
    C, V = 6, 40
    rng = np.random.default_rng([EDGE_SEED, 416])
    cat = np.maximum(rng.dirichlet(np.full(V, 0.4), size=C), 1e-9)
    cat[:-1, V - 1] = 0.0
    cat[2, 5:] = 0.0
    P = R.normalise(cat)
    base = np.array([1, 1, 0, 1, 1, 1], dtype=np.uint8)
    docs, allowed = [], []

    def draw(N, rows, w):
        p = np.asarray(w) @ P[rows]
        return rng.multinomial(N, p / p.sum())

    docs.append(R._rows(rng, draw(1500, [0, 1, 5], [0.5, 0.3, 0.2]))); allowed.append(base)
    docs.append((np.zeros(0, np.int32), np.zeros(0, np.int32))); allowed.append(base)
    docs.append((np.asarray([7], np.int32), np.asarray([1], np.int32))); allowed.append(base)
    no5 = base.copy(); no5[5] = 0
    docs.append(R._rows(rng, draw(900, [0, 3, 5], [0.5, 0.3, 0.2]) * (np.arange(V) < V - 1))); allowed.append(no5)
    only5 = np.zeros(C, dtype=np.uint8); only5[5] = 1
    docs.append(R._rows(rng, draw(400, [5], [1.0]))); allowed.append(only5)
    n = draw(800, [0, 4, 5], [0.4, 0.3, 0.3]); n[V - 1] = max(n[V - 1], 4)
    docs.append(R._rows(rng, n)); allowed.append(base)
    docs.append(R._rows(rng, n)); allowed.append(no5)
    n = draw(1000, [0, 1], [0.6, 0.4]); n[:5] = 0
    docs.append(R._rows(rng, n)); allowed.append(base)
    dp, term, count = R._csr(docs)
    return PCorpus("edge", len(docs), C, V, dp, term, count, cat, np.stack(allowed), np.asarray([5, 1, 2], dtype=np.int32), 150, 1e-9, 16, 77, 3)


@functools.lru_cache(maxsize=None)
def corpora():
    """every corpus the GPU tests run against the restatement"""
    return [corpus(C, V) for (C, V) in SHAPES] + [edge_corpus()]


_REF = {}


def reference(c):
    if c.name not in _REF:
        _REF[c.name] = presence(c)
    return _REF[c.name]


def planted_corpus(seed=3, C=4, V=24, n_with=4, n_without=40, N=2000, share=0.1):
    """C Dirichlet(0.3) signatures over V terms, target 0.  n_with samples hold the target with weight `share`, n_without are drawn from the
    other signatures alone; every sample allows the whole catalogue.  -> (PCorpus, with [D] bool)"""
    rng = np.random.default_rng([seed, 417])
    cat = rng.dirichlet(np.full(V, 0.3), size=C)
    D = n_with + n_without
    docs = []
    for d in range(D):
        w = rng.dirichlet(np.full(C - 1, 2.0))
        p = (1 - share) * (w @ cat[1:]) + share * cat[0] if d < n_with else w @ cat[1:]
        n = rng.multinomial(N, p / p.sum())
        v = np.flatnonzero(n)
        docs.append((v.astype(np.int32), n[v].astype(np.int32)))
    dp, term, count = R._csr(docs)
    return PCorpus("planted", D, C, V, dp, term, count, cat, None, np.asarray([0], dtype=np.int32), 300, 1e-9, 15, 5, 0), np.arange(D) < n_with
