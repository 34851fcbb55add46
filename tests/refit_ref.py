"""numpy restatements of mmm_refit_exposures (include/mmmusig.h) and the corpora its tests share.

`refit` follows the definition literally in float64, the order of every sum included: q_v and Σ_c w sequentially over c (np.cumsum adds
along an axis one element after the other), g_c and ll as 64 partial sums over l, l + 64, ... combined by the butterfly l ^ 32, ^ 16, ^ 8,
^ 4, ^ 2, ^ 1.  Only +, x, / and comparisons decide w, active, order, iters and unexplained, so a device that keeps the same order gives
the same bits; ll and cost contain a log and are compared against `ll_longdouble` on the same q.  Besides the outputs `refit` returns the
margin of every decision: per document and round the relative gap between the two smallest active weights and |Δ - penalty| / penalty
(penalty = 0: |Δ| / |ll(A)|).  The integer outputs of two implementations are comparable where these margins are far above rounding;
tests/test_refit_cpu.py asserts that for every corpus the GPU tests use."""
import functools
from collections import namedtuple

import numpy as np

_LANE = np.arange(64)

RefOut = namedtuple("RefOut", "w active order cost ll_doc unexplained iters q rounds gap_margin pen_margin")
RefOut.__doc__ = """w, active, order, cost [D, C]; ll_doc, unexplained, iters [D]; q [D, V]: the final mixture of every document; rounds: per
document the list of (q_A, q_B) of every round that ran (accepted or not); gap_margin, pen_margin: per document the list of margins."""


def normalise(cat):
    cat = np.asarray(cat, dtype=np.float64)
    return cat / np.cumsum(cat, axis=1)[:, -1][:, None]


def butterfly(p):
    """p [..., 64] -> [...]: the total every lane holds after l += l ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1"""
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[..., _LANE ^ off]
    return p[..., 0]


def partials(x):
    """x [..., V] (>= 0) -> [..., 64]: partial l = x[l] + x[l + 64] + ... in ascending order (padding adds +0: no bit changes)"""
    V = x.shape[-1]
    S = -(-V // 64)
    pad = np.zeros(x.shape[:-1] + (S * 64,), dtype=x.dtype)
    pad[..., :V] = x
    return np.cumsum(pad.reshape(x.shape[:-1] + (S, 64)), axis=-2)[..., -1, :]


def mixture(w, PA):
    return np.cumsum(w[:, None] * PA, axis=0)[-1]


def ll_float(n, q):
    m = (n > 0) & (q > 0)
    t = np.zeros_like(q)
    t[m] = n[m] * np.log(q[m])
    return float(butterfly(partials(t))), float(n[(n > 0) & ~(q > 0)].sum())


def ll_longdouble(n, q):
    """Σ n_v log q_v over n_v > 0, q_v > 0 in np.longdouble, and the bound (V + 2) 2^-52 Σ n_v |log q_v| a float64 evaluation may differ by:
    one rounding per addition, one for the product, less than 1 ulp for the log"""
    m = (n > 0) & (q > 0)
    t = n[m].astype(np.longdouble) * np.log(q[m].astype(np.longdouble))
    return t.sum(dtype=np.longdouble), float((q.size + 2) * 2.0 ** -52 * np.abs(t).sum(dtype=np.longdouble))


def fit(PA, n, f, maxiter, tol, trace=None):
    """fit(A) on the rows PA [k, V] of the normalised catalogue -> (w [k], ll, u, iterations, q)"""
    k = PA.shape[0]
    w = np.full(k, 1.0 / k)
    pos = n > 0
    it = 0
    while it < maxiter:
        it += 1
        q = mixture(w, PA)
        r = np.zeros_like(q)
        m = pos & (q > 0)
        r[m] = f[m] / q[m]
        g = butterfly(partials(r[None, :] * PA))
        wn = w * g
        md = np.abs(wn - w).max()
        w = wn
        if trace is not None:                            # ll of the normalised iterate
            trace.append(ll_float(n, mixture(w / np.cumsum(w)[-1], PA))[0])
        if md < tol:
            break
    S = np.cumsum(w)[-1]
    if S > 0:
        w = w / S
    q = mixture(w, PA)
    ll, u = ll_float(n, q)
    return w, ll, u, it, q


def refit(D, C, V, doc_ptr, term, count, cat, allowed=None, penalty=None, maxiter=1000, tol=1e-9):
    P = normalise(cat)
    same_row = lambda a, b: np.array_equal(P[a], P[b])
    W = np.zeros((D, C)); act = np.zeros((D, C), dtype=np.uint8); order = np.full((D, C), -1, dtype=np.int32); cost = np.zeros((D, C))
    ll_doc = np.zeros(D); unex = np.zeros(D); iters = np.zeros(D, dtype=np.int64); Q = np.zeros((D, V))
    rounds, gaps, pens = [], [], []
    for d in range(D):
        rounds.append([]); gaps.append([]); pens.append([])
        n = np.zeros(V)
        np.add.at(n, term[doc_ptr[d]:doc_ptr[d + 1]], count[doc_ptr[d]:doc_ptr[d + 1]].astype(np.float64))
        N = n.sum()
        A = np.flatnonzero(allowed[d]) if allowed is not None else np.arange(C)
        if N == 0 or A.size == 0:
            unex[d] = N
            continue
        f = n / N
        w, ll, u, it, q = fit(P[A], n, f, maxiter, tol)
        iters[d] += it
        j = 0
        while penalty is not None and A.size > 1:
            o = np.lexsort((np.arange(A.size), w))            # smallest weight first, ties to the lowest c
            i0, i1 = o[0], o[1]
            if w[i1] == w[i0]:
                gaps[d].append(np.inf if same_row(A[i0], A[i1]) else 0.0)        # a tie between identical rows is exact by symmetry
            else:
                gaps[d].append((w[i1] - w[i0]) / w[i1])
            B = np.delete(A, i0)
            wB, llB, uB, it, qB = fit(P[B], n, f, maxiter, tol)
            iters[d] += it
            rounds[d].append((q, qB))
            delta = ll - llB if uB == u else np.inf
            pen = float(penalty[d])
            pens[d].append(np.inf if not np.isfinite(delta) else (abs(delta - pen) / pen if pen > 0 else abs(delta) / abs(ll)))
            if not delta < pen:
                break
            order[d, j] = A[i0]; cost[d, j] = delta; j += 1
            A, w, ll, q = B, wB, llB, qB
        W[d, A] = w; act[d, A] = 1; ll_doc[d] = ll; unex[d] = u; Q[d] = q
    return RefOut(W, act, order, cost, ll_doc, unex, iters, Q, rounds, gaps, pens)


# ---- corpora ---------------------------------------------------------------------------------------------------------------------------------
Corpus = namedtuple("Corpus", "name D C V doc_ptr term count cat allowed penalty maxiter")

# (C, V): regular documents, maxiter -- the smallest shapes at which each piece of the kernel can go wrong: fewer terms than lanes, the tails of
# the 64 partial sums, more signatures than lanes (and than one 32-wide chunk), the limit C = 256, a catalogue beyond LDS
SHAPES = {(1, 1): (2, 30), (2, 5): (3, 40), (12, 96): (6, 40), (12, 97): (3, 60), (12, 130): (3, 60), (65, 96): (3, 40), (256, 96): (3, 50),
          (70, 1536): (4, 100), (3, 7001): (2, 30)}          # V = 7001: the per-wave count vectors no longer fit LDS either


def _csr(docs):
    dp = np.zeros(len(docs) + 1, dtype=np.int64)
    for i, (t, c) in enumerate(docs):
        dp[i + 1] = dp[i] + len(t)
    term = np.concatenate([np.asarray(t, dtype=np.int32) for t, _ in docs]) if docs else np.zeros(0, np.int32)
    count = np.concatenate([np.asarray(c, dtype=np.int32) for _, c in docs]) if docs else np.zeros(0, np.int32)
    return dp, term.astype(np.int32), count.astype(np.int32)


def _rows(rng, n):
    """a count vector as CSR rows with zero-count entries and duplicate terms, in shuffled order"""
    v = np.flatnonzero(n)
    t = list(v); c = list(n[v].astype(np.int64))
    if len(t):
        i = int(rng.integers(len(t)))
        if c[i] >= 2:                                   # a duplicate term: the count in two entries
            c.append(c[i] // 2); t.append(t[i]); c[i] -= c[i] // 2
        t.append(int(rng.integers(n.size))); c.append(0)      # a zero-count entry
    p = rng.permutation(len(t))
    return np.asarray(t, dtype=np.int32)[p], np.asarray(c, dtype=np.int32)[p]


def bic(doc_ptr, count):
    """0.5 log N_d, with N_d = 1 taken as 2: a penalty of exactly 0 would let the sign of a difference of two logs decide"""
    N = np.add.reduceat(np.concatenate([count, [0]]).astype(np.float64), doc_ptr[:-1])
    N[doc_ptr[:-1] == doc_ptr[1:]] = 0
    return np.where(N > 0, 0.5 * np.log(np.maximum(N, 2.0)), 0.0)


@functools.lru_cache(maxsize=None)
def corpus(C, V, seed=0):
    """regular documents (planted signatures among the allowed ones, multinomial counts), then: an empty document, a one-mutation document,
    an `allowed` row with one signature, an empty `allowed` row and -- where the shape has room for it (C, V >= 2) -- a document with a term
    that none of its allowed signatures produces and one for which removing a signature would raise `unexplained`"""
    ndocs, maxiter = SHAPES[(C, V)]
    rng = np.random.default_rng([C, V, seed])
    cat = rng.dirichlet(np.full(V, 0.3), size=C) * rng.uniform(0.5, 2.0, size=(C, 1)) if V > 1 else rng.uniform(0.5, 2.0, size=(C, 1))
    cat = np.maximum(cat, 1e-12 if V > 1 else 0)
    if C >= 2 and V >= 2:
        cat[:-1, V - 1] = 0.0                           # only the last signature produces the last term
    P = normalise(cat)
    docs, allowed = [], []
    for i in range(ndocs):
        al = np.ones(C, dtype=np.uint8)
        if C > 16 and (i > 0 or V > 1000):              # one document with the whole catalogue (V = 1536: 40 of it), the others with part of it
            al[:] = 0
            al[rng.choice(C, size=12 + 3 * i if i else 40, replace=False)] = 1
        k = min(int(al.sum()), 3 + (i % 2))
        planted = rng.choice(np.flatnonzero(al), size=k, replace=False)
        wt = rng.dirichlet(np.full(k, 2.0))
        n = rng.multinomial(int(rng.integers(800, 6000)), wt @ P[planted] / (wt @ P[planted]).sum())
        docs.append(_rows(rng, n)); allowed.append(al)
    one = np.ones(C, dtype=np.uint8)
    docs.append((np.zeros(0, np.int32), np.zeros(0, np.int32))); allowed.append(one)                        # empty document
    few = one.copy()
    if C > 16:
        few[:] = 0; few[rng.choice(C, size=2, replace=False)] = 1      # (more would underflow to equal zeros within maxiter)
    docs.append((np.asarray([int(rng.integers(max(V - 1, 1)))], np.int32), np.asarray([1], np.int32))); allowed.append(few)      # one mutation
    single = np.zeros(C, dtype=np.uint8); single[int(rng.integers(C))] = 1
    docs.append(_rows(rng, rng.multinomial(500, P[int(np.flatnonzero(single)[0])]))); allowed.append(single)   # one allowed signature
    docs.append(_rows(rng, rng.multinomial(300, P[0]))); allowed.append(np.zeros(C, dtype=np.uint8))         # empty allowed row
    if C >= 2 and V >= 2:
        n = rng.multinomial(700, 0.5 * (P[0] + P[C - 1]))
        n[V - 1] = max(n[V - 1], 5)
        no_last = one.copy(); no_last[C - 1] = 0
        if C > 16:
            no_last[rng.choice(C - 1, size=C - 9, replace=False)] = 0
        docs.append(_rows(rng, n)); allowed.append(no_last)                                                   # unexplained > 0
        with_last = no_last.copy(); with_last[C - 1] = 1
        docs.append(_rows(rng, n)); allowed.append(with_last)                                                 # removing the last one is refused
    dp, term, count = _csr(docs)
    return Corpus("C%dV%d" % (C, V), len(docs), C, V, dp, term, count, cat, np.stack(allowed), bic(dp, count), maxiter)


def take(c, docs):
    """the documents `docs` of a corpus as a corpus of their own"""
    rows = [(c.term[c.doc_ptr[d]:c.doc_ptr[d + 1]], c.count[c.doc_ptr[d]:c.doc_ptr[d + 1]]) for d in docs]
    dp, term, count = _csr(rows)
    return c._replace(D=len(docs), doc_ptr=dp, term=term, count=count, allowed=c.allowed[list(docs)], penalty=c.penalty[list(docs)])


@functools.lru_cache(maxsize=None)
def twin_corpus():
    """the (12, 96) corpus with catalogue row 5 = 2 x row 4: the two normalised rows are equal bit for bit, so are their weights in every
    fit that holds both, and the tie goes to the lower index"""
    c = corpus(12, 96)
    cat = c.cat.copy()
    cat[5] = 2.0 * cat[4]
    return c._replace(name="twin", cat=cat)


@functools.lru_cache(maxsize=None)
def cases():
    """every (corpus, tol) the GPU tests run against the restatement: every shape, all its documents, at tol = 0 and tol = 1e-9"""
    out = []
    for (C, V) in SHAPES:
        c = corpus(C, V)
        out.append((c, 0.0))
        out.append((c, 1e-9))
    out.append((twin_corpus(), 1e-9))
    return out


_REF = {}


def reference(c, tol):
    key = (c.name, c.D, tol)
    if key not in _REF:
        _REF[key] = refit(c.D, c.C, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, c.penalty, c.maxiter, tol)
    return _REF[key]


def planted(C, V, N, k, seed):
    """an identifiable input: Dirichlet(0.3) signatures, k planted with weights >= 0.15 -> (cat, CSR of one document, planted set)"""
    rng = np.random.default_rng([C, V, N, k, seed])
    cat = rng.dirichlet(np.full(V, 0.3), size=C)
    which = np.sort(rng.choice(C, size=k, replace=False))
    wt = 0.15 + (1 - 0.15 * k) * rng.dirichlet(np.full(k, 2.0))
    n = rng.multinomial(N, wt @ cat[which])
    v = np.flatnonzero(n)
    return cat, np.asarray([0, v.size], dtype=np.int64), v.astype(np.int32), n[v].astype(np.int32), which
