"""numpy restatement of mmm_attribute_mutations (include/mmmusig.h) and the corpora its tests share.

`attribute` follows the definition literally in float64: fit(A) is `refit_ref.fit` (the order of every sum included), the replicate is
`bootstrap_ref.resample_doc` counted by term, the mixture q_v is the sequential sum over c ascending, the posterior one product and one
division, x = floor(ρ 2^24) an exact integer.  No log is involved, so a device that keeps the same order gives the same bits and the same
integers; every comparison of the GPU tests is exact.

The corpora reuse `refit_ref.SHAPES` (the smallest shapes at which the pieces of the fit can go wrong) up to the entry's limit V <= 4096,
plus one corpus at V = 4096 itself; 3-6 documents each, maxiter <= 100, B <= 8."""
import functools
from collections import namedtuple

import numpy as np

import bootstrap_ref as BR
import refit_ref as R

FX_ONE = 1 << 24

Case = namedtuple("Case", "name D C V doc_ptr term count cat allowed q_ptr q_term q_mult q_group G B seed stream maxiter tol")
Out = namedtuple("Out", "w post status iters sum_fx sumsq_fx top_count void_count group_fx rep_post")


def dense(c, d):
    n = np.zeros(c.V)
    sl = slice(c.doc_ptr[d], c.doc_ptr[d + 1])
    np.add.at(n, c.term[sl], c.count[sl].astype(np.float64))
    return n


def posterior(w, PA, q, terms):
    """rows [nq, k]: (w_c P[c][v]) / q_v where q_v > 0, else 0"""
    num = (w[:, None] * PA[:, terms]).T
    qv = q[terms][:, None]
    out = np.zeros_like(num)
    np.divide(num, qv, out=out, where=qv > 0)
    return out


def attribute(c, B=None, b0=0):
    """the outputs of mmm_attribute_mutations for the case c (replicates b0 .. b0 + B - 1)"""
    B = c.B if B is None else B
    D, C, V, G = c.D, c.C, c.V, c.G
    Q = int(c.q_ptr[-1])
    P = R.normalise(c.cat)
    o = Out(np.zeros((D, C)), np.zeros((Q, C)), np.zeros(D, np.int8), np.zeros(D, np.int64), np.zeros((Q, C), np.uint64), np.zeros((Q, C), np.uint64),
            np.zeros((Q, C), np.int32), np.zeros(Q, np.int32), np.zeros((B, G, C), np.uint64), np.zeros((B, Q, C)))
    mult = c.q_mult if c.q_mult is not None else np.ones(Q, np.int32)
    for d in range(D):
        qs = slice(c.q_ptr[d], c.q_ptr[d + 1])
        if qs.start == qs.stop:
            o.status[d] = 4
            continue
        n = dense(c, d)
        N = n.sum()
        A = np.flatnonzero(c.allowed[d]) if c.allowed is not None else np.arange(C)
        if N == 0 or A.size == 0:
            o.status[d] = 3
            continue
        terms = c.q_term[qs]
        w, _, _, it, q = R.fit(P[A], n, n / N, c.maxiter, c.tol)
        o.w[d, A] = w
        o.iters[d] += it
        e_all = np.arange(qs.start, qs.stop)
        o.post[np.ix_(e_all, A)] = posterior(w, P[A], q, terms)
        es = slice(c.doc_ptr[d], c.doc_ptr[d + 1])
        for b in range(B):
            nb = np.zeros(V)
            np.add.at(nb, c.term[es], BR.resample_doc(c.count[es], d, b0 + b, c.seed, c.stream).astype(np.float64))
            assert nb.sum() == N
            wb, _, _, it, qb = R.fit(P[A], nb, nb / N, c.maxiter, c.tol)
            o.iters[d] += it
            rho = posterior(wb, P[A], qb, terms)
            x = np.floor(rho * FX_ONE).astype(np.uint64)
            assert (x <= FX_ONE).all() and (rho * FX_ONE == np.ldexp(rho, 24)).all()
            o.rep_post[b][np.ix_(e_all, A)] = rho
            o.sum_fx[np.ix_(e_all, A)] += x
            o.sumsq_fx[np.ix_(e_all, A)] += x * x
            void = ~(qb[terms] > 0)
            o.void_count[qs] += void
            top = A[np.argmax(rho, axis=1)]                      # the first largest: ties go to the lowest c
            np.add.at(o.top_count, (e_all[~void], top[~void]), 1)
            if c.q_group is not None and G:
                g = c.q_group[qs]
                m = g >= 0
                gx = np.zeros((G, C), np.uint64)
                full = np.zeros((terms.size, C), np.uint64)
                full[:, A] = x * mult[qs].astype(np.uint64)[:, None]
                np.add.at(gx, g[m], full[m])
                o.group_fx[b] += gx
    return o


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [s for s in R.SHAPES if s[1] <= 4096] + [(3, 4096)]
B, SEED, STREAM, G = 5, 0x1234567890ABCDEF, 3, 3


def _v4096():
    """V = 4096, the limit: three signatures, three documents (rows of well under 4096 entries)"""
    C, V = 3, 4096
    rng = np.random.default_rng([C, V])
    cat = np.maximum(rng.dirichlet(np.full(V, 0.3), size=C), 1e-12)
    P = R.normalise(cat)
    docs, allowed = [], []
    for i in range(3):
        wt = rng.dirichlet(np.full(C, 2.0))
        docs.append(R._rows(rng, rng.multinomial(1500 + 500 * i, wt @ P / (wt @ P).sum())))
        al = np.ones(C, np.uint8)
        if i == 2:
            al[1] = 0
        allowed.append(al)
    dp, term, count = R._csr(docs)
    return R.Corpus("C3V4096", 3, C, V, dp, term, count, cat, np.stack(allowed), R.bic(dp, count), 30)


def _documents(C, V):
    """3-6 documents of the refit corpus: two regular ones, the empty one, the one-mutation one, the empty `allowed` row and -- where the
    shape has it -- the document with a term none of its allowed signatures produces"""
    if (C, V) == (3, 4096):
        return _v4096()
    c = R.corpus(C, V)
    nd = R.SHAPES[(C, V)][0]
    pick = [0, 1, nd, nd + 1, nd + 3] + ([nd + 4] if C >= 2 and V >= 2 else [])
    return R.take(c, pick)


@functools.lru_cache(maxsize=None)
def case(C, V):
    """queries: every non-zero entry of every document but document 1 (which stays without queries), with mult = its count; per document
    also a term the document lacks (where there is one), and its first query again with mult 2; groups -1 .. G - 1 at random.  The (2, 5)
    case repeats document 0's queries beyond 4096, the number a block stages in LDS."""
    c = _documents(C, V)
    rng = np.random.default_rng([C, V, 77])
    q_ptr, q_term, q_mult = [0], [], []
    for d in range(c.D):
        sl = slice(c.doc_ptr[d], c.doc_ptr[d + 1])
        t, n = c.term[sl], c.count[sl]
        if d != 1:
            qt = list(t[n > 0]); qm = list(n[n > 0])
            absent = np.setdiff1d(np.arange(V), t[n > 0])
            if absent.size:
                qt.append(int(absent[rng.integers(absent.size)])); qm.append(1)
            if qt:
                qt.append(qt[0]); qm.append(2)
            if (C, V) == (2, 5) and d == 0:
                reps = -(-4100 // len(qt))
                qt, qm = qt * reps, qm * reps
            q_term += qt; q_mult += qm
        q_ptr.append(len(q_term))
    Q = len(q_term)
    q_group = rng.integers(-1, G, size=Q).astype(np.int32)
    return Case(c.name, c.D, C, V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, np.asarray(q_ptr, np.int64), np.asarray(q_term, np.int32),
                np.asarray(q_mult, np.int32), q_group, G, B, SEED, STREAM, c.maxiter, 1e-9)


@functools.lru_cache(maxsize=None)
def reference(C, V):
    return attribute(case(C, V))


@functools.lru_cache(maxsize=None)
def planted():
    """Two signatures with disjoint support: every posterior is exactly 0 or 1 and p_top is 1.  Document 0 holds mutations of both, document
    1 twenty mutations of signature 0 and ONE of signature 1: a replicate that does not draw it fits w_1 = 0 exactly, so the queries on
    signature 1's terms have q_v = 0 in that replicate (void) while the observed q_v is positive."""
    C, V = 2, 8
    cat = np.zeros((C, V))
    cat[0, :4] = [4, 3, 2, 1]; cat[1, 4:] = [1, 2, 3, 4]
    docs = [(np.arange(8, dtype=np.int32), np.asarray([9, 7, 5, 3, 2, 4, 6, 8], np.int32)),
            (np.asarray([0, 1, 2, 5], np.int32), np.asarray([10, 6, 4, 1], np.int32))]
    dp, term, count = R._csr(docs)
    q_ptr = np.asarray([0, 8, 12], np.int64)
    q_term = np.concatenate([np.arange(8), [0, 1, 2, 5]]).astype(np.int32)
    q_mult = np.concatenate([docs[0][1], docs[1][1]]).astype(np.int32)
    q_group = (q_term >= 4).astype(np.int32)
    return Case("planted", 2, C, V, dp, term, count, cat, np.ones((2, C), np.uint8), q_ptr, q_term, q_mult, q_group, 2, 8, 11, 0, 50, 1e-9)


@functools.lru_cache(maxsize=None)
def twin():
    """the (12, 96) case with catalogue row 5 = 2 x row 4 and rows 4, 5 and 9 allowed (the empty row stays empty): the normalised rows are
    equal bit for bit, so are their weights and posteriors, and where they are the largest the tie goes to row 4"""
    c = case(12, 96)
    cat = c.cat.copy()
    cat[5] = 2.0 * cat[4]
    al = np.zeros_like(c.allowed)
    al[:, [4, 5, 9]] = 1
    al[c.allowed.sum(axis=1) == 0] = 0
    return c._replace(name="twin", cat=cat, allowed=al)


def as_X(c):
    """the corpus as the Python layer takes it: a list of W_d x 2 matrices with 1-based terms"""
    return [np.stack([c.term[a:b].astype(np.int64) + 1, c.count[a:b].astype(np.int64)], axis=1) for a, b in zip(c.doc_ptr[:-1], c.doc_ptr[1:])]
