"""numpy restatement of mmm_extract_signatures (include/mmmusig.h) and the cases its tests share.

`extract` follows the definition literally in float64, the order of every sum included: the mixture sequentially over the rows (np.cumsum adds
along an axis one element after the other), g, z and ll as the 64 partial sums and the butterfly of tests/refit_ref.py, the sums over
documents as a cumsum over every stripe's documents (d mod 16) and a cumsum over the 16 stripe sums.  Only +, x, / and comparisons decide sig,
w, iters and unexplained, so a device that keeps the same order gives the same bits; ll and ll_doc contain a log and are compared against
`refit_ref.ll_longdouble` on the same q.  Besides the outputs it returns q of the finish and the md of every iteration: the stopping decisions
of two implementations are comparable where no md is near tol (tests/test_extract_cpu.py asserts that for every case with tol > 0)."""
import functools
from collections import namedtuple

import numpy as np

from bootstrap_ref import philox4x32_10
from refit_ref import _csr, _rows, butterfly, ll_float, normalise, partials

STRIPES = 16

ExOut = namedtuple("ExOut", "sig w ll ll_doc unexplained iters q md")
ExOut.__doc__ = """sig [R, J, V]; w [R, D, K]; ll [R]; ll_doc, unexplained [R, D]; iters [R] int32; q [R, D, V]: the final mixtures; md: per
restart the list of max(max |w' - w|, max |Q' - Q|) of every iteration that ran."""


def dense(D, V, doc_ptr, term, count):
    n = np.zeros((D, V))
    np.add.at(n, (np.repeat(np.arange(D), np.diff(doc_ptr)), term), count.astype(np.float64))
    return n


def start_rows(J, V, r, seed, stream):
    """Q0 of the restart with GLOBAL index r: (u + 1) 2^-32 with u word v % 4 of the block (v / 4, 0x80000000 | j, r, stream), divided by the sequential sum"""
    nb = (V + 3) // 4
    z = np.zeros(nb, np.uint64)
    Q = np.zeros((J, V))
    for j in range(J):
        w = philox4x32_10(np.arange(nb, dtype=np.uint64), z + np.uint64(0x80000000 | j), z + np.uint64(r), z + np.uint64(stream), int(seed) & 0xFFFFFFFF,
                          int(seed) >> 32)
        u = np.stack(w, axis=1).ravel()[:V]
        Q[j] = (u.astype(np.float64) + 1.0) * 2.0 ** -32
    return Q / np.cumsum(Q, axis=1)[:, -1][:, None] if J else Q


def mixtures(w, P):
    """q [D, V] = sum_k w[d, k] P[k, v], k ascending"""
    return np.cumsum(w[:, :, None] * P[None, :, :], axis=1)[:, -1]


def stripe_sum(x):
    """x [D, ...] -> [...]: every stripe's documents in ascending order, then the 16 stripe sums in stripe order"""
    parts = [np.cumsum(x[st::STRIPES], axis=0)[-1] if x[st::STRIPES].shape[0] else np.zeros(x.shape[1:]) for st in range(STRIPES)]
    return np.cumsum(np.stack(parts), axis=0)[-1]


def step(w, P, F, n, f, N):
    """one iteration -> (w', P', md, r)"""
    q = mixtures(w, P)
    m = (n > 0) & (q > 0)
    r = np.zeros_like(q)
    r[m] = f[m] / q[m]
    g = butterfly(partials(r[:, None, :] * P[None, :, :]))
    wn = w * g
    md = np.abs(wn - w).max() if w.size else 0.0
    Pn = P
    if P.shape[0] > F:
        Q = P[F:]
        a = N[:, None] * w[:, F:]
        s = stripe_sum(a[:, :, None] * r[:, None, :])
        t = Q * s
        z = butterfly(partials(t))
        Qn = Q.copy()
        ok = z > 0
        Qn[ok] = t[ok] / z[ok][:, None]
        md = max(md, np.abs(Qn - Q).max())
        Pn = np.concatenate([P[:F], Qn])
    return wn, Pn, md, r


def finish(w, P, n, live, N):
    D = w.shape[0]
    S = np.cumsum(w, axis=1)[:, -1]
    w = w.copy()
    w[S > 0] = w[S > 0] / S[S > 0][:, None]
    q = mixtures(w, P)
    ll_doc = np.zeros(D); unex = N.copy()
    for d in np.flatnonzero(live):
        ll_doc[d], unex[d] = ll_float(n[d], q[d])
    return w, q, ll_doc, unex


def extract(D, F, J, V, doc_ptr, term, count, cat=None, allowed=None, R=1, r0=0, seed=0, stream=0, init=None, maxiter=100, tol=0.0, on_iter=None):
    K = F + J
    Pfix = normalise(cat) if F else np.zeros((0, V))
    n = dense(D, V, doc_ptr, term, count)
    N = n.sum(axis=1)
    A = np.ones((D, K), dtype=bool)
    if allowed is not None and F:
        A[:, :F] = np.asarray(allowed) != 0
    cnt = A.sum(axis=1)
    live = (N > 0) & (cnt > 0)
    f = np.zeros_like(n)
    f[N > 0] = n[N > 0] / N[N > 0][:, None]
    w0 = np.zeros((D, K))
    w0[live] = np.where(A[live], (1.0 / cnt[live])[:, None], 0.0)
    out = ExOut(np.zeros((R, J, V)), np.zeros((R, D, K)), np.zeros(R), np.zeros((R, D)), np.zeros((R, D)), np.zeros(R, dtype=np.int32), np.zeros((R, D, V)), [])
    for r in range(R):
        Q = normalise(init[r]) if init is not None and J else start_rows(J, V, r0 + r, seed, stream)
        P = np.concatenate([Pfix, Q])
        w = w0.copy()
        mds = []
        it = 0
        while it < maxiter:
            it += 1
            w, P, md, _ = step(w, P, F, n, f, N)
            mds.append(md)
            if on_iter is not None:
                on_iter(r, it, w, P)
            if md < tol:
                break
        wf, q, ll_doc, unex = finish(w, P, n, live, N)
        out.sig[r] = P[F:]; out.w[r] = wf; out.ll_doc[r] = ll_doc; out.unexplained[r] = unex; out.iters[r] = it; out.q[r] = q
        out.ll[r] = stripe_sum(ll_doc)
        out.md.append(mds)
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name D F J V doc_ptr term count cat allowed R seed init maxiter tol")

# (F, J, V, D): (R, maxiter, tol, extras) -- the smallest shapes at which each piece of the kernel can go wrong
SHAPES = {
    (0, 1, 1, 1): (1, 30, 0.0),
    (1, 1, 5, 3): (3, 30, 0.0),             # fewer documents than stripes
    (3, 1, 96, 17): (3, 40, 0.0),           # one stripe with two documents
    (3, 2, 97, 33): (3, 40, 1e-3),          # tails of the 64 partial sums
    (0, 4, 130, 16): (1, 30, 0.0),          # F = 0; V beyond the register accumulators
    (2, 4, 128, 18): (1, 30, 1e-3),         # the register accumulators at both of their limits
    (2, 5, 128, 18): (1, 30, 0.0),          # J beyond them
    (33, 2, 96, 20): (1, 30, 0.0),          # more than one 32-wide chunk of g
    (5, 32, 64, 40): (1, 30, 0.0),          # the J limit
    (224, 32, 7, 6): (1, 30, 0.0),          # K = 256
    (2, 3, 1536, 18): (1, 30, 0.0),         # accumulators beyond registers; P and 16 waves' r exceed the LDS of a block: the library halves the waves
    (2, 3, 2000, 17): (1, 8, 0.0),          # ... twice
    (2, 1, 8, 6759): (1, 6, 0.0),           # the largest D whose w [D][K] still fits LDS beside P and 16 waves' r
    (2, 1, 8, 6760): (1, 6, 0.0),           # the smallest whose w goes to the workspace
    (4, 0, 96, 21): (1, 40, 0.0),           # J = 0: the plain refit, with catalogue zeros that leave terms unexplained
}


@functools.lru_cache(maxsize=None)
def corpus(F, J, V, D, seed=0):
    """D documents drawn from the F catalogue rows and J hidden ones (Dirichlet(0.3) rows, Dirichlet(0.5) exposures, multinomial counts), as CSR
    rows with duplicate terms and zero-count entries; document 1 is empty (D >= 3), document 3 has an empty `allowed` row (D >= 5, F >= 1),
    document 4 may use the first fixed row only (D >= 5); where F >= 2 and V >= 2 only the last fixed row produces the last term (J = 0: a
    document that may not use that row has unexplained mutations)"""
    rng = np.random.default_rng([F, J, V, D, seed])
    rows = rng.dirichlet(np.full(V, 0.3), size=F + J) if V > 1 else np.ones((F + J, 1))
    rows = np.maximum(rows, 1e-12 if V > 1 else 0)
    if F >= 2 and V >= 2:
        rows[:F - 1, V - 1] = 0.0
        if J == 0:
            rows[F - 1, V - 1] = max(rows[F - 1, V - 1], 0.05)
    cat = rows[:F] * rng.uniform(0.5, 2.0, size=(F, 1))
    P = rows / rows.sum(1)[:, None]
    docs, allowed = [], np.ones((D, F), dtype=np.uint8)
    for d in range(D):
        use = rng.choice(F + J, size=min(F + J, 4), replace=False)
        wt = rng.dirichlet(np.full(use.size, 0.5))
        n = rng.multinomial(int(rng.integers(200, 3000)), wt @ P[use] / (wt @ P[use]).sum())
        if D >= 3 and d == 1:
            docs.append((np.zeros(0, np.int32), np.zeros(0, np.int32)))
            continue
        if D >= 5 and d == 3 and F:
            allowed[d] = 0
        if D >= 5 and d == 4 and F:
            allowed[d] = 0; allowed[d, 0] = 1
            if F >= 2 and V >= 2:
                n[V - 1] = max(n[V - 1], 5)
        if d >= 6 and F > 4:
            allowed[d, rng.choice(F, size=F // 3, replace=False)] = 0
        docs.append(_rows(rng, n))
    dp, term, count = _csr(docs)
    return dp, term, count, cat, allowed


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for (F, J, V, D), (R, maxiter, tol) in SHAPES.items():
        dp, term, count, cat, allowed = corpus(F, J, V, D)
        out.append(Case("F%dJ%dV%dD%d" % (F, J, V, D), D, F, J, V, dp, term, count, cat if F else None, allowed if F else None, R, 0x9e3779b97f4a7c15 + 7 * V + D,
                        None, maxiter, tol))
    # a caller's init (rows not normalised), and more restarts than CUs
    dp, term, count, cat, allowed = corpus(3, 2, 97, 33)
    init = np.random.default_rng(5).uniform(0.0, 3.0, size=(3, 2, 97)); init[1, 0, :40] = 0.0
    out.append(Case("init", 33, 3, 2, 97, dp, term, count, cat, allowed, 3, 1, init, 30, 0.0))
    dp, term, count, cat, allowed = corpus(1, 1, 5, 3)
    out.append(Case("R300", 3, 1, 1, 5, dp, term, count, cat, allowed, 300, 11, None, 4, 0.0))
    return out


_REF = {}


def reference(c, r0=0, R=None):
    key = (c.name, r0, R)
    if key not in _REF:
        _REF[key] = extract(c.D, c.F, c.J, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, c.R if R is None else R, r0, c.seed,
                            0, c.init if c.init is None or R is None else c.init[r0:r0 + R], c.maxiter, c.tol)
    return _REF[key]


def planted(seed=0):
    """D = 40, V = 96: three catalogue rows and one hidden row, Dirichlet(0.3); exposures Dirichlet(0.5); N_d in [200, 3000) -> (CSR, cat, hidden)"""
    rng = np.random.default_rng([40, 96, seed])
    rows = rng.dirichlet(np.full(96, 0.3), size=4)
    E = rng.dirichlet(np.full(4, 0.5), size=40)
    docs = []
    for d in range(40):
        n = rng.multinomial(int(rng.integers(200, 3000)), E[d] @ rows / (E[d] @ rows).sum())
        v = np.flatnonzero(n)
        docs.append((v.astype(np.int32), n[v].astype(np.int32)))
    return _csr(docs), rows[:3], rows[3]
