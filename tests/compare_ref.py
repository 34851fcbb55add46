"""numpy restatement of mmm_deal_counts and mmm_compare_exposures (include/mmmusig.h) and the corpora its tests share.

Built only from the restatements that already exist: `refit_ref.fit` / `normalise` / `ll_longdouble` for the fits, the Philox4x32-10 words as
`simulate_ref.words` / `select_ref.fold_words` form them (another counter), and `np.lexsort` for the selection of the N_a smallest
(key, index) pairs.  It imports nothing from the product and shares nothing with the kernel: the kernel never sorts, it selects by radix.
Per sample and replicate it returns T, its longdouble value on the same mixtures with the rounding bound, and whether the replicate's
partition IS the observed one (an exact tie by construction) -- what makes count_ge comparable across two implementations of log
(tests/test_compare_cpu.py asserts the separation for every corpus the GPU tests use)."""
import functools
from collections import namedtuple

import numpy as np

import refit_ref as R
from bootstrap_ref import philox4x32_10

DEAL_TAG = 0xD0000000         # high nibble of the SECOND counter word of a dealing


def deal_words(N, d, b, seed, stream=0):
    """[len(b), N] random words of the replicates b (global indices) of sample d: mutation i takes word i % 4 of the block with counter
    (i / 4, 0xD0000000 | d, b, stream) under the key (seed low, seed high)"""
    b = np.atleast_1d(np.asarray(b, dtype=np.uint64))
    nblk = (int(N) + 3) // 4
    c0 = np.arange(nblk, dtype=np.uint64)[None, :]
    z = np.zeros((b.size, nblk), np.uint64)
    w = philox4x32_10(z + c0, z + np.uint64(DEAL_TAG | int(d)), z + b[:, None], z + np.uint64(stream), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return np.stack(w, axis=-1).reshape(b.size, 4 * nblk)[:, :int(N)]


def deal_members(N, Na, d, b, seed, stream=0, key_bits=32):
    """[len(b), N] bool: is mutation i in set a -- the Na smallest (key, index) pairs, key = word >> (32 - key_bits)"""
    b = np.atleast_1d(b)
    keys = deal_words(N, d, b, seed, stream) >> np.uint64(32 - key_bits)
    idx = np.arange(int(N))
    out = np.zeros((b.size, int(N)), dtype=bool)
    for r in range(b.size):
        out[r, np.lexsort((idx, keys[r]))[:int(Na)]] = True        # the last key of lexsort is the primary one
    return out


def deal_doc(count, Na, d, b, seed, stream=0, key_bits=32):
    """[len(b), W] the part of every entry that goes to set a; count: the counts in the order the mutations are numbered in"""
    count = np.asarray(count, dtype=np.int64)
    b = np.atleast_1d(b)
    N = int(count.sum())
    out = np.zeros((b.size, count.size), dtype=np.int64)
    if N == 0 or int(Na) == 0:
        return out
    entry = np.searchsorted(np.cumsum(count), np.arange(N, dtype=np.int64), side="right")       # cum[e-1] <= i < cum[e]
    member = deal_members(N, Na, d, b, seed, stream, key_bits)
    for r in range(b.size):
        out[r] = np.bincount(entry[member[r]], minlength=count.size)
    return out


def deal(doc_ptr, count, n_a, B, b0=0, seed=0, stream=0, key_bits=32):
    """mmm_deal_counts -> int64 [B, nnz]"""
    D = len(doc_ptr) - 1
    out = np.zeros((B, int(doc_ptr[D])), dtype=np.int64)
    for d in range(D):
        s, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        if e > s and B:
            out[:, s:e] = deal_doc(count[s:e], n_a[d], d, b0 + np.arange(B), seed, stream, key_bits)
    return out


# ---- the test -----------------------------------------------------------------------------------------------------------------------------------
CCorpus = namedtuple("CCorpus", "name D C V ptr_a term_a count_a ptr_b term_b count_b cat allowed maxiter tol B seed stream")

RefOut = namedtuple("RefOut", "w_a w_b w_pool stat stat_ld bound t_obs ll_pool count_ge count_sig count_max status unexplained iters delta rep rep_ld rep_bound "
                    "rep_same dealt N_a N_b n_allowed")
RefOut.__doc__ = """w_a, w_b, w_pool, delta [D, C]; stat, t_obs, ll_pool, unexplained [D]; stat_ld, bound [D]: max(2 (T_obs - ll_0), 0) in longdouble on
the same mixtures and 2 (bound(ll_x) + bound(ll_y) + bound(ll_0)); count_ge [D], count_sig, count_max [D, C] int32; status int8, iters int64
[D]; rep [B, D] = 2 (T_b - ll_0) (NaN for status 3), rep_ld, rep_bound likewise; rep_same [B, D] bool: the replicate's partition is the observed
one (or its mirror image where N_a = N_b), so T_b = T_obs bit for bit in any implementation; dealt [B, D, V] the vectors n^{a,b}; N_a, N_b [D]; n_allowed [D] = |A|: with ONE
allowed signature every fit is w = 1 and T is the same for every partition up to rounding -- count_ge of such a sample is decided by the last
bits of log and is not comparable between implementations (nor informative)."""


def dense(V, ptr, term, count, d):
    n = np.zeros(V)
    np.add.at(n, term[ptr[d]:ptr[d + 1]], count[ptr[d]:ptr[d + 1]].astype(np.float64))
    return n


def pair(PA, x, y, maxiter, tol):
    """the statistic of a pair of count vectors -> (w_x, w_y, T, T in longdouble, bound, iterations)"""
    wx, llx, _, itx, qx = R.fit(PA, x, x / x.sum(), maxiter, tol)
    wy, lly, _, ity, qy = R.fit(PA, y, y / y.sum(), maxiter, tol)
    (Lx, bx), (Ly, by) = R.ll_longdouble(x, qx), R.ll_longdouble(y, qy)
    return wx, wy, llx + lly, Lx + Ly, bx + by, itx + ity


def compare(c, B=None, b0=0, key_bits=32):
    B = c.B if B is None else B
    P = R.normalise(c.cat)
    D, C, V = c.D, c.C, c.V
    o = RefOut(np.zeros((D, C)), np.zeros((D, C)), np.zeros((D, C)), np.zeros(D), np.zeros(D), np.zeros(D), np.zeros(D), np.zeros(D), np.zeros(D, np.int32),
               np.zeros((D, C), np.int32), np.zeros((D, C), np.int32), np.zeros(D, np.int8), np.zeros(D), np.zeros(D, np.int64), np.zeros((D, C)),
               *[np.full((B, D), np.nan) for _ in range(3)], np.zeros((B, D), bool), np.zeros((B, D, V), np.int64), np.zeros(D, np.int64), np.zeros(D, np.int64),
               np.zeros(D, np.int64))
    for d in range(D):
        na, nb = dense(V, c.ptr_a, c.term_a, c.count_a, d), dense(V, c.ptr_b, c.term_b, c.count_b, d)
        Na, Nb = int(na.sum()), int(nb.sum())
        o.N_a[d], o.N_b[d] = Na, Nb
        A = np.flatnonzero(c.allowed[d]) if c.allowed is not None else np.arange(C)
        o.n_allowed[d] = A.size
        if Na == 0 or Nb == 0 or A.size == 0:
            o.status[d] = 3
            continue
        n = na + nb
        wx, wy, T, T_ld, bd, it = pair(P[A], na, nb, c.maxiter, c.tol)
        w0, ll0, u0, it0, q0 = R.fit(P[A], n, n / n.sum(), c.maxiter, c.tol)
        L0, bd0 = R.ll_longdouble(n, q0)
        o.w_a[d, A], o.w_b[d, A], o.w_pool[d, A] = wx, wy, w0
        o.t_obs[d], o.ll_pool[d], o.unexplained[d], o.iters[d] = T, ll0, u0, it + it0
        o.stat[d] = max(2.0 * (T - ll0), 0.0)
        o.stat_ld[d] = max(float(2 * (T_ld - L0)), 0.0)
        o.bound[d] = 2.0 * (bd + bd0)
        dobs = np.abs(wx - wy)
        o.delta[d, A] = dobs
        if B == 0:
            continue
        o.dealt[:, d, :] = deal_doc(n.astype(np.int64), Na, d, b0 + np.arange(B), c.seed, c.stream, key_bits)
        for b in range(B):
            x = o.dealt[b, d].astype(np.float64)
            y = n - x
            rx, ry, Tb, Tb_ld, bb, itb = pair(P[A], x, y, c.maxiter, c.tol)
            o.iters[d] += itb
            o.rep[b, d], o.rep_ld[b, d], o.rep_bound[b, d] = 2.0 * (Tb - ll0), float(2 * (Tb_ld - L0)), 2.0 * (bb + bd0)
            o.rep_same[b, d] = np.array_equal(x, na) or (Na == Nb and np.array_equal(x, nb))
            db = np.abs(rx - ry)
            o.count_ge[d] += Tb >= T
            o.count_sig[d, A] += db >= dobs
            o.count_max[d, A] += db.max() >= dobs
    return o


# ---- corpora -----------------------------------------------------------------------------------------------------------------------------------
# (C, V): replicates -- the smallest shapes at which each mechanism can go wrong: one signature and fewer terms than lanes; exactly one slot of 64
# terms; the workload's shape (second slot half empty) with two 32-wide reduction chunks; a list padded beyond 64 with a ragged third slot
SHAPES = {(1, 5): 24, (3, 64): 24, (33, 96): 16, (70, 130): 12}
SEEDS = {(1, 5): 0, (3, 64): 0, (33, 96): 0, (70, 130): 0}


def _ordered(n):
    v = np.flatnonzero(n)
    return v.astype(np.int32), n[v].astype(np.int32)


@functools.lru_cache(maxsize=None)
def corpus(C, V):
    """Samples: 0 N_a = 260 (just over one step of 256 mutations), N over 1024 (several Philox steps, a partial last block); 1 a per-sample
    `allowed` subset; 2 N_a = 1; 3 N_b = 1 (N_a = N - 1); 4 N = 2; 5 N_a = 0, 6 N_b = 0, 7 an empty `allowed` row (status 3 each); 8 (C, V >= 2)
    a term that no allowed signature produces (u_0 > 0).  Table a is in term order; table b holds duplicate terms, zero counts and entries
    out of term order (refit_ref._rows)."""
    B = SHAPES[(C, V)]
    rng = np.random.default_rng([C, V, SEEDS[(C, V)], 423])
    cat = np.maximum(rng.dirichlet(np.full(V, 0.3 if V > 5 else 1.0), size=C) * rng.uniform(0.5, 2.0, size=(C, 1)), 1e-12)
    if C >= 2:
        cat[:-1, V - 1] = 0.0                           # only the last signature produces the last term
    P = R.normalise(cat)
    one = np.ones(C, dtype=np.uint8)
    A, Bt, allowed = [], [], []

    def draw(N, al):
        on = np.flatnonzero(al if al.any() else one)
        k = min(on.size, 3)
        rows = rng.choice(on, size=k, replace=False)
        p = rng.dirichlet(np.full(k, 2.0)) @ P[rows]
        return rng.multinomial(N, p / p.sum())

    def add(Na, Nb, al):
        A.append(_ordered(draw(Na, al)) if Na else (np.zeros(0, np.int32), np.zeros(0, np.int32)))
        Bt.append(R._rows(rng, draw(Nb, al)) if Nb else (np.zeros(0, np.int32), np.zeros(0, np.int32)))
        allowed.append(al)

    add(260, 1027 - 260 + int(rng.integers(0, 60)), one)
    part = one.copy()
    if C >= 3:
        part[:] = 0
        part[rng.choice(C, size=max(2, C // 3), replace=False)] = 1
    add(int(rng.integers(80, 200)), int(rng.integers(80, 200)), part)
    add(1, 57, one)
    add(61, 1, one)
    add(1, 1, one)
    add(0, 40, one)
    add(40, 0, one)
    add(30, 30, np.zeros(C, dtype=np.uint8))
    if C >= 2:
        no_last = one.copy(); no_last[C - 1] = 0
        na, nb = draw(90, one), draw(120, one)
        na[V - 1] = max(na[V - 1], 3)
        A.append(_ordered(na)); Bt.append(R._rows(rng, nb)); allowed.append(no_last)
    pa, ta, ca = R._csr(A)
    pb, tb, cb = R._csr(Bt)
    return CCorpus("C%dV%d" % (C, V), len(A), C, V, pa, ta, ca, pb, tb, cb, cat, np.stack(allowed), 60, 1e-9, B, 4230 + C, V % 5)


@functools.lru_cache(maxsize=None)
def edge_corpus():
    """C = 4, V = 12, for the Python layer: sample 0 regular, 1 without set-a mutations, 2 without set-b mutations, 3 with nothing allowed, 4 regular
    with two signatures allowed"""
    C, V = 4, 12
    rng = np.random.default_rng([0, 424])
    cat = np.maximum(rng.dirichlet(np.full(V, 0.5), size=C), 1e-9)
    one = np.ones(C, dtype=np.uint8)
    two = np.array([1, 0, 1, 0], dtype=np.uint8)
    mk = lambda N, w: _ordered(rng.multinomial(N, np.asarray(w) @ cat / (np.asarray(w) @ cat).sum()))
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    A = [mk(300, [0.5, 0.2, 0.2, 0.1]), empty, mk(100, [1, 0, 0, 0]), mk(50, [0, 1, 0, 0]), mk(200, [0.6, 0, 0.4, 0])]
    Bt = [mk(250, [0.1, 0.2, 0.2, 0.5]), mk(100, [0, 0, 1, 0]), empty, mk(50, [0, 1, 0, 0]), mk(150, [0.5, 0, 0.5, 0])]
    pa, ta, ca = R._csr(A)
    pb, tb, cb = R._csr(Bt)
    return CCorpus("edge", 5, C, V, pa, ta, ca, pb, tb, cb, cat, np.stack([one, one, one, np.zeros(C, np.uint8), two]), 60, 1e-9, 16, 99, 2)


@functools.lru_cache(maxsize=None)
def corpora():
    """every corpus the GPU tests run against the restatement"""
    return [corpus(C, V) for (C, V) in SHAPES]


KEY_BITS = (32, 3)             # the contract's, and the hook that puts ties at the threshold in essentially every replicate
_REF = {}


def reference(c, key_bits=32):
    if (c.name, key_bits) not in _REF:
        _REF[(c.name, key_bits)] = compare(c, key_bits=key_bits)
    return _REF[(c.name, key_bits)]


def planted_corpus(seed=1, C=3, V=16, n_changed=4, n_same=40, N=600, share=0.5):
    """C Dirichlet(0.3) signatures over V terms.  Every sample draws both sets from one mixture, except that set b of the first n_changed
    samples carries an extra `share` of signature 0.  -> (CCorpus, changed [D] bool)"""
    rng = np.random.default_rng([seed, 425])
    cat = rng.dirichlet(np.full(V, 0.3), size=C)
    D = n_changed + n_same
    A, Bt = [], []
    for d in range(D):
        w = rng.dirichlet(np.full(C, 2.0))
        p = w @ cat
        pb = (1 - share) * p + share * cat[0] if d < n_changed else p
        A.append(_ordered(rng.multinomial(N, p / p.sum()))); Bt.append(_ordered(rng.multinomial(N, pb / pb.sum())))
    pa, ta, ca = R._csr(A)
    pb_, tb, cb = R._csr(Bt)
    return CCorpus("planted", D, C, V, pa, ta, ca, pb_, tb, cb, cat, None, 40, 1e-6, 39, 7, 0), np.arange(D) < n_changed
