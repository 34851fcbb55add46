"""Held-out selection of the number of signatures on the device: the split against its numpy restatement (tests/select_ref.py) integer for
integer, the score against a longdouble restatement, the handle form against the array form bit for bit, the drivers against their
compositions done by hand, and a planted K found again."""
import numpy as np
import pytest

import np_ref
import select_ref as sr

pytestmark = pytest.mark.gpu

SEED = 0x1234567800000005


def _corpus():
    X, _ = np_ref.synth_lda(40, 96, 6, seed=31, mean_n=400)
    X = [x.copy() for x in X]
    X[3][2, 1] = 0                       # an entry with count 0, added by hand
    return X


def _odd_corpus():
    """an empty document, a one-entry document, all-zero rows, a 1,536-term document of 24,000 mutations, a row of 2,500 entries (terms
    below 1,536, so with duplicates), and a few ordinary documents"""
    rng = np.random.default_rng(8)
    X = [np.zeros((0, 2), np.int64), np.array([[7, 13]], np.int64), np.stack([np.arange(1, 6), np.zeros(5, np.int64)], axis=1).astype(np.int64)]
    X.append(np.stack([np.arange(1, 1537), rng.multinomial(24000, rng.dirichlet(np.full(1536, 0.5)))], axis=1).astype(np.int64))
    X.append(np.stack([rng.integers(1, 1537, size=2500), rng.integers(0, 9, size=2500)], axis=1).astype(np.int64))
    for _ in range(3):
        t = np.sort(rng.choice(1536, size=70, replace=False)) + 1
        X.append(np.stack([t, rng.integers(1, 30, size=70)], axis=1).astype(np.int64))
    return X


def _counts(parts):
    return sr.counts_matrix(parts)


# ---- 1. split -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 3, 16])
def test_split_equals_the_restatement(mmm, F):
    for X in (_corpus(), _odd_corpus()):       # odd corpus, F = 16: the 1,536-term row and the 2,500-entry row count through global memory
        got = mmm.split_counts(X, F, SEED)
        want = sr.split(X, F, SEED)
        assert len(got) == F
        for g, w in zip(got, want):
            assert len(g) == len(X) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(g, w))
        assert np.array_equal(_counts(got).sum(axis=0), np.concatenate([x[:, 1] for x in X]))
        again = mmm.split_counts(X, F, SEED)
        assert np.array_equal(_counts(got), _counts(again))                        # two runs, equal bits


def test_split_arguments_and_errors(mmm):
    X = _corpus()[:8]
    ctx = mmm.default_context()
    dp, term, count = mmm.pack_lda(X)
    raw = mmm.select._split_csr
    base = raw(ctx, len(X), dp, count, 3, 0, SEED, 0)
    assert np.array_equal(base, _counts(sr.split(X, 3, SEED)))
    for kw in (dict(seed=SEED + 1), dict(seed=SEED + (1 << 32)), dict(rep=1), dict(stream=1)):      # both key words, rep and stream enter
        a = dict(rep=0, seed=SEED, stream=0); a.update(kw)
        got = raw(ctx, len(X), dp, count, 3, a["rep"], a["seed"], a["stream"])
        assert not np.array_equal(got, base)
        assert np.array_equal(got, _counts(sr.split(X, 3, a["seed"], rep=a["rep"], stream=a["stream"])))
    out = np.zeros((65, count.size), np.int32)
    L = mmm.lib()
    for F in (0, 65):
        assert L.mmm_split_counts(ctx.h, len(X), dp, count.ctypes.data, F, 0, 1, 0, out.ctypes.data) == -1
    assert L.mmm_split_counts(ctx.h, len(X), dp, count.ctypes.data, 2, 0, 1, 1 << 31, out.ctypes.data) == -1        # the stream's high bit is the split's
    assert L.mmm_split_counts(ctx.h, 0, np.zeros(1, np.int64), None, 2, 0, 1, 0, None) == 0                          # nnz = 0: nothing written
    with pytest.raises(ValueError):
        mmm.split_counts(X, 0, 1)


def test_split_python_nestings(mmm):
    X = _corpus()[:6]
    got = mmm.split_counts(X, 3, 11, rep=2)
    want = sr.split(X, 3, 11, rep=2)
    assert all(np.array_equal(a, b) for g, w in zip(got, want) for a, b in zip(g, w))
    Xm, _ = np_ref.synth_mm(6, [96, 48], [3, 2], seed=4, means=[300, 80], empty_frac=0.3)
    got = mmm.split_counts(Xm, 2, 11)
    want = sr.split_mm(Xm, 2, 11)                                                 # modality m with stream = m
    for f in range(2):
        for d in range(6):
            for m in range(2):
                assert np.array_equal(got[f][d][m], want[f][d][m])
    mod1 = [Xm[d][1] for d in range(6)]                                            # (some of them empty: compare the modality as a whole)
    assert sum(x[:, 1].sum() for x in mod1) > 0
    assert not np.array_equal(sr.counts_matrix([[got[0][d][1] for d in range(6)]]), sr.counts_matrix([sr.split(mod1, 2, 11, stream=0)[0]]))


# ---- 2. score -------------------------------------------------------------------------------------------------------------------------------
def _fold5(X):
    """the 40-document corpus folded onto 5 terms (duplicate terms within a document) plus an empty document"""
    return [np.stack([(x[:, 0] - 1) % 5 + 1, x[:, 1]], axis=1) for x in X] + [np.zeros((0, 2), np.int64)]


@pytest.mark.parametrize("K,V", [(1, 5), (7, 96), (32, 1536)])
def test_score_against_longdouble(mmm, K, V):
    X = {5: _fold5(_corpus()), 96: _corpus() + [np.zeros((0, 2), np.int64)], 1536: _odd_corpus()}[V]
    rng = np.random.default_rng(100 + K)
    D = len(X)
    θ = rng.dirichlet(np.full(K, 0.7), size=D).T                                  # K x D
    β = rng.dirichlet(np.full(V, 0.5), size=K).T + 1e-9                            # V x K
    β /= β.sum(axis=0)
    got = mmm.score_exposures(X, θ, β)
    ll, n_doc, cos = sr.score(X, θ, β)
    N = np.array([int(np.asarray(x).reshape(-1, 2)[:, 1].sum()) for x in X])
    assert np.array_equal(got.n_doc, N.astype(np.float64))                          # exact
    rel_ll = np.abs((got.ll_doc - ll) / np.where(ll != 0, ll, 1)).astype(np.float64)
    rel_cos = np.abs((got.cosine_doc - cos) / np.where(cos != 0, cos, 1)).astype(np.float64)
    print("K=%d V=%d: max relative deviation ll_doc %.3e, cos_doc %.3e" % (K, V, rel_ll.max(), rel_cos.max()))
    assert rel_ll.max() <= 1e-12 and rel_cos.max() <= 1e-12
    empty = N == 0
    assert empty.any() and (got.ll_doc[empty] == 0).all() and (got.cosine_doc[empty] == 0).all()
    assert (got.cosine_doc[~empty] > 0).all()
    if V == 96:                                                                     # no duplicate terms: a cosine proper
        assert (got.cosine_doc <= 1 + 1e-12).all()
    assert got.ll == mmm.calculate_loglikelihood(X, θ, β)                           # the mixture ll of the free function, bit for bit
    # totals leave the empty documents out
    ctx = mmm.default_context()
    dp, term, count = mmm.pack_lda(X)
    th = np.ascontiguousarray(θ.T).ravel(); be = np.ascontiguousarray(β.T).ravel()
    total = np.zeros(4)
    rc = mmm.lib().mmm_mixture_score(ctx.h, D, K, V, dp, term.ctypes.data, count.ctypes.data, th, be, None, None, None, total)     # NULL outputs
    assert rc == 0 and total[0] == got.ll and total[3] == got.cosine
    assert total[2] == N.sum() and abs(total[1] - float(ll.sum())) <= 1e-12 * abs(float(ll.sum()))
    assert abs(total[3] - float(cos[~empty].mean())) <= 1e-12


# ---- 3. handle form ---------------------------------------------------------------------------------------------------------------------------
def test_score_restarts_equals_the_array_form(mmm):
    X = _corpus()
    test = mmm.split_counts(X, 2, 5)[0]
    lam0 = [np.random.default_rng(40 + r).integers(1, 101, size=(96, 6)).astype(np.float64) for r in range(8)]
    A = mmm.LDA(6, 0.1, 0.1, 96, X, λ0=lam0, restarts=8)
    B = mmm.LDA(6, 0.1, 0.1, 96, X, λ0=lam0, restarts=8)                           # a twin that is never scored
    with pytest.raises(mmm.MmmError, match="no pass has run"):
        mmm.score_restarts(A, test)
    for m in (A, B):
        mmm.fit_restarts(m, maxiter=5)                                            # every restart stands at pass 5
    A.select(3)
    ll0, lam3 = A.restart_ll.copy(), A.λ
    total = mmm.score_restarts(A, test)
    assert A.selected == 3 and np.array_equal(A.restart_ll, ll0) and np.array_equal(A.λ, lam3)
    s = mmm.score_exposures(test, A.θ, A.β)
    assert total[3, 0] == s.ll and total[3, 3] == s.cosine
    A.select(0)
    for m in (A, B):
        mmm.fit_restarts(m)                                                       # to convergence: the restarts stop at passes of their own
    assert np.array_equal(A.restart_ll, B.restart_ll) and np.array_equal(A.restart_iters, B.restart_iters)      # the score left no trace
    iters = np.asarray(A.restart_iters)
    print("passes per restart: %r" % (iters.tolist(),))
    assert len(set((iters % 3).tolist())) > 1                                     # different ring slots: a wrong slot would show
    total, ll_doc, cos_doc = mmm.score_restarts(A, test, per_document=True)
    assert total.shape == (8, 4) and ll_doc.shape == (8, 40) and cos_doc.shape == (8, 40)
    for r in range(8):
        A.select(r); B.select(r)
        assert np.array_equal(A.λ, B.λ)
        s = mmm.score_exposures(test, A.θ, A.β)
        assert total[r, 0] == s.ll and total[r, 3] == s.cosine
        assert abs(total[r, 1] - s.ll_doc.sum()) <= 1e-12 * abs(total[r, 1])
        assert total[r, 2] == s.n_doc.sum()
        assert np.array_equal(ll_doc[r], s.ll_doc) and np.array_equal(cos_doc[r], s.cosine_doc)
    assert len(set(total[:, 0].tolist())) > 1
    with pytest.raises(mmm.MmmError):
        mmm.score_restarts(A, [np.array([[97, 1]])] * 40)                         # a term beyond V
    with pytest.raises(ValueError):
        mmm.score_restarts(A, test[:39])
    A.close(); B.close()


def test_score_restarts_on_ordinary_and_ilda_handles(mmm):
    X = _corpus()
    test = mmm.split_counts(X, 2, 5)[1]
    g = mmm.LDA(5, 0.1, 0.1, 96, X, seed=2)
    with pytest.raises(mmm.MmmError, match="no pass has run"):
        mmm.score_restarts(g, test)
    mmm.fit(g, maxiter=7, tol=0.0, verbose=False)                                 # 7 passes: the ring stands at slot 1
    total, ll_doc, cos_doc = mmm.score_restarts(g, test, per_document=True)
    s = mmm.score_exposures(test, g.θ, g.β)
    assert total.shape == (1, 4) and total[0, 0] == s.ll and np.array_equal(ll_doc[0], s.ll_doc) and np.array_equal(cos_doc[0], s.cosine_doc)
    g.close()
    feats = np.stack([np.arange(96) // 16 + 1, np.arange(96) % 16 + 1], axis=1)
    il = mmm.ILDA(4, 0.1, 0.1, feats, X, seed=3)
    mmm.fit(il, maxiter=3, tol=0.0, verbose=False)
    with pytest.raises(mmm.MmmError, match="ILDA"):
        mmm.score_restarts(il, test)
    il.close()


# ---- 4. the drivers are their compositions ------------------------------------------------------------------------------------------------------
def test_lda_driver_is_its_composition(mmm):
    X, _ = np_ref.synth_lda(24, 96, 3, seed=17, mean_n=300)
    V = max(int(x[:, 0].max()) for x in X)
    kw = dict(folds=2, reps=1, restarts=3, seed=7, maxiter=30, tol=1e-4, full_fit=False)
    res = mmm.select_num_signatures(X, [2, 3], 0.1, 0.1, **kw)
    assert res.heldout.shape == (2, 2) and res.heldout_all.shape == (2, 2, 3) and res.train_ll is None
    parts = mmm.split_counts(X, 2, 7, rep=0)
    for f in range(2):
        train, test = mmm.holdout(X, parts, f)
        for i, K in enumerate([2, 3]):
            seeds = np.random.default_rng([7, K, 0, f]).integers(1, 2 ** 62, size=3)
            lam0 = [np.random.default_rng(int(s)).integers(1, 101, size=(V, K)).astype(np.float64) for s in seeds]
            model = mmm.LDA(K, 0.1, 0.1, V, train, λ0=lam0, restarts=3)
            mmm.fit_restarts(model, maxiter=30, tol=1e-4)
            total = mmm.score_restarts(model, test)
            best = int(np.argmax(model.restart_ll))                                # the best TRAINING log-likelihood picks the restart
            assert np.array_equal(res.heldout_all[i, f], total[:, 0]) and res.heldout[i, f] == total[best, 0]
            model.close()
    p = mmm.pick_k([2, 3], res.heldout)
    assert np.array_equal(res.mean, p.mean) and np.array_equal(res.se, p.se) and (res.best, res.pick) == (p.best, p.pick)
    again = mmm.select_num_signatures(X, [2, 3], 0.1, 0.1, **kw)
    assert np.array_equal(again.heldout_all, res.heldout_all) and np.array_equal(again.heldout, res.heldout)
    other = mmm.select_num_signatures(X, [2, 3], 0.1, 0.1, **dict(kw, seed=8))
    assert not np.array_equal(other.heldout, res.heldout)


def test_mmctm_driver_is_its_composition(mmm):
    Vm, K, α = [24, 12], [3, 2], [0.1, 0.1]
    X, _ = np_ref.synth_mm(16, Vm, K, seed=21, means=[300, 100])
    kw = dict(folds=2, reps=1, restarts=2, seed=3, maxiter=10, tol=1e-4)
    res = mmm.select_num_signatures_mmctm(X, [K], α, Vm, pick=True, **kw)
    assert res.heldout.shape == (1, 2, 2) and np.isfinite(res.heldout).all() and [p.pick for p in res.picks] == K
    fit_seed_models, seed_and_fit_restart = mmm.restarts.fit_seed_models, mmm.restarts.seed_and_fit_restart
    parts = mmm.split_counts(X, 2, 3)
    for f in range(2):
        train, test = mmm.holdout(X, parts, f)
        seeds = [int(s) for s in np.random.default_rng([3, 0, 0, f]).integers(1, 2 ** 62, size=2)]
        opt_gamma, _, _ = fit_seed_models(train, K, α, Vm, seeds, maxiter=10, tol=1e-4)
        model = seed_and_fit_restart(train, K, α, Vm, opt_gamma, maxiter=10, tol=1e-5)
        for m in range(2):
            Xm = [test[d][m] for d in range(16)]
            props = [model.props[d][m] for d in range(16)]
            ϕ = [model.ϕ[m][k] for k in range(K[m])]
            s = mmm.score_exposures(Xm, np.stack(props, axis=1), np.stack(ϕ, axis=1))
            assert res.heldout[0, f, m] == s.ll == mmm.calculate_modality_loglikelihood(Xm, props, ϕ)
        model.close()


# ---- 5. a planted K -----------------------------------------------------------------------------------------------------------------------------
def test_finds_a_planted_k(mmm):
    """48 documents drawn from 3 signatures over 24 terms.  A plain numpy variational LDA (80 passes, the same initialisations, the same split
    definition) gave held-out means -2.122 / -1.892 / -1.790 / -1.791 / -1.793 for K = 1..5 with se of 0.007-0.009: a gap of about 0.10
    = 12 se between K = 2 and K = 3, and pick = 3."""
    X, _ = np_ref.synth_lda(48, 24, 3, seed=5, mean_n=300)
    Ks = [1, 2, 3, 4, 5]
    res = mmm.select_num_signatures(X, Ks, 0.1, 0.1, folds=4, reps=1, restarts=4, seed=20260101)
    print("held-out mean per K: %r\nse: %r\nbest %d pick %d\ntrain ll %r\ncosine %r\nstability %r" % (
        res.mean.tolist(), res.se.tolist(), res.best, res.pick, res.train_ll.tolist(), res.cosine.tolist(), [s.tolist() for s in res.stability]))
    assert res.pick == 3
    assert res.mean[2] - res.mean[1] > 5 * res.se.max()
    assert res.heldout.shape == (5, 4) and res.heldout_all.shape == (5, 4, 4)
    assert [len(s) for s in res.stability] == Ks and np.all(np.diff(res.train_ll[:3]) > 0)
    assert ((res.cosine > 0) & (res.cosine <= 1 + 1e-12)).all() and res.cosine[2] > res.cosine[0]
