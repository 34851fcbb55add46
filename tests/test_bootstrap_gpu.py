"""Bootstrap of the exposures on the device: the resampling and the summary against the numpy restatement of their definitions
(tests/bootstrap_ref.py; bit for bit where the definition is integer), the bootstrap against the composition it is defined as
(`transform` on the stacked replicate corpus: exact equality), and the checks a user would make."""
import warnings

import numpy as np
import pytest

import bootstrap_ref as br
import np_ref
from test_inference_gpu import _ctm_trained, _lda_pair

pytestmark = pytest.mark.gpu

SEED = 20260101
Q5 = [0.0, 0.025, 0.5, 0.975, 1.0]


def _csr(mmm, X):
    return mmm.pack_lda(X)


def _dev_counts(mmm, X, B, seed, b0=0, stream=0):
    """mmm_resample_counts through the C entry -> [B, nnz]"""
    from multimodalmusig_jl_amd.bootstrap import _resample_csr
    dp, _, c = _csr(mmm, X)
    return _resample_csr(mmm.default_context(), len(X), dp, c, B, b0, seed, stream)


def _base_corpus():
    X, _ = np_ref.synth_lda(40, 96, 6, seed=31, mean_n=400)
    X = [x.copy() for x in X]
    X[3][2, 1] = 0
    return X


def _odd_corpus():
    """an empty document, a one-entry document, >= 20,000 mutations over 1,536 terms, and a row of 2,500 entries (beyond the 2,048 the
    resampling kernel keeps in LDS: the global-memory path), between ordinary ones"""
    rng = np.random.default_rng(77)
    X, _ = np_ref.synth_lda(6, 96, 6, seed=32, mean_n=300)
    wide = rng.multinomial(24000, rng.dirichlet(np.full(1536, 0.3)))
    assert wide.sum() >= 20000
    long_row = rng.integers(0, 6, size=2500)
    docs = [X[0], np.zeros((0, 2), np.int64), X[1], np.array([[17, 345]], np.int64), X[2],
            np.stack([np.arange(1, 1537), wide], axis=1).astype(np.int64), X[3],
            np.stack([np.arange(1, 2501), long_row], axis=1).astype(np.int64), X[4], np.array([[5, 0], [9, 0]], np.int64), X[5]]
    return docs


# ------------------------------------------------------------------------------------------------------------ 1. resampling
@pytest.mark.parametrize("which", ["base", "odd"])
def test_resampling_is_the_definition(mmm, which):
    X = _base_corpus() if which == "base" else _odd_corpus()
    for B in (1, 7, 256):
        got = _dev_counts(mmm, X, B, SEED)
        want = br.counts_matrix(br.resample(X, B, SEED))
        assert got.shape == want.shape and np.array_equal(got, want), "B = %d: %d entries differ" % (B, int((got != want).sum()))
    big = _dev_counts(mmm, X, 256, SEED)
    assert np.array_equal(_dev_counts(mmm, X, 8, SEED, b0=64), big[64:72])                     # chunked calls are slices
    assert np.array_equal(_dev_counts(mmm, X, 256, SEED), big)                                 # same bits on every run
    assert np.array_equal(_dev_counts(mmm, X, 5, SEED, stream=1), br.counts_matrix(br.resample(X, 5, SEED, stream=1)))
    assert not np.array_equal(_dev_counts(mmm, X, 5, SEED, stream=1), big[:5])
    s64 = (0xDEADBEEF << 32) | 12345                                                           # both key words
    assert np.array_equal(_dev_counts(mmm, X, 3, s64), br.counts_matrix(br.resample(X, 3, s64)))


def test_resample_counts_python_entry(mmm):
    X = _base_corpus()
    reps = mmm.resample_counts(X, 4, SEED, b0=2)
    want = br.resample(X, 4, SEED, b0=2)
    assert len(reps) == 4 and all(len(r) == len(X) for r in reps)
    for r, w in zip(reps, want):
        for a, b in zip(r, w):
            assert a.dtype == np.int64 and np.array_equal(a, b)                                # zero rows kept, same terms
    Xm, _ = np_ref.synth_mm(12, [40, 24], [5, 4], seed=3, means=[600, 80], empty_frac=0.2)
    repm = mmm.resample_counts(Xm, 3, SEED)
    wantm = br.resample_mm(Xm, 3, SEED)
    for b in range(3):
        for d in range(12):
            for m in range(2):
                assert np.array_equal(repm[b][d][m], wantm[b][d][m])
    assert mmm.resample_counts(X, 0, SEED) == []


# ------------------------------------------------------------------------------------------------------------ 2. summary
@pytest.mark.parametrize("B", [1, 2, 5, 64, 1000, 4096])
def test_summary_is_the_definition(mmm, B):
    n = 3001
    rng = np.random.default_rng(100 + B)
    x = rng.random((B, n))
    x[:, 5] = 0.25; x[:, 77] = 0.0; x[:, 3000] = 1.0                                           # constant columns
    x[:, 10:40] = np.round(x[:, 10:40] * 4) / 4                                                # ties
    mean, sd, quant = mmm.replicate_summary(x, Q5)
    rm, rs, rq = br.summary(x, Q5)
    const = [5, 77, 3000]
    np.testing.assert_allclose(mean, rm, rtol=1e-12)
    np.testing.assert_allclose(sd, rs, rtol=1e-10, atol=1e-16)
    assert np.all(np.abs(sd[const]) <= 1e-16)
    np.testing.assert_allclose(quant, rq, rtol=0, atol=1e-15)
    assert np.array_equal(quant[0], x.min(axis=0)) and np.array_equal(quant[4], x.max(axis=0))
    if B == 1:
        assert not sd.any()
    # a NaN anywhere in a column gives NaN in all its outputs, and only there
    y = x.copy(); y[B // 2, 123] = np.nan
    mean, sd, quant = mmm.replicate_summary(y, Q5)
    assert np.isnan(mean[123]) and np.isnan(sd[123]) and np.isnan(quant[:, 123]).all()
    keep = np.arange(n) != 123
    assert np.array_equal(mean[keep], mmm.replicate_summary(x, Q5)[0][keep]) and not np.isnan(quant[:, keep]).any()


def test_summary_limits_and_null_outputs(mmm):
    L, ctx = mmm.lib(), mmm.default_context()
    x = np.random.default_rng(1).random((4097, 3))
    with pytest.raises(mmm.MmmError, match="status -4"):
        mmm.replicate_summary(x, [0.5])
    with pytest.raises(mmm.MmmError, match="status -1"):
        mmm.replicate_summary(x[:10], [1.5])
    x = np.ascontiguousarray(x[:9]); sd = np.zeros(3)
    assert L.mmm_replicate_summary(ctx.h, 9, 3, x.ctypes.data, 0, None, None, sd.ctypes.data, None) == 0
    np.testing.assert_allclose(sd, x.std(axis=0, ddof=1), rtol=1e-10)
    m3, s3, q3 = mmm.replicate_summary(np.random.default_rng(2).random((6, 2, 5)), [0.5])      # trailing axes keep their shape
    assert m3.shape == (2, 5) and q3.shape == (1, 2, 5)


# ------------------------------------------------------------------------------------------------------------ 3. LDA composition
def _check_summary(res, q):
    rm, rs, rq = br.summary(res.replicates, q)
    np.testing.assert_allclose(res.mean, rm, rtol=1e-12)
    np.testing.assert_allclose(res.sd, rs, rtol=1e-10, atol=1e-16)
    np.testing.assert_allclose(res.quantiles, rq, rtol=0, atol=1e-15)


def _lda_composition(mmm, oracle):
    g, _, Xn = _lda_pair(mmm, oracle)
    D, B, maxiter, tol = len(Xn), 48, 40, 1e-5
    beta0 = g.β.copy()
    reps = br.resample(Xn, B, SEED)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = mmm.bootstrap_exposures(g, Xn, B, SEED, q=Q5, maxiter=maxiter, tol=tol, init_seed=7, return_replicates=True)
        th = mmm.transform(g, br.stack(reps), maxiter=maxiter, tol=tol, seed=7)
        assert res.replicates.shape == (B, g.K, D) and res.mean.shape == (g.K, D) and res.quantiles.shape == (5, g.K, D)
        assert len(res.n_iter) == 1 and res.B == B
        for b in range(B):
            assert np.array_equal(res.replicates[b], th[:, b * D:(b + 1) * D]), "replicate %d differs from transform on the stack" % b
        _check_summary(res, Q5)
        # batch = 16: three transform calls on the three 16-replicate stacks
        res16 = mmm.bootstrap_exposures(g, Xn, B, SEED, q=Q5, batch=16, maxiter=maxiter, tol=tol, init_seed=7, return_replicates=True)
        assert len(res16.n_iter) == 3 and len(res16.converged) == 3
        for c in range(3):
            thc = mmm.transform(g, br.stack(reps[16 * c:16 * (c + 1)]), maxiter=maxiter, tol=tol, seed=7)
            for b in range(16):
                assert np.array_equal(res16.replicates[16 * c + b], thc[:, b * D:(b + 1) * D]), "chunk %d replicate %d" % (c, b)
        _check_summary(res16, Q5)
    assert res.replicates.min() >= 0 and np.allclose(res.replicates.sum(axis=1), 1.0, rtol=1e-12)
    assert np.array_equal(g.β, beta0)
    return g


def test_lda_bootstrap_is_the_composition(mmm, oracle):
    _lda_composition(mmm, oracle)


def test_lda_bootstrap_is_the_composition_on_dense_row_handles(mmm, oracle, tuning):
    """the forced dense-row build: the 16-bit count rows of the stacked handle see the zero counts that resampling leaves"""
    tuning(lda_build="dense")
    _lda_composition(mmm, oracle)


# ------------------------------------------------------------------------------------------------------------ 4. MMCTM composition
@pytest.mark.filterwarnings("ignore:bootstrap_exposures")
def test_mmctm_bootstrap_is_the_composition(mmm, oracle):
    g, _, Xn, K, V, alpha = _ctm_trained(mmm, oracle)
    D, B, MK = len(Xn), 24, sum(K)
    phi0 = g._get("phi").copy()
    reps = br.resample_mm(Xn, B, SEED)
    # empty modalities stay empty in every replicate
    empties = [(d, m) for d in range(D) for m in range(2) if Xn[d][m].shape[0] == 0]
    assert empties and all(reps[b][d][m].shape == (0, 2) for b in range(B) for d, m in empties)
    # maxiter = 8 ends before the stopping rule may fire (> 10 passes): the chunks report converged = False and warn
    res = mmm.bootstrap_exposures(g, Xn, B, SEED, q=Q5, maxiter=8, init_seed=5, return_replicates=True)
    new = mmm.transform(g, br.stack(reps), maxiter=8, fit_gaussian=False, seed=5)
    props = new._get("props").reshape(B * D, MK).T                                           # ΣK x (B D), modality-major rows
    assert res.replicates.shape == (B, MK, D) and res.n_iter == [len(new.ll_history)]
    for b in range(B):
        assert np.array_equal(res.replicates[b], props[:, b * D:(b + 1) * D]), "replicate %d differs from transform on the stack" % b
    _check_summary(res, Q5)
    res8 = mmm.bootstrap_exposures(g, Xn, B, SEED, q=Q5, batch=8, maxiter=8, init_seed=5, return_replicates=True)
    for c in range(3):
        newc = mmm.transform(g, br.stack(reps[8 * c:8 * (c + 1)]), maxiter=8, fit_gaussian=False, seed=5)
        pc = newc._get("props").reshape(8 * D, MK).T
        for b in range(8):
            assert np.array_equal(res8.replicates[8 * c + b], pc[:, b * D:(b + 1) * D]), "chunk %d replicate %d" % (c, b)
    # props of each modality are proportions
    np.testing.assert_allclose(res.replicates[:, :K[0]].sum(axis=1), 1.0, rtol=1e-12)
    assert np.array_equal(g._get("phi"), phi0)


# ------------------------------------------------------------------------------------------------------------ 5. sanity
def test_point_estimate_lies_within_its_replicates(mmm, oracle):
    g, _, Xn = _lda_pair(mmm, oracle)
    res = mmm.bootstrap_exposures(g, Xn, 100, SEED, return_replicates=True)
    point = mmm.transform(g, Xn)
    lo, hi = res.replicates.min(axis=0), res.replicates.max(axis=0)
    inside = float(np.mean((point >= lo) & (point <= hi)))
    inside95 = float(np.mean((point >= res.quantiles[0]) & (point <= res.quantiles[2])))
    print("point estimate inside [min, max] of 100 replicates: %.4f of %d cells; inside the 2.5-97.5 %% interval: %.4f; passes %s; mean sd %.4f"
          % (inside, point.size, inside95, res.n_iter, res.sd.mean()))
    assert inside >= 0.95
    assert res.converged == [True]


def test_more_mutations_give_narrower_intervals(mmm, oracle):
    g, _, _ = _lda_pair(mmm, oracle)
    sds = []
    for mean_n in (500, 5000):
        X, _ = np_ref.synth_lda(70, 96, 6, seed=104, mean_n=mean_n)
        sds.append(float(mmm.bootstrap_exposures(g, X, 100, SEED).sd.mean()))
    print("mean sd of the exposures: mean_n = 500: %.5f, mean_n = 5000: %.5f" % tuple(sds))
    assert sds[1] < sds[0]


# ------------------------------------------------------------------------------------------------------------ 6. errors
def test_errors_and_the_trained_model_is_untouched(mmm, oracle):
    g, _, Xn = _lda_pair(mmm, oracle)
    beta0, lam0 = g.β.copy(), g.λ.copy()
    with pytest.raises(ValueError):
        mmm.bootstrap_exposures(g, Xn, 0, SEED)
    feats = np.stack([np.arange(96) // 16 + 1, np.arange(96) % 16 + 1], axis=1)
    il = mmm.ILDA(4, 0.1, [0.1, 0.1], feats, Xn, seed=1)
    with pytest.raises(TypeError):
        mmm.bootstrap_exposures(il, Xn, 4, SEED)
    Xm, _ = np_ref.synth_mm(10, [96], [3], seed=2, means=[300])
    im = mmm.IMMCTM([3], [0.1], [feats], Xm, seed=1)
    with pytest.raises(TypeError):
        mmm.bootstrap_exposures(im, Xm, 4, SEED)
    # the C entry: negative count, decreasing doc_ptr, negative B / b0 -> MMM_ERR_ARG; N_d >= 2^31 -> MMM_ERR_UNSUPPORTED
    L, ctx = mmm.lib(), mmm.default_context()
    dp = np.array([0, 2, 3], np.int64); out = np.zeros(3 * 2, np.int32)

    def call(dp, cnt, B=2, b0=0):
        cnt = np.ascontiguousarray(cnt, np.int32)
        return L.mmm_resample_counts(ctx.h, len(dp) - 1, np.ascontiguousarray(dp, np.int64), cnt.ctypes.data, B, b0, 1, 0, out.ctypes.data)
    assert call(dp, [3, -1, 2]) == -1
    assert call(np.array([0, 2, 1], np.int64), [3, 1, 2]) == -1
    assert call(dp, [3, 1, 2], B=-1) == -1 and call(dp, [3, 1, 2], b0=-1) == -1
    assert call(dp, [2 ** 31 - 1, 1, 2]) == -4
    assert call(dp, [3, 1, 2], B=0) == 0 and not out.any()
    assert call(dp, [3, 1, 2]) == 0 and out.reshape(2, 3)[:, :2].sum(axis=1).tolist() == [4, 4] and out.reshape(2, 3)[:, 2].tolist() == [2, 2]
    # the trained model is as it was and goes on training
    mmm.bootstrap_exposures(g, Xn, 8, SEED)
    assert np.array_equal(g.β, beta0) and np.array_equal(g.λ, lam0)
    twin, _, _ = _lda_pair(mmm, oracle)                 # the same training, no bootstrap in between
    assert np.array_equal(twin.λ, lam0)
    ll = mmm.fit(g, maxiter=3, tol=0.0, verbose=False)
    ll_twin = mmm.fit(twin, maxiter=3, tol=0.0, verbose=False)
    assert np.array_equal(ll, ll_twin) and np.array_equal(g.λ, twin.λ) and np.array_equal(g.θ, twin.θ)
