"""k_lda_estep_block keeps its LDS table as topic pairs ([KP / 2][V][2]) and r as document pairs ([ND / 2][Vs][2]), so that every read of
either is 16 bytes.  The shapes here are the ones at which those two layouts can go wrong and that test_lda_block_stats_gpu.py does not
hold: a padded topic inside the last pair of the VT = 96 build with an odd document count (the last document pair half empty), KP = 12 at a
run-time stride that is no multiple of 16, 4 and 8 documents per block (the table staged by the loop, not from registers), rows of 32-bit
counts, padded (term,count) rows, CSR (zero fill and scattered r stores) and a 3-replica batch.  Bounds as in that file: 12 fused passes
with tol = 0 against the C oracle -- ll history, γ, λ, Elnβ and ELBO at 1e-9 relative, ϕ / θ at 1e-5 -- and the fit repeated once must
repeat its bits; every replica of the batch equals its single fit bit for bit."""
import numpy as np
import pytest

import np_ref

pytestmark = pytest.mark.gpu

PASSES = 12
ARRAYS = ("ll", "gamma", "lambda", "Elnbeta", "phi", "theta")


def _fit(mmm, tuning, X, lam0, K, V, **tune):
    tuning(**tune)
    g = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lam0)
    geo = g.geometry()
    assert geo["single_step"] == 1 and geo["block_stats"] == 1, geo
    ll = np.array(mmm.fit(g, maxiter=PASSES, tol=0.0, verbose=False))
    r = {"ll": ll, "gamma": g.γ.copy(), "lambda": g.λ.copy(), "Elnbeta": g.Elnβ.copy(), "elbo": np.float64(g.elbo),
         "phi": g.phi_flat().copy(), "theta": g.θ.copy(), "geo": geo}
    g.close()
    return r


def _hold(r, o, D, V, K):
    np.testing.assert_allclose(r["ll"], o.ll_hist, rtol=1e-9)
    np.testing.assert_allclose(r["gamma"], o.gamma.reshape(D, K).T, rtol=1e-9)
    np.testing.assert_allclose(r["lambda"], o.lam.reshape(K, V).T, rtol=1e-9)
    np.testing.assert_allclose(r["Elnbeta"], o.Elnbeta.reshape(K, V).T, rtol=1e-9, atol=1e-12)
    assert r["elbo"] == pytest.approx(o.elbo_value, rel=1e-9)
    np.testing.assert_allclose(r["phi"], o.phi.reshape(-1, K), rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(r["theta"], o.theta.reshape(D, K).T, rtol=1e-5)


def _check(mmm, oracle, tuning, X, lam0, D, V, K, **tune):
    o = oracle.LdaOracle(K, 0.1, 0.1, X, V=V, lambda0=lam0)
    o.fit(maxiter=PASSES, tol=0.0)
    new = _fit(mmm, tuning, X, lam0, K, V, **tune)
    _hold(new, o, D, V, K)
    again = _fit(mmm, tuning, X, lam0, K, V, **tune)
    for k in ARRAYS:
        np.testing.assert_array_equal(new[k], again[k], err_msg="the fit does not repeat its bits: " + k)
    assert new["elbo"] == again["elbo"]
    return new


def test_padded_topic_in_the_last_pair_and_a_half_empty_document_pair(mmm, oracle, tuning):
    """K = 9 on the VT = 96 build: topic 9 of the pair (8, 9) is padding; 41 documents: the last pair holds one."""
    D, V, K = 41, 96, 9
    X, lam0 = np_ref.synth_lda(D, V, K, seed=601, mean_n=400)
    new = _check(mmm, oracle, tuning, X, lam0, D, V, K)
    assert new["geo"]["KP"] == 10


def test_twelve_topic_slots_at_a_ragged_run_time_stride(mmm, oracle, tuning):
    """K = 11: KP = 12, the table carried to the barrier in five registers; V = 90: run-time stride, the last chunk of a row has 10 terms."""
    D, V, K = 30, 90, 11
    X, lam0 = np_ref.synth_lda(D, V, K, seed=602, mean_n=400)
    new = _check(mmm, oracle, tuning, X, lam0, D, V, K)
    assert new["geo"]["KP"] == 12


@pytest.mark.parametrize("waves", [1, 2])
def test_two_and_four_document_pairs_per_block(mmm, oracle, tuning, waves):
    """One wave: 4 documents, two pairs, and the table staged by the loop instead of from registers; two waves: 8 documents."""
    D, V, K = 70, 96, 10
    X, lam0 = np_ref.synth_lda(D, V, K, seed=603, mean_n=400)
    new = _check(mmm, oracle, tuning, X, lam0, D, V, K, waves_per_block=waves)
    assert new["geo"]["waves_e"] == waves


def _corpus_with_a_large_count(mean_n):
    D, V, K = 50, 96, 10
    X, lam0 = np_ref.synth_lda(D, V, K, seed=604, mean_n=mean_n)
    X[7] = X[7].copy()
    assert len(X[7]) > 0
    X[7][0, 1] = 70000                         # above 65,535: the rows of counts cannot be 16-bit
    return X, lam0, D, V, K


def test_rows_of_32_bit_counts(mmm, oracle, tuning):
    X, lam0, D, V, K = _corpus_with_a_large_count(400)
    new = _check(mmm, oracle, tuning, X, lam0, D, V, K)
    assert new["geo"]["row_bytes"] == 4 * V, new["geo"]


def test_padded_term_count_rows(mmm, oracle, tuning):
    X, lam0, D, V, K = _corpus_with_a_large_count(400)
    new = _check(mmm, oracle, tuning, X, lam0, D, V, K, disable=("lda_count_rows",))
    assert new["geo"]["row_bytes"] == 8 * V, new["geo"]


def test_csr_zero_fill_and_scattered_r(mmm, oracle, tuning):
    """About 30 draws over 96 terms: most cells of r are the zero the kernel filled in, the others are stored at the terms' own cells."""
    X, lam0, D, V, K = _corpus_with_a_large_count(30)
    new = _check(mmm, oracle, tuning, X, lam0, D, V, K, disable=("lda_padded_rows", "lda_count_rows"))
    assert new["geo"]["row_bytes"] in (0, 8 * V), new["geo"]      # no rows of counts (padded rows, if any, serve the ll blocks only)


def test_batch_replicas_equal_their_single_fits(mmm, tuning):
    D, V, K, R = 37, 96, 10, 3
    X, _ = np_ref.synth_lda(D, V, K, seed=605, mean_n=400)
    rng = np.random.default_rng(606)
    lams = [rng.integers(1, 101, size=(V, K)).astype(np.float64) for _ in range(R)]
    tuning()
    batch = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lams, restarts=R)
    geo = batch.geometry()
    assert geo["single_step"] == 1 and geo["block_stats"] == 1, geo
    hists = mmm.fit_restarts(batch, maxiter=PASSES, tol=0.0)
    assert len(hists) == R
    for r in range(R):
        tuning(disable=("lda_merged",))          # the single handle a replica must equal runs the split pipeline
        g = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lams[r])
        gg = g.geometry()
        assert gg["block_stats"] == 1 and gg["grid_e"] == geo["grid_e"] and gg["waves_e"] == geo["waves_e"], gg
        ll = mmm.fit(g, maxiter=PASSES, tol=0.0, verbose=False)
        batch.select(r)
        assert np.array_equal(hists[r], ll), (r, hists[r], ll)
        assert batch.restart_elbo[r] == g.elbo
        for f in ("λ", "Elnβ", "β", "γ", "Elnθ", "θ"):
            assert np.array_equal(getattr(batch, f), getattr(g, f)), (r, f)
        assert np.array_equal(batch.phi_flat(), g.phi_flat()), r
        g.close()
    batch.close()
