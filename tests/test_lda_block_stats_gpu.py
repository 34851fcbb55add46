"""Single-step LDA E-step with the block's λ statistics as a product (k_lda_estep_block: S_kv = B_kv Σ_d a_dk r_dv, no LDS atomics, no
per-wave slabs) and the slab build it replaces (`disable=("lda_block_stats",)`, k_lda_estep): EACH is held against the C oracle after 12
fused passes with tol = 0 at the project's bounds -- ll history, γ, λ, Elnβ and ELBO at 1e-9 relative, ϕ / θ at 1e-5 -- and the new build
must repeat itself bit for bit.  The largest relative distance between the two builds is printed per array (run with -s), not asserted:
they associate the cross-document sums differently, and each has its own bound against the oracle.
Shapes are the smallest that reach every path of the kernel: ragged last wave, empty / one-term documents, a padded topic with the generic
row stride, K = 1 / 2 / 12, (term,count) rows and CSR with most terms absent (the zero fill of r), 1 / 3 / 12 waves per block, a block
count pinned by geometry_cus, and a corpus with a term listed twice, which must keep the slab build."""
import numpy as np
import pytest

import np_ref

pytestmark = pytest.mark.gpu

PASSES = 12


def _corpus(D, V, K, seed, mean_n=400):
    return np_ref.synth_lda(D, V, K, seed=seed, mean_n=mean_n)


def _fit(mmm, tuning, X, lam0, K, V, off, want_block, disable=(), **tune):
    tuning(disable=tuple(disable) + (("lda_block_stats",) if off else ()), **tune)
    g = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lam0)
    geo = g.geometry()
    assert geo["single_step"] == 1, geo
    assert geo["block_stats"] == (0 if off else want_block), geo
    ll = np.array(mmm.fit(g, maxiter=PASSES, tol=0.0, verbose=False))
    return {"ll": ll, "gamma": g.γ.copy(), "lambda": g.λ.copy(), "Elnbeta": g.Elnβ.copy(), "elbo": np.float64(g.elbo),
            "phi": g.phi_flat().copy(), "theta": g.θ.copy(), "geo": geo}


def _hold(r, o, D, V, K):
    np.testing.assert_allclose(r["ll"], o.ll_hist, rtol=1e-9)
    np.testing.assert_allclose(r["gamma"], o.gamma.reshape(D, K).T, rtol=1e-9)
    np.testing.assert_allclose(r["lambda"], o.lam.reshape(K, V).T, rtol=1e-9)
    np.testing.assert_allclose(r["Elnbeta"], o.Elnbeta.reshape(K, V).T, rtol=1e-9, atol=1e-12)
    assert r["elbo"] == pytest.approx(o.elbo_value, rel=1e-9)
    np.testing.assert_allclose(r["phi"], o.phi.reshape(-1, K), rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(r["theta"], o.theta.reshape(D, K).T, rtol=1e-5)


def _distance(a, b):
    out = {}
    for k in ("ll", "gamma", "lambda", "Elnbeta", "phi", "theta"):
        den = np.maximum(np.abs(b[k]), 1e-300)
        out[k] = float(np.max(np.abs(a[k] - b[k]) / den)) if a[k].size else 0.0
    out["elbo"] = float(abs(a["elbo"] - b["elbo"]) / abs(b["elbo"]))
    return out


def _both_paths(mmm, oracle, tuning, X, lam0, D, V, K, want_block=1, disable=(), **tune):
    o = oracle.LdaOracle(K, 0.1, 0.1, X, V=V, lambda0=lam0)
    o.fit(maxiter=PASSES, tol=0.0)
    new = _fit(mmm, tuning, X, lam0, K, V, False, want_block, disable, **tune)
    old = _fit(mmm, tuning, X, lam0, K, V, True, want_block, disable, **tune)
    print("\n(D, V, K) = (%d, %d, %d) %s: largest relative distance block product vs slabs: %s" % (D, V, K, dict(tune, disable=disable), _distance(new, old)))
    _hold(new, o, D, V, K)
    _hold(old, o, D, V, K)
    again = _fit(mmm, tuning, X, lam0, K, V, False, want_block, disable, **tune)
    for k in ("ll", "gamma", "lambda", "Elnbeta", "phi", "theta"):
        np.testing.assert_array_equal(new[k], again[k], err_msg="the block-product build does not repeat its bits: " + k)
    assert new["elbo"] == again["elbo"]
    assert all(new["geo"][k] == old["geo"][k] for k in ("L", "grid_e", "waves_e", "KP", "row_bytes")), (new["geo"], old["geo"])
    return new, old


def test_ragged_block_with_an_empty_and_a_one_term_document(mmm, oracle, tuning):
    """37 documents: a ragged last wave (one document of four), the VT = 96 build; document 5 empty, document 6 a single term."""
    D, V, K = 37, 96, 10
    X, lam0 = _corpus(D, V, K, seed=501)
    X[5] = np.zeros((0, 2), dtype=np.int64)
    X[6] = X[6][:1].copy()
    _both_paths(mmm, oracle, tuning, X, lam0, D, V, K)


def test_padded_topic_and_generic_stride(mmm, oracle, tuning):
    """K = 7 runs as KP = 8 with a padded topic; V = 50 takes the run-time row stride and rows of 64 slots (14 of them past V)."""
    D, V, K = 300, 50, 7
    X, lam0 = _corpus(D, V, K, seed=502)
    new, _ = _both_paths(mmm, oracle, tuning, X, lam0, D, V, K)
    assert new["geo"]["KP"] == 8


@pytest.mark.parametrize("D,V,K", [(120, 96, 12), (64, 5, 2), (20, 30, 1)])
def test_topic_count_extremes(mmm, oracle, tuning, D, V, K):
    X, lam0 = _corpus(D, V, K, seed=503 + K)
    _both_paths(mmm, oracle, tuning, X, lam0, D, V, K)


def test_csr_rows_with_most_terms_absent(mmm, oracle, tuning):
    """No padded rows, no rows of counts: the kernel walks doc_ptr -> (term, count) and visits the listed terms only, so every other r must
    be the zero it filled in (about 30 draws over 96 terms: most cells)."""
    D, V, K = 200, 96, 10
    X, lam0 = _corpus(D, V, K, seed=504, mean_n=30)
    new, _ = _both_paths(mmm, oracle, tuning, X, lam0, D, V, K, disable=("lda_padded_rows", "lda_count_rows"))
    assert new["geo"]["row_bytes"] in (0, 8 * V)      # no rows of counts


@pytest.mark.parametrize("waves", [1, 3, 12])
def test_waves_per_block(mmm, oracle, tuning, waves):
    """1 and 3 waves: the table does not fit the registers that carry it to the barrier, the product loops over (v, topic pair); 12: 48 documents."""
    D, V, K = 100, 96, 10
    X, lam0 = _corpus(D, V, K, seed=505)
    new, _ = _both_paths(mmm, oracle, tuning, X, lam0, D, V, K, waves_per_block=waves)
    assert new["geo"]["waves_e"] == waves


def test_two_pretended_cus(mmm, oracle, tuning):
    D, V, K = 96, 96, 10
    X, lam0 = _corpus(D, V, K, seed=506)
    new, _ = _both_paths(mmm, oracle, tuning, X, lam0, D, V, K, geometry_cus=2)
    assert new["geo"]["grid_e"] == 2 and new["geo"]["waves_e"] == 12


def test_duplicate_term_keeps_the_slab_build(mmm, oracle, tuning):
    """A document that lists a term twice would store two r into one cell: the handle must report the slab build, and fit to the oracle."""
    D, V, K = 50, 96, 10
    X, lam0 = _corpus(D, V, K, seed=507)
    X[11] = np.concatenate([X[11], np.array([[X[11][0, 0], 3]], dtype=np.int64)])
    _both_paths(mmm, oracle, tuning, X, lam0, D, V, K, want_block=0)


def test_stopping_rule(mmm, oracle, tuning):
    """fit!(maxiter = 200, tol = 1e-4): the same number of passes and the same `converged` as the oracle, on both builds."""
    D, V, K = 300, 96, 4
    X, lam0 = _corpus(D, V, K, seed=508)
    o = oracle.LdaOracle(K, 0.1, 0.1, X, V=V, lambda0=lam0)
    ll_o = o.fit(maxiter=200, tol=1e-4)
    for off in (False, True):
        tuning(disable=("lda_block_stats",) if off else ())
        g = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lam0)
        assert g.geometry()["block_stats"] == (0 if off else 1)
        ll = mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
        assert len(ll) == len(ll_o) and g.converged == o.converged
        np.testing.assert_allclose(ll, ll_o, rtol=1e-9)
