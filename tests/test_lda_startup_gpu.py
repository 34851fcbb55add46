"""Start-up loads of the single-step LDA pass (k_lda_estep_block, k_lda_estep, the ll blocks of k_lda_reduce_ll_mstep): every load of a block's
first third leaves in one group -- unconditional, at clamped indices (document 0 for a lane past D, topic K - 1, table entry K V - 1), the masks
applied where the values are used -- and the stop flag is a vector load consumed ahead of the first store.  What that can break, at the smallest
shapes at which it can:
  * a lane past D reads somebody's row and must add nothing (D = 1, 3, 37: a wave with one, three and one live document group; every corpus
    form; V = 96 / K = 10 and V = 50 / K = 7: run-time stride, padded topic, slots past V);
  * the 16-byte load of the last document's last lane ends inside the rows' allocation (D = 4 n, 16-bit rows);
  * passes enqueued beyond the stop leave the handle as the stopping pass left it (the test of the flag now stands later in the ll blocks);
  * a mask applied to the wrong chunk after the loads were regrouped: the four corpus forms give the same fit.
Bounds are the project's: ll, γ, λ, Elnβ, ELBO at 1e-9 relative, ϕ / θ at 1e-5 against the C oracle after 12 passes with tol = 0."""
import numpy as np
import pytest

import np_ref

pytestmark = pytest.mark.gpu

PASSES = 12
# corpus form -> what is switched off to get it: rows of 16-bit counts (default), rows of 32-bit counts, padded (term,count) rows, CSR
FORMS = {"rows16": (), "rows32": ("lda_rows16",), "pairs": ("lda_count_rows",), "csr": ("lda_padded_rows", "lda_count_rows")}
ARRAYS = ("ll", "gamma", "lambda", "Elnbeta", "phi", "theta")

_cache = {}


def _case(oracle, D, V, K, seed=900):
    """corpus, initial λ and the oracle's 12 passes: computed once per shape, shared, never written to"""
    key = (D, V, K, seed)
    if key not in _cache:
        X, lam0 = np_ref.synth_lda(D, V, K, seed=seed + D + V, mean_n=300)
        o = oracle.LdaOracle(K, 0.1, 0.1, X, V=V, lambda0=lam0)
        o.fit(maxiter=PASSES, tol=0.0)
        _cache[key] = (X, lam0, o)
    return _cache[key]


def _state(g, ll):
    return {"ll": np.asarray(ll).copy(), "gamma": g.γ.copy(), "lambda": g.λ.copy(), "Elnbeta": g.Elnβ.copy(), "phi": g.phi_flat().copy(),
            "theta": g.θ.copy(), "elbo": np.float64(g.elbo)}


def _fit(mmm, tuning, X, lam0, K, V, form, **tune):
    tuning(disable=FORMS[form] + tuple(tune.pop("disable", ())), **tune)
    g = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lam0)
    geo = g.geometry()
    assert geo["single_step"] == 1, geo
    return _state(g, mmm.fit(g, maxiter=PASSES, tol=0.0, verbose=False)), geo


def _hold(r, o, D, V, K):
    np.testing.assert_allclose(r["ll"], o.ll_hist, rtol=1e-9)
    np.testing.assert_allclose(r["gamma"], o.gamma.reshape(D, K).T, rtol=1e-9)
    np.testing.assert_allclose(r["lambda"], o.lam.reshape(K, V).T, rtol=1e-9)
    np.testing.assert_allclose(r["Elnbeta"], o.Elnbeta.reshape(K, V).T, rtol=1e-9, atol=1e-12)
    assert r["elbo"] == pytest.approx(o.elbo_value, rel=1e-9)
    np.testing.assert_allclose(r["phi"], o.phi.reshape(-1, K), rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(r["theta"], o.theta.reshape(D, K).T, rtol=1e-5)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("V,K", [(96, 10), (50, 7)])
@pytest.mark.parametrize("D", [1, 3, 37])
def test_documents_past_D_add_nothing(mmm, oracle, tuning, D, V, K, form):
    X, lam0, o = _case(oracle, D, V, K)
    r, geo = _fit(mmm, tuning, X, lam0, K, V, form)
    assert geo["block_stats"] == 1, geo
    print("\n(D, V, K) = (%d, %d, %d) %s: row_bytes %d, largest relative distance to the oracle: ll %.3g gamma %.3g lambda %.3g" % (
        D, V, K, form, geo["row_bytes"], np.max(np.abs(r["ll"] / o.ll_hist - 1)), np.max(np.abs(r["gamma"] / o.gamma.reshape(D, K).T - 1)),
        np.max(np.abs(r["lambda"] / o.lam.reshape(K, V).T - 1))))
    _hold(r, o, D, V, K)
    again, _ = _fit(mmm, tuning, X, lam0, K, V, form)
    for k in ARRAYS:
        np.testing.assert_array_equal(r[k], again[k], err_msg="the second run does not repeat the first: " + k)
    assert r["elbo"] == again["elbo"]


@pytest.mark.parametrize("D", [4, 52])
def test_last_row_ends_the_allocation(mmm, oracle, tuning, D):
    """D = 4 n documents over 16-bit rows: lane 15 of the last document group requests the last 16 bytes the rows' allocation was given to spare
    (12 bytes of its 6 slots + 4).  D = 52: the last group of a second block."""
    V, K = 96, 10
    X, lam0, o = _case(oracle, D, V, K)
    r, geo = _fit(mmm, tuning, X, lam0, K, V, "rows16")
    assert geo["row_bytes"] == 2 * 96, geo          # 16-bit counts
    np.testing.assert_allclose(r["gamma"][:, D - 1], o.gamma.reshape(D, K).T[:, D - 1], rtol=1e-9)
    _hold(r, o, D, V, K)


@pytest.mark.parametrize("disable", [(), ("lda_merged",), ("lda_early_prologue",)])
def test_passes_beyond_the_stop_leave_the_handle_alone(mmm, tuning, disable):
    """fit(maxiter = 200, tol = 1e-4) enqueues passes well beyond the one that meets the stopping rule; each of them finds the flag set.  Afterwards
    ll history, γ, λ, Elnβ, θ and Elnθ (the slot the merged launch's early prologue writes) are bit-equal to a fresh handle run for exactly len(ll) passes with tol = 0: a deferred test of the flag that stood
    behind a store would have written pass t + 1's state into the stopped handle without any error.
    Then three more passes through mmm_lda_iterate.  That call clears the flag (a handle that stopped can be iterated further: lda.hip,
    mmm_lda_iterate), so the arrays do move -- to exactly where len(ll) + 3 passes of a fresh handle end: whatever the no-op launches had touched
    would show there as well."""
    D, V, K = 300, 96, 4
    X, lam0 = np_ref.synth_lda(D, V, K, seed=508, mean_n=400)
    tuning(disable=disable)
    g = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lam0)
    ll = np.asarray(mmm.fit(g, maxiter=200, tol=1e-4, verbose=False))
    assert g.converged and 11 <= len(ll) < 200, len(ll)       # the rule fired, with no-op passes enqueued behind it
    got = {"ll": ll.copy(), "gamma": g.γ.copy(), "lambda": g.λ.copy(), "Elnbeta": g.Elnβ.copy(), "theta": g.θ.copy(), "Elntheta": g.Elnθ.copy()}
    f = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lam0)
    want_ll = np.asarray(mmm.fit(f, maxiter=len(ll), tol=0.0, verbose=False))
    want = {"ll": want_ll, "gamma": f.γ.copy(), "lambda": f.λ.copy(), "Elnbeta": f.Elnβ.copy(), "theta": f.θ.copy(), "Elntheta": f.Elnθ.copy()}
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="stopped handle vs %d passes of a fresh one: %s" % (len(ll), k))
    mmm._lib.check(mmm.lib().mmm_lda_iterate(g._h, 3), g.ctx.h, "iterate")
    mmm._lib.check(mmm.lib().mmm_lda_iterate(f._h, 3), f.ctx.h, "iterate")
    for k, a, b in (("gamma", g.γ, f.γ), ("lambda", g.λ, f.λ), ("Elnbeta", g.Elnβ, f.Elnβ), ("theta", g.θ, f.θ), ("Elntheta", g.Elnθ, f.Elnθ)):
        np.testing.assert_array_equal(a, b, err_msg="three passes on from the stop: " + k)


def test_every_corpus_form_gives_the_same_fit(mmm, oracle, tuning):
    """One corpus under the four forms (a ragged last wave, an empty and a one-term document): each within the oracle's bounds, ll histories within
    1e-12 relative of each other (the forms differ in which slots are visited, not in any sum's order over the visited ones)."""
    D, V, K = 101, 96, 10
    X, lam0 = np_ref.synth_lda(D, V, K, seed=930, mean_n=300)
    X[7] = np.zeros((0, 2), dtype=np.int64)
    X[8] = X[8][:1].copy()
    o = oracle.LdaOracle(K, 0.1, 0.1, X, V=V, lambda0=lam0)
    o.fit(maxiter=PASSES, tol=0.0)
    runs = {}
    for form in FORMS:
        runs[form], geo = _fit(mmm, tuning, X, lam0, K, V, form)
        assert geo["block_stats"] == 1, geo
        _hold(runs[form], o, D, V, K)
    ref = runs["rows16"]["ll"]
    for form, r in runs.items():
        print("\n%s: largest relative ll distance to rows16 %.3g" % (form, np.max(np.abs(r["ll"] / ref - 1))))
        np.testing.assert_allclose(r["ll"], ref, rtol=1e-12, err_msg=form)
