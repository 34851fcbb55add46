"""The C oracle's LDA frozen-topic inference (LdaOracle.transform / fit_heldout / _infer, oracle/mmm_oracle.c) against tests/lda_infer_ref.py,
the numpy restatement of LDA.jl:226-295 in extended precision, on every case of lda_infer_ref.cases() and in both modes -- and the
conditions that keep tests/test_lda_infer_dispatch_gpu.py, which holds the device to the same restatement on the same cases, from hiding
a failure: every case has its edge documents, no θ is so small that a relative bound says nothing, and no stopped run ends on a pass whose
stop ratio is within 5 % of the tolerance.  No GPU: the topics are trained by the oracle here (by the device there).

Bound: rtol 1e-11 on everything (ϕ with atol 1e-300).  The oracle sums in double: a sum over W <= 300 terms is off by at most W 2^-53 =
3e-14, the passes do not compound (each is a contraction towards the fixed point) but ϕ is the exponential of Elnθ, |Elnθ| <= 30, so a
rounding of the exponent weighs 30 times in ϕ: 12 x 3e-14 x 30 = 1e-11.

Largest relative gaps measured, oracle against restatement over all 43 cases (printed by the last test):
    12 passes at tol = 0    ll 1.9e-14   γ 4.4e-14   θ 4.4e-14   ϕ 2.9e-13   ELBO 1.7e-12
    stopped at tol = 1e-4   ll 1.9e-14   γ 1.3e-13   θ 1.3e-13   ϕ 7.7e-13   ELBO 1.1e-13   (11 to 25 passes)
smallest θ 1.5e-6 (the document holding a count of 65536); the stop ratio nearest to tol = 1e-4 after the 10th pass is 5.5 % of tol away.
A corpus of ONE document (s16_k2_v50_d1) cannot hold an empty, a one-entry and a zero-count document: it is the zero-count one."""
import numpy as np
import pytest

import lda_infer_ref as ref
from lda_infer_ref import dist

CASES = ref.cases()
IDS = [c["name"] for c in CASES]
BOUND = 1e-11
TOL, MAXITER = 1e-4, 200
GAPS = {}               # (run, quantity) -> largest gap
SEEN = {"theta_min": 1.0, "margin": np.inf, "passes": []}
_TRAINED = {}


def trained(oracle, c):
    """The case's topics: TRAIN_PASSES oracle passes over the training corpus."""
    if c["name"] not in _TRAINED:
        o = oracle.LdaOracle(c["K"], c["alpha"], c["eta"], c["Xt"], V=c["V"], lambda0=c["lam0"])
        o.fit(maxiter=ref.TRAIN_PASSES, tol=0.0)
        _TRAINED[c["name"]] = o
    return _TRAINED[c["name"]]


def tables(o):
    V, K = o.V, o.K
    return o.lam.reshape(V, K, order="F"), o.beta.reshape(V, K, order="F"), o.Elnbeta.reshape(V, K, order="F")


def put(run, what, v):
    GAPS[(run, what)] = max(GAPS.get((run, what), 0.0), v)


def compare(run, name, new, r, elbo=None):
    """The oracle model `new` after its run against the restatement's Run r."""
    K, D = new.K, new.D
    assert len(new.ll_hist) == len(r.ll) and new.converged == r.converged, (name, len(new.ll_hist), len(r.ll), new.converged, r.converged)
    w = dict(ll=dist(new.ll_hist, r.ll), γ=dist(new.gamma.reshape(D, K).T, r.gamma), θ=dist(new.theta.reshape(D, K).T, r.theta),
             ϕ=dist(new.phi.reshape(-1, K), ref.phi_rows(r.phi), atol=1e-300))
    if elbo is not None:
        w["ELBO"] = dist(elbo, r.model.elbo_terms()[0])
    for k, v in w.items():
        put(run, k, v)
        assert v <= BOUND, "%s %s: %s differs by %.3g (bound %g)" % (name, run, k, v, BOUND)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_cases_carry_their_edge_documents(c):
    assert ref.has_edge_documents(c)
    assert all(x.shape[0] == 0 or (1 <= x[:, 0].min() and x[:, 0].max() <= c["V"] and x[:, 1].min() >= 0) for x in c["Xn"])
    assert len(c["Xn"]) == c["D"] and c["mean_n"] <= 500
    W = np.array([x.shape[0] for x in c["Xn"]])
    if c["name"] == "csr_v300_k5":                   # rows beyond the prefetched 96 entries of a 16-lane group, and beyond twice that
        assert ((W > 96) & (W <= 192)).any() and (W > 192).any()
    if c["name"] == "csr_dup_v24_k6":
        assert any(len(set(x[:, 0])) < x.shape[0] for x in c["Xn"]) and W.max() > c["V"]
    if c["name"] == "s32_k10_v96_bigcount":
        assert max(int(x[:, 1].max()) for x in c["Xn"] if x.shape[0]) >= 65536


@pytest.mark.parametrize("unsmoothed", [True, False], ids=["unsmoothed", "smoothed"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_twelve_passes(oracle, c, unsmoothed):
    """12 passes at tol = 0: ll history, γ, θ, ϕ and the ELBO."""
    o = trained(oracle, c)
    lam, beta, Elnbeta = tables(o)
    if unsmoothed:
        _, new = o.transform(c["Xn"], maxiter=ref.PASSES, tol=0.0)
        lam_n, Eln_n = new.lam.reshape(o.V, o.K, order="F"), new.Elnbeta.reshape(o.V, o.K, order="F")     # the constructor's own (LDA.jl:36-39)
    else:
        new = oracle.LdaOracle(o.K, o.alpha, o.eta, c["Xn"], V=o.V, seed=1)
        new.lam[:] = o.lam; new.beta[:] = o.beta; new.Elnbeta[:] = o.Elnbeta
        new._infer(False, ref.PASSES, 0.0)
        lam_n, Eln_n = lam, Elnbeta
    r = ref.infer(c["Xn"], c["K"], c["alpha"], beta, Eln_n, lam_n, unsmoothed, ref.PASSES, 0.0, eta=c["eta"])
    assert len(r.ll) == ref.PASSES and not r.converged
    compare("12 passes", c["name"], new, r, elbo=new.elbo()[0])
    SEEN["theta_min"] = min(SEEN["theta_min"], float(r.theta.min()))
    assert r.theta.min() >= 1e-6, "%s: a θ of %.3g: relative bounds on θ say little there" % (c["name"], r.theta.min())
    np.testing.assert_allclose(r.gamma.sum(axis=0), c["K"] * c["alpha"] + r.model.N, rtol=1e-13)


@pytest.mark.parametrize("unsmoothed", [True, False], ids=["unsmoothed", "smoothed"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_stopped_run(oracle, c, unsmoothed):
    """tol = 1e-4: the same number of passes and `converged`, and the pass count does not hinge on a last-bit difference."""
    o = trained(oracle, c)
    lam, beta, Elnbeta = tables(o)
    if unsmoothed:
        _, new = o.transform(c["Xn"], maxiter=MAXITER, tol=TOL)
    else:
        new = o.fit_heldout(c["Xn"], maxiter=MAXITER)              # tol = 1e-4 (LDA.jl:286)
    r = ref.infer(c["Xn"], c["K"], c["alpha"], beta, Elnbeta, lam, unsmoothed, MAXITER, TOL, eta=c["eta"])
    compare("stopped", c["name"], new, r, elbo=None if unsmoothed else new.elbo_value)
    assert r.converged and 11 <= len(r.ll) < MAXITER
    margin = float(np.abs(r.ratio[10:] / TOL - 1.0).min())
    SEEN["margin"] = min(SEEN["margin"], margin); SEEN["passes"].append(len(r.ll))
    assert margin >= 0.05, "%s: a stop ratio %.3g of tol away from it: choose another corpus seed" % (c["name"], margin)


def test_zz_largest_gaps():
    """Runs last: the largest oracle-against-restatement gap per quantity (the figures of the docstring)."""
    for run in ("12 passes", "stopped"):
        print("\n%-10s %s" % (run, "  ".join("%s %.1e" % (k, v) for (r, k), v in sorted(GAPS.items()) if r == run)))
    if SEEN["passes"]:
        print("smallest θ %.2e; stopped runs took %d to %d passes, the nearest stop ratio %.3f of tol away" %
              (SEEN["theta_min"], min(SEEN["passes"]), max(SEEN["passes"]), SEEN["margin"]))
    assert all(v <= BOUND for v in GAPS.values())
