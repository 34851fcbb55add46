"""The C oracle's ILDA (oracle/mmm_oracle.c orc_ilda_*) held to tests/ilda_ref.py, the numpy restatement written from ILDA.jl with
extended-precision sums, on every case of ilda_ref.draw_cases(): feature tables far from the reference's V = 4 toy (one feature, eight
features, a feature of 200 values, sum J = 512, 1536 terms, values no term carries, fewer terms than values).  The GPU tests compare the
device with both; a reading of ILDA.jl shared by oracle and kernels would show here.

Measured 2026-10-16 over the whole list, oracle against ilda_ref, worst relative distance after each of six passes:
ll 1.0e-13, λ 5.5e-13, β 3.7e-13, γ 3.8e-13, θ 3.8e-13, Elnβ 3.3e-13 and Elnθ 1.9e-13 (beyond atol 1e-13), ϕ 1.8e-12, ELBO terms
1.0e-12.  Both sides are double sums of at most a few thousand terms and differ in libm / scipy digamma; the bounds are ten times the
measured worst rounded up to a power of ten (RTOL for the state, RTOL_PHI for ϕ, RTOL_ELBO for the terms, whose sums cancel), never
looser than 1e-10.  The test prints what it saw."""
import numpy as np
import pytest

import ilda_ref
from ilda_ref import dist, heldout_docs, oracle_of

RTOL = 1e-11            # 10 x 5.5e-13 -> 1e-11
RTOL_ELN = 1e-11        # 10 x 3.3e-13 -> 1e-11, with the atol = 1e-13 of test_ilda_gpu.py next to Elnβ's zero
RTOL_PHI = 1e-10        # 10 x 1.8e-12 -> 1e-10
RTOL_ELBO = 1e-10       # 10 x 1.0e-12 = 1.02e-11 -> 1e-10 (the cap)
CASES = ilda_ref.draw_cases()
WORST = {}


def state_dist(o, r, w):
    K, D = r.K, r.D
    for i in range(r.I):
        w["λ"] = max(w.get("λ", 0.0), dist(o.mat(o.lam, i), r.lam[i]))
        w["Elnβ"] = max(w.get("Elnβ", 0.0), dist(o.mat(o.Elnbeta, i), r.Elnbeta[i], atol=1e-13))
        if r.beta is not None:
            w["β"] = max(w.get("β", 0.0), dist(o.mat(o.beta, i), r.beta[i]))
    w["γ"] = max(w.get("γ", 0.0), dist(o.gamma.reshape(D, K).T, r.gamma))
    w["Elnθ"] = max(w.get("Elnθ", 0.0), dist(o.Elntheta.reshape(D, K).T, r.Elntheta, atol=1e-13))
    if r.theta is not None:
        w["θ"] = max(w.get("θ", 0.0), dist(o.theta.reshape(D, K).T, r.theta))
    w["ϕ"] = max(w.get("ϕ", 0.0), max([dist(o.phi_doc(d), r.phi[d], atol=1e-300) for d in range(D)] or [0.0]))
    return w


def check(w, name):
    for k, v in w.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        bound = {"elbo": RTOL_ELBO, "ϕ": RTOL_PHI, "Elnβ": RTOL_ELN, "Elnθ": RTOL_ELN}.get(k, RTOL)
        assert v <= bound, "%s: %s differs by %.3g (bound %g)" % (name, k, v, bound)


def test_case_list_holds_the_tables_each_branch_needs():
    by = {c["name"]: c for c in CASES}
    assert len(by) == len(CASES) == len(ilda_ref.NAMED) + ilda_ref.N_DRAWN and ilda_ref.N_DRAWN >= 12
    for c in CASES:
        f = c["features"]
        assert f.shape == (c["V"], c["I"]) and f.min() >= 1 and [int(j) for j in f.max(axis=0)] == c["J"]
        assert all(x.shape[1] == 2 and (x.size == 0 or (x[:, 0].min() >= 1 and x[:, 0].max() <= c["V"])) for x in c["X"])
    c = by["identity"]; assert c["I"] == 1 and 17 <= c["V"] <= 128 and np.array_equal(c["features"][:, 0], np.arange(1, c["V"] + 1))
    c = by["identity_small"]; assert c["I"] == 1 and c["V"] <= 16 and np.array_equal(c["features"][:, 0], np.arange(1, c["V"] + 1))
    c = by["I8"]; assert c["I"] == 8 and all(2 <= j <= 3 for j in c["J"])
    c = by["bigJ"]; assert c["J"] == [200, 5] and 300 < c["V"] < 600 and 200 in c["features"][:, 0]
    assert len(set(range(1, 201)) - set(c["features"][:, 0])) >= 50 and (c["features"][:, 0] > 64).sum() > 50
    assert sum(by["sj512"]["J"]) == 512 and max(by["sj512"]["J"]) > 64
    c = by["penta"]; assert (c["V"], c["J"], c["K"]) == (1536, [6, 4, 4, 4, 4], 10) and len({tuple(r) for r in c["features"]}) == 1536
    c = by["v257"]; assert 256 < c["V"] <= 272 and sum(c["J"]) <= 16 and c["K"] <= 8
    a, b = by["sj16"], by["sj17"]
    assert sum(a["J"]) == 16 and sum(b["J"]) == 17 and (a["features"] != b["features"]).sum() == 1 and all(np.array_equal(x, y) for x, y in zip(a["X"], b["X"]))
    c = by["tiny"]; assert c["V"] == 5 < sum(c["J"])
    c = by["holes"]; assert 3 not in c["features"][:, 0] and c["J"][0] == 6 and c["V"] % 16 != 0
    assert [by[n]["K"] for n in ("K1", "K33", "K65", "K100")] == [1, 33, 65, 100] and all(by[n]["V"] == 96 for n in ("K1", "K33", "K65", "K100"))
    assert any(len(set(x[:, 0])) < x.shape[0] for x in by["dup"]["X"])
    assert by["empty"]["X"][0].shape[0] == 0 and by["empty"]["X"][-1].shape[0] == 0
    for c in CASES[len(ilda_ref.NAMED):]:
        assert 1 <= c["I"] <= 5 and all(2 <= j <= 8 for j in c["J"]) and 5 <= c["V"] <= 400 and 1 <= c["K"] <= 24 and 3 <= c["D"] <= 700
    again = ilda_ref.draw_cases()
    assert all(np.array_equal(a["features"], b["features"]) and all(np.array_equal(x, y) for x, y in zip(a["X"], b["X"])) for a, b in zip(CASES, again))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_six_passes_and_elbo_terms(oracle, c):
    """The constructor state, then six passes of the stage sequence of fit! with the whole state compared after each, then the seven ELBO
    terms (ElnQβ: the last feature's term alone, as ILDA.jl:174-181 computes it)."""
    r = ilda_ref.model_of(c)
    o = oracle_of(oracle, c)
    assert o.J.tolist() == r.J
    w = state_dist(o, r, {})
    for it in range(6):
        ll_r = r.one_pass()
        o.update_gamma(); o.update_phi(); o.update_lambda(); o.update_beta(); o.update_theta()
        w["ll"] = max(w.get("ll", 0.0), dist(o.loglik(), ll_r))
        state_dist(o, r, w)
    eo, to = o.elbo()
    er, tr = r.elbo_terms()
    w["elbo"] = max(dist(to, tr), dist(eo, er))
    print("\n%-15s oracle vs ilda_ref: %s" % (c["name"], "  ".join("%s %.1e" % kv for kv in w.items())))
    check(w, c["name"])
    if c["I"] >= 2:
        assert tr[4] == pytest.approx(r.ElnQbeta_of(c["I"] - 1), rel=1e-15)


def test_zz_print_the_measured_distance():
    """Runs after the parametrised test above (same module, later in the file): the worst distances seen over the case list."""
    print("\noracle vs ilda_ref, worst over %d cases: %s" % (len(CASES), "  ".join("%s %.2e" % kv for kv in sorted(WORST.items()))))
    assert max(WORST.values(), default=0.0) <= 1e-10


def stop_margin(ll, tol, converged):
    """How far the stopping rule (ILDA.jl:263, common.jl:53-56) was from deciding otherwise: the smallest factor between tol and the
    relative ll change of any pass at which the rule was evaluated."""
    ll = np.asarray(ll)
    rd = np.abs(ll[:-1] - ll[1:]) / np.abs(ll[1:])                 # rd[p - 2]: the rule's quantity after pass p
    m = np.inf
    for p in range(11, len(ll) + 1):
        stopped = converged and p == len(ll)
        m = min(m, tol / rd[p - 2] if stopped else rd[p - 2] / tol)
    return m


# (case, maxiter, tol, passes): tiny stops at pass 16 after a run of eligible passes that did not; dup at pass 11, the first pass the
# rule looks at (pass 10 already satisfied it: `length(ll) > 10`); empty never stops
FITS = [("tiny", 60, 1e-8, 16, True), ("dup", 60, 2e-2, 11, True), ("empty", 25, 1e-5, 25, False)]


@pytest.mark.parametrize("name,maxiter,tol,passes,conv", FITS, ids=[f[0] for f in FITS])
def test_fit_to_convergence(oracle, name, maxiter, tol, passes, conv):
    c = next(c for c in CASES if c["name"] == name)
    r = ilda_ref.model_of(c)
    ll_r = r.fit(maxiter=maxiter, tol=tol)
    margin = stop_margin(ll_r, tol, r.converged)
    print("\n%s: %d passes, converged %s, the stopping rule's margin is a factor %.3g" % (name, len(ll_r), r.converged, margin))
    assert margin >= 10.0, "the case no longer keeps the stopping rule a factor 10 from tol"
    assert (len(ll_r), r.converged) == (passes, conv)
    o = oracle_of(oracle, c)
    ll_o = o.fit(maxiter=maxiter, tol=tol)
    assert len(ll_o) == len(ll_r) and o.converged == r.converged
    assert dist(ll_o, ll_r) <= RTOL
    assert dist(o.elbo_value, r.elbo) <= RTOL_ELBO
    check(state_dist(o, r, {}), name)


HELDOUT = ("bigJ", "sj16")


@pytest.mark.parametrize("name", HELDOUT)
def test_fit_heldout(oracle, name):
    """The frozen-topic loop of fit_heldout (ILDA.jl:323-353) after six training passes."""
    c = next(c for c in CASES if c["name"] == name)
    r = ilda_ref.model_of(c); r.fit(maxiter=6, tol=0.0)
    o = oracle_of(oracle, c); o.fit(maxiter=6, tol=0.0)
    Xn = heldout_docs(c)
    hr = r.fit_heldout(Xn, maxiter=40)
    ho = o.fit_heldout(Xn, maxiter=40)
    margin = stop_margin(hr.ll_history, 1e-4, hr.converged)
    print("\n%s held out: %d passes, converged %s, margin %.3g" % (name, len(hr.ll_history), hr.converged, margin))
    assert margin >= 1.001
    assert len(ho.ll_hist) == len(hr.ll_history) and ho.converged == hr.converged
    assert dist(ho.ll_hist, hr.ll_history) <= RTOL
    assert dist(ho.theta.reshape(hr.D, hr.K).T, hr.theta) <= RTOL
    assert dist(ho.elbo_value, hr.elbo) <= RTOL_ELBO


@pytest.mark.parametrize("name", ["identity", "identity_small"])
def test_one_feature_whose_value_is_the_term_is_lda(oracle, name):
    """ILDA with features[v] = v is LDA from the same λ0: ilda_ref, IldaOracle and LdaOracle over 15 passes."""
    c = next(c for c in CASES if c["name"] == name)
    V, K, D = c["V"], c["K"], c["D"]
    r = ilda_ref.model_of(c)
    ll_r = r.fit(maxiter=15, tol=0.0)
    o = oracle_of(oracle, c); ll_o = o.fit(maxiter=15, tol=0.0)
    l = oracle.LdaOracle(K, c["alpha"], c["eta"][0], c["X"], V=V, lambda0=c["lam0"][0])
    ll_l = l.fit(maxiter=15, tol=0.0)
    assert dist(ll_l, ll_r) <= RTOL and dist(ll_o, ll_r) <= RTOL
    assert dist(l.lam.reshape(V, K, order="F"), r.lam[0]) <= RTOL and dist(l.gamma.reshape(D, K).T, r.gamma) <= RTOL
    assert dist(l.elbo_value, r.elbo) <= RTOL_ELBO and dist(o.elbo_value, r.elbo) <= RTOL_ELBO
