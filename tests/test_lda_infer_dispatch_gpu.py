"""LDA frozen-topic inference (`transform`, `fit_heldout`: mmm_lda_infer -> frozen_passes, csrc/lda.hip) on every E-step build it can take,
case by case (lda_infer_ref.cases()), against tests/lda_infer_ref.py -- the numpy restatement of LDA.jl:226-295 in extended precision, which
tests/test_lda_infer_ref_cpu.py holds the C oracle to.  On a handle that is not on the wide path these passes launch the LL = true builds of
k_lda_estep (csrc/lda_estep.cuh), which no fit reaches (a fit evaluates its ll in the reduce launch): 16-, 32- and 64-lane groups, single-step
and grid-stride, rows of 16- and 32-bit counts, padded pairs and the CSR reader, pinned waves per block; on the wide path k_lda_tables_by_term
with β and k_lda_estep_wide / k_lda_estep_big with do_ll.  Every case asserts the geometry its handle reports before it compares anything.

Per case the topics are trained once on the device (120 documents, 15 passes) and downloaded; the restatement runs on those very tables, so
inference is tested by itself.  Held-out handles are built under the case's tuning as test_lda_transform_stops_like_the_reference builds its.

Bounds (those tests/test_inference_gpu.py holds): θ and γ rtol 1e-9, ll history rtol 1e-10, ϕ rtol 1e-9 with atol 1e-300, ELBO rel 1e-9; γ
columns sum to K α + N_d at rtol 1e-12, θ columns to 1 at rtol 1e-13.  Every test prints the largest distance it saw per quantity.
WIDER names the cases held to the fit suite's bound instead (ll, γ, ELBO 1e-9; θ, ϕ 1e-5), with the measured error and its source: no case
needs it.  Largest distances measured on an MI355X over the whole file: ll 3.7e-16, γ and θ 7.0e-14, ϕ 5.4e-13 (wide_k65_v96, stopped at
pass 23), ELBO 1.8e-14; the 50 documents inferred alone and among 200 agree in every bit."""
import ctypes as C
import warnings

import numpy as np
import pytest

import lda_infer_ref as ref
from lda_infer_ref import dist

pytestmark = pytest.mark.gpu
CASES = ref.cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}
MODES = pytest.mark.parametrize("unsmoothed", [True, False], ids=["unsmoothed", "smoothed"])
PRIMARY = {"ll": 1e-10, "γ": 1e-9, "θ": 1e-9, "ϕ": 1e-9, "ELBO": 1e-9}
FIT_SUITE = {"ll": 1e-9, "γ": 1e-9, "θ": 1e-5, "ϕ": 1e-5, "ELBO": 1e-9}
WIDER = ()              # names of the cases held to FIT_SUITE: none
TOL, MAXITER = 1e-4, 200
STOP_CASES = ref.REPRESENTATIVES + ("w1_k10_v96", "k13_v130_g2", "l64_k32_v120", "wide_k65_v96")
_TRAINED, _REF = {}, {}


def infer_on(new, unsmoothed, maxiter, tol):
    from multimodalmusig_jl_amd.inference import _lda_infer
    return _lda_infer(new, unsmoothed, maxiter, tol, False)


def trained(mmm, c, keep=False):
    """(λ, β, Elnβ) of the case's topics: TRAIN_PASSES passes of a device fit over the training corpus, downloaded.  Default tuning."""
    if keep or c["name"] not in _TRAINED:
        g = mmm.LDA(c["K"], c["alpha"], c["eta"], c["V"], c["Xt"], λ0=c["lam0"])
        ll = mmm.fit(g, maxiter=ref.TRAIN_PASSES, tol=0.0, verbose=False)
        assert len(ll) == ref.TRAIN_PASSES and np.all(np.isfinite(ll))
        _TRAINED[c["name"]] = (g.λ, g.β, g.Elnβ)
        if keep:
            return g
        g.close()
    return _TRAINED[c["name"]]


def assert_geometry(new, c, what=None):
    geo = new.geometry()
    want = c["geometry"] if what is None else {k: c["geometry"][k] for k in what}
    got = {k: geo[k] for k in want}
    assert got == want, "%s took another build: reports %s, the case is meant for %s" % (c["name"], got, want)


def heldout_handle(mmm, tuning, c, T, unsmoothed, X=None, geometry=True):
    """A constructor-state handle on the held-out documents under the case's tuning, holding the copies `transform` (LDA.jl:237) or
    `fit_heldout` (:269-271) makes."""
    lam, beta, Elnbeta = T
    tuning(**c["tuning"])
    new = mmm.LDA(c["K"], c["alpha"], c["eta"], c["V"], c["Xn"] if X is None else X, seed=3)
    tuning()
    if unsmoothed:
        new.β = beta
    else:
        new.λ = lam; new.β = beta; new.Elnβ = Elnbeta
    if geometry:
        assert_geometry(new, c)
    return new


def reference(c, T, unsmoothed, maxiter=ref.PASSES, tol=0.0):
    """The restatement's run on the tables downloaded from the device (computed once per case, mode and loop limits; never modified)."""
    key = (c["name"], unsmoothed, maxiter, tol)
    if key not in _REF:
        lam, beta, Elnbeta = T
        _REF[key] = ref.infer(c["Xn"], c["K"], c["alpha"], beta, None if unsmoothed else Elnbeta, None if unsmoothed else lam, unsmoothed,
                              maxiter, tol, eta=c["eta"])
    return _REF[key]


def distances(new, hist, r, elbo=None):
    w = {"ll": dist(hist, r.ll), "γ": dist(new.γ, r.gamma), "θ": dist(new.θ, r.theta), "ϕ": dist(new.phi_flat(), ref.phi_rows(r.phi), atol=1e-300)}
    if elbo is not None:
        w["ELBO"] = dist(elbo, r.model.elbo_terms()[0])
    return w


def hold(w, name, tag=""):
    print("\n%-22s %-12s %s" % (name, tag, "  ".join("%s %.1e" % kv for kv in w.items())))
    bounds = FIT_SUITE if name in WIDER else PRIMARY
    for k, v in w.items():
        assert v <= bounds[k], "%s %s: %s is %.3g from the restatement (bound %g)" % (name, tag, k, v, bounds[k])


def conserved(new, c, X=None):
    N = np.array([int(x[:, 1].sum()) for x in (c["Xn"] if X is None else X)], dtype=np.float64)
    np.testing.assert_allclose(new.γ.sum(axis=0), c["K"] * c["alpha"] + N, rtol=1e-12)
    np.testing.assert_allclose(new.θ.sum(axis=0), 1.0, rtol=1e-13)


def margin(r):
    """How far, as a fraction of tol, the nearest stop ratio after the 10th pass is from tol."""
    return float(np.abs(r.ratio[10:] / TOL - 1.0).min()) if len(r.ll) > 10 else np.inf


def same_bits(a, b, what):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel(); b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape, what
    n = int((a.view(np.int64) != b.view(np.int64)).sum())
    assert n == 0, "%s: %d of %d values differ in their bits" % (what, n, a.size)


# ------------------------------------------------------------------------------------------------------------- the walk
@MODES
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_twelve_frozen_passes_on_every_build(mmm, tuning, c, unsmoothed):
    """12 passes at tol = 0 on the build the case names: ll history, γ, θ, ϕ (smoothed: the ELBO too) against the restatement; mass
    conservation."""
    T = trained(mmm, c)
    new = heldout_handle(mmm, tuning, c, T, unsmoothed)
    hist = infer_on(new, unsmoothed, ref.PASSES, 0.0)
    assert len(hist) == ref.PASSES and not new.converged
    r = reference(c, T, unsmoothed)
    w = distances(new, hist, r, elbo=None if unsmoothed else mmm.calculate_elbo(new))
    hold(w, c["name"], "unsmoothed" if unsmoothed else "smoothed")
    conserved(new, c)
    new.close()


# ------------------------------------------------------------------------------------------------------------- properties
@MODES
@pytest.mark.parametrize("name", ref.REPRESENTATIVES)
def test_split_calls(mmm, tuning, name, unsmoothed):
    """(1) 5 + 7 passes in two calls on one handle are the 12 passes of one call on another, bit for bit; with tol = 1e-4 a first call of
    6 passes cannot stop, and the second stops on more than 10 values of its OWN history, at the pass the restatement names when it is run
    the same way (from the first run's ϕ, with a fresh history)."""
    c = BY[name]
    T = trained(mmm, c)
    a = heldout_handle(mmm, tuning, c, T, unsmoothed); b = heldout_handle(mmm, tuning, c, T, unsmoothed)
    ha = np.concatenate([infer_on(a, unsmoothed, 5, 0.0), infer_on(a, unsmoothed, 7, 0.0)])
    hb = infer_on(b, unsmoothed, ref.PASSES, 0.0)
    assert len(ha) == ref.PASSES
    same_bits(ha, hb, "ll history"); same_bits(a.γ, b.γ, "γ"); same_bits(a.θ, b.θ, "θ")
    hold(distances(a, ha, reference(c, T, unsmoothed)), name, "5 + 7 passes")
    a.close(); b.close()
    # the stop rule across calls
    s = heldout_handle(mmm, tuning, c, T, unsmoothed)
    h1 = infer_on(s, unsmoothed, 6, TOL)
    assert len(h1) == 6 and not s.converged
    h2 = infer_on(s, unsmoothed, 60, TOL)
    r1 = reference(c, T, unsmoothed, 6, TOL)
    lam, beta, Elnbeta = T
    r2 = ref.infer(c["Xn"], c["K"], c["alpha"], beta, None if unsmoothed else Elnbeta, None if unsmoothed else lam, unsmoothed, 60, TOL,
                   phi0=r1.phi, eta=c["eta"])
    assert r2.converged and 11 <= len(r2.ll) < 60 and margin(r2) >= 0.05, (len(r2.ll), margin(r2))
    assert len(h2) == len(r2.ll) and s.converged, "second call ran %d passes (converged %s), the restatement %d" % (len(h2), s.converged, len(r2.ll))
    np.testing.assert_allclose(h1, r1.ll, rtol=PRIMARY["ll"])
    hold(distances(s, h2, r2), name, "6 + %d stopped" % len(h2))
    s.close()


@MODES
@pytest.mark.parametrize("fitted", [7, 8])
@pytest.mark.parametrize("name", ref.REPRESENTATIVES)
def test_ring_slots(mmm, tuning, name, fitted, unsmoothed):
    """(2) a handle FITTED for 7 / 8 passes holds its current topics in ring slot 1 / 2: three frozen passes on it against the restatement
    started from the handle's own ϕ, and λ, β, Elnβ read back afterwards are what they were."""
    c = BY[name]
    tuning(**c["tuning"])
    g = mmm.LDA(c["K"], c["alpha"], c["eta"], c["V"], c["Xn"], λ0=c["lam0"])
    tuning()
    assert_geometry(g, c)
    assert len(mmm.fit(g, maxiter=fitted, tol=0.0, verbose=False)) == fitted
    lam, beta, Elnbeta = g.λ, g.β, g.Elnβ
    phi0 = ref.phi_docs(g.phi_flat(), c["Xn"])
    hist = infer_on(g, unsmoothed, 3, 0.0)
    assert len(hist) == 3
    r = ref.infer(c["Xn"], c["K"], c["alpha"], beta, Elnbeta, lam, unsmoothed, 3, 0.0, phi0=phi0, eta=c["eta"])
    hold(distances(g, hist, r, elbo=None if unsmoothed else mmm.calculate_elbo(g)), name, "fitted %d" % fitted)
    conserved(g, c)
    same_bits(g.λ, lam, "λ"); same_bits(g.β, beta, "β"); same_bits(g.Elnβ, Elnbeta, "Elnβ")
    g.close()


@MODES
@pytest.mark.parametrize("name", STOP_CASES)
def test_stop_rule_and_the_launches_after_it(mmm, tuning, name, unsmoothed):
    """(3) tol = 1e-4, at most 200 passes: the pass count and `converged` of the restatement; γ, θ, ϕ are those of the stopping pass -- the
    passes enqueued after k_lda_infer_tail has set the stop flag leave the handle alone."""
    c = BY[name]
    T = trained(mmm, c)
    r = reference(c, T, unsmoothed, MAXITER, TOL)
    assert r.converged and 11 <= len(r.ll) < MAXITER and margin(r) >= 0.05, (len(r.ll), margin(r))
    new = heldout_handle(mmm, tuning, c, T, unsmoothed)
    hist = infer_on(new, unsmoothed, MAXITER, TOL)
    assert len(hist) == len(r.ll) and new.converged, "%d passes (converged %s), the restatement %d" % (len(hist), new.converged, len(r.ll))
    hold(distances(new, hist, r, elbo=None if unsmoothed else mmm.calculate_elbo(new)), name, "stopped at %d" % len(hist))
    conserved(new, c)
    new.close()


@MODES
@pytest.mark.parametrize("name", ref.REPRESENTATIVES)
def test_a_document_reads_nothing_from_its_companions(mmm, tuning, name, unsmoothed):
    """(4) the first 50 of 200 documents inferred alone and among all 200, same topics and tuning: γ and θ of the 50 agree at rtol 1e-11.  A
    document's solve reads only its own row; the order of its sums may differ through the chunk rotation with the group index (12 passes x 96
    terms x 2^-53 = 1.3e-13, the bound is a hundred times that)."""
    c = BY[name]
    T = trained(mmm, c)
    n = CASES.index(c)
    X = ref.heldout_corpus(7000 + n, 200, c["V"], c["K"], c["mean_n"], 1.0)
    few = heldout_handle(mmm, tuning, c, T, unsmoothed, X=X[:50], geometry=False)
    many = heldout_handle(mmm, tuning, c, T, unsmoothed, X=X, geometry=False)
    assert_geometry(few, c, ("L", "KP", "wide")); assert_geometry(many, c, ("L", "KP", "wide"))
    infer_on(few, unsmoothed, ref.PASSES, 0.0); infer_on(many, unsmoothed, ref.PASSES, 0.0)
    w = {"γ": dist(few.γ, many.γ[:, :50]), "θ": dist(few.θ, many.θ[:, :50])}
    print("\n%-22s 50 alone / among 200: %s" % (name, "  ".join("%s %.1e" % kv for kv in w.items())))
    assert max(w.values()) <= 1e-11, w
    conserved(few, c, X[:50]); conserved(many, c, X)
    few.close(); many.close()


@pytest.mark.parametrize("name", ["l32_k20_v96_g2", "wide_k48_v96"])
def test_python_entries(mmm, tuning, name):
    """(5) mmm.transform and mmm.fit_heldout themselves (the glue: which tables are copied, what is returned) against the restatement."""
    c = BY[name]
    g = trained(mmm, c, keep=True)
    T = _TRAINED[name]
    tuning(**c["tuning"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # "transform did not converge": 12 passes at tol = 0
        th = mmm.transform(g, c["Xn"], maxiter=ref.PASSES, tol=0.0)
    h = mmm.fit_heldout(c["Xn"], g, maxiter=ref.PASSES)     # tol = 1e-4 (LDA.jl:286)
    tuning()
    assert_geometry(h, c)
    rt = reference(c, T, True)
    rh = reference(c, T, False, ref.PASSES, TOL)
    assert margin(rh) >= 0.05
    assert len(h.ll_history) == len(rh.ll) and h.converged == rh.converged
    w = distances(h, h.ll_history, rh, elbo=h.elbo)
    w["θ transform"] = dist(th, rt.theta)
    assert h.ll == h.ll_history[-1]
    print("\n%-22s %s" % (name, "  ".join("%s %.1e" % kv for kv in w.items())))
    for k, v in w.items():
        assert v <= PRIMARY[k.split()[0]], (name, k, v)
    same_bits(g.β, T[1], "the trained model's β")
    h.close(); g.close()


def test_refusals(mmm):
    """(6) maxiter = 0 is MMM_ERR_ARG; a restart batch is refused (MMM_ERR_UNSUPPORTED); the handle and the context stay usable."""
    c = BY["s16_k6_v96_d70"]
    L = mmm.lib()
    ni, cv = C.c_int(), C.c_int()
    new = mmm.LDA(c["K"], c["alpha"], c["eta"], c["V"], c["Xn"], seed=3)
    new.β = np.full((c["V"], c["K"]), 1.0 / c["V"])         # (β of the constructor state is undefined, LDA.jl:37)
    assert L.mmm_lda_infer(new._h, 1, 0, 1e-4, None, C.byref(ni), C.byref(cv)) == -1
    assert b"maxiter < 1" in L.mmm_last_error(new.ctx.h)
    assert L.mmm_lda_infer(new._h, 1, -3, 1e-4, None, C.byref(ni), C.byref(cv)) == -1
    batch = mmm.LDA(c["K"], c["alpha"], c["eta"], c["V"], c["Xn"], seed=3, restarts=2)
    assert L.mmm_lda_infer(batch._h, 1, 5, 1e-4, None, C.byref(ni), C.byref(cv)) == -4
    batch.close()
    hist = infer_on(new, True, 3, 0.0)
    assert len(hist) == 3 and np.all(np.isfinite(hist))
    new.close()
