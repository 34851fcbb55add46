"""Every ELBO term of every build against tests/elbo_ref.py (np.longdouble, lgamma from mpmath; tests/test_elbo_ref_cpu.py holds the C
oracle to it inside the same bound).  The ELBO is a pure function of the state a handle holds, so each test evaluates the restatement on
that very state and compares `calculate_elbo(model, terms=True)` term by term at max(γ_n A_t, 4 unit_t), absolute (elbo_ref.bound; n is
derived from the kernels in elbo_ref.lda_roundings / ctm_roundings).  Every case asserts the geometry its handle reports first and prints
its ratio to the bound per term; DESIGN.md sections 4.7 / 4.9 carry the largest.

Which case reaches what:

    k_lda_elbo_docs                 (a) k1_v1_d1 .. k64_v256_d17 (K = 64: every lane), both ILDA cases; (c) single_step, dense_row, grid_stride, wide
    k_lda_elbo_docs_big             (a) k65_v257_d17 (one lane in slot 2), k128_v96_d3 (2 slots), k129_v96_d16 (3), k256_v96_d1 (4); (c) k65
    k_lda_elbo_topics               every LDA case; V = 257: a second stride of the 256 threads
    k_ilda_elbo_topics              (a) ilda_snv3 (I = 3), ilda_i2_eta (I = 2, η unequal)
    k_ctm_elbo_docs<true>           (b) k1, k2, k7_7, k28, k63, k64_lds48 (dynamic LDS 55,296 B > 48 KB), m8_k1, both IMMCTM cases; (c) lds,
                                    rows_of_counts, imm_snv3; (d); (e)
    k_ctm_elbo_docs<false>          (b) k7_7_wide (the state of k7_7), k33_4, wide_tab; (c) wide
    k_ctm_elbo_docs_big             (b) k65, k128, k256; (c) k65
    k_ctm_elbo_topics, LDS branch   every CTM case with ΣK <= 64; IMMCTM with three features: imm_snv3, imm_2mod
    k_ctm_elbo_topics, big_scratch  (b) k65, k128, k256; (c) k65
    k_sum_columns (both files)      every case; a second document step per wave: D = 17 (LDA), D = 13 (CTM) under geometry_cus = 1
    lda_elbo_finish / elbo_finish   every case (the total is the terms' sum bit for bit)
    materialise_phi                 (c) phi_valid after set (a), phi_from_prev after passes, reset by a stage call; constructor state
    materialise_theta               (c) theta_state 0 (constructor), 1 (after passes), 2 (set / update_θ); (d) theta_spill of replicas r > 0
    replica offsets of elbo_enqueue (d) r = 1, 2 of a CTM batch with its own α per replica; an LDA batch"""
import numpy as np
import pytest

import ctm_dense_ref as CR
import elbo_ref as R
from lda_infer_ref import dist

pytestmark = pytest.mark.gpu

LDA_NAMES = [c["name"] for c in R.LDA_CASES]
CTM_NAMES = [c["name"] for c in R.CTM_CASES]
_REF = {}          # restatements of the written states, evaluated once
# Cases whose device value needs more than the bound, with the function and the argument where it happens (none: every term of every case
# is inside max(γ_n A_t, 4 unit_t)).
WIDER = {}


def _cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _sum7(t):
    return t[0] + t[1] + t[2] + t[3] - t[4] - t[5] - t[6]


def _show(name, names, r):
    print("%-16s %s" % (name, " ".join("%s %.3f" % (a, b) for a, b in zip(names, r))))


def _check(name, names, e, terms, t, n, extra=None):
    r = R.ratios(terms, t, n, extra)
    _show(name, names, r)
    assert np.all(r <= 1.0), "%s: %s off by %s of the bound" % (name, [names[i] for i in np.nonzero(r > 1.0)[0]], r[r > 1.0])
    assert e == _sum7(terms), "%s: the total is not the sum of its terms" % name
    return r


def _iterate(mmm, g, n):
    if isinstance(g, mmm.LDA):
        mmm._lib.check(mmm.lib().mmm_lda_iterate(g._h, n), g.ctx.h, "iterate")
    else:
        mmm._lib.check(mmm.lib().mmm_ctm_iterate(g._h, n, 1), g.ctx.h, "iterate")


# ---------------------------------------------------------------------------------------------------------- (a) LDA, written state
def _lda_geometry(g, K):
    geo = g.geometry()
    KP = next((o for o in (2, 4, 6, 8, 10, 12, 16, 20, 24, 32) if K <= o), (K + 1) & ~1)
    assert geo["L"] == (16 if K <= 15 else (32 if K <= 31 else 64)) and geo["KP"] == KP, geo
    assert geo["wide"] == int(KP >= 32), geo            # 25 topics and more: the wide path; K > 64 then takes k_lda_elbo_docs_big
    return geo


def _lda_handle(mmm, st):
    K, V = st["K"], st["V"]
    if st["features"] is None:
        g = mmm.LDA(K, st["alpha"], st["eta"], V, st["X"], λ0=st["lam"])
        g.λ = st["lam"]; g.Elnβ = st["Elnbeta"]
    else:
        g = mmm.ILDA(K, st["alpha"], st["eta"], st["features"], st["X"], λ0=st["lam"])
        g._set("ilambda", np.concatenate([x.ravel(order="F") for x in st["lam"]]))
        g._set("iElnbeta", np.concatenate([x.ravel(order="F") for x in st["Elnbeta"]]))
    g.γ = st["gamma"]; g.Elnθ = st["Elntheta"]
    g._set("phi", st["phi"].ravel())
    assert np.array_equal(g.γ, st["gamma"]) and np.array_equal(g.phi_flat(), st["phi"])          # the handle holds what was written
    return g


@pytest.mark.parametrize("name", LDA_NAMES)
def test_lda_written_state(mmm, tuning, name):
    c, st = R.lda_written(name)
    tuning(geometry_cus=1)
    g = _lda_handle(mmm, st)
    _lda_geometry(g, c["K"])
    e, terms = mmm.calculate_elbo(g, terms=True)
    t = _cached(("lda", name), lambda: R.lda_terms(st))
    _check(name, R.LDA_TERMS, e, terms, t, R.lda_case_roundings(c))
    g.close()


# ---------------------------------------------------------------------------------------------------------- (b) CTM, written state
def _ctm_handle(mmm, lay, st, alpha=None, gamma0=None):
    s = lay.s
    alpha = st["alpha"] if alpha is None else alpha
    g0 = st["gamma"] if gamma0 is None else gamma0
    if lay.imm:
        off = np.concatenate([[0], np.cumsum(s.I)])
        a = [np.asarray(alpha)[off[m]:off[m + 1]] for m in range(lay.M)] if np.ndim(alpha[0]) == 0 else alpha
        return mmm.IMMCTM(lay.K, a, s.features, s.X, γ0=g0)
    return mmm.MMCTM(lay.K, alpha, lay.V, s.X, γ0=R.nested_gamma(lay, g0))


def _ctm_write(g, st):
    for f, k in (("mu", "mu"), ("invSigma", "invSigma"), ("gamma", "gamma"), ("Elnphi", "Elnphi"), ("lambda", "lam"), ("nu", "nu"), ("zeta", "zeta"),
                 ("theta", "theta")):
        g._set(f, np.asarray(st[k]).ravel())
    assert np.array_equal(g._get("theta"), st["theta"]) and np.array_equal(g._get("zeta"), st["zeta"].ravel())


def _ctm_geometry(g, lay, forced_wide=False, tdense=0):
    geo = g.geometry()
    assert geo["L"] == (16 if lay.MK <= 16 else (32 if lay.MK <= 32 else 64)), geo
    assert geo["wide"] == int(R.ctm_is_wide(lay, forced_wide)) and geo["tdense"] == tdense, geo
    if lay.MK > 64:          # the handle is `big`: lane l holds coordinates l + 64 q
        assert geo["Ls"] == 64 and geo["cpl"] == 4, geo
    return geo


def _ctm_readback(g, lay):
    return dict(alpha=g._get("alpha"), mu=g._get("mu"), invSigma=g._get("invSigma").reshape(lay.MK, lay.MK), gamma=g._get("gamma"),
                Elnphi=g._get("Elnphi"), lam=g._get("lambda").reshape(lay.D, lay.MK), nu=g._get("nu").reshape(lay.D, lay.MK),
                zeta=g._get("zeta").reshape(lay.D, lay.M))


def _ctm_written_terms(mmm, tuning, name):
    c, lay, st = R.ctm_written(name)
    tuning(geometry_cus=1, ctm_build=c.get("build", "auto"))
    g = _ctm_handle(mmm, lay, st)
    _ctm_write(g, st)
    _ctm_geometry(g, lay, forced_wide=c.get("build") == "wide")
    e, terms = mmm.calculate_elbo(g, terms=True)
    g.close()
    t = _cached(("ctm", c.get("twin", name)), lambda: R.ctm_terms(lay, st))
    return lay, e, terms, t


@pytest.mark.parametrize("name", CTM_NAMES)
def test_ctm_written_state(mmm, tuning, name):
    lay, e, terms, t = _ctm_written_terms(mmm, tuning, name)
    _check(name, R.CTM_TERMS, e, terms, t, R.ctm_roundings(lay, cus=1))


def test_ctm_table_in_lds_and_through_l2_agree(mmm, tuning):
    """k_ctm_elbo_docs<true> and <false> on one state ([7,7] x [96,48], the second handle forced wide): their terms agree within the bound"""
    lay, _, a, t = _ctm_written_terms(mmm, tuning, "k7_7")
    _, _, b, _ = _ctm_written_terms(mmm, tuning, "k7_7_wide")
    gap = np.abs(a - b) / R.bound(t, R.ctm_roundings(lay, cus=1))
    _show("lds vs wide", R.CTM_TERMS, gap)
    assert np.all(gap <= 1.0), gap


# ---------------------------------------------------------------------------------------------------------- (c) the state machines
def _lda_readback(g, X):
    K, V, D = g.K, g.V, g.D
    return dict(K=K, V=V, D=D, X=X, alpha=g.α, eta=g.η, features=None, lam=g.λ, Elnbeta=g.Elnβ, gamma=g.γ, Elntheta=g.Elnθ)


def _lda_pair(mmm, tuning, c, passes):
    X, lam0 = R.pass_lda(c)
    tuning(**c["tune"])
    out = []
    for n in passes:
        g = mmm.LDA(c["K"], 0.1, 0.1, c["V"], X, λ0=lam0)
        geo = g.geometry()
        assert all(geo[k] == v for k, v in c["geo"].items()), (c["name"], geo)
        if n:
            _iterate(mmm, g, n)
        out.append(g)
    return X, out


def _lda_lazy_check(name, c, X, e, terms, st, Elnbeta_prev, phi_dev):
    """terms against the restatement on the read-back state WITH ϕ_n = softmax(Elnθ, the given Elnβ), and the device's ϕ against ϕ_n"""
    phi_n = R.lda_phi(X, st["Elntheta"], Elnbeta_prev)
    w = dist(phi_dev, phi_n.astype(np.float64), atol=1e-300)
    print("%-16s ϕ against ϕ_n: rel %.2e" % (name, w))
    assert w <= 1e-9
    t = R.lda_terms(R.with_phi(st, phi_n))
    eps = float(R.gam(R.phi_roundings(st["Elntheta"], Elnbeta_prev, c["K"])))
    extra = R.stale_allowance(t, eps, R.qz_scale_lda(R.with_phi(st, phi_n.astype(np.float64))))
    n = R.lda_roundings(c["K"], c["V"], c["D"], max(x.shape[0] for x in X))
    return _check(name, R.LDA_TERMS, e, terms, t, n, extra)


@pytest.mark.parametrize("name", [c["name"] for c in R.PASS_LDA])
def test_lda_after_passes(mmm, tuning, name):
    """B has run n fused passes, A n - 1: ϕ_n is formed from (Elnθ of B, Elnβ of A) -- a ϕ taken one pass late misses by > 1e10 bounds"""
    c = next(x for x in R.PASS_LDA if x["name"] == name)
    X, (A, B) = _lda_pair(mmm, tuning, c, (R.N_PASSES - 1, R.N_PASSES))
    e, terms = mmm.calculate_elbo(B, terms=True)
    _lda_lazy_check(name, c, X, e, terms, _lda_readback(B, X), A.Elnβ, B.phi_flat())
    A.close(); B.close()


def test_lda_call_orders(mmm, tuning):
    c = R.PASS_LDA[0]
    n = R.N_PASSES
    X, (B, B2, C, Z) = _lda_pair(mmm, tuning, c, (n, n, 0, 0))
    e1, t1 = mmm.calculate_elbo(B, terms=True)
    B.phi_flat()
    e2, t2 = mmm.calculate_elbo(B, terms=True)
    B2.phi_flat()
    e3, t3 = mmm.calculate_elbo(B2, terms=True)
    assert e1 == e2 == e3 and np.array_equal(t1, t2) and np.array_equal(t1, t3)          # before / after phi_flat(): the same bits
    mmm.fit(C, maxiter=n, tol=0.0, verbose=False)
    assert mmm.calculate_elbo(C) == C.elbo                                               # fit's ELBO is calculate_elbo's, bit for bit
    # the constructor state: ϕ = 1 / K
    e, terms = mmm.calculate_elbo(Z, terms=True)
    st = _lda_readback(Z, X)
    nnz = sum(x.shape[0] for x in X)
    t = R.lda_terms(R.with_phi(st, np.full((nnz, c["K"]), 1.0 / c["K"])))
    _check("constructor", R.LDA_TERMS, e, terms, t, R.lda_roundings(c["K"], c["V"], c["D"], max(x.shape[0] for x in X)))
    # a stage call after passes: update_ϕ! forms ϕ from the CURRENT tables, and the lazy ϕ of the passes is gone
    mmm.update_θ(B); mmm.update_ϕ(B)
    e, terms = mmm.calculate_elbo(B, terms=True)
    st = _lda_readback(B, X)
    _lda_lazy_check("after update_ϕ!", c, X, e, terms, st, st["Elnbeta"], B.phi_flat())
    for g in (B, B2, C, Z):
        g.close()


def _ctm_pair(mmm, tuning, c, passes):
    lay, alpha, g0 = R.pass_ctm(c)
    tuning(**c["tune"])
    out = []
    for n in passes:
        g = _ctm_handle(mmm, lay, None, alpha=alpha, gamma0=g0)
        geo = g.geometry()
        assert all(geo[k] == v for k, v in c["geo"].items()), (c["name"], geo)
        if n:
            _iterate(mmm, g, n)
        out.append(g)
    return lay, out


def _ctm_lazy_check(name, lay, e, terms, st, lam_prev, Elnphi_prev, theta_dev):
    th_n = R.theta_from(lay, lam_prev, Elnphi_prev)
    nr = R.theta_roundings(lay, lam_prev, Elnphi_prev)
    unit = CR.rel_gap(R.theta_from(lay, lam_prev, Elnphi_prev, np.float64), th_n)
    w = CR.ratio_rel(theta_dev, th_n, CR._gam(nr), unit)
    print("%-16s θ against θ_n: %.3f of its bound" % (name, w))
    assert w <= 1.0
    stn = R.with_theta(st, th_n)
    t = R.ctm_terms(lay, stn)
    extra = R.stale_allowance(t, float(CR._gam(nr)), R.qz_scale_ctm(lay, R.with_theta(st, th_n.astype(np.float64))))
    return _check(name, R.CTM_TERMS, e, terms, t, R.ctm_roundings(lay), extra)


@pytest.mark.parametrize("name", [c["name"] for c in R.PASS_CTM])
def test_ctm_after_passes(mmm, tuning, name):
    """θ_n = update_θ!(λ and Elnϕ of A, which has run n - 1 passes); B's terms are those of its read-back state with THAT θ"""
    c = next(x for x in R.PASS_CTM if x["name"] == name)
    lay, (A, B) = _ctm_pair(mmm, tuning, c, (R.N_PASSES - 1, R.N_PASSES))
    e, terms = mmm.calculate_elbo(B, terms=True)
    _ctm_lazy_check(name, lay, e, terms, _ctm_readback(B, lay), A._get("lambda"), A._get("Elnphi"), B._get("theta"))
    A.close(); B.close()


def test_ctm_call_orders(mmm, tuning):
    c = R.PASS_CTM[0]
    n = R.N_PASSES
    lay, (B, B2, C, Z) = _ctm_pair(mmm, tuning, c, (n, n, 0, 0))
    e1, t1 = mmm.calculate_elbo(B, terms=True)
    B._get("theta")
    e2, t2 = mmm.calculate_elbo(B, terms=True)
    B2._get("theta")
    e3, t3 = mmm.calculate_elbo(B2, terms=True)
    assert e1 == e2 == e3 and np.array_equal(t1, t2) and np.array_equal(t1, t3)
    mmm.fit(C, maxiter=n, tol=0.0, verbose=False)
    assert mmm.calculate_elbo(C) == C.elbo
    # the constructor state: θ = 1 / K_m (theta_state 0)
    e, terms = mmm.calculate_elbo(Z, terms=True)
    st = _ctm_readback(Z, lay)
    th = np.concatenate([np.full(int(lay.nnz[m]) * lay.K[m], 1.0 / lay.K[m]) for m in range(lay.M)])
    _check("constructor", R.CTM_TERMS, e, terms, R.ctm_terms(lay, R.with_theta(st, th)), R.ctm_roundings(lay))
    # update_θ! after passes: θ from the CURRENT λ and Elnϕ (theta_state 2)
    mmm.update_θ(B)
    e, terms = mmm.calculate_elbo(B, terms=True)
    st = _ctm_readback(B, lay)
    _ctm_lazy_check("after update_θ!", lay, e, terms, st, st["lam"], st["Elnphi"], B._get("theta"))
    for g in (B, B2, C, Z):
        g.close()


# ---------------------------------------------------------------------------------------------------------- (d) replicas
def test_ctm_batch_replicas(mmm, tuning):
    """three restarts with their own γ0, autoα for 4 passes (every replica its own α): select(r), then the seven terms against the
    restatement on that replica's read-back state; restart_elbo[r] is the total bit for bit"""
    c = R.PASS_CTM[0]
    lay, alpha, _ = R.pass_ctm(c)
    tuning()
    rng = np.random.default_rng(5)
    g0 = [R.nested_gamma(lay, rng.integers(1, 101, size=int(lay.s.goff[-1])).astype(np.float64)) for _ in range(3)]
    g = mmm.MMCTM(lay.K, alpha, lay.V, lay.s.X, γ0=g0, restarts=3)
    _ctm_geometry(g, lay)
    mmm.fit_restarts(g, maxiter=4, tol=0.0, autoα=True)
    seen, alphas = [], []
    for r in range(3):
        g.select(r)
        e, terms = mmm.calculate_elbo(g, terms=True)
        st = _ctm_readback(g, lay)
        st["theta"] = g._get("theta")
        _check("replica %d" % r, R.CTM_TERMS, e, terms, R.ctm_terms(lay, st), R.ctm_roundings(lay))
        assert e == g.restart_elbo[r]
        seen.append(terms); alphas.append(st["alpha"])
    assert not np.any(seen[1] == seen[0]) and not np.any(seen[2] == seen[0])
    assert not np.array_equal(alphas[0], alphas[1]) and not np.array_equal(alphas[0], np.asarray(alpha))
    g.close()


def test_lda_batch_replicas(mmm, tuning):
    c = R.PASS_LDA[0]
    X, _ = R.pass_lda(c)
    tuning()
    rng = np.random.default_rng(6)
    g = mmm.LDA(c["K"], 0.1, 0.1, c["V"], X, λ0=[rng.integers(1, 101, size=(c["V"], c["K"])).astype(np.float64) for _ in range(3)], restarts=3)
    mmm.fit_restarts(g, maxiter=4, tol=0.0)
    seen = []
    for r in range(3):
        g.select(r)
        e, terms = mmm.calculate_elbo(g, terms=True)
        st = _lda_readback(g, X)
        st["phi"] = g.phi_flat()
        _check("replica %d" % r, R.LDA_TERMS, e, terms, R.lda_terms(st), R.lda_roundings(c["K"], c["V"], c["D"], max(x.shape[0] for x in X)))
        assert e == g.restart_elbo[r]
        seen.append(terms)
    assert not np.any(seen[1][[0, 2, 3, 4, 5, 6]] == seen[0][[0, 2, 3, 4, 5, 6]])
    g.close()


# ---------------------------------------------------------------------------------------------------------- (e) held-out handles
def test_lda_heldout_elbo(mmm, tuning):
    c = R.PASS_LDA[0]
    X, lam0 = R.pass_lda(c)
    Xh, _ = R.pass_lda(dict(c, D=21), seed=77)
    tuning()
    g = mmm.LDA(c["K"], 0.1, 0.1, c["V"], X, λ0=lam0)
    mmm.fit(g, maxiter=5, tol=0.0, verbose=False)
    new = mmm.fit_heldout(Xh, g, maxiter=12)
    e, terms = mmm.calculate_elbo(new, terms=True)
    assert e == new.elbo
    st = _lda_readback(new, Xh)
    st["phi"] = new.phi_flat()
    t = R.lda_terms(st)
    n = R.lda_roundings(c["K"], c["V"], 21, max(x.shape[0] for x in Xh))
    _check("held-out", R.LDA_TERMS, e, terms, t, n)
    assert abs(float(np.longdouble(new.elbo) - R.total(t))) <= R.bound(t, n).sum()
    new.close(); g.close()


def test_ctm_heldout_elbo(mmm, tuning):
    c = R.PASS_CTM[0]
    lay, alpha, g0 = R.pass_ctm(c)
    layh, _, _ = R.pass_ctm(dict(c, D=21), seed=78)
    tuning()
    g = _ctm_handle(mmm, lay, None, alpha=alpha, gamma0=g0)
    mmm.fit(g, maxiter=3, tol=0.0, verbose=False)
    new = mmm.fit_heldout(layh.s.X, g, maxiter=4)
    e, terms = mmm.calculate_elbo(new, terms=True)
    st = _ctm_readback(new, layh)
    st["theta"] = new._get("theta")
    _check("held-out", R.CTM_TERMS, e, terms, R.ctm_terms(layh, st), R.ctm_roundings(layh))
    new.close(); g.close()
