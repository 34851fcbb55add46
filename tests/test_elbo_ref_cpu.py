"""tests/elbo_ref.py checked without a GPU: the C oracle (oracle/mmm_oracle.c: LdaOracle.elbo, IldaOracle.elbo, CtmOracle.elbo) and np_ref
against the restatement on the WRITTEN state of every case, term by term, within the bound the device is held to in
tests/test_elbo_gpu.py (max(γ_n A_t, 4 unit_t), n from the device kernels) -- so the reference alone stays inside that bound; the conditions
by which every case reaches the kernel, step count and LDS size it is there for, beside the arithmetic that derives them; and the margin
by which a θ (ϕ) taken one pass late would show in ElnPZ, ElnPX and ElnQZ, from the CPU oracle's trajectories.  The largest ratio per
term is printed (DESIGN.md sections 4.7 / 4.9 carry them)."""
import numpy as np
import pytest

import elbo_ref as R
import np_ref

LDA_NAMES = [c["name"] for c in R.LDA_CASES]
CTM_NAMES = [c["name"] for c in R.CTM_CASES]
WORST = {}


def _note(kind, names, r):
    w = WORST.setdefault(kind, np.zeros(7))
    np.maximum(w, np.where(np.isfinite(r), r, np.inf), out=w)
    return " ".join("%s %.3f" % (t, x) for t, x in zip(names, r))


def pow_allowance(weight):
    """ORACLE-ONLY allowance on ElnQZ.  The C oracle evaluates the reference's own expression log(θ ^ θ) (LDA.jl:157, MMCTM.jl:365): θ ^ θ lies in
    [e^(-1/e), 1], its rounding (pow within 2 u) becomes an ABSOLUTE 2 u in the logarithm, plus the logarithm's own rounding -- 3 u per
    summand times its count, however small θ log θ is.  The restatement, np_ref and the device (dev_xlogx) multiply θ by log θ and stay
    relative; they get no allowance."""
    out = np.zeros(7)
    out[6] = 3.0 * R.U * weight
    return out


# ---------------------------------------------------------------------------------------------------------- the oracle against the restatement
@pytest.mark.parametrize("name", LDA_NAMES)
def test_lda_oracle_meets_the_restatement(oracle, name):
    c, st = R.lda_written(name)
    t = R.lda_terms(st)
    n = R.lda_case_roundings(c)
    if st["features"] is None:
        o = oracle.LdaOracle(c["K"], st["alpha"], st["eta"], st["X"], V=c["V"], lambda0=st["lam"])
        o.Elnbeta[:] = st["Elnbeta"].ravel(order="F")
    else:
        o = oracle.IldaOracle(c["K"], st["alpha"], st["eta"], st["features"], st["X"], lambda0=np.concatenate([x.ravel(order="F") for x in st["lam"]]))
        o.Elnbeta[:] = np.concatenate([x.ravel(order="F") for x in st["Elnbeta"]])
    o.gamma[:] = st["gamma"].ravel(order="F"); o.Elntheta[:] = st["Elntheta"].ravel(order="F"); o.phi[:] = st["phi"].ravel()
    e, terms = o.elbo()
    r = R.ratios(terms, t, n, extra=pow_allowance(st["phi"].size))
    print("%-14s C oracle: %s" % (name, _note("lda_oracle", R.LDA_TERMS, r)))
    assert np.all(r <= 1.0), (name, r)
    assert abs(e - float(R.total(t))) <= R.bound(t, n).sum() + pow_allowance(st["phi"].size).sum()
    if st["features"] is None:
        phi_docs, a = [], 0
        for x in st["X"]:
            phi_docs.append(st["phi"][a:a + x.shape[0]].T); a += x.shape[0]
        _, tn = np_ref.lda_elbo(st["X"], c["K"], st["alpha"], st["eta"], st["lam"], st["Elnbeta"], st["gamma"], st["Elntheta"], phi_docs)
        r = R.ratios(tn, t, n)
        print("%-14s np_ref:   %s" % (name, _note("lda_np_ref", R.LDA_TERMS, r)))
        assert np.all(r <= 1.0), (name, r)


def ctm_oracle(oracle, lay, alpha_flat, gamma0):
    s = lay.s
    if lay.imm:
        off = np.concatenate([[0], np.cumsum(s.I)])
        alpha = [np.asarray(alpha_flat)[off[m]:off[m + 1]] for m in range(lay.M)]
        return oracle.CtmOracle(lay.K, alpha, s.X, features=s.features, gamma0=gamma0)
    return oracle.CtmOracle(lay.K, alpha_flat, s.X, V=lay.V, gamma0=gamma0)


@pytest.mark.parametrize("name", CTM_NAMES)
def test_ctm_oracle_meets_the_restatement(oracle, name):
    c, lay, st = R.ctm_written(name)
    t = R.ctm_terms(lay, st)
    n = R.ctm_roundings(lay, cus=1)
    o = ctm_oracle(oracle, lay, st["alpha"], st["gamma"])
    o.Elnphi[:] = st["Elnphi"]; o.mu[:] = st["mu"]; o.invSigma[:] = st["invSigma"].ravel()
    o.lam[:] = st["lam"].ravel(); o.nu[:] = st["nu"].ravel(); o.zeta[:] = st["zeta"].ravel(); o.theta[:] = st["theta"]
    e, terms = o.elbo()
    weight = sum(float(np.asarray(lay.s.X[d][m]).reshape(-1, 2)[:, 1].sum()) * lay.K[m] for d in range(lay.D) for m in range(lay.M))
    r = R.ratios(terms, t, n, extra=pow_allowance(weight))
    print("%-10s C oracle: %s" % (name, _note("ctm_oracle", R.CTM_TERMS, r)))
    assert np.all(r <= 1.0), (name, r)
    if not lay.imm:
        s = lay.s
        th = [[lay.theta_dm(st["theta"], d, m).T for m in range(lay.M)] for d in range(lay.D)]
        _, tn = np_ref.mmctm_elbo(s.X, lay.K, lay.V, st["alpha"], st["mu"], st["invSigma"], [s.unflatten(st["gamma"], m) for m in range(lay.M)],
                                  [s.unflatten(st["Elnphi"], m) for m in range(lay.M)], st["lam"], st["nu"], st["zeta"], th)
        r = R.ratios(tn, t, n)
        print("%-10s np_ref:   %s" % (name, _note("ctm_np_ref", R.CTM_TERMS, r)))
        assert np.all(r <= 1.0), (name, r)


def test_zz_print_worst():
    for k, v in WORST.items():
        print("worst %-11s %s" % (k, " ".join("%.3f" % x for x in v)))


# ---------------------------------------------------------------------------------------------------------- what every case is there for
def test_lda_cases_reach_what_they_are_for():
    """k_lda_elbo_docs holds one topic per lane (K <= 64), k_lda_elbo_docs_big topics l + 64 s in up to 4 slots; under geometry_cus = 1 the
    stage grid is min(ceil(D / 4), 4) blocks of 4 waves, so a wave takes ceil(D / (4 grid_s)) document steps; a lane takes ceil(W / 64) token
    steps; k_lda_elbo_topics strides V by 256 threads."""
    by = {c["name"]: c for c in R.LDA_CASES}
    slots = {c["name"]: -(-c["K"] // 64) for c in R.LDA_CASES}
    assert [n for n in by if by[n]["K"] > 64] == ["k65_v257_d17", "k128_v96_d3", "k129_v96_d16", "k256_v96_d1"]          # k_lda_elbo_docs_big
    assert by["k64_v256_d17"]["K"] == 64 and slots["k64_v256_d17"] == 1                                                    # the full wave
    assert slots["k65_v257_d17"] == 2 and 65 - 64 == 1                                                                     # one lane in the second slot
    assert slots["k128_v96_d3"] == 2 and slots["k129_v96_d16"] == 3 and slots["k256_v96_d1"] == 4
    assert {c["K"] for c in R.LDA_CASES if not c.get("J")} == {1, 2, 10, 63, 64, 65, 128, 129, 256}
    assert {c["V"] for c in R.LDA_CASES if not c.get("J")} == {1, 96, 255, 256, 257}
    assert {-(-c["V"] // 256) for c in R.LDA_CASES} == {1, 2}                                                               # 257: a second stride
    steps = {}
    for c in R.LDA_CASES:
        gs = R.lda_grid_s(c["D"], 1)
        assert gs <= 4
        steps[c["D"]] = (gs, -(-c["D"] // (4 * gs)))
    assert steps == {1: (1, 1), 3: (1, 1), 16: (4, 1), 17: (4, 2)}          # 17: a second step with one live wave (17 - 16 = 1)
    for big in (False, True):          # every document length under both document kernels
        seen = set()
        for c in R.LDA_CASES:
            if (c["K"] > 64) == big:
                seen |= set(R._lens(c["D"], c["lens"]))
        assert set(R.LEN_EDGES) <= seen, (big, seen)
    assert {-(-w // 64) for w in R.LEN_EDGES} == {0, 1, 2, 3}                # 0, 1, 63, 64 | 65 | 130 listed terms
    # the planted values
    st = R.lda_state(np.random.default_rng(2), by["k10_v96_d17"])
    assert set(R.SPECIAL) <= set(st["gamma"].ravel()) and (st["phi"] == 0).any()
    assert any(x[:, 1].max(initial=0) == 70000 for x in st["X"])
    assert any(len(set(x[:, 0])) < x.shape[0] for x in st["X"])              # a duplicated term
    # ILDA: I = 3 (SNV3) and I = 2 with unequal η
    assert by["ilda_snv3"]["J"] == (6, 4, 4) and len(set(by["ilda_i2_eta"]["eta"])) == 2


def test_ctm_cases_reach_what_they_are_for():
    """ΣK <= 64: k_ctm_elbo_docs<TAB_LDS> (TAB_LDS = the handle is not wide) and the LDS branch of k_ctm_elbo_topics; ΣK > 64: k_ctm_elbo_docs_big
    and the big_scratch branch.  Under geometry_cus = 1 the stage grid is min(ceil(D / 4), 3) blocks of 4 waves."""
    reach = {}
    for c in R.CTM_CASES:
        lay = R.ctm_layout(np.random.default_rng(0), c)
        wide = R.ctm_is_wide(lay, forced=c.get("build") == "wide")
        big = lay.MK > 64
        gs = R.ctm_grid_s(lay.D, 1)
        reach[c["name"]] = dict(kernel="big" if big else ("wide" if wide else "lds"), MK=lay.MK, M=lay.M, steps=-(-lay.D // (4 * gs)), gs=gs,
                                lds=R.elbo_docs_lds(lay, wide), wide=wide, tok=int(-(-lay.W.max() // 64)))
        assert gs <= 3
    k = lambda name: reach[name]["kernel"]
    assert [n for n in reach if k(n) == "big"] == ["k65", "k128", "k256"]                            # k_ctm_elbo_docs_big + big_scratch
    assert [n for n in reach if k(n) == "wide"] == ["k7_7_wide", "k33_4", "wide_tab"]                # k_ctm_elbo_docs<false>
    assert k("k7_7") == "lds" and R.ctm_case("k7_7_wide")["twin"] == "k7_7"                          # both TAB_LDS values on one state
    assert sorted(r["MK"] for r in reach.values() if r["MK"] not in (14, 37, 24, 5, 7, 8)) == [1, 2, 28, 63, 64, 65, 128, 256]
    assert {r["M"] for r in reach.values()} >= {1, 3, 8} and reach["m8_k1"]["MK"] == reach["m8_k1"]["M"] == 8   # lane < M and lane < ΣK coincide
    assert {reach[n]["steps"] for n in reach} == {1, 2} and reach["k2"]["steps"] == 1 and reach["k7_7"]["steps"] == 2   # D = 12 | 13
    assert all(r["tok"] >= 2 for n, r in reach.items() if n not in ("k1", "k2"))                     # 65 listed terms: a second token step
    # wide_tab: the table alone (K V = 16 700 + 8 260 doubles) is beyond the 160 KB a block can ask for; k33_4: a modality above 32 topics
    lay = R.ctm_layout(np.random.default_rng(0), R.ctm_case("wide_tab"))
    assert 8 * (16 * 700 + 8 * 260 + 64 + 16 * 700) > 160 * 1024 and R.ctm_is_wide(lay)
    # k64_lds48: create allows a non-wide handle (8 (2560 + 8 64 + 8 1280) = 106,496 B <= 150 KB) whose ELBO launch needs 8 (64^2 + 2560 + 256) =
    # 55,296 B > 48 KB of dynamic LDS: the hipFuncSetAttribute branch of elbo_enqueue
    r = reach["k64_lds48"]
    assert not r["wide"] and r["lds"] == 55296 and r["lds"] > 48 * 1024
    assert all(r["lds"] <= 48 * 1024 for n, r in reach.items() if n != "k64_lds48" and r["kernel"] != "big")
    # values
    lay, st = R.ctm_state(np.random.default_rng(1), R.ctm_case("k28"))
    assert st["nu"].min() == 1e-6 and st["nu"].max() == 50.0 and st["zeta"].min() == 1e-3 and st["zeta"].max() == 1e6
    assert (st["theta"] == 0).any() and np.abs(st["lam"]).max() <= 6 and st["mu"].mean() > 9
    assert np.linalg.cond(st["invSigma"]) <= 1e4 and np.array_equal(st["invSigma"], st["invSigma"].T)
    assert len(set(st["alpha"])) == lay.M
    assert (lay.W.sum(axis=1) == 0).any() and ((lay.W == 0).any(axis=1) & (lay.W.sum(axis=1) > 0)).any()     # empty everywhere / in one modality
    lay, st = R.ctm_state(np.random.default_rng(1), R.ctm_case("imm_2mod"))
    assert lay.s.I == [3, 2] and len(set(st["alpha"])) == 5                                         # different feature counts, α unequal per feature
    assert R.ctm_layout(np.random.default_rng(0), R.ctm_case("imm_snv3")).s.J == [[6, 4, 4]]


def test_pass_cases_meet_their_builds():
    for c in R.PASS_CTM:
        lay, _, _ = R.pass_ctm(c)
        forced = c["tune"].get("ctm_build")
        assert R.ctm_is_wide(lay, forced == "wide") == bool(c["geo"]["wide"]), c["name"]
        if c["geo"].get("tdense"):
            assert R.rows_of_counts_ok(lay), c["name"]
        assert lay.D <= 130 and max(lay.V) <= 300
    for c in R.PASS_LDA:
        X, _ = R.pass_lda(c)
        assert all(len(set(x[:, 0])) == x.shape[0] for x in X) and c["D"] <= 130
        assert (c["K"] > 64) == (c["name"] == "k65")


# ---------------------------------------------------------------------------------------------------------- staleness has to be visible
STALE = (2, 3, 6)          # ElnPZ, ElnPX, ElnQZ


@pytest.mark.parametrize("name", [c["name"] for c in R.PASS_LDA])
def test_lda_stale_phi_would_show(oracle, name):
    """ϕ of pass n is softmax(Elnθ_n + Elnβ_{n-1}); that of pass n - 1 in its place moves ElnPZ, ElnPX and ElnQZ by more than 1000 bounds"""
    c = next(x for x in R.PASS_LDA if x["name"] == name)
    X, lam0 = R.pass_lda(c)
    runs = []
    for k in (R.N_PASSES - 2, R.N_PASSES - 1, R.N_PASSES):
        o = oracle.LdaOracle(c["K"], 0.1, 0.1, X, V=c["V"], lambda0=lam0)
        o.fit(maxiter=k, tol=0.0)
        runs.append(o)
    mat = lambda a, r, cc: a.reshape(r, cc, order="F")
    o2, o1, o0 = runs[2], runs[1], runs[0]
    K, V, D = c["K"], c["V"], c["D"]
    st = dict(K=K, V=V, D=D, X=X, alpha=0.1, eta=0.1, features=None, lam=mat(o2.lam, V, K), Elnbeta=mat(o2.Elnbeta, V, K),
              gamma=mat(o2.gamma, K, D), Elntheta=mat(o2.Elntheta, K, D))
    phi_n = R.lda_phi(X, mat(o2.Elntheta, K, D), mat(o1.Elnbeta, V, K))
    phi_p = R.lda_phi(X, mat(o1.Elntheta, K, D), mat(o0.Elnbeta, V, K))
    tn, tp = R.lda_terms(R.with_phi(st, phi_n)), R.lda_terms(R.with_phi(st, phi_p))
    b = R.bound(tn, R.lda_roundings(K, V, D, max(x.shape[0] for x in X)))
    margin = np.abs((tn.value - tp.value).astype(np.float64)) / b
    print("%-12s stale/bound: %s" % (name, " ".join("%s %.2e" % (R.LDA_TERMS[i], margin[i]) for i in STALE)))
    assert all(margin[i] > 1000.0 for i in STALE), margin
    # and the oracle's own stored ϕ is that of pass n
    assert np.abs(o2.phi.reshape(-1, K) - phi_n.astype(np.float64)).max() < 1e-12


@pytest.mark.parametrize("name", [c["name"] for c in R.PASS_CTM])
def test_ctm_stale_theta_would_show(oracle, name):
    """θ of pass n is update_θ!(λ_{n-1}, Elnϕ_{n-1})"""
    c = next(x for x in R.PASS_CTM if x["name"] == name)
    lay, alpha, g0 = R.pass_ctm(c)
    aflat = np.concatenate([np.atleast_1d(a) for a in alpha]) if lay.imm else np.asarray(alpha)
    runs = []
    for k in (R.N_PASSES - 2, R.N_PASSES - 1, R.N_PASSES):
        o = ctm_oracle(oracle, lay, aflat, g0)
        o.fit(maxiter=k, tol=0.0)
        runs.append(o)
    o0, o1, o2 = runs
    st = dict(alpha=aflat, mu=o2.mu, invSigma=o2.invSigma.reshape(lay.MK, lay.MK), gamma=o2.gamma, Elnphi=o2.Elnphi, lam=o2.lam.reshape(lay.D, lay.MK),
              nu=o2.nu.reshape(lay.D, lay.MK), zeta=o2.zeta.reshape(lay.D, lay.M))
    th_n = R.theta_from(lay, o1.lam, o1.Elnphi); th_p = R.theta_from(lay, o0.lam, o0.Elnphi)
    tn, tp = R.ctm_terms(lay, R.with_theta(st, th_n)), R.ctm_terms(lay, R.with_theta(st, th_p))
    b = R.bound(tn, R.ctm_roundings(lay))
    margin = np.abs((tn.value - tp.value).astype(np.float64)) / b
    print("%-14s stale/bound: %s" % (name, " ".join("%s %.2e" % (R.CTM_TERMS[i], margin[i]) for i in STALE)))
    assert all(margin[i] > 1000.0 for i in STALE), margin
    assert np.abs(o2.theta - th_n.astype(np.float64)).max() < 1e-10
