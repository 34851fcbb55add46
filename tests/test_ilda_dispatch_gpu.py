"""ILDA on the device over its whole dispatch space, case by case (ilda_ref.draw_cases): every E-step build and both M-step
implementations (k_ilda_mstep; the ILDA branch of the merged reduce + ll + M-step launch, taken for V <= 256 and sum J <= 16) against
tests/ilda_ref.py -- the numpy restatement of ILDA.jl -- AND the C oracle, which tests/test_ilda_ref_cpu.py holds to each other.  The
tables go where the SNV3 table of test_ilda_gpu.py does not: one feature and eight, a feature of 200 values (the 64-value chunks of the
fold), sum J = 512, V > 256 (the fold loop over global memory), 1536 terms (tables beyond LDS), values no term carries, V < sum J, V no
multiple of 16, K = 1 / 33 / 65 / 100.

Bounds: six fused passes rtol 1e-9 on ll, λ, β, γ, θ, ELBO (the bound of test_random_shapes_every_estep_build_against_oracle), Elnβ
rtol 1e-8 with atol 1e-13 next to its zero; one stage from an uploaded state rtol 1e-13 on λ and γ, 1e-12 on Elnβ, Elnθ, ϕ, β, 1e-10 on
the ELBO terms (the bounds of the known-answer tests in test_ilda_gpu.py).  Every test prints the worst distance it saw."""
import ctypes as C

import numpy as np
import pytest

import ilda_ref
from ilda_ref import dist, heldout_docs, oracle_of

pytestmark = pytest.mark.gpu
CASES = ilda_ref.draw_cases()
BY = {c["name"]: c for c in CASES}
RUN = 1e-9              # six fused passes
RUN_ELN = 1e-8          # ... Elnβ, with atol 1e-13
PAIRS = {}              # case name -> settings that ran

# case/setting pairs of part (a) for the fixed list: 29 x ({}, grid_blocks, wide) + dense on the 18 cases with V <= 128 + (lda_merged
# off, resident_cap) on the 17 cases with V <= 256 and sum J <= 16 + lda_ll_join off on the 7 cases with D > 400
N_PAIRS = 29 * 3 + 18 + 2 * 17 + 7


def merged_shape(c):
    """The merged launch has an ILDA build for V <= 256 and sum J <= 16 (csrc/lda.hip fused_passes)."""
    return c["V"] <= 256 and sum(c["J"]) <= 16


def dense_build_exists(c):
    """mmm_lda_geometry [5] / MMM_BUILD_DENSE: rows of counts over <= 128 terms, no term listed twice in a document, 16-lane groups
    (K <= 15) with at least 4 padded topics and KP x slots <= 64 doubles per lane; other shapes fall back."""
    V, K = c["V"], c["K"]
    if V > 128 or K > 15 or K < 3:
        return False
    KP = next(o for o in (4, 6, 8, 10, 12, 16) if K <= o)
    SL = 2 if V <= 32 else (3 if V <= 48 else (6 if V <= 96 else 8))
    return KP * SL <= 64 and not any(len(set(x[:, 0])) < x.shape[0] for x in c["X"])


def settings_of(c):
    V, K = c["V"], c["K"]
    s = [{}, {"grid_blocks": 3}, {"lda_build": "wide"}]
    if V <= 128:
        s.append({"lda_build": "dense"})
    if merged_shape(c):
        Vp = (V + 15) & ~15
        s.append({"disable": ("lda_merged",)})
        s.append({"resident_cap": Vp * K // 16})          # one short of the launch's reduce blocks + 1: the split kernels run
    if c["D"] > 400:
        s.append({"disable": ("lda_ll_join",)})
    return s


def device_model(mmm, c, eta=None, features=None, lam0=None, X=None):
    return mmm.ILDA(c["K"], c["alpha"], c["eta"] if eta is None else eta, c["features"] if features is None else features,
                    c["X"] if X is None else X, λ0=c["lam0"] if lam0 is None else lam0)


def factors(g, name):
    flat = g._get(name)
    return [flat[g._ioff[i]:g._ioff[i + 1]].reshape(g.J[i], g.K, order="F") for i in range(g.I)]


def reference_runs(oracle, c, passes=6):
    r = ilda_ref.model_of(c)
    ll_r = r.fit(maxiter=passes, tol=0.0)
    o = oracle_of(oracle, c)
    ll_o = o.fit(maxiter=passes, tol=0.0)
    return r, ll_r, o, ll_o


def device_state(g):
    return dict(λ=factors(g, "ilambda"), Elnβ=factors(g, "iElnbeta"), β=factors(g, "ibeta"), γ=g.γ, θ=g.θ, elbo=g.elbo)


def state_distance(s, ll, ref_state, ref_ll, w, tag):
    """Worst relative distances of one device run from a reference state, accumulated into w under `tag`."""
    def put(k, v):
        w[(tag, k)] = max(w.get((tag, k), 0.0), v)
    put("ll", dist(ll, ref_ll))
    for i in range(len(s["λ"])):
        put("λ", dist(s["λ"][i], ref_state["λ"][i]))
        put("Elnβ", dist(s["Elnβ"][i], ref_state["Elnβ"][i], atol=1e-13))
        put("β", dist(s["β"][i], ref_state["β"][i]))
    put("γ", dist(s["γ"], ref_state["γ"]))
    put("θ", dist(s["θ"], ref_state["θ"]))
    put("elbo", dist(s["elbo"], ref_state["elbo"]))


def ref_state_of(r):
    return dict(λ=r.lam, Elnβ=r.Elnbeta, β=r.beta, γ=r.gamma, θ=r.theta, elbo=r.elbo)


def oracle_state_of(o):
    K, D, I = o.K, o.D, o.I
    return dict(λ=[o.mat(o.lam, i) for i in range(I)], Elnβ=[o.mat(o.Elnbeta, i) for i in range(I)], β=[o.mat(o.beta, i) for i in range(I)],
                γ=o.gamma.reshape(D, K).T, θ=o.theta.reshape(D, K).T, elbo=o.elbo_value)


def assert_run(w, name):
    for (tag, k), v in w.items():
        bound = RUN_ELN if k == "Elnβ" else RUN
        assert v <= bound, "%s: %s against %s differs by %.3g (bound %g)" % (name, k, tag, v, bound)


def ref_from_device(c, g, eta=None, features=None):
    """An ilda_ref model holding the device's own state."""
    r = ilda_ref.Ilda(c["K"], c["alpha"], c["eta"] if eta is None else eta, c["features"] if features is None else features, c["X"],
                      factors(g, "ilambda"))
    r.Elnbeta = factors(g, "iElnbeta"); r.beta = factors(g, "ibeta")
    r.gamma = g.γ; r.Elntheta = g.Elnθ; r.theta = g.θ
    r.phi = _phi_docs(g)
    return r


def _phi_docs(g):
    flat = g.phi_flat()
    return [flat[int(g._doc_ptr[d]):int(g._doc_ptr[d + 1])].T.copy() for d in range(g.D)]


# ----------------------------------------------------------------------------------------------------- (a), (c)
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_six_fused_passes_under_every_build(mmm, oracle, tuning, c):
    """(a) six `fit` passes (tol = 0) under every setting the shape has a build for, each against ilda_ref and the oracle: ll history,
    every λ[i], Elnβ[i], β[i], γ, θ, model.elbo.  (c) the seven ELBO terms of the default run against ilda_ref's evaluation of the state
    downloaded from the device."""
    name = c["name"]
    r, ll_r, o, ll_o = reference_runs(oracle, c)
    refs = {"ilda_ref": (ref_state_of(r), ll_r), "oracle": (oracle_state_of(o), ll_o)}
    runs = {}
    PAIRS[name] = []
    for env in settings_of(c):
        key = repr(env)
        tuning(**env)
        g = device_model(mmm, c)
        tuning()
        geo = g.geometry()
        if env.get("lda_build") == "wide":
            assert geo["wide"] == 1, (name, geo)
        if env.get("lda_build") == "dense" and dense_build_exists(c):
            assert geo["dense"] == 1, (name, geo)
        if name == "v257" and not env:
            assert geo["wide"] == 0, geo             # small tables above 256 terms: the LDS path with k_ilda_mstep's general fold loop
        if name == "penta" and not env:
            lda = mmm.LDA(c["K"], c["alpha"], 0.1, c["V"], c["X"], seed=1)
            assert geo["wide"] == 1 and geo == lda.geometry(), (geo, lda.geometry())      # ILDA runs the LDA E-step on effective tables
            lda.close()
        ll = mmm.fit(g, maxiter=6, tol=0.0, verbose=False)
        assert len(ll) == 6 and not g.converged
        s = device_state(g)
        w = {}
        for tag, (st, ll_ref) in refs.items():
            state_distance(s, ll, st, ll_ref, w, tag)
        print("\n%-15s %-32s %s" % (name, key, "  ".join("%s/%s %.1e" % (t[:3], k, v) for (t, k), v in sorted(w.items()) if t == "ilda_ref")))
        assert_run(w, "%s %s %s" % (name, key, geo))
        runs[key] = (s, ll)
        if not env:                                  # (c)
            e, t = mmm.calculate_elbo(g, terms=True)
            er, tr = ref_from_device(c, g).elbo_terms()
            d = max(dist(t, tr), dist(e, er))
            print("%-15s ELBO terms from the device's own state: %.1e" % (name, d))
            assert d <= 1e-10, (name, t, tr)
            assert e == pytest.approx(g.elbo, rel=1e-12)
        g.close()
        PAIRS[name].append(key)
    if merged_shape(c):                              # both M-step implementations on the same input, against each other
        a, b = runs[repr({})], runs[repr({"disable": ("lda_merged",)})]
        w = {}
        state_distance(a[0], a[1], b[0], b[1], w, "split kernels")
        print("%-15s merged launch against the split kernels: %s" % (name, "  ".join("%s %.1e" % (k, v) for (_, k), v in sorted(w.items()))))
        assert_run(w, name)
    assert len(PAIRS[name]) == len(settings_of(c))


def test_zz_every_pair_ran():
    """Runs after the parametrised test (later in the file).  With the whole file selected, every case/setting pair of the fixed list ran."""
    assert sum(len(settings_of(c)) for c in CASES) == N_PAIRS
    ran = sum(len(v) for v in PAIRS.values())
    print("\ncase/setting pairs run: %d of %d" % (ran, N_PAIRS))
    if len(PAIRS) == len(CASES):
        assert ran == N_PAIRS


@pytest.mark.parametrize("name", ["sj17", "I8", "v257"])
def test_elbo_keeps_the_last_feature_of_ElnQbeta(mmm, name):
    """(c) calculate_ElnQβ overwrites its accumulator per feature (ILDA.jl:174-181): the ELBO holds the LAST feature's term.  On cases
    where that differs from the sum over the features by more than 1 % (asserted, in both orders of the columns), the device's term is
    the last feature's; with the feature columns reversed (λ0, η alike) every other term is unchanged and ElnQβ is the other end's term."""
    c = BY[name]
    out = []
    for rev in (False, True):
        f = c["features"][:, ::-1] if rev else c["features"]
        lam0 = c["lam0"][::-1] if rev else c["lam0"]
        eta = c["eta"][::-1] if rev else c["eta"]
        g = device_model(mmm, c, eta=eta, features=f, lam0=lam0)
        mmm.fit(g, maxiter=6, tol=0.0, verbose=False)
        e, t = mmm.calculate_elbo(g, terms=True)
        r = ref_from_device(c, g, eta=eta, features=np.ascontiguousarray(f))
        q = [r.ElnQbeta_of(i) for i in range(c["I"])]
        assert abs(sum(q) - q[-1]) > 0.01 * abs(q[-1])          # the check discriminates
        assert t[4] == pytest.approx(q[-1], rel=1e-10)
        out.append((t, q))
        g.close()
    (t0, q0), (t1, q1) = out
    keep = [0, 1, 2, 3, 5, 6]
    print("\n%s: ElnQβ %.6g (features as given) / %.6g (reversed); other terms differ by %.1e" % (name, t0[4], t1[4], dist(t1[keep], t0[keep])))
    np.testing.assert_allclose(t1[keep], t0[keep], rtol=RUN)
    assert t1[4] == pytest.approx(q0[0], rel=RUN) and t0[4] == pytest.approx(q1[0], rel=RUN)


# ----------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", ["bigJ", "I8", "holes", "v257"])
def test_one_stage_from_an_uploaded_state(mmm, name):
    """(b) random ϕ (columns summing to 1) and random positive λ[i] uploaded, then one stage at a time against the single ilda_ref step
    from the same arrays; then Elnβ[i] / β[i] assigned: update_ϕ!, the log-likelihood and fit_heldout use the effective tables of the
    assigned factors."""
    c = BY[name]
    K, D, I, J = c["K"], c["D"], c["I"], c["J"]
    rng = np.random.Generator(np.random.PCG64([5, c["V"]]))
    phi = [np.ascontiguousarray(rng.dirichlet(np.full(K, 0.7), size=x.shape[0]).T) for x in c["X"]]
    lam = [rng.uniform(0.05, 60.0, size=(j, K)) for j in J]
    g = device_model(mmm, c)
    r = ilda_ref.model_of(c)
    w = {}
    # update_λ! (λ and Elnβ) from the uploaded ϕ
    g.ϕ = phi; r.phi = [p.copy() for p in phi]
    mmm.update_λ(g); r.update_lambda()
    w["update_λ λ"] = max(dist(a, b) for a, b in zip(factors(g, "ilambda"), r.lam))
    w["update_λ Elnβ"] = max(dist(a, b) for a, b in zip(factors(g, "iElnbeta"), r.Elnbeta))
    # update_Elnβ! alone, from an uploaded λ
    g.λ = lam; r.lam = [l.copy() for l in lam]
    mmm.update_Elnβ(g); r.update_Elnbeta()
    assert all(np.array_equal(a, b) for a, b in zip(factors(g, "ilambda"), lam))
    w["update_Elnβ Elnβ"] = max(dist(a, b) for a, b in zip(factors(g, "iElnbeta"), r.Elnbeta))
    mmm.update_β(g); r.update_beta()
    w["update_β β"] = max(dist(a, b) for a, b in zip(factors(g, "ibeta"), r.beta))
    # update_γ! (γ and Elnθ) from the uploaded ϕ
    mmm.update_γ(g); r.update_gamma()
    w["update_γ γ"] = dist(g.γ, r.gamma)
    w["update_γ Elnθ"] = dist(g.Elnθ, r.Elntheta)
    # update_ϕ! from the arrays the device holds
    r.Elntheta = g.Elnθ; r.Elnbeta = factors(g, "iElnbeta")
    mmm.update_ϕ(g); r.update_phi()
    w["update_ϕ ϕ"] = max(dist(a, b, atol=1e-300) for a, b in zip(_phi_docs(g), r.phi))
    # the ELBO of this state
    mmm.update_θ(g); r.update_theta()
    e, t = mmm.calculate_elbo(g, terms=True)
    er, tr = ref_from_device(c, g).elbo_terms()
    w["elbo terms"] = max(dist(t, tr), dist(e, er))
    # Elnβ[i] and β[i] assigned (not what λ implies): the effective tables follow
    lam2 = [rng.uniform(0.05, 60.0, size=(j, K)) for j in J]
    r2 = ilda_ref.Ilda(K, c["alpha"], c["eta"], c["features"], c["X"], lam2); r2.update_beta()
    g.Elnβ = r2.Elnbeta; g.β = r2.beta
    assert all(np.array_equal(a, b) for a, b in zip(factors(g, "iElnbeta"), r2.Elnbeta)) and all(np.array_equal(a, b) for a, b in zip(factors(g, "ibeta"), r2.beta))
    r.Elnbeta = r2.Elnbeta; r.beta = r2.beta
    mmm.update_ϕ(g); r.update_phi()
    w["assigned Elnβ ϕ"] = max(dist(a, b, atol=1e-300) for a, b in zip(_phi_docs(g), r.phi))
    r.theta = g.θ
    w["assigned β ll"] = dist(mmm.calculate_loglikelihood(g), r.loglikelihood())
    Xn = heldout_docs(c)
    hg = mmm.fit_heldout(Xn, g, maxiter=30)
    hr = r.fit_heldout(Xn, maxiter=30)
    assert len(hg.ll_history) == len(hr.ll_history) and hg.converged == hr.converged
    w["assigned heldout ll"] = dist(hg.ll_history, hr.ll_history)
    w["assigned heldout θ"] = dist(hg.θ, hr.theta)
    print("\n%s: %s" % (name, "  ".join("%s %.1e" % kv for kv in w.items())))
    bounds = {"update_λ λ": 1e-13, "update_γ γ": 1e-13, "elbo terms": 1e-10, "assigned heldout ll": RUN, "assigned heldout θ": RUN}
    for k, v in w.items():
        assert v <= bounds.get(k, 1e-12), "%s: %s differs by %.3g (bound %g)" % (name, k, v, bounds.get(k, 1e-12))
    hg.close(); g.close()


# ----------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("build", ["auto", "dense", "wide"])
@pytest.mark.parametrize("name", ["identity", "identity_small"])
def test_one_feature_whose_value_is_the_term_is_lda(mmm, tuning, name, build):
    """(d) features[v] = v: the ILDA handle against an LDA handle from the same λ0 -- ll history, λ[0] against λ, γ, the seven ELBO terms."""
    c = BY[name]
    tuning(lda_build=build)
    g = device_model(mmm, c)
    l = mmm.LDA(c["K"], c["alpha"], c["eta"][0], c["V"], c["X"], λ0=c["lam0"][0])
    tuning()
    ll_g = mmm.fit(g, maxiter=8, tol=0.0, verbose=False)
    ll_l = mmm.fit(l, maxiter=8, tol=0.0, verbose=False)
    tg = mmm.calculate_elbo(g, terms=True)[1]; tl = mmm.calculate_elbo(l, terms=True)[1]
    w = dict(ll=dist(ll_g, ll_l), λ=dist(g.λ[0], l.λ), γ=dist(g.γ, l.γ), elbo=dist(tg, tl))
    print("\n%s %s: ILDA against LDA %s" % (name, build, "  ".join("%s %.1e" % kv for kv in w.items())))
    assert max(w.values()) <= RUN, w
    g.close(); l.close()


@pytest.mark.parametrize("name", ["sj16", "holes", "bigJ"])
def test_relabelling_the_values_of_a_feature(mmm, name):
    """(d) the values of feature 0 permuted, the rows of λ0[0] alike: same ll history and γ, λ[0] permuted."""
    c = BY[name]
    J0 = c["J"][0]
    perm = np.concatenate([np.random.default_rng(3).permutation(J0 - 1), [J0 - 1]])   # new value of old value j (0-based); the top value stays, so J does
    f = c["features"].copy(); f[:, 0] = perm[f[:, 0] - 1] + 1
    lam0 = [l.copy() for l in c["lam0"]]
    lam0[0] = np.empty_like(c["lam0"][0]); lam0[0][perm] = c["lam0"][0]
    a = device_model(mmm, c); b = device_model(mmm, c, features=f, lam0=lam0)
    ll_a = mmm.fit(a, maxiter=6, tol=0.0, verbose=False); ll_b = mmm.fit(b, maxiter=6, tol=0.0, verbose=False)
    la, lb = factors(a, "ilambda"), factors(b, "ilambda")
    w = dict(ll=dist(ll_b, ll_a), γ=dist(b.γ, a.γ), λ0=dist(lb[0][perm], la[0]), λrest=max([dist(x, y) for x, y in zip(lb[1:], la[1:])] or [0.0]))
    print("\n%s relabelled: %s" % (name, "  ".join("%s %.1e" % kv for kv in w.items())))
    assert max(w.values()) <= RUN, w
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------- (e)
def _fits(mmm, c):
    g = device_model(mmm, c)
    ll = mmm.fit(g, maxiter=3, tol=0.0, verbose=False)
    g.close()
    return len(ll) == 3 and bool(np.all(np.isfinite(ll)))


def test_limits_are_refused_on_the_host_and_leave_the_context_usable(mmm):
    """(e) I = 8 and sum J = 512 create and fit; I = 9 and sum J = 513 are MMM_ERR_UNSUPPORTED with the limit in the message; a feature
    value outside 0..J_i-1 through the C entry is MMM_ERR_ARG.  All argument checks on the host, before any launch; after each refusal
    the context creates and fits another model."""
    small = BY["tiny"]
    assert BY["I8"]["I"] == 8 and _fits(mmm, BY["I8"])
    assert sum(BY["sj512"]["J"]) == 512 and _fits(mmm, BY["sj512"])
    rng = np.random.default_rng(9)
    X = small["X"]
    f9 = ilda_ref.random_table(rng, 5, [2] * 9)
    with pytest.raises(mmm.MmmError, match=r"status -4: .*I=9 features \(max 8\)"):
        mmm.ILDA(3, 0.1, 0.1, f9, X, seed=1)
    assert _fits(mmm, small)
    c = BY["sj512"]
    f513 = c["features"].copy(); f513[0, 2] = c["J"][2] + 1
    with pytest.raises(mmm.MmmError, match=r"status -4: .*sum\(J\)=513 \(max 512\)"):
        mmm.ILDA(c["K"], 0.1, 0.1, f513, c["X"], seed=1)
    assert _fits(mmm, small)
    # the C entry with J given: a value == J_i, then a negative one
    L, ctx = mmm.lib(), mmm.default_context()
    doc_ptr, term, count = mmm.pack_lda(X)
    J = np.array([3, 3], dtype=np.int32); eta = np.array([0.1, 0.1]); lam0 = np.ones(3 * 6)
    for bad in (3, -1):
        feat = np.ascontiguousarray((small["features"] - 1).T.ravel(), dtype=np.int32)
        feat[7] = bad
        h = C.c_void_p()
        rc = L.mmm_ilda_create(ctx.h, len(X), 5, 3, 0.1, 2, J, eta, feat, doc_ptr, term.ctypes.data, count.ctypes.data, lam0, C.byref(h))
        assert rc == -1 and not h.value                                           # MMM_ERR_ARG
        assert b"feature value out of range (i=1 v=2)" in L.mmm_last_error(ctx.h)
        assert _fits(mmm, small)


# ----------------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("name", ["sj16", "sj17", "v257"])
def test_eta_per_feature_changed_between_two_fits(mmm, name):
    """(f) model.η = [...] between two `fit` calls of three passes each (mmm_lda_set_hyper with one η per feature) against ilda_ref with
    the same switch, on the merged launch (sj16), k_ilda_mstep (sj17) and its general fold loop (v257)."""
    c = BY[name]
    eta2 = [0.7, 0.02, 1.3][:c["I"]]
    g = device_model(mmm, c); r = ilda_ref.model_of(c)
    ll1 = mmm.fit(g, maxiter=3, tol=0.0, verbose=False); ll1r = r.fit(maxiter=3, tol=0.0)
    g.η = np.array(eta2); r.eta = np.array(eta2)
    ll2 = mmm.fit(g, maxiter=3, tol=0.0, verbose=False); ll2r = r.fit(maxiter=3, tol=0.0)
    w = {}
    state_distance(device_state(g), np.concatenate([ll1, ll2]), ref_state_of(r), np.concatenate([ll1r, ll2r]), w, "ilda_ref")
    print("\n%s, η switched after three passes: %s" % (name, "  ".join("%s %.1e" % (k, v) for (_, k), v in sorted(w.items()))))
    assert_run(w, name)
    keep = ilda_ref.model_of(c); keep.fit(maxiter=6, tol=0.0)
    assert dist(keep.lam[0], r.lam[0]) > 1e-3                                      # the switch matters on this case
    g.close()


# ----------------------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("name", ["bigJ", "penta"])
def test_fit_heldout_against_the_frozen_loop(mmm, name):
    """(g) fit_heldout of a model fitted for six passes, against ilda_ref's frozen-topic loop (ILDA.jl:323-353): pass count, converged,
    ll history, θ, ELBO."""
    c = BY[name]
    g = device_model(mmm, c); r = ilda_ref.model_of(c)
    mmm.fit(g, maxiter=6, tol=0.0, verbose=False); r.fit(maxiter=6, tol=0.0)
    Xn = heldout_docs(c)
    hg = mmm.fit_heldout(Xn, g, maxiter=40)
    hr = r.fit_heldout(Xn, maxiter=40)
    assert len(hg.ll_history) == len(hr.ll_history) and hg.converged == hr.converged
    w = dict(ll=dist(hg.ll_history, hr.ll_history), θ=dist(hg.θ, hr.theta), elbo=dist(hg.elbo, hr.elbo))
    print("\n%s held out, %d passes, converged %s: %s" % (name, len(hr.ll_history), hr.converged, "  ".join("%s %.1e" % kv for kv in w.items())))
    assert max(w.values()) <= RUN, w
    hg.close(); g.close()
