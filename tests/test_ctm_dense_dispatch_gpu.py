"""The CTM kernels that run over lane-major rows of 16-bit counts -- k_ctm_theta_dense<KMX, SL> (ζ, θ n, Σθ, the γ statistics;
csrc/ctm_estep.cuh) and k_ctm_loglik_dense<KMX> (props, per-modality ll; csrc/ctm_mstep.cuh) -- on every build `launch_theta_dense` and
`run_loglik` dispatch, against tests/ctm_dense_ref.py: a numpy restatement of the reference's lines in np.longdouble that shares nothing
with the product or with oracle/ (the order-matched oracle of the bit-for-bit tests shares mmm_arith.h and the tables with the kernels and
mirrors their association, so a slot or a padded lane mis-indexed the same way in both passes there).

Every case writes λ (spread over ±6) and ν (0.05 ... 2), asserts `geometry()["tdense"]`, runs ONE fused pass and compares
  * ζ, γ, Elnϕ with the restatement of the written state and the Elnϕ the handle started from (neither depends on the LD_MMA solves),
  * props and ll with the restatement of the λ and γ read back after the pass (so the solves drop out again),
  * calculate_sumθ of a few documents: mmm_ctm_doc_sums does NOT return what k_ctm_theta_dense stored in `sumth` -- it sums the θ that is
    rebuilt on demand from the λ₍ₜ₋₁₎ and exp table the dense kernel KEPT (its lam_keep / expE_keep stores), which is what this checks,
  * the Σθ the kernel did store through the only thing that reads it, the λ solve: at its stationary point Σθ = Σ⁻¹(λ - μ) + (N / ζ) exp(λ +
    ν / 2) with the constructor's μ = 0, Σ⁻¹ = I, so the λ, ν, ζ read back imply a Σθ, held to the restatement's within what the solver's
    x-tolerance leaves (`_stationarity`).
Bounds: max(a-priori bound, F = 4 units), ctm_dense_ref.py; nothing is a measured tolerance.  The worst ratio per quantity and group is
printed by test_zz_report (DESIGN.md sections 4.4 / 4.7 carry the numbers).

Held-out inference: `frozen_pass` runs its θ phase without the γ slabs, so k_ctm_theta_dense is not reached; its ll launch is `run_loglik`,
so a dense held-out handle does reach k_ctm_loglik_dense (test_heldout_handle_over_rows_of_counts)."""
import ctypes as C

import numpy as np
import pytest

import ctm_dense_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
NAMES = [c["name"] for c in CASES]
BY_GROUP = {g: [c["name"] for c in CASES if c["group"] == g] for g in ("build", "mixed", "rows", "refused", "half", "grid")}
WORST = {}                     # (quantity, group) -> worst ratio
RAN = set()
_REF = {}                      # (case, bytes of the starting Elnϕ) -> R.Reference
_ORC = {}                      # case -> stationarity residual of the index-order oracle's pass (the unit of `_stationarity`)
FIELDS = ("lambda", "nu", "zeta", "gamma", "mu", "Sigma", "invSigma")
XTOL = 1e-4                    # xtol_rel of the LD_MMA solves (MMCTM.jl:129)


def _case(name):
    return CASES[NAMES.index(name)]


def _flat_g0(c, g0=None):
    g0 = c["g0"] if g0 is None else g0
    return g0 if c["features"] is not None else np.concatenate([np.asarray(g).ravel() for g in g0])


def _make(mmm, c, g0=None, restarts=None):
    g0 = c["g0"] if g0 is None else g0
    if c["features"] is not None:
        return mmm.IMMCTM(c["K"], c["alpha"], c["features"], c["X"], γ0=g0, restarts=restarts)
    return mmm.MMCTM(c["K"], c["alpha"], c["V"], c["X"], γ0=g0, restarts=restarts)


def _iterate(mmm, g, n=1):
    mmm._lib.check(mmm.lib().mmm_ctm_iterate(g._h, n, 1), g.ctx.h, "iterate")       # MMM_FIT_UPDATE_SIGMA


def _last_ll(mmm, g):
    ll = np.zeros(g.M); n = C.c_int()
    mmm._lib.check(mmm.lib().mmm_ctm_ll_history(g._h, ll.ctypes.data, 1, C.byref(n)), g.ctx.h, "ll_history")
    assert n.value == 1
    return ll


def _reference(c, s, lam, nu, E0):
    key = (c["name"], lam.tobytes()[:64], E0.tobytes())
    if key not in _REF:
        _REF[key] = R.Reference(s, lam, nu, E0)
    return _REF[key]


def _implied_residual(s, lam1, nu1, zeta, sumth_ref):
    """|λ + (N / ζ) exp(λ + ν / 2) - Σθ| / (|Σθ| + |λ| + 1) per coordinate, [D, ΣK]: the gradient of the λ objective (common.jl:11-23) under
    μ = 0, Σ⁻¹ = I, scaled."""
    lam1 = np.reshape(lam1, (s.D, s.MK)).astype(R.LD); nu1 = np.reshape(nu1, (s.D, s.MK)).astype(R.LD); zeta = np.reshape(zeta, (s.D, s.M)).astype(R.LD)
    c = np.concatenate([np.repeat((s.N[m].sum(axis=1).astype(R.LD) / zeta[:, m])[:, None], s.K[m], axis=1) for m in range(s.M)], axis=1)
    sth = np.asarray(sumth_ref, dtype=R.LD)
    return np.asarray(np.abs(lam1 + c * np.exp(lam1 + R.LD(0.5) * nu1) - sth) / (np.abs(sth) + np.abs(lam1) + 1), dtype=np.float64)


def _stationarity(oracle, c, s, ref, lam1, nu1, zeta):
    """The Σθ that k_ctm_theta_dense stored is read by the λ solve alone.  LD_MMA stops when a step's Σ|Δλ| < xtol Σ|λ| (or every |Δλ_k| <
    1e-4); a step Δλ moves coordinate k of the gradient by (1 + (N / ζ) exp(λ_k + ν_k / 2)) Δλ_k, and (N / ζ) exp(...) = Σθ_k - λ_k at the
    stationary point, so in the scale |Σθ| + |λ| + 1 the residual left is at most Σ|Δλ| < xtol Σ_k |λ_k|.  The bound is the larger of that and
    F times the residual of the index-order oracle's own pass from the same state (the reference's own error).  -> worst ratio."""
    if c["name"] not in _ORC:
        o = oracle.CtmOracle(c["K"], c["alpha"], c["X"], V=None if s.imm else c["V"], features=c["features"], gamma0=_flat_g0(c))
        o.lam[:] = c["lam"].ravel(); o.nu[:] = c["nu"].ravel()
        o.fit(maxiter=1, tol=0.0)
        _ORC[c["name"]] = float(_implied_residual(s, o.lam, o.nu, o.zeta, ref.ld["sumth"]).max())
    res = _implied_residual(s, lam1, nu1, zeta, ref.ld["sumth"])
    if not np.all(np.isfinite(res)):
        return float("inf")
    bound = np.maximum(R.F * _ORC[c["name"]], XTOL * np.abs(np.reshape(lam1, (s.D, s.MK))).sum(axis=1, keepdims=True))
    return float((res / bound).max())


def _check(c, r, what):
    for q, v in r.items():
        key = (q, c["group"])
        WORST[key] = max(WORST.get(key, 0.0), v)
    print("%-18s %-30s %s" % (c["name"], what, " ".join("%s %.3f" % kv for kv in r.items())))
    bad = {q: v for q, v in r.items() if not v <= 1.0}
    assert not bad, "%s: off by (in units of the bound) %s" % (c["name"], bad)


def _sample_docs(s):
    """first, last, two in between and the emptiest document"""
    tot = sum(n.sum(axis=1) for n in s.N)
    return sorted({0, s.D - 1, s.D // 2, s.D // 3, int(np.argmin(tot))})


def _pass_and_compare(mmm, oracle, tuning, c):
    s = R.spec_of(c)
    tuning(ctm_build="dense", **c["tune"])
    g = _make(mmm, c)
    tuning()
    geo = g.geometry()
    builds, kmx = R.dense_build(c["K"], c["V"])
    assert geo["tdense"] == int(c["dense"]), (c["name"], geo)
    if c["tune"].get("grid_blocks"):
        assert geo["grid_e"] == c["tune"]["grid_blocks"]
    g._set("lambda", c["lam"].ravel()); g._set("nu", c["nu"].ravel())
    E0 = g._get("Elnphi")
    _iterate(mmm, g)
    zeta, gamma, Eln, lam1, nu1 = g._get("zeta"), g._get("gamma"), g._get("Elnphi"), g._get("lambda"), g._get("nu")
    props, ll = g._get("props"), _last_ll(mmm, g)
    docs = _sample_docs(s)
    sumth = np.stack([mmm.calculate_sumθ(g, d) for d in docs])
    g.close()
    ref = _reference(c, s, c["lam"], c["nu"], E0)
    r = ref.compare_state(zeta, gamma, Eln, sumth=sumth, docs=docs)
    r.update(ref.compare_after(lam1, gamma, props, ll)[0])
    r["stationary"] = _stationarity(oracle, c, s, ref, lam1, nu1, zeta)
    what = ("theta %s ll <%d>" % (" ".join("(%d,%d)" % b for b in builds), kmx)) if c["dense"] else "slabs (tdense 0)"
    _check(c, r, what)
    RAN.add(c["name"])


# ------------------------------------------------------------------------------------------ every build, the mixed handles, the rows
@pytest.mark.parametrize("name", BY_GROUP["build"] + BY_GROUP["mixed"] + BY_GROUP["rows"] + BY_GROUP["half"])
def test_rows_of_counts_builds_meet_the_restatement(mmm, oracle, tuning, name):
    _pass_and_compare(mmm, oracle, tuning, _case(name))


# ------------------------------------------------------------------------------------------ refusals: the slab kernels, same comparison
@pytest.mark.parametrize("name", BY_GROUP["refused"])
def test_refused_corpora_take_the_slab_kernels_and_meet_the_restatement(mmm, oracle, tuning, name):
    _pass_and_compare(mmm, oracle, tuning, _case(name))


# ------------------------------------------------------------------------------------------ grid edges (the arithmetic: ctm_dense_ref.GRID_EDGES)
@pytest.mark.parametrize("name", BY_GROUP["grid"])
def test_grid_edges(mmm, oracle, tuning, name):
    _pass_and_compare(mmm, oracle, tuning, _case(name))


# ------------------------------------------------------------------------------------------ the ll switch
def _bits(a, b, what):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel(); b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    k = int((a.view(np.int64) != b.view(np.int64)).sum())
    assert k == 0, "%s: %d of %d values differ in their bits (max abs diff %.3g)" % (what, k, a.size, np.abs(a - b).max())


@pytest.mark.parametrize("name", ["mix8_9", "imm_snv3"])
def test_ll_switch_sends_a_rows_handle_through_the_csr_sweep(mmm, tuning, name):
    """`disable=("ctm_ll_rows",)`: the handle keeps its rows of counts (tdense = 1) and its ll launch is k_ctm_loglik over the (term, count)
    lists.  props and ll are outside the feedback loop: the state is bit-equal over three passes, props / ll of both meet the restatement."""
    c = _case(name)
    s = R.spec_of(c)
    out = {}
    for key, off in (("rows", ()), ("csr", ("ctm_ll_rows",))):
        tuning(ctm_build="dense", disable=off)
        g = _make(mmm, c)
        tuning()
        assert g.geometry()["tdense"] == 1
        g._set("lambda", c["lam"].ravel()); g._set("nu", c["nu"].ravel())
        hist = []
        for it in range(3):
            before = (g._get("lambda"), g._get("nu"), g._get("Elnphi"))
            _iterate(mmm, g)
            hist.append({f: g._get(f) for f in FIELDS + ("Elnphi",)})
        out[key] = (hist, before, g._get("props"), _last_ll(mmm, g))
        g.close()
    for it in range(3):
        for f in FIELDS + ("Elnphi",):
            _bits(out["rows"][0][it][f], out["csr"][0][it][f], "%s after pass %d, rows against csr ll sweep" % (f, it + 1))
    for key in ("rows", "csr"):
        hist, (lam2, nu2, E2), props, ll = out[key]
        ref = _reference(c, s, lam2.reshape(s.D, s.MK), nu2.reshape(s.D, s.MK), E2)
        r = ref.compare_state(hist[2]["zeta"], hist[2]["gamma"], hist[2]["Elnphi"])
        r.update(ref.compare_after(hist[2]["lambda"], hist[2]["gamma"], props, ll)[0])
        _check(dict(c, group="llswitch_" + key), r, "third pass, ll over %s" % key)
    d = float(np.abs(out["rows"][3] - out["csr"][3]).max())
    print("ll rows - ll csr: %.2e" % d)
    RAN.add("llswitch_" + name)


# ------------------------------------------------------------------------------------------ a batch with a stopped replica
def test_batch_with_the_middle_replica_stopped(mmm, tuning):
    """R = 3 over the mixed-KMX corpus of mix2_16.  The stopping rule needs more than ten rows (MMCTM.jl:485), so: eleven passes with tol = 0
    give every replica's relative ll change at row 11; with tol between the smallest and the next, the replica with the smallest (put in
    the middle) stops after pass 11 and pass 12 runs with it inactive.  Batched fits are deterministic, so the state after eleven passes
    (handle A) is the state pass 12 of handle B starts from: replicas 0 and 2 of B meet the restatement of A's state, replica 1 of B equals
    A's in every bit."""
    c = _case("mix2_16")
    s = R.spec_of(c)
    inits = [[np.random.default_rng([41, r, m]).integers(1, 101, size=(c["K"][m], c["V"][m])).astype(np.float64) for m in range(s.M)] for r in range(3)]

    def batch(g0, maxiter, tol):
        tuning(ctm_build="dense")
        g = _make(mmm, c, g0=g0, restarts=3)
        tuning()
        assert g.geometry()["tdense"] == 1
        for r in range(3):
            g.select(r)
            g._set("lambda", c["lam"].ravel()); g._set("nu", c["nu"].ravel())
        return g, mmm.fit_restarts(g, maxiter=maxiter, tol=tol)

    g, h = batch(inits, 11, 0.0)
    g.close()
    rel = np.array([np.abs((x[9] - x[10]) / x[10]).max() for x in h])
    order = np.argsort(rel)
    assert rel[order[0]] < rel[order[1]]
    tol = float(np.sqrt(rel[order[0]] * rel[order[1]]))
    inits = [inits[order[1]], inits[order[0]], inits[order[2]]]
    A, hA = batch(inits, 11, tol)
    B, hB = batch(inits, 12, tol)
    assert list(A.restart_iters) == [11, 11, 11] and list(A.restart_converged) == [False, True, False]
    assert list(B.restart_iters) == [12, 11, 12]
    every = FIELDS + ("Elnphi", "props")
    A.select(1); B.select(1)
    for f in every:
        _bits(B._get(f), A._get(f), "replica 1 (stopped), %s" % f)
    _bits(hB[1], hA[1], "replica 1, ll history")
    for r in (0, 2):
        A.select(r); B.select(r)
        lam, nu, E = A._get("lambda").reshape(s.D, s.MK), A._get("nu").reshape(s.D, s.MK), A._get("Elnphi")
        ref = R.Reference(s, lam, nu, E)
        rr = ref.compare_state(B._get("zeta"), B._get("gamma"), B._get("Elnphi"))
        rr.update(ref.compare_after(B._get("lambda"), B._get("gamma"), B._get("props"), hB[r][11])[0])
        _check(dict(c, group="batch"), rr, "replica %d, pass 12" % r)
        assert not np.array_equal(B._get("lambda"), A._get("lambda"))
    A.close(); B.close()
    RAN.add("batch")


# ------------------------------------------------------------------------------------------ held-out inference
def test_heldout_handle_over_rows_of_counts(mmm, tuning):
    """fit_heldout (MMCTM.jl:554-586) on dense held-out documents: the new handle takes rows of counts, its frozen passes run the slab-less θ
    phase and k_ctm_loglik_dense.  First pass: ζ of the constructor's λ = 0, ν = 1; then a second frozen pass from a written state."""
    c = _case("mix8_9")
    tuning(ctm_build="dense")
    model = _make(mmm, c)
    mmm.fit(model, maxiter=2, tol=0.0, verbose=False)
    Xh = R.heldout_docs(c)
    new = mmm.fit_heldout(Xh, model, maxiter=1)
    tuning()
    assert model.geometry()["tdense"] == 1 and new.geometry()["tdense"] == 1
    s = R.Spec(c["K"], c["alpha"], c["V"], Xh)
    gamma, E = model._get("gamma"), model._get("Elnphi")
    hc = dict(c, group="heldout", name="heldout")

    def compare(lam, nu, ll, what):
        ref = R.Reference(s, lam, nu, E)
        r = dict(zeta=R.ratio_rel(new._get("zeta").reshape(s.D, s.M), ref.ld["zeta"], ref.bound["zeta"], ref.unit["zeta"]))
        r.update(ref.compare_after(new._get("lambda"), gamma, new._get("props"), ll)[0])
        _check(hc, r, what)

    compare(np.zeros((s.D, s.MK)), np.ones((s.D, s.MK)), new.ll_history[-1], "first frozen pass")
    _bits(new._get("gamma"), gamma, "held-out handle: gamma is the model's")
    rng = np.random.default_rng(9)
    lam, nu = R.state(rng, s.D, s.MK)
    new._set("lambda", lam.ravel()); new._set("nu", nu.ravel())
    hist = mmm.inference._ctm_infer(new, 0, 1, 1e-4, False)
    compare(lam, nu, hist[-1], "frozen pass from a written state")
    new.close(); model.close()
    RAN.add("heldout")


def test_zz_report(request):
    """Runs after the others (later in the file): the worst ratio per quantity and group; with the whole file selected, every case ran."""
    groups = sorted({g for _, g in WORST})
    qs = ("zeta", "gamma", "Elnphi", "sumth", "stationary", "props", "ll")
    print("\nworst ratio to max(a-priori bound, 4 units)\n%-16s %s" % ("group", " ".join("%10s" % q for q in qs)))
    for g in groups:
        print("%-16s %s" % (g, " ".join("%10s" % ("%.3f" % WORST[(q, g)] if (q, g) in WORST else "-") for q in qs)))
    whole = not request.config.getoption("keyword") and not any("::" in a for a in request.config.args)
    if whole:
        want = set(NAMES) | {"llswitch_mix8_9", "llswitch_imm_snv3", "batch", "heldout"}
        assert RAN == want, sorted(want ^ RAN)
