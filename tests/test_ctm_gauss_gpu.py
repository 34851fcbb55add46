"""The Gaussian M-step of the CTM on the device -- update_μ! / update_Σ! / inv(Σ) (MMCTM.jl:200-212): k_ctm_moments, k_reduce_partials,
ctm_gauss_mstep with its three Gauss-Jordan inversions (block_inverse_pipelined for ΣK <= 32, block_inverse_wide for 33 ... 64 and where
`ctm_pipe_gauss` is switched off, block_inverse_big beyond) -- on inputs at which every branch of them runs.

The states come from tests/gauss_ref.py and are uploaded through the stage API (`g.λ = …; g.ν = …; update_μ(g); update_Σ(g)`).  The
suite's other inputs are Σ that fits produce, nearly diagonally dominant: counted on the CPU, the eliminations of
test_ctm_gpu.py::test_estep_mstep_against_oracle swap rows at 1 of 156 columns and those of ::test_random_shapes_bit_identical_to_oracle
at 2 of 1071.  On the "pivot" states here they swap at 20 of 32, 34 of 64, 162 of 256 columns, always at column 0 and in the last three
(asserted in tests/test_gauss_ref_cpu.py), so the swap branches of all three builds, of the look-ahead of the pipelined one and of the
ELBO's log det run with operands that differ.

  (a) μ, Σ, Σ^-1 equal, bit for bit, the order-matched oracle's (orc_twin_moments + orc_twin_gauss at the handle's grid_m): every size of
      gauss_ref.cases() x {pivot, typical, shifted(100)}; for ΣK <= 32 also with `ctm_pipe_gauss` off, and both device results equal;
      for ΣK = 28 and 65 also with 3 moment blocks and with D + 5 (blocks with an empty document range).
  (b) the same results against np.longdouble: Σ within gauss_ref.sigma_bound (derived, a priori) of the reference's centred formula,
      Σ^-1 within F = 4 units of gauss_ref.inv_error_bound of the LU + Newton-Schulz inverse; shifts 10, 100, 1000 at ΣK = 10 and 65.
  (c) a μ set by hand (update_Σ! alone: the branch that reads the stored μ with a μ that is not the mean).
  (d) the ELBO's terms after the pivot update against the literal oracle with the device's state copied in, rtol 1e-9: the log det is
      block_inverse_wide for every ΣK <= 64 and block_inverse_big beyond.
  (e) an exactly singular Σ is a reported status (MMM_ERR_NUMERIC, -5), with the zero pivot at column 0 and at column 1 (inside the
      look-ahead of the pipelined build); the context goes on working.
  (f) `ctm_pipe_gauss` and `ctm_fused_gauss` inside two-pass fits: the M-step as an extra block of k_ctm_loglik / k_ctm_loglik_dense and
      as its own launch, single fits and a batch of three -- every bit of μ, Σ, Σ^-1, the ll history and the ELBO equal across the four.

Uploaded pivot-prone states cannot reach the fused launch contexts -- a pass solves λ again before its M-step -- so (f) covers those
contexts on the states fits produce and (a) covers the branches.  Every test prints the ratios it saw; test_zz_every_case_ran counts."""
import numpy as np
import pytest

import gauss_ref as G
import np_ref

pytestmark = pytest.mark.gpu

LD = G.LD
CASES = G.cases()
SPLIT = dict(CASES)
KINDS_A = ("pivot", "typical", "shifted")
MB_SIZES = (28, 65)                       # sizes that also run with 3 and with D + 5 moment blocks
SHIFT_SIZES, SHIFTS = (10, 65), (10.0, 100.0, 1000.0)
MU_SIZES = (10, 33, 65)
ELBO_SIZES = (10, 32, 33, 64, 65, 256)
SING_SIZES = (2, 32, 33, 65)
FIT_CASES = ("dense10", "sparse28", "batch3")
FIT_SETTINGS = {"default": (), "pipe_off": ("ctm_pipe_gauss",), "fused_off": ("ctm_fused_gauss",), "both_off": ("ctm_pipe_gauss", "ctm_fused_gauss")}
N_TRIPLES = 148                           # (case, kind, setting) triples of the whole file: see _expected()
RAN = set()
_REF = {}                                 # Σ (bytes) -> (bound, X, log det, unit) of gauss_ref.inv_error_bound
_DEV = {}                                 # (n, kind, shift, setting) -> (lam, nu, μ, Σ, Σ^-1, grid_m)


def _settings(n):
    s = ["default"]
    if n <= 32:
        s.append("pipe_off")
    if n in MB_SIZES:
        s += ["blocks3", "blocksD5"]
    return s


def _sing_settings(n):
    return ["default", "pipe_off"] if n <= 32 else ["default"]


def _expected():
    e = set()
    for n, _ in CASES:
        for kind in KINDS_A:
            e |= {(n, kind, s) for s in _settings(n)} | {(n, kind, "accuracy")}
    e |= {(n, "shifted%g" % s, "default") for n in SHIFT_SIZES for s in SHIFTS if s != 100.0}
    e |= {(n, "pivot", "mu_by_hand") for n in MU_SIZES} | {(n, "pivot", "elbo") for n in ELBO_SIZES}
    e |= {(n, kind, s) for n in SING_SIZES for kind in ("singular0", "singular_mid") for s in _sing_settings(n)}
    e |= {(c, "fit", s) for c in FIT_CASES for s in FIT_SETTINGS}
    return e


def _tune(tuning, n, setting):
    D = 2 * n + 3
    tuning(**{"default": {}, "pipe_off": dict(disable=("ctm_pipe_gauss",)), "blocks3": dict(moment_blocks=3), "blocksD5": dict(moment_blocks=D + 5)}[setting])


def _model(mmm, n):
    K = SPLIT[n]
    X, V = G.corpus(n, K)
    g0 = [np.random.default_rng([n, m]).integers(1, 101, size=(K[m], V[m])).astype(np.float64) for m in range(len(K))]
    return mmm.MMCTM(K, [0.1] * len(K), V, X, γ0=g0), X, V, g0


def _bits(a, b, what):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel(); b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    k = int((a.view(np.int64) != b.view(np.int64)).sum())
    assert k == 0, "%s: %d of %d values differ in their bits (max abs diff %.3g)" % (what, k, a.size, np.abs(a - b).max())


def _device(mmm, tuning, n, kind, setting="default", shift=100.0):
    """update_μ! + update_Σ! of the uploaded state on the device, once per (size, kind, setting)"""
    key = (n, kind, shift, setting)
    if key not in _DEV:
        _tune(tuning, n, setting)
        g = _model(mmm, n)[0]
        tuning()
        lam, nu = G.state(n, kind, shift=shift)
        g.λ = lam; g.ν = nu
        mmm.update_μ(g); mmm.update_Σ(g)
        _DEV[key] = (lam, nu, np.array(g.μ), np.array(g.Σ), np.array(g.invΣ), g.geometry()["grid_m"], g)
        if not (kind == "pivot" and setting == "default" and n in ELBO_SIZES):      # (d) goes on with that handle
            g.close()
    return _DEV[key]


def _twin_bits(oracle, n, dev, what):
    lam, nu, mu, S, Si, grid_m = dev[:6]
    rc, tmu, tS, tSi, _ = G.twin(oracle, n, SPLIT[n], lam, nu, grid_m)
    assert rc == 0
    _bits(mu, tmu, what + " mu"); _bits(S, tS, what + " Sigma"); _bits(Si, tSi, what + " invSigma")


def _ref(oracle, S):
    k = S.tobytes()
    if k not in _REF:
        _REF[k] = G.inv_error_bound(oracle, S)
    return _REF[k]


def _accuracy(oracle, lam, nu, mu, S, Si, what):
    """Σ against the centred formula at the device's μ within sigma_bound, Σ^-1 against the np.longdouble inverse of the device's Σ within
    the F-bound; returns (Σ error / bound, Σ^-1 error / unit, relative error of Σ)."""
    eS = np.abs(S.astype(LD) - G.sigma_ref(lam, nu, mu))
    rS = float((eS / G.sigma_bound(lam, nu, mu)).max())
    bound, X, _, unit = _ref(oracle, S)
    err = float(np.abs(Si.astype(LD) - X).max())
    rel = float(eS.max() / np.abs(S).max())
    print("%s: Σ rel err %.2e = %.3f of its bound; Σ^-1 off by %.2e = %.2f units (bound 4)" % (what, rel, rS, err, err / unit))
    assert rS <= 1.0, what
    assert err <= bound, what
    return rS, err / unit, rel


# ------------------------------------------------------------------------------------------ (a) bits against the twin
@pytest.mark.parametrize("kind", KINDS_A)
@pytest.mark.parametrize("n", [n for n, _ in CASES])
def test_bits_against_the_order_matched_oracle(mmm, oracle, tuning, n, kind):
    res = {}
    for setting in _settings(n):
        res[setting] = _device(mmm, tuning, n, kind, setting)
        if setting.startswith("blocks"):
            assert res[setting][5] == (3 if setting == "blocks3" else 2 * n + 8)
        _twin_bits(oracle, n, res[setting], "ΣK = %d %s [%s]" % (n, kind, setting))
        RAN.add((n, kind, setting))
    if "pipe_off" in res:
        for i, f in ((2, "mu"), (3, "Sigma"), (4, "invSigma")):
            _bits(res["default"][i], res["pipe_off"][i], "ΣK = %d %s: %s, pipelined against wide" % (n, kind, f))


# ------------------------------------------------------------------------------------------ (b) accuracy against extended precision
@pytest.mark.parametrize("kind", KINDS_A)
@pytest.mark.parametrize("n", [n for n, _ in CASES])
def test_accuracy_against_longdouble(mmm, oracle, tuning, n, kind):
    lam, nu, mu, S, Si = _device(mmm, tuning, n, kind)[:5]
    _accuracy(oracle, lam, nu, mu, S, Si, "ΣK = %d %s" % (n, kind))
    RAN.add((n, kind, "accuracy"))


@pytest.mark.parametrize("n", SHIFT_SIZES)
def test_what_the_raw_moment_form_loses_to_a_shift(mmm, oracle, tuning, n):
    """|μ| >> the spread of λ: Σλλ' - μΣλ' - Σλμ' + Dμμ' cancels where the reference's centred sum does not.  The loss is bounded a priori
    (sigma_bound grows with D|μ_i μ_j|) and measured: the table of DESIGN.md section 4.6."""
    for shift in SHIFTS:
        kind = "shifted" if shift == 100.0 else "shifted%g" % shift
        dev = _device(mmm, tuning, n, "shifted", shift=shift)
        _twin_bits(oracle, n, dev, "ΣK = %d shift %g" % (n, shift))
        lam, nu, mu, S, Si = dev[:5]
        _accuracy(oracle, lam, nu, mu, S, Si, "ΣK = %d shift %g" % (n, shift))
        if shift != 100.0:
            RAN.add((n, kind, "default"))


# ------------------------------------------------------------------------------------------ (c) μ set by hand
@pytest.mark.parametrize("n", MU_SIZES)
def test_update_Sigma_with_a_mu_that_is_not_the_mean(mmm, oracle, n):
    g = _model(mmm, n)[0]
    lam, nu = G.state(n, "pivot")
    mu = lam.mean(axis=0) + 0.25 * lam.std(axis=0) * np.random.default_rng(n).standard_normal(n)
    g.λ = lam; g.ν = nu; g.μ = mu
    mmm.update_Σ(g)
    _bits(g.μ, mu, "mu after update_Σ!")
    _accuracy(oracle, lam, nu, mu, np.array(g.Σ), np.array(g.invΣ), "ΣK = %d, μ by hand" % n)
    RAN.add((n, "pivot", "mu_by_hand"))


# ------------------------------------------------------------------------------------------ (d) the ELBO's log det
@pytest.mark.parametrize("n", ELBO_SIZES)
def test_elbo_terms_after_the_pivot_update(mmm, oracle, tuning, n):
    g = _device(mmm, tuning, n, "pivot")[6]
    K = SPLIT[n]
    X, V = G.corpus(n, K)
    e, t = mmm.calculate_elbo(g, terms=True)
    o = oracle.CtmOracle(K, [0.1] * len(K), X, V=V, gamma0=g._get("gamma"))
    o.lam[:] = g.lam_matrix().ravel(); o.nu[:] = g.nu_matrix().ravel(); o.zeta[:] = g._get("zeta"); o.theta[:] = g._get("theta")
    o.mu[:] = g.μ; o.Sigma[:] = np.asarray(g.Σ).ravel(order="F"); o.invSigma[:] = np.asarray(g.invΣ).ravel(order="F")
    o.gamma[:] = g._get("gamma"); o.Elnphi[:] = g._get("Elnphi")
    eo, to = o.elbo()
    print("ΣK = %d: ELBO terms rel err %s" % (n, " ".join("%.1e" % x for x in np.abs(np.asarray(t) / to - 1))))
    np.testing.assert_allclose(t, to, rtol=1e-9)
    assert e == pytest.approx(eo, rel=1e-9)
    RAN.add((n, "pivot", "elbo"))


# ------------------------------------------------------------------------------------------ (e) singular Σ
@pytest.mark.parametrize("kind", ["singular0", "singular_mid"])
@pytest.mark.parametrize("n", SING_SIZES)
def test_singular_Sigma_is_a_reported_status(mmm, oracle, tuning, n, kind):
    lam, nu = G.state(n, kind)
    for setting in _sing_settings(n):
        _tune(tuning, n, setting)
        g = _model(mmm, n)[0]
        g.λ = lam; g.ν = nu
        mmm.update_μ(g)
        with pytest.raises(mmm.MmmError, match=r"status -5: .*Sigma is singular"):
            mmm.update_Σ(g)
        g.close()
        # the context goes on: a typical state on a new handle, same setting, every bit
        h = _model(mmm, n)[0]
        tuning()
        tl, tn = G.state(n, "typical")
        h.λ = tl; h.ν = tn
        mmm.update_μ(h); mmm.update_Σ(h)
        _twin_bits(oracle, n, (tl, tn, np.array(h.μ), np.array(h.Σ), np.array(h.invΣ), h.geometry()["grid_m"]), "after the singular Σ [%s]" % setting)
        h.close()
        RAN.add((n, kind, setting))


# ------------------------------------------------------------------------------------------ (f) the switches inside fits
def _fit(mmm, tuning, case, off):
    if case == "dense10":          # rows of counts: the M-step is an extra block of k_ctm_loglik_dense
        D, K, V, means, kw = 203, [6, 4], [40, 24], [600, 200], dict(ctm_build="dense")
    elif case == "sparse28":       # slabs: an extra block of k_ctm_loglik
        D, K, V, means, kw = 90, [10, 10, 8], [96, 38, 32], [2000, 150, 100], {}
    else:
        D, K, V, means, kw = 70, [5, 4], [40, 24], [600, 80], {}
    X, g0 = np_ref.synth_mm(D, V, K, seed=71, means=means, empty_frac=0.1)
    tuning(disable=off, **kw)
    if case == "batch3":
        g0 = [[np.random.default_rng([r, m]).integers(1, 101, size=(K[m], V[m])).astype(np.float64) for m in range(len(K))] for r in range(3)]
        g = mmm.MMCTM(K, [0.1] * len(K), V, X, γ0=g0, restarts=3)
    else:
        g = mmm.MMCTM(K, [0.1] * len(K), V, X, γ0=g0)
    tuning()
    assert g.geometry()["tdense"] == (1 if case == "dense10" else 0)
    out = []
    if case == "batch3":
        hists = mmm.fit_restarts(g, maxiter=2, tol=0.0)
        for r in range(3):
            g.select(r)
            out += [np.array(g.μ), np.array(g.Σ), np.array(g.invΣ), np.asarray(hists[r])]
        out.append(np.asarray(g.restart_elbo))
    else:
        ll = mmm.fit(g, maxiter=2, tol=0.0, verbose=False)
        out = [np.array(g.μ), np.array(g.Σ), np.array(g.invΣ), np.asarray(ll), np.array([g.elbo])]
    g.close()
    return out


@pytest.mark.parametrize("case", FIT_CASES)
def test_gauss_switches_inside_fits(mmm, tuning, case):
    base = _fit(mmm, tuning, case, ())
    assert all(np.isfinite(x).all() for x in base)
    RAN.add((case, "fit", "default"))
    for name, off in FIT_SETTINGS.items():
        if name == "default":
            continue
        res = _fit(mmm, tuning, case, off)
        for i, (a, b) in enumerate(zip(base, res)):
            _bits(a, b, "%s [%s] item %d" % (case, name, i))
        RAN.add((case, "fit", name))


def test_zz_every_case_ran(request):
    """Runs after the others (later in the file).  With the whole file selected, every (case, kind, setting) triple of the fixed list ran."""
    exp = _expected()
    assert len(exp) == N_TRIPLES
    assert RAN <= exp
    print("\n(case, kind, setting) triples run: %d of %d" % (len(RAN), N_TRIPLES))
    whole = not request.config.getoption("keyword") and not any("::" in a for a in request.config.args)
    if whole:
        assert len(RAN) == N_TRIPLES, sorted(exp - RAN, key=str)
