"""A NaN that reaches a dense log-likelihood sweep must come out of it as a NaN.  The sweeps take their log from dev_log_tab (dev_math.h), which
reads the exponent and the table index off the bits of its argument: unless NaN and +inf are sent down its special-case branch they are read as
numbers near 2^1024, and a NaN probability adds count x 710 to the numerator -- a log-likelihood that is finite and wrong, which
`n_nonfinite_ll` (counted on the host with isfinite) never sees.  The reference's log returns NaN (LDA.jl:174-188; MMCTM.jl:384-448).
Smallest shapes; every call site of the log: the three corpus forms of the LDA ll blocks and the grid-stride build, k_ctm_loglik and
k_ctm_loglik_dense."""
import numpy as np
import pytest

import np_ref
from test_lda_startup_gpu import FORMS

pytestmark = pytest.mark.gpu

# corpus form (test_lda_startup_gpu.FORMS) and tuning beyond it; the last one leaves the single-step pass for the grid-stride kernels
LDA_BUILDS = [(form, {}) for form in FORMS] + [("csr", dict(grid_blocks=2, waves_per_block=1))]


@pytest.mark.parametrize("form,tune", LDA_BUILDS, ids=[f + ("-gridstride" if t else "") for f, t in LDA_BUILDS])
def test_lda_nan_topic_entry_makes_every_later_ll_nan(mmm, tuning, form, tune):
    D, V, K = 37, 50, 7
    X, lam0 = np_ref.synth_lda(D, V, K, seed=900 + D + V, mean_n=300)
    tuning(disable=FORMS[form], **tune)
    g = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lam0)
    assert g.geometry()["single_step"] == (0 if tune else 1), g.geometry()
    ll = np.asarray(mmm.fit(g, maxiter=3, tol=0.0, verbose=False))
    assert len(ll) == 3 and np.isfinite(ll).all() and g.events()["n_nonfinite_ll"] == 0
    E = g.Elnβ.copy(); E[5, 3] = np.nan
    g.Elnβ = E
    ll = np.asarray(mmm.fit(g, maxiter=3, tol=0.0, verbose=False))
    print("\n%s %s: ll after the NaN %s" % (form, tune, ll))
    assert len(ll) == 3 and np.isnan(ll).all(), ll
    assert g.events()["n_nonfinite_ll"] == 3, g.events()
    g.close()


def _ctm_shape(case):
    if case == "mm":
        return 70, [5, 4], [40, 24], [600, 80]
    return 60, [10, 10, 8], [96, 38, 32], [2000, 150, 100]         # cfg4_shape


@pytest.mark.parametrize("build", ["dense", "sparse"])
@pytest.mark.parametrize("case", ["mm", "cfg4_shape"])
def test_ctm_nan_lambda_reaches_the_loglikelihoods(mmm, tuning, case, build):
    """update_props! / calculate_loglikelihoods after a NaN in one document's λ, through k_ctm_loglik_dense (rows of counts) and through
    k_ctm_loglik.  props is a softmax per modality (MMCTM.jl:145-154), so λ[1] = NaN makes the props of the document's FIRST modality NaN: that
    modality's ll is NaN and the other modalities keep, bit for bit, the values of the handle without the NaN.  With a NaN in every modality's
    block of λ every modality's ll is NaN (the document has words in every modality)."""
    D, K, V, means = _ctm_shape(case)
    M = len(K)
    X, g0 = np_ref.synth_mm(D, V, K, seed=3, means=means, empty_frac=0.0)
    bad = 7
    assert all(len(X[bad][m]) > 0 for m in range(M))
    tuning(ctm_build=build)
    g, clean = (mmm.MMCTM(K, [0.1] * M, V, X, γ0=g0) for _ in range(2))
    assert g.geometry()["tdense"] == (1 if build == "dense" else 0) and g.geometry()["wide"] == 0, g.geometry()
    for h in (g, clean):
        mmm._lib.check(mmm.lib().mmm_ctm_iterate(h._h, 2, 1), h.ctx.h, "iterate")
    mmm.update_props(clean)
    want = mmm.calculate_loglikelihoods(clean)
    assert np.isfinite(want).all()
    lam = g.λ[bad].copy(); lam[1] = np.nan
    g.λ[bad] = lam
    mmm.update_props(g)
    ll = mmm.calculate_loglikelihoods(g)
    print("\n%s %s: ll %s, with λ[%d][1] = NaN %s" % (case, build, want, bad, ll))
    assert np.isnan(g._get("props")).sum() == K[0]
    assert np.isnan(ll[0]), ll
    assert np.array_equal(ll[1:], want[1:]), (ll, want)
    off = np.concatenate([[0], np.cumsum(K)])[:-1]
    lam[off + 1] = np.nan
    g.λ[bad] = lam
    mmm.update_props(g)
    ll = mmm.calculate_loglikelihoods(g)
    print("with a NaN in every modality's block: %s" % ll)
    assert np.isnan(g._get("props")).sum() == sum(K)
    assert np.isnan(ll).all(), ll
    for h in (g, clean):
        h.close()
