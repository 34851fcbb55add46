"""mmm_simulate_counts / mmm_fit_check on the device against their numpy restatement (tests/simulate_ref.py): the draws integer for integer
and both statistics, observed and per replicate, bit for bit (only +, -, x, /, sqrt and comparisons decide them); the invariances the
definition promises; every error with the outputs untouched; the limits of V; the Python layer against its compositions done by hand."""
import functools

import numpy as np
import pytest

import np_ref
import simulate_ref as S
from simulate_ref import DRAW_SEED, PLANTED_B, PLANTED_SEED

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
# (V, K, B, b0, stream): V around the 64-lane step and a long row, K = 1 / few / many, B against the 4 waves of a block
CASES = [(1, 1, 1, 0, 0), (5, 3, 4, 7, 1), (64, 10, 5, 0, 0), (65, 1, 9, 7, 3), (96, 3, 9, 0, 0), (130, 10, 5, 7, 0xFFFFFFFF), (1536, 3, 4, 0, 2), (96, 10, 1, 7, 0)]


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _n_doc(dp, count):
    return np.asarray([int(count[dp[d]:dp[d + 1]].sum()) for d in range(len(dp) - 1)], dtype=np.int32)


def _sim(mmm, props, phi, n_doc, B, b0=0, seed=SEED, stream=0, fill=0):
    D, K = props.shape
    V = phi.shape[1]
    out = np.full((B, D, V), fill, dtype=np.int32)
    rc = mmm.lib().mmm_simulate_counts(mmm.default_context().h, D, K, V, _ptr(props), _ptr(phi), _ptr(n_doc), B, b0, seed, stream, _ptr(out))
    return rc, out


def _fit(mmm, dp, term, count, props, phi, B, b0=0, seed=SEED, stream=0, fill=-7.0, rep=True):
    D, K = props.shape
    V = phi.shape[1]
    r = dict(cos_obs=np.full(D, fill), chi_obs=np.full(D, fill), cos_le=np.full(D, int(fill), np.int32), chi_ge=np.full(D, int(fill), np.int32),
             cos_rep=np.full((max(B, 0), D), fill) if rep else None, chi_rep=np.full((max(B, 0), D), fill) if rep else None)
    rc = mmm.lib().mmm_fit_check(mmm.default_context().h, D, K, V, dp.ctypes.data, _ptr(term), _ptr(count), _ptr(props), _ptr(phi), B, b0, seed, stream,
                                 _ptr(r["cos_obs"]), _ptr(r["chi_obs"]), _ptr(r["cos_le"]), _ptr(r["chi_ge"]), _ptr(r["cos_rep"]), _ptr(r["chi_rep"]))
    return rc, r


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


KEYS = ("cos_obs", "chi_obs", "cos_le", "chi_ge", "cos_rep", "chi_rep")


def _same(a, b, what=""):
    for k in KEYS:
        assert _bits(a[k], b[k]), (what, k, a[k], b[k])


@functools.lru_cache(maxsize=None)
def _case(i):
    V, K, B, b0, stream = CASES[i]
    dp, term, count, props, phi, zero = S.edge_corpus(V, K)
    n_doc = _n_doc(dp, count)
    want_counts = S.simulate(props, phi, n_doc, B, b0=b0, seed=SEED, stream=stream)
    want = S.fit_check(dp, term, count, props, phi, B, b0=b0, seed=SEED, stream=stream)
    return dp, term, count, props, phi, zero, n_doc, want_counts, want


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "V%d-K%d-B%d-b%d" % CASES[i][:4])
def test_draws_and_statistics_equal_the_restatement(mmm, i):
    V, K, B, b0, stream = CASES[i]
    dp, term, count, props, phi, zero, n_doc, want_counts, want = _case(i)
    assert sorted(set(n_doc.tolist()) - {int(n_doc[0])}) == [0, 1, 3, 4, 5, 255, 256, 257] and 5000 <= n_doc[0] <= 5006
    rc, out = _sim(mmm, props, phi, n_doc, B, b0, stream=stream, fill=-1)
    assert rc == 0
    assert np.array_equal(out, want_counts), np.argwhere(out != want_counts)[:5]
    assert np.array_equal(out.sum(axis=2), np.tile(n_doc, (B, 1))) and not out[:, :, zero].any()
    rc, got = _fit(mmm, dp, term, count, props, phi, B, b0, stream=stream)
    assert rc == 0
    _same(got, want, CASES[i])
    # the fused replicates are the statistics of what mmm_simulate_counts gives for the same arguments
    for d in range(len(n_doc)):
        c, x = S.statistics(out[:, d, :], S.thresholds(S.mixture(props[d], phi))[0], n_doc[d]) if n_doc[d] else (np.zeros(B), np.zeros(B))
        assert _bits(got["cos_rep"][:, d], c) and _bits(got["chi_rep"][:, d], x), d
    assert got["cos_le"][1] == B and got["chi_ge"][1] == B and got["cos_obs"][1] == 0 and got["chi_obs"][1] == 0          # the empty document
    if zero.any():            # document 3 holds a mutation its mixture cannot produce
        assert np.isposinf(got["chi_obs"][3]) and got["chi_ge"][3] == 0 and np.isfinite(got["chi_rep"][:, 3]).all()


def test_two_runs_slices_and_neighbours(mmm):
    dp, term, count, props, phi, zero, n_doc, _, _ = _case(4)
    B = 9
    rc, a = _fit(mmm, dp, term, count, props, phi, B)
    rc2, b = _fit(mmm, dp, term, count, props, phi, B)
    assert rc == 0 and rc2 == 0
    _same(a, b, "two runs")
    _, s1 = _sim(mmm, props, phi, n_doc, B)
    _, s2 = _sim(mmm, props, phi, n_doc, B)
    assert np.array_equal(s1, s2)
    # (b0, B) slices of the larger call; the counts of the chunks add
    le = np.zeros_like(a["cos_le"]); ge = np.zeros_like(a["chi_ge"])
    for b0, nb in ((0, 4), (4, 5)):
        rc, part = _fit(mmm, dp, term, count, props, phi, nb, b0)
        assert rc == 0 and _bits(part["cos_rep"], a["cos_rep"][b0:b0 + nb]) and _bits(part["chi_rep"], a["chi_rep"][b0:b0 + nb])
        assert _bits(part["cos_obs"], a["cos_obs"]) and _bits(part["chi_obs"], a["chi_obs"])
        le += part["cos_le"]; ge += part["chi_ge"]
        rc, sp = _sim(mmm, props, phi, n_doc, nb, b0)
        assert rc == 0 and np.array_equal(sp, s1[b0:b0 + nb])
    assert np.array_equal(le, a["cos_le"]) and np.array_equal(ge, a["chi_ge"])
    # without the replicate arrays: the same counts
    rc, c = _fit(mmm, dp, term, count, props, phi, B, rep=False)
    assert rc == 0 and all(_bits(c[k], a[k]) for k in KEYS[:4])
    # a document at the same index with other neighbours (other props, other documents, fewer of them)
    for d in (0, 3, 8):
        keep = list(range(d + 1))
        docs = [(term[dp[d]:dp[d + 1]], count[dp[d]:dp[d + 1]]) if j == d else (np.asarray([j % 96], np.int32), np.asarray([j + 1], np.int32)) for j in keep]
        dp2, term2, count2 = S.csr(docs)
        props2 = np.ascontiguousarray(np.where(np.arange(d + 1)[:, None] == d, props[:d + 1], 1.0 + props[:d + 1][::-1]))
        rc, one = _fit(mmm, dp2, term2, count2, props2, phi, B)
        assert rc == 0
        for k in KEYS:
            assert _bits(one[k][..., d], a[k][..., d]), (d, k)
        rc, so = _sim(mmm, props2, phi, _n_doc(dp2, count2), B)
        assert rc == 0 and np.array_equal(so[:, d], s1[:, d])


def test_no_replicates_and_no_documents(mmm):
    dp, term, count, props, phi, zero, n_doc, _, want = _case(4)
    rc, out = _sim(mmm, props, phi, n_doc, 0)
    assert rc == 0 and out.size == 0
    rc, got = _fit(mmm, dp, term, count, props, phi, 0)
    assert rc == 0 and _bits(got["cos_obs"], want["cos_obs"]) and _bits(got["chi_obs"], want["chi_obs"])
    assert not got["cos_le"].any() and not got["chi_ge"].any()
    L, h = mmm.lib(), mmm.default_context().h
    assert L.mmm_simulate_counts(h, 0, 3, 96, None, _ptr(phi), None, 4, 0, 1, 0, None) == 0
    dp0 = np.zeros(1, np.int64)
    assert L.mmm_fit_check(h, 0, 3, 96, dp0.ctypes.data, None, None, None, _ptr(phi), 4, 0, 1, 0, None, None, None, None, None, None) == 0


def test_every_error_leaves_the_outputs_untouched(mmm):
    dp, term, count, props, phi, zero, n_doc, _, _ = _case(4)
    ctx = mmm.default_context()
    B = 3

    def sim(rc_want, props=props, phi=phi, n_doc=n_doc, B=B, b0=0, match=None):
        out = np.full((max(B, 1), len(n_doc), phi.shape[1]), -5, np.int32)
        rc = mmm.lib().mmm_simulate_counts(ctx.h, props.shape[0], props.shape[1], phi.shape[1], _ptr(props), _ptr(phi), _ptr(n_doc), B, b0, SEED, 0, _ptr(out))
        assert rc == rc_want and (out == -5).all(), (rc, rc_want)
        if match:
            assert match in mmm.lib().mmm_last_error(ctx.h).decode(), mmm.lib().mmm_last_error(ctx.h)

    def fit(rc_want, dp=dp, term=term, count=count, props=props, phi=phi, B=B, b0=0, match=None):
        rc, r = _fit(mmm, dp, term, count, props, phi, B, b0, fill=-5.0)
        assert rc == rc_want, (rc, rc_want)
        assert all((r[k] == -5).all() for k in KEYS), "an output was written"
        if match:
            assert match in mmm.lib().mmm_last_error(ctx.h).decode(), mmm.lib().mmm_last_error(ctx.h)

    def poke(a, idx, v):
        a = a.copy(); a[idx] = v
        return a

    sim(-1, B=-1); sim(-1, b0=-1); sim(-1, b0=2 ** 31 - 3)                             # b0 + B > 2^31 - 1
    sim(-1, n_doc=poke(n_doc, 2, -1))
    for bad in (-1e-300, np.nan, np.inf):
        sim(-1, props=poke(props, (2, 1), bad)); sim(-1, phi=poke(phi, (1, 7), bad))
        fit(-1, props=poke(props, (2, 1), bad)); fit(-1, phi=poke(phi, (1, 7), bad))
    zero_props = poke(props, 4, 0.0)                                                  # document 4 has 4 mutations and a mixture that sums to 0
    sim(-1, props=zero_props, match="document 4"); fit(-1, props=zero_props, match="document 4")
    huge = np.full_like(props, 1e200)
    sim(-1, props=huge, phi=np.full_like(phi, 1e200), match="document 0")             # S overflows
    fit(-1, props=huge, phi=np.full_like(phi, 1e200), match="document 0")
    ok_empty = poke(props, 1, 0.0)                                                    # document 1 is empty: its mixture is never used
    assert _sim(mmm, ok_empty, phi, n_doc, B)[0] == 0 and _fit(mmm, dp, term, count, ok_empty, phi, B)[0] == 0
    fit(-1, B=-1); fit(-1, b0=-1); fit(-1, b0=2 ** 31 - 3)
    fit(-1, count=poke(count, 5, -1)); fit(-1, term=poke(term, 5, 96)); fit(-1, term=poke(term, 5, -1))
    fit(-1, dp=poke(dp, 0, 1)); fit(-1, dp=poke(dp, 3, int(dp[4]) + 1))
    big = poke(poke(count, int(dp[0]), 2 ** 30), int(dp[0]) + 1, 2 ** 30)
    fit(-4, count=big, match="2^31")                                                  # N_0 >= 2^31
    # NULL pointers
    L = mmm.lib()
    out = np.full((B, len(n_doc), 96), -5, np.int32)
    assert L.mmm_simulate_counts(ctx.h, len(n_doc), 3, 96, None, _ptr(phi), _ptr(n_doc), B, 0, 1, 0, _ptr(out)) == -1
    assert L.mmm_simulate_counts(ctx.h, len(n_doc), 3, 96, _ptr(props), None, _ptr(n_doc), B, 0, 1, 0, _ptr(out)) == -1
    assert L.mmm_simulate_counts(ctx.h, len(n_doc), 3, 96, _ptr(props), _ptr(phi), None, B, 0, 1, 0, _ptr(out)) == -1
    assert L.mmm_simulate_counts(ctx.h, len(n_doc), 3, 96, _ptr(props), _ptr(phi), _ptr(n_doc), B, 0, 1, 0, None) == -1
    assert L.mmm_simulate_counts(ctx.h, len(n_doc), 0, 96, _ptr(props), _ptr(phi), _ptr(n_doc), B, 0, 1, 0, _ptr(out)) == -1
    assert (out == -5).all()
    o = np.full(len(n_doc), -5.0); c = np.full(len(n_doc), -5, np.int32)
    args = (B, 0, 1, 0)
    assert L.mmm_fit_check(ctx.h, len(n_doc), 3, 96, None, _ptr(term), _ptr(count), _ptr(props), _ptr(phi), *args, _ptr(o), _ptr(o), _ptr(c), _ptr(c), None, None) == -1
    assert L.mmm_fit_check(ctx.h, len(n_doc), 3, 96, dp.ctypes.data, _ptr(term), _ptr(count), _ptr(props), _ptr(phi), *args, None, _ptr(o), _ptr(c), _ptr(c), None, None) == -1
    assert L.mmm_fit_check(ctx.h, len(n_doc), 3, 96, dp.ctypes.data, _ptr(term), _ptr(count), _ptr(props), _ptr(phi), *args, _ptr(o), _ptr(o), _ptr(c), None, None, None) == -1
    assert L.mmm_fit_check(ctx.h, len(n_doc), 3, 96, dp.ctypes.data, None, _ptr(count), _ptr(props), _ptr(phi), *args, _ptr(o), _ptr(o), _ptr(c), _ptr(c), None, None) == -1
    assert (o == -5).all() and (c == -5).all()


def test_the_largest_row_and_the_first_refused(mmm):
    rng = np.random.default_rng(7)
    V, K = 4096, 2
    phi = rng.gamma(0.3, size=(K, V)) + 1e-6
    phi[:, [0, 1, 2047, 4095]] = 0.0
    props = rng.gamma(1.0, size=(3, K)) + 0.1
    n_doc = np.asarray([700, 0, 5], np.int32)
    rc, out = _sim(mmm, props, phi, n_doc, 5, 2)
    assert rc == 0 and np.array_equal(out, S.simulate(props, phi, n_doc, 5, b0=2, seed=SEED))
    docs = [(np.flatnonzero(out[0, d]), out[0, d][np.flatnonzero(out[0, d])]) for d in range(3)]
    dp, term, count = S.csr(docs)
    rc, got = _fit(mmm, dp, term, count, props, phi, 5, 2)
    assert rc == 0
    _same(got, S.fit_check(dp, term, count, props, phi, 5, b0=2, seed=SEED), "V = 4096")
    assert got["cos_le"][0] >= 1 and got["chi_ge"][0] >= 1            # replicate 2 of the call is the observed vector itself
    phi2 = np.concatenate([phi, np.ones((K, 1))], axis=1)
    rc, out = _sim(mmm, props, phi2, n_doc, 2, fill=-5)
    assert rc == -4 and (out == -5).all() and "4096" in mmm.lib().mmm_last_error(mmm.default_context().h).decode()
    dp0 = np.zeros(4, np.int64)
    rc, r = _fit(mmm, dp0, np.zeros(0, np.int32), np.zeros(0, np.int32), props, phi2, 2, fill=-5.0)
    assert rc == -4 and all((r[k] == -5).all() for k in KEYS)


def test_python_layer_is_its_compositions(mmm):
    dp, term, count, props, phi, bad = S.planted(PLANTED_SEED)
    X = [np.stack([term[dp[d]:dp[d + 1]] + 1, count[dp[d]:dp[d + 1]]], axis=1).astype(np.int64) for d in range(24)]
    θ, β = props.T, phi.T
    want = S.fit_check(dp, term, count, props, phi, PLANTED_B, seed=DRAW_SEED)
    fc = mmm.goodness_of_fit(X, θ, β, B=PLANTED_B, seed=DRAW_SEED, summary=True)
    assert _bits(fc.cosine, want["cos_obs"]) and _bits(fc.chi2, want["chi_obs"]) and fc.B == PLANTED_B and np.array_equal(fc.n_doc, want["n_doc"])
    assert _bits(fc.p_cosine, (1.0 + want["cos_le"]) / 200.0) and _bits(fc.p_chi2, (1.0 + want["chi_ge"]) / 200.0)
    assert _bits(fc.cosine_rep, want["cos_rep"]) and _bits(fc.chi2_rep, want["chi_rep"])
    # the planted contamination is flagged exactly as the restatement flags it: all of the contaminated half, none of the clean one
    for stat, p in (("chi2", (1.0 + want["chi_ge"]) / 200.0), ("cosine", (1.0 + want["cos_le"]) / 200.0)):
        for alpha in (0.01, 0.05):
            assert np.array_equal(fc.flagged(alpha, stat), np.flatnonzero(p <= alpha)), (stat, alpha)
    assert np.array_equal(fc.flagged(), np.flatnonzero(bad)) and np.array_equal(fc.flagged(0.01, "cosine"), np.flatnonzero(bad))
    for got_z, obs, reps in ((fc.z_chi2, want["chi_obs"], want["chi_rep"]), (fc.z_cosine, want["cos_obs"], want["cos_rep"])):
        assert np.abs(got_z - (obs - reps.mean(axis=0)) / reps.std(axis=0, ddof=1)).max() < 1e-9          # in units of the replicates' sd
    assert (fc.z_chi2[bad] > 0).all() and (fc.z_cosine[bad] < 0).all()                                      # beyond every replicate, so beyond their mean
    lean = mmm.goodness_of_fit(X, θ, β, B=PLANTED_B, seed=DRAW_SEED)
    assert lean.cosine_rep is None and lean.z_chi2 is None and _bits(lean.p_chi2, fc.p_chi2)
    with pytest.raises(ValueError):
        mmm.goodness_of_fit(X, θ, β, B=4097, summary=True)
    with pytest.raises(ValueError):
        fc.flagged(0.01, "ll")
    # simulate_counts: the array form, and its corpora through pack_lda
    N = want["n_doc"]
    sim = mmm.simulate_counts(θ, β, N, B=3, seed=5, b0=2, stream=1)
    assert sim.dtype == np.int32 and np.array_equal(sim, S.simulate(props, phi, N, 3, b0=2, seed=5, stream=1))
    corp = mmm.simulate_counts(θ, β, N, B=3, seed=5, b0=2, stream=1, as_corpus=True)
    assert len(corp) == 3
    for b in range(3):
        dpb, tb, cb = mmm.pack_lda(corp[b])
        assert (cb > 0).all()
        back = np.stack([S.dense(96, tb[dpb[d]:dpb[d + 1]], cb[dpb[d]:dpb[d + 1]]) for d in range(24)])
        assert np.array_equal(back, sim[b])
    g = mmm.LDA(5, 0.1, 0.1, 96, corp[0], seed=1)              # a simulated cohort is a corpus an LDA accepts
    try:
        mmm.fit(g, maxiter=8, tol=0.0, verbose=False)
        a = mmm.goodness_of_fit(g, B=20, seed=3)
        b = mmm.goodness_of_fit(corp[0], g.θ, g.β, B=20, seed=3)
        assert all(_bits(x, y) for x, y in zip(a[:5], b[:5]))
        assert np.array_equal(mmm.simulate_counts(g, B=2, seed=4), mmm.simulate_counts(g.θ, g.β, a.n_doc, B=2, seed=4))
    finally:
        g.close()


def test_model_forms_of_an_mmctm_and_factorised_models(mmm):
    Vm, K = [24, 12], [3, 2]
    X, _ = np_ref.synth_mm(16, Vm, K, seed=21, means=[300, 100])
    g = mmm.MMCTM(K, [0.1, 0.1], Vm, X, seed=1)
    try:
        mmm.fit(g, maxiter=5, tol=0.0, verbose=False)
        with pytest.raises(ValueError, match="modality"):
            mmm.goodness_of_fit(g, B=4)
        props = g._get("props").reshape(16, 5)
        for m, (lo, hi) in enumerate(((0, 3), (3, 5))):
            θ = props[:, lo:hi].T
            β = np.stack([np.asarray(g.ϕ[m][k], dtype=np.float64) for k in range(K[m])], axis=1)
            a = mmm.goodness_of_fit(g, B=12, seed=3, modality=m, keep_replicates=True)
            b = mmm.goodness_of_fit([x[m] for x in X], θ, β, B=12, seed=3, stream=m, keep_replicates=True)
            c = mmm.goodness_of_fit(X, θ, β, B=12, seed=3, stream=m, modality=m, keep_replicates=True)
            assert all(_bits(x, y) and _bits(x, w) for x, y, w in zip(a[:8], b[:8], c[:8]))
            assert np.array_equal(mmm.simulate_counts(g, B=2, seed=4, modality=m), mmm.simulate_counts(θ, β, a.n_doc, B=2, seed=4, stream=m))
    finally:
        g.close()
    feats = np.stack([np.arange(96) // 16 + 1, np.arange(96) % 16 + 1], axis=1)
    Xl, _ = np_ref.synth_lda(12, 96, 4, seed=3, mean_n=300)
    il = mmm.ILDA(4, 0.1, [0.1, 0.1], feats, Xl, seed=1)
    Xm, _ = np_ref.synth_mm(10, [96], [3], seed=2, means=[300])
    im = mmm.IMMCTM([3], [0.1], [feats], Xm, seed=1)
    try:
        for model in (il, im):
            with pytest.raises(TypeError):
                mmm.goodness_of_fit(model, B=4)
            with pytest.raises(TypeError):
                mmm.simulate_counts(model, B=1)
    finally:
        il.close(); im.close()
