"""LDA restart batches (mmm_lda_create_batch / mmm_lda_fit_batch; Python LDA(..., restarts=R), fit_restarts, fit_lda_restarts): every
replica of a batch is, bit for bit, the single split-pipeline fit from its own lambda0, whatever R and its companions; config 1 against
the oracle; R = 1 is the ordinary handle; the shapes and entry points a batch refuses."""
import ctypes as C
import os

import numpy as np
import pytest

import np_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FIELDS = ("λ", "Elnβ", "β", "γ", "Elnθ", "θ")


def _lams(V, K, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 101, size=(V, K)).astype(np.float64) for _ in range(n)]


def _single(mmm, tuning, opts, K, V, X, lam, maxiter, tol):
    """The single handle a replica must equal: the same tuning plus the split pipeline (MMM_OFF_LDA_MERGED)."""
    o = dict(opts)
    o["disable"] = tuple(o.get("disable", ())) + ("lda_merged",)
    tuning(**o)
    g = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lam)
    ll = mmm.fit(g, maxiter=maxiter, tol=tol, verbose=False)
    return g, ll


def _same_replica(batch, r, hist, single, ll_single):
    batch.select(r)
    assert batch.selected == r
    assert np.array_equal(hist, ll_single), (r, hist, ll_single)
    assert batch.restart_iters[r] == len(ll_single) and bool(batch.restart_converged[r]) == single.converged
    assert batch.restart_elbo[r] == single.elbo
    for f in FIELDS:
        assert np.array_equal(getattr(batch, f), getattr(single, f)), (r, f)
    assert np.array_equal(batch.phi_flat(), single.phi_flat()), r


def _corpus(kind):
    if kind == "empty":
        X, _ = np_ref.synth_lda(240, 60, 7, seed=11, mean_n=300)
        for d in (0, 5, 6, 100, 239):
            X[d] = np.zeros((0, 2), dtype=np.int64)
        return X, 60, 7
    if kind == "k20":
        X, _ = np_ref.synth_lda(200, 60, 20, seed=12, mean_n=300)
        return X, 60, 20
    X, _ = np_ref.synth_lda(300, 96, 10, seed=10, mean_n=400)
    return X, 96, 10


# (corpus, tuning, expected build): single-step, grid-stride (CSR and 32-lane), dense-row over 16-bit and int32 rows, empty documents
BUILDS = [
    ("k10", {}, {"single_step": 1, "dense": 0}),
    ("k10", {"grid_blocks": 3}, {"single_step": 0, "dense": 0}),
    ("k10", {"lda_build": "dense"}, {"single_step": 0, "dense": 1}),
    ("k10", {"lda_build": "dense", "disable": ("lda_rows16",)}, {"single_step": 0, "dense": 1}),
    ("empty", {}, {"single_step": 1, "dense": 0}),
    ("k20", {"lda_build": "sparse", "grid_blocks": 5}, {"single_step": 0, "dense": 0, "L": 32}),
]


@pytest.mark.parametrize("kind,opts,build", BUILDS, ids=["single_step", "grid_stride", "dense16", "dense32", "empty_docs", "grid_stride_L32"])
def test_batch_replicas_bitwise_equal_single_fits(mmm, tuning, kind, opts, build):
    X, V, K = _corpus(kind)
    lams = _lams(V, K, 4, seed=sum(map(ord, kind)))
    tuning(**opts)
    batch = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lams, restarts=4)
    geo = batch.geometry()
    for key, val in build.items():
        assert geo[key] == val, (key, geo)
    if "disable" in opts:
        assert geo["row_bytes"] == 4 * 16 * geo["SL"]           # int32 rows
    elif build["dense"]:
        assert geo["row_bytes"] < 4 * 16 * geo["SL"]            # 16-bit rows
    hists = mmm.fit_restarts(batch, maxiter=40, tol=2e-3)
    assert len(hists) == 4
    for r in range(4):
        g, ll = _single(mmm, tuning, opts, K, V, X, lams[r], 40, 2e-3)
        assert g.geometry()["grid_e"] == geo["grid_e"] and g.geometry()["single_step"] == geo["single_step"]
        _same_replica(batch, r, hists[r], g, ll)
        assert mmm.calculate_elbo(batch) == g.elbo             # mmm_lda_elbo on the selected replica
        g.close()
    batch.close()


@pytest.mark.parametrize("D,cus", [(300, 0), (190, 4), (200, 4)])
def test_replica_bits_do_not_depend_on_R_or_companions(mmm, tuning, D, cus):
    """The same lambda0 as replica 0 of an R = 2 batch and replica 5 of an R = 7 batch: identical bits.  D = 190 / 200 with the geometry
    of a 4-CU device sit on either side of the single-step / grid-stride boundary (192 documents), which D x R would cross."""
    X, _ = np_ref.synth_lda(D, 96, 10, seed=20 + D, mean_n=300)
    lams = _lams(96, 10, 8, seed=D)
    tuning(geometry_cus=cus)
    b2 = mmm.LDA(10, 0.1, 0.1, 96, X, λ0=[lams[0], lams[1]], restarts=2)
    b7 = mmm.LDA(10, 0.1, 0.1, 96, X, λ0=[lams[2], lams[3], lams[4], lams[5], lams[6], lams[0], lams[7]], restarts=7)
    if cus:
        assert b2.geometry()["single_step"] == (1 if D <= 192 else 0)
    assert b2.geometry() == b7.geometry()
    h2 = mmm.fit_restarts(b2, maxiter=30, tol=2e-3)
    h7 = mmm.fit_restarts(b7, maxiter=30, tol=2e-3)
    assert np.array_equal(h2[0], h7[5])
    assert b2.restart_elbo[0] == b7.restart_elbo[5] and b2.restart_converged[0] == b7.restart_converged[5]
    b2.select(0); b7.select(5)
    for f in FIELDS:
        assert np.array_equal(getattr(b2, f), getattr(b7, f)), f
    assert np.array_equal(b2.phi_flat(), b7.phi_flat())
    b2.close(); b7.close()


def test_config1_batch_against_oracle(mmm, oracle):
    """BASELINE config 1 shape (BRCA SNV, K = 7), R = 8 restarts to convergence: every replica against the oracle from its lambda0
    (the bounds of test_brca_gpu.py)."""
    terms, samples, snv = mmm.read_counts_tsv(os.path.join(GOLD, "brca-eu_snv_counts.tsv"))
    X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
    lams = _lams(96, 7, 8, seed=3)
    batch = mmm.LDA(7, 0.1, 0.1, X, λ0=lams, restarts=8)
    hists = mmm.fit_restarts(batch, maxiter=1000, tol=1e-4)
    for r in range(8):
        o = oracle.LdaOracle(7, 0.1, 0.1, X, V=96, lambda0=lams[r])
        llo = o.fit(maxiter=1000, tol=1e-4)
        assert len(hists[r]) == len(llo) and bool(batch.restart_converged[r]) == o.converged, r
        np.testing.assert_allclose(hists[r], llo, rtol=1e-9)
        assert batch.restart_elbo[r] == pytest.approx(o.elbo_value, rel=1e-5)
    batch.close()


def test_R1_batch_is_the_ordinary_handle(mmm):
    """create_batch with R = 1 is mmm_lda_create under the default tuning, merged launch (and its moved prologue) included."""
    X, lam = np_ref.synth_lda(300, 96, 10, seed=30, mean_n=400)
    b = mmm.LDA(10, 0.1, 0.1, 96, X, λ0=[lam], restarts=1)
    g = mmm.LDA(10, 0.1, 0.1, 96, X, λ0=lam)
    assert lib_replicas(mmm, b) == 1
    h = mmm.fit_restarts(b, maxiter=40, tol=2e-3)
    ll = mmm.fit(g, maxiter=40, tol=2e-3, verbose=False)
    assert b.geometry() == g.geometry() and b.geometry()["prologue_moved"] == 1
    _same_replica(b, 0, h[0], g, ll)


def lib_replicas(mmm, model):
    return int(mmm.lib().mmm_lda_replicas(model._h))


def _status(exc):
    return str(exc.value)


def test_refused_shapes_and_calls(mmm, tuning):
    X, _ = np_ref.synth_lda(120, 96, 10, seed=40, mean_n=300)
    with pytest.raises(mmm.MmmError) as e:                        # K >= 25: the wide path under MMM_BUILD_AUTO
        mmm.LDA(40, 0.1, 0.1, 96, X, restarts=2, seed=1)
    assert "status -4" in _status(e) and "wide path" in _status(e)
    tuning(lda_build="wide")
    with pytest.raises(mmm.MmmError) as e:
        mmm.LDA(10, 0.1, 0.1, 96, X, restarts=2, seed=1)
    assert "status -4" in _status(e) and "MMM_BUILD_WIDE" in _status(e)
    tuning()
    with pytest.raises(mmm.MmmError) as e:                        # R < 1
        mmm.LDA(10, 0.1, 0.1, 96, X, restarts=0)
    assert "status -1" in _status(e)
    with pytest.raises(ValueError):
        mmm.LDA(10, 0.1, 0.1, 96, X, λ0=_lams(96, 10, 2, 1), restarts=3)
    feats = np.stack([np.arange(96) % 6 + 1, np.arange(96) // 6 + 1], axis=1)
    il = mmm.ILDA(10, 0.1, 0.1, feats, X, seed=2)
    with pytest.raises(mmm.MmmError) as e:                        # no ILDA batches
        mmm.fit_restarts(il, maxiter=5)
    assert "status -4" in _status(e) and "ILDA" in _status(e)
    il.close()

    lams = _lams(96, 10, 3, seed=41)
    b = mmm.LDA(10, 0.1, 0.1, 96, X, λ0=lams, restarts=3)
    L, h = mmm.lib(), b._h
    ni, cv = C.c_int(), C.c_int()
    one = np.zeros(96 * 10)
    calls = [("update_gamma", lambda: L.mmm_lda_update_gamma(h)), ("update_lambda", lambda: L.mmm_lda_update_lambda(h)),
             ("set", lambda: L.mmm_lda_set(h, 0, one, one.size)), ("iterate", lambda: L.mmm_lda_iterate(h, 3)),
             ("fit", lambda: L.mmm_lda_fit(h, 5, 1e-4, None, C.byref(ni), C.byref(cv), None)),
             ("infer", lambda: L.mmm_lda_infer(h, 0, 5, 1e-4, None, C.byref(ni), C.byref(cv)))]
    for name, call in calls:
        assert call() == -4, name
        assert b"fit_batch" in L.mmm_last_error(b.ctx.h), name
    with pytest.raises(ValueError, match="fit_restarts"):
        mmm.fit(b, maxiter=5)
    assert L.mmm_lda_select(h, 3) == -1
    # the refused calls left the handle as it was: it fits exactly like a fresh batch from the same inits
    hb = mmm.fit_restarts(b, maxiter=30, tol=2e-3)
    fresh = mmm.LDA(10, 0.1, 0.1, 96, X, λ0=lams, restarts=3)
    hf = mmm.fit_restarts(fresh, maxiter=30, tol=2e-3)
    for r in range(3):
        assert np.array_equal(hb[r], hf[r])
        b.select(r); fresh.select(r)
        assert np.array_equal(b.λ, fresh.λ) and np.array_equal(b.γ, fresh.γ)
    b.close(); fresh.close()


def test_python_surface(mmm, tuning):
    X, _ = np_ref.synth_lda(150, 96, 8, seed=50, mean_n=300)
    b = mmm.LDA(8, 0.1, 0.1, 96, X, restarts=3, seed=17)
    assert b.R == 3 and b.selected == 0
    for r in range(3):                                              # replica r is drawn as LDA(..., seed=seed + r)
        g = mmm.LDA(8, 0.1, 0.1, 96, X, seed=17 + r)
        b.select(r)
        # (β is not formed before the first update_β!, LDA.jl:36-49: not compared here)
        assert np.array_equal(b.λ, g.λ) and np.array_equal(b.Elnβ, g.Elnβ) and np.array_equal(b.γ, g.γ) and np.array_equal(b.Elnθ, g.Elnθ)
        assert np.array_equal(b.phi_flat(), g.phi_flat())
        g.close()
    mmm.fit_restarts(b, maxiter=25, tol=2e-3)
    assert b.selected == 2 and b.ll == b.restart_ll[2] and b.elbo == b.restart_elbo[2]
    lam = [b.select(r).λ for r in range(3)]
    assert not np.array_equal(lam[0], lam[1])
    assert np.array_equal(b.select(0).λ, lam[0]) and b.selected == 0
    np.testing.assert_allclose(b.select(1).θ.sum(axis=0), 1.0, rtol=1e-12)
    b.close()

    # fit_lda_restarts: two batches (batch_size 3 over 5 seeds); the final lls are the single fits', the winner is their argmax
    seeds = [101, 5, 77, 9, 1234]
    win, lamw, gamw, all_ll = mmm.fit_lda_restarts(X, 8, 0.1, 0.1, seeds, V=96, batch_size=3, maxiter=25, tol=2e-3)
    assert all_ll.shape == (5,) and win == int(np.argmax(all_ll))
    tuning(disable=("lda_merged",))
    for i, s in enumerate(seeds):
        g = mmm.LDA(8, 0.1, 0.1, 96, X, seed=s)
        ll = mmm.fit(g, maxiter=25, tol=2e-3, verbose=False)
        assert ll[-1] == all_ll[i], i
        if i == win:
            assert np.array_equal(g.λ, lamw) and np.array_equal(g.γ, gamw)
        g.close()
