"""mmm_refit_exposures on the device against its float64 restatement (tests/refit_ref.py): w, active, order, iters and unexplained bit for
bit / integer for integer (only +, x, / and max decide them; tests/test_refit_cpu.py asserts that no decision of these corpora is near a
tie), ll_doc and cost against a longdouble evaluation on the same q within (V + 2) 2^-52 Σ n_v |log q_v| (cost: twice that); the
invariances the definition promises; every error; the Python layer against its compositions done by hand."""
import ctypes

import numpy as np
import pytest

import np_ref
import refit_ref as R

pytestmark = pytest.mark.gpu

BITWISE = ("w", "active", "order", "iters", "unexplained")
ALL = BITWISE + ("cost", "ll_doc")


def _run(mmm, c, tol, **kw):
    kw.setdefault("penalty", c.penalty)
    kw.setdefault("allowed", c.allowed)
    return mmm.refit._raw(mmm.default_context(), c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, maxiter=c.maxiter, tol=tol, **kw)


def _dense(c, d):
    n = np.zeros(c.V)
    np.add.at(n, c.term[c.doc_ptr[d]:c.doc_ptr[d + 1]], c.count[c.doc_ptr[d]:c.doc_ptr[d + 1]].astype(np.float64))
    return n


def _same(a, b, keys=ALL, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _against_reference(c, tol, got):
    ref = R.reference(c, tol)
    want = dict(w=ref.w, active=ref.active, order=ref.order, iters=ref.iters, unexplained=ref.unexplained)
    for k in BITWISE:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.flatnonzero((got[k].reshape(c.D, -1).view(np.uint8) != want[k].reshape(c.D, -1).view(np.uint8)).any(axis=1))
        assert bad.size == 0, "%s tol %g: %s differs in documents %s" % (c.name, tol, k, bad.tolist())
    worst = 0.0
    for d in range(c.D):
        n = _dense(c, d)
        ll, bound = R.ll_longdouble(n, ref.q[d])
        err = abs(float(np.longdouble(got["ll_doc"][d]) - ll))
        worst = max(worst, err / bound if bound else (0.0 if err == 0 else np.inf))
        assert err <= bound, "%s tol %g document %d: ll %r, longdouble %r, bound %g" % (c.name, tol, d, got["ll_doc"][d], ll, bound)
        nrem = int((ref.order[d] >= 0).sum())
        for j in range(nrem):
            (la, ba), (lb, bb) = R.ll_longdouble(n, ref.rounds[d][j][0]), R.ll_longdouble(n, ref.rounds[d][j][1])
            err = abs(float(np.longdouble(got["cost"][d, j]) - (la - lb)))
            assert err <= 2 * max(ba, bb), "%s tol %g document %d round %d: cost %r, longdouble %r" % (c.name, tol, d, j, got["cost"][d, j], la - lb)
        assert (got["cost"][d, nrem:] == 0).all()
    print("%s tol %g: largest ll error / bound = %.3f" % (c.name, tol, worst))


@pytest.mark.parametrize("i", range(len(R.SHAPES) * 2 + 1), ids=lambda i: "%s-tol%g" % (R.cases()[i][0].name, R.cases()[i][1]))
def test_outputs_equal_the_restatement(mmm, i):
    c, tol = R.cases()[i]
    got = _run(mmm, c, tol)
    _against_reference(c, tol, got)
    if c.name == "twin":          # rows 4 and 5 are equal: in the round that meets them as the two smallest weights the tie is exact and 4 goes: wherever both are removed, 4 is removed first
        both = 0
        for d in range(c.D):
            o = got["order"][d].tolist()
            if 4 in o and 5 in o:
                both += 1
                assert o.index(4) < o.index(5), (d, o)
        assert both >= 3


def test_many_documents_through_the_work_counter(mmm):
    """100,003 documents (a stacked bootstrap reaches that size): the corpus' distinct documents, repeated, each equal to the restatement's"""
    c = R.corpus(2, 5)
    big = R.take(c, [i % c.D for i in range(100003)])
    got = _run(mmm, big._replace(maxiter=8), 0.0)
    ref = R.refit(c.D, c.C, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, c.penalty, 8, 0.0)
    idx = np.arange(100003) % c.D
    for k, want in (("w", ref.w), ("active", ref.active), ("order", ref.order), ("iters", ref.iters), ("unexplained", ref.unexplained)):
        assert np.array_equal(got[k].view(np.uint8), want[idx].view(np.uint8)), k


def test_two_runs_and_a_document_alone_give_equal_bits(mmm):
    c = R.corpus(12, 96)
    c40 = R.take(c, [i % c.D for i in range(40)])
    a, b = _run(mmm, c40, 1e-9), _run(mmm, c40, 1e-9)
    _same(a, b, what="two runs")
    for d in range(c.D):
        one = _run(mmm, R.take(c40, [d + c.D]), 1e-9)                      # the same document, alone (D = 1)
        for k in ALL:
            assert np.array_equal(one[k][:1].view(np.uint8), a[k][d + c.D:d + c.D + 1].view(np.uint8)), (d, k)


@pytest.mark.parametrize("C,V", [(12, 96), (65, 96), (12, 130)])
def test_catalogue_in_lds_and_through_l2_give_equal_bits(mmm, C, V):
    c = R.corpus(C, V)
    a, b = _run(mmm, c, 1e-9), _run(mmm, c, 1e-9, catalogue_in_lds=False)
    _same(a, b, what="LDS against L2")
    assert mmm.default_context().get_tuning().disable == 0                # the hook is undone


def test_a_plain_refit_on_the_chosen_set_reproduces_the_weights(mmm):
    c = R.corpus(65, 96)
    a = _run(mmm, c, 1e-9)
    b = _run(mmm, c, 1e-9, penalty=None, allowed=a["active"])
    _same(a, b, keys=("w", "active", "ll_doc", "unexplained"), what="penalty=None on the chosen set")
    assert (b["order"] == -1).all() and (b["cost"] == 0).all()
    only_w = _run(mmm, c, 1e-9, penalty=None, allowed=a["active"], outputs="w")
    assert list(only_w) == ["w"] and np.array_equal(only_w["w"].view(np.uint8), a["w"].view(np.uint8))


def test_every_error(mmm):
    c = R.take(R.corpus(12, 96), [0, 1])
    L, ctx = mmm.lib(), mmm.default_context()
    D, C, V = c.D, c.C, c.V

    def rc_of(D=D, C=C, V=V, dp=c.doc_ptr, term=c.term, count=c.count, cat=c.cat, penalty=c.penalty, maxiter=5, tol=0.0, w=True):
        out = np.zeros((max(D, 1), C))
        p = None if penalty is None else np.ascontiguousarray(penalty, dtype=np.float64)
        rc = L.mmm_refit_exposures(ctx.h, D, C, V, np.ascontiguousarray(dp, dtype=np.int64), term.ctypes.data, count.ctypes.data,
                                   np.ascontiguousarray(cat, dtype=np.float64).ravel(), None, None if p is None else p.ctypes.data, maxiter, tol,
                                   out.ctypes.data if w else None, None, None, None, None, None, None)
        return rc, (L.mmm_last_error(ctx.h) or b"").decode()

    assert rc_of()[0] == 0 and rc_of(penalty=None)[0] == 0 and rc_of(D=0)[0] == 0
    assert rc_of(w=False)[0] == -1                                                         # NULL w
    assert L.mmm_refit_exposures(None, D, C, V, c.doc_ptr, None, None, c.cat.ravel(), None, None, 5, 0.0, None, None, None, None, None, None, None) == -1
    # NULL cat, doc_ptr, term, count (nnz > 0): through a prototype of plain pointers (the binding's array types refuse None)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, ctypes.c_double, vp, vp, vp, vp, vp, vp, vp)(("mmm_refit_exposures", L))
    out = np.zeros((D, C))
    ptrs = dict(dp=c.doc_ptr.ctypes.data, term=c.term.ctypes.data, count=c.count.ctypes.data, cat=c.cat.ctypes.data)
    for null in (None, "cat", "dp", "term", "count"):
        a = dict(ptrs)
        if null:
            a[null] = None
        rc = plain(ctx.h, D, C, V, a["dp"], a["term"], a["count"], a["cat"], None, None, 5, 0.0, out.ctypes.data, None, None, None, None, None, None)
        assert rc == (-1 if null else 0), null
    for bad in (-1e-3, np.nan, np.inf):
        cat = c.cat.copy(); cat[3, 7] = bad
        rc, msg = rc_of(cat=cat)
        assert rc == -1 and "catalogue entry (3, 7)" in msg, (bad, msg)
        pen = c.penalty.copy(); pen[1] = bad if bad > 0 or np.isnan(bad) else -1.0
        rc, msg = rc_of(penalty=pen)
        assert rc == -1 and "penalty[1]" in msg, (bad, msg)
    cat = c.cat.copy(); cat[5] = 0.0
    rc, msg = rc_of(cat=cat)
    assert rc == -1 and "row 5" in msg
    assert rc_of(maxiter=0)[0] == -1 and rc_of(tol=-1e-12)[0] == -1 and rc_of(C=0)[0] == -1 and rc_of(V=0)[0] == -1 and rc_of(D=-1)[0] == -1
    term = c.term.copy(); term[4] = V
    assert rc_of(term=term)[0] == -1
    term[4] = -1
    assert rc_of(term=term)[0] == -1
    count = c.count.copy(); count[2] = -1
    assert rc_of(count=count)[0] == -1
    dp = c.doc_ptr.copy(); dp[0] = 1
    assert rc_of(dp=dp)[0] == -1
    dp = c.doc_ptr.copy(); dp[1] = dp[2] + 1
    assert rc_of(dp=dp)[0] == -1
    rc, msg = rc_of(C=257, cat=np.ones((257, V)))
    assert rc == -4 and "257" in msg and "256" in msg, msg
    with pytest.raises(ValueError, match="256"):
        mmm.refit_exposures([np.asarray([[1, 3]])], np.ones((257, 4)))
    # D = 0 writes nothing
    w = np.full((1, C), 7.0)
    assert L.mmm_refit_exposures(ctx.h, 0, C, V, np.zeros(1, np.int64), None, None, c.cat.ravel(), None, None, 5, 0.0, w.ctypes.data, None, None, None, None, None,
                                 None) == 0 and (w == 7.0).all()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def _as_X(c):
    return [np.stack([c.term[a:b].astype(np.int64) + 1, c.count[a:b].astype(np.int64)], axis=1) for a, b in zip(c.doc_ptr[:-1], c.doc_ptr[1:])]


def test_python_penalties_allowed_forms_and_names(mmm):
    c = R.corpus(12, 96)
    X = _as_X(c)
    N = np.asarray([x[:, 1].sum() for x in X], dtype=np.float64)
    names = ["S%d" % i for i in range(c.C)]
    r = mmm.refit_exposures(X, (names, ["t%d" % v for v in range(c.V)], c.cat), maxiter=60)
    raw = mmm.refit._raw(mmm.default_context(), c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, None, 0.5 * np.log(np.maximum(N, 1.0)), 60, 1e-9)
    assert r.names == names and r.intervals is None
    assert np.array_equal(r.exposures, raw["w"].T) and np.array_equal(r.active, raw["active"].T != 0) and np.array_equal(r.order, raw["order"])
    assert np.array_equal(r.cost, raw["cost"]) and np.array_equal(r.ll_doc, raw["ll_doc"]) and np.array_equal(r.iters, raw["iters"])
    assert np.array_equal(r.counts, r.exposures * N[None, :]) and np.array_equal(r.unexplained, raw["unexplained"])
    assert (r.exposures[~r.active] == 0).all() and np.allclose(r.exposures.sum(0)[N > 0], 1.0, atol=1e-12)
    # names through `allowed`, a shared mask, a D x C mask
    some = ["S1", "S4", "S7", "S11"]
    mask = np.isin(np.arange(c.C), [1, 4, 7, 11])
    a = mmm.refit_exposures(X, (names, None, c.cat), allowed=some, penalty=2.0, maxiter=60)
    b = mmm.refit_exposures(X, c.cat, allowed=mask, penalty=2.0, maxiter=60)
    d = mmm.refit_exposures(X, c.cat, allowed=np.tile(mask, (c.D, 1)), penalty=2.0, maxiter=60)
    assert np.array_equal(a.exposures, b.exposures) and np.array_equal(a.exposures, d.exposures) and not a.active[~mask].any() and a.active.any()
    plain = mmm.refit_exposures(X, c.cat, penalty=None, maxiter=60)
    assert (plain.order == -1).all() and plain.active[:, N > 0].all()
    with pytest.raises(ValueError):
        mmm.refit_exposures(X, c.cat, allowed=some)                      # names without a named catalogue
    with pytest.raises(ValueError):
        mmm.refit_exposures(X, (names, None, c.cat), allowed=["S1", "nope"])
    with pytest.raises(ValueError):
        mmm.refit_exposures(X, c.cat[:, :50])                             # X holds terms the catalogue lacks


def test_python_mmctm_nesting_and_models_as_catalogue(mmm):
    c = R.corpus(12, 96)
    X = _as_X(c)
    other = [np.asarray([[1, 2], [3, 1]], dtype=np.int64) for _ in X]
    nested = [[o, x] for o, x in zip(other, X)]
    a = mmm.refit_exposures(nested, c.cat, modality=1, maxiter=40)
    b = mmm.refit_exposures(X, c.cat, maxiter=40)
    for f in ("exposures", "active", "order", "cost", "ll_doc", "unexplained", "iters"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    with pytest.raises(ValueError):
        mmm.refit_exposures(nested, c.cat)
    # a fitted LDA as catalogue: the columns of its β
    Xl, lam0 = np_ref.synth_lda(24, 96, 5, seed=3, mean_n=600)
    g = mmm.LDA(5, 0.1, 0.1, 96, Xl, λ0=lam0)
    try:
        mmm.fit(g, maxiter=15, tol=0.0, verbose=False)
        m = mmm.refit_exposures(Xl, g, maxiter=50)
        h = mmm.refit_exposures(Xl, np.ascontiguousarray(g.β.T), maxiter=50)
        assert m.exposures.shape == (5, 24) and np.array_equal(m.exposures, h.exposures) and np.array_equal(m.order, h.order)
    finally:
        g.close()
    feats = np.stack([np.arange(96) // 16 + 1, np.arange(96) % 16 + 1], axis=1)
    il = mmm.ILDA(4, 0.1, [0.1, 0.1], feats, Xl, seed=1)
    try:
        with pytest.raises(TypeError):
            mmm.refit_exposures(Xl, il)                                   # factorised tables: no V x K signatures
    finally:
        il.close()


def test_python_bootstrap_equals_the_composition_by_hand(mmm):
    c = R.take(R.corpus(12, 96), range(9))
    X = _as_X(c)
    seed, B, q = 0x51ed270b00000003, 8, (0.1, 0.5, 0.9)
    r = mmm.refit_exposures(X, c.cat, maxiter=60, bootstrap=B, seed=seed, q=q)
    reps = mmm.resample_counts(X, B, seed)
    w = np.stack([mmm.refit_exposures(Xb, c.cat, penalty=None, allowed=r.active.T, maxiter=60).exposures.T for Xb in reps])        # [B, D, C]
    mean, sd, quant = mmm.replicate_summary(w, q)
    iv = r.intervals
    assert iv.B == B and iv.q == q and iv.mean.shape == (c.C, c.D) and iv.quantiles.shape == (3, c.C, c.D)
    assert np.array_equal(iv.mean, mean.T) and np.array_equal(iv.sd, sd.T) and np.array_equal(iv.quantiles, quant.transpose(0, 2, 1))
    assert (iv.mean[~r.active] == 0).all() and (iv.sd[r.active].max() > 0)
    with pytest.raises(ValueError):
        mmm.refit_exposures(X, c.cat, bootstrap=4)                        # no seed
