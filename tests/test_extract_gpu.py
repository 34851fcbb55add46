"""mmm_extract_signatures on the device against its float64 restatement (tests/extract_ref.py): sig, w, iters and unexplained bit for bit (only
+, x, / and comparisons decide them; tests/test_extract_cpu.py asserts that no stopping decision of these cases is near a tie), ll_doc against
a longdouble evaluation on the same q within (V + 2) 2^-52 Σ n_v |log q_v|, ll within the sum of those bounds plus the rounding of its own
D + 16 additions; the invariances the definition promises; every error; the Python layer against its compositions done by hand."""
import ctypes

import numpy as np
import pytest

import extract_ref as E
import refit_ref as R

pytestmark = pytest.mark.gpu

BITWISE = ("sig", "w", "iters", "unexplained")
CASES = {c.name: c for c in E.cases()}


def _run(mmm, c, r0=0, R_=None, waves=0, **kw):
    Rn = c.R if R_ is None else R_
    init = None if c.init is None else c.init[r0:r0 + Rn]
    return mmm.extract._raw(mmm.default_context(), c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, c.J, c.allowed, Rn, r0, c.seed, 0, init, c.maxiter, c.tol,
                            waves, **kw)


def _same(a, b, keys, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_equal_the_restatement(mmm, name):
    c = CASES[name]
    got, ref = _run(mmm, c), E.reference(c)
    for k in BITWISE:
        want = getattr(ref, k)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        bad = np.flatnonzero((got[k].reshape(c.R, -1).view(np.uint8) != want.reshape(c.R, -1).view(np.uint8)).any(axis=1))
        assert bad.size == 0, "%s: %s differs in restarts %s" % (name, k, bad.tolist()[:10])
    n = E.dense(c.D, c.V, c.doc_ptr, c.term, c.count)
    worst = 0.0
    for r in range(min(c.R, 3)):
        total = np.longdouble(0); tb = 0.0; mag = 0.0
        for d in range(c.D):
            ll, bound = R.ll_longdouble(n[d], ref.q[r, d]) if ref.w[r, d].any() else (np.longdouble(0), 0.0)
            err = abs(float(np.longdouble(got["ll_doc"][r, d]) - ll))
            worst = max(worst, err / bound if bound else (0.0 if err == 0 else np.inf))
            assert err <= bound, "%s restart %d document %d: ll %r, longdouble %r, bound %g" % (name, r, d, got["ll_doc"][r, d], ll, bound)
            total += ll; tb += bound; mag += abs(float(ll))
        # the D + 16 additions of the stripe order, one rounding each, on partial sums no larger than Σ |ll_d|
        assert abs(float(np.longdouble(got["ll"][r]) - total)) <= tb + (c.D + 16) * 2.0 ** -53 * mag, (name, r)
    print("%s: largest ll error / bound = %.3f" % (name, worst))


@pytest.mark.parametrize("name", ["F1J1V5D3", "F3J2V97D33", "F2J5V128D18", "F33J2V96D20", "F2J1V8D6760"])
def test_every_geometry_and_a_second_run_give_equal_bits(mmm, name):
    c = CASES[name]
    base = _run(mmm, c)
    _same(base, _run(mmm, c), BITWISE + ("ll", "ll_doc"), "second run")
    for waves in (1, 4, 16):
        _same(base, _run(mmm, c, waves=waves), BITWISE + ("ll", "ll_doc"), "waves %d" % waves)


@pytest.mark.parametrize("name", ["F3J1V96D17", "init"])
def test_a_call_is_a_slice_of_the_call_from_zero(mmm, name):
    c = CASES[name]
    whole, part = _run(mmm, c), _run(mmm, c, r0=2, R_=1)
    for k in BITWISE + ("ll", "ll_doc"):
        assert np.array_equal(part[k].view(np.uint8), whole[k][2:3].view(np.uint8)), k
    only = _run(mmm, c, r0=2, R_=1, outputs=())
    assert sorted(only) == ["iters", "ll", "sig"] and np.array_equal(only["sig"], part["sig"]) and np.array_equal(only["ll"], part["ll"])


@pytest.mark.parametrize("name", ["F4J0V96D21", "F33J2V96D20", "F3J2V97D33"])
def test_without_free_rows_it_is_the_refit_bit_for_bit(mmm, name):
    c = CASES[name]
    ctx = mmm.default_context()
    a = mmm.extract._raw(ctx, c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, 0, c.allowed, 1, 0, 0, 0, None, 25, 0.0)
    b = mmm.refit._raw(ctx, c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, None, 25, 0.0)
    assert a["sig"].shape == (1, 0, c.V) and a["iters"][0] == 25
    for k, kb in (("w", "w"), ("ll_doc", "ll_doc"), ("unexplained", "unexplained")):
        assert np.array_equal(a[k][0].view(np.uint8), b[kb].view(np.uint8)), k


def test_every_error(mmm):
    c = CASES["F3J2V97D33"]
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, ci, ctypes.c_uint64, ctypes.c_uint32, vp, ci, ctypes.c_double, ci, vp, vp, vp, vp, vp,
                             vp)(("mmm_extract_signatures", L))
    keep = []

    def call(h=True, D=c.D, F=c.F, J=c.J, V=c.V, dp=c.doc_ptr, term=c.term, count=c.count, cat=c.cat, allowed=c.allowed, R_=2, r0=0, init=None, maxiter=3, tol=0.0,
             waves=0, null=()):
        K = max(F + J, 1)
        out = dict(sig=np.full((max(R_, 1), max(J, 1), V), 7.0), w=np.full((max(R_, 1), max(D, 1), K), 7.0), ll=np.full(max(R_, 1), 7.0),
                   ll_doc=np.full((max(R_, 1), max(D, 1)), 7.0), unex=np.full((max(R_, 1), max(D, 1)), 7.0), iters=np.full(max(R_, 1), 7, dtype=np.int32))
        arrs = dict(dp=np.ascontiguousarray(dp, dtype=np.int64), term=term, count=count, cat=None if cat is None else np.ascontiguousarray(cat, dtype=np.float64),
                    allowed=allowed, init=None if init is None else np.ascontiguousarray(init, dtype=np.float64))
        keep.append(arrs)
        p = {k: (None if v is None or k in null else v.ctypes.data) for k, v in list(arrs.items()) + list(out.items())}
        rc = plain(ctx.h if h else None, D, F, J, V, p["dp"], p["term"], p["count"], p["cat"], p["allowed"], R_, r0, 5, 0, p["init"], maxiter, tol, waves, p["sig"],
                   p["w"], p["ll"], p["ll_doc"], p["unex"], p["iters"])
        untouched = all((v == 7).all() for v in out.values())
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    rc, _, untouched = call()
    assert rc == 0 and not untouched
    assert call(null=("w", "ll_doc", "unex"))[0] == 0 and call(allowed=None)[0] == 0
    for kw in (dict(D=0), dict(R_=0)):                                   # nothing to do: nothing written
        rc, _, untouched = call(**kw)
        assert rc == 0 and untouched, kw
    arg = [dict(h=False), dict(D=-1), dict(F=-1), dict(J=-1), dict(F=0, J=0, cat=None, allowed=None), dict(V=0), dict(R_=-1), dict(r0=-1), dict(r0=2 ** 31 - 2, R_=2),
           dict(maxiter=0), dict(tol=-1e-12), dict(tol=np.nan), dict(waves=3), dict(waves=32), dict(waves=-1), dict(null=("cat",)), dict(null=("sig",)),
           dict(null=("ll",)), dict(null=("iters",)), dict(null=("dp",)), dict(null=("term",)), dict(null=("count",))]
    for kw in arg:
        rc, msg, untouched = call(**kw)
        assert rc == -1 and untouched, (kw, rc, msg)
    for bad in (-1e-3, np.nan, np.inf):
        cat = c.cat.copy(); cat[1, 7] = bad
        rc, msg, untouched = call(cat=cat)
        assert rc == -1 and untouched and "catalogue entry (1, 7)" in msg, (bad, msg)
        init = np.ones((2, c.J, c.V)); init[1, 0, 5] = bad
        rc, msg, untouched = call(init=init)
        assert rc == -1 and untouched and "init entry (1, 0, 5)" in msg, (bad, msg)
    cat = c.cat.copy(); cat[2] = 0.0
    rc, msg, untouched = call(cat=cat)
    assert rc == -1 and untouched and "row 2" in msg
    init = np.ones((2, c.J, c.V)); init[0, 1] = 0.0
    rc, msg, untouched = call(init=init)
    assert rc == -1 and untouched and "init row (0, 1)" in msg
    term = c.term.copy(); term[4] = c.V
    assert call(term=term)[0] == -1
    count = c.count.copy(); count[2] = -1
    assert call(count=count)[0] == -1
    dp = c.doc_ptr.copy(); dp[0] = 1
    assert call(dp=dp)[0] == -1
    dp = c.doc_ptr.copy(); dp[1] = dp[2] + 1
    assert call(dp=dp)[0] == -1
    # limits, each with its figure in the message
    none = np.zeros(0, np.int32)
    rc, msg, untouched = call(F=250, J=7, V=4, D=1, dp=np.zeros(2, np.int64), term=none, count=none, cat=np.ones((250, 4)), allowed=None)
    assert rc == -4 and untouched and "257" in msg and "256" in msg, msg
    rc, msg, untouched = call(F=1, J=33, V=4, D=1, dp=np.zeros(2, np.int64), term=none, count=none, cat=np.ones((1, 4)), allowed=None)
    assert rc == -4 and untouched and "33" in msg and "32" in msg, msg
    rc, msg, untouched = call(F=200, J=1, V=200, D=1, dp=np.zeros(2, np.int64), term=none, count=none, cat=np.ones((200, 200)), allowed=None)
    assert rc == -4 and untouched and "LDS" in msg and str(160 * 1024) in msg, msg
    rc, msg, untouched = call(F=2, J=3, V=1536, D=1, dp=np.zeros(2, np.int64), term=none, count=none, cat=np.ones((2, 1536)), allowed=None, waves=16)
    assert rc == -4 and untouched and "16 waves" in msg, msg


def test_the_size_limits_of_the_document_arrays(mmm):
    """D K and D V of 2^31 and more are refused before anything is allocated (documents without entries: the CSR is a row of zeros)"""
    L, ctx = mmm.lib(), mmm.default_context()
    out = np.full(8, 7.0); it = np.full(2, 7, dtype=np.int32)
    for F, V, D in ((255, 1, 2 ** 23), (0, 8192, 2 ** 18)):
        cat, sig = np.ones((max(F, 1), V)), np.full((1, 1, V), 7.0)
        rc = L.mmm_extract_signatures(ctx.h, D, F, 1, V, np.zeros(D + 1, np.int64), None, None, cat.ctypes.data if F else None, None, 1, 0, 1, 0, None, 2, 0.0, 1,
                                      sig.ctypes.data, None, out.ctypes.data, None, None, it.ctypes.data)
        msg = (L.mmm_last_error(ctx.h) or b"").decode()
        assert rc == -4 and "2^31" in msg and (out == 7).all() and (it == 7).all() and (sig == 7).all(), (F, V, D, rc, msg)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def _as_X(c):
    return [np.stack([c.term[a:b].astype(np.int64) + 1, c.count[a:b].astype(np.int64)], axis=1) for a, b in zip(c.doc_ptr[:-1], c.doc_ptr[1:])]


def test_python_best_restart_both_exposure_routes_and_consensus(mmm, monkeypatch):
    c = CASES["F3J2V97D33"]
    X = _as_X(c)
    names = ["S%d" % i for i in range(c.F)]
    ex = mmm.extract_signatures(X, (names, None, c.cat), n_new=2, restarts=4, seed=c.seed, allowed=c.allowed, maxiter=30, tol=0.0, consensus=True)
    raw = mmm.extract._raw(mmm.default_context(), c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, 2, c.allowed, 4, 0, c.seed, 0, None, 30, 0.0)
    best = int(np.argmax(raw["ll"]))
    assert ex.best == best and ex.ll == raw["ll"][best] and np.array_equal(ex.ll_all, raw["ll"]) and np.array_equal(ex.iters, raw["iters"])
    assert np.array_equal(ex.all_signatures, raw["sig"]) and np.array_equal(ex.signatures, raw["sig"][best])
    assert np.array_equal(ex.exposures, raw["w"][best]) and np.array_equal(ex.unexplained, raw["unexplained"][best])
    assert ex.names == names + ["NEW1", "NEW2"] and ex.exposures.shape == (c.D, 5)
    assert np.array_equal(ex.stability, mmm.signature_consensus(raw["sig"], best, q=()).stability) and ex.stability.shape == (2,)
    # the second-call route: the best restart alone is a slice of the same call
    monkeypatch.setattr(mmm.extract, "W_ALL_LIMIT", 0)
    again = mmm.extract_signatures(X, (names, None, c.cat), n_new=2, restarts=4, seed=c.seed, allowed=c.allowed, maxiter=30, tol=0.0)
    assert again.best == best and again.stability is None
    assert np.array_equal(again.exposures.view(np.uint8), ex.exposures.view(np.uint8)) and np.array_equal(again.unexplained, ex.unexplained)
    # ties go to the lowest restart: two restarts from the same rows
    init = np.random.default_rng(3).uniform(0.1, 1.0, size=(1, 2, c.V))
    for limit in (0, 1 << 24):
        monkeypatch.setattr(mmm.extract, "W_ALL_LIMIT", limit)
        tie = mmm.extract_signatures(X, c.cat, n_new=2, restarts=2, init=np.concatenate([init, init]), maxiter=10, tol=0.0)
        assert tie.best == 0 and tie.ll_all[0] == tie.ll_all[1] and np.array_equal(tie.all_signatures[0], tie.all_signatures[1])
        assert tie.names == ["FIXED1", "FIXED2", "FIXED3", "NEW1", "NEW2"]
    # without a catalogue every row is new and V is the largest term of X
    free = mmm.extract_signatures(X, None, n_new=3, restarts=2, seed=1, maxiter=10, tol=0.0)
    V = int(c.term.max()) + 1
    assert free.signatures.shape == (3, V) and free.exposures.shape == (c.D, 3) and free.names == ["NEW1", "NEW2", "NEW3"]
    assert np.allclose(free.signatures.sum(axis=1), 1.0, atol=1e-12)


def test_python_catalogue_goes_into_refit_and_presence(mmm):
    c = CASES["F3J2V97D33"]
    X = _as_X(c)
    ex = mmm.extract_signatures(X, c.cat, n_new=2, restarts=2, seed=3, maxiter=30, tol=0.0)
    names, terms, table = ex.catalogue()
    assert names == ex.names and terms is None and table.shape == (5, c.V) and np.array_equal(table[:3], c.cat) and np.array_equal(table[3:], ex.signatures)
    r = mmm.refit_exposures(X, ex.catalogue(), penalty=None, maxiter=30, tol=0.0)
    assert r.names == ex.names and r.exposures.shape == (5, c.D)
    # the refit under the extended catalogue is J = 0 extraction under it: the same call, the same bits
    a = mmm.extract_signatures(X, ex.catalogue(), n_new=0, restarts=1, maxiter=30, tol=0.0)
    assert np.array_equal(a.exposures.view(np.uint8), np.ascontiguousarray(r.exposures.T).view(np.uint8)) and a.signatures.shape == (0, c.V)
    p = mmm.signature_presence(X, ex.catalogue(), ["NEW1"], B=4, seed=1, maxiter=30)
    assert p.p.shape == (1, c.D)


def test_python_argument_errors_need_no_device(mmm):
    c = CASES["F1J1V5D3"]
    X = _as_X(c)

    class NoDevice:
        @property
        def h(self):
            raise AssertionError("a device was asked for")

    bad = [dict(n_new=-1), dict(n_new=33), dict(n_new=0, catalogue=None), dict(restarts=0), dict(maxiter=0), dict(tol=-1.0), dict(tol=np.nan),
           dict(consensus=True, restarts=1), dict(consensus=True, n_new=0), dict(allowed=["S9"]), dict(allowed=np.ones(7)), dict(names=["a", "b"]),
           dict(init=np.ones((2, 1, 5))), dict(init=-np.ones((3, 1, 5))), dict(init=np.zeros((3, 1, 5))), dict(catalogue=np.ones((256, 5))),
           dict(catalogue=np.ones((1, 1))), dict(catalogue=-np.ones((1, 5)))]
    for kw in bad:
        args = dict(catalogue=c.cat, n_new=1, restarts=3, ctx=NoDevice())
        args.update(kw)
        with pytest.raises(ValueError):
            mmm.extract_signatures(X, **args)
    with pytest.raises(ValueError):
        mmm.extract_signatures([[x, x] for x in X], c.cat, ctx=NoDevice())          # the MMCTM nesting
