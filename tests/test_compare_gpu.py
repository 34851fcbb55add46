"""mmm_deal_counts and mmm_compare_exposures on the device against their numpy restatement (tests/compare_ref.py): the dealt counts in every
integer at key_bits 32, 8 and 3 (the last two put ties at the threshold in essentially every replicate); the weights, count_sig, count_max,
status, unexplained and iters bit for bit at key_bits 32 and 3, wherever the catalogue is read from; count_ge as an integer (tests/
test_compare_cpu.py asserts that no comparison of these corpora is near a tie, and says why a sample with ONE allowed signature is left out);
stat and the kept replicates against a longdouble evaluation on the same mixtures within the bound test_presence_gpu.py / test_refit_gpu.py
apply to ll-derived values ((V + 2) 2^-52 Σ n_v |log q_v| per log-likelihood, doubled with the statistic); the shipped entries the definition is
composed of; chunks, runs and geometries; every error."""
import ctypes

import numpy as np
import pytest

import compare_ref as CR

pytestmark = pytest.mark.gpu

BITWISE = ("w_a", "w_b", "w_pool", "count_sig", "count_max", "status", "unexplained", "iters", "count_ge")
ALL = BITWISE + ("stat", "rep_stat")


def _run(mmm, c, B=None, b0=0, keep=True, **kw):
    return mmm.compare._raw(mmm.default_context(), c.D, c.V, (c.ptr_a, c.term_a, c.count_a), (c.ptr_b, c.term_b, c.count_b), c.cat, c.allowed,
                            c.B if B is None else B, b0, c.seed, c.stream, c.maxiter, c.tol, keep=keep, **kw)


def _same(a, b, keys=ALL, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _within(got, ld, bound, what):
    """got against the longdouble values ld within bound, element by element; NaN must sit in the same places"""
    got, ld, bound = np.asarray(got).ravel(), np.asarray(ld).ravel(), np.asarray(bound).ravel()
    fin = np.isfinite(ld)
    assert np.array_equal(np.isnan(got), np.isnan(ld)) and np.isfinite(got[fin]).all(), what
    err = np.abs(got[fin] - ld[fin])
    bad = np.flatnonzero(err > bound[fin])
    assert bad.size == 0, "%s: %d values beyond the bound, the first %r against %r (bound %g)" % (what, bad.size, got[fin][bad[0]], ld[fin][bad[0]], bound[fin][bad[0]])
    return float((err / np.maximum(bound[fin], 1e-300)).max()) if err.size and (bound[fin] > 0).any() else 0.0


# ---- the dealing --------------------------------------------------------------------------------------------------------------------------------
def _deal_corpus():
    """rows: a few entries; one entry; none; 300 entries with N over 1024 and N_a = 257 (several steps, a partial last Philox block); N_a = N - 1;
    N_a = 0; N_a = N; one mutation; entries with zero counts throughout"""
    rng = np.random.default_rng(5)
    docs = [rng.integers(0, 9, size=w) for w in (7, 1, 0, 300, 12, 20, 20, 1, 40)]
    docs[1][:] = 6; docs[7][:] = 1
    docs[8][::2] = 0
    dp = np.concatenate([[0], np.cumsum([d.size for d in docs])]).astype(np.int64)
    N = np.array([int(d.sum()) for d in docs])
    assert N[3] > 1024 and N[3] % 4 != 0
    n_a = np.array([3, 2, 0, 257, N[4] - 1, 0, N[6], 1, 17], dtype=np.int32)
    return dp, np.concatenate(docs).astype(np.int32), n_a


@pytest.mark.parametrize("key_bits", (32, 8, 3))
def test_dealt_counts_equal_the_restatement_in_every_integer(mmm, tuning, key_bits):
    dp, count, n_a = _deal_corpus()
    ctx = mmm.default_context()
    D, B = n_a.size, 24
    want = CR.deal(dp, count, n_a, B, 0, seed=2 ** 35 + 9, stream=4, key_bits=key_bits)
    got = mmm.compare._deal_raw(ctx, D, dp, count, n_a, B, 0, 2 ** 35 + 9, 4, key_bits)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for d in range(D):
        assert (got[:, dp[d]:dp[d + 1]].sum(axis=1) == n_a[d]).all()
    part = mmm.compare._deal_raw(ctx, D, dp, count, n_a, 5, 19, 2 ** 35 + 9, 4, key_bits)
    assert np.array_equal(part, want[19:])
    tuning(geometry_cus=3)
    assert np.array_equal(mmm.compare._deal_raw(ctx, D, dp, count, n_a, B, 0, 2 ** 35 + 9, 4, key_bits), want)


def test_deal_counts_through_the_python_layer(mmm):
    """duplicate terms and shuffled entries: the mutations are numbered in term order of the dense vector"""
    X = [np.array([[5, 3], [2, 4], [5, 2], [9, 1]]), np.zeros((0, 2), dtype=np.int64), np.array([[1, 7]])]
    dense = np.array([[0, 4, 0, 0, 5, 0, 0, 0, 1], [0] * 9, [7] + [0] * 8])
    got = mmm.deal_counts(X, [4, 0, 7], 6, seed=3, stream=1, b0=2)
    assert got.shape == (6, 3, 9) and (got.sum(axis=2) == np.array([4, 0, 7])).all() and (got <= dense[None]).all() and (got >= 0).all()
    for d in (0, 2):
        want = CR.deal_doc(dense[d], [4, 0, 7][d], d, 2 + np.arange(6), 3, 1)
        assert np.array_equal(got[:, d], want)
    assert mmm.deal_counts(X, [4, 0, 7], 2, seed=3, V=12).shape == (2, 3, 12)
    assert mmm.deal_counts(X, [4, 0, 7], 0, seed=3).shape == (0, 3, 9)


# ---- the test -----------------------------------------------------------------------------------------------------------------------------------
def _against_reference(c, got, key_bits):
    ref = CR.reference(c, key_bits)
    want = dict(w_a=ref.w_a, w_b=ref.w_b, w_pool=ref.w_pool, count_sig=ref.count_sig, count_max=ref.count_max, status=ref.status, unexplained=ref.unexplained,
                iters=ref.iters)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.flatnonzero((got[k].reshape(c.D, -1).view(np.uint8) != want[k].reshape(c.D, -1).view(np.uint8)).any(axis=1))
        assert bad.size == 0, "%s: %s differs in samples %s" % (c.name, k, bad.tolist())
    cmp = ref.n_allowed > 1            # one allowed signature: T is the same for every partition up to rounding (tests/test_compare_cpu.py)
    assert got["count_ge"].dtype == np.int32 and np.array_equal(got["count_ge"][cmp], ref.count_ge[cmp]), (got["count_ge"], ref.count_ge)
    assert (got["count_ge"][ref.status == 3] == 0).all() and (got["count_ge"] >= 0).all() and (got["count_ge"] <= c.B).all()
    worst = _within(got["stat"], ref.stat_ld, ref.bound, c.name + " stat")
    worst = max(worst, _within(got["rep_stat"], ref.rep_ld, ref.rep_bound, c.name + " replicates"))
    print("%s key_bits %d: largest error / bound of stat and rep_stat = %.3f" % (c.name, key_bits, worst))


@pytest.mark.parametrize("key_bits", CR.KEY_BITS)
@pytest.mark.parametrize("i", range(len(CR.SHAPES)), ids=lambda i: CR.corpora()[i].name)
def test_outputs_equal_the_restatement_wherever_the_catalogue_is_read_from(mmm, i, key_bits):
    c = CR.corpora()[i]
    got = _run(mmm, c, key_bits=key_bits)
    _against_reference(c, got, key_bits)
    l2 = _run(mmm, c, key_bits=key_bits, catalogue_in_lds=False)
    _same(got, l2, what="LDS against L2")
    assert mmm.default_context().get_tuning().disable == 0                # the hook is undone


def _as_X(ptr, term, count):
    return [np.stack([term[a:b].astype(np.int64) + 1, count[a:b].astype(np.int64)], axis=1) for a, b in zip(ptr[:-1], ptr[1:])]


def test_the_fits_are_the_shipped_refit_and_the_replicates_the_shipped_dealing(mmm):
    """The observed weights are refit_exposures(penalty=None) of the two tables and of the pooled one, bit for bit.  Every kept replicate
    against the composition of the public entries: deal_counts on the pooled table under the same seed and stream, two plain refits of the
    stacked replicates (set a, and pooled minus set a) and the pooled refit; the two values hold the same sums and differ by the rounding
    bound at most."""
    c = CR.corpus(33, 96)
    ctx = mmm.default_context()
    ref = CR.reference(c)
    got = _run(mmm, c)
    D, C, V, B = c.D, c.C, c.V, c.B
    pooled = np.stack([CR.dense(V, c.ptr_a, c.term_a, c.count_a, d) + CR.dense(V, c.ptr_b, c.term_b, c.count_b, d) for d in range(D)]).astype(np.int64)
    plain = {}
    for k, (p, t, n) in (("w_a", (c.ptr_a, c.term_a, c.count_a)), ("w_b", (c.ptr_b, c.term_b, c.count_b))):
        plain[k] = mmm.refit._raw(ctx, D, V, p, t, n, c.cat, c.allowed, None, c.maxiter, c.tol)
    dpV = np.arange(D + 1, dtype=np.int64) * V
    allv = np.tile(np.arange(V, dtype=np.int32), D)
    plain["w_pool"] = mmm.refit._raw(ctx, D, V, dpV, allv, pooled.ravel(), c.cat, c.allowed, None, c.maxiter, c.tol)
    tested = got["status"] == 0
    for k in ("w_a", "w_b", "w_pool"):
        assert np.array_equal(plain[k]["w"][tested].view(np.uint8), got[k][tested].view(np.uint8)), k
    assert np.array_equal(plain["w_pool"]["unexplained"][tested], got["unexplained"][tested])
    Xp = [np.stack([np.flatnonzero(n) + 1, n[np.flatnonzero(n)]], axis=1) for n in pooled]
    dealt = mmm.deal_counts(Xp, ref.N_a, B, seed=c.seed, stream=c.stream, V=V)                   # [B, D, V]
    assert np.array_equal(dealt[:, tested], ref.dealt[:, tested])
    dp = np.arange(B * D + 1, dtype=np.int64) * V
    term = np.tile(np.arange(V, dtype=np.int32), B * D)
    al = np.tile(c.allowed, (B, 1))
    fa = mmm.refit._raw(ctx, B * D, V, dp, term, dealt.ravel(), c.cat, al, None, c.maxiter, c.tol)
    fb = mmm.refit._raw(ctx, B * D, V, dp, term, (pooled[None] - dealt).ravel(), c.cat, al, None, c.maxiter, c.tol)
    lam = 2.0 * ((fa["ll_doc"] + fb["ll_doc"]).reshape(B, D) - plain["w_pool"]["ll_doc"][None, :])
    k = got["rep_stat"]
    assert (np.abs(k[:, tested] - lam[:, tested]) <= 2 * ref.rep_bound[:, tested]).all()
    delta = np.abs(fa["w"] - fb["w"]).reshape(B, D, C)
    dobs = np.abs(got["w_a"] - got["w_b"])
    on = (c.allowed != 0) & tested[:, None]
    assert np.array_equal(np.where(on, (delta >= dobs[None]).sum(axis=0), 0), got["count_sig"])
    assert np.array_equal(np.where(on, (np.where(on[None], delta, 0).max(axis=2, keepdims=True) >= dobs[None]).sum(axis=0), 0), got["count_max"])
    assert np.array_equal((fa["iters"] + fb["iters"]).reshape(B, D).sum(axis=0)[tested] + sum(plain[k]["iters"] for k in plain)[tested], got["iters"][tested])


def test_chunked_calls_add_and_runs_and_geometries_give_equal_bits(mmm, tuning):
    c = CR.corpus(3, 64)
    B, cut = c.B, 7
    whole, again = _run(mmm, c), _run(mmm, c)
    _same(whole, again, what="two runs")
    a, b, obs = _run(mmm, c, B=cut), _run(mmm, c, B=B - cut, b0=cut), _run(mmm, c, B=0)
    for k in ("w_a", "w_b", "w_pool", "status", "stat", "unexplained"):
        _same(whole, a, keys=(k,), what="first chunk"); _same(whole, b, keys=(k,), what="second chunk"); _same(whole, obs, keys=(k,), what="B = 0")
    for k in ("count_ge", "count_sig", "count_max"):
        assert np.array_equal(whole[k], a[k] + b[k]), k
        assert (obs[k] == 0).all(), k
    assert np.array_equal(whole["iters"], a["iters"] + b["iters"] - obs["iters"])
    assert np.array_equal(np.concatenate([a["rep_stat"], b["rep_stat"]]).view(np.uint8), whole["rep_stat"].view(np.uint8))
    assert obs["rep_stat"].shape == (0, c.D)
    _same(whole, _run(mmm, c, keep=False), keys=BITWISE + ("stat",), what="keep=False")
    full = _run(mmm, c._replace(allowed=None), B=4)
    ones = _run(mmm, c._replace(allowed=np.ones((c.D, c.C), dtype=np.uint8)), B=4)
    _same(full, ones, what="allowed = NULL")
    for cus in (1, 7):
        tuning(geometry_cus=cus)
        _same(whole, _run(mmm, c), what="geometry_cus = %d" % cus)
        tuning()
    big = CR.corpus(70, 130)
    ref = _run(mmm, big, key_bits=3)
    tuning(geometry_cus=2)
    _same(ref, _run(mmm, big, key_bits=3), what="geometry_cus = 2, key_bits = 3")


def test_every_error_and_the_degenerate_calls(mmm):
    c = CR.corpus(3, 64)
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, ci, ctypes.c_double, vp, vp, vp, vp, vp,
                             vp, vp, vp, vp, vp, vp)(("mmm_compare_exposures", L))
    D, C, V = c.D, c.C, c.V
    OUT = ("w_a", "w_b", "w_pool", "stat", "count_ge", "count_sig", "count_max", "status", "unexplained", "iters", "rep")

    def rc_of(D=D, C=C, V=V, pa=c.ptr_a, ta=c.term_a, ca=c.count_a, pb=c.ptr_b, tb=c.term_b, cb=c.count_b, cat=c.cat, allowed=c.allowed, B=3, b0=0, stream=0,
              key_bits=32, maxiter=5, tol=0.0, null=None, rows=None):
        n, m = rows or max(D, 1), max(C, 1)
        out = dict(w_a=np.full((n, m), 7.0), w_b=np.full((n, m), 7.0), w_pool=np.full((n, m), 7.0), stat=np.full(n, 7.0), count_ge=np.full(n, 7, np.int32),
                   count_sig=np.full((n, m), 7, np.int32), count_max=np.full((n, m), 7, np.int32), status=np.full(n, 7, np.int8), unexplained=np.full(n, 7.0),
                   iters=np.full(n, 7, np.int64), rep=np.full((max(B, 1), n), 7.0))
        names = ("pa", "ta", "ca", "pb", "tb", "cb", "cat", "allowed")
        keep = [np.ascontiguousarray(pa, dtype=np.int64), np.ascontiguousarray(ta, dtype=np.int32), np.ascontiguousarray(ca, dtype=np.int32),
                np.ascontiguousarray(pb, dtype=np.int64), np.ascontiguousarray(tb, dtype=np.int32), np.ascontiguousarray(cb, dtype=np.int32),
                np.ascontiguousarray(cat, dtype=np.float64), None if allowed is None else np.ascontiguousarray(allowed, dtype=np.uint8)]
        p = {k: (None if a is None or k == null else a.ctypes.data) for k, a in zip(names, keep)}
        o = {k: (None if k == null else a.ctypes.data) for k, a in out.items()}
        rc = plain(ctx.h, D, C, V, p["pa"], p["ta"], p["ca"], p["pb"], p["tb"], p["cb"], p["cat"], p["allowed"], B, b0, 9, stream, key_bits, maxiter, tol,
                   *[o[k] for k in OUT])
        untouched = all((a == 7).all() for a in out.values())
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    rc, _, untouched = rc_of()
    assert rc == 0 and not untouched
    assert rc_of(allowed=None)[0] == 0 and rc_of(B=0)[0] == 0 and rc_of(null="rep")[0] == 0 and rc_of(key_bits=1)[0] == 0
    rc, _, untouched = rc_of(D=0, pa=np.zeros(1, np.int64), pb=np.zeros(1, np.int64))
    assert rc == 0 and untouched                                                           # D = 0 writes nothing
    assert plain(None, *([0] * 29)) == -1

    def refused(code, needle=None, **kw):
        rc, msg, untouched = rc_of(**kw)
        assert rc == code and untouched and (needle is None or needle in msg), (sorted(kw), rc, msg, untouched)

    for null in ("cat", "pa", "ta", "ca", "pb", "tb", "cb") + OUT[:-1]:
        refused(-1, null=null)
    refused(-1, "key_bits", key_bits=0); refused(-1, "key_bits", key_bits=33)
    refused(-1, B=-1); refused(-1, b0=-1); refused(-1, "2^31 - 1", B=3, b0=2 ** 31 - 3)
    assert rc_of(B=3, b0=2 ** 31 - 4)[0] == 0
    refused(-1, "stream", stream=2 ** 31)
    assert rc_of(stream=2 ** 31 - 1)[0] == 0
    refused(-1, maxiter=0); refused(-1, tol=-1e-12); refused(-1, C=0); refused(-1, V=0); refused(-1, D=-1)
    for bad in (-1e-3, np.nan, np.inf):
        cat = c.cat.copy(); cat[2, 3] = bad
        refused(-1, "catalogue entry (2, 3)", cat=cat)
    cat = c.cat.copy(); cat[1] = 0.0
    refused(-1, "row 1", cat=cat)
    for which in ("a", "b"):
        term = (c.term_a if which == "a" else c.term_b).copy(); term[2] = V
        refused(-1, **{"t" + which: term})
        count = (c.count_a if which == "a" else c.count_b).copy(); count[1] = -1
        refused(-1, **{"c" + which: count})
        dp = (c.ptr_a if which == "a" else c.ptr_b).copy(); dp[0] = 1
        refused(-1, **{"p" + which: dp})
    refused(-4, "256", C=257, cat=np.ones((257, V)), allowed=None)
    refused(-4, "4096", V=4097, cat=np.ones((C, 4097)))
    refused(-4, "2^28", D=2 ** 28 + 1, rows=1)                                             # refused before an array is read
    one = np.asarray([0, 1], np.int64)
    half = dict(D=1, pa=one, ta=np.asarray([0], np.int32), ca=np.asarray([2 ** 30], np.int32), pb=one, tb=np.asarray([1], np.int32), allowed=c.allowed[:1])
    refused(-4, "2^31", cb=np.asarray([2 ** 30], np.int32), **half)
    big = np.asarray([2 ** 30, 2 ** 30], np.int32)
    refused(-4, "2^31", D=1, pa=np.asarray([0, 2], np.int64), ta=np.asarray([0, 1], np.int32), ca=big, pb=one, tb=np.asarray([1], np.int32),
            cb=np.asarray([1], np.int32), allowed=c.allowed[:1])
    with pytest.raises(mmm.MmmError, match="mmm_compare_exposures"):
        _run(mmm, c._replace(maxiter=0), B=2)

    # ---- mmm_deal_counts
    deal = ctypes.CFUNCTYPE(ci, vp, ci, vp, vp, vp, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, vp)(("mmm_deal_counts", L))
    dp, count, n_a = _deal_corpus()

    def deal_rc(D=n_a.size, dp=dp, count=count, n_a=n_a, B=2, b0=0, stream=0, key_bits=32, null=None):
        out = np.full((max(B, 1), max(int(np.asarray(dp)[-1]), 1)), 7, np.int32)
        keep = dict(dp=np.ascontiguousarray(dp, dtype=np.int64), count=np.ascontiguousarray(count, dtype=np.int32), n_a=np.ascontiguousarray(n_a, dtype=np.int32), out=out)
        p = {k: (None if k == null else a.ctypes.data) for k, a in keep.items()}
        rc = deal(ctx.h, D, p["dp"], p["count"], p["n_a"], B, b0, 9, stream, key_bits, p["out"])
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), bool((out == 7).all())

    rc, _, untouched = deal_rc()
    assert rc == 0 and not untouched
    for kw in (dict(B=0), dict(D=0, dp=np.zeros(1, np.int64))):
        rc, _, untouched = deal_rc(**kw)
        assert rc == 0 and untouched
    assert deal(None, *([0] * 10)) == -1

    def deal_refused(code, needle=None, **kw):
        rc, msg, untouched = deal_rc(**kw)
        assert rc == code and untouched and (needle is None or needle in msg), (sorted(kw), rc, msg, untouched)

    for null in ("dp", "count", "n_a", "out"):
        deal_refused(-1, null=null)
    deal_refused(-1, "key_bits", key_bits=0); deal_refused(-1, "key_bits", key_bits=33)
    deal_refused(-1, B=-1); deal_refused(-1, b0=-1); deal_refused(-1, "2^31 - 1", B=3, b0=2 ** 31 - 3); deal_refused(-1, "stream", stream=2 ** 31)
    bad = n_a.copy(); bad[0] = -1
    deal_refused(-1, "n_a[0]", n_a=bad)
    bad = n_a.copy(); bad[1] = 7
    deal_refused(-1, "n_a[1]", n_a=bad)
    bad = count.copy(); bad[3] = -2
    deal_refused(-1, count=bad)
    bad = dp.copy(); bad[2] = bad[1] - 1
    deal_refused(-1, dp=bad)
    deal_refused(-4, "2^31", D=1, dp=np.asarray([0, 2], np.int64), count=big, n_a=np.asarray([1], np.int32))
    deal_refused(-4, "2^28", D=2 ** 28 + 1)                                                # refused before an array is read


def test_edge_samples_through_the_python_layer(mmm):
    c = CR.edge_corpus()
    D, B, C = c.D, c.B, c.C
    names = ["S%d" % i for i in range(C)]
    Xa, Xb = _as_X(c.ptr_a, c.term_a, c.count_a), _as_X(c.ptr_b, c.term_b, c.count_b)
    r = mmm.compare_exposures(Xa, Xb, (names, None, c.cat), allowed=c.allowed, B=B, seed=c.seed, stream=c.stream, maxiter=c.maxiter, tol=c.tol, keep_replicates=True)
    raw = _run(mmm, c)
    ref = CR.compare(c)
    assert r.names == names and r.B == B and r.p.shape == (D,) and r.exposures_a.shape == (C, D) and r.replicates.shape == (B, D)
    for f, k in (("stat", "stat"), ("count_ge", "count_ge"), ("status", "status"), ("unexplained", "unexplained"), ("iters", "iters")):
        assert np.array_equal(getattr(r, f).view(np.uint8), raw[k].view(np.uint8)), f
    for f, k in (("exposures_a", "w_a"), ("exposures_b", "w_b"), ("exposures_pooled", "w_pool"), ("count_sig", "count_sig"), ("count_max", "count_max")):
        assert np.array_equal(getattr(r, f).T, raw[k]), f
    assert np.array_equal(r.replicates, raw["rep_stat"], equal_nan=True)
    assert np.array_equal(r.status, ref.status) and r.status.tolist() == [0, 3, 3, 3, 0]
    assert np.array_equal(np.ascontiguousarray(r.exposures_a.T).view(np.uint8), ref.w_a.view(np.uint8)) and np.array_equal(r.count_max.T, ref.count_max)
    assert np.array_equal(r.delta, np.abs(r.exposures_a - r.exposures_b))
    un = r.status == 3
    assert np.isnan(r.p[un]).all() and np.isnan(r.p_signature[:, un]).all() and np.isnan(r.p_adjusted[:, un]).all() and np.isnan(r.replicates[:, un]).all()
    assert (r.exposures_a[:, un] == 0).all() and (r.exposures_pooled[:, un] == 0).all() and (r.count_ge[un] == 0).all() and (r.iters[un] == 0).all() and (r.stat[un] == 0).all()
    assert np.array_equal(r.p[~un], (1.0 + r.count_ge[~un]) / (B + 1.0)) and np.isfinite(r.replicates[:, ~un]).all()
    off = c.allowed.T == 0
    assert np.isnan(r.p_adjusted[off]).all() and (r.exposures_a[off] == 0).all() and (r.count_sig[off] == 0).all()
    on = ~off & ~un[None, :]
    assert np.array_equal(r.p_adjusted[on], (1.0 + r.count_max[on]) / (B + 1.0)) and (r.p_adjusted[on] >= r.p_signature[on]).all()
    assert np.isnan(r.q[un]).all() and np.isfinite(r.q[~un]).all()
    assert set(r.changed(1.0)) == {0, 4} and all(d in (0, 4) and s in names for d, s in r.changed_signatures(1.0))
    # B = 0: the observed phase only
    r0 = mmm.compare_exposures(Xa, Xb, c.cat, allowed=c.allowed, B=0, maxiter=c.maxiter, tol=c.tol)
    assert np.isnan(r0.p).all() and np.array_equal(r0.stat, r.stat) and np.array_equal(r0.status, r.status) and (r0.count_sig == 0).all() and r0.replicates is None
    assert r0.names is None and r0.changed_signatures(1.0) == []
    # a RefitResult as `allowed`: its chosen sets -- the pooled refit, as the docstring recommends
    pooled = [np.concatenate([a, b]) for a, b in zip(Xa, Xb)]
    rr = mmm.refit_exposures(pooled, c.cat, maxiter=c.maxiter)
    x = mmm.compare_exposures(Xa, Xb, c.cat, allowed=rr, B=4, seed=1, maxiter=c.maxiter)
    y = mmm.compare_exposures(Xa, Xb, c.cat, allowed=rr.active.T, B=4, seed=1, maxiter=c.maxiter)
    assert np.array_equal(x.stat, y.stat) and np.array_equal(x.count_ge, y.count_ge) and np.array_equal(x.exposures_a, y.exposures_a)
    assert ((x.exposures_a > 0) <= rr.active).all()
