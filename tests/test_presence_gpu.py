"""mmm_presence_test on the device against its float64 restatement (tests/presence_ref.py): the null weights, the score, the target's weight in
the larger fit, status, count_zero and iters bit for bit / integer for integer (only +, x, / and comparisons decide them); Λ_obs and the kept
Λ_b against a longdouble evaluation on the same mixtures within 2 (bound(ll0) + bound(ll1)); count_ge as an integer (tests/
test_presence_cpu.py asserts that no comparison of these corpora is near a tie); the two places the catalogue is read from; the shipped
entries the definition is composed of; every error."""
import ctypes

import numpy as np
import pytest

import presence_ref as PR
import refit_ref as R

pytestmark = pytest.mark.gpu

BITWISE = ("w_null", "score", "w_alt", "status", "count_zero", "iters", "count_ge")
ALL = BITWISE + ("stat", "rep_stat")


def _run(mmm, c, B=None, b0=0, keep=True, **kw):
    return mmm.presence._raw(mmm.default_context(), c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, c.targets, c.allowed, c.B if B is None else B, b0, c.seed,
                             c.stream, c.maxiter, c.tol, keep=keep, **kw)


def _same(a, b, keys=ALL, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _within(got, ld, bound, what):
    """got against the longdouble values ld within bound, element by element; inf and NaN must sit in the same places"""
    got, ld, bound = np.asarray(got).ravel(), np.asarray(ld).ravel(), np.asarray(bound).ravel()
    fin = np.isfinite(ld)
    assert np.array_equal(np.isnan(got), np.isnan(ld)) and np.array_equal(got[~fin & ~np.isnan(ld)], ld[~fin & ~np.isnan(ld)]), what
    err = np.abs(got[fin] - ld[fin])
    bad = np.flatnonzero(err > bound[fin])
    assert bad.size == 0, "%s: %d values beyond the bound, the first %r against %r (bound %g)" % (what, bad.size, got[fin][bad[0]], ld[fin][bad[0]], bound[fin][bad[0]])
    return float((err / np.maximum(bound[fin], 1e-300)).max()) if err.size and (bound[fin] > 0).any() else 0.0


def _against_reference(c, got):
    ref = PR.reference(c)
    want = dict(w_null=ref.w_null, score=ref.score, w_alt=ref.w_alt, status=ref.status, count_zero=ref.count_zero, iters=ref.iters, count_ge=ref.count_ge)
    for k in BITWISE:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.flatnonzero((got[k].reshape(ref.status.size, -1).view(np.uint8) != want[k].reshape(ref.status.size, -1).view(np.uint8)).any(axis=1))
        assert bad.size == 0, "%s: %s differs in items %s" % (c.name, k, bad.tolist())
    worst = _within(got["stat"], ref.stat_ld, ref.bound, c.name + " stat")
    worst = max(worst, _within(got["rep_stat"], ref.rep_ld, ref.rep_bound, c.name + " replicates"))
    # the branch of every replicate: Λ_b is 0 exactly where fit(A1) was skipped or clamped, in the same places
    assert np.array_equal(got["rep_stat"] == 0, ref.rep == 0)
    print("%s: largest Λ error / bound = %.3f" % (c.name, worst))


@pytest.mark.parametrize("i", range(len(PR.SHAPES) + 1), ids=lambda i: PR.corpora()[i].name)
def test_outputs_equal_the_restatement_wherever_the_catalogue_is_read_from(mmm, i):
    c = PR.corpora()[i]
    got = _run(mmm, c)
    _against_reference(c, got)
    l2 = _run(mmm, c, catalogue_in_lds=False)
    _same(got, l2, what="LDS against L2")
    assert mmm.default_context().get_tuning().disable == 0                # the hook is undone
    if c.name == "C6V1536":       # the shape at which only the two-row items fit LDS beside four waves' buffers: both launches ran
        n1 = [PR.sets(c, j)[3].size for j in range(got["status"].size) if got["status"][j] == 0]
        assert min(n1) <= 2 < max(n1), n1


def _as_X(c):
    return [np.stack([c.term[a:b].astype(np.int64) + 1, c.count[a:b].astype(np.int64)], axis=1) for a, b in zip(c.doc_ptr[:-1], c.doc_ptr[1:])]


def test_edge_items_through_the_python_layer(mmm):
    c = PR.edge_corpus()
    D, B = c.D, c.B
    names = ["S%d" % i for i in range(c.C)]
    r = mmm.signature_presence(_as_X(c), (names, None, c.cat), ["S5", "S1", "S2"], allowed=c.allowed, B=B, seed=c.seed, stream=c.stream, maxiter=c.maxiter,
                               tol=c.tol, keep_replicates=True)
    raw = _run(mmm, c)
    ref = PR.reference(c)
    assert r.names == ["S5", "S1", "S2"] and r.B == B and r.p.shape == (3, D) and r.exposures_null.shape == (3, c.C, D) and r.replicates.shape == (B, 3, D)
    for f, k in (("stat", "stat"), ("score", "score"), ("exposure_alt", "w_alt"), ("count_ge", "count_ge"), ("count_zero", "count_zero"), ("status", "status"),
                 ("iters", "iters")):
        assert np.array_equal(getattr(r, f).ravel().view(np.uint8), raw[k].view(np.uint8)), f
    assert np.array_equal(r.exposures_null.transpose(0, 2, 1).reshape(3 * D, c.C), raw["w_null"])
    assert np.array_equal(r.replicates.reshape(B, 3 * D), raw["rep_stat"], equal_nan=True)
    st = r.status
    assert (st[:, 1] == 3).all() and np.isnan(r.p[:, 1]).all()                              # the empty document
    assert st[0, 4] == 3 and np.isnan(r.p[0, 4]) and (r.exposures_null[0, :, 4] == 0).all()    # the target is the only allowed signature: A0 empty
    assert st[1, 4] != 3 and st[2, 4] != 3                                                  # ... the other targets are tested against it
    assert (st[:, 2] != 3).all()                                                            # one mutation
    assert st[0, 3] in (0, 1) and r.exposures_null[0, 5, 3] == 0                            # target outside `allowed`: added to A1, absent from A0
    assert st[0, 5] == 2 and st[0, 6] == 2 and np.isinf(r.stat[0, 5]) and r.p[0, 5] == 1.0 / (B + 1) and r.count_ge[0, 5] == 0   # only the target produces the term
    assert st[1, 6] in (0, 1) and np.isfinite(r.stat[1, 6])                                 # the term stays unexplained with and without target 1
    assert st[2, 7] == 1 and r.score[2, 7] == 0 and r.p[2, 7] == 1.0 and r.count_ge[2, 7] == B and r.count_zero[2, 7] == 0   # the target cannot improve it
    assert (r.exposures_null[2, 2, :] == 0).all()                                           # a row no document allows, as a target
    untested = st != 0
    assert np.isnan(r.replicates[:, untested]).all() and np.isfinite(r.replicates[:, ~untested]).all() and (r.count_zero[untested] == 0).all()
    assert np.array_equal(r.p[st != 3], (1.0 + r.count_ge[st != 3]) / (B + 1.0))
    assert np.array_equal(r.significant(1.0 / (B + 1)), np.nan_to_num(r.p, nan=2.0) <= 1.0 / (B + 1)) and r.significant(1.0 / (B + 1))[0, 5]
    assert np.array_equal(st.ravel(), ref.status)
    # B = 0: the observed phase only
    r0 = mmm.signature_presence(_as_X(c), c.cat, [5, 1, 2], allowed=c.allowed, B=0, maxiter=c.maxiter, tol=c.tol)
    assert np.isnan(r0.p).all() and np.array_equal(r0.stat, r.stat) and np.array_equal(r0.status, st) and (r0.count_zero == 0).all() and r0.replicates is None
    # a RefitResult as `allowed`: its chosen sets
    rr = mmm.refit_exposures(_as_X(c), c.cat, allowed=c.allowed, maxiter=c.maxiter)
    a = mmm.signature_presence(_as_X(c), c.cat, [1], allowed=rr, B=4, seed=1, maxiter=c.maxiter)
    b = mmm.signature_presence(_as_X(c), c.cat, [1], allowed=rr.active.T, B=4, seed=1, maxiter=c.maxiter)
    assert np.array_equal(a.stat, b.stat) and np.array_equal(a.count_ge, b.count_ge) and np.array_equal(a.exposures_null, b.exposures_null)


def test_the_null_fit_is_the_shipped_refit_and_the_replicates_are_the_shipped_draws(mmm):
    """exposures_null = refit_exposures(penalty=None, allowed=A0) bit for bit.  Every kept Λ_b against the composition of the public entries:
    simulate_counts(w0, P, N) under the same seed and stream, then two plain refits of the stacked replicates.  Where the kernel ran both
    fits the two values hold the same sums and differ by the rounding bound at most; where it skipped fit(A1) (Λ_b = 0 exactly) the composed
    value is what tests/test_presence_cpu.py bounds: below 1e-4."""
    c = PR.corpus(12, 96)
    ctx = mmm.default_context()
    ref = PR.reference(c)
    got = _run(mmm, c)
    D, C, V, B, T = c.D, c.C, c.V, c.B, len(c.targets)
    P = R.normalise(c.cat)
    N = np.tile(ref.N, T)
    sim = mmm.simulate_counts(got["w_null"].T, P.T, N, B=B, seed=c.seed, stream=c.stream, ctx=ctx)          # [B, T D, V]
    for ti, t in enumerate(c.targets):
        a0 = c.allowed.copy(); a0[:, t] = 0
        a1 = c.allowed.copy(); a1[:, t] = 1
        plain = mmm.refit._raw(ctx, D, V, c.doc_ptr, c.term, c.count, c.cat, a0, None, c.maxiter, c.tol)
        assert np.array_equal(plain["w"].view(np.uint8), got["w_null"][ti * D:(ti + 1) * D].view(np.uint8)), t
        counts = sim[:, ti * D:(ti + 1) * D, :].reshape(B * D, V)
        dp = np.arange(B * D + 1, dtype=np.int64) * V
        term = np.tile(np.arange(V, dtype=np.int32), B * D)
        f0 = mmm.refit._raw(ctx, B * D, V, dp, term, counts.ravel(), c.cat, np.tile(a0, (B, 1)), None, c.maxiter, c.tol)
        f1 = mmm.refit._raw(ctx, B * D, V, dp, term, counts.ravel(), c.cat, np.tile(a1, (B, 1)), None, c.maxiter, c.tol)
        lam = np.maximum(2.0 * (f1["ll_doc"] - f0["ll_doc"]), 0.0).reshape(B, D)
        for d in range(D):
            j = ti * D + d
            if got["status"][j] != 0:
                continue
            assert np.array_equal(counts.reshape(B, D, V)[:, d].sum(axis=1), np.full(B, ref.N[d]))
            k = got["rep_stat"][:, j]
            ran = k > 0
            assert (np.abs(k[ran] - lam[ran, d]) <= 2 * ref.rep_bound[ran, j]).all(), (j, k[ran], lam[ran, d])
            assert (lam[~ran, d] < 1e-4).all(), (j, lam[~ran, d])


def test_chunked_calls_add_and_two_runs_give_equal_bits(mmm):
    c = PR.corpus(12, 96)
    B, cut = c.B, 7
    whole, again = _run(mmm, c), _run(mmm, c)
    _same(whole, again, what="two runs")
    a, b, obs = _run(mmm, c, B=cut), _run(mmm, c, B=B - cut, b0=cut), _run(mmm, c, B=0)
    tested = whole["status"] == 0
    for k in ("w_null", "score", "w_alt", "status", "stat"):
        _same(whole, a, keys=(k,), what="first chunk"); _same(whole, b, keys=(k,), what="second chunk"); _same(whole, obs, keys=(k,), what="B = 0")
    assert np.array_equal(whole["count_ge"][tested], (a["count_ge"] + b["count_ge"])[tested]) and np.array_equal(whole["count_zero"], a["count_zero"] + b["count_zero"])
    assert (a["count_ge"][whole["status"] == 1] == cut).all() and (obs["count_ge"] == 0).all() and (obs["count_zero"] == 0).all()
    assert np.array_equal(whole["iters"], a["iters"] + b["iters"] - obs["iters"])
    assert np.array_equal(np.concatenate([a["rep_stat"], b["rep_stat"]]).view(np.uint8), whole["rep_stat"].view(np.uint8))
    assert obs["rep_stat"].shape == (0, whole["status"].size)
    # without the replicate buffer: the same counts
    _same(whole, _run(mmm, c, keep=False), keys=BITWISE + ("stat",), what="keep=False")
    # no `allowed`: the whole catalogue
    full = _run(mmm, c._replace(allowed=None), B=4)
    ones = _run(mmm, c._replace(allowed=np.ones((c.D, c.C), dtype=np.uint8)), B=4)
    _same(full, ones, what="allowed = NULL")


def test_every_error(mmm):
    c = PR.corpus(4, 5)
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, ctypes.c_double, vp, vp, vp, vp, vp,
                             vp, vp, vp, vp)(("mmm_presence_test", L))
    D, C, V, T = c.D, c.C, c.V, len(c.targets)

    def rc_of(D=D, C=C, V=V, dp=c.doc_ptr, term=c.term, count=c.count, cat=c.cat, allowed=c.allowed, T=T, targets=c.targets, B=3, b0=0, maxiter=5, tol=0.0,
              null=None, h=None):
        n = max(T if T < 100 else 1, 1) * max(D, 1)
        out = dict(w_null=np.full((n, max(C, 1)), 7.0), stat=np.full(n, 7.0), score=np.full(n, 7.0), w_alt=np.full(n, 7.0), count_ge=np.full(n, 7, np.int32),
                   count_zero=np.full(n, 7, np.int32), status=np.full(n, 7, np.int8), iters=np.full(n, 7, np.int64), rep=np.full((max(B, 1), n), 7.0))
        keep = [np.ascontiguousarray(dp, dtype=np.int64), np.ascontiguousarray(term, dtype=np.int32), np.ascontiguousarray(count, dtype=np.int32),
                np.ascontiguousarray(cat, dtype=np.float64), None if allowed is None else np.ascontiguousarray(allowed, dtype=np.uint8),
                np.ascontiguousarray(targets, dtype=np.int32)]
        p = {k: (None if a is None or k == null else a.ctypes.data) for k, a in zip(("dp", "term", "count", "cat", "allowed", "targets"), keep)}
        o = {k: (None if k == null else a.ctypes.data) for k, a in out.items()}
        rc = plain(ctx.h if h is None else h, D, C, V, p["dp"], p["term"], p["count"], p["cat"], p["allowed"], T, p["targets"], B, b0, 9, 0, maxiter, tol, o["w_null"],
                   o["stat"], o["score"], o["w_alt"], o["count_ge"], o["count_zero"], o["status"], o["iters"], o["rep"])
        untouched = all((a == 7).all() for a in out.values())
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    rc, _, untouched = rc_of()
    assert rc == 0 and not untouched
    assert rc_of(allowed=None)[0] == 0 and rc_of(B=0)[0] == 0 and rc_of(null="rep")[0] == 0
    rc, _, untouched = rc_of(D=0, dp=np.zeros(1, np.int64))
    assert rc == 0 and untouched                                                           # D = 0 writes nothing
    assert plain(None, *([0] * 25)) == -1

    def refused(code, needle=None, **kw):
        rc, msg, untouched = rc_of(**kw)
        assert rc == code and untouched and (needle is None or needle in msg), (kw.keys(), rc, msg, untouched)

    for null in ("cat", "dp", "term", "count", "targets", "w_null", "stat", "score", "w_alt", "count_ge", "count_zero", "status", "iters"):
        refused(-1, null=null)
    refused(-1, T=0)
    refused(-1, "targets[1]", targets=np.asarray([0, C], np.int32))
    refused(-1, "targets[0]", targets=np.asarray([-1, 1], np.int32))
    refused(-1, B=-1); refused(-1, b0=-1); refused(-1, "2^31 - 1", B=3, b0=2 ** 31 - 3)
    assert rc_of(B=3, b0=2 ** 31 - 4)[0] == 0
    refused(-1, maxiter=0); refused(-1, tol=-1e-12); refused(-1, C=0); refused(-1, V=0); refused(-1, D=-1)
    for bad in (-1e-3, np.nan, np.inf):
        cat = c.cat.copy(); cat[2, 3] = bad
        refused(-1, "catalogue entry (2, 3)", cat=cat)
    cat = c.cat.copy(); cat[1] = 0.0
    refused(-1, "row 1", cat=cat)
    term = c.term.copy(); term[2] = V
    refused(-1, term=term)
    count = c.count.copy(); count[1] = -1
    refused(-1, count=count)
    dp = c.doc_ptr.copy(); dp[0] = 1
    refused(-1, dp=dp)
    refused(-4, "256", C=257, cat=np.ones((257, V)), allowed=None)
    refused(-4, "4096", V=4097, cat=np.ones((C, 4097)))
    refused(-4, "items", T=2 ** 30, D=2, dp=c.doc_ptr[:3], allowed=c.allowed[:2])
    big = np.asarray([2 ** 30, 2 ** 30], np.int32)
    refused(-4, "2^31", D=1, dp=np.asarray([0, 2], np.int64), term=np.asarray([0, 1], np.int32), count=big, allowed=c.allowed[:1])
    with pytest.raises(mmm.MmmError, match="mmm_presence_test"):
        mmm.presence._raw(ctx, c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, c.targets, c.allowed, B=2, maxiter=0)
