"""mmm_attribute_mutations on the device against its float64 restatement (tests/attribute_ref.py).  No log is involved and every accumulator
is an integer, so EVERY comparison here is bit for bit or integer for integer and nothing is excluded: the observed weights and posteriors,
the kept posteriors of every replicate, the fixed-point sums, the top and void counts, the group totals and the iteration counts; the
shipped entries the definition is composed of; every launch geometry, both places the catalogue is read from, two runs, chunked calls;
the edges; every refusal; the Python layer."""
import ctypes

import numpy as np
import pytest

import attribute_ref as A
import refit_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("w", "post", "status", "iters", "sum_fx", "sumsq_fx", "top_count", "void_count", "group_fx", "rep_post")


def _run(mmm, c, B=None, b0=0, keep=True):
    return mmm.attribute._raw(mmm.default_context(), c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, c.q_ptr, c.q_term, c.q_mult, c.q_group, c.G,
                              c.B if B is None else B, b0, c.seed, c.stream, c.maxiter, c.tol, keep=keep)


def _same(a, b, keys=KEYS, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _against(ref, got, name):
    for k in KEYS:
        want = getattr(ref, k)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, k, got[k].dtype, want.dtype, got[k].shape, want.shape)
        bad = np.flatnonzero(got[k].ravel().view(np.uint8) != want.ravel().view(np.uint8))
        assert bad.size == 0, "%s: %s differs, first at flat byte %d: %r against %r" % (
            name, k, bad[0], got[k].ravel()[bad[0] // got[k].itemsize], want.ravel()[bad[0] // got[k].itemsize])


@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "C%dV%d" % s)
def test_every_output_equals_the_restatement_and_w_is_the_shipped_refit(mmm, shape):
    c, ref = A.case(*shape), A.reference(*shape)
    got = _run(mmm, c)
    _against(ref, got, c.name)
    plain = mmm.refit._raw(mmm.default_context(), c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, None, c.maxiter, c.tol)
    ran = got["status"] == 0
    assert ran.any() and np.array_equal(plain["w"][ran].view(np.uint8), got["w"][ran].view(np.uint8)) and (got["w"][~ran] == 0).all()
    assert np.array_equal(got["status"] == 3, (np.diff(c.q_ptr) > 0) & ~(plain["w"] > 0).any(axis=1))


@pytest.mark.parametrize("shape", [(12, 96), (65, 96)], ids=lambda s: "C%dV%d" % s)
def test_kept_posteriors_equal_the_composed_shipped_path(mmm, shape):
    """mmm_resample_counts under the same seed and stream, mmm_refit_exposures (penalty = NULL) on the stacked replicates, the posterior in
    numpy: the bits of rep_post"""
    c = A.case(*shape)
    ctx = mmm.default_context()
    got = _run(mmm, c)
    D, B, nnz = c.D, c.B, int(c.doc_ptr[-1])
    rc = mmm.bootstrap._resample_csr(ctx, D, c.doc_ptr, c.count, B, 0, c.seed, c.stream)
    dps = np.concatenate([(c.doc_ptr[:-1][None, :] + nnz * np.arange(B, dtype=np.int64)[:, None]).ravel(), [B * nnz]])
    fit = mmm.refit._raw(ctx, B * D, c.V, dps, np.tile(c.term, B), rc.ravel(), c.cat, np.tile(c.allowed, (B, 1)), None, c.maxiter, c.tol, outputs="w")
    w = fit["w"].reshape(B, D, c.C)
    P = R.normalise(c.cat)
    for d in np.flatnonzero(got["status"] == 0):
        Ad = np.flatnonzero(c.allowed[d])
        e = np.arange(c.q_ptr[d], c.q_ptr[d + 1])
        for b in range(B):
            q = R.mixture(w[b, d, Ad], P[Ad])
            want = np.zeros((e.size, c.C))
            want[:, Ad] = A.posterior(w[b, d, Ad], P[Ad], q, c.q_term[e])
            assert np.array_equal(want.view(np.uint8), got["rep_post"][b, e].view(np.uint8)), (d, b)


def test_equal_bits_across_geometries_catalogue_places_runs_and_chunks(mmm, tuning):
    for shape in ((12, 96), (70, 1536), (2, 5)):
        c = A.case(*shape)
        whole = _run(mmm, c)
        _same(whole, _run(mmm, c), what="two runs")
        for cus in (1, 3):
            tuning(geometry_cus=cus)
            _same(whole, _run(mmm, c), what="geometry_cus=%d" % cus)
        tuning(disable=("refit_lds",))
        _same(whole, _run(mmm, c), what="catalogue through L2")
        tuning()
        assert mmm.default_context().get_tuning().disable == 0 and mmm.default_context().get_tuning().geometry_cus == 0      # the hook is undone
        cut = 2
        a, b, obs = _run(mmm, c, B=cut), _run(mmm, c, B=c.B - cut, b0=cut), _run(mmm, c, B=0)
        for k in ("w", "post", "status"):
            _same(whole, a, keys=(k,), what="first chunk"); _same(whole, b, keys=(k,), what="second chunk"); _same(whole, obs, keys=(k,), what="B = 0")
        for k in ("sum_fx", "sumsq_fx", "top_count", "void_count"):
            assert np.array_equal(a[k] + b[k], whole[k]), k
            assert not obs[k].any()
        assert np.array_equal(np.concatenate([a["group_fx"], b["group_fx"]]), whole["group_fx"])
        assert np.array_equal(np.concatenate([a["rep_post"], b["rep_post"]]).view(np.uint8), whole["rep_post"].view(np.uint8))
        assert np.array_equal(whole["iters"], a["iters"] + b["iters"] - obs["iters"]) and obs["rep_post"].shape[0] == 0
        _same(whole, _run(mmm, c, keep=False), keys=KEYS[:-1], what="without rep_post")


def test_edges(mmm):
    c, ref = A.case(12, 96), A.reference(12, 96)
    got = _run(mmm, c)
    doc = np.repeat(np.arange(c.D), np.diff(c.q_ptr))
    st = got["status"]
    assert st.tolist() == [0, 4, 3, 0, 3, 0]                   # queried / no queries / N = 0 / one mutation / empty allowed row / unexplained term
    for d in (1, 2, 4):                                        # nothing else is written for them, no replicates run
        m = doc == d
        assert (got["w"][d] == 0).all() and got["iters"][d] == 0
        assert not got["post"][m].any() and not got["sum_fx"][m].any() and not got["top_count"][m].any() and not got["void_count"][m].any() and not got["rep_post"][:, m].any()
    # a query on a term no allowed signature produces: void observed and in every replicate
    e = np.flatnonzero((doc == 5) & (c.q_term == c.V - 1))
    assert e.size and not got["post"][e].any() and (got["void_count"][e] == c.B).all() and not got["top_count"][e].any()
    # a query on a term absent from the document: a posterior all the same
    n0 = A.dense(c, 0)
    absent = np.flatnonzero((doc == 0) & (n0[c.q_term] == 0))
    assert absent.size and (np.abs(got["post"][absent].sum(axis=1) - 1) <= c.C * 2.0 ** -52).all()
    # duplicate queries: equal rows
    dup = np.flatnonzero((doc == 0) & (c.q_term == c.q_term[0]))
    assert dup.size >= 2 and np.array_equal(got["post"][dup[0]], got["post"][dup[-1]]) and np.array_equal(got["sumsq_fx"][dup[0]], got["sumsq_fx"][dup[-1]])
    # mult > 1 and group -1 enter group_fx as the definition says
    x = np.floor(got["rep_post"] * A.FX_ONE).astype(np.uint64)
    g = np.zeros_like(got["group_fx"])
    m = c.q_group >= 0
    for b in range(c.B):
        np.add.at(g[b], c.q_group[m], x[b][m] * c.q_mult[m].astype(np.uint64)[:, None])
    assert (c.q_mult[m] > 1).any() and (~m).any() and np.array_equal(g, got["group_fx"])
    # G = 0 with and without a group array, mult = NULL: the other outputs keep their bits; mult NULL is mult 1
    rest = tuple(k for k in KEYS if k != "group_fx")
    for variant in (c._replace(G=0, q_group=None), c._replace(G=0, q_group=np.full(c.q_term.size, -1, np.int32)), c._replace(q_group=None)):
        r = _run(mmm, variant)
        _same(got, r, keys=rest, what="no groups")
        assert not r["group_fx"].any()
    _same(_run(mmm, c._replace(q_mult=None)), _run(mmm, c._replace(q_mult=np.ones_like(c.q_mult))), what="mult = NULL")
    # allowed = NULL is the whole catalogue
    _same(_run(mmm, c._replace(allowed=None), B=2), _run(mmm, c._replace(allowed=np.ones_like(c.allowed)), B=2), what="allowed = NULL")
    # identical catalogue rows tie, the lowest c takes the count
    t = A.twin()
    r = _run(mmm, t)
    _against(A.attribute(t), r, "twin")
    assert np.array_equal(r["post"][:, 4], r["post"][:, 5]) and not r["top_count"][:, 5].any() and r["top_count"][:, 4].any()


def test_planted_disjoint_signatures_and_a_replicate_that_loses_one(mmm):
    c = A.planted()
    got = _run(mmm, c)
    _against(A.attribute(c), got, c.name)
    assert set(np.unique(got["post"])) == {0.0, 1.0} and set(np.unique(got["rep_post"])) == {0.0, 1.0}
    first = slice(0, int(c.q_ptr[1]))                         # document 0: p_top = 1 for the planted signature of every term
    assert np.array_equal(got["top_count"][first], (got["post"][first] * c.B).astype(np.int32)) and not got["void_count"][first].any()
    e = int(c.q_ptr[1]) + 3                                   # document 1's single mutation of signature 1: lost in some replicates
    assert got["post"][e, 1] == 1 and 0 < got["void_count"][e] < c.B and got["top_count"][e, 1] == c.B - got["void_count"][e]
    assert got["sum_fx"][e, 1] == int(c.B - got["void_count"][e]) * A.FX_ONE


def test_every_refusal_writes_nothing(mmm):
    c = A.case(2, 5)
    c = c._replace(q_ptr=np.minimum(c.q_ptr, 40), q_term=c.q_term[:40], q_mult=c.q_mult[:40], q_group=c.q_group[:40])      # 40 queries, all of document 0
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, ctypes.c_double, vp, vp, vp,
                             vp, vp, vp, vp, vp, vp, vp)(("mmm_attribute_mutations", L))
    D, C, V, G = c.D, c.C, c.V, c.G
    Q = 40

    def rc_of(D=D, C=C, V=V, dp=c.doc_ptr, term=c.term, count=c.count, cat=c.cat, allowed=c.allowed, qp=c.q_ptr, qt=c.q_term, qm=c.q_mult, qg=c.q_group, G=G, B=3,
              b0=0, maxiter=5, tol=0.0, null=None, h=None):
        nq, nd, nc = max(Q, len(qt)), max(D, 1), max(C, 1)
        out = dict(w=np.full((nd, nc), 7.0), post=np.full((nq, nc), 7.0), status=np.full(nd, 7, np.int8), iters=np.full(nd, 7, np.int64),
                   sum_fx=np.full((nq, nc), 7, np.uint64), sumsq_fx=np.full((nq, nc), 7, np.uint64), top_count=np.full((nq, nc), 7, np.int32),
                   void_count=np.full(nq, 7, np.int32), group_fx=np.full((min(max(B, 1), 8), max(G, 1), nc), 7, np.uint64),
                   rep_post=np.full((min(max(B, 1), 8), nq, nc), 7.0))
        names = ("dp", "term", "count", "cat", "allowed", "qp", "qt", "qm", "qg")
        types = (np.int64, np.int32, np.int32, np.float64, np.uint8, np.int64, np.int32, np.int32, np.int32)
        keep = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in zip((dp, term, count, cat, allowed, qp, qt, qm, qg), types)]
        p = {k: (None if a is None or k == null else a.ctypes.data) for k, a in zip(names, keep)}
        o = {k: (None if k == null else a.ctypes.data) for k, a in out.items()}
        rc = plain(ctx.h if h is None else h, D, C, V, p["dp"], p["term"], p["count"], p["cat"], p["allowed"], p["qp"], p["qt"], p["qm"], p["qg"], G, B, b0, 9, 0,
                   maxiter, tol, *[o[k] for k in KEYS])
        untouched = all((a == 7).all() for a in out.values())
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    rc, _, untouched = rc_of()
    assert rc == 0 and not untouched
    assert rc_of(allowed=None)[0] == 0 and rc_of(B=0)[0] == 0 and rc_of(null="rep_post")[0] == 0 and rc_of(qm=None)[0] == 0 and rc_of(qg=None)[0] == 0
    assert rc_of(G=0, qg=None, null="group_fx")[0] == 0
    assert rc_of(B=0, null="sum_fx")[0] == 0                                               # the replicate outputs may be NULL when B = 0
    rc, _, untouched = rc_of(D=0, dp=np.zeros(1, np.int64), qp=np.zeros(1, np.int64))
    assert rc == 0 and untouched                                                           # D = 0 writes nothing
    rc, _, untouched = rc_of(qp=np.zeros(D + 1, np.int64))
    assert rc == 0 and untouched                                                           # Q = 0 writes nothing
    assert plain(None, *([0] * 29)) == -1

    def refused(code, needle=None, **kw):
        rc, msg, untouched = rc_of(**kw)
        assert rc == code and untouched and (needle is None or needle in msg), (list(kw), rc, msg, untouched)

    for null in ("cat", "dp", "term", "count", "qp", "qt", "w", "post", "status", "iters", "sum_fx", "sumsq_fx", "top_count", "void_count", "group_fx"):
        refused(-1, null=null)
    qp = c.q_ptr.copy(); qp[0] = 1
    refused(-1, "q_ptr[0]", qp=qp)
    qp = c.q_ptr.copy(); qp[2] = qp[1] - 1
    refused(-1, "q_ptr decreases", qp=qp)
    qt = c.q_term.copy(); qt[3] = V
    refused(-1, "query 3", qt=qt)
    qt = c.q_term.copy(); qt[0] = -1
    refused(-1, "query 0", qt=qt)
    qm = c.q_mult.copy(); qm[5] = 0
    refused(-1, "mult", qm=qm)
    for bad in (-2, G):
        qg = c.q_group.copy(); qg[7] = bad
        refused(-1, "group", qg=qg)
    refused(-1, G=-1, qg=None)
    refused(-1, B=-1); refused(-1, b0=-1); refused(-1, "2^31 - 1", B=3, b0=2 ** 31 - 3)
    assert rc_of(B=3, b0=2 ** 31 - 4)[0] == 0
    refused(-1, maxiter=0); refused(-1, tol=-1e-12); refused(-1, C=0); refused(-1, V=0); refused(-1, D=-1)
    for bad in (-1e-3, np.nan, np.inf):
        cat = c.cat.copy(); cat[1, 3] = bad
        refused(-1, "catalogue entry (1, 3)", cat=cat)
    cat = c.cat.copy(); cat[1] = 0.0
    refused(-1, "row 1", cat=cat)
    term = c.term.copy(); term[2] = V
    refused(-1, term=term)
    count = c.count.copy(); count[1] = -1
    refused(-1, count=count)
    dp = c.doc_ptr.copy(); dp[0] = 1
    refused(-1, dp=dp)
    one = np.asarray([0, 1], np.int64)
    refused(-4, "256", C=257, cat=np.ones((257, V)), allowed=None)
    refused(-4, "4096", V=4097, cat=np.ones((C, 4097)))
    refused(-4, "4096", B=4097)
    assert rc_of(B=8)[0] == 0
    big = np.asarray([2 ** 30, 2 ** 30], np.int32)
    refused(-4, "2^31", D=1, dp=np.asarray([0, 2], np.int64), term=np.asarray([0, 1], np.int32), count=big, allowed=c.allowed[:1], qp=one, qt=[0], qm=[1], qg=[0])
    long = 4097
    refused(-4, "4096", D=1, dp=np.asarray([0, long], np.int64), term=np.arange(long, dtype=np.int32) % V, count=np.ones(long, np.int32), allowed=c.allowed[:1],
            qp=one, qt=[0], qm=[1], qg=[0])
    # ... an unqueried document may be that long
    assert rc_of(D=2, dp=np.asarray([0, long, long + 1], np.int64), term=np.arange(long + 1, dtype=np.int32) % V, count=np.ones(long + 1, np.int32),
                 allowed=c.allowed[:2], qp=np.asarray([0, 0, 1], np.int64), qt=[0], qm=[1], qg=[0])[0] == 0
    refused(-4, "group 1", D=1, dp=c.doc_ptr[:2], allowed=c.allowed[:1], qp=np.asarray([0, 2], np.int64), qt=[0, 1], qm=big, qg=[1, 1])
    with pytest.raises(mmm.MmmError, match="mmm_attribute_mutations"):
        mmm.attribute._raw(ctx, c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, c.q_ptr, c.q_term, maxiter=0)


def test_the_python_layer(mmm, monkeypatch):
    c = A.case(12, 96)
    raw = _run(mmm, c)
    X = A.as_X(c)
    Q = c.q_term.size
    doc = np.repeat(np.arange(c.D), np.diff(c.q_ptr))
    perm = np.random.default_rng(3).permutation(Q)
    queries = [(int(doc[i]), int(c.q_term[i]) + 1, int(c.q_mult[i])) for i in perm]
    labels = [None if c.q_group[i] < 0 else "gene%d" % c.q_group[i] for i in perm]
    names = ["S%d" % i for i in range(c.C)]
    kw = dict(queries=queries, groups=labels, allowed=c.allowed, B=c.B, seed=c.seed, maxiter=c.maxiter, tol=c.tol)
    r = mmm.attribute_mutations(X, (names, None, c.cat), **kw)
    # the Python layer draws with stream 0 (the stream of refit_exposures(bootstrap=B)): the raw call under that stream
    raw0 = _run(mmm, c._replace(stream=0))
    assert np.array_equal(r.posterior.view(np.uint8), raw["post"][perm].view(np.uint8)) and np.array_equal(r.exposures, raw["w"].T)
    assert np.array_equal(r.status, raw["status"]) and np.array_equal(r.iters, raw0["iters"]) and np.array_equal(r.void, raw0["void_count"][perm])
    assert np.array_equal(r.p_top, raw0["top_count"][perm] / c.B) and r.B == c.B and r.names == names and np.array_equal(r.queries, np.asarray(queries))
    n = c.B - raw0["void_count"][perm]
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(r.mean, np.where(n[:, None] > 0, raw0["sum_fx"][perm].astype(np.float64) / n[:, None] / A.FX_ONE, np.nan), equal_nan=True)
    x = raw0["rep_post"][:, perm]
    fx = np.floor(x * A.FX_ONE) / A.FX_ONE
    some = n == c.B
    assert np.allclose(r.sd[some], fx[:, some].std(axis=0, ddof=1), rtol=0, atol=1e-12) and some.any()
    top = np.where(raw["post"][perm].max(axis=1) > 0, raw["post"][perm].argmax(axis=1), -1)
    assert np.array_equal(r.top, top) and (top == -1).any()
    order = {g: i for i, g in enumerate(r.groups)}
    gid = np.asarray([-1 if g is None else order[g] for g in labels])
    assert sorted(r.groups) == ["gene0", "gene1", "gene2"]
    want = np.zeros((3, c.C))
    np.add.at(want, gid[gid >= 0], (np.floor(r.posterior * A.FX_ONE) * np.asarray([q[2] for q in queries])[:, None])[gid >= 0])
    assert np.array_equal(r.group_share, want / want.sum(axis=1, keepdims=True))
    relabel = np.asarray([int(g[4:]) for g in r.groups])
    gm, gq = mmm.attribute._group_summary(raw0["group_fx"][:, relabel], r.q)
    assert np.array_equal(r.group_mean, gm) and np.array_equal(r.group_quantiles, gq) and r.quantiles is None and r.replicates is None
    i = int(np.flatnonzero(top >= 0)[0])
    assert r.describe(i).startswith("sample %d, term %d: " % queries[i][:2]) and "%% S%d (sd " % r.top[i] in r.describe(i) and "replicates" in r.describe(i)
    header, rows = mmm.mutation_table(r)
    assert header[:7] == ["sample", "term", "mult", "top", "posterior", "sd", "p_top"] and header[7:] == names and len(rows) == Q and rows[0][7:] == r.posterior[0].tolist()
    # quantiles: samples in chunks within the host budget (here: one sample at a time), each reduced by mmm_replicate_summary
    monkeypatch.setattr(mmm.attribute, "REPLICATE_BYTES", 1)
    rq = mmm.attribute_mutations(X, (names, None, c.cat), quantiles=True, keep_replicates=True, **kw)
    for f in ("posterior", "mean", "sd", "p_top", "void", "exposures", "status", "group_share", "group_mean", "group_quantiles"):
        assert np.array_equal(getattr(rq, f), getattr(r, f), equal_nan=True), f
    assert np.array_equal(rq.replicates.view(np.uint8), x.view(np.uint8))
    assert np.array_equal(rq.quantiles, mmm.replicate_summary(x, r.q)[2]) and rq.quantiles.shape == (3, Q, c.C)
    assert "%% S%d [" % r.top[i] in rq.describe(i) and rq.describe(int(np.flatnonzero(top == -1)[0])).endswith("no allowed signature produces it")
    # more replicates than one call of the entry takes go through several calls whose sums add (here: 2 + 2 + 1)
    monkeypatch.setattr(mmm.attribute, "MAX_CALL_B", 2)
    rc = mmm.attribute_mutations(X, (names, None, c.cat), **kw)
    for f in ("posterior", "mean", "sd", "p_top", "void", "exposures", "status", "group_share", "group_mean", "group_quantiles"):
        assert np.array_equal(getattr(rc, f), getattr(r, f), equal_nan=True), f
    assert np.array_equal(rc.iters, r.iters + 2 * _run(mmm, c, B=0)["iters"])                 # the observed fit ran in each of the three calls
    monkeypatch.undo()
    # queries=None: every non-zero entry with its count; allowed=None: the chosen sets of the BIC refit; a RefitResult is taken as it is
    rr = mmm.refit_exposures(X, c.cat, "bic", allowed=None, maxiter=c.maxiter)
    a = mmm.attribute_mutations(X, c.cat, B=2, seed=5, maxiter=c.maxiter)
    b = mmm.attribute_mutations(X, c.cat, allowed=rr, B=2, seed=5, maxiter=c.maxiter)
    assert np.array_equal(a.posterior, b.posterior) and np.array_equal(a.mean, b.mean, equal_nan=True) and a.queries.shape[0] == int((c.count > 0).sum())
    assert np.array_equal(a.exposures[:, a.status == 0], rr.exposures[:, a.status == 0]) and not a.posterior[:, ~rr.active[:, 0]][a.queries[:, 0] == 0].any()
