"""mmm_exposure_trajectory on the device against its numpy restatement (tests/trajectory_ref.py): the weights, status, unexplained and iters bit
for bit at key_bits 32 and 3, wherever the catalogue is read from; the host's dynamic program and scan recomputed from the device's own
seg_ll bit for bit; seg_ll, gain_cut, stat and the kept replicates against a longdouble evaluation on the same mixtures within the bound
test_compare_gpu.py applies to ll-derived values; cut, n_cp, cp, count_ge and count_cut as integers (tests/test_trajectory_cpu.py asserts that
no deciding comparison of these cases is near a tie, and says why a sample with ONE allowed signature is left out); the shipped entries the
definition is composed of; chunks, runs and geometries; the Python layer; every error."""
import ctypes

import numpy as np
import pytest

import trajectory_ref as TR

pytestmark = pytest.mark.gpu

BITWISE = ("seg_ll", "best", "n_cp", "cp", "w_seg", "w_bin", "gain_cut", "cut", "stat", "count_ge", "count_cut", "status", "unexplained", "iters")
ALL = BITWISE + ("rep_stat",)


def _run(mmm, c, B=None, b0=0, keep=True, **kw):
    D, nbins, dp, term, count, bin_ptr = TR.csr(c)
    return mmm.trajectory._raw(mmm.default_context(), D, c.V, nbins, dp, term, count, bin_ptr, c.cat, c.allowed, c.L, c.M, c.penalty, c.B if B is None else B, b0,
                               c.seed, c.stream, c.maxiter, c.tol, keep=keep, **kw)


def _same(a, b, keys=ALL, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _within(got, ld, bound, what):
    """got against the longdouble values ld within bound, element by element; NaN must sit in the same places"""
    got, ld, bound = np.asarray(got).ravel(), np.asarray(ld).ravel(), np.asarray(bound).ravel()
    fin = np.isfinite(ld)
    assert np.array_equal(np.isnan(got), np.isnan(ld)) and np.isfinite(got[fin]).all(), what
    err = np.abs(got[fin] - ld[fin]).astype(np.float64)
    bad = np.flatnonzero(err > bound[fin])
    assert bad.size == 0, "%s: %d values beyond the bound, the first %r against %r (bound %g)" % (what, bad.size, got[fin][bad[0]], ld[fin][bad[0]], bound[fin][bad[0]])
    return float((err / np.maximum(bound[fin], 1e-300)).max()) if err.size and (bound[fin] > 0).any() else 0.0


def _host_part_from_the_table(c, got):
    """the dynamic program and the scan, recomputed from the device's own seg_ll: plain double arithmetic, so bit for bit"""
    D = len(c.bins)
    bin_ptr = np.concatenate([[0], np.cumsum([len(s) for s in c.bins])])
    seg0 = np.concatenate([[0], np.cumsum([len(s) * (len(s) + 1) // 2 for s in c.bins])])
    for d in range(D):
        T = len(c.bins[d])
        tab = got["seg_ll"][seg0[d]:seg0[d + 1]]
        if got["status"][d] == 3:
            assert np.isnan(tab).all() and np.isnan(got["best"][d]).all() and got["n_cp"][d] == 0 and (got["cp"][d] == -1).all() and got["cut"][d] == -1
            assert (got["w_seg"][d] == 0).all() and got["stat"][d] == 0 and got["iters"][d] == 0 and got["unexplained"][d] == 0
            assert np.isnan(got["gain_cut"][bin_ptr[d]:bin_ptr[d + 1]]).all() and (got["count_cut"][bin_ptr[d]:bin_ptr[d + 1]] == 0).all()
            assert (got["w_bin"][bin_ptr[d]:bin_ptr[d + 1]] == 0).all()
            continue
        best, n_cp, cp = TR.partition(tab, T, c.L, c.M, c.penalty[d])
        assert np.array_equal(best.view(np.uint8), got["best"][d].view(np.uint8)) and n_cp == got["n_cp"][d] and np.array_equal(cp, got["cp"][d]), d
        assert (got["w_seg"][d, n_cp + 1:] == 0).all()
        gain = np.full(T, np.nan)
        cuts = list(range(c.L, T - c.L + 1))
        ll = lambda i, j: float(tab[TR.seg_index(T, i, j)])
        G = {t: ll(0, t) + ll(t, T) for t in cuts}
        for t in cuts:
            gain[t] = G[t] - ll(0, T)
        assert np.array_equal(gain.view(np.uint8), got["gain_cut"][bin_ptr[d]:bin_ptr[d + 1]].view(np.uint8)), d
        if cuts:
            gmax = max(G.values())
            assert got["status"][d] == 0 and got["cut"][d] == min(t for t in cuts if G[t] == gmax) and got["stat"][d] == max(2.0 * (gmax - ll(0, T)), 0.0)
        else:
            assert got["status"][d] == 1 and got["cut"][d] == -1 and got["stat"][d] == 0 and got["count_ge"][d] == 0


def _against_reference(c, got, key_bits):
    ref = TR.reference(c.name, key_bits)
    D = len(c.bins)
    want = dict(w_seg=ref.w_seg, w_bin=ref.w_bin, status=ref.status, unexplained=ref.unexplained, iters=ref.iters)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if k == "w_bin":
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
            continue
        bad = np.flatnonzero((got[k].reshape(D, -1).view(np.uint8) != want[k].reshape(D, -1).view(np.uint8)).any(axis=1))
        assert bad.size == 0, "%s: %s differs in samples %s" % (c.name, k, bad.tolist())
    _host_part_from_the_table(c, got)
    worst = _within(got["seg_ll"], ref.seg_ld, ref.seg_bd, c.name + " seg_ll")
    worst = max(worst, _within(got["gain_cut"], ref.gain_ld, ref.gain_bd, c.name + " gain_cut"))
    worst = max(worst, _within(got["stat"], ref.stat_ld, ref.stat_bd, c.name + " stat"))
    worst = max(worst, _within(got["rep_stat"], ref.rep_ld, ref.rep_bd, c.name + " replicates"))
    print("%s key_bits %d: largest error / bound of seg_ll, gain_cut, stat and rep_stat = %.3f" % (c.name, key_bits, worst))
    cmp = ref.n_allowed != 1           # one allowed signature: every partition has the same likelihood up to rounding (tests/test_trajectory_cpu.py)
    for k in ("cut", "n_cp", "count_ge"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k][cmp], getattr(ref, k)[cmp]), (k, got[k], getattr(ref, k))
    assert np.array_equal(got["cp"][cmp], ref.cp[cmp])
    on = np.repeat(cmp, np.diff(ref.bin_ptr))
    assert got["count_cut"].dtype == np.int32 and np.array_equal(got["count_cut"][on], ref.count_cut[on])
    assert (got["count_ge"] >= 0).all() and (got["count_ge"] <= c.B).all() and (got["count_cut"] >= 0).all() and (got["count_cut"] <= c.B).all()
    assert (got["count_cut"][np.isnan(got["gain_cut"])] == 0).all()
    assert np.array_equal(np.isnan(got["rep_stat"]), np.tile(ref.status != 0, (c.B, 1)))


@pytest.mark.parametrize("name,key_bits", TR.RUNS, ids=["%s-%d" % r for r in TR.RUNS])
def test_outputs_equal_the_restatement_wherever_the_catalogue_is_read_from(mmm, name, key_bits):
    c = TR.case(name)
    got = _run(mmm, c, key_bits=key_bits)
    _against_reference(c, got, key_bits)
    l2 = _run(mmm, c, key_bits=key_bits, catalogue_in_lds=False)
    _same(got, l2, what="LDS against L2")
    assert mmm.default_context().get_tuning().disable == 0                # the hook is undone


def test_chunked_calls_add_and_runs_and_geometries_give_equal_bits(mmm, tuning):
    c = TR.case("V64")
    B, cut = c.B, 7
    whole, again = _run(mmm, c), _run(mmm, c)
    _same(whole, again, what="two runs")
    a, b, obs = _run(mmm, c, B=cut), _run(mmm, c, B=B - cut, b0=cut), _run(mmm, c, B=0)
    fixed = tuple(k for k in BITWISE if k not in ("count_ge", "count_cut", "iters"))
    _same(whole, a, keys=fixed, what="first chunk"); _same(whole, b, keys=fixed, what="second chunk"); _same(whole, obs, keys=fixed, what="B = 0")
    for k in ("count_ge", "count_cut"):
        assert np.array_equal(whole[k], a[k] + b[k]), k
        assert (obs[k] == 0).all(), k
    assert np.array_equal(whole["iters"], a["iters"] + b["iters"] - obs["iters"])
    assert np.array_equal(np.concatenate([a["rep_stat"], b["rep_stat"]]).view(np.uint8), whole["rep_stat"].view(np.uint8))
    assert obs["rep_stat"].shape == (0, len(c.bins))
    _same(whole, _run(mmm, c, keep=False), keys=BITWISE, what="keep=False")
    nobins = _run(mmm, c, bins=False)
    _same(whole, nobins, keys=tuple(k for k in ALL if k != "w_bin"), what="w_bin = NULL")
    v7 = TR.case("V7")
    full = _run(mmm, v7, B=4)
    ones = _run(mmm, v7._replace(allowed=np.ones((len(v7.bins), v7.C), dtype=np.uint8)), B=4)
    _same(full, ones, what="allowed = NULL")
    for cus in (3, 1):
        tuning(geometry_cus=cus)
        _same(whole, _run(mmm, c), what="geometry_cus = %d" % cus)
        tuning()
    big = TR.case("V65")
    ref = _run(mmm, big, key_bits=3)
    tuning(geometry_cus=3)
    _same(ref, _run(mmm, big, key_bits=3), what="geometry_cus = 3, key_bits = 3")


def _as_X(rows):
    return [np.stack([np.flatnonzero(n) + 1, n[np.flatnonzero(n)]], axis=1).astype(np.int64) for n in rows]


def test_the_weights_are_the_shipped_refit_and_the_replicates_the_shipped_dealing(mmm):
    """w_bin and w_seg are refit_exposures(penalty=None) of the summed tables, bit for bit.  Every kept replicate of one sample against the
    composition of the public entries: deal_counts on the pooled table with n_a = C_t under the same seed and stream for every cut, two plain
    refits of the stacked prefixes and suffixes, the maximum over the cuts and the pooled refit; the two values hold the same sums and
    differ by the rounding bound at most."""
    c = TR.case("V64")
    ctx = mmm.default_context()
    ref = TR.reference("V64")
    got = _run(mmm, c)
    D, C, V, B = len(c.bins), c.C, c.V, c.B
    dense = [TR.dense_bins(c, d) for d in range(D)]

    def plain(rows, allowed):
        rows = np.asarray(rows, dtype=np.int64)
        n = rows.shape[0]
        return mmm.refit._raw(ctx, n, V, np.arange(n + 1, dtype=np.int64) * V, np.tile(np.arange(V, dtype=np.int32), n), rows.ravel(), c.cat, allowed, None, c.maxiter, c.tol)

    allb = np.concatenate(dense)
    alb = np.repeat(c.allowed, [len(s) for s in c.bins], axis=0)
    live = np.repeat(got["status"] != 3, [len(s) for s in c.bins])
    fb = plain(allb, alb)
    assert np.array_equal(fb["w"][live].view(np.uint8), got["w_bin"][live].view(np.uint8)) and (got["w_bin"][~live] == 0).all()
    segs, sal, where = [], [], []
    for d in range(D):
        if got["status"][d] == 3:
            continue
        k = int(got["n_cp"][d])
        b = [0] + got["cp"][d, :k].tolist() + [len(c.bins[d])]
        for j in range(k + 1):
            segs.append(dense[d][b[j]:b[j + 1]].sum(axis=0)); sal.append(c.allowed[d]); where.append((d, j))
    fs = plain(segs, np.stack(sal))
    for i, (d, j) in enumerate(where):
        assert np.array_equal(fs["w"][i].view(np.uint8), got["w_seg"][d, j].view(np.uint8)), (d, j)
    assert sum(int(got["n_cp"][d]) for d in range(D)) >= 3
    # the replicates of sample 1 (T = 5, L = 2: the cuts 2 and 3)
    d = 1
    assert got["status"][d] == 0
    pooled = np.stack([x.sum(axis=0) for x in dense])
    cuts = list(range(c.L, len(c.bins[d]) - c.L + 1))
    G = []
    for t in cuts:
        n_a = np.zeros(D, dtype=np.int64); n_a[d] = ref.C_t[d][t]
        dealt = mmm.deal_counts(_as_X(pooled), n_a, B, seed=c.seed, stream=c.stream, V=V)[:, d]        # [B, V]
        assert all(np.array_equal(dealt[b], ref.prefixes[(d, b)][t]) for b in range(B))
        al = np.tile(c.allowed[d], (B, 1))
        fa, fz = plain(dealt, al), plain(pooled[d][None] - dealt, al)
        G.append(fa["ll_doc"] + fz["ll_doc"])
    f0 = plain(pooled[d][None], c.allowed[d][None])
    assert np.array_equal(f0["unexplained"], got["unexplained"][d:d + 1])
    lam = 2.0 * (np.max(G, axis=0) - f0["ll_doc"][0])
    assert (np.abs(got["rep_stat"][:, d] - lam) <= 2 * ref.rep_bd[:, d]).all()


def test_the_python_layer_edges_and_the_change_point_tests(mmm):
    c = TR.case("V64")
    D, B, C = len(c.bins), 12, c.C
    names = ["S%d" % i for i in range(C)]
    tl = [[np.stack([np.asarray(t, np.int64) + 1, np.asarray(n, np.int64)], axis=1) for t, n in s] for s in c.bins]
    kw = dict(allowed=c.allowed, min_len=c.L, max_changepoints=c.M, B=B, seed=c.seed, stream=c.stream, maxiter=c.maxiter, tol=c.tol)
    r = mmm.exposure_trajectory(tl, (names, None, c.cat), penalty=c.penalty, keep_replicates=True, **kw)
    raw = _run(mmm, c, B=B)
    assert r.names == names and r.B == B and r.p.shape == (D,) and r.replicates.shape == (B, D) and r.best.shape == (D, c.M + 1)
    for f, k in (("stat", "stat"), ("cut", "cut"), ("count_ge", "count_ge"), ("status", "status"), ("unexplained", "unexplained"), ("iters", "iters"),
                 ("n_changepoints", "n_cp"), ("changepoints", "cp"), ("best", "best"), ("seg_ll", "seg_ll")):
        assert np.array_equal(getattr(r, f).view(np.uint8), raw[k].view(np.uint8)), f
    assert np.array_equal(r.replicates, raw["rep_stat"], equal_nan=True)
    bp = r.bin_ptr
    for d in range(D):
        s = slice(bp[d], bp[d + 1])
        assert np.array_equal(r.exposures_bin[d], raw["w_bin"][s]) and np.array_equal(r.gain[d], raw["gain_cut"][s], equal_nan=True)
        assert np.array_equal(r.exposures_segment[d], raw["w_seg"][d, :raw["n_cp"][d] + 1]) and np.array_equal(r.count_cut[d], raw["count_cut"][s])
        on = ~np.isnan(raw["gain_cut"][s])
        assert np.array_equal(r.p_cut[d][on], (1.0 + raw["count_cut"][s][on]) / (B + 1.0)) and np.isnan(r.p_cut[d][~on]).all()
        segs = r.segments(d)
        assert len(segs) == (0 if r.status[d] == 3 else r.n_changepoints[d] + 1)
        if segs:
            assert segs[0][0] == 0 and segs[-1][1] == bp[d + 1] - bp[d] and all(a[1] == b[0] for a, b in zip(segs[:-1], segs[1:]))
    assert r.status.tolist() == [1, 0, 0, 1, 3, 0]
    un = r.status != 0
    assert np.isnan(r.p[un]).all() and np.array_equal(r.p[~un], (1.0 + r.count_ge[~un]) / (B + 1.0)) and np.isnan(r.q[un]).all() and np.isfinite(r.q[~un]).all()
    assert set(r.changed(1.0)) == set(np.flatnonzero(~un))
    # the "bic" penalty is the one the case table uses: 0.5 (|A| + 1) log N
    rb = mmm.exposure_trajectory(tl, c.cat, penalty="bic", changepoint_tests=False, **kw)
    live = r.status != 3
    assert np.array_equal(rb.n_changepoints[live], r.n_changepoints[live]) and np.array_equal(rb.changepoints[live], r.changepoints[live]) and rb.names is None
    assert np.isnan(rb.p_changepoint).all()
    # p_changepoint: a direct call on the hand-built windows, stacked in the order (sample, k)
    windows, wal, where = [], [], []
    for d in range(D):
        k = int(r.n_changepoints[d])
        b = [0] + r.changepoints[d, :k].tolist() + [bp[d + 1] - bp[d]]
        for j in range(k):
            windows.append(tl[d][b[j]:b[j + 2]]); wal.append(c.allowed[d]); where.append((d, j))
    assert len(windows) >= 3
    w = mmm.exposure_trajectory(windows, c.cat, penalty=0.0, changepoint_tests=False, **dict(kw, allowed=np.stack(wal), max_changepoints=0))
    want = np.full((D, c.M), np.nan)
    for i, (d, j) in enumerate(where):
        want[d, j] = w.p[i]
    assert np.array_equal(r.p_changepoint, want, equal_nan=True) and np.isfinite(w.p).all()
    # B = 0: the observed part only; a dense timeline; a RefitResult as `allowed`
    r0 = mmm.exposure_trajectory(tl, c.cat, penalty=c.penalty, **dict(kw, B=0))
    assert np.isnan(r0.p).all() and np.array_equal(r0.stat, r.stat) and np.array_equal(r0.changepoints, r.changepoints) and r0.replicates is None
    assert np.isnan(r0.p_changepoint).all() and (r0.count_ge == 0).all()
    none = mmm.exposure_trajectory([[], []], c.cat, B=3, seed=1)                             # no bins at all: the entry writes nothing, every sample untestable
    assert none.status.tolist() == [3, 3] and np.isnan(none.p).all() and np.isnan(none.best).all() and (none.cut == -1).all() and none.segments(0) == []
    dense = np.stack([TR.dense_bins(c, d) for d in (1, 5)])
    x = mmm.exposure_trajectory(dense, c.cat, allowed=c.allowed[[1, 5]], min_len=c.L, max_changepoints=c.M, penalty=c.penalty[[1, 5]], B=0, maxiter=c.maxiter)
    assert np.array_equal(x.changepoints, r.changepoints[[1, 5]]) and np.array_equal(x.stat, r.stat[[1, 5]])
    pooled = [np.concatenate(s) for s in tl]
    rr = mmm.refit_exposures(pooled, c.cat, maxiter=c.maxiter)
    y = mmm.exposure_trajectory(tl, c.cat, allowed=rr, B=4, seed=1, maxiter=c.maxiter, min_len=c.L, changepoint_tests=False)
    z = mmm.exposure_trajectory(tl, c.cat, allowed=rr.active.T, B=4, seed=1, maxiter=c.maxiter, min_len=c.L, changepoint_tests=False)
    assert np.array_equal(y.stat, z.stat) and np.array_equal(y.count_ge, z.count_ge) and all(np.array_equal(a, b) for a, b in zip(y.exposures_segment, z.exposures_segment))
    assert all(((e > 0) <= rr.active[:, d][None, :]).all() for d, e in enumerate(y.exposures_bin))


def test_every_error_and_the_degenerate_calls(mmm):
    c = TR.case("V7")
    L_, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, ci, ctypes.c_double,
                             *([vp] * 15))(("mmm_exposure_trajectory", L_))
    D0, nb0, dp0, term0, count0, bp0 = TR.csr(c)
    C, V = c.C, c.V
    OUT = ("seg_ll", "best", "n_cp", "cp", "w_seg", "w_bin", "gain_cut", "cut", "stat", "count_ge", "count_cut", "status", "unexplained", "iters", "rep")

    def rc_of(D=D0, C=C, V=V, nbins=nb0, dp=dp0, term=term0, count=count0, bp=bp0, cat=c.cat, allowed=None, L=1, M=2, pen=c.penalty, B=3, b0=0, stream=0,
              key_bits=32, maxiter=5, tol=0.0, null=None, rows=None):
        n, m, nb = rows or max(D, 1), max(C, 1), max(nbins, 1)
        S = max(int(sum(t * (t + 1) // 2 for t in np.diff(np.asarray(bp)[:n + 1]))), 1) if rows is None else 1
        out = dict(seg_ll=np.full(S, 7.0), best=np.full((n, M + 1), 7.0), n_cp=np.full(n, 7, np.int32), cp=np.full((n, max(M, 1)), 7, np.int32),
                   w_seg=np.full((n, M + 1, m), 7.0), w_bin=np.full((nb, m), 7.0), gain_cut=np.full(nb, 7.0), cut=np.full(n, 7, np.int32), stat=np.full(n, 7.0),
                   count_ge=np.full(n, 7, np.int32), count_cut=np.full(nb, 7, np.int32), status=np.full(n, 7, np.int8), unexplained=np.full(n, 7.0),
                   iters=np.full(n, 7, np.int64), rep=np.full((max(B, 1), n), 7.0))
        names = ("dp", "term", "count", "bp", "cat", "allowed", "pen")
        keep = [np.ascontiguousarray(dp, dtype=np.int64), np.ascontiguousarray(term, dtype=np.int32), np.ascontiguousarray(count, dtype=np.int32),
                np.ascontiguousarray(bp, dtype=np.int64), np.ascontiguousarray(cat, dtype=np.float64),
                None if allowed is None else np.ascontiguousarray(allowed, dtype=np.uint8), np.ascontiguousarray(pen, dtype=np.float64)]
        p = {k: (None if a is None or k == null else a.ctypes.data) for k, a in zip(names, keep)}
        o = {k: (None if k == null else a.ctypes.data) for k, a in out.items()}
        rc = plain(ctx.h, D, C, V, nbins, p["dp"], p["term"], p["count"], p["bp"], p["cat"], p["allowed"], L, M, p["pen"], B, b0, 9, stream, key_bits, maxiter, tol,
                   *[o[k] for k in OUT])
        untouched = all((a == 7).all() for a in out.values())
        return rc, (L_.mmm_last_error(ctx.h) or b"").decode(), untouched

    rc, _, untouched = rc_of()
    assert rc == 0 and not untouched
    assert rc_of(allowed=np.ones((D0, C), np.uint8))[0] == 0 and rc_of(B=0)[0] == 0 and rc_of(null="rep")[0] == 0 and rc_of(null="w_bin")[0] == 0
    assert rc_of(key_bits=1)[0] == 0 and rc_of(M=0, null="cp")[0] == 0 and rc_of(L=3)[0] == 0
    rc, _, untouched = rc_of(D=0, nbins=0, dp=np.zeros(1, np.int64), bp=np.zeros(1, np.int64))
    assert rc == 0 and untouched                                                           # D = 0 writes nothing
    rc, _, untouched = rc_of(D=2, nbins=0, dp=np.zeros(1, np.int64), bp=np.zeros(3, np.int64), pen=np.ones(2))
    assert rc == 0 and untouched                                                           # nbins = 0 writes nothing
    assert plain(None, *([0] * 35)) == -1

    def refused(code, needle=None, **kw):
        rc, msg, untouched = rc_of(**kw)
        assert rc == code and untouched and (needle is None or needle in msg), (sorted(kw), rc, msg, untouched)

    for null in ("cat", "dp", "term", "count", "bp", "pen") + tuple(k for k in OUT if k not in ("rep", "w_bin")):
        refused(-1, null=null)
    refused(-1, "key_bits", key_bits=0); refused(-1, "key_bits", key_bits=33)
    refused(-1, B=-1); refused(-1, b0=-1); refused(-1, "2^31 - 1", B=3, b0=2 ** 31 - 3)
    assert rc_of(B=3, b0=2 ** 31 - 4)[0] == 0
    refused(-1, "stream", stream=2 ** 31)
    assert rc_of(stream=2 ** 31 - 1)[0] == 0
    refused(-1, maxiter=0); refused(-1, tol=-1e-12); refused(-1, C=0); refused(-1, V=0); refused(-1, D=-1); refused(-1, nbins=-1)
    refused(-1, "min_len", L=0); refused(-1, "max_cp", M=-1)
    for bad in (-1e-3, np.nan, np.inf):
        pen = c.penalty.copy(); pen[2] = bad
        refused(-1, "penalty[2]", pen=pen)
        cat = c.cat.copy(); cat[1, 3] = bad
        refused(-1, "catalogue entry (1, 3)", cat=cat)
    cat = c.cat.copy(); cat[1] = 0.0
    refused(-1, "row 1", cat=cat)
    bp = bp0.copy(); bp[0] = 1
    refused(-1, "bin_ptr", bp=bp)
    bp = bp0.copy(); bp[2] = bp[1] - 1
    refused(-1, "bin_ptr decreases", bp=bp)
    bp = bp0.copy(); bp[-1] -= 1
    refused(-1, "nbins", bp=bp)
    term = term0.copy(); term[2] = V
    refused(-1, term=term)
    count = count0.copy(); count[1] = -1
    refused(-1, count=count)
    dp = dp0.copy(); dp[0] = 1
    refused(-1, dp=dp)
    refused(-4, "256", C=257, cat=np.ones((257, V)))
    refused(-4, "4096", V=4097, cat=np.ones((C, 4097)))
    refused(-4, "2^28", D=2 ** 28 + 1, rows=1)                                             # refused before an array is read
    T = 129
    refused(-4, "limit 128", D=1, nbins=T, dp=np.arange(T + 1), term=np.zeros(T, np.int32), count=np.ones(T, np.int32), bp=np.asarray([0, T]), pen=np.ones(1))
    assert rc_of(D=1, nbins=128, dp=np.arange(129), term=np.zeros(128, np.int32), count=np.ones(128, np.int32), bp=np.asarray([0, 128]), pen=np.ones(1), M=0, B=1)[0] == 0
    big = np.asarray([2 ** 30, 2 ** 30], np.int32)
    refused(-4, "2^31", D=1, nbins=2, dp=np.asarray([0, 1, 2]), term=np.zeros(2, np.int32), count=big, bp=np.asarray([0, 2]), pen=np.ones(1))
    refused(-4, "2^31", D=1, nbins=1, dp=np.asarray([0, 2]), term=np.asarray([0, 1], np.int32), count=big, bp=np.asarray([0, 1]), pen=np.ones(1))
    with pytest.raises(mmm.MmmError, match="mmm_exposure_trajectory"):
        _run(mmm, c._replace(maxiter=0), B=2)
