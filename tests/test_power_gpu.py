"""mmm_presence_power on the device against its float64 restatement (tests/power_ref.py): the observed phase, count_zero and iters bit for
bit / integer for integer; count_reject as an integer (tests/test_power_cpu.py asserts that no comparison of these cases is near a tie);
crit and the kept Λ against a longdouble evaluation on the same mixtures within 2 (bound(ll0) + bound(ll1)); the shipped entries the
definition is composed of, device to device; launch geometries; chunked calls; every status; every error."""
import ctypes

import numpy as np
import pytest

import power_ref as W
import presence_ref as PR
import refit_ref as R

pytestmark = pytest.mark.gpu

G = len(W.FRACTIONS)
G1 = G + 1
KEYS = ("w_null", "stat", "score", "w_alt", "status", "iters", "crit", "count_reject", "count_zero", "rep_stat")


def _n_level(c):
    return W.n_levels(c, PR.presence(c, B=0))


def _run(mmm, c, B, alpha, b0=0, crit=None, keep=True, n_level="two", fractions=W.FRACTIONS, seed=None):
    return mmm.power._raw(mmm.default_context(), c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, c.targets, fractions, _n_level(c) if isinstance(n_level, str) else n_level,
                          alpha, c.allowed, B, b0, W.SEEDS.get(c.name, c.seed) if seed is None else seed, c.stream, crit, c.maxiter, c.tol, keep=keep)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _same(a, b, keys=KEYS, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _within(got, ld, bound, what):
    """got against the longdouble values ld within bound, element by element; inf and NaN must sit in the same places"""
    got, ld, bound = np.asarray(got).ravel(), np.asarray(ld).ravel(), np.asarray(bound).ravel()
    fin = np.isfinite(ld)
    assert np.array_equal(np.isnan(got), np.isnan(ld)) and np.array_equal(got[~fin & ~np.isnan(ld)], ld[~fin & ~np.isnan(ld)]), what
    err = np.abs(got[fin] - ld[fin])
    bad = np.flatnonzero(err > bound[fin])
    assert bad.size == 0, "%s: %d values beyond the bound, the first %r against %r (bound %g)" % (what, bad.size, got[fin][bad[0]], ld[fin][bad[0]], bound[fin][bad[0]])


@pytest.mark.parametrize("i", range(len(W.SHAPES) + 1), ids=lambda i: W.corpora()[i].name)
def test_outputs_equal_the_restatement(mmm, i):
    c = W.corpora()[i]
    lv = W.reference_levels(i)
    obs = lv.obs
    live = obs.status != 3
    for B, alpha in W.CASES:
        ref = W.power(lv, G, alpha, B=B)
        got = _run(mmm, c, B, alpha)
        what = "%s B=%d α=%g" % (c.name, B, alpha)
        for k, want in (("w_null", obs.w_null), ("score", obs.score), ("w_alt", obs.w_alt), ("status", obs.status), ("count_zero", ref.count_zero),
                        ("iters", ref.iters), ("count_reject", ref.count_reject)):
            assert got[k].dtype == want.dtype and got[k].shape == want.shape and np.array_equal(_bits(got[k]), _bits(want)), (what, k)
        _within(got["stat"], obs.stat_ld, obs.bound, what + " stat")
        _within(got["rep_stat"], ref.rep_ld, ref.rep_bound, what + " replicates")
        # the branch of every replicate: Λ is 0 exactly where fit(A1) was skipped or clamped, in the same places
        assert np.array_equal(got["rep_stat"] == 0, ref.rep == 0)
        # crit: the element of the null replicates the restatement selects (no tie: the same element), within that element's bound
        for h in range(2):
            null = ref.rep[h * G1]
            for j in np.flatnonzero(live):
                b = np.argsort(-null[:, j], kind="stable")[ref.m]
                assert got["crit"][h, j] == got["rep_stat"][h * G1, b, j], (what, h, j)
                _within(got["crit"][h, j], ref.rep_ld[h * G1, b, j], ref.rep_bound[h * G1, b, j], what + " crit")
        assert (got["crit"][:, ~live] == 0).all() and np.isnan(got["rep_stat"][:, :, ~live]).all()
        assert (got["count_reject"][0::G1] <= max(ref.m, 0)).all()


def test_level_zero_is_the_presence_test_and_a_level_is_the_shipped_draw_refitted(mmm):
    """Device to device.  The kept level-0 statistics at the observed totals equal mmm_presence_test's rep_stat under the same seed and
    stream bit for bit.  For the level (total 50, φ = 0.07): simulate_counts(w^l, P, N^h) on the L T D-document layout, fed back as a corpus
    into mmm_presence_test with B = 0, gives the kept Λ^l_b bit for bit."""
    c = PR.corpus(12, 96)
    ctx = mmm.default_context()
    B, alpha = 24, 0.2
    seed = W.SEEDS[c.name]
    got = _run(mmm, c, B, alpha)
    D, C, V, T = c.D, c.C, c.V, len(c.targets)
    TD = T * D
    pres = mmm.presence._raw(ctx, D, V, c.doc_ptr, c.term, c.count, c.cat, c.targets, c.allowed, B, 0, seed, c.stream, c.maxiter, c.tol, keep=True)
    tested = pres["status"] == 0
    assert tested.any() and np.array_equal(_bits(pres["rep_stat"][:, tested]), _bits(got["rep_stat"][0][:, tested]))
    _same(pres, got, keys=("w_null", "stat", "score", "w_alt", "status"), what="observed phase")
    # one alternative level through the shipped entries
    h, g = 1, 1
    lvl = h * G1 + g
    L = 2 * G1
    live = got["status"] != 3
    P = R.normalise(c.cat)
    props = np.zeros((L * TD, C)); n_doc = np.zeros(L * TD, dtype=np.int64)
    for j in np.flatnonzero(live):
        props[lvl * TD + j] = W.level_weights(got["w_null"][j], int(c.targets[j // D]), W.FRACTIONS[g - 1])
        n_doc[lvl * TD + j] = W.FIXED_TOTAL
    props[n_doc == 0, 0] = 1.0                                # the documents of the layout that are not drawn here
    sim = mmm.simulate_counts(props.T, P.T, n_doc, B=B, seed=seed, stream=c.stream, ctx=ctx)[:, lvl * TD:(lvl + 1) * TD, :]          # [B, TD, V]
    assert np.array_equal(sim.sum(axis=2)[:, live], np.full((B, live.sum()), W.FIXED_TOTAL))
    dp = np.arange(B * D + 1, dtype=np.int64) * V
    term = np.tile(np.arange(V, dtype=np.int32), B * D)
    for ti in range(T):
        counts = np.ascontiguousarray(sim[:, ti * D:(ti + 1) * D, :].reshape(B * D, V), dtype=np.int32)
        fed = mmm.presence._raw(ctx, B * D, V, dp, term, counts.ravel(), c.cat, c.targets[ti:ti + 1], np.tile(c.allowed, (B, 1)), 0, 0, 0, 0, c.maxiter, c.tol)
        want = got["rep_stat"][lvl][:, ti * D:(ti + 1) * D]
        ok = live[ti * D:(ti + 1) * D]
        assert ok.any() and np.array_equal(_bits(fed["stat"].reshape(B, D)[:, ok]), _bits(want[:, ok])), ti


@pytest.mark.parametrize("shape", [(40, 96), (6, 1536)], ids=lambda s: "C%dV%d" % s)
def test_launch_geometry_and_the_place_of_the_catalogue_cannot_change_a_bit(mmm, tuning, shape):
    c = PR.corpus(*shape)
    B, alpha = 12, 0.2                                         # m = 1
    base = _run(mmm, c, B, alpha)
    assert (base["status"] != 3).all() and np.isfinite(base["crit"]).all()
    if shape == (6, 1536):        # the shape at which only the two-row items fit LDS beside four waves' buffers: staged and direct items in one call
        n1 = [PR.sets(c, j)[3].size for j in range(base["status"].size)]
        assert min(n1) <= 2 < max(n1), n1
    tuning(geometry_cus=1)
    _same(base, _run(mmm, c, B, alpha), what="one CU")
    tuning(disable=("refit_lds",))
    _same(base, _run(mmm, c, B, alpha), what="catalogue through L2")
    tuning()
    _same(base, _run(mmm, c, B, alpha), what="defaults again")


def test_chunked_calls_add_with_crit_given_and_two_runs_give_equal_bits(mmm):
    c = PR.corpus(12, 96)
    B, cut, alpha = 24, 7, 0.2
    whole, again = _run(mmm, c, B, alpha), _run(mmm, c, B, alpha)
    _same(whole, again, what="two runs")
    crit = whole["crit"]
    full = _run(mmm, c, B, alpha, crit=crit)
    a, b = _run(mmm, c, cut, alpha, crit=crit), _run(mmm, c, B - cut, alpha, b0=cut, crit=crit)
    obs = _run(mmm, c, 0, alpha, crit=crit)
    for k in ("w_null", "stat", "score", "w_alt", "status", "crit"):
        for r, what in ((full, "crit given"), (a, "first chunk"), (b, "second chunk"), (obs, "B = 0")):
            _same(whole, r, keys=(k,), what=what)
    assert np.array_equal(full["count_reject"], a["count_reject"] + b["count_reject"]) and np.array_equal(full["count_zero"], a["count_zero"] + b["count_zero"])
    assert np.array_equal(full["iters"], a["iters"] + b["iters"] - obs["iters"])
    assert (obs["count_reject"] == 0).all() and (obs["count_zero"] == 0).all() and obs["rep_stat"].shape == (2 * G1, 0, whole["status"].size)
    # the null levels are not run; every other level is what the call that selected crit itself gives
    assert (full["count_reject"][0::G1] == 0).all() and (full["count_zero"][0::G1] == 0).all() and np.isnan(full["rep_stat"][0::G1]).all()
    alt = np.arange(2 * G1) % G1 != 0
    assert np.array_equal(full["count_reject"][alt], whole["count_reject"][alt]) and np.array_equal(full["count_zero"][alt], whole["count_zero"][alt])
    assert np.array_equal(_bits(np.concatenate([a["rep_stat"], b["rep_stat"]], axis=1)[alt]), _bits(whole["rep_stat"][alt]))
    extra = whole["iters"] - full["iters"]                    # the fits of the null levels: some for every testable item
    assert (extra >= 0).all() and np.array_equal(extra > 0, whole["status"] != 3)
    # without the replicate buffer: the same counts; the observed totals alone (n_level = NULL) are the first total of the pair
    _same(whole, _run(mmm, c, B, alpha, keep=False), keys=KEYS[:-1], what="keep=False")
    one = _run(mmm, c, B, alpha, n_level=None)
    for k in ("crit", "count_reject", "count_zero", "rep_stat"):
        assert np.array_equal(_bits(one[k]), _bits(whole[k][:len(one[k])])), k


def _as_X(c):
    return [np.stack([c.term[a:b].astype(np.int64) + 1, c.count[a:b].astype(np.int64)], axis=1) for a, b in zip(c.doc_ptr[:-1], c.doc_ptr[1:])]


def test_every_status_through_the_python_layer(mmm):
    """the edge corpus of the presence test: untestable pairs give NaN power and nothing else; pairs with Λ_obs = 0 and Λ_obs = +inf get power
    like any other; φ = 1 (every draw from the target) and a total of one mutation"""
    c = PR.edge_corpus()
    D, B, alpha, T = c.D, 12, 0.2, 3
    names = ["S%d" % i for i in range(c.C)]
    fr = (0.07, 1.0)
    r = mmm.presence_power(_as_X(c), (names, None, c.cat), ["S5", "S1", "S2"], fractions=fr, n_mutations=[1, 50], alpha=alpha, allowed=c.allowed, B=B, seed=c.seed,
                           stream=c.stream, maxiter=c.maxiter, tol=c.tol, keep_replicates=True)
    raw = _run(mmm, c, B, alpha, n_level=np.repeat(np.asarray([[1], [50]], dtype=np.int32), D, axis=1), fractions=fr, seed=c.seed)
    assert r.names == ["S5", "S1", "S2"] and r.B == B and r.alpha == alpha and np.array_equal(r.fractions, fr) and np.array_equal(r.n_mutations, np.repeat([[1], [50]], D, axis=1))
    assert r.power.shape == (2, 2, T, D) and r.size.shape == r.crit.shape == (2, T, D) and r.count_zero.shape == (2, 3, T, D) and r.replicates.shape == (2, 3, B, T, D)
    cr = raw["count_reject"].reshape(2, 3, T, D)
    assert np.array_equal(r.count_reject, cr[:, 1:]) and np.array_equal(r.count_zero.ravel(), raw["count_zero"].ravel()) and np.array_equal(r.crit.ravel(), raw["crit"].ravel())
    assert np.array_equal(r.replicates.ravel(), raw["rep_stat"].ravel(), equal_nan=True) and np.array_equal(r.status.ravel(), raw["status"])
    assert np.array_equal(r.exposures_null.transpose(0, 2, 1).reshape(T * D, c.C), raw["w_null"]) and np.array_equal(r.iters.ravel(), raw["iters"])
    ref = PR.reference(c)
    st = r.status
    assert np.array_equal(st.ravel(), ref.status) and set(np.unique(st)) == {0, 1, 2, 3}
    dead = st == 3
    assert np.isnan(r.power[:, :, dead]).all() and np.isnan(r.size[:, dead]).all() and np.isnan(r.replicates[:, :, :, dead]).all()
    assert (r.crit[:, dead] == 0).all() and (r.count_reject[:, :, dead] == 0).all() and (r.count_zero[:, :, dead] == 0).all() and (r.iters[dead] == 0).all()
    assert np.array_equal(r.power[:, :, ~dead], r.count_reject[:, :, ~dead] / float(B)) and np.array_equal(r.size[:, ~dead], cr[:, 0][:, ~dead] / float(B))
    assert not np.isnan(r.replicates[:, :, :, ~dead]).any() and np.isfinite(r.crit[:, ~dead]).all()
    m = int(np.floor(alpha * (B + 1))) - 1
    assert m == 1 and (r.size[:, ~dead] <= m / B).all()
    for s in (1, 2):                                           # Λ_obs = 0 and Λ_obs = +inf: replicates at every level, as for status 0
        assert (st == s).any() and (r.iters[st == s] > 2 * 3 * B).all()
    # one mutation: a replicate is a single term; the statistic is still defined, and a draw the null cannot produce is +inf
    assert np.isfinite(r.replicates[0, 0][:, ~dead]).all()
    # φ = 1 at 50 mutations for target 5, the only signature producing the last term, where 5 is allowed: a draw of the last term is +inf
    assert st[0, 5] == 2 and np.isinf(r.replicates[1, 2, :, 0, 5]).any() and r.power[1, 1, 0, 5] > 0
    d = r.detectable(0.5)
    assert d.shape == (2, T, D) and np.isnan(d[:, dead]).all() and np.isin(d[:, ~dead], [0.07, 1.0, np.inf]).all()
    assert r.needed_mutations(1.0, 0.5).shape == (T, D)
    # crit handed back through the Python layer: the null levels are not run, size is NaN
    r2 = mmm.presence_power(_as_X(c), c.cat, [5, 1, 2], fractions=fr, n_mutations=[1, 50], alpha=alpha, allowed=c.allowed, B=B, seed=c.seed, stream=c.stream,
                            maxiter=c.maxiter, tol=c.tol, crit=r.crit)
    assert np.array_equal(r2.count_reject, r.count_reject) and np.isnan(r2.size).all() and r2.replicates is None and np.array_equal(r2.power, r.power, equal_nan=True)


def test_every_error(mmm):
    c = PR.corpus(4, 5)
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, ci, vp, ci, vp, cd, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, cd, vp, vp, vp, vp, vp, vp,
                             vp, vp, vp, vp, vp)(("mmm_presence_power", L))
    D, C, V, T = c.D, c.C, c.V, len(c.targets)
    fr0 = np.asarray([0.1, 0.5])
    nl0 = np.full((2, D), 30, dtype=np.int32)

    def rc_of(D=D, C=C, V=V, dp=c.doc_ptr, term=c.term, count=c.count, cat=c.cat, allowed=c.allowed, T=T, targets=c.targets, G=2, fr=fr0, H=2, nl=nl0, alpha=0.2,
              B=9, b0=0, maxiter=5, tol=0.0, crit_in=None, null=None):
        n = max(T if T < 100 else 1, 1) * max(D, 1)
        Hn, Ln = max(min(H, 70), 1), max(min(H, 70), 1) * (1 + max(min(G, 70), 1))
        out = dict(w_null=np.full((n, max(C, 1)), 7.0), stat=np.full(n, 7.0), score=np.full(n, 7.0), w_alt=np.full(n, 7.0), status=np.full(n, 7, np.int8),
                   iters=np.full(n, 7, np.int64), crit=np.full((Hn, n), 7.0), count_reject=np.full((Ln, n), 7, np.int32), count_zero=np.full((Ln, n), 7, np.int32),
                   rep=np.full((Ln, max(B, 1), n), 7.0))
        keep = [np.ascontiguousarray(dp, dtype=np.int64), np.ascontiguousarray(term, dtype=np.int32), np.ascontiguousarray(count, dtype=np.int32),
                np.ascontiguousarray(cat, dtype=np.float64), None if allowed is None else np.ascontiguousarray(allowed, dtype=np.uint8),
                np.ascontiguousarray(targets, dtype=np.int32), None if fr is None else np.ascontiguousarray(fr, dtype=np.float64),
                None if nl is None else np.ascontiguousarray(nl, dtype=np.int32), None if crit_in is None else np.ascontiguousarray(crit_in, dtype=np.float64)]
        p = {k: (None if a is None or k == null else a.ctypes.data) for k, a in zip(("dp", "term", "count", "cat", "allowed", "targets", "fr", "nl", "crit_in"), keep)}
        o = {k: (None if k == null else a.ctypes.data) for k, a in out.items()}
        rc = plain(ctx.h, D, C, V, p["dp"], p["term"], p["count"], p["cat"], p["allowed"], T, p["targets"], G, p["fr"], H, p["nl"], alpha, B, b0, 9, 0, maxiter, tol,
                   p["crit_in"], o["w_null"], o["stat"], o["score"], o["w_alt"], o["status"], o["iters"], o["crit"], o["count_reject"], o["count_zero"], o["rep"])
        untouched = all((a == 7).all() for a in out.values())
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    rc, _, untouched = rc_of()
    assert rc == 0 and not untouched
    assert rc_of(allowed=None)[0] == 0 and rc_of(null="rep")[0] == 0 and rc_of(H=1, nl=None)[0] == 0 and rc_of(B=0, crit_in=np.zeros((2, T * D)))[0] == 0
    assert rc_of(G=1, fr=np.asarray([1.0]))[0] == 0
    rc, _, untouched = rc_of(D=0, dp=np.zeros(1, np.int64))
    assert rc == 0 and untouched                                                           # D = 0 writes nothing
    assert plain(None, *([0] * 32)) == -1

    def refused(code, needle=None, **kw):
        rc, msg, untouched = rc_of(**kw)
        assert rc == code and untouched and (needle is None or needle in msg), (kw.keys(), rc, msg, untouched)

    for null in ("cat", "dp", "term", "count", "targets", "fr", "w_null", "stat", "score", "w_alt", "status", "iters", "crit", "count_reject", "count_zero"):
        refused(-1, null=null)
    refused(-1, "H = 1", null="nl")                                                        # no totals given means the observed ones alone
    refused(-1, T=0); refused(-1, G=0); refused(-1, H=0)
    refused(-1, "targets[1]", targets=np.asarray([0, C], np.int32))
    refused(-1, "critical value", B=0); refused(-1, B=-1); refused(-1, b0=-1); refused(-1, "2^31 - 1", B=3, b0=2 ** 31 - 3)
    for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
        refused(-1, "alpha", alpha=bad)
    for bad in ([0.5, 0.1], [0.1, 0.1], [0.0, 0.5], [0.5, 1.0000001], [-0.1, 0.5], [0.1, np.nan]):
        refused(-1, "fractions[", fr=np.asarray(bad))
    nl = nl0.copy(); nl[1, 2] = 0
    refused(-1, "n_level[1][2]", nl=nl)
    refused(-1, maxiter=0); refused(-1, tol=-1e-12); refused(-1, C=0); refused(-1, V=0); refused(-1, D=-1)
    cat = c.cat.copy(); cat[2, 3] = np.nan
    refused(-1, "catalogue entry (2, 3)", cat=cat)
    term = c.term.copy(); term[2] = V
    refused(-1, term=term)
    count = c.count.copy(); count[1] = -1
    refused(-1, count=count)
    refused(-4, "256", C=257, cat=np.ones((257, V)), allowed=None)
    refused(-4, "4096", V=4097, cat=np.ones((C, 4097)))
    refused(-4, "limit 64", G=65, fr=np.linspace(0.01, 0.9, 65))
    refused(-4, "limit 64", H=65, nl=np.full((65, D), 5, np.int32))
    refused(-4, "level items", T=2 ** 28, D=2, dp=c.doc_ptr[:3], allowed=c.allowed[:2], nl=nl0[:, :2])       # 6 levels x 2^29 items
    big = np.asarray([2 ** 30, 2 ** 30], np.int32)
    refused(-4, "2^31", D=1, dp=np.asarray([0, 2], np.int64), term=np.asarray([0, 1], np.int32), count=big, allowed=c.allowed[:1], nl=nl0[:, :1])
    with pytest.raises(mmm.MmmError, match="mmm_presence_power"):
        mmm.power._raw(ctx, c.D, c.V, c.doc_ptr, c.term, c.count, c.cat, c.targets, (0.5,), None, 0.05, c.allowed, B=2, seed=1, maxiter=0)


def test_planted_signature_power_grows_with_the_fraction_and_the_total(mmm):
    """presence_ref.planted_corpus(n_with=4, n_without=4): 8 samples of 2000 mutations, target 0 (planted at 0.1 in the first four), levels
    of 50 and 500 mutations x fractions (0.02, 0.1), α = 0.05, B = 19 (m = 0: crit is the largest null statistic), seed 5.
    tests/power_ref.py gives for it count_reject summed over the four planted samples, [total][fraction] = [[10, 63], [49, 76]] of 76 (over
    all eight: [[27, 127], [108, 152]] of 152), no comparison nearer than 1.7e-3 to crit, rounding bounds below 4e-11.  Only the orderings of
    those sums are asserted on the device -- no power threshold was fixed before that evaluation -- and the size, which the definition proves."""
    c, has = PR.planted_corpus(n_with=4, n_without=4)
    B, alpha = 19, 0.05
    r = mmm.presence_power(_as_X(c), c.cat, [0], fractions=(0.02, 0.1), n_mutations=[50, 500], alpha=alpha, B=B, seed=c.seed, stream=c.stream, maxiter=c.maxiter,
                           tol=c.tol)
    assert (r.status != 3).all() and (r.size <= alpha).all() and (r.size == 0).all() and (r.count_reject <= B).all()
    tot = r.count_reject[:, :, 0, :][:, :, has].sum(axis=2)              # [total, fraction]
    print("count_reject over the planted samples, [total][fraction]: %s" % tot.tolist())
    assert tot[0, 0] < tot[0, 1] and tot[1, 0] < tot[1, 1]              # in φ at either total
    assert tot[0, 0] < tot[1, 0] and tot[0, 1] < tot[1, 1]              # in N at either fraction
