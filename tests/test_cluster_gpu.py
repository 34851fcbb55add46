"""mmm_cluster_samples on the device against its float64 restatement (tests/cluster_ref.py): every output bit for bit (only +, -, x, /,
comparisons and integers decide them); the invariances the definition promises (waves, placement, a second run, slices, additivity); the
invariants of the pair counts; every error; the Python layer against its composition done by hand; the planted groups."""
import ctypes
import os

import numpy as np
import pytest

import cluster_ref as C

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("labels", "iters", "inertia", "together", "same", "ambiguous", "valid")
CASES = {c.name: c for c in C.cases()}


def _run(mmm, c, b0=None, B=None, waves=0, placement=0, **kw):
    return mmm.cluster._raw(mmm.default_context(), c.x, c.ks, c.B if B is None else B, c.b0 if b0 is None else b0, c.keep, c.seed, 0, c.maxiter, c.pac_lo,
                            c.pac_hi, waves, placement, **kw)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _same(a, b, what=""):
    for k in KEYS:
        assert _bits(a[k], b[k]), (what, k)


def _invariants(got):
    tog, same = got["together"], got["same"]
    assert (same <= tog).all()
    assert np.array_equal(same, same.transpose(0, 2, 1)) and np.array_equal(tog, tog.transpose(0, 2, 1))
    i = np.arange(tog.shape[1])
    assert np.array_equal(same[:, i, i], tog[:, i, i])
    assert (got["ambiguous"] >= 0).all() and (got["ambiguous"] <= got["valid"]).all()


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_equal_the_restatement(mmm, name):
    c = CASES[name]
    got, ref = _run(mmm, c), C.reference(c)
    for k in KEYS:
        want = getattr(ref, k)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        if k in ("labels", "iters", "inertia"):
            bad = np.argwhere((got[k].reshape(len(c.ks), c.B, -1).view(np.uint8) != want.reshape(len(c.ks), c.B, -1).view(np.uint8)).any(axis=2))
            assert bad.size == 0, "%s: %s differs in the pairs (ki, b) %s" % (name, k, bad.tolist()[:10])
        assert _bits(got[k], want), (name, k)
    _invariants(got)


@pytest.mark.parametrize("name", ["D5P2keep", "D12twokeep", "D130P33", "D257P1", "D40k32", "nk16", "ldsfits", "ldsover"])
def test_every_geometry_and_a_second_run_give_equal_bits(mmm, name):
    """ldsfits / ldsover stand on either side of the one threshold the code has (the per-block arrays in LDS or in memory); every case runs
    under both placement pins: 1 on ldsover cannot fit and takes the workspace, 2 on the others forces it"""
    c = CASES[name]
    base = _run(mmm, c)
    _same(base, _run(mmm, c), "second run")
    for waves in (1, 4, 16):
        _same(base, _run(mmm, c, waves=waves), "waves %d" % waves)
    for placement in (1, 2):
        _same(base, _run(mmm, c, placement=placement), "placement %d" % placement)
    _same(base, _run(mmm, c, waves=1, placement=2), "waves 1 in memory")


def test_a_call_is_a_slice_and_counts_add(mmm):
    c = CASES["b0"]
    whole, head, tail = _run(mmm, c), _run(mmm, c, b0=0, B=2), _run(mmm, c, b0=2, B=4)
    for k in ("labels", "iters", "inertia"):
        assert _bits(np.ascontiguousarray(whole[k][:, 2:]), tail[k]) and _bits(np.ascontiguousarray(whole[k][:, :2]), head[k]), k
    for k in ("together", "same"):
        assert _bits(whole[k], head[k] + tail[k]), k
    amb, val = C.pac_counts(head["together"] + tail["together"], head["same"] + tail["same"], c.pac_lo, c.pac_hi)
    assert _bits(whole["ambiguous"], amb) and _bits(whole["valid"], val)
    ref = C.reference(c, b0=2, B=4)
    for k in KEYS:
        assert _bits(tail[k], getattr(ref, k)), k
    # more pairs than blocks in flight, from a large b0
    many = _run(mmm, CASES["D5P2keep"], b0=2 ** 31 - 1 - 3000, B=3000)
    again = _run(mmm, CASES["D5P2keep"], b0=2 ** 31 - 1 - 3000, B=3000, waves=1)
    _same(many, again, "3000 replicates")
    part = C.reference(CASES["D5P2keep"], b0=2 ** 31 - 1 - 4, B=4)
    assert _bits(np.ascontiguousarray(many["labels"][:, -4:]), part.labels) and _bits(np.ascontiguousarray(many["inertia"][:, -4:]), part.inertia)
    _invariants(many)


def test_null_outputs_are_accepted(mmm):
    c = CASES["D65P3"]
    full = _run(mmm, c)
    for outs in ((), ("together",), ("same",), ("ambiguous", "valid"), ("valid",), ("same", "ambiguous")):
        got = _run(mmm, c, outputs=outs)
        assert sorted(got) == sorted(("labels", "iters", "inertia") + outs)
        for k in got:
            assert _bits(got[k], full[k]), (outs, k)


def test_every_error(mmm):
    c = CASES["D65P3"]
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, vp, ci, vp, ci, ci, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp,
                             vp)(("mmm_cluster_samples", L))
    keep = []

    def call(h=True, x=c.x, D=None, P=None, ks=c.ks, nk=None, B=2, b0=0, maxiter=3, lo=100, hi=900, waves=0, placement=0, null=(), big_out=True):
        x = np.ascontiguousarray(x, dtype=np.float64)
        D = x.shape[0] if D is None else D
        P = x.shape[1] if P is None else P
        ksa = np.ascontiguousarray(ks, dtype=np.int32)
        nk = ksa.size if nk is None else nk
        n1, B1, D1 = max(nk, 1), max(B, 1) if big_out else 1, max(D, 1) if big_out else 1
        out = dict(labels=np.full((n1, B1, D1), 7, dtype=np.int8), iters=np.full((n1, B1), 7, dtype=np.int32), inertia=np.full((n1, B1), 7.0),
                   together=np.full((n1, D1, D1), 7, dtype=np.uint32), same=np.full((n1, D1, D1), 7, dtype=np.uint32),
                   ambiguous=np.full(n1, 7, dtype=np.int64), valid=np.full(n1, 7, dtype=np.int64))
        arrs = dict(x=x, ks=ksa)
        keep.append((arrs, out))
        p = {k: (None if k in null else v.ctypes.data) for k, v in list(arrs.items()) + list(out.items())}
        rc = plain(ctx.h if h else None, D, P, p["x"], nk, p["ks"], B, b0, c.keep, 5, 0, maxiter, lo, hi, waves, placement, p["labels"], p["iters"], p["inertia"],
                   p["together"], p["same"], p["ambiguous"], p["valid"])
        untouched = all((v == 7).all() for v in out.values())
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    rc, _, untouched = call()
    assert rc == 0 and not untouched
    rc, _, untouched = call(B=0)                                         # nothing to do: nothing written
    assert rc == 0 and untouched
    arg = [dict(h=False), dict(D=0), dict(D=-1), dict(P=0), dict(nk=0), dict(nk=-1), dict(ks=(2, 0)), dict(ks=(-1,)), dict(B=-1), dict(b0=-1),
           dict(b0=2 ** 31 - 2, B=2), dict(maxiter=0), dict(lo=-1), dict(lo=900, hi=900), dict(lo=901, hi=900), dict(hi=1001), dict(waves=3), dict(waves=32),
           dict(waves=-1), dict(placement=3), dict(placement=-1), dict(null=("x",)), dict(null=("ks",)), dict(null=("labels",)), dict(null=("iters",)),
           dict(null=("inertia",))]
    for kw in arg:
        rc, msg, untouched = call(**kw)
        assert rc == -1 and untouched, (kw, rc, msg)
    for bad in (np.nan, np.inf, -np.inf, 1.0000001e150, -2e150):
        x = c.x.copy(); x[7, 2] = bad
        rc, msg, untouched = call(x=x)
        assert rc == -1 and untouched and "x entry (7, 2)" in msg, (bad, msg)
    x = c.x.copy(); x[7, 2] = 1e150; x[8, 0] = -1e150                    # the bound itself is accepted
    assert call(x=x)[0] == 0
    # limits, each with its figure in the message
    rc, msg, untouched = call(x=np.zeros((4097, 1)), ks=(1,), big_out=False)
    assert rc == -4 and untouched and "4097" in msg and "4096" in msg, msg
    rc, msg, untouched = call(x=np.zeros((2, 257)), ks=(1,))
    assert rc == -4 and untouched and "257" in msg and "256" in msg, msg
    rc, msg, untouched = call(ks=tuple(range(1, 18)))
    assert rc == -4 and untouched and "17" in msg and "16" in msg, msg
    rc, msg, untouched = call(ks=(2, 33))
    assert rc == -4 and untouched and "33" in msg and "32" in msg, msg
    rc, msg, untouched = call(x=np.zeros((4096, 1)), ks=(1,), B=2 ** 19, big_out=False)
    assert rc == -4 and untouched and "2^31" in msg and str(2 ** 31) in msg, msg


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_python_is_its_composition_done_by_hand(mmm):
    E = np.abs(C.blobs(70, 5, 3, 11, 0.05)) + 1e-3
    ks = [2, 3, 4, 5]
    r = mmm.cluster_samples(E, ks=ks, replicates=40, subsample=0.75, seed=21, maxiter=60, pac=(0.05, 0.95))
    x = np.sqrt(E / E.sum(axis=1, keepdims=True))
    raw = mmm.cluster._raw(mmm.default_context(), x, ks, 40, 0, int(np.floor(0.75 * 2 ** 32)), 21, 0, 60, 50, 950)
    ref = C.cluster(x, ks, 40, 0, C.keep_of(0.75), 21, 0, 60, 50, 950)
    for k in KEYS:
        assert _bits(raw[k], getattr(ref, k)), k
    pac = raw["ambiguous"] / raw["valid"].astype(np.float64)
    cons = C.consensus(raw["together"], raw["same"])
    pick = int(np.argmin(pac))
    assert np.array_equal(r.ks, ks) and _bits(r.pac, pac) and r.k == ks[pick] and r.replicates == 40
    assert _bits(r.consensus, cons) and _bits(r.together, raw["together"]) and _bits(r.iters, raw["iters"]) and _bits(r.inertia, raw["inertia"])
    for i, k in enumerate(ks):
        assert np.array_equal(r.labels_by_k[i], C.upgma(1.0 - cons[i], k)), k
    assert np.array_equal(r.labels, r.labels_by_k[pick])
    item = np.full(70, np.nan)
    for d in range(70):
        others = np.flatnonzero((r.labels == r.labels[d]) & (np.arange(70) != d))
        if others.size:
            item[d] = cons[pick][d, others].mean()
    assert np.allclose(r.item_consensus, item, rtol=1e-13, atol=0, equal_nan=True)
    for g in range(r.k):
        idx = np.flatnonzero(r.labels == g)
        if idx.size > 1:
            sub = cons[pick][np.ix_(idx, idx)]
            assert np.isclose(r.cluster_consensus[g], sub[np.triu_indices(idx.size, 1)].mean(), rtol=1e-13, atol=0)
    assert np.array_equal(r.flagged(0.9), np.flatnonzero(item < 0.9))
    assert np.array_equal(r.skipped, [0, 0, 0, 0]) and np.array_equal(r.unsettled, (raw["iters"] == 60).sum(axis=1))
    # k= overrides the choice; counts=False leaves the matrices out; subsample = 1 keeps every sample; euclidean passes the array on
    other = ks[(pick + 1) % 4]
    o = mmm.cluster_samples(E, ks=ks, replicates=40, subsample=0.75, seed=21, maxiter=60, pac=(0.05, 0.95), k=other, counts=False)
    assert o.k == other and np.array_equal(o.labels, r.labels_by_k[ks.index(other)]) and o.consensus is None and o.together is None
    e = mmm.cluster_samples(x, ks=[3], replicates=6, subsample=1.0, seed=2, metric="euclidean")
    raw1 = mmm.cluster._raw(mmm.default_context(), x, [3], 6, 0, 0, 2, 0, 100, 100, 900)
    assert (raw1["labels"] >= 0).all() and _bits(e.together, raw1["together"]) and (e.together == 6).all() and e.k == 3


def test_python_takes_fitted_models_on_the_shipped_tables(mmm):
    _, samples, snv = mmm.read_counts_tsv(os.path.join(GOLD, "brca-eu_snv_counts.tsv"))
    _, samples2, sv = mmm.read_counts_tsv(os.path.join(GOLD, "brca-eu_sv_counts.tsv"))
    snv_d, sv_d = {s: snv[:, i] for i, s in enumerate(samples)}, {s: sv[:, i] for i, s in enumerate(samples)}
    g = mmm.LDA(5, 0.1, 0.1, mmm.format_counts_lda(snv_d, samples), seed=1)
    try:
        mmm.fit(g, maxiter=10, tol=0.0, verbose=False)
        r = mmm.cluster_samples(g, ks=[2, 3], replicates=8, seed=4)
        th = np.asarray(g.θ)
        by_hand = mmm.cluster_samples(np.ascontiguousarray((th / th.sum(axis=0, keepdims=True)).T), ks=[2, 3], replicates=8, seed=4)
        assert r.labels.shape == (560,) and _bits(r.together, by_hand.together) and _bits(r.consensus, by_hand.consensus) and np.array_equal(r.labels, by_hand.labels)
        assert set(np.unique(r.labels)) == set(range(r.k))
    finally:
        g.close()
    rng = np.random.default_rng(2)
    g0 = [rng.integers(1, 101, size=(4, 96)).astype(np.float64), rng.integers(1, 101, size=(3, 48)).astype(np.float64)]
    m = mmm.MMCTM([4, 3], [0.1, 0.1], [96, 48], mmm.format_counts_mmctm([snv_d, sv_d], samples), γ0=g0)
    try:
        mmm.fit(m, maxiter=3, tol=0.0, verbose=False)
        props = m._get("props").reshape(560, 7)
        both = mmm.cluster_samples(m, ks=[2], replicates=6, seed=4)
        assert _bits(both.together, mmm.cluster_samples(props, ks=[2], replicates=6, seed=4).together)
        sv_only = mmm.cluster_samples(m, ks=[2], replicates=6, seed=4, modalities=[1])
        assert _bits(sv_only.consensus, mmm.cluster_samples(props[:, 4:], ks=[2], replicates=6, seed=4).consensus)
        with pytest.raises(ValueError):
            mmm.cluster_samples(m, ks=[2], replicates=6, modalities=[2])
    finally:
        m.close()


@pytest.mark.parametrize("D,P,G,conc,seed", C.PLANTED)
def test_planted_groups_come_back_on_the_device(mmm, D, P, G, conc, seed):
    """follows from the bitwise equality with the restatement (whose behaviour on these inputs tests/test_cluster_cpu.py asserts); asserted anyway"""
    x, truth = C.planted(D, P, G, conc, seed)
    ks = list(range(2, G + 3))
    ref = C.planted_reference(D, P, G, conc, seed)
    raw = mmm.cluster._raw(mmm.default_context(), x, ks, 100, 0, C.keep_of(0.8), 1000 + seed, 0, 100, 100, 900)
    for k in KEYS:
        assert _bits(raw[k], getattr(ref, k)), k
    r = mmm.cluster_samples(x, ks=ks, replicates=100, subsample=0.8, seed=1000 + seed, metric="euclidean")
    assert r.k == G and len(set(zip(r.labels.tolist(), truth.tolist()))) == G
    assert all(r.pac[i] >= r.pac[ks.index(G)] + 0.05 for i in range(len(ks)) if ks[i] != G)
