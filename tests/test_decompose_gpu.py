"""The signature decomposition on the device against its numpy restatement (tests/decompose_ref.py): subset, weight, gain and cosine of
mmm_decompose_search bit for bit on the same (G, b, ss); the moments of mmm_signature_decompose within their a-priori bound and its search
bit for bit on its own moments; ranks next to 2^32; both routes of G, repeated runs and batch sizes give equal bits; every error; the
Python layer against the composition done by hand."""
import functools

import numpy as np
import pytest

import decompose_ref as DR
import np_ref

pytestmark = pytest.mark.gpu


def _bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same(got, want, what):
    for name, g, w in zip(("subset", "weight", "gain", "cosine"), got, want):
        if not _bits(g, w):
            bad = np.argwhere(np.asarray(g) != np.asarray(w))
            raise AssertionError("%s: %s differs at %d places, first %r: device %r, restatement %r" % (what, name, len(bad), tuple(bad[0]), g[tuple(bad[0])],
                                                                                                   w[tuple(bad[0])]))


@functools.lru_cache(maxsize=None)
def _case(C, S, n):
    G, b, ss = DR.search_case(C, S, n)
    return G, b, ss, DR.search(G, b, ss, S)


# ------------------------------------------------------------------------------------------------------------ 1. the search
@pytest.mark.parametrize("n", DR.SEARCH_N)
@pytest.mark.parametrize("C,S", DR.SEARCH_SHAPES)
def test_search_equals_the_restatement_bit_for_bit(mmm, C, S, n):
    G, b, ss, want = _case(C, S, n)
    got = mmm.decompose_search(G, b, ss, S)
    assert got.subset.dtype == np.int32 and got.subset.shape == (n, S, S) and got.gain.shape == (n, S)
    _same(got, want, "C = %d, S = %d, n = %d" % (C, S, n))
    found = got.subset[:, :, 0] >= 0
    print("C = %d, S = %d, n = %d: %d of %d (signature, size) pairs have an admissible subset" % (C, S, n, int(found.sum()), found.size))
    assert not found[ss == 0].any() and found[ss > 0][:, 0].all()
    if S > C:
        assert not found[:, C:].any()


def test_two_runs_and_a_signature_alone_give_the_bits_of_the_batch(mmm):
    G, b, ss, _ = _case(20, 4, 70)
    a = mmm.decompose_search(G, b, ss, 4)
    again = mmm.decompose_search(G, b, ss, 4)
    _same(again, a, "second run")
    for i in (0, 1, 33, 69):
        one = mmm.decompose_search(G, b[i:i + 1], ss[i:i + 1], 4)
        _same(one, tuple(x[i:i + 1] for x in a), "signature %d alone" % i)
    empty = mmm.decompose_search(G, np.zeros((0, 20)), np.zeros(0), 4)
    assert empty.subset.shape == (0, 4, 4)


@pytest.mark.parametrize("C", [128, 129])
def test_either_side_of_the_lds_threshold(mmm, C):
    """C = 128 is the largest G staged in LDS (128 KiB of the 160), C = 129 the first read through L2"""
    G, b, ss, want = _case(C, 3, 7)
    _same(mmm.decompose_search(G, b, ss, 3), want, "C = %d" % C)


@pytest.mark.parametrize("C,S", [(12, 3), (86, 3)])
def test_lds_and_l2_routes_give_equal_bits(mmm, C, S):
    G, b, ss, want = _case(C, S, 7)
    l2 = mmm.decompose_search(G, b, ss, S, in_lds=False)
    assert mmm.default_context().get_tuning().disable == 0                # the hook is undone
    _same(l2, want, "through L2")
    _same(mmm.decompose_search(G, b, ss, S), want, "in LDS")


# ------------------------------------------------------------------------------------------------------------ 2. moments, then search
@pytest.mark.parametrize("V", DR.MOMENT_V)
def test_signature_decompose_moments_and_search(mmm, V):
    rng = np.random.default_rng(500 + V)
    C, S, n = 14, 3, 7
    cat = DR.catalogue(rng, C, V)
    sig = DR.signatures(rng, cat, n)
    ctx = mmm.default_context()
    got, (G, b, ss) = mmm.decompose._raw(ctx, sig, cat, S, moments=True)
    eG, eb, es = DR.moments_exact(sig, cat)
    bound = (V + 2) * 2.0 ** -52                                          # x the sum of |terms| = the exact entry (all terms are >= 0)
    for name, g, e in (("G", G, eG), ("b", b, eb), ("ss", ss, es)):
        err = float((np.abs(g - e) / np.where(e > 0, e, 1.0)).max())
        print("V = %d: max |%s - exact| / sum |terms| = %.3g (bound %.3g)" % (V, name, err, bound))
        assert (np.abs(g - e) <= bound * e).all(), name
    assert np.array_equal(G, G.T) and not ss[4] and not b[4].any()         # symmetric by construction; the zero row
    _same(got, DR.search(G, b, ss, S), "V = %d, on the device's own moments" % V)
    plain = mmm.decompose._raw(ctx, sig, cat, S)                           # without the moment outputs
    _same(plain, got, "NULL moment outputs")
    _same(mmm.decompose_search(G, b, ss, S), got, "the search alone on the downloaded moments")


def test_more_signatures_than_one_launch_takes(mmm):
    """1030 signatures: moments and search both go through in chunks of 1024; the last six land where they belong"""
    rng = np.random.default_rng(1030)
    cat = DR.catalogue(rng, 6, 8, degenerate=False)
    sig = DR.signatures(rng, cat, 1030)
    got, (G, b, ss) = mmm.decompose._raw(mmm.default_context(), sig, cat, 2, moments=True)
    eG, eb, es = DR.moments_exact(sig[1020:], cat)
    assert (np.abs(b[1020:] - eb) <= 10 * 2.0 ** -52 * eb).all() and (np.abs(ss[1020:] - es) <= 10 * 2.0 ** -52 * es).all()
    _same(got, DR.search(G, b, ss, 2), "n = 1030")


# ------------------------------------------------------------------------------------------------------------ 3. ranks next to 2^32
def test_ranks_close_to_the_limit(mmm):
    """C = 86, S = 6: 4.7e8 subsets of size 6 (ranks up to binom(86, 6) - 1 = 469,959,722 of the 2^32 - 1 allowed), one noisy signature
    planted on the rows 80 .. 85 -- the last prefixes and the last extensions."""
    import time
    rng = np.random.default_rng(86)
    cat = DR.catalogue(rng, 86, 96, degenerate=False)
    planted = np.arange(80, 86)
    sig = (rng.uniform(0.5, 1.0, size=6) @ cat[planted] * rng.gamma(2500.0, 1.0 / 2500.0, size=96))[None]
    G, b, ss = DR.moments(sig, cat)
    mmm.decompose_search(G, b, ss, 2)                                      # (context and library are up before the clock starts)
    t0 = time.perf_counter()
    got = mmm.decompose_search(G, b, ss, 6)
    print("C = 86, S = 6, n = 1: %.3f s" % (time.perf_counter() - t0))
    for s in range(1, 7):
        m = got.subset[0, s - 1]
        assert (m[:s] >= 0).all() and (np.diff(m[:s]) > 0).all() and (m[s:] == -1).all(), m
        ok, gain, w = DR.evaluate(G, b[0], m[:s])
        assert ok and _bits(gain, got.gain[0, s - 1]) and _bits(w, got.weight[0, s - 1, :s]) and not got.weight[0, s - 1, s:].any(), s
        assert _bits(np.sqrt(min(gain / ss[0], 1.0)), got.cosine[0, s - 1])
    ok, gain, _ = DR.evaluate(G, b[0], planted)
    print("planted subset admissible: %s, its gain %.17g, the device's size-6 gain %.17g" % (ok, gain, got.gain[0, 5]))
    assert ok and got.gain[0, 5] >= gain


# ------------------------------------------------------------------------------------------------------------ 4. errors
def test_every_error_and_limit(mmm):
    L, ctx = mmm.lib(), mmm.default_context()
    G, b, ss, want = _case(12, 6, 7)
    n, C = b.shape

    def search(n=n, C=C, S=2, G=G, b=b, ss=ss, null=None, h=ctx.h):
        out = [np.full((max(n, 1), S, S), -7, dtype=np.int32), np.zeros((max(n, 1), S, S)), np.zeros((max(n, 1), S)), np.zeros((max(n, 1), S))]
        arrs = dict(G=np.ascontiguousarray(G), b=np.ascontiguousarray(b), ss=np.ascontiguousarray(ss), subset=out[0], weight=out[1], gain=out[2], cosine=out[3])
        p = {k: (None if k == null else v.ctypes.data) for k, v in arrs.items()}
        rc = L.mmm_decompose_search(h, n, C, S, p["G"], p["b"], p["ss"], p["subset"], p["weight"], p["gain"], p["cosine"])
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), out

    assert search()[0] == 0 and search(h=None)[0] == -1
    for null in ("G", "b", "ss", "subset", "weight", "gain", "cosine"):
        assert search(null=null)[0] == -1, null
    assert search(S=0)[0] == -1 and search(C=0)[0] == -1 and search(n=-1)[0] == -1
    rc, msg, out = search(n=0)
    assert rc == 0 and (out[0] == -7).all()                               # n = 0 writes nothing
    rc, msg, _ = search(S=7)
    assert rc == -4 and "S = 7" in msg and "limit 6" in msg, msg
    big = np.eye(257)
    rc, msg, _ = search(C=257, G=big, b=np.ones((n, 257)))
    assert rc == -4 and "C = 257" in msg and "limit 256" in msg, msg
    rc, msg, _ = search(C=256, S=5, G=big[:256, :256], b=np.ones((n, 256)))
    assert rc == -4 and "8809549056" in msg and "2^32" in msg, msg
    assert search(C=256, S=4, n=1, G=big[:256, :256], b=np.ones((1, 256)), ss=np.ones(1))[0] == 0      # binom(256, 4) = 174,792,640 is allowed
    # moments that are not finite: the signature is marked, the others are computed, the call says which
    for bad in (np.nan, np.inf):
        b2 = b.copy(); b2[2, 5] = bad
        rc, msg, out = search(b=b2, S=3)
        assert rc == -1 and "signature 2" in msg, msg
        assert (out[0][2] == -1).all() and not out[1][2].any() and not out[2][2].any() and not out[3][2].any()
        keep = [i for i in range(n) if i != 2]
        ref = DR.search(G, b, ss, 3)
        assert all(_bits(o[keep], r[keep]) for o, r in zip(out, ref))
    s2 = ss.copy(); s2[1] = np.nan
    rc, msg, out = search(ss=s2)
    assert rc == -1 and "signature 1" in msg and (out[0][1] == -1).all()
    G2 = G.copy(); G2[3, 4] = np.nan
    rc, msg, out = search(G=G2)
    assert rc == -1 and "G[3][4]" in msg and (out[0] == -1).all() and not out[2].any()
    with pytest.raises(mmm.MmmError, match="signature 2"):
        b2 = b.copy(); b2[2, 0] = np.nan
        mmm.decompose_search(G, b2, ss, 2)

    rng = np.random.default_rng(3)
    cat = DR.catalogue(rng, 6, 10, degenerate=False); sig = DR.signatures(rng, cat, 3)

    def full(n=3, C=6, V=10, S=2, sig=sig, cat=cat, null=None):
        out = [np.zeros((max(n, 1), S, S), dtype=np.int32), np.zeros((max(n, 1), S, S)), np.zeros((max(n, 1), S)), np.zeros((max(n, 1), S))]
        arrs = dict(sig=np.ascontiguousarray(sig), cat=np.ascontiguousarray(cat), subset=out[0], weight=out[1], gain=out[2], cosine=out[3])
        p = {k: (None if k == null else v.ctypes.data) for k, v in arrs.items()}
        rc = L.mmm_signature_decompose(ctx.h, n, C, V, p["sig"], p["cat"], S, p["subset"], p["weight"], p["gain"], p["cosine"], None, None, None)
        return rc, (L.mmm_last_error(ctx.h) or b"").decode()

    assert full()[0] == 0
    for null in ("sig", "cat", "subset", "weight", "gain", "cosine"):
        assert full(null=null)[0] == -1, null
    assert full(V=0)[0] == -1 and full(S=0)[0] == -1 and full(C=0)[0] == -1 and full(n=-1)[0] == -1
    assert full(S=7)[0] == -4 and full(C=257, cat=np.ones((257, 10)))[0] == -4
    for bad in (-1e-3, np.nan, np.inf):
        c2 = cat.copy(); c2[3, 7] = bad
        rc, msg = full(cat=c2)
        assert rc == -1 and "catalogue entry (3, 7)" in msg, msg
        s2 = sig.copy(); s2[1, 4] = bad
        rc, msg = full(sig=s2)
        assert rc == -1 and "signature entry (1, 4)" in msg, msg
    c2 = cat.copy(); c2[5] = 0.0
    rc, msg = full(cat=c2)
    assert rc == -1 and "row 5 is all zero" in msg, msg
    Gout = np.full((6, 6), -1.0)                                           # n = 0: the moments asked for and nothing else
    assert L.mmm_signature_decompose(ctx.h, 0, 6, 10, None, cat.ctypes.data, 2, None, None, None, None, Gout.ctypes.data, None, None) == 0
    assert _bits(Gout, mmm.decompose._raw(ctx, sig, cat, 2, moments=True)[1][0])


# ------------------------------------------------------------------------------------------------------------ 5. the Python layer
def _by_hand(mmm, sig2d, cat, S, min_gain):
    """the composition of `decompose_signatures` from the raw search, written out again"""
    G, b, ss = mmm.decompose._raw(mmm.default_context(), sig2d, cat, S, moments=True)[1]
    subset, weight, gain, cosine = DR.search(G, b, ss, S)
    a = cat.sum(axis=1)
    out = []
    for i in range(sig2d.shape[0]):
        cbest = [max(cosine[i, :s + 1]) for s in range(S)]
        s = min(s for s in range(S) if cbest[S - 1] - cbest[s] < min_gain)
        t = min(t for t in range(s + 1) if cosine[i, t] == cbest[s])
        m = subset[i, t]; w = weight[i, t]
        mass = np.array([w[j] * a[m[j]] if m[j] >= 0 else 0.0 for j in range(S)])
        out.append((int((m >= 0).sum()), m, w, mass / mass.sum() if mass.sum() > 0 else mass, cosine[i, t]))
    return out, (subset, weight, cosine)


def test_decompose_signatures_is_the_composition_done_by_hand(mmm):
    rng = np.random.default_rng(77)
    C, V, S = 20, 96, 3
    cat = DR.catalogue(rng, C, V)
    names = ["SBS%d" % (c + 1) for c in range(C)]
    sig = DR.signatures(rng, cat, 10)
    d = mmm.decompose_signatures(sig, cat, max_size=S, names=names)
    want, path = _by_hand(mmm, sig, cat, S, 0.01)
    assert d.size.shape == (10,) and d.members.shape == (10, S) and d.path_members.shape == (10, S, S) and d.names == names
    for i, (size, m, w, sh, cs) in enumerate(want):
        assert d.size[i] == size and _bits(d.members[i], m) and _bits(d.weights[i], w) and _bits(d.shares[i], sh) and _bits(d.cosine[i], cs), i
    assert _bits(d.path_members, path[0]) and _bits(d.path_weights, path[1]) and _bits(d.path_cosine, path[2])
    assert d.size[4] == 0 and (d.members[4] == -1).all()                   # the zero row
    assert d.path_cosine[1].max() >= 1 - 1e-12 and d.cosine[1] > 0.989     # an exact planted mixture of at most 3 rows is reconstructed
    text = d.describe()
    assert len(text) == 10 and text[4] == "no admissible mixture" and all("SBS%d" % (m + 1) in text[i] for i in (0, 1) for m in d.members[i][d.members[i] >= 0])
    mask = np.zeros(C, dtype=bool)
    for i in range(10):
        for m in d.members[i]:
            if m >= 0:
                mask[m] = True
    assert d.allowed(C).dtype == bool and np.array_equal(d.allowed(C), mask) and 0 < mask.sum() < C
    # [R, K, V]: every replica as it comes out alone; a (names, terms, S) catalogue keeps its names
    stack = np.stack([sig[:5], sig[5:]])
    d3 = mmm.decompose_signatures(stack, (names, ["t%d" % v for v in range(V)], cat), max_size=S)
    assert d3.size.shape == (2, 5) and d3.members.shape == (2, 5, S) and d3.path_weights.shape == (2, 5, S, S) and d3.names == names
    for f in ("size", "members", "weights", "shares", "cosine", "path_members", "path_weights", "path_cosine"):
        assert _bits(getattr(d3, f).reshape(getattr(d, f).shape), getattr(d, f)), f
    # a larger margin never chooses a larger size
    wide = mmm.decompose_signatures(sig, cat, max_size=S, min_gain=0.2)
    assert (wide.size <= d.size).all()


def test_fitted_lda_and_the_mask_in_a_refit(mmm):
    rng = np.random.default_rng(9)
    V, K, C = 96, 3, 12
    X, _ = np_ref.synth_lda(40, V, K, seed=31, mean_n=500)
    g = mmm.LDA(K, 0.1, 0.1, V, X, seed=4)
    mmm.fit(g, maxiter=20, tol=0.0, verbose=False)
    cat = DR.catalogue(rng, C, V, degenerate=False)
    d = mmm.decompose_signatures(g, cat, max_size=2)
    sig = np.ascontiguousarray(g.β.T)
    want, _ = _by_hand(mmm, sig, cat, 2, 0.01)
    for i, (size, m, w, sh, cs) in enumerate(want):
        assert d.size[i] == size and _bits(d.members[i], m) and _bits(d.weights[i], w) and _bits(d.shares[i], sh) and _bits(d.cosine[i], cs), i
    mask = d.allowed(C)
    assert mask.shape == (C,) and mask.any() and not mask.all()
    r = mmm.refit_exposures(X, cat, allowed=mask)
    assert not r.exposures[~mask].any() and not r.active[~mask].any()      # exactly 0 outside the mask
    assert r.exposures[mask].sum() > 0
    feats = np.stack([np.arange(V) // 16 + 1, np.arange(V) % 16 + 1], axis=1)
    with pytest.raises(TypeError, match="factorised"):
        mmm.decompose_signatures(mmm.ILDA(K, 0.1, [0.1, 0.1], feats, X, seed=1), cat)
