"""What the comparison test's GPU suite rests on, checked on the numpy restatement alone (tests/compare_ref.py): the dealing against a
brute-force sort, its invariants, its uniformity and the documented bias of the key_bits hook, the calibration of the test, the separation
that makes count_ge comparable across implementations of log; and the argument checks of the Python layer that need no device."""
import numpy as np
import pytest

import compare_ref as CR


def test_dealing_is_the_brute_force_sort_of_key_and_index():
    """tiny N: sorted() on (key, index) tuples, in plain Python integers, against the lexsort of the restatement, at every kind of key width"""
    count = np.array([3, 0, 2, 1, 4, 0, 1])
    N = int(count.sum())
    entry = np.repeat(np.arange(count.size), count)
    for key_bits in (32, 8, 3, 1):
        for Na in (0, 1, 5, N - 1, N):
            got = CR.deal_doc(count, Na, 6, np.arange(3, 9), seed=2 ** 40 + 17, stream=5, key_bits=key_bits)
            words = CR.deal_words(N, 6, np.arange(3, 9), 2 ** 40 + 17, 5)
            for r in range(6):
                pairs = sorted((int(words[r, i]) >> (32 - key_bits), i) for i in range(N))
                want = np.bincount([entry[i] for _, i in pairs[:Na]], minlength=count.size)
                assert np.array_equal(got[r], want), (key_bits, Na, r)


def test_dealt_counts_sum_to_n_a_stay_within_the_entry_and_chunked_calls_are_slices():
    rng = np.random.default_rng(5)
    docs = [rng.integers(0, 9, size=w) for w in (7, 1, 0, 300, 12)]
    dp = np.concatenate([[0], np.cumsum([d.size for d in docs])]).astype(np.int64)
    count = np.concatenate(docs)
    N = np.array([d.sum() for d in docs])
    n_a = np.array([3, N[1], 0, 257, N[4] - 1])
    for key_bits in (32, 3):
        whole = CR.deal(dp, count, n_a, 11, 0, seed=9, stream=1, key_bits=key_bits)
        assert (whole >= 0).all() and (whole <= count[None, :]).all()
        for d in range(len(docs)):
            assert (whole[:, dp[d]:dp[d + 1]].sum(axis=1) == n_a[d]).all()
        assert np.array_equal(CR.deal(dp, count, n_a, 4, 7, seed=9, stream=1, key_bits=key_bits), whole[7:])
        assert np.array_equal(CR.deal(dp, count, n_a, 7, 0, seed=9, stream=1, key_bits=key_bits), whole[:7])
    assert not np.array_equal(CR.deal(dp, count, n_a, 3, 0, seed=9, stream=2), CR.deal(dp, count, n_a, 3, 0, seed=9, stream=1))


def test_every_mutation_is_dealt_equally_often_and_small_keys_favour_low_indices():
    """N = 40, N_a = 15, B = 4000: under a uniform subset every mutation's inclusion count is Binomial(4000, 0.375), sd 30.6; all 40 within
    4.5 sd (two-sided 7e-6 each) at key_bits = 32.  At key_bits = 2 a quarter of the mutations share each key and the lowest indices of
    the threshold's group win: the threshold is almost always key 1, mutation 0 is in with every key <= 1 (about 0.5), mutation 39 only
    with key 0 (about 0.25) -- the hook is biased as the header says."""
    N, Na, B = 40, 15, 4000
    m32 = CR.deal_members(N, Na, 3, np.arange(B), seed=77, stream=0, key_bits=32)
    assert (m32.sum(axis=1) == Na).all()
    inc = m32.sum(axis=0)
    sd = np.sqrt(B * 0.375 * 0.625)
    print("inclusion counts at key_bits = 32: %d .. %d (mean %.0f, sd %.1f)" % (inc.min(), inc.max(), B * 0.375, sd))
    assert (np.abs(inc - B * 0.375) <= 4.5 * sd).all()
    m2 = CR.deal_members(N, Na, 3, np.arange(B), seed=77, stream=0, key_bits=2)
    assert (m2.sum(axis=1) == Na).all()
    f = m2.mean(axis=0)
    print("inclusion frequency at key_bits = 2: mutation 0 %.3f, mutation %d %.3f" % (f[0], N - 1, f[-1]))
    assert f[0] - f[-1] > 0.15 and f[:5].mean() > 0.45 and f[-5:].mean() < 0.30


def test_unchanged_samples_have_uniform_p_values_and_planted_changes_are_found():
    """40 samples whose two sets come from one mixture, 4 whose set b carries an extra 50 % of signature 0; N = 600 per set, B = 39, so p lies
    on the grid k / 40.  Under H0 p is uniform on it: #{p <= 0.25} is Binomial(40, 0.25) = 10 +- 2.7, asserted within [2, 19] (3.2 sd: both
    tails below 1e-3), and the mean of p is 0.5125 +- 0.0456, asserted within 3 sd.  The planted samples are found at the level 0.05, and
    so is signature 0 in them by the adjusted per-signature p-value."""
    c, changed = CR.planted_corpus()
    o = CR.compare(c)
    assert (o.status == 0).all()
    p = (1.0 + o.count_ge) / (c.B + 1.0)
    same = ~changed
    k = int((p[same] <= 0.25).sum())
    print("unchanged: #{p <= 0.25} = %d of %d, mean p %.3f; planted p %s" % (k, same.sum(), p[same].mean(), p[changed]))
    assert 2 <= k <= 19
    assert abs(p[same].mean() - 0.5125) <= 3 * 0.0456
    assert (p[changed] <= 0.05).all()
    p_adj = (1.0 + o.count_max) / (c.B + 1.0)
    assert (p_adj[changed, 0] <= 0.05).all()
    assert (o.count_max >= o.count_sig).all()            # the maximum is at least every single difference: the adjusted p is never smaller
    assert (o.w_b[changed, 0] > o.w_a[changed, 0]).all()


@pytest.mark.parametrize("key_bits", CR.KEY_BITS)
@pytest.mark.parametrize("i", range(len(CR.SHAPES)), ids=lambda i: CR.corpora()[i].name)
def test_no_comparison_of_the_gpu_corpora_is_near_a_tie(i, key_bits):
    """count_ge compares values that hold a device log; two implementations agree on it as an integer where no T_b is near T_obs.  For every
    corpus of tests/test_compare_gpu.py, on the scale of the likelihood ratio (Λ = 2 (T - ll_0)): a replicate either deals the observed
    partition again (or its mirror image where N_a = N_b) -- then T_b = T_obs bit for bit in any implementation, the same operations on the
    same operands -- or |Λ_b - Λ_obs| >= 1e-6 max(1, Λ_obs), the margin of tests/test_presence_cpu.py.  The rounding bounds are below 1e-7.
    The exception is a sample with ONE allowed signature (all of C1V5): every fit is w = 1, T = Σ_v n_v log P_v whatever the partition, and the
    replicates differ from T_obs by rounding alone (asserted: within the bounds) -- the GPU test leaves count_ge of such samples out.
    Smallest gaps found (seeds of compare_ref), key_bits 32 / 3: C3V64 3.6e-2 / 5.5e-3, C33V96 7.0e-3 / 0.22, C70V130 4.9e-2 / 9.6e-2."""
    c = CR.corpora()[i]
    o = CR.reference(c, key_bits)
    tested = o.status == 0
    assert tested.sum() >= 5 and (o.status[~tested] == 3).all() and (~tested).sum() == 3
    lam_obs = 2.0 * (o.t_obs - o.ll_pool)
    gap = np.abs(o.rep - lam_obs[None, :]) / np.maximum(1.0, lam_obs)[None, :]
    free = (tested & (o.n_allowed > 1))[None, :] & ~o.rep_same
    one = (tested & (o.n_allowed == 1))[None, :].repeat(c.B, axis=0)
    assert (np.abs(o.rep - lam_obs[None, :])[one] <= (o.rep_bound + o.bound[None, :])[one]).all()
    print("%s key_bits %d: smallest |Λ_b - Λ_obs| / max(1, Λ_obs) %.3g over %d replicates (%d deal the observed partition); largest bound %.3g"
          % (c.name, key_bits, gap[free].min() if free.any() else np.nan, free.sum(), (o.rep_same & tested[None, :]).sum(), np.nanmax(o.rep_bound)))
    assert (gap[free] >= 1e-6).all()
    assert (o.rep[o.rep_same] == lam_obs[None, :].repeat(c.B, axis=0)[o.rep_same]).all()
    assert max(np.nanmax(o.rep_bound), o.bound.max()) < 1e-7
    # the shapes do what they are there for
    assert o.N_a[0] == 260 and o.N_a[0] + o.N_b[0] > 1024 and o.N_a[2] == 1 and o.N_b[3] == 1 and o.N_a[4] + o.N_b[4] == 2
    assert (o.dealt.sum(axis=2)[:, tested] == o.N_a[tested][None, :]).all()
    if c.C == 1:
        assert not free.any()
        return
    assert o.unexplained[8] > 0 and o.status[8] == 0
    if key_bits == 3:       # ties at the threshold in essentially every replicate of every sample with more than a few mutations
        d = 0
        keys = CR.deal_words(o.N_a[d] + o.N_b[d], d, np.arange(c.B), c.seed, c.stream) >> np.uint64(29)
        cut = np.sort(keys, axis=1)[:, o.N_a[d] - 1]
        assert ((keys == cut[:, None]).sum(axis=1) > 1).all()


def test_arguments_are_checked_before_a_device_is_asked_for(mmm):
    rng = np.random.default_rng(0)
    cat = rng.dirichlet(np.ones(8), size=3)
    Xa = [np.array([[1, 4], [3, 2]]), np.array([[2, 5]])]
    Xb = [np.array([[2, 1]]), np.array([[2, 5], [8, 1]])]
    with pytest.raises(ValueError, match="need a seed"):
        mmm.compare_exposures(Xa, Xb, cat)
    with pytest.raises(ValueError, match="2\\^31"):
        mmm.compare_exposures(Xa, Xb, cat, B=5, b0=2 ** 31 - 3, seed=1)
    with pytest.raises(ValueError, match="stream"):
        mmm.compare_exposures(Xa, Xb, cat, B=5, seed=1, stream=2 ** 31)
    with pytest.raises(ValueError, match="X_b holds term 9"):
        mmm.compare_exposures(Xa, [np.array([[9, 1]]), Xb[1]], cat, seed=1)
    with pytest.raises(ValueError, match="X_a holds 2 samples, X_b 1"):
        mmm.compare_exposures(Xa, Xb[:1], cat, seed=1)
    with pytest.raises(ValueError, match="limit 4096"):
        mmm.compare_exposures(Xa, Xb, np.ones((2, 4097)), seed=1)
    with pytest.raises(ValueError, match="limit 256"):
        mmm.compare_exposures(Xa, Xb, np.ones((257, 8)), seed=1)
    with pytest.raises(ValueError, match="maxiter"):
        mmm.compare_exposures(Xa, Xb, cat, seed=1, maxiter=0)
    with pytest.raises(ValueError, match="allowed"):
        mmm.compare_exposures(Xa, Xb, cat, seed=1, allowed=np.ones((3, 3)))
    with pytest.raises(ValueError, match="without names"):
        mmm.compare_exposures(Xa, Xb, cat, seed=1, allowed=["A"])
    for kind in (mmm.ILDA, mmm.IMMCTM):
        with pytest.raises(TypeError, match="factorised"):
            mmm.compare_exposures(Xa, Xb, object.__new__(kind), seed=1)
    with pytest.raises(ValueError, match="n_a"):
        mmm.deal_counts(Xa, [7, 1], 3, seed=1)
    with pytest.raises(ValueError, match="n_a"):
        mmm.deal_counts(Xa, [1], 3, seed=1)
    with pytest.raises(ValueError, match="V = 2"):
        mmm.deal_counts(Xa, [1, 1], 3, seed=1, V=2)
    with pytest.raises(ValueError, match="2\\^31"):
        mmm.deal_counts(Xa, [1, 1], -1, seed=1)
    assert {"compare_exposures", "deal_counts", "ComparisonResult"} <= set(mmm.__all__)
    assert {"mmm_compare_exposures", "mmm_deal_counts"} <= set(mmm._lib.declared_symbols())
    p = np.array([0.01, np.nan, 0.5, 0.02])
    padj = np.array([[0.5, np.nan, 0.01, 0.04], [0.03, np.nan, 0.9, np.nan]])
    r = mmm.ComparisonResult(p, *[None] * 6, padj, *[None] * 8, ["S1", "S2"])
    assert r.changed(0.05).tolist() == [0, 3]
    assert r.changed_signatures(0.05) == [(0, "S2"), (2, "S1"), (3, "S1")]
    q = r.q
    assert np.isnan(q[1]) and np.allclose(q[[0, 2, 3]], [0.03, 0.5, 0.03])
