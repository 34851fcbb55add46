"""What makes mmm_exposure_trajectory comparable between the device and its numpy restatement (tests/trajectory_ref.py), asserted on the
restatement alone: every comparison that decides an integer output of the cases the GPU tests use has operands of equal provenance or is
far from a tie; the case table reaches every condition the GPU tests are meant to run; the dynamic program is the brute force over all
partitions; the prefixes of a replicate are nested and are the shipped dealing; `bin_by_order` round-trips; the Python layer refuses every
bad argument without a device."""
import numpy as np
import pytest

import compare_ref as CR
import trajectory_ref as TR


@pytest.mark.parametrize("name,key_bits", TR.RUNS, ids=["%s-%d" % r for r in TR.RUNS])
def test_no_deciding_comparison_of_the_gpu_cases_is_near_a_tie(name, key_bits):
    """cut, n_cp, cp, count_ge and count_cut compare values that hold a device log.  Two implementations agree on them as integers where every
    deciding comparison either has operands of equal provenance (the same count vectors, added in the same order: equal bits in any
    deterministic implementation -- a replicate that deals the observed partition again, an empty bin between two cuts) or is apart by more
    than 10^3 times the sum of the two rounding bounds.  The only samples left out are those constructed with ONE allowed signature, where
    every partition has the same likelihood up to rounding: at most one per case."""
    o = TR.reference(name, key_bits)
    single = np.flatnonzero((o.n_allowed == 1) & (o.status != 3))
    assert single.size <= 1
    assert single.size == (1 if name in ("V1", "V129") else 0)
    seen = 0
    for chk in o.checks:
        if chk[0] in single:
            continue
        seen += 1
        assert TR.decided(chk), (name, chk[0], chk[1], chk[2], chk[5], chk[3] + chk[6])
    assert seen > 0 or name == "V1"


def test_the_case_table_reaches_every_condition():
    cases = [TR.case(n) for n in TR.SHAPES]
    refs = [TR.reference(n) for n in TR.SHAPES]
    assert {c.V for c in cases} >= {1, 7, 64, 65, 129, 200, 4096}
    assert {int(a) for o in refs for a in o.n_allowed} >= {0, 1, 2, 5, 33, 70}
    assert any(c.allowed is None for c in cases) and any(c.allowed is not None and (c.allowed.sum(axis=1) == 0).any() for c in cases)
    Ts = [[len(s) for s in c.bins] for c in cases]
    assert {t for T in Ts for t in T} >= {1, 2, 3, 5, 17, 128} and any(len(set(T)) >= 5 for T in Ts)
    assert {c.L for c in cases} == {1, 2, 3}
    assert {int(s) for o in refs for s in o.status} == {0, 1, 3}
    assert any(c.L > 1 and (o.status == 1).any() for c, o in zip(cases, refs))
    t128 = TR.case("T128")
    assert (t128.C, t128.V, t128.maxiter, t128.B, len(t128.bins[0])) == (3, 7, 50, 2, 128) and refs[-1].seg_ll.size == 8256
    N = np.array([n for c in cases[:-1] for d in range(len(c.bins)) for n in TR.dense_bins(c, d).sum(axis=1)])
    assert (N[:-1] > 1024).any() and (N == 0).any()
    assert set(TR.dense_bins(t128, 0).sum(axis=1)) == {1, 2, 3}
    v7 = TR.case("V7")
    sizes = [TR.dense_bins(v7, d).sum(axis=1).tolist() for d in range(len(v7.bins))]
    assert any(s[0] == 0 and s[-1] == 0 and 0 in s[1:-1] and sum(s) > 0 for s in sizes)             # empty first, middle and last bins
    assert any(sum(s) > 0 and sum(x > 0 for x in s) == 1 and len(s) > 1 for s in sizes)              # all mutations in one bin
    assert any(sum(s) == 0 for s in sizes)                                                           # N = 0
    assert any((o.unexplained > 0).any() for o in refs)
    assert any((o.n_cp >= 2).any() for o in refs) and sum(int((o.n_cp >= 1).sum()) for o in refs) >= 3
    v65 = refs[TR.SHAPES.index("V65")]
    assert v65.n_cp[1] == 2 and v65.cp[1, :2].tolist() == [6, 12]                                    # the planted changes are found where they are
    assert all(c.B == 24 for c in cases[:-1]) and TR.KEY_BITS == (32, 3)
    hot = np.flatnonzero(TR.case("V4096").cat.sum(axis=0))
    assert hot.size == 12


def test_the_dynamic_program_is_the_brute_force_over_all_partitions():
    rng = np.random.default_rng(7)
    for T in range(1, 8):
        for L in (1, 2, 3):
            for M in (0, 1, 2, 4):
                tab = -rng.uniform(1.0, 50.0, size=T * (T + 1) // 2) * rng.integers(1, 4, size=T * (T + 1) // 2)
                for i in range(T):
                    for j in range(i + 1, T + 1):
                        if not TR.defined(T, L, i, j):
                            tab[TR.seg_index(T, i, j)] = np.nan
                best, n_cp, cp = TR.partition(tab, T, L, M, pen=3.0)
                want = TR.brute_force(tab, T, L, M)
                assert np.array_equal(best, want, equal_nan=True), (T, L, M)
                assert np.isnan(best[min(M, max(T // L - 1, 0)) + 1:]).all() and not np.isnan(best[0])
                score = np.where(np.isnan(best), -np.inf, best - 3.0 * np.arange(M + 1))
                assert n_cp == int(np.argmax(score))
                b = [0] + cp[:n_cp].tolist() + [T]
                assert (cp[n_cp:] == -1).all() and all(TR.defined(T, L, b[k], b[k + 1]) for k in range(n_cp + 1))
                v = tab[TR.seg_index(T, b[0], b[1])]
                for k in range(1, n_cp + 1):
                    v = v + tab[TR.seg_index(T, b[k], b[k + 1])]
                assert v == best[n_cp]
    # ties go to the lowest i and to the smallest m
    T = 4
    tab = np.full(T * (T + 1) // 2, -1.0)
    best, n_cp, cp = TR.partition(tab, T, 1, 2, pen=0.0)
    assert best.tolist() == [-1.0, -2.0, -3.0] and n_cp == 0
    best, n_cp, cp = TR.partition(tab, T, 1, 2, pen=0.0)
    tab[TR.seg_index(T, 0, 4)] = -2.0
    best, n_cp, cp = TR.partition(tab, T, 1, 1, pen=0.0)
    assert n_cp == 0 and best.tolist() == [-2.0, -2.0]
    tab[TR.seg_index(T, 0, 4)] = -5.0
    best, n_cp, cp = TR.partition(tab, T, 1, 1, pen=0.0)
    assert n_cp == 1 and cp.tolist() == [1]


@pytest.mark.parametrize("key_bits", TR.KEY_BITS)
def test_prefixes_are_nested_sum_to_their_totals_and_are_the_dealing_of_the_two_set_test(key_bits):
    for name in ("V7", "V64"):
        c = TR.case(name)
        o = TR.reference(name, key_bits)
        assert o.prefixes
        for (d, b), pre in o.prefixes.items():
            T = len(c.bins[d])
            cuts = list(range(c.L, T - c.L + 1))
            pooled = TR.dense_bins(c, d).sum(axis=0)
            for t in cuts:
                assert pre[t].sum() == o.C_t[d][t] and (pre[t] >= 0).all() and (pre[t] <= pooled).all()
            for t, t2 in zip(cuts[:-1], cuts[1:]):
                assert (pre[t] <= pre[t2]).all(), (name, d, b, t)
            t = cuts[len(cuts) // 2]
            if o.C_t[d][t]:
                assert np.array_equal(pre[t], CR.deal_doc(pooled, int(o.C_t[d][t]), d, [b], c.seed, c.stream, key_bits)[0])


def test_bin_by_order_round_trips(mmm):
    rng = np.random.default_rng(3)
    terms = [rng.integers(1, 9, size=n) for n in (250, 7, 0, 100)]
    key = [rng.uniform(size=t.size) for t in terms]
    key[0][:10] = 0.5                                           # equal keys keep their input order
    tl = mmm.bin_by_order(terms, key, bin_size=100)
    assert [len(s) for s in tl] == [3, 1, 0, 1]
    assert [int(b[:, 1].sum()) for b in tl[0]] == [100, 100, 50] and int(tl[1][0][:, 1].sum()) == 7
    for d in range(4):
        o = np.argsort(-key[d], kind="stable")
        for t, b in enumerate(tl[d]):
            want = np.bincount(terms[d][o[100 * t:100 * (t + 1)]], minlength=9)
            got = np.zeros(9, np.int64); got[b[:, 0]] = b[:, 1]
            assert np.array_equal(got, want) and (b[:, 1] > 0).all() and (np.diff(b[:, 0]) > 0).all()
    up = mmm.bin_by_order(terms, key, bin_size=100, descending=False)
    first = np.zeros(9, np.int64); first[up[0][0][:, 0]] = up[0][0][:, 1]
    assert np.array_equal(first, np.bincount(terms[0][np.argsort(key[0], kind="stable")[:100]], minlength=9))
    whole = mmm.bin_by_order(terms, key, bin_size=10 ** 6)
    assert [len(s) for s in whole] == [1, 1, 0, 1]
    with pytest.raises(ValueError, match="bin_size"):
        mmm.bin_by_order(terms, key, bin_size=0)
    with pytest.raises(ValueError, match="keys"):
        mmm.bin_by_order(terms, [k[:-1] if k.size else k for k in key])
    with pytest.raises(ValueError, match="1-based"):
        mmm.bin_by_order([np.array([0, 1])], [np.array([0.1, 0.2])])
    with pytest.raises(ValueError, match="NaN"):
        mmm.bin_by_order([np.array([1, 1])], [np.array([0.1, np.nan])])


def test_arguments_are_checked_before_a_device_is_asked_for(mmm):
    rng = np.random.default_rng(0)
    cat = rng.dirichlet(np.ones(8), size=3)
    tl = [[np.array([[1, 4], [3, 2]]), np.array([[2, 5]])], [np.array([[2, 1]]), np.array([[2, 5], [8, 1]]), np.array([[1, 1]])]]
    f = mmm.exposure_trajectory
    with pytest.raises(ValueError, match="need a seed"):
        f(tl, cat)
    with pytest.raises(ValueError, match="2\\^31"):
        f(tl, cat, B=5, b0=2 ** 31 - 3, seed=1)
    with pytest.raises(ValueError, match="stream"):
        f(tl, cat, B=5, seed=1, stream=2 ** 31)
    with pytest.raises(ValueError, match="holds term 9"):
        f([[np.array([[9, 1]])], tl[1]], cat, seed=1)
    with pytest.raises(ValueError, match="limit 4096"):
        f(tl, np.ones((2, 4097)), seed=1)
    with pytest.raises(ValueError, match="limit 256"):
        f(tl, np.ones((257, 8)), seed=1)
    with pytest.raises(ValueError, match="limit 128"):
        f([[np.array([[1, 1]])] * 129], cat, seed=1)
    with pytest.raises(ValueError, match="maxiter"):
        f(tl, cat, seed=1, maxiter=0)
    with pytest.raises(ValueError, match="min_len"):
        f(tl, cat, seed=1, min_len=0)
    with pytest.raises(ValueError, match="max_changepoints"):
        f(tl, cat, seed=1, max_changepoints=-1)
    with pytest.raises(ValueError, match="penalty"):
        f(tl, cat, seed=1, penalty="aic")
    with pytest.raises(ValueError, match="penalty"):
        f(tl, cat, seed=1, penalty=[1.0, 2.0, 3.0])
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="negative or not finite"):
            f(tl, cat, seed=1, penalty=bad)
    with pytest.raises(ValueError, match="allowed"):
        f(tl, cat, seed=1, allowed=np.ones((3, 3)))
    with pytest.raises(ValueError, match="without names"):
        f(tl, cat, seed=1, allowed=["A"])
    with pytest.raises(ValueError, match="\\[D, T, V\\]"):
        f(np.ones((2, 8)), cat, seed=1)
    with pytest.raises(ValueError, match="integers"):
        f(np.full((2, 3, 8), 0.5), cat, seed=1)
    for kind in (mmm.ILDA, mmm.IMMCTM):
        with pytest.raises(TypeError, match="factorised"):
            f(tl, object.__new__(kind), seed=1)
    assert {"exposure_trajectory", "bin_by_order", "TrajectoryResult"} <= set(mmm.__all__)
    assert "mmm_exposure_trajectory" in set(mmm._lib.declared_symbols())
    # the result's helpers, on hand-made fields
    p = np.array([0.01, np.nan, 0.5, 0.02])
    fields = dict.fromkeys(mmm.TrajectoryResult._fields)
    fields.update(p=p, status=np.array([0, 3, 0, 0], np.int8), n_changepoints=np.array([1, 0, 0, 2], np.int32),
                  changepoints=np.array([[2, -1], [-1, -1], [-1, -1], [1, 3]], np.int32), bin_ptr=np.array([0, 4, 4, 6, 11]),
                  exposures_segment=[np.eye(2), np.zeros((1, 2)), np.ones((1, 2)), np.arange(6.0).reshape(3, 2)])
    r = mmm.TrajectoryResult(**fields)
    assert r.changed(0.05).tolist() == [0, 3]
    q = r.q
    assert np.isnan(q[1]) and np.allclose(q[[0, 2, 3]], [0.03, 0.5, 0.03])
    assert [(a, b) for a, b, _ in r.segments(0)] == [(0, 2), (2, 4)] and r.segments(1) == [] and [(a, b) for a, b, _ in r.segments(2)] == [(0, 2)]
    assert [(a, b) for a, b, _ in r.segments(3)] == [(0, 1), (1, 3), (3, 5)] and r.segments(3)[2][2].tolist() == [4.0, 5.0]
