"""The definition of mmm_cluster_samples as its numpy restatement computes it (tests/cluster_ref.py): it is textbook k-means from a k-means++
start, its start draws follow md / S, the case table the GPU tests share reaches every branch of the definition, planted groups come back with
PAC smallest at their number; the package's average linkage against scipy and against its tie rule; every refusal of the Python layer."""
import numpy as np
import pytest

import cluster_ref as C


def _textbook(X, cent, maxiter):
    """Lloyd's algorithm in np.longdouble with naive sums, from the given centres"""
    ld = np.longdouble
    X, cent = X.astype(ld), cent.astype(ld).copy()
    lab = np.full(X.shape[0], -1)
    for _ in range(maxiter):
        new = np.argmin(((X[:, None, :] - cent[None, :, :]) ** 2).sum(axis=2), axis=1)
        if (new == lab).all():
            break
        lab = new
        for c in range(cent.shape[0]):
            if (lab == c).any():
                cent[c] = X[lab == c].sum(axis=0) / ld((lab == c).sum())
    return lab, cent


@pytest.mark.parametrize("name", ["D65P3", "D130P33", "D257P1"])
def test_the_restatement_is_textbook_kmeans_from_the_same_start(name):
    """Labels equal; every centre entry within (m + 17) 2^-53 max|x| of the longdouble mean.  Derivation: with equal labels a centre is the mean
    of the same m <= n rows in both; the float64 sum passes every row through at most m + 16 additions (its stripe's, then the 16 stripe sums),
    each with relative error 2^-53 on a partial sum no larger than m max|x|, and the division adds one more rounding: the error of the mean is at
    most (m + 17) 2^-53 max|x| to first order (n <= 257 here, so second-order terms are below 2^-90); the longdouble side's own error,
    (m + 1) 2^-64 max|x|, is absorbed by taking n + 17 for m + 17."""
    c = next(v for v in C.cases() if v.name == name)
    D = c.x.shape[0]
    for b in range(2):
        mem = C.members(D, b, c.keep, c.seed, 0)
        X = c.x[mem]
        for k in c.ks:
            lab, it, _, cent, flags = C.kmeans(X, mem, k, b, c.seed, 0, 100)
            assert "settled" in flags
            chosen, _ = C.start(X, k, b, c.seed, 0)
            tl, tc = _textbook(X, X[chosen], 100)
            assert np.array_equal(lab, tl), (name, b, k)
            bound = (X.shape[0] + 17) * 2.0 ** -53 * np.abs(X).max()
            err = np.abs(cent.astype(np.longdouble) - tc).max()
            assert err <= bound, (name, b, k, float(err), bound)


def test_the_start_draws_follow_md_over_S():
    """k = 2 on six fixed points over N replicates: the first centre is uniform (floor(u n / 2^32)), the second is drawn with probability
    md_a / S given the first.  Every count within 5 standard deviations of its binomial (N, p_a) -- 12 counts, so a false alarm has probability
    below 12 x 6e-7."""
    X = np.array([[0.0], [1.0], [1.5], [4.0], [4.1], [9.0]])
    n, N = X.shape[0], 6000
    first = np.zeros(n); second = np.zeros(n)
    for b in range(N):
        ch, s0 = C.start(X, 2, b, 77, 3)
        assert not s0 and ch[0] != ch[1]
        first[ch[0]] += 1; second[ch[1]] += 1
    p2 = np.zeros(n)
    for f in range(n):
        md = C.dist(X, X[f])
        p2 += md / md.sum() / n
    for cnt, p in ((first, np.full(n, 1.0 / n)), (second, p2)):
        assert (np.abs(cnt - N * p) <= 5.0 * np.sqrt(N * p * (1.0 - p))).all(), (cnt, N * p)


def test_average_linkage_equals_scipy_on_tie_free_matrices(mmm):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    rng = np.random.default_rng(5)
    for D in (2, 7, 40, 90):
        pts = rng.standard_normal((D, 3))
        dm = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(axis=2))
        Z = hier.linkage(squareform(dm, checks=False), method="average")
        for k in sorted({1, 2, min(3, D), D // 2 + 1, D}):
            want = hier.fcluster(Z, k, criterion="maxclust")
            got = mmm.cluster.average_linkage(dm, k)
            assert got.max() + 1 == k and np.array_equal(got, C.upgma(dm, k)), (D, k)
            # the same partition: the groups of one are the groups of the other
            assert len(set(zip(got.tolist(), want.tolist()))) == k, (D, k)
            # numbered by their smallest member
            firsts = [int(np.flatnonzero(got == g)[0]) for g in range(k)]
            assert firsts == sorted(firsts)


def test_average_linkage_takes_the_lowest_pair_among_ties(mmm):
    """all distances equal: the closest pair is always the lowest (i, j) -- 0 and 1 merge first, then {0, 1} and 2 (its average distance ties
    with every other pair, and (0, 2) is the lowest), ..."""
    dm = np.ones((6, 6)) - np.eye(6)
    for k, want in ((5, [0, 0, 1, 2, 3, 4]), (4, [0, 0, 0, 1, 2, 3]), (2, [0, 0, 0, 0, 0, 1]), (1, [0] * 6)):
        assert mmm.cluster.average_linkage(dm, k).tolist() == want
        assert C.upgma(dm, k).tolist() == want
    # two tied pairs that are not neighbours: (1, 4) and (2, 3) at the same distance -> (1, 4) first
    dm = np.full((5, 5), 3.0); np.fill_diagonal(dm, 0.0)
    dm[1, 4] = dm[4, 1] = dm[2, 3] = dm[3, 2] = 1.0
    assert mmm.cluster.average_linkage(dm, 4).tolist() == [0, 1, 2, 3, 1]
    assert mmm.cluster.average_linkage(dm, 3).tolist() == [0, 1, 2, 2, 1]


@pytest.mark.parametrize("D,P,G,conc,seed", C.PLANTED)
def test_planted_groups_have_the_smallest_pac_and_come_back(D, P, G, conc, seed):
    """A condition on the inputs, which tests/test_cluster_gpu.py relies on: with these seeds the restatement alone puts the smallest PAC at
    k = G, by at least 0.05 over every other k in 2 .. G + 2, and its final labels at k = G are the planted groups (purity 1)."""
    x, truth = C.planted(D, P, G, conc, seed)
    ks = tuple(range(2, G + 3))
    r = C.planted_reference(D, P, G, conc, seed)
    pac = r.ambiguous / r.valid.astype(np.float64)
    print("PAC", dict(zip(ks, np.round(pac, 4))))
    g = ks.index(G)
    assert all(pac[i] >= pac[g] + 0.05 for i in range(len(ks)) if i != g), pac
    lab = C.upgma(1.0 - C.consensus(r.together[g], r.same[g]), G)
    assert len(set(zip(lab.tolist(), truth.tolist()))) == G


def test_the_case_table_reaches_every_branch():
    seen = set()
    for c in C.cases():
        if c.x.shape[0] > 300:
            continue                                    # the placement cases repeat the branches of the small ones
        r = C.reference(c)
        for fl in r.flags.values():
            seen |= fl
        if c.name == "D5P2keep":
            n = (r.labels[0] >= 0).sum(axis=1)          # k = 1 is skipped only where n = 0
            assert (n == 0).any() and ((n > 0) & (n < 3)).any()
        if c.name == "D12two":
            assert all({"s0", "empty"} <= fl for fl in r.flags.values())
        if c.name == "maxiter2":
            assert all("maxiter" in fl and "settled" not in fl for fl in r.flags.values())
        assert (r.same <= r.together).all()
    assert seen == {"skipped", "s0", "empty", "maxiter", "settled"}, seen
    assert any(c.x.shape[1] % 4 for c in C.cases())


def test_python_argument_errors_need_no_device(mmm):
    class NoDevice:
        @property
        def h(self):
            raise AssertionError("a device was asked for")

    E = np.random.default_rng(1).uniform(0.1, 1.0, size=(20, 4))
    bad = [dict(ks=[]), dict(ks=range(1, 18)), dict(ks=[2, 2]), dict(ks=[0]), dict(ks=[33]), dict(ks=[21]), dict(ks=[2.5]), dict(ks=3), dict(replicates=0),
           dict(replicates=2 ** 31), dict(subsample=0.0), dict(subsample=1.5), dict(subsample=np.nan), dict(seed=-1), dict(seed=2 ** 64),
           dict(metric="cosine"), dict(maxiter=0), dict(pac=(0.9, 0.1)), dict(pac=(0.5, 0.5)), dict(pac=(-0.1, 0.9)), dict(pac=(0.1, 1.1)), dict(pac=0.5),
           dict(pac=(0.1, 0.1004)), dict(k=9), dict(modalities=[0]), dict(E=np.ones(5)), dict(E=np.ones((2, 3, 4))), dict(E=np.ones((4097, 1))),
           dict(E=np.ones((3, 257))), dict(E=-E), dict(E=np.zeros((4, 2))), dict(E=np.full((4, 2), np.nan)), dict(E=np.full((4, 2), np.inf), metric="euclidean"),
           dict(E=np.full((4, 2), 1e151), metric="euclidean"), dict(ks=[2], replicates=2 ** 27)]
    for kw in bad:
        args = dict(E=E, ks=[2, 3], replicates=5, ctx=NoDevice())
        args.update(kw)
        with pytest.raises(ValueError):
            mmm.cluster_samples(**args)
    assert mmm.cluster._keep(1.0) == 0 and mmm.cluster._keep(0.8) == int(np.floor(0.8 * 2 ** 32)) and mmm.cluster._keep(1e-12) == 1
    assert mmm.cluster._pick(np.array([0.2, 0.1, np.nan, 0.1]), [5, 4, 2, 3]) == 3 and mmm.cluster._pick(np.array([np.nan, np.nan]), [3, 2]) == 1
    assert mmm.cluster._keep(1.0 - 2.0 ** -53) == 2 ** 32 - 1 and mmm.cluster._per_mille((0.1, 0.9)) == (100, 900)
