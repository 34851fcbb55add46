"""The definition of mmm_associate_exposures as its numpy restatement computes it (tests/associate_ref.py), held to outside facts: the published
Philox vector, scipy's Kruskal-Wallis H and Spearman's rho, permutations that keep every stratum and are uniform, planted associations found
and null ones left alone, a confounder removed by strata; then the host side of the Python layer: every refusal, Benjamini-Hochberg by hand,
the reading of covariate columns."""
import itertools

import numpy as np
import pytest

import associate_ref as A


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    z = np.zeros(1, np.uint64)
    assert [int(v[0]) for v in A.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = z + np.uint64(0xFFFFFFFF)
    assert [int(v[0]) for v in A.philox4x32_10(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_statistic_is_kruskal_wallis_and_spearman():
    st = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(12)
    for D, tied in itertools.product((7, 40, 133), (False, True)):
        x = rng.standard_normal((D, 3))
        num = rng.standard_normal(D)
        if tied:
            x = np.round(x * 2.0) / 2.0
            x[rng.permutation(D)[:D // 2], 0] = 0.0
            num = np.round(num)
        y = np.stack([rng.integers(0, 3, size=D).astype(np.float64), num, rng.integers(0, 2, size=D).astype(np.float64)], axis=1)
        r = A.associate(x, (3, 0, 2), y, None, 0, 0, 1)
        Rx = np.stack([A.r2(x[:, p]) for p in range(3)], axis=1)
        ssx = ((Rx - (D + 1)) ** 2).sum(axis=0).astype(np.float64)
        ssy = float(((A.r2(num) - (D + 1)) ** 2).sum())
        for p in range(3):
            for c, G in ((0, 3), (2, 2)):
                H = st.kruskal(*[x[y[:, c] == g, p] for g in range(G)]).statistic
                assert np.isclose((D - 1) * r.obs[p, c], H, rtol=1e-12, atol=1e-12), (D, tied, p, c, (D - 1) * r.obs[p, c], H)
            rho = st.spearmanr(x[:, p], num).statistic
            assert np.isclose(r.zc_obs[p, 3] / np.sqrt(ssx[p] * ssy), rho, rtol=1e-12, atol=1e-12), (D, tied, p)
            assert np.isclose((D - 1) * r.obs[p, 1], (D - 1) * rho * rho, rtol=1e-12, atol=1e-12)


def test_midranks_are_the_definition():
    v = np.array([0.0, -0.0, 3.0, 3.0, 3.0, -1.0, 7.5])
    r = A.r2(v)
    assert r.tolist() == [5, 5, 10, 10, 10, 2, 14] and r.sum() == 7 * 8


def test_pi_is_a_permutation_that_keeps_every_stratum():
    rng = np.random.default_rng(3)
    for D, strata in ((1, None), (9, None), (64, np.array([2, 0, 0] + [1] * 61)), (41, rng.integers(0, 4, size=41)[::-1] * 10), (30, np.arange(30)[::-1])):
        moved = 0
        for b in range(20):
            pi = A.permutation(D, strata, b, 5)
            assert sorted(pi.tolist()) == list(range(D))
            if strata is not None:
                assert np.array_equal(np.asarray(strata)[pi], np.asarray(strata))
            moved += int((pi != np.arange(D)).sum())
        alone = strata is not None and len(set(np.asarray(strata).tolist())) == D
        assert (moved == 0) == (D == 1 or alone)


def test_the_six_orders_of_three_samples_are_equally_frequent():
    """6000 permutations, each order expected 1000 times with sd 29: between 880 and 1120 (seed 1 passes, checked on the restatement)"""
    count = {o: 0 for o in itertools.permutations(range(3))}
    for b in range(6000):
        count[tuple(A.permutation(3, None, b, 1).tolist())] += 1
    print(count)
    assert all(880 <= n <= 1120 for n in count.values()), count


def test_planted_associations_are_found_and_null_pairs_left_alone():
    """A condition on the inputs, which tests/test_associate_gpu.py relies on: with this seed the restatement alone gives the planted pairs
    p_adj <= 0.01 at B = 999 and no null pair p_adj below 0.05"""
    x, y, levels, pairs = A.planted()
    r = A.planted_reference()
    p_adj = (1.0 + r.ge_max) / (1.0 + A.PLANTED_B)
    print(np.round(p_adj, 3))
    for p in range(6):
        for c in range(3):
            if (p, c) in pairs:
                assert p_adj[p, c] <= 0.01, (p, c, p_adj[p, c])
            else:
                assert p_adj[p, c] >= 0.05, (p, c, p_adj[p, c])
    assert (r.ge_max >= r.ge).all() and (r.ge >= 0).all()


def test_strata_remove_a_confounder():
    x, y, levels, s = A.confounded()
    free = A.associate(x, levels, y, None, 999, 0, 11)
    held = A.associate(x, levels, y, s, 999, 0, 11)
    p_free, p_held = (1.0 + free.ge[0, 0]) / 1000.0, (1.0 + held.ge[0, 0]) / 1000.0
    print(p_free, p_held)
    assert np.array_equal(free.obs, held.obs) and p_free <= 0.001 and p_held > 0.05


def test_the_case_table_holds_what_it_promises():
    cs = {c.name: c for c in A.cases()}
    assert {c.x.shape[0] for c in cs.values()} >= {1, 2, 5, 63, 64, 65, 257, 4096} and {c.x.shape[1] for c in cs.values()} >= {1, 33, 256}
    assert sum(max(g, 1) for g in cs["Q256"].levels) == 256 and cs["Q1"].levels == (0,) and cs["many"].B == 3000
    c = cs["contents"]
    r = A.reference(c)
    assert (c.x[:, 0] == 0).mean() == 0.8 and (r.obs[1] == 0).all() and (r.obs[:, 1] == 0).all()          # the constant feature, the constant covariate
    assert not (c.y[:, 0] == 3).any() and np.signbit(c.x[:, 2]).any() and (c.x[:, 2] == 0).sum() > np.signbit(c.x[:, 2]).sum()
    assert (A.reference(cs["D1"]).obs == 0).all()
    alone = A.reference(cs["allalone"])
    assert (alone.ge == cs["allalone"].B).all() and (alone.ge_max == cs["allalone"].B).all()         # every pi is the identity


# ---- the Python layer, host side ---------------------------------------------------------------------------------------------------------------
def test_benjamini_hochberg_by_hand(mmm):
    """p = 0.01, 0.04, 0.03, 0.20: sorted 0.01, 0.03, 0.04, 0.20 times 4 / rank = 0.04, 0.06, 0.16 / 3, 0.20; running minimum from the right:
    0.04, 0.16 / 3, 0.16 / 3, 0.20"""
    q = mmm.associate.benjamini_hochberg(np.array([[0.01, 0.04], [0.03, 0.20]]))
    assert q.shape == (2, 2) and np.allclose(q, [[0.04, 0.16 / 3], [0.16 / 3, 0.20]], rtol=1e-15, atol=0)
    assert np.allclose(mmm.associate.benjamini_hochberg([0.9, 0.8, 0.7]), [0.9, 0.9, 0.9]) and np.allclose(mmm.associate.benjamini_hochberg([0.5]), [0.5])
    rng = np.random.default_rng(0)
    p = rng.random(37)
    assert np.allclose(mmm.associate.benjamini_hochberg(p), A.bh(p), rtol=1e-14, atol=0)


def test_covariate_columns_are_read_by_their_type(mmm):
    D = 6
    cov = {"sex": np.array(["f", "m", "f", "f", "m", "m"]), "age": np.array([31.0, 55.5, 47.0, 47.0, 60.0, 18.0]), "grade": np.array([3, 1, 2, 3, 3, 1]),
           "brca": np.array([True, False, False, True, False, False])}
    names, y, levels, values = mmm.associate._covariates(cov, None, None, D)
    assert names == ["sex", "age", "grade", "brca"] and levels.tolist() == [2, 0, 3, 2]
    assert y[:, 0].tolist() == [0, 1, 0, 0, 1, 1] and y[:, 1].tolist() == cov["age"].tolist() and y[:, 2].tolist() == [2, 0, 1, 2, 2, 0] and y[:, 3].tolist() == [1, 0, 0, 1, 0, 0]
    assert values[0].tolist() == ["f", "m"] and values[1] is None and values[2].tolist() == [1, 2, 3]
    _, y2, lv2, _ = mmm.associate._covariates(cov, {"grade": "numeric", "age": "categorical"}, None, D)
    assert lv2.tolist() == [2, 5, 0, 2] and y2[:, 2].tolist() == [3, 1, 2, 3, 3, 1]
    n3, y3, lv3, _ = mmm.associate._covariates(np.array([[0.5, 1.0], [0.25, 0.0], [1.5, 1.0]]), [None, "categorical"], ["a", "b"], 3)
    assert n3 == ["a", "b"] and lv3.tolist() == [0, 2] and y3[:, 1].tolist() == [1, 0, 1]
    assert mmm.associate._covariates(np.arange(4), None, None, 4)[2].tolist() == [4]
    for v in (np.array([0.0, -0.0, 3.0, 3.0, -1.0]), np.random.default_rng(1).integers(0, 5, size=50).astype(float)):
        assert np.array_equal(mmm.associate._midranks2(v), A.r2(v))


def test_python_argument_errors_need_no_device(mmm):
    class NoDevice:
        @property
        def h(self):
            raise AssertionError("a device was asked for")

    rng = np.random.default_rng(1)
    E = rng.uniform(0.1, 1.0, size=(20, 4))
    cov = {"g": rng.integers(0, 3, size=20), "v": rng.standard_normal(20)}
    nan = cov["v"].copy(); nan[3] = np.nan
    inf = cov["v"].copy(); inf[3] = np.inf
    none = np.array(["a", None] * 10, dtype=object)
    Enan = E.copy(); Enan[2, 1] = np.nan
    bad = [dict(E=np.ones(5)), dict(E=np.ones((2, 3, 4))), dict(E=np.ones((4097, 1)), covariates=np.zeros((4097, 1))), dict(E=np.ones((20, 257))), dict(E=Enan),
           dict(E=np.full((20, 2), np.inf)), dict(covariates={"g": cov["g"], "v": nan}), dict(covariates={"v": inf}), dict(covariates={"s": none}),
           dict(covariates={"g": cov["g"][:19]}), dict(covariates=np.zeros((20, 2, 2))), dict(covariates={}), dict(covariates=np.zeros((20, 2)), names=["a"]),
           dict(names=["a", "b"]), dict(kinds=["numeric"]), dict(kinds={"g": "ordinal"}), dict(kinds={"h": "numeric"}),
           dict(covariates={"s": np.array(["a", "b"] * 10)}, kinds=["numeric"]), dict(strata=np.zeros(19)), dict(strata=nan), dict(strata=none),
           dict(permutations=0), dict(permutations=2 ** 31), dict(permutations=2.5), dict(permutations="many"), dict(seed=-1), dict(seed=2 ** 64),
           dict(modalities=[0]), dict(E=np.ones((300, 1)), covariates={"id": np.arange(300)})]
    for kw in bad:
        args = dict(E=E, covariates=cov, permutations=5, ctx=NoDevice())
        args.update(kw)
        with pytest.raises(ValueError):
            mmm.associate_exposures(**args)
    for col, name in ((nan, "v"), (none, "tumour type")):
        with pytest.raises(ValueError, match=name):
            mmm.associate_exposures(E, {"g": cov["g"], name: col}, permutations=5, ctx=NoDevice())
