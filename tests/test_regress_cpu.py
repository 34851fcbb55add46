"""The definition of mmm_regress_exposures as its numpy restatement computes it (tests/regress_ref.py), held to outside facts: the published
Philox vector, permutations that keep every stratum, the nested-model F and the OLS t of np.linalg.lstsq, the literal Freedman-Lane refit of
fitted part + permuted residuals, the rank statistics of mmm_associate_exposures when nothing is adjusted for, planted effects found and a
confounded covariate left alone once the confounder is adjusted for, the type-I error under confounding; then the host side of the Python
layer: every refusal, the design built by hand, the reported columns and Benjamini-Hochberg by hand."""
import numpy as np
import pytest

import associate_ref as A
import regress_ref as R


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    z = np.zeros(1, np.uint64)
    assert [int(v[0]) for v in R.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = z + np.uint64(0xFFFFFFFF)
    assert [int(v[0]) for v in R.philox4x32_10(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    pi = int("243F6A88", 16), int("85A308D3", 16), int("13198A2E", 16), int("03707344", 16)
    got = R.philox4x32_10(*[z + np.uint64(v) for v in pi], int("A4093822", 16), int("299F31D0", 16))
    assert [int(v[0]) for v in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_the_counter_word_is_this_call_s_own():
    """the keys differ from those of mmm_associate_exposures under the same seed, replicate and stream: only the second counter word differs"""
    assert R.BITS == 0xF0000000 and A.BITS == 0xE0000000
    assert not np.array_equal(R.keys(9, [3], 5)[0], A.keys(9, 3, 5, 0))
    z = np.zeros(1, np.uint64)
    want = R.philox4x32_10(z + np.uint64(1), z + np.uint64(0xF0000000), z + np.uint64(3), z + np.uint64(2), 5, 1)
    assert R.keys(8, [3], 5 + (1 << 32), stream=2)[0, 4:8].tolist() == [int(v[0]) for v in want]


def test_pi_is_a_permutation_that_keeps_every_stratum():
    rng = np.random.default_rng(3)
    for D, strata in ((1, None), (9, None), (64, np.array([2, 0, 0] + [1] * 61)), (41, rng.integers(0, 4, size=41)[::-1] * 10), (30, np.arange(30)[::-1])):
        moved = 0
        for pi in R.permutations(D, strata, np.arange(20), 5):
            assert sorted(pi.tolist()) == list(range(D))
            if strata is not None:
                assert np.array_equal(np.asarray(strata)[pi], np.asarray(strata))
            moved += int((pi != np.arange(D)).sum())
        alone = strata is not None and len(set(np.asarray(strata).tolist())) == D
        assert (moved == 0) == (D == 1 or alone)


def _cohort(seed, D=50, P=3):
    """two adjusters (one numeric, one of two levels) that drive the features, a numeric and a 3-level tested covariate"""
    rng = np.random.default_rng(seed)
    age, site = rng.standard_normal(D), rng.integers(0, 2, size=D).astype(np.float64)
    num, fac = 0.5 * age + rng.standard_normal(D), rng.integers(0, 3, size=D)
    x = rng.standard_normal((D, P)) + age[:, None] - 0.7 * site[:, None]
    x[:, 0] += 0.8 * num
    x[:, 1] += 0.9 * (fac == 2)
    Z = np.stack([np.ones(D), age, site], axis=1)
    return x, Z, [num[:, None], R.indicators(fac)]


def _rss(M, y):
    r = y - M @ np.linalg.lstsq(M, y, rcond=None)[0]
    return (r * r).sum(axis=0)


def test_t_is_the_partial_r2_and_gives_the_nested_model_F():
    for seed in (1, 2, 3):
        x, Z, blocks = _cohort(seed)
        D, A = Z.shape
        e, qz, cols, w = R.design(x, Z, blocks)
        r = R.regress(e, qz, cols, w, None, 0, 0, 1)
        for c, blk in enumerate(blocks):
            k = blk.shape[1]
            rss0, rss1 = _rss(Z, x), _rss(np.concatenate([Z, blk], axis=1), x)
            F = ((rss0 - rss1) / k) / (rss1 / (D - A - k))
            t = r.obs[:, c]
            assert np.allclose((t / k) / ((1.0 - t) / (D - A - k)), F, rtol=1e-9, atol=1e-9), (seed, c)
            assert np.allclose(t, (rss0 - rss1) / rss0, rtol=1e-9, atol=1e-12)
        assert np.allclose(r.rz_obs, _rss(Z, x), rtol=1e-10)


def test_a_permuted_t_is_the_literal_freedman_lane_refit():
    """Y* = the fitted part of the reduced model + its permuted residuals; refit reduced and full model on Y*; partial R^2 of the covariate"""
    x, Z, blocks = _cohort(4)
    D, A = Z.shape
    e, qz, cols, w = R.design(x, Z, blocks)
    fitted = x - e
    strata = np.arange(D) % 3
    r = R.regress(e, qz, cols, w, strata, 6, 40, 9)
    for b in range(6):
        pi = R.permutation(D, strata, 40 + b, 9)
        ystar = fitted + e[pi]
        rss0 = _rss(Z, ystar)
        t = np.stack([(rss0 - _rss(np.concatenate([Z, blk], axis=1), ystar)) / rss0 for blk in blocks], axis=1)
        assert np.allclose(t.max(axis=0), r.maxstat[b], rtol=1e-9, atol=1e-12), b


def test_a_one_column_signed_t_is_the_ols_t_statistic():
    x, Z, blocks = _cohort(5)
    D, A = Z.shape
    e, qz, cols, w = R.design(x, Z, blocks)
    r = R.regress(e, qz, cols, w, None, 0, 0, 1)
    M = np.concatenate([Z, blocks[0]], axis=1)
    beta = np.linalg.lstsq(M, x, rcond=None)[0]
    s2 = _rss(M, x) / (D - A - 1)
    se = np.sqrt(s2 * np.linalg.inv(M.T @ M)[-1, -1])
    t = r.obs[:, 0]
    F = t / ((1.0 - t) / (D - A - 1))
    rv = blocks[0][:, 0] - qz @ (qz.T @ blocks[0][:, 0])
    sign = np.sign(r.u_obs[:, 0]) * np.sign(w[:, 0] @ rv)            # QR may have turned the column round
    assert np.allclose(sign * np.sqrt(F), beta[-1] / se, rtol=1e-9, atol=1e-9)
    assert np.allclose(r.u_obs[:, 0] / (w[:, 0] @ rv), beta[-1], rtol=1e-9, atol=1e-12)          # the coefficient, by Frisch-Waugh


def test_without_adjusters_ranks_give_the_statistics_of_associate_exposures():
    """the intercept alone and midranks: partial R^2 = Spearman's rho^2 of a numeric covariate, (D - 1) partial R^2 = the tie-corrected
    Kruskal-Wallis H of a categorical one -- the restatement of mmm_associate_exposures is the outside fact"""
    try:
        import scipy.stats as st
    except ImportError:
        st = None
    rng = np.random.default_rng(12)
    for D, tied in ((7, False), (40, True), (133, True)):
        x = rng.standard_normal((D, 3))
        num, fac = rng.standard_normal(D), rng.integers(0, 3, size=D)
        if tied:
            x = np.round(x * 2.0) / 2.0
            x[rng.permutation(D)[:D // 2], 0] = 0.0
            num = np.round(num)
        rx = np.stack([R.midrank(x[:, p]) for p in range(3)], axis=1)
        e, qz, cols, w = R.design(rx, np.ones((D, 1)), [R.midrank(num)[:, None], R.indicators(fac)])
        r = R.regress(e, qz, cols, w, None, 0, 0, 1)
        a = A.associate(x, (0, 3), np.stack([num, fac.astype(np.float64)], axis=1), None, 0, 0, 1)
        assert np.allclose(r.obs[:, 0], a.obs[:, 0], rtol=1e-12, atol=1e-12), (D, tied)
        assert np.allclose(r.obs[:, 1], a.obs[:, 1], rtol=1e-10, atol=1e-13), (D, tied)
        if st is not None:
            H = np.array([st.kruskal(*[x[fac == g, p] for g in range(3)]).statistic for p in range(3)])
            assert np.allclose((D - 1) * r.obs[:, 1], H, rtol=1e-10, atol=0), (D, tied)


def test_planted_effects_are_found_and_the_confounded_covariate_is_left_alone():
    """A condition on the inputs, which tests/test_regress_gpu.py relies on.  numpy seed 4, Philox seed 1004, B = 999, on the restatement alone:
    exactly (0, grp) and (1, num) have p_adj <= 0.01 (0.001 each) and <= 0.05; conf has p_adj >= 0.578 on every feature when age is adjusted for
    and 0.001 on the features 0 .. 2 when it is not"""
    _, cov, _, pairs = R.planted()
    r, free = R.planted_reference(True), R.planted_reference(False)
    p_adj, p_free = (1.0 + r.ge_max) / (1.0 + R.PLANTED_B), (1.0 + free.ge_max) / (1.0 + R.PLANTED_B)
    print(np.round(p_adj, 3), np.round(p_free[:, 3], 3))
    assert list(cov) == ["grp", "num", "batch", "conf"]
    for alpha in (0.01, 0.05):
        assert sorted((int(i), int(j)) for i, j in np.argwhere(p_adj <= alpha)) == sorted(pairs), alpha
    assert (p_adj[:, 3] > 0.05).all() and (p_free[:3, 3] <= 0.001).all()
    assert (r.ge_max >= r.ge).all()


def test_type_one_error_under_confounding():
    """400 null cohorts (numpy seeds 5000 .. 5399, Philox seed = the same number) of D = 60 in which the adjuster drives the feature and the
    tested covariate, B = 199, alpha = 0.05: the rejection rate must lie in [0.02, 0.09], the 99.9 % binomial range around 0.05.  Observed on
    the restatement: 0.0575.  Without the adjuster the first cohort alone is rejected at p = 0.005."""
    rejected = 0
    for k in range(400):
        e, qz, cols, w = R.confounded_inputs(5000 + k)
        r = R.regress(e, qz, cols, w, None, R.CONFOUNDED_B, 0, 5000 + k)
        rejected += int((1.0 + r.ge[0, 0]) / (1.0 + R.CONFOUNDED_B) <= 0.05)
    rate = rejected / 400.0
    print("rejection rate", rate)
    assert 0.02 <= rate <= 0.09, rate
    e, qz, cols, w = R.confounded_inputs(5000, adjusted=False)
    assert (1.0 + R.regress(e, qz, cols, w, None, R.CONFOUNDED_B, 0, 5000).ge[0, 0]) / (1.0 + R.CONFOUNDED_B) <= 0.01


def test_the_case_table_holds_what_it_promises():
    cs = {c.name: c for c in R.cases()}
    A_of = lambda c: 0 if c.qz is None else c.qz.shape[1]
    assert {c.e.shape[0] for c in cs.values()} >= {2, 15, 16, 17, 63, 64, 65, 257, 4096} and {c.e.shape[1] for c in cs.values()} >= {1, 33, 64}
    assert {A_of(c) for c in cs.values()} >= {0, 1, 32} and cs["D2"].qz is None and cs["D4096"].e.shape[1] == 2
    assert {c.cols for c in cs.values()} >= {(1,), (1, 2, 1), (31, 33), (1,) * 64} and cs["many"].B == 3000
    for c in cs.values():
        assert all(c.e.shape[0] - A_of(c) - k >= 1 for k in c.cols) and c.w.shape == (c.e.shape[0], sum(c.cols)), c.name
    c = cs["contents"]
    r = R.reference(c)
    assert (c.e[:, 1] == 0).all() and (r.obs[1] == 0).all() and (c.w[:, 2] == 0).all() and (r.u_obs[:, 2] == 0).all()
    assert np.abs(c.qz.T @ c.e[:, 2]).max() > 0.2 and abs(r.rz_obs[3]) < 1e-14
    neg = R.reference(cs["rzneg"])
    assert neg.rz_obs[0] < 0 and (neg.obs[0] == 0).all() and (neg.ge[0] == cs["rzneg"].B).all() and (neg.obs[1:] > 0).all()
    alone = R.reference(cs["allalone"])
    assert (alone.ge == cs["allalone"].B).all() and (alone.ge_max == cs["allalone"].B).all()         # every pi is the identity
    assert sorted(set(cs["sizes"].strata.tolist())) == [0, 1, 2] and np.bincount(cs["sizes"].strata).tolist() == [2, 61, 1]


# ---- the Python layer, host side ---------------------------------------------------------------------------------------------------------------
def _inputs(mmm, x, cov, adj, ranks, kinds=None, akinds=None):
    D = x.shape[0]
    names, y, levels, _ = mmm.associate._covariates(cov, kinds, None, D)
    if adj:
        an, ay, al, _ = mmm.associate._covariates(adj, akinds, None, D)
    else:
        an, ay, al = [], np.zeros((D, 0)), np.zeros(0, dtype=np.int32)
    return mmm.regress._design(x, y, levels, names, ay, al, an, ranks)


def test_the_design_is_what_one_builds_by_hand(mmm):
    rng = np.random.default_rng(21)
    D = 30
    x = rng.random((D, 4))
    x[rng.permutation(D)[:18], 1] = 0.0
    x[:, 2] = 0.25                                                       # a constant feature
    age, site = np.round(rng.uniform(30, 80, size=D)), np.array(["a", "b", "c"])[np.arange(D) % 3]
    x[:, 3] = 2.0 * age - 1.0 + (site == "b")                            # explained by the adjusters (ranks=False)
    cov = {"brca": rng.integers(0, 2, size=D).astype(bool), "burden": rng.standard_normal(D), "grade": rng.integers(0, 3, size=D)}
    for ranks in (True, False):
        d = _inputs(mmm, x, cov, {"age": age, "site": site}, ranks)
        rk = R.midrank if ranks else (lambda v: np.asarray(v, np.float64))
        Z = np.stack([np.ones(D), rk(age), (site == "b").astype(float), (site == "c").astype(float)], axis=1)
        blocks = [cov["brca"].astype(float)[:, None], rk(cov["burden"])[:, None], R.indicators(cov["grade"])]
        e, qz, cols, w = R.design(np.stack([rk(x[:, p]) for p in range(4)], axis=1), Z, blocks)
        assert d["cols"].dtype == np.int32 and d["cols"].tolist() == [1, 1, 2] == cols and d["qz"].shape == (D, 4) and d["w"].shape == (D, 4)
        full = np.concatenate([d["qz"], d["w"][:, :1]], axis=1)
        assert np.allclose(full.T @ full, np.eye(5), atol=1e-13) and np.allclose(d["w"][:, 2:].T @ d["w"][:, 2:], np.eye(2), atol=1e-13)
        assert np.allclose(d["qz"].T @ d["w"], 0.0, atol=1e-13)
        assert np.allclose(d["qz"] @ d["qz"].T, qz @ qz.T, atol=1e-12)                          # the same adjustment space
        col0 = [0, 1, 2, 4]
        for c in range(3):
            mine, theirs = d["w"][:, col0[c]:col0[c + 1]], w[:, col0[c]:col0[c + 1]]
            assert np.allclose(mine @ mine.T, theirs @ theirs.T, atol=1e-12), c                 # the same space per covariate
        assert np.allclose(d["qz"][:, 0], 1.0 / np.sqrt(D)) and (d["w"][:, 0] @ blocks[0][:, 0]) > 0       # Gram-Schmidt keeps the direction
        assert np.allclose(d["e"][:, :2], e[:, :2], atol=1e-11) and (d["e"][:, 2] == 0).all()
        assert (d["e"][:, 3] == 0).all() if not ranks else np.abs(d["e"][:, 3]).max() > 0
        rv = blocks[1][:, 0] - qz @ (qz.T @ blocks[1][:, 0])
        assert np.isclose(d["scale"][1], np.linalg.norm(rv), rtol=1e-12) and np.isnan(d["scale"][2])
    none = _inputs(mmm, x, cov, None, True)
    assert none["qz"].shape == (D, 1) and np.allclose(none["e"][:, 0], R.midrank(x[:, 0]) - (D + 1) / 2.0, atol=1e-12)


def test_the_report_by_hand(mmm):
    """p = (1 + ge) / (1 + B); F from the partial R^2; t and coef from u_obs for one-column covariates; Benjamini-Hochberg over all P C"""
    D, B = 20, 9
    d = dict(cols=np.array([1, 2], dtype=np.int32), qz=np.zeros((D, 3)), scale=np.array([4.0, np.nan]))
    r = dict(obs=np.array([[0.5, 0.2], [0.1, 0.0]]), u_obs=np.array([[-2.0, 1.0, 1.0], [1.0, 0.0, 0.0]]), ge=np.array([[0, 3], [2, 9]], dtype=np.uint32),
             ge_max=np.array([[0, 4], [5, 9]], dtype=np.uint32))
    out = mmm.regress._report(r, d, D, B, ["a", "b"], [None, np.array([0, 1, 2])])
    assert out.df.tolist() == [[1, 16], [2, 15]] and out.permutations == B and out.names == ["a", "b"]
    assert np.allclose(out.F, [[0.5 / (0.5 / 16), (0.2 / 2) / (0.8 / 15)], [0.1 / (0.9 / 16), 0.0]], rtol=1e-15)
    assert np.allclose(out.t[:, 0], [-np.sqrt(16.0), np.sqrt(16.0 / 9.0)], rtol=1e-15) and np.isnan(out.t[:, 1]).all()
    assert out.coef[:, 0].tolist() == [-0.5, 0.25] and np.isnan(out.coef[:, 1]).all()
    assert out.p.tolist() == [[0.1, 0.4], [0.3, 1.0]] and out.p_adj.tolist() == [[0.1, 0.5], [0.6, 1.0]]
    # sorted 0.1, 0.3, 0.4, 1.0 times 4 / rank = 0.4, 0.6, 1.6 / 3, 1.0; running minimum from the right: 0.4, 1.6 / 3, 1.6 / 3, 1.0
    assert np.allclose(out.q, [[0.4, 1.6 / 3], [1.6 / 3, 1.0]], rtol=1e-15) and np.allclose(out.q.ravel(), A.bh(out.p.ravel()), rtol=1e-14)
    assert out.significant(0.1) == [(0, 0)] and out.significant(0.4, adjusted=False) == [(0, 0)]
    rows = out.table()
    assert len(rows) == 4 and rows[1] == dict(feature=0, covariate="b", partial_r2=0.2, F=out.F[0, 1], t=rows[1]["t"], coef=rows[1]["coef"], p=0.4, p_adj=0.5,
                                              q=out.q[0, 1]) and np.isnan(rows[1]["t"])


def test_python_argument_errors_need_no_device(mmm):
    class NoDevice:
        @property
        def h(self):
            raise AssertionError("a device was asked for")

    rng = np.random.default_rng(1)
    D = 20
    E = rng.uniform(0.1, 1.0, size=(D, 4))
    cov = {"g": rng.integers(0, 3, size=D), "v": rng.standard_normal(D)}
    adj = {"age": rng.standard_normal(D), "site": np.arange(D) % 2}
    nan = cov["v"].copy(); nan[3] = np.nan
    inf = cov["v"].copy(); inf[3] = np.inf
    none = np.array(["a", None] * 10, dtype=object)
    Enan = E.copy(); Enan[2, 1] = np.nan
    wide = {"f%d" % j: rng.standard_normal(D) for j in range(9)}
    bad = [dict(E=np.ones(5)), dict(E=np.ones((2, 3, 4))), dict(E=np.ones((4097, 1)), covariates=np.zeros((4097, 1)), adjust=None), dict(E=np.ones((20, 65))),
           dict(E=Enan), dict(covariates={"g": cov["g"], "v": nan}), dict(covariates={"v": inf}), dict(covariates={"s": none}), dict(covariates={}),
           dict(covariates={"g": cov["g"][:19]}), dict(covariates=np.zeros((20, 2)), names=["a"]), dict(kinds=["numeric"]), dict(kinds={"g": "ordinal"}),
           dict(adjust={"age": nan}), dict(adjust={"age": inf}), dict(adjust={"s": none}), dict(adjust={"age": adj["age"][:19]}), dict(adjust=np.zeros((20, 2, 2))),
           dict(adjust_kinds=["numeric"]), dict(adjust_kinds={"age": "ordinal"}), dict(adjust_kinds={"h": "numeric"}), dict(adjust=None, adjust_kinds=["numeric"]),
           dict(strata=np.zeros(19)), dict(strata=nan), dict(strata=none), dict(ranks="yes"), dict(ranks=1),
           dict(permutations=0), dict(permutations=2 ** 31), dict(permutations=2.5), dict(permutations="many"), dict(seed=-1), dict(seed=2 ** 64),
           dict(modalities=[0]),
           dict(E=np.ones((300, 1)), covariates={"id": np.arange(300)}, adjust=None),             # 299 tested columns
           dict(E=np.ones((300, 1)), covariates={"v": np.arange(300.0)}, adjust={"id": np.arange(300) % 40}),          # 40 adjustment columns
           dict(E=E[:12], covariates={"g": np.arange(12) % 3}, adjust={k: v[:12] for k, v in wide.items()})]            # 12 - 10 - 2 < 1
    for kw in bad:
        args = dict(E=E, covariates=cov, adjust=adj, permutations=5, ctx=NoDevice())
        args.update(kw)
        with pytest.raises(ValueError):
            mmm.regress_exposures(**args)
    call = lambda c, a, **kw: mmm.regress_exposures(E, c, a, permutations=5, ctx=NoDevice(), **kw)
    for col, name in ((nan, "v"), (none, "tumour type")):
        with pytest.raises(ValueError, match=name):
            call({"g": cov["g"], name: col}, adj)
        with pytest.raises(ValueError, match=name):
            call(cov, {"age": adj["age"], name: col})
    # collinear columns, each by its name
    with pytest.raises(ValueError, match="'twice'"):
        call({"g": cov["g"], "twice": 2.0 * adj["age"] + 1.0}, adj, ranks=False)
    with pytest.raises(ValueError, match="'same'"):
        call({"same": adj["site"]}, adj)
    with pytest.raises(ValueError, match="'flat'"):
        call({"flat": np.full(D, 3.5)}, adj)
    with pytest.raises(ValueError, match="'one'"):
        call({"one": np.zeros(D, dtype=int)}, adj)
    with pytest.raises(ValueError, match="adjuster 'again'"):
        call(cov, {"age": adj["age"], "again": 3.0 - adj["age"]}, ranks=False)
    with pytest.raises(ValueError, match="adjuster 'flat'"):
        call(cov, {"flat": np.full(D, 2.0)})
    with pytest.raises(ValueError, match="degrees of freedom"):
        mmm.regress_exposures(E[:12], {"g": np.arange(12) % 3}, {k: v[:12] for k, v in wide.items()}, permutations=5, ctx=NoDevice())
    # an adjuster of one level adds no column and is no error; the call then reaches the device
    with pytest.raises(AssertionError, match="a device was asked for"):
        call(cov, {"age": adj["age"], "centre": np.zeros(D, dtype=int)})
