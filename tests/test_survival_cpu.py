"""The definition of mmm_survival_association as its numpy restatement computes it (tests/survival_ref.py), held to outside facts: the published
Philox vectors, the observed-minus-expected events of a textbook risk-set table, the sign of scipy's log-rank statistic, the exact mean and
variance of every kind of test column under the permutation, permutations that keep every stratum, the consequences the header lists,
planted effects found and null ones left alone, a confounder removed by strata; then the host side of the Python layer: the scores against
the restatement, every refusal, Kaplan-Meier by hand, Benjamini-Hochberg."""
import numpy as np
import pytest

import survival_ref as S

CASES = {c.name: c for c in S.cases()}
COUNTS = ("ge_trend", "gemax_trend", "ge_cut", "gemax_cut", "ge_group")
IDENTITY = ("obs_trend", "z_trend", "obs_group", "u_group", "obs_cut", "cut_at")


def _run(c, b0=None, B=None, seed=None):
    return S.survival(c.x, c.levels, c.groups, c.time, c.event, c.strata, c.m_lo, c.B if B is None else B, c.b0 if b0 is None else b0,
                      c.seed if seed is None else seed)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    z = np.zeros(1, np.uint64)
    assert [int(v[0]) for v in S.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = z + np.uint64(0xFFFFFFFF)
    assert [int(v[0]) for v in S.philox4x32_10(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    pi = [int(v[0]) for v in S.philox4x32_10(z + np.uint64(0x243f6a88), z + np.uint64(0x85a308d3), z + np.uint64(0x13198a2e), z + np.uint64(0x03707344), 0xa4093822, 0x299f31d0)]
    assert pi == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def _risk_set_table(time, event, group, g):
    """observed and expected events of group g, the textbook way: at every distinct event time, the events of the group, and the events of all
    times the group's share of those at risk"""
    O = E = 0.0
    for u in sorted({t for t, e in zip(time, event) if e}):
        at_risk = [i for i in range(len(time)) if time[i] >= u]
        dead = [i for i in at_risk if time[i] == u and event[i]]
        O += sum(1 for i in dead if group[i] == g)
        E += len(dead) * sum(1 for i in at_risk if group[i] == g) / len(at_risk)
    return O, E


def test_group_score_sums_are_observed_minus_expected():
    rng = np.random.default_rng(21)
    for D, tied, nstrata in ((9, False, 1), (40, True, 1), (57, False, 3), (80, True, 4)):
        time = rng.exponential(1.0, size=D)
        if tied:
            time = np.round(time, 1)
        event = (rng.random(D) < 0.7).astype(np.uint8)
        group = rng.integers(0, 3, size=D)
        strata = rng.integers(0, nstrata, size=D)
        a, A = S.scores(time, event, strata if nstrata > 1 else None)
        assert np.abs(A - a * 2.0 ** 24).max() <= 0.5 and abs(a.sum()) < 1e-10
        for g in range(3):
            O = E = 0.0
            for s in range(nstrata):
                m = strata == s
                o, e = _risk_set_table(time[m].tolist(), event[m].tolist(), group[m].tolist(), g)
                O, E = O + o, E + e
            assert abs(a[group == g].sum() - (O - E)) < 1e-10, (D, tied, nstrata, g)
            assert abs(A[group == g].sum() / 2.0 ** 24 - (O - E)) < D * 2.0 ** -24


def test_sign_agrees_with_scipy_logrank():
    st = pytest.importorskip("scipy.stats")
    if not hasattr(st, "logrank"):
        pytest.skip("scipy.stats.logrank is missing")
    rng = np.random.default_rng(22)
    for rate in (0.4, 2.5):
        D = 60
        g = rng.integers(0, 2, size=D)
        t_event = rng.exponential(1.0, size=D) / np.where(g == 1, rate, 1.0)
        t_cens = rng.exponential(2.0, size=D)
        time, event = np.minimum(t_event, t_cens), (t_event <= t_cens).astype(np.uint8)
        r = S.survival(np.zeros((D, 1)), (2,), g[:, None], time, event, None, 0, 0, 0, 1)
        cd = lambda m: st.CensoredData(uncensored=time[m & (event == 1)], right=time[m & (event == 0)])
        ref = st.logrank(cd(g == 1), cd(g == 0))               # positive when the first sample has more events than expected
        assert np.sign(r.u_group[1]) == np.sign(ref.statistic) == np.sign(rate - 1.0) and abs(int(r.u_group[0]) + int(r.u_group[1])) <= D // 2      # each A_i is within 1/2 of a_i 2^24


def test_moments_are_those_of_the_permutation_distribution():
    """N = 4000 permutations of D = 40 samples without strata.  T is a linear permutation statistic: its mean E and variance V are exact, so
    the empirical mean lies within 5 sqrt(V / N) of E.  The variance of the empirical variance is (kappa - 1) V^2 / N with kappa the kurtosis
    of T, and to first order kappa = 3 + g(f) g(A) / D, g the excess kurtosis of a column (Hoeffding's combinatorial central limit theorem
    with its 1 / D term): the empirical variance lies within 5 V sqrt((kappa - 1) / N) of V."""
    c = CASES["contents"]
    pl = S.Plan(c.x, c.levels, c.groups, c.time, c.event, None, 1)
    D, N = pl.D, 4000
    low = np.zeros(D, np.int64)
    low[pl.order[3][:17]] = 1
    cols = {"trend": (pl.Rx[:, 3], pl.Et[3], pl.Vt[3]), "group": (pl.ind[:, 5], pl.Eg[5], pl.Vg[5]), "cut": (low, pl.Ec[3][16], pl.Vc[3][16])}
    T = {k: np.zeros(N) for k in cols}
    for b in range(N):
        Api = pl.A[S.permutation(D, None, b, 77)]
        for k, (f, _, _) in cols.items():
            T[k][b] = float((f * Api).sum())
    excess = lambda v: float(((v - v.mean()) ** 4).mean() / ((v - v.mean()) ** 2).mean() ** 2 - 3.0)
    for k, (f, E, V) in cols.items():
        assert V > 0
        kappa = 3.0 + excess(f.astype(np.float64)) * excess(pl.A.astype(np.float64)) / D
        se_mean, se_var = np.sqrt(V / N), V * np.sqrt((kappa - 1.0) / N)
        print(k, (T[k].mean() - E) / se_mean, (T[k].var(ddof=1) - V) / se_var, kappa)
        assert abs(T[k].mean() - E) <= 5 * se_mean and abs(T[k].var(ddof=1) - V) <= 5 * se_var, k


def test_moments_with_strata_by_enumeration():
    """two strata of three: all 36 within-stratum permutations, the mean and variance of T exactly"""
    import itertools
    time, event = np.array([1.0, 2.0, 2.0, 3.0, 0.5, 4.0]), np.array([1, 1, 0, 1, 1, 0], np.uint8)
    strata = np.array([0, 1, 0, 1, 1, 0])
    x = np.array([0.3, 0.1, 0.9, 0.5, 0.2, 0.7])[:, None]
    pl = S.Plan(x, (2,), np.array([0, 1, 1, 0, 0, 1])[:, None], time, event, strata, 1)
    for f, E, V in ((pl.Rx[:, 0], pl.Et[0], pl.Vt[0]), (pl.ind[:, 1], pl.Eg[1], pl.Vg[1])):
        Ts = []
        for p0 in itertools.permutations([0, 2, 5]):
            for p1 in itertools.permutations([1, 3, 4]):
                pi = np.arange(6)
                pi[[0, 2, 5]], pi[[1, 3, 4]] = p0, p1
                Ts.append(float((f * pl.A[pi]).sum()))
        assert np.isclose(np.mean(Ts), E, rtol=1e-12) and np.isclose(np.var(Ts), V, rtol=1e-12)


def test_pi_is_a_permutation_that_keeps_every_stratum():
    rng = np.random.default_rng(3)
    for D, strata in ((1, None), (9, None), (64, np.array([2, 0, 0] + [1] * 61)), (41, rng.integers(0, 4, size=41)[::-1] * 10), (30, np.arange(30)[::-1])):
        moved = 0
        for b in range(20):
            pi = S.permutation(D, strata, b, 5)
            assert sorted(pi.tolist()) == list(range(D))
            if strata is not None:
                assert np.array_equal(np.asarray(strata)[pi], np.asarray(strata))
            moved += int((pi != np.arange(D)).sum())
        alone = strata is not None and len(set(np.asarray(strata).tolist())) == D
        assert (moved == 0) == (D == 1 or alone)


def test_the_consequences_the_header_lists():
    c = CASES["D65"]
    whole, head, tail = _run(c, b0=0, B=9), _run(c, b0=0, B=4), _run(c, b0=4, B=5)
    assert whole.maxstat[:4].tobytes() == head.maxstat.tobytes() and whole.maxstat[4:].tobytes() == tail.maxstat.tobytes()        # (b)
    for k in COUNTS:
        assert np.array_equal(getattr(whole, k), getattr(head, k) + getattr(tail, k)), k                                         # (c)
    other = _run(c, b0=100, B=2, seed=99)
    for k in IDENTITY:
        assert getattr(whole, k).tobytes() == getattr(other, k).tobytes(), k                                                      # (d)
    assert whole.maxstat[:2].tobytes() != other.maxstat.tobytes()
    for name in ("allalone", "censored"):                                                                                       # (e), (f)
        c = CASES[name]
        r = S.reference(c)
        assert all((getattr(r, k) == c.B).all() for k in COUNTS) and (r.maxstat == 0).all() and (r.cut_at == 0).all()
        assert all((getattr(r, k) == 0).all() for k in ("obs_trend", "obs_group", "obs_cut"))
    assert (S.scores(CASES["censored"].time, CASES["censored"].event)[1] == 0).all()


def test_the_case_table_holds_what_it_promises():
    cs = CASES
    assert {c.x.shape[0] for c in cs.values()} >= {1, 2, 5, 63, 64, 65, 257, 300, 4096} and {c.x.shape[1] for c in cs.values()} >= {1, 33, 256}
    assert sum(cs["Q256"].levels) == 256 and cs["C0"].levels == () and cs["many"].B == 3000 and cs["D4096"].m_lo == 0 and cs["D300"].m_lo == 30
    assert len(set(cs["strata64"].strata.tolist())) == 64 and sorted(np.bincount(cs["sizes"].strata).tolist()) == [1, 2, 61]
    c = cs["contents"]
    r = S.reference(c)
    assert (c.x[:, 0] == 0).mean() == 0.8 and r.obs_trend[1] == 0 and r.obs_cut[1] == 0 and r.cut_at[1] == 0                    # the constant feature
    assert not (c.groups[:, 0] == 3).any() and np.signbit(c.x[:, 2]).any() and (c.x[:, 2] == 0).sum() > np.signbit(c.x[:, 2]).sum()
    both = set(c.time[c.event == 1].tolist()) & set(c.time[c.event == 0].tolist())
    assert both and len(set(c.time.tolist())) < c.time.size                                                                    # events and censorings at one time
    assert len(set(cs["onetime"].time[cs["onetime"].event == 1].tolist())) == 1 and not cs["censored"].event.any()
    allowed = lambda c: [int((S.Plan(c.x, c.levels, c.groups, c.time, c.event, c.strata, c.m_lo).Vc[p] > 0).sum()) for p in range(c.x.shape[1])]
    assert allowed(c)[:2] == [8, 0] and max(allowed(cs["onecut"])) == 1 and allowed(cs["nocut"])[:2] == [0, 0] and cs["onecut"].m_lo == 20
    assert (S.reference(cs["D1"]).obs_trend == 0).all() and (S.reference(cs["D1"]).ge_cut == 5).all()


def test_planted_effects_are_found_and_null_ones_left_alone():
    """A condition on the inputs, which tests/test_survival_gpu.py relies on.  Of the seeds 4, 5 and 6 the restatement alone satisfies every
    condition at 5 and 6 (at 4 the cut of feature 1 has p_cut_adj = 0.033); seed 5 gives p_adj(trend 0) = 0.001, p_cut_adj(feature 1) = 0.001
    with cut_value 0.498 against the planted 0.5, p(group 0) = 0.004, every null feature's adjusted p >= 0.36 and the noise group's p = 0.216"""
    x, groups, levels, time, event = S.planted()
    r = S.planted_reference()
    B, D = S.PLANTED_B, x.shape[0]
    p_adj, p_cut_adj, p_group = (1.0 + r.gemax_trend) / (1.0 + B), (1.0 + r.gemax_cut) / (1.0 + B), (1.0 + r.ge_group) / (1.0 + B)
    print(np.round(p_adj, 3), np.round(p_cut_adj, 3), np.round(p_group, 3), r.cut_at)
    assert p_adj[0] <= 0.01 and p_cut_adj[1] <= 0.01 and p_group[0] <= 0.01
    assert (p_adj[2:] >= 0.05).all() and (p_cut_adj[2:] >= 0.05).all() and p_group[1] >= 0.05
    # the planted cut: cut_at is the number of samples at or below the cut; 0.5 has that rank within D / 6 (the central third)
    assert abs(int(r.cut_at[1]) - int((x[:, 1] <= 0.5).sum())) <= D // 6
    pl = S.Plan(x, levels, groups, time, event, None, S.PLANTED_MLO)
    assert r.z_trend[0] > pl.Et[0] and r.z_trend[1] > pl.Et[1] and r.u_group[1] > 0                         # more events than expected
    low1 = np.cumsum(pl.A[pl.order[1]])[r.cut_at[1] - 1]
    assert low1 < pl.Ec[1][r.cut_at[1] - 1]                                                                # the low group has fewer
    assert (r.gemax_trend >= r.ge_trend).all() and (r.gemax_cut >= r.ge_cut).all()


def test_strata_remove_a_confounder():
    x, time, event, s = S.confounded()
    free = S.survival(x, (), None, time, event, None, 0, 999, 0, 11)
    held = S.survival(x, (), None, time, event, s, 0, 999, 0, 11)
    p_free, p_held = (1.0 + free.ge_trend[0]) / 1000.0, (1.0 + held.ge_trend[0]) / 1000.0
    print(p_free, p_held)
    assert p_free <= 0.001 and p_held > 0.05


# ---- the Python layer, host side ---------------------------------------------------------------------------------------------------------------
def test_survival_scores_are_the_restatements(mmm):
    for c in S.cases():
        a, A = mmm.survival_scores(c.time, c.event, c.strata)
        ra, rA = S.scores(c.time, c.event, c.strata)
        assert a.tobytes() == ra.tobytes() and A.dtype == np.int32 and np.array_equal(A, rA), c.name
    # three samples by hand: events at 1 and 3, a censoring at 2: H = 1/3, 1/3, 1/3 + 1
    a, A = mmm.survival_scores([1.0, 2.0, 3.0], [1, 0, 1])
    assert np.allclose(a, [1 - 1 / 3, -1 / 3, 1 - 4 / 3], rtol=1e-15) and A.tolist() == [11184811, -5592405, -5592405]
    t, e = [3.0, 1.0, 2.0, 2.0, 5.0], [1, 1, 0, 1, 1]
    assert np.array_equal(mmm.survival_scores(t, e, ["b", "a", "b", "a", "b"])[1], mmm.survival_scores(t, e, [1, 0, 1, 0, 1])[1])
    for bad in (dict(time=[1.0, 2.0], event=[1, 0], strata=[0]), dict(time=[1.0, np.nan]), dict(time=[1.0, -2.0]), dict(event=[0, 2]), dict(event=[1])):
        kw = dict(time=[1.0, 2.0], event=[1, 0])
        kw.update(bad)
        with pytest.raises(ValueError):
            mmm.survival_scores(**kw)


def test_kaplan_meier_by_hand(mmm):
    """times 1, 2, 2+, 3, 4+, 5: S = 5/6 at 1 (6 at risk), 5/6 x 4/5 = 2/3 at 2 (5 at risk), 2/3 x 2/3 = 4/9 at 3 (3 at risk), 0 at 5 (1 at risk);
    the median is 3"""
    time, event = [1.0, 2.0, 2.0, 3.0, 4.0, 5.0], [1, 1, 0, 1, 0, 1]
    km = mmm.kaplan_meier(time, event)
    assert km.times.tolist() == [1.0, 2.0, 3.0, 5.0] and km.at_risk.tolist() == [6, 5, 3, 1] and km.median == 3.0
    assert np.allclose(km.survival, [5 / 6, 2 / 3, 4 / 9, 0.0], rtol=1e-15, atol=0)
    by = mmm.kaplan_meier(time, event, groups=["a", "b", "a", "b", "a", "b"])
    assert sorted(by) == ["a", "b"] and by["a"].times.tolist() == [1.0] and by["a"].median is None and np.allclose(by["a"].survival, [2 / 3])
    assert by["b"].times.tolist() == [2.0, 3.0, 5.0] and np.allclose(by["b"].survival, [2 / 3, 1 / 3, 0.0]) and by["b"].median == 3.0
    assert mmm.kaplan_meier([1.0, 2.0], [0, 0]).times.size == 0 and mmm.kaplan_meier([1.0, 2.0], [0, 0]).median is None
    with pytest.raises(ValueError, match="time"):
        mmm.kaplan_meier([1.0, np.nan], [1, 1])


def test_benjamini_hochberg_is_the_definition(mmm):
    p = np.random.default_rng(0).random(23)
    assert np.allclose(mmm.survival.benjamini_hochberg(p), S.bh(p), rtol=1e-14, atol=0)


def test_python_argument_errors_need_no_device(mmm):
    class NoDevice:
        @property
        def h(self):
            raise AssertionError("a device was asked for")

    rng = np.random.default_rng(1)
    D = 20
    E = rng.uniform(0.1, 1.0, size=(D, 4))
    time, event = rng.exponential(1.0, size=D), rng.integers(0, 2, size=D)
    grp = {"g": rng.integers(0, 3, size=D)}
    nan = time.copy(); nan[3] = np.nan
    none = np.array(["a", None] * 10, dtype=object)
    Enan = E.copy(); Enan[2, 1] = np.nan
    bad = [dict(E=np.ones(5)), dict(E=np.ones((2, 3, 4))), dict(E=np.ones((4097, 1))), dict(E=np.ones((D, 257))), dict(E=Enan), dict(time=nan), dict(time=-time),
           dict(time=time[:19]), dict(time=np.full(D, np.inf)), dict(time=none), dict(event=event[:19]), dict(event=event + 1), dict(event=nan), dict(event=none),
           dict(groups={"g": grp["g"][:19]}), dict(groups={"g": nan}), dict(groups={"g": none}), dict(groups=np.zeros((D, 2, 2))), dict(strata=np.zeros(19)),
           dict(strata=nan), dict(strata=none), dict(E=np.ones((130, 1)), time=np.ones(130), event=np.ones(130, int), groups=None, strata=np.arange(130)),
           dict(E=np.ones((300, 1)), time=np.ones(300), event=np.ones(300, int), groups={"id": np.arange(300)}), dict(min_fraction=0.6), dict(min_fraction=-0.1),
           dict(permutations=0), dict(permutations=2 ** 31), dict(permutations=2.5), dict(permutations="many"), dict(seed=-1), dict(seed=2 ** 64), dict(modalities=[0])]
    for kw in bad:
        args = dict(E=E, time=time, event=event, groups=grp, permutations=5, ctx=NoDevice())
        args.update(kw)
        with pytest.raises(ValueError):
            mmm.survival_association(**args)
    for kw, name in ((dict(time=nan), "time"), (dict(event=none), "event"), (dict(strata=none), "strata"), (dict(groups={"tumour type": none}), "tumour type")):
        args = dict(E=E, time=time, event=event, groups=grp, permutations=5, ctx=NoDevice())
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            mmm.survival_association(**args)
