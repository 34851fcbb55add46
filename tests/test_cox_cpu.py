"""The numpy restatement of mmm_cox_exposures (tests/cox_ref.py) held to outside facts: Random123's Philox vectors, the permutation's and the
folds' structure, the log-rank scores of `survival_scores` at w = 0, scipy's minimisers of the penalised Breslow partial likelihood, a
triple-loop Harrell's C, the consequences the header lists, what the case table promises, a planted and a null outcome, and every refusal of
the Python layer (which needs no device)."""
import numpy as np
import pytest

import cox_ref as K

CASES = {c.name: c for c in K.cases()}


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    z = np.zeros(1, np.uint64)
    assert [int(v[0]) for v in K.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = z + np.uint64(0xFFFFFFFF)
    assert [int(v[0]) for v in K.philox4x32_10(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    pi = [int(v[0]) for v in K.philox4x32_10(z + np.uint64(0x243f6a88), z + np.uint64(0x85a308d3), z + np.uint64(0x13198a2e), z + np.uint64(0x03707344), 0xa4093822, 0x299f31d0)]
    assert pi == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    assert K.BITS == 0xB0000000                                          # bits 31, 29 and 28, without 30


def test_pi_is_a_permutation_that_keeps_every_stratum():
    rng = np.random.default_rng(3)
    for D, strata in ((2, None), (9, None), (64, np.array([2, 0, 0] + [1] * 61)), (41, rng.integers(0, 4, size=41)[::-1] * 10), (30, np.arange(30)[::-1])):
        moved = 0
        for b in range(20):
            pi = K.permutation(D, strata, b, 7)
            assert sorted(pi.tolist()) == list(range(D))
            if strata is not None:
                assert (strata[pi] == strata).all()
            moved += int((pi != np.arange(D)).sum())
        assert (moved == 0) == (strata is not None and len(set(strata.tolist())) == D)


def test_residuals_at_zero_are_the_log_rank_scores(mmm, oracle):
    """At w = 0 every u is 1, S0 is an exact integer (the size of the risk set) and M_i = event_i - Hhat_i is the log-rank score a_i of
    `survival_scores`; only the association of the hazard sum differs (chunks from the stratum's end here, one running sum there), so the
    bound is the a-priori rounding bound of a sum of at most D non-negative terms: D 2^-52 max Hhat."""
    rng = np.random.default_rng(4)
    for D, nstrata, decimals in ((40, 1, 1), (97, 1, 3), (130, 3, 1), (300, 4, 2)):
        time = np.round(rng.exponential(size=D), decimals)
        event = (rng.random(D) < 0.65).astype(np.uint8)
        strata = None if nstrata == 1 else rng.integers(0, nstrata, size=D)
        tb = K.tables(time, event, strata)
        assert decimals > 1 or tb.NG < D                                 # tied times
        z = rng.standard_normal((1, D, 2))[:, tb.ord]
        _, Hhat, _, M, _, _ = K.iteration_terms(z, np.zeros((1, 2)), np.ones((1, D), bool), event[tb.ord], tb)
        got = np.empty(D)
        got[tb.ord] = M[0]
        want = mmm.survival.survival_scores(time, event, strata)[0]
        bound = D * 2.0 ** -52 * Hhat.max()
        print("D %d, %d strata: max |M - a| = %.3g, bound %.3g" % (D, nstrata, np.abs(got - want).max(), bound))
        assert np.abs(got - want).max() <= bound


def _neg_log_pl(w, x, time, event, strata, lam):
    """the penalised negative Breslow log partial likelihood and its gradient, with plain loops"""
    D, P = len(x), len(x[0])
    eta = [sum(x[i][j] * w[j] for j in range(P)) for i in range(D)]
    val = 0.5 * lam * sum(v * v for v in w)
    grad = [lam * v for v in w]
    for i in range(D):
        if not event[i]:
            continue
        s0, s1 = 0.0, [0.0] * P
        for m in range(D):
            if strata[m] == strata[i] and time[m] >= time[i]:
                e = np.exp(eta[m])
                s0 += e
                for j in range(P):
                    s1[j] += e * x[m][j]
        val -= eta[i] - np.log(s0)
        for j in range(P):
            grad[j] -= x[i][j] - s1[j] / s0
    return val, np.array(grad)


def test_coefficients_are_scipys(oracle):
    """The all-sample fit against scipy.optimize.minimize of the penalised Breslow partial likelihood written above, with ties and strata, at
    three penalties.  The bound is measured here against scipy's own converged solutions: twice the largest difference BFGS and Newton-CG
    show between them on the same problem (printed; DESIGN.md section 4.22 records one run)."""
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(5)
    D, P = 60, 3
    x = rng.standard_normal((D, P))
    strata = rng.integers(0, 2, size=D)
    te = rng.exponential(size=D) / np.exp(0.8 * x[:, 0] - 0.5 * x[:, 2])
    tc = rng.exponential(size=D) * 1.5
    time, event = np.round(np.minimum(te, tc), 1), (te <= tc).astype(np.uint8)
    tb = K.tables(time, event, strata)
    assert tb.NG < D - 10                                                # tied times
    xl, tl, el, sl = x.tolist(), time.tolist(), event.tolist(), strata.tolist()
    for lam in (0.1, 1.0, 10.0):
        w, its, status = K.fit_batch(x[None], np.zeros(1, np.int64), event, np.ones((1, D), bool), np.array([lam]), tb, 30, 1e-12)
        assert status[0] == 0 and its[0] <= 12
        fun = lambda v: _neg_log_pl(v.tolist(), xl, tl, el, sl, lam)
        sp = {"BFGS": opt.minimize(fun, np.zeros(P), jac=True, method="BFGS", options=dict(gtol=1e-10, maxiter=10000)).x,
              "Newton-CG": opt.minimize(fun, np.zeros(P), jac=True, method="Newton-CG", options=dict(xtol=1e-14, maxiter=10000)).x}
        bound = 2.0 * np.abs(sp["BFGS"] - sp["Newton-CG"]).max()
        err = min(np.abs(w[0] - v).max() for v in sp.values())
        print("lambda %g: scipy's methods differ by %.3g, the restatement from the nearer by %.3g" % (lam, bound / 2, err))
        assert err <= bound, (lam, err, bound)


def test_u2_is_a_triple_loop_harrells_c():
    rng = np.random.default_rng(6)
    for D, nstrata in ((7, 1), (40, 2), (120, 3)):
        time = rng.integers(0, 8, size=D) / 2.0                          # tied times
        event = (rng.random(D) < 0.6).astype(np.uint8)
        event[:2] = (1, 0)
        time[:2] = (0.0, 0.5)
        strata = np.zeros(D, np.int64) if nstrata == 1 else np.r_[0, 0, rng.integers(0, nstrata, size=D - 2)]
        s = rng.integers(0, 6, size=D) / 4.0                             # tied scores; quarters are exact
        conc, pairs = 0.0, 0
        for code in range(nstrata):
            for i in range(D):
                for j in range(D):
                    if strata[i] != code or strata[j] != code or not event[i]:
                        continue
                    if time[j] > time[i] or (time[j] == time[i] and not event[j]):
                        pairs += 1
                        conc += 1.0 if s[i] > s[j] else (0.5 if s[i] == s[j] else 0.0)
        tb = K.tables(time, event, strata)
        assert tb.n_pairs == pairs > 0 and K.u2(s, tb.comparable) / (2.0 * tb.n_pairs) == conc / pairs
    tb = K.tables([1.0, 2.0, 3.0, 4.0], [1, 1, 1, 0], None)
    assert K.u2(np.array([np.nan, 1.0, 0.5, np.nan]), tb.comparable) == 2      # a NaN compares false: only (1.0, 0.5) counts


def test_folds_are_balanced_inside_every_cell(mmm):
    rng = np.random.default_rng(7)
    for D, nstrata, F, R in ((96, 1, 4, 2), (61, 3, 5, 3), (40, 2, 7, 1)):
        event = (rng.random(D) < 0.5).astype(np.uint8)
        s = None if nstrata == 1 else rng.integers(0, nstrata, size=D)
        fold = mmm.cox.make_folds(event, s, F, R, 11)
        assert fold.shape == (R, D) and fold.dtype == np.uint8 and fold.max() < F
        assert (fold == mmm.cox.make_folds(event, s, F, R, 11)).all() and (R == 1 or (fold[0] != fold[1]).any())
        for r in range(R):
            for code in range(nstrata):
                for c in (0, 1):
                    n = np.bincount(fold[r][(event == c) & ((s if s is not None else np.zeros(D, int)) == code)], minlength=F)
                    assert n.max() - n.min() <= 1
            assert np.bincount(fold[r], minlength=F).max() - np.bincount(fold[r], minlength=F).min() <= 1      # the deal goes on from cell to cell
            for f in range(F):
                assert event[fold[r] != f].any()


def test_comparable_pairs_of_the_python_layer(mmm):
    for c in CASES.values():
        assert mmm.cox.comparable_pairs(c.time, c.event, c.strata) == K.tables(c.time, c.event, c.strata).n_pairs, c.name


def test_the_consequences_the_header_lists(oracle):
    c = CASES["ties"]
    run = lambda **kw: K.cox(c.x, c.time, c.event, c.strata, c.fold, c.F, c.lambdas, c.maxiter, c.tol, kw.get("B", c.B), kw.get("b0", 0), kw.get("seed", c.seed),
                             kw.get("stream", 0))
    whole, head, tail = run(B=9), run(B=4), run(B=5, b0=4)
    assert whole.maxstat[:4].tobytes() == head.maxstat.tobytes() and whole.maxstat[4:].tobytes() == tail.maxstat.tobytes()        # (b)
    assert (whole.ge == head.ge + tail.ge).all() and (whole.gemax == head.gemax + tail.gemax).all() and (whole.events[2:] == head.events[2:] + tail.events[2:]).all()
    other = run(B=3, seed=99, stream=4)
    for k in ("scores", "u2_obs", "s_obs", "n_pairs", "coef", "full_iters"):                                                        # (d)
        assert getattr(other, k).tobytes() == getattr(whole, k).tobytes(), k
    assert (other.events[:2] == whole.events[:2]).all() and other.maxstat.tobytes() != whole.maxstat[:3].tobytes()
    assert (whole.gemax >= whole.ge).all() and (whole.s_obs == whole.u2_obs.sum(axis=0)).all()
    assert (whole.maxstat <= 2 * c.fold.shape[0] * whole.n_pairs[0]).all() and (whole.maxstat >= 0).all()
    none = run(B=0)                                                                                                                  # (c)
    assert none.maxstat.size == 0 and not none.ge.any() and none.s_obs.tobytes() == whole.s_obs.tobytes()


def test_the_case_table_holds_what_it_promises(oracle):
    cs = CASES
    assert {c.x.shape[0] for c in cs.values()} >= {4, 5, 17, 33, 65, 257, 300} and {c.x.shape[1] for c in cs.values()} >= {1, 33, 64}
    assert {c.lambdas.size for c in cs.values()} >= {1, 8} and {c.fold.shape[0] for c in cs.values()} >= {1, 3} and {c.F for c in cs.values()} >= {2, 5}
    assert all((c.B + 1) * c.fold.shape[0] * c.F * c.lambdas.size <= 2500 for c in cs.values())
    tbs = {n: K.tables(c.time, c.event, c.strata) for n, c in cs.items()}
    for n, c in cs.items():                                                  # every case is one the library accepts
        assert tbs[n].n_pairs > 0 and all(c.event[c.fold[r] != f].any() for r in range(c.fold.shape[0]) for f in range(c.F)), n
    assert cs["D4"].event.sum() == 2 and tbs["D5"].NC == 1 and tbs["D17"].NC == 2 and tbs["D257"].NC == 17 and cs["Fmin"].F == cs["Fmin"].event.sum() == 6
    t = tbs["tied_times"]                                                    # a tie group across the chunk edge, with events and censored samples
    g = int(np.flatnonzero((t.gstart < 16) & (t.gend >= 16))[0])
    members = cs["tied_times"].event[t.ord[t.gstart[g]:t.gend[g] + 1]]
    assert (t.gstart[g], t.gend[g]) == (13, 18) and 0 < members.sum() < members.size and t.cst.tolist() == [0, 16, 32, 40]
    assert cs["all_events"].event.all() and tbs["all_events"].NG < 30
    o = cs["one_event_stratum"]
    assert [int(o.event[o.strata == s].sum()) for s in (0, 1, 2)] == [10, 1, 0]
    assert np.bincount(cs["sizes"].strata).tolist() == [2, 61, 1] and tbs["sizes"].cst.tolist() == [0, 2, 18, 34, 50, 63, 64]
    assert tbs["sizes"].cfirst.tolist() == [True, True, False, False, False, True] and tbs["sizes"].clast.tolist() == [True, False, False, False, True, True]
    assert (np.diff(cs["unordered"].strata) < 0).any() and (np.diff(cs["unordered"].strata) > 0).any()
    place = {n: K.placement(c.x.shape[0], c.x.shape[1], tbs[n].NG, tbs[n].NC) for n, c in cs.items()}
    assert all(tbs[n].NG == 300 and tbs[n].NC == 19 for n in ("rows_lds", "rows_mem", "zbar_lds", "zbar_mem", "both_mem"))
    assert place["rows_lds"] == (True, True) and place["rows_mem"] == (False, True) and place["zbar_lds"] == (False, True) and place["zbar_mem"] == (True, False)
    assert place["both_mem"] == (False, False)
    assert [cs[n].x.shape[1] for n in ("rows_lds", "rows_mem", "zbar_lds", "zbar_mem")] == [10, 11, 19, 20]         # neighbours: the boundary lies between them
    t = K.reference(cs["ties"])
    assert any(np.unique(t.scores[0, l]).size < 36 for l in range(2))                        # tied scores
    s = K.reference(cs["monotone"])
    assert s.full_iters.tolist() == [[3, 1]] and s.events[0] == 4 and s.events[2] > 0 and s.events[1] == 0
    b = K.reference(cs["scaled"])
    assert (b.full_iters[:, 1] == 2).all() and b.events[1] == 3 * 2 + 2 and b.events[3] == cs["scaled"].B * 6 and (b.coef == 0).all()
    assert all(K.reference(c).events.sum() == 0 for n, c in cs.items() if n not in ("monotone", "scaled"))


def _planted(mmm, E, time, event):
    z, _, _ = mmm.classify.standardise(E)
    fold = mmm.cox.make_folds(event, None, K.PLANTED_F, K.PLANTED_R, K.PLANTED_SEED)
    return K.cox(z, time, event, None, fold, K.PLANTED_F, K.PLANTED_PENALTIES, 30, 1e-8, K.PLANTED_B, 0, K.PLANTED_SEED)


def test_a_planted_effect_is_found_and_a_null_outcome_left_alone(mmm, oracle):
    """A condition on the inputs, which tests/test_cox_gpu.py relies on: D = 96, P = 6 uniform features, hazard exp(2.5 * feature 2),
    exponential censoring (mean 0.5), times rounded to 0.01, B = 199, R = 2, F = 4, seed 1 (of the data, the folds and the permutations
    alike).  The restatement alone gives, at seed 1: 59 events, 47 distinct times, a cross-validated C of 0.651 .. 0.654 over the penalties,
    p_best = 0.005, at most 5 Newton iterations and no status other than 0; the null outcome (the same outcome rows in a shuffled order)
    has p >= 0.775 at every penalty.  Seeds 2 and 3 meet p_best <= 0.01 as well (p_best = 0.005 at C = 0.74 and 0.68); seed 1 is used."""
    E, time, event = K.planted()
    r = _planted(mmm, E, time, event)
    best = int(np.flatnonzero(r.s_obs == r.s_obs.max())[-1])
    p_best = (1.0 + r.gemax[best]) / (1.0 + K.PLANTED_B)
    print("planted: %d events, %d distinct times, C %s, p_best %.4f, iterations at most %d, events %s" % (
        event.sum(), np.unique(time).size, (r.s_obs / (2.0 * K.PLANTED_R * r.n_pairs[0])).round(4).tolist(), p_best, r.full_iters[:, 0].max(), r.events.tolist()))
    assert p_best <= 0.01 and r.events.sum() == 0 and r.full_iters[:, 0].max() <= 12 and np.unique(time).size < 96
    order = np.random.default_rng(K.PLANTED_SEED).permutation(96)
    null = _planted(mmm, E, time[order], event[order])
    p = (1.0 + null.ge) / (1.0 + K.PLANTED_B)
    nb = int(np.flatnonzero(null.s_obs == null.s_obs.max())[-1])
    print("null: p %s, p_best %.4f" % (p.tolist(), (1.0 + null.gemax[nb]) / (1.0 + K.PLANTED_B)))
    assert (p >= 0.05).all() and null.events.sum() == 0


def test_every_refusal_of_the_python_layer(mmm):
    """each is raised before a device is asked for: this test runs without one"""
    rng = np.random.default_rng(9)
    E = rng.random((30, 3))
    time = np.arange(1.0, 31.0)
    event = np.arange(30) % 3 == 0
    ok = dict(folds=3, repeats=1, permutations=5)
    nan = lambda v: np.where(np.arange(30) == 3, np.nan, np.asarray(v, float))
    bad = [
        (dict(E=E[:1], time=time[:1], event=event[:1]), "samples"), (dict(E=rng.random((30, 65))), "features"),
        (dict(E=np.where(np.arange(90).reshape(30, 3) == 4, np.nan, E)), "not finite"), (dict(E=E[0]), "[D, P]"),
        (dict(time=time[:29]), "time has shape"), (dict(event=event[:29]), "event has shape"), (dict(time=nan(time)), "time holds a missing"),
        (dict(event=nan(event)), "event holds a missing"), (dict(event=np.array([None] + [1, 0] * 14 + [1], dtype=object)), "event holds a missing"),
        (dict(strata=nan(np.ones(30))), "strata holds a missing"), (dict(strata=np.zeros(29)), "strata has shape"),
        (dict(time=-time), "negative"), (dict(time=np.where(np.arange(30) == 5, np.inf, time)), "not finite"), (dict(time=["a"] * 30), "time is not numeric"),
        (dict(event=np.arange(30) % 3), "event must hold"),
        (dict(penalties=()), "penalties"), (dict(penalties=(1.0, 0.0)), "penalties"), (dict(penalties=(1.0, np.inf)), "penalties"),
        (dict(penalties=np.arange(1, 34)), "penalties"), (dict(penalties=("a",)), "penalties"), (dict(folds=1), "folds"), (dict(folds=2.5), "folds"),
        (dict(folds=11), "number of events (10)"), (dict(repeats=0), "repeats"), (dict(repeats=65), "repeats"), (dict(permutations=0), "permutations"),
        (dict(permutations=1.5), "permutations"), (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(maxiter=0), "maxiter"), (dict(tol=-1.0), "tol"),
        (dict(tol=np.nan), "tol"), (dict(modalities=[0]), "modalities"),
        (dict(time=np.minimum(time, 28.0), event=np.arange(30) >= 27), "no comparable pair"),      # three events, tied at the latest time
        (dict(event=np.zeros(30)), "number of events (0)"),
        (dict(strata=np.arange(30) // 3), "holds no event"),            # the event, then two censored samples, in every stratum: fold 2 holds every event
    ]
    for kw, word in bad:
        args = dict(ok, E=E, time=time, event=event)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            mmm.cox_exposures(**args)
        assert word in str(e.value), (kw, str(e.value))
