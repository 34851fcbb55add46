"""mmm_cox_exposures on the device against its numpy restatement (tests/cox_ref.py): every output bit for bit over the case table (the scores
are sums in a written order, everything after them is an integer); the invariances the definition promises (waves, a second run, slices,
additivity, identity outputs independent of the permutations); B = 0; NULL outputs; every error with the outputs untouched; the Python layer
against its composition by hand; the planted effect."""
import ctypes

import numpy as np
import pytest

import cox_ref as K

pytestmark = pytest.mark.gpu

IDENTITY = ("scores", "u2_obs", "s_obs", "n_pairs", "coef", "full_iters")
COUNTS = ("ge", "gemax")
ALL = IDENTITY + COUNTS + ("maxstat", "events")
CASES = {c.name: c for c in K.cases()}


def _run(mmm, c, b0=None, B=None, waves=0, seed=None, stream=0, **kw):
    return mmm.cox._raw(mmm.default_context(), c.x, c.time, c.event, c.strata, c.fold, c.F, c.lambdas, c.maxiter, c.tol, c.B if B is None else B,
                        c.b0 if b0 is None else b0, c.seed if seed is None else seed, stream, waves, **kw)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _same(a, b, what=""):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert _bits(a[k], b[k]), (what, k)


def _equals_reference(got, ref, what=""):
    assert sorted(got) == sorted(ALL), what
    for k in got:
        want = getattr(ref, k)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (what, k, got[k].dtype, want.dtype, got[k].shape, want.shape)
        assert _bits(got[k], want), (what, k, np.argwhere(got[k] != want)[:10].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_equal_the_restatement(mmm, name):
    c = CASES[name]
    _equals_reference(_run(mmm, c), K.reference(c), name)


@pytest.mark.parametrize("name", ["D4", "D5", "D17", "D65", "D257", "P33", "P64", "tied_times", "one_event_stratum", "sizes", "ties", "scaled", "rows_lds", "rows_mem",
                                  "zbar_lds", "zbar_mem", "both_mem"])
def test_every_geometry_and_a_second_run_give_equal_bits(mmm, name):
    c = CASES[name]
    base = _run(mmm, c)
    _same(base, _run(mmm, c), "second run")
    for waves in (1, 2, 4, 8, 16):
        _same(base, _run(mmm, c, waves=waves), "waves %d" % waves)


def test_a_call_is_a_slice_and_counts_add(mmm):
    for name in ("D65", "monotone"):                                     # the second has permutation events to add
        c = CASES[name]
        whole, head, tail = _run(mmm, c, b0=0, B=9), _run(mmm, c, b0=0, B=4), _run(mmm, c, b0=4, B=5)
        assert _bits(np.ascontiguousarray(whole["maxstat"][:4]), head["maxstat"]) and _bits(np.ascontiguousarray(whole["maxstat"][4:]), tail["maxstat"])
        for k in COUNTS:
            assert _bits(whole[k], head[k] + tail[k]), k
        assert _bits(whole["events"][2:], head["events"][2:] + tail["events"][2:]) and _bits(whole["events"][:2], head["events"][:2])
        for k in IDENTITY:
            assert _bits(whole[k], head[k]) and _bits(whole[k], tail[k]), k
    assert CASES["monotone"].B and _run(mmm, CASES["monotone"])["events"][2] > 0
    # more replicates than blocks in flight, up to the last global index
    many = CASES["many"]
    top = 2 ** 31 - 1 - many.B
    high = _run(mmm, many, b0=top)
    _same(high, _run(mmm, many, b0=top, waves=1), "1100 replicates")
    part = K.reference(many, b0=2 ** 31 - 1 - 4, B=4)
    assert _bits(np.ascontiguousarray(high["maxstat"][-4:]), part.maxstat)
    rest, last = _run(mmm, many, b0=top, B=many.B - 4), _run(mmm, many, b0=2 ** 31 - 1 - 4, B=4)
    for k in COUNTS:
        assert _bits(last[k], getattr(part, k)) and _bits(high[k], rest[k] + last[k]), k


def test_identity_outputs_do_not_depend_on_the_permutations(mmm):
    c = CASES["ties"]
    base = _run(mmm, c)
    for kw in (dict(seed=99), dict(B=3), dict(b0=1000), dict(B=0), dict(stream=5)):
        got = _run(mmm, c, **kw)
        for k in IDENTITY:
            assert _bits(got[k], base[k]), (kw, k)
        assert _bits(got["events"][:2], base["events"][:2]), kw
    assert not _bits(_run(mmm, c, seed=99)["maxstat"], base["maxstat"]) and not _bits(_run(mmm, c, stream=5)["maxstat"], base["maxstat"])


def test_no_permutations(mmm):
    c = CASES["D17"]
    ref = K.reference(c)
    got = _run(mmm, c, B=0)
    for k in IDENTITY:
        assert _bits(got[k], getattr(ref, k)), k
    assert got["maxstat"].shape == (0,) and all((got[k] == 0).all() for k in COUNTS) and _bits(got["events"], K.reference(c, B=0).events)


def test_null_outputs_are_accepted(mmm):
    c = CASES["D65"]
    full = _run(mmm, c)
    for outs in ((), ("scores",), ("u2_obs",), ("coef",), ("full_iters",), ("maxstat",)):
        got = _run(mmm, c, outputs=outs)
        assert sorted(got) == sorted({"s_obs", "n_pairs", "ge", "gemax", "events"} | set(outs))
        for k in got:
            assert _bits(got[k], full[k]), (outs, k)


def test_every_error(mmm):
    c = CASES["D65"]
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, vp, vp, vp, vp, ci, ci, vp, ci, vp, ci, ctypes.c_double, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, *([vp] * 10))(
        ("mmm_cox_exposures", L))
    keep = []
    everything = set(ALL)

    def call(h=True, x=c.x, time=c.time, event=c.event, fold=c.fold, lambdas=c.lambdas, D=None, P=None, R=None, F=c.F, nl=None, strata=None, maxiter=30, tol=1e-8, B=2,
             b0=0, waves=0, null=()):
        x = np.ascontiguousarray(x, dtype=np.float64)
        time = np.ascontiguousarray(time, dtype=np.float64)
        event = np.ascontiguousarray(event, dtype=np.uint8)
        fold = np.ascontiguousarray(fold, dtype=np.uint8)
        lam = np.ascontiguousarray(lambdas, dtype=np.float64)
        D = x.shape[0] if D is None else D
        P = x.shape[1] if P is None else P
        R = fold.shape[0] if R is None else R
        nl = lam.size if nl is None else nl
        st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32)
        D1, P1, R1, L1 = max(D, 1), max(P, 1), max(R, 1), max(nl, 1)
        u32, f7 = np.uint32, lambda n, dt=np.float64: np.full(n, 7, dtype=dt)
        out = dict(scores=f7((R1, L1, D1)), u2_obs=f7((R1, L1), np.int64), s_obs=f7(L1, np.int64), n_pairs=f7(1, np.int64), coef=f7((L1, P1)),
                   full_iters=f7((L1, 2), np.int32), ge=f7(L1, u32), gemax=f7(L1, u32), maxstat=f7(max(B, 1), np.int64), events=f7(4, u32))
        arrs = dict(x=x, time=time, event=event, fold=fold, lambdas=lam)
        keep.append((arrs, out, st))
        p = {k: (None if k in null else v.ctypes.data) for k, v in list(arrs.items()) + list(out.items())}
        rc = plain(ctx.h if h else None, D, P, p["x"], p["time"], p["event"], None if st is None else st.ctypes.data, R, F, p["fold"], nl, p["lambdas"], maxiter, tol, B,
                   b0, 5, 0, waves, p["scores"], p["u2_obs"], p["s_obs"], p["n_pairs"], p["coef"], p["full_iters"], p["ge"], p["gemax"], p["maxstat"], p["events"])
        untouched = {k for k, v in out.items() if (v == 7).all()}
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    rc, _, untouched = call()
    assert rc == 0 and not untouched
    rc, _, untouched = call(B=0)                                         # the identity outputs are written, the counts are not
    assert rc == 0 and untouched == {"ge", "gemax", "maxstat"}
    rc, _, untouched = call(B=0, null=("scores", "u2_obs", "coef", "full_iters", "ge", "gemax", "maxstat"))
    assert rc == 0 and untouched == everything - {"s_obs", "n_pairs", "events"}
    no_event = np.where(c.event == 1, 0, c.fold[0])[None, :]             # every event in fold 0: its training set has none
    late = np.where(c.event == 1, c.time.max() + 1.0, c.time)            # every event after everything else, all tied: no comparable pair
    arg = [dict(h=False), dict(D=1), dict(D=0), dict(D=-1), dict(P=0), dict(R=0), dict(F=1), dict(F=0), dict(nl=0), dict(B=-1), dict(b0=-1), dict(b0=2 ** 31 - 2, B=2),
           dict(waves=3), dict(waves=32), dict(waves=-1), dict(maxiter=0), dict(tol=-1.0), dict(tol=np.nan), dict(null=("x",)), dict(null=("time",)), dict(null=("event",)),
           dict(null=("fold",)), dict(null=("lambdas",)), dict(null=("s_obs",)), dict(null=("n_pairs",)), dict(null=("events",)), dict(null=("ge",)), dict(null=("gemax",)),
           dict(strata=[0] * 64 + [65]), dict(strata=[-1] + [0] * 64), dict(event=np.zeros(65)), dict(fold=no_event), dict(time=late), dict(F=4)]      # F = 4: the folds hold a 4
    for kw in arg:
        rc, msg, untouched = call(**kw)
        assert rc == -1 and untouched == everything, (kw, rc, msg)
    assert call(strata=[64] + [0] * 64)[0] == 0 and call(tol=0.0, maxiter=1)[0] == 0        # the bounds themselves are accepted
    for bad in (np.nan, np.inf, -np.inf):
        x = c.x.copy(); x[7, 2] = bad
        rc, msg, untouched = call(x=x)
        assert rc == -1 and untouched == everything and "x entry (7, 2)" in msg, (bad, msg)
    for bad in (0.0, -1.0, np.nan, np.inf):
        lam = c.lambdas.copy(); lam[3] = bad
        rc, msg, untouched = call(lambdas=lam)
        assert rc == -1 and untouched == everything and "lambda[3]" in msg, (bad, msg)
    for bad in (np.nan, np.inf, -1.0):
        t = c.time.copy(); t[13] = bad
        rc, msg, untouched = call(time=t)
        assert rc == -1 and untouched == everything and "time[13]" in msg, (bad, msg)
    e = c.event.copy(); e[11] = 2
    rc, msg, untouched = call(event=e)
    assert rc == -1 and untouched == everything and "event[11]" in msg, msg
    f = c.fold.copy(); f[0, 9] = 5
    rc, msg, untouched = call(fold=f)
    assert rc == -1 and untouched == everything and "fold entry (0, 9)" in msg, msg
    # limits, each with its figure in the message
    small = lambda n: dict(time=np.arange(1.0, n + 1), event=np.arange(n) % 2, fold=(np.arange(n) // 2 % 2)[None, :])
    rc, msg, untouched = call(x=np.zeros((4097, 1)), F=2, **small(4097))
    assert rc == -4 and untouched == everything and "4097" in msg and "4096" in msg, msg
    rc, msg, untouched = call(x=np.zeros((8, 65)), F=2, **small(8))
    assert rc == -4 and untouched == everything and "65" in msg and "64" in msg, msg
    s8 = small(8)
    rc, msg, untouched = call(x=np.zeros((8, 2)), F=2, time=s8["time"], event=s8["event"], fold=np.repeat(s8["fold"], 65, axis=0))
    assert rc == -4 and untouched == everything and "65" in msg and "64" in msg, msg
    rc, msg, untouched = call(x=np.zeros((8, 2)), F=256, **s8)
    assert rc == -4 and untouched == everything and "256" in msg and "255" in msg, msg
    rc, msg, untouched = call(x=np.zeros((8, 2)), F=2, lambdas=np.ones(33), **s8)
    assert rc == -4 and untouched == everything and "33" in msg and "32" in msg, msg
    assert call(x=np.zeros((8, 2)), F=2, lambdas=np.ones(2), **s8)[0] == 0                  # the same small inputs inside the limits


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_python_is_its_composition_done_by_hand(mmm):
    rng = np.random.default_rng(8)
    D, P, B, R, F = 50, 4, 40, 2, 3
    E = rng.random((D, P))
    E[:, 3] = 0.25                                                       # a constant column becomes 0
    time = np.round(rng.exponential(size=D) / np.exp(1.5 * E[:, 0]), 1)
    event = rng.random(D) < 0.6
    site = np.array(["x", "y"])[rng.integers(0, 2, size=D)]
    pens = (0.5, 5.0, 50.0)
    r = mmm.cox_exposures(E, time, event, strata=site, penalties=pens, folds=F, repeats=R, permutations=B, seed=13, maxiter=25, tol=1e-9)
    ev = event.astype(np.uint8)
    s = (site == "y").astype(np.int32)
    mean, sd = E.mean(axis=0), E.std(axis=0)
    z = np.zeros_like(E)
    z[:, :3] = (E[:, :3] - mean[:3]) / sd[:3]
    fold = mmm.cox.make_folds(ev, s, F, R, 13)
    ref = K.cox(z, time, ev, s, fold, F, pens, 25, 1e-9, B, 0, 13)
    _equals_reference(mmm.cox._raw(mmm.default_context(), z, time, ev, s, fold, F, pens, 25, 1e-9, B, 0, 13), ref)
    n_pairs = int(ref.n_pairs[0])
    best = max(range(3), key=lambda l: (ref.s_obs[l], l))
    assert r.n_pairs == n_pairs and r.permutations == B and r.best == best and r.penalty == pens[best] and r.penalties.tolist() == list(pens)
    assert _bits(r.c_index, ref.s_obs / (R * 2.0 * n_pairs)) and _bits(r.c_index_repeats, ref.u2_obs / (2.0 * n_pairs)) and _bits(r.p, (1.0 + ref.ge) / (1.0 + B))
    assert r.p_best == (1.0 + ref.gemax[best]) / (1.0 + B) and _bits(r.coef, np.ascontiguousarray(ref.coef[best])) and _bits(r.hazard_ratio, np.exp(ref.coef[best]))
    assert _bits(r.oof_risk, ref.scores[:, best, :].mean(axis=0)) and r.coef[3] == 0.0 and r.scale[3] == 1.0 and _bits(r.mean, mean) and _bits(r.scale[:3], sd[:3])
    assert r.events == dict(identity_maxiter=int(ref.events[0]), identity_pivot=int(ref.events[1]), permutations_maxiter=int(ref.events[2]), permutations_pivot=int(ref.events[3]))
    new = rng.random((7, P))
    assert np.allclose(r.predict_risk(new), ((new - mean) / r.scale) @ ref.coef[best], rtol=1e-13, atol=1e-13)
    groups = r.risk_groups(3)
    assert sorted(np.bincount(groups).tolist()) == [16, 17, 17] and r.oof_risk[groups == 0].max() <= r.oof_risk[groups == 1].min() <= r.oof_risk[groups == 2].min()
    assert set(mmm.kaplan_meier(time, event, groups=r.risk_groups())) == {0, 1}
    rows = r.table()
    assert len(rows) == 3 + P and rows[1] == dict(penalty=5.0, c_index=r.c_index[1], p=r.p[1], best=best == 1) and rows[3]["feature"] == r.names[0]
    assert rows[3]["hazard_ratio"] == float(np.exp(ref.coef[best, 0]))


def test_planted_effect_comes_back_on_the_device(mmm):
    """follows from the bitwise equality with the restatement (whose behaviour on these inputs tests/test_cox_cpu.py asserts); asserted anyway"""
    E, time, event = K.planted()
    kw = dict(penalties=K.PLANTED_PENALTIES, folds=K.PLANTED_F, repeats=K.PLANTED_R, permutations=K.PLANTED_B, seed=K.PLANTED_SEED)
    r = mmm.cox_exposures(E, time, event, **kw)
    assert r.p_best <= 0.01 and r.c_index[r.best] > 0.6 and int(np.argmax(np.abs(r.coef))) == 2 and r.coef[2] > 0 and not any(r.events.values())
    order = np.random.default_rng(K.PLANTED_SEED).permutation(96)
    null = mmm.cox_exposures(E, time[order], event[order], **kw)
    assert (null.p >= 0.05).all()
