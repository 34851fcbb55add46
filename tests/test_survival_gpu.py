"""mmm_survival_association on the device against its numpy restatement (tests/survival_ref.py): every output bit for bit (the sums are
integers, a statistic is -, x, / in a written order); the invariances the definition promises (waves, a second run, slices, additivity,
identity outputs independent of the permutations); B = 0; NULL outputs; every error with the outputs untouched; the Python layer against its
composition by hand; the planted effects; and mmm_associate_exposures, whose sort the new kernel shares, still equal to its own reference."""
import ctypes

import numpy as np
import pytest

import associate_ref as A
import survival_ref as S

pytestmark = pytest.mark.gpu

IDENTITY = ("obs_trend", "z_trend", "obs_group", "u_group")
COUNTS = ("ge_trend", "gemax_trend", "ge_group")
CUT_IDENTITY = ("obs_cut", "cut_at")
CUT_COUNTS = ("ge_cut", "gemax_cut")
CASES = {c.name: c for c in S.cases()}


def _keys(m_lo):
    return IDENTITY + COUNTS + ("maxstat",) + ((CUT_IDENTITY + CUT_COUNTS) if m_lo >= 1 else ())


def _run(mmm, c, b0=None, B=None, waves=0, seed=None, stream=0, **kw):
    return mmm.survival._raw(mmm.default_context(), c.x, c.levels, c.groups, c.time, c.event, c.strata, c.m_lo, c.B if B is None else B,
                             c.b0 if b0 is None else b0, c.seed if seed is None else seed, stream, waves, **kw)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _same(a, b, what=""):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert _bits(a[k], b[k]), (what, k)


def _equals_reference(got, ref, m_lo, what=""):
    assert sorted(got) == sorted(_keys(m_lo)), what
    for k in got:
        want = getattr(ref, k)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (what, k, got[k].dtype, want.dtype, got[k].shape, want.shape)
        assert _bits(got[k], want), (what, k, np.argwhere(got[k] != want)[:10].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_equal_the_restatement(mmm, name):
    c = CASES[name]
    _equals_reference(_run(mmm, c), S.reference(c), c.m_lo, name)


@pytest.mark.parametrize("name", ["D1", "D5", "D65", "D257", "D300", "P33", "P256", "C0", "Q256", "contents", "sizes", "unordered", "strata64"])
def test_every_geometry_and_a_second_run_give_equal_bits(mmm, name):
    c = CASES[name]
    base = _run(mmm, c)
    _same(base, _run(mmm, c), "second run")
    for waves in (1, 2, 4, 8, 16):
        _same(base, _run(mmm, c, waves=waves), "waves %d" % waves)


def test_a_call_is_a_slice_and_counts_add(mmm):
    c = CASES["D65"]
    whole, head, tail = _run(mmm, c, b0=0, B=9), _run(mmm, c, b0=0, B=4), _run(mmm, c, b0=4, B=5)
    assert _bits(np.ascontiguousarray(whole["maxstat"][:4]), head["maxstat"]) and _bits(np.ascontiguousarray(whole["maxstat"][4:]), tail["maxstat"])
    for k in COUNTS + CUT_COUNTS:
        assert _bits(whole[k], head[k] + tail[k]), k
    for k in IDENTITY + CUT_IDENTITY:
        assert _bits(whole[k], head[k]) and _bits(whole[k], tail[k]), k
    # more replicates than blocks in flight, up to the last global index
    many = CASES["many"]
    top = 2 ** 31 - 1 - many.B
    high = _run(mmm, many, b0=top)
    _same(high, _run(mmm, many, b0=top, waves=1), "3000 replicates")
    part = S.reference(many, b0=2 ** 31 - 1 - 4, B=4)
    assert _bits(np.ascontiguousarray(high["maxstat"][-4:]), part.maxstat)
    rest, last = _run(mmm, many, b0=top, B=many.B - 4), _run(mmm, many, b0=2 ** 31 - 1 - 4, B=4)
    for k in COUNTS + CUT_COUNTS:
        assert _bits(last[k], getattr(part, k)) and _bits(high[k], rest[k] + last[k]), k


def test_identity_outputs_do_not_depend_on_the_permutations(mmm):
    c = CASES["contents"]
    base = _run(mmm, c)
    for kw in (dict(seed=99), dict(B=3), dict(b0=1000), dict(B=0), dict(stream=5)):
        got = _run(mmm, c, **kw)
        for k in IDENTITY + CUT_IDENTITY:
            assert _bits(got[k], base[k]), (kw, k)
    assert not _bits(_run(mmm, c, seed=99)["maxstat"], base["maxstat"]) and not _bits(_run(mmm, c, stream=5)["maxstat"], base["maxstat"])


def test_no_permutations_no_variance_no_events(mmm):
    c = CASES["D63"]
    ref = S.reference(c)
    got = _run(mmm, c, B=0)
    for k in IDENTITY + CUT_IDENTITY:
        assert _bits(got[k], getattr(ref, k)), k
    assert got["maxstat"].shape == (0, 2) and all((got[k] == 0).all() for k in COUNTS + CUT_COUNTS)
    for name in ("allalone", "censored"):
        c = CASES[name]
        r = _run(mmm, c)
        assert all((r[k] == c.B).all() for k in COUNTS + CUT_COUNTS) and all((r[k] == 0).all() for k in ("obs_trend", "obs_group", "obs_cut", "cut_at", "maxstat")), name


def test_null_outputs_are_accepted(mmm):
    c = CASES["D65"]
    full = _run(mmm, c)
    for outs in ((), ("z_trend",), ("u_group",), ("maxstat",)):
        got = _run(mmm, c, outputs=outs)
        assert sorted(got) == sorted(set(_keys(1)) - {"z_trend", "u_group", "maxstat"} | set(outs))
        for k in got:
            assert _bits(got[k], full[k]), (outs, k)


def test_every_error(mmm):
    c = CASES["D65"]
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, *([vp] * 12))(("mmm_survival_association", L))
    keep = []
    cut_outs = {"obs_cut", "cut_at", "ge_cut", "gemax_cut"}
    everything = {"obs_trend", "z_trend", "obs_group", "u_group", "ge_trend", "gemax_trend", "ge_group", "maxstat"} | cut_outs

    def call(h=True, x=c.x, levels=c.levels, groups=c.groups, time=c.time, event=c.event, D=None, P=None, C=None, strata=None, m_lo=1, B=2, b0=0, waves=0, null=()):
        x = np.ascontiguousarray(x, dtype=np.float64)
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        g = np.ascontiguousarray(groups, dtype=np.int32)
        time = np.ascontiguousarray(time, dtype=np.float64)
        event = np.ascontiguousarray(event, dtype=np.uint8)
        D = x.shape[0] if D is None else D
        P = x.shape[1] if P is None else P
        C = lv.size if C is None else C
        st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32)
        P1, C1, Q1 = max(P, 1), max(C, 1), max(int(np.abs(lv).sum()), 1)
        u32, f7 = np.uint32, lambda n, dt=np.float64: np.full(n, 7, dtype=dt)
        out = dict(obs_trend=f7(P1), z_trend=f7(P1, np.int64), obs_group=f7(C1), u_group=f7(Q1, np.int64), obs_cut=f7(P1), cut_at=f7(P1, np.int32), ge_trend=f7(P1, u32),
                   gemax_trend=f7(P1, u32), ge_cut=f7(P1, u32), gemax_cut=f7(P1, u32), ge_group=f7(C1, u32), maxstat=f7((max(B, 1), 2)))
        arrs = dict(x=x, levels=lv, groups=g, time=time, event=event)
        keep.append((arrs, out, st))
        p = {k: (None if k in null else v.ctypes.data) for k, v in list(arrs.items()) + list(out.items())}
        rc = plain(ctx.h if h else None, D, P, p["x"], C, p["levels"], p["groups"], p["time"], p["event"], None if st is None else st.ctypes.data, m_lo, B, b0, 5, 0, waves,
                   p["obs_trend"], p["z_trend"], p["obs_group"], p["u_group"], p["obs_cut"], p["cut_at"], p["ge_trend"], p["gemax_trend"], p["ge_cut"], p["gemax_cut"],
                   p["ge_group"], p["maxstat"])
        untouched = {k for k, v in out.items() if (v == 7).all()}
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    rc, _, untouched = call()
    assert rc == 0 and not untouched
    rc, _, untouched = call(B=0)                                         # the identity outputs are written, the counts are not
    assert rc == 0 and untouched == {"ge_trend", "gemax_trend", "ge_cut", "gemax_cut", "ge_group", "maxstat"}
    rc, _, untouched = call(B=0, null=("z_trend", "u_group", "ge_trend", "gemax_trend", "ge_cut", "gemax_cut", "ge_group", "maxstat"))
    assert rc == 0 and untouched == everything - {"obs_trend", "obs_group", "obs_cut", "cut_at"}
    rc, _, untouched = call(m_lo=0, null=tuple(cut_outs))                # the cuts off: their four pointers may be NULL
    assert rc == 0 and not untouched - cut_outs
    rc, _, untouched = call(m_lo=0)                                      # .. and are not written where given
    assert rc == 0 and untouched == cut_outs
    rc, _, untouched = call(C=0, null=("levels", "groups", "obs_group", "ge_group"))
    assert rc == 0 and untouched == {"obs_group", "u_group", "ge_group"}
    arg = [dict(h=False), dict(D=0), dict(D=-1), dict(P=0), dict(C=-1), dict(levels=(2, 0)), dict(levels=(2, -3)), dict(B=-1), dict(b0=-1), dict(b0=2 ** 31 - 2, B=2),
           dict(waves=3), dict(waves=32), dict(waves=-1), dict(m_lo=-1), dict(m_lo=33), dict(null=("x",)), dict(null=("levels",)), dict(null=("groups",)),
           dict(null=("time",)), dict(null=("event",)), dict(null=("obs_trend",)), dict(null=("obs_group",)), dict(null=("obs_cut",)), dict(null=("cut_at",)),
           dict(null=("ge_trend",)), dict(null=("gemax_trend",)), dict(null=("ge_cut",)), dict(null=("gemax_cut",)), dict(null=("ge_group",)),
           dict(strata=[0] * 64 + [65]), dict(strata=[-1] + [0] * 64)]
    for kw in arg:
        rc, msg, untouched = call(**kw)
        assert rc == -1 and untouched == everything, (kw, rc, msg)
    assert call(m_lo=32)[0] == 0 and call(strata=[64] + [0] * 64)[0] == 0                    # the bounds themselves are accepted
    for bad in (np.nan, np.inf, -np.inf):
        x = c.x.copy(); x[7, 2] = bad
        rc, msg, untouched = call(x=x)
        assert rc == -1 and untouched == everything and "x entry (7, 2)" in msg, (bad, msg)
    for bad in (np.nan, np.inf, -1.0):
        t = c.time.copy(); t[9] = bad
        rc, msg, untouched = call(time=t)
        assert rc == -1 and untouched == everything and "time[9]" in msg, (bad, msg)
    e = c.event.copy(); e[11] = 2
    rc, msg, untouched = call(event=e)
    assert rc == -1 and untouched == everything and "event[11]" in msg, msg
    for bad in (3, -1):                                                  # covariate 1 has the codes 0 .. 2
        g = c.groups.copy(); g[9, 1] = bad
        rc, msg, untouched = call(groups=g)
        assert rc == -1 and untouched == everything and "groups entry (9, 1)" in msg, (bad, msg)
    # limits, each with its figure in the message
    big = dict(levels=(1,), m_lo=0)
    rc, msg, untouched = call(x=np.zeros((4097, 1)), groups=np.zeros((4097, 1)), time=np.ones(4097), event=np.ones(4097), **big)
    assert rc == -4 and untouched == everything and "4097" in msg and "4096" in msg, msg
    rc, msg, untouched = call(x=np.zeros((2, 257)), groups=np.zeros((2, 1)), time=np.ones(2), event=np.ones(2), **big)
    assert rc == -4 and untouched == everything and "257" in msg and "256" in msg, msg
    rc, msg, untouched = call(x=np.zeros((3, 1)), levels=(255, 2), groups=np.zeros((3, 2)), time=np.ones(3), event=np.ones(3), m_lo=0)
    assert rc == -4 and untouched == everything and "257" in msg and "256" in msg, msg
    rc, msg, untouched = call(strata=np.arange(65))
    assert rc == -4 and untouched == everything and "65" in msg and "64" in msg, msg


def test_associate_exposures_still_equals_its_reference(mmm):
    """k_assoc now takes its sort from the header it shares with k_survival"""
    for name in ("D65", "sizes", "unordered"):
        c = next(v for v in A.cases() if v.name == name)
        got, ref = mmm.associate._raw(mmm.default_context(), c.x, c.levels, c.y, c.strata, c.B, c.b0, c.seed, 0, 0), A.reference(c)
        for k in ("obs", "zc_obs", "ge", "ge_max", "maxstat"):
            assert _bits(got[k], getattr(ref, k)), (name, k)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_python_is_its_composition_done_by_hand(mmm):
    rng = np.random.default_rng(8)
    D, P, B = 50, 4, 60
    E = rng.random((D, P))
    E[rng.permutation(D)[:30], 1] = 0.0
    grp = np.array(["lum", "basal", "her2"])[rng.integers(0, 3, size=D)]
    flag = rng.integers(0, 2, size=D).astype(bool)
    site = np.array(["x", "y"])[rng.integers(0, 2, size=D)]
    time = np.round(rng.exponential(1.0, size=D), 1)
    event = rng.random(D) < 0.7
    r = mmm.survival_association(E, time, event, groups={"subtype": grp, "flag": flag}, strata=site, min_fraction=0.2, permutations=B, seed=13)
    lv, codes = np.unique(grp, return_inverse=True)
    g = np.stack([codes, flag.astype(int)], axis=1)
    s = (site == "y").astype(np.int32)
    ref = S.survival(E, (3, 2), g, time, event, s, 10, B, 0, 13)
    _equals_reference(mmm.survival._raw(mmm.default_context(), E, (3, 2), g, time, event.astype(np.uint8), s, 10, B, 0, 13), ref, 10)
    pl = S.Plan(E, (3, 2), g, time, event, s, 10)
    assert r.permutations == B and [t.name for t in r.groups] == ["subtype", "flag"] and r.groups[0].levels.tolist() == lv.tolist()
    assert _bits(r.p, (1.0 + ref.ge_trend) / (1.0 + B)) and _bits(r.p_adj, (1.0 + ref.gemax_trend) / (1.0 + B))
    assert _bits(r.p_cut, (1.0 + ref.ge_cut) / (1.0 + B)) and _bits(r.p_cut_adj, (1.0 + ref.gemax_cut) / (1.0 + B))
    assert np.allclose(r.q, S.bh(r.p), rtol=1e-14, atol=0)
    assert _bits(r.z, np.sign(ref.z_trend - pl.Et) * np.sqrt(ref.obs_trend))
    for p in range(P):
        at = int(ref.cut_at[p])
        assert at > 0 and r.cut_value[p] == E[pl.order[p][at - 1], p] and r.n_high[p] == D - at == int((E[:, p] > r.cut_value[p]).sum())
        low = np.cumsum(pl.A[pl.order[p]])[at - 1]
        assert r.z_cut[p] == -np.sign(low - pl.Ec[p][at - 1]) * np.sqrt(ref.obs_cut[p])
    for c, (t, G, q0) in enumerate(zip(r.groups, (3, 2), (0, 3))):
        assert t.chi2 == ref.obs_group[c] / (2.0 if G == 2 else 1.0) and t.p == (1.0 + ref.ge_group[c]) / (1.0 + B)
        assert t.n.tolist() == np.bincount(g[:, c], minlength=G).tolist() and t.observed.tolist() == [int(event[g[:, c] == k].sum()) for k in range(G)]
        assert np.allclose(t.observed - t.expected, [pl.a[g[:, c] == k].sum() for k in range(G)], rtol=0, atol=D * 2.0 ** -24)
    assert r.significant(0.5) == np.flatnonzero(r.p_adj <= 0.5).tolist() and r.significant(0.5, adjusted=False) == np.flatnonzero(r.q <= 0.5).tolist()
    rows = r.table()
    assert len(rows) == P + 2 and rows[1] == dict(feature=1, z=r.z[1], p=r.p[1], p_adj=r.p_adj[1], q=r.q[1], cut_value=r.cut_value[1], n_high=r.n_high[1], z_cut=r.z_cut[1],
                                                   p_cut=r.p_cut[1], p_cut_adj=r.p_cut_adj[1]) and rows[P] == dict(group="subtype", chi2=r.groups[0].chi2, p=r.groups[0].p)
    # an array of groups; cluster labels as they stand; the cuts off; no groups
    a = mmm.survival_association(E, time, event, groups=g, strata=s, min_fraction=0.2, permutations=B, seed=13)
    assert _bits(a.p, r.p) and _bits(a.p_cut_adj, r.p_cut_adj) and a.groups[1].p == r.groups[1].p and [t.name for t in a.groups] == ["group0", "group1"]
    b = mmm.survival_association(E, time, event, groups={"cluster": np.arange(D, dtype=np.int64) % 3}, cutpoints=False, permutations=10, seed=1)
    assert b.groups[0].levels.tolist() == [0, 1, 2] and b.p.shape == (P,) and b.p_cut is None and b.cut_value is None and len(b.table()[0]) == 5
    assert mmm.survival_association(E, time, event, permutations=10).groups == []


def test_planted_effects_come_back_on_the_device(mmm):
    """follows from the bitwise equality with the restatement (whose behaviour on these inputs tests/test_survival_cpu.py asserts); asserted anyway"""
    x, groups, levels, time, event = S.planted()
    ref = S.planted_reference()
    B = S.PLANTED_B
    _equals_reference(mmm.survival._raw(mmm.default_context(), x, levels, groups, time, event, None, S.PLANTED_MLO, B, 0, 1000 + S.PLANTED_SEED), ref, S.PLANTED_MLO)
    r = mmm.survival_association(x, time, event, groups={"group": groups[:, 0], "batch": groups[:, 1]}, permutations=B, seed=1000 + S.PLANTED_SEED)
    assert _bits(r.p, (1.0 + ref.ge_trend) / (1.0 + B)) and _bits(r.p_adj, (1.0 + ref.gemax_trend) / (1.0 + B)) and _bits(r.p_cut, (1.0 + ref.ge_cut) / (1.0 + B))
    assert _bits(r.p_cut_adj, (1.0 + ref.gemax_cut) / (1.0 + B)) and [t.p for t in r.groups] == ((1.0 + ref.ge_group) / (1.0 + B)).tolist()
    assert r.p_adj[0] <= 0.01 and r.p_cut_adj[1] <= 0.01 and r.groups[0].p <= 0.01 and (r.p_adj[2:] >= 0.05).all() and (r.p_cut_adj[2:] >= 0.05).all() and r.groups[1].p >= 0.05
    assert r.z[0] > 0 and r.z[1] > 0 and r.z_cut[1] > 0 and abs((x.shape[0] - int(r.n_high[1])) - int((x[:, 1] <= 0.5).sum())) <= x.shape[0] // 6 and r.groups[0].observed[1] > r.groups[0].expected[1]
    xc, tc, ec, s = S.confounded()
    free = mmm.survival_association(xc, tc, ec, cutpoints=False, permutations=999, seed=11)
    held = mmm.survival_association(xc, tc, ec, strata=s, cutpoints=False, permutations=999, seed=11)
    assert free.p_adj[0] <= 0.001 and held.p_adj[0] > 0.05
