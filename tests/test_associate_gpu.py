"""mmm_associate_exposures on the device against its numpy restatement (tests/associate_ref.py): every output bit for bit (the sums are
integers, t is +, x, / in a written order); the invariances the definition promises (waves, a second run, slices, additivity, obs independent
of the permutations); B = 0; NULL outputs; every error with the outputs untouched; the Python layer against its composition by hand; the
planted associations."""
import ctypes

import numpy as np
import pytest

import associate_ref as A

pytestmark = pytest.mark.gpu

KEYS = ("obs", "zc_obs", "ge", "ge_max", "maxstat")
CASES = {c.name: c for c in A.cases()}


def _run(mmm, c, b0=None, B=None, waves=0, seed=None, **kw):
    return mmm.associate._raw(mmm.default_context(), c.x, c.levels, c.y, c.strata, c.B if B is None else B, c.b0 if b0 is None else b0,
                              c.seed if seed is None else seed, 0, waves, **kw)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _same(a, b, what=""):
    for k in KEYS:
        assert _bits(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_equal_the_restatement(mmm, name):
    c = CASES[name]
    got, ref = _run(mmm, c), A.reference(c)
    for k in KEYS:
        want = getattr(ref, k)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, k)
        assert _bits(got[k], want), (name, k, np.argwhere(got[k] != want)[:10].tolist())


@pytest.mark.parametrize("name", ["D1", "D5", "D65", "D257", "P33", "P256", "PC4097", "Q256", "contents", "sizes", "unordered"])
def test_every_geometry_and_a_second_run_give_equal_bits(mmm, name):
    c = CASES[name]
    base = _run(mmm, c)
    _same(base, _run(mmm, c), "second run")
    for waves in (1, 4, 16):
        _same(base, _run(mmm, c, waves=waves), "waves %d" % waves)


def test_a_call_is_a_slice_and_counts_add(mmm):
    c = CASES["D65"]
    whole, head, tail = _run(mmm, c, b0=0, B=9), _run(mmm, c, b0=0, B=4), _run(mmm, c, b0=4, B=5)
    assert _bits(np.ascontiguousarray(whole["maxstat"][:4]), head["maxstat"]) and _bits(np.ascontiguousarray(whole["maxstat"][4:]), tail["maxstat"])
    for k in ("ge", "ge_max"):
        assert _bits(whole[k], head[k] + tail[k]), k
    for k in ("obs", "zc_obs"):
        assert _bits(whole[k], head[k]) and _bits(whole[k], tail[k]), k
    # more replicates than blocks in flight, up to the last global index
    many = CASES["many"]
    top = 2 ** 31 - 1 - many.B
    high = _run(mmm, many, b0=top)
    _same(high, _run(mmm, many, b0=top, waves=1), "3000 replicates")
    part = A.reference(many, b0=2 ** 31 - 1 - 4, B=4)
    assert _bits(np.ascontiguousarray(high["maxstat"][-4:]), part.maxstat)
    rest, last = _run(mmm, many, b0=top, B=many.B - 4), _run(mmm, many, b0=2 ** 31 - 1 - 4, B=4)
    assert _bits(last["ge"], part.ge) and _bits(last["ge_max"], part.ge_max)
    assert _bits(high["ge"], rest["ge"] + last["ge"]) and _bits(high["ge_max"], rest["ge_max"] + last["ge_max"])


def test_obs_does_not_depend_on_the_permutations(mmm):
    c = CASES["contents"]
    base = _run(mmm, c)
    for kw in (dict(seed=99), dict(B=3), dict(b0=1000), dict(B=0)):
        got = _run(mmm, c, **kw)
        assert _bits(got["obs"], base["obs"]) and _bits(got["zc_obs"], base["zc_obs"]), kw
    assert not _bits(_run(mmm, c, seed=99)["maxstat"], base["maxstat"])


def test_no_permutations_and_strata_of_one(mmm):
    c = CASES["D63"]
    ref = A.reference(c)
    got = _run(mmm, c, B=0)
    assert _bits(got["obs"], ref.obs) and _bits(got["zc_obs"], ref.zc_obs) and got["maxstat"].shape == (0, 3)
    alone = _run(mmm, CASES["allalone"])
    assert (alone["ge"] == 10).all() and (alone["ge_max"] == 10).all() and _bits(alone["maxstat"], np.tile(alone["obs"].max(axis=0), (10, 1)))


def test_null_outputs_are_accepted(mmm):
    c = CASES["D65"]
    full = _run(mmm, c)
    for outs in ((), ("zc_obs",), ("maxstat",)):
        got = _run(mmm, c, outputs=outs)
        assert sorted(got) == sorted(("obs", "ge", "ge_max") + outs)
        for k in got:
            assert _bits(got[k], full[k]), (outs, k)


def test_every_error(mmm):
    c = CASES["D65"]
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, vp, ci, vp, vp, vp, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, vp, vp, vp, vp, vp)(("mmm_associate_exposures", L))
    keep = []

    def call(h=True, x=c.x, y=c.y, levels=c.levels, D=None, P=None, C=None, strata=None, B=2, b0=0, waves=0, null=()):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        D = x.shape[0] if D is None else D
        P = x.shape[1] if P is None else P
        C = lv.size if C is None else C
        st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32)
        P1, C1, Q1 = max(P, 1), max(C, 1), max(int(np.where(lv > 0, lv, 1).sum()), 1)
        out = dict(obs=np.full((P1, C1), 7.0), zc_obs=np.full((P1, Q1), 7, dtype=np.int64), ge=np.full((P1, C1), 7, dtype=np.uint32),
                   ge_max=np.full((P1, C1), 7, dtype=np.uint32), maxstat=np.full((max(B, 1), C1), 7.0))
        arrs = dict(x=x, levels=lv, y=y)
        keep.append((arrs, out, st))
        p = {k: (None if k in null else v.ctypes.data) for k, v in list(arrs.items()) + list(out.items())}
        rc = plain(ctx.h if h else None, D, P, p["x"], C, p["levels"], p["y"], None if st is None else st.ctypes.data, B, b0, 5, 0, waves, p["obs"], p["zc_obs"],
                   p["ge"], p["ge_max"], p["maxstat"])
        untouched = {k for k, v in out.items() if (v == 7).all()}
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    everything = {"obs", "zc_obs", "ge", "ge_max", "maxstat"}
    rc, _, untouched = call()
    assert rc == 0 and not untouched
    rc, _, untouched = call(B=0)                                         # obs and zc_obs are written, the counts are not
    assert rc == 0 and untouched == {"ge", "ge_max", "maxstat"}
    rc, _, untouched = call(B=0, null=("ge", "ge_max", "maxstat", "zc_obs"))
    assert rc == 0 and untouched == everything - {"obs"}
    arg = [dict(h=False), dict(D=0), dict(D=-1), dict(P=0), dict(C=0), dict(C=-1), dict(levels=(0, -1, 2)), dict(B=-1), dict(b0=-1), dict(b0=2 ** 31 - 2, B=2),
           dict(waves=3), dict(waves=32), dict(waves=-1), dict(null=("x",)), dict(null=("levels",)), dict(null=("y",)), dict(null=("obs",)), dict(null=("ge",)),
           dict(null=("ge_max",)), dict(strata=[0] * 64 + [65]), dict(strata=[-1] + [0] * 64)]
    for kw in arg:
        rc, msg, untouched = call(**kw)
        assert rc == -1 and untouched == everything, (kw, rc, msg)
    for bad in (np.nan, np.inf, -np.inf):
        x = c.x.copy(); x[7, 2] = bad
        rc, msg, untouched = call(x=x)
        assert rc == -1 and untouched == everything and "x entry (7, 2)" in msg, (bad, msg)
        y = c.y.copy(); y[9, 0] = bad
        rc, msg, untouched = call(y=y)
        assert rc == -1 and untouched == everything and "y entry (9, 0)" in msg, (bad, msg)
    for bad in (0.5, 3.0, -1.0):                                         # covariate 1 has the codes 0 .. 2
        y = c.y.copy(); y[9, 1] = bad
        rc, msg, untouched = call(y=y)
        assert rc == -1 and untouched == everything and "y entry (9, 1)" in msg, (bad, msg)
    assert call(strata=[64] + [0] * 64)[0] == 0                          # the bound itself is accepted
    # limits, each with its figure in the message
    rc, msg, untouched = call(x=np.zeros((4097, 1)), y=np.zeros((4097, 1)), levels=(0,))
    assert rc == -4 and untouched == everything and "4097" in msg and "4096" in msg, msg
    rc, msg, untouched = call(x=np.zeros((2, 257)), y=np.zeros((2, 1)), levels=(0,))
    assert rc == -4 and untouched == everything and "257" in msg and "256" in msg, msg
    rc, msg, untouched = call(x=np.zeros((3, 1)), y=np.zeros((3, 2)), levels=(255, 2))
    assert rc == -4 and untouched == everything and "257" in msg and "256" in msg, msg


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_python_is_its_composition_done_by_hand(mmm):
    rng = np.random.default_rng(8)
    D, P, B = 50, 4, 60
    E = rng.random((D, P))
    E[rng.permutation(D)[:30], 1] = 0.0
    grp = np.array(["lum", "basal", "her2"])[rng.integers(0, 3, size=D)]
    age = np.round(rng.uniform(30, 80, size=D))
    site = rng.integers(0, 2, size=D)
    r = mmm.associate_exposures(E, {"subtype": grp, "age": age}, strata=site, permutations=B, seed=13)
    lv, codes = np.unique(grp, return_inverse=True)
    y = np.stack([codes.astype(np.float64), age], axis=1)
    ref = A.associate(E, (3, 0), y, site, B, 0, 13)
    raw = mmm.associate._raw(mmm.default_context(), E, (3, 0), y, site, B, 0, 13)
    for k in KEYS:
        assert _bits(raw[k], getattr(ref, k)), k
    assert r.permutations == B and r.names == ["subtype", "age"] and r.levels[0].tolist() == lv.tolist() and r.levels[1] is None
    assert _bits(r.statistic, (D - 1) * ref.obs) and _bits(r.p, (1.0 + ref.ge) / (1.0 + B)) and _bits(r.p_adj, (1.0 + ref.ge_max) / (1.0 + B))
    assert np.allclose(r.q, A.bh(r.p.ravel()).reshape(P, 2), rtol=1e-14, atol=0)
    Rx = np.stack([A.r2(E[:, p]) for p in range(P)], axis=1)
    ra = A.r2(age)
    for p in range(P):
        want = np.corrcoef(Rx[:, p], ra)[0, 1]
        assert np.isclose(r.rho[p, 1], want, rtol=1e-12, atol=1e-12) and np.isnan(r.rho[p, 0])
        assert np.isclose(r.statistic[p, 1], (D - 1) * want * want, rtol=1e-10, atol=1e-12)
        for g in range(3):
            assert np.isclose(r.mean_rank[0][p, g], Rx[codes == g, p].mean() / 2.0, rtol=1e-13, atol=0)
    assert r.mean_rank[1] is None
    assert r.significant(0.3) == [(int(i), int(j)) for i, j in np.argwhere(r.p_adj <= 0.3)]
    assert r.significant(0.3, adjusted=False) == [(int(i), int(j)) for i, j in np.argwhere(r.q <= 0.3)]
    rows = r.table()
    assert len(rows) == P * 2 and rows[3] == dict(feature=1, covariate="age", statistic=r.statistic[1, 1], rho=r.rho[1, 1], p=r.p[1, 1], p_adj=r.p_adj[1, 1], q=r.q[1, 1])
    # an array of covariates with names and kinds; cluster labels as they stand
    a = mmm.associate_exposures(E, np.stack([codes, age], axis=1), kinds=["categorical", None], names=["subtype", "age"], strata=site, permutations=B, seed=13)
    assert _bits(a.p, r.p) and _bits(a.p_adj, r.p_adj) and _bits(a.statistic, r.statistic)
    labels = np.arange(D, dtype=np.int64) % 3
    b = mmm.associate_exposures(E, {"cluster": labels}, permutations=10, seed=1)
    assert b.levels[0].tolist() == [0, 1, 2] and b.p.shape == (P, 1)


def test_planted_associations_come_back_on_the_device(mmm):
    """follows from the bitwise equality with the restatement (whose behaviour on these inputs tests/test_associate_cpu.py asserts); asserted anyway"""
    x, y, levels, pairs = A.planted()
    ref = A.planted_reference()
    raw = mmm.associate._raw(mmm.default_context(), x, levels, y, None, A.PLANTED_B, 0, 1000 + A.PLANTED_SEED)
    for k in KEYS:
        assert _bits(raw[k], getattr(ref, k)), k
    r = mmm.associate_exposures(x, {"group": y[:, 0].astype(int), "score": y[:, 1], "batch": y[:, 2].astype(int)}, permutations=A.PLANTED_B, seed=1000 + A.PLANTED_SEED)
    assert sorted(r.significant(0.01)) == sorted(pairs) and sorted(r.significant(0.05)) == sorted(pairs)
    assert r.rho[1, 1] > 0.5
    xc, yc, lc, s = A.confounded()
    free = mmm.associate_exposures(xc, {"v": yc[:, 0]}, permutations=999, seed=11)
    held = mmm.associate_exposures(xc, {"v": yc[:, 0]}, strata=s, permutations=999, seed=11)
    assert free.p_adj[0, 0] <= 0.001 and held.p_adj[0, 0] > 0.05 and _bits(free.statistic, held.statistic)
