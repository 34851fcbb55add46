"""mmm_regress_exposures on the device against its numpy restatement (tests/regress_ref.py): every output bit for bit (every f64 sum runs in a
written order, nothing is contracted); the invariances the definition promises (waves -- which also move the tile shape and, with it, whether
the rows sit in LDS --, a second run, slices, additivity, the identity outputs independent of the permutations); B = 0; NULL outputs; every
error with the outputs untouched; the Python layer against its composition by hand; the planted and the confounded cohorts."""
import ctypes

import numpy as np
import pytest

import regress_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("obs", "u_obs", "rz_obs", "ge", "ge_max", "maxstat")
CASES = {c.name: c for c in R.cases()}


def _run(mmm, c, b0=None, B=None, waves=0, seed=None, **kw):
    return mmm.regress._raw(mmm.default_context(), c.e, c.qz, c.cols, c.w, c.strata, c.B if B is None else B, c.b0 if b0 is None else b0,
                            c.seed if seed is None else seed, 0, waves, **kw)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _same(a, b, what=""):
    for k in KEYS:
        assert _bits(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_equal_the_restatement(mmm, name):
    c = CASES[name]
    got, ref = _run(mmm, c), R.reference(c)
    for k in KEYS:
        want = getattr(ref, k)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, k)
        assert _bits(got[k], want), (name, k, np.argwhere(got[k] != want)[:10].tolist())


# D4096 and full read their rows from memory, the others hold them in LDS; P33, P64, ones64, Q64 and full take 4 x 4 tiles at some or all waves
@pytest.mark.parametrize("name", ["D2", "D17", "D65", "D257", "D4096", "P33", "P64", "A0", "A32", "Q64", "ones64", "full", "contents", "rzneg", "sizes", "unordered"])
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
    for k in ("obs", "u_obs", "rz_obs"):
        assert _bits(whole[k], head[k]) and _bits(whole[k], tail[k]), k
    # more replicates than blocks in flight, up to the last global index
    many = CASES["many"]
    top = 2 ** 31 - 1 - many.B
    high = _run(mmm, many, b0=top)
    _same(high, _run(mmm, many, b0=top, waves=1), "3000 replicates")
    part = R.reference(many, b0=2 ** 31 - 1 - 4, B=4)
    assert _bits(np.ascontiguousarray(high["maxstat"][-4:]), part.maxstat)
    rest, last = _run(mmm, many, b0=top, B=many.B - 4), _run(mmm, many, b0=2 ** 31 - 1 - 4, B=4)
    assert _bits(last["ge"], part.ge) and _bits(last["ge_max"], part.ge_max)
    assert _bits(high["ge"], rest["ge"] + last["ge"]) and _bits(high["ge_max"], rest["ge_max"] + last["ge_max"])


def test_the_identity_outputs_do_not_depend_on_the_permutations(mmm):
    c = CASES["contents"]
    base = _run(mmm, c)
    for kw in (dict(seed=99), dict(B=3), dict(b0=1000), dict(B=0)):
        got = _run(mmm, c, **kw)
        assert _bits(got["obs"], base["obs"]) and _bits(got["u_obs"], base["u_obs"]) and _bits(got["rz_obs"], base["rz_obs"]), kw
    assert not _bits(_run(mmm, c, seed=99)["maxstat"], base["maxstat"])


def test_no_permutations_and_strata_of_one(mmm):
    c = CASES["D63"]
    ref = R.reference(c)
    got = _run(mmm, c, B=0)
    assert _bits(got["obs"], ref.obs) and _bits(got["u_obs"], ref.u_obs) and _bits(got["rz_obs"], ref.rz_obs) and got["maxstat"].shape == (0, 3)
    assert not got["ge"].any() and not got["ge_max"].any()
    alone = _run(mmm, CASES["allalone"])
    assert (alone["ge"] == 10).all() and (alone["ge_max"] == 10).all() and _bits(alone["maxstat"], np.tile(alone["obs"].max(axis=0), (10, 1)))


def test_null_outputs_are_accepted(mmm):
    c = CASES["D65"]
    full = _run(mmm, c)
    for outs in ((), ("u_obs",), ("rz_obs",), ("maxstat",), ("u_obs", "rz_obs")):
        got = _run(mmm, c, outputs=outs)
        assert sorted(got) == sorted(("obs", "ge", "ge_max") + outs)
        for k in got:
            assert _bits(got[k], full[k]), (outs, k)


def test_every_error(mmm):
    c = CASES["D65"]
    L, ctx = mmm.lib(), mmm.default_context()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    plain = ctypes.CFUNCTYPE(ci, vp, ci, ci, vp, ci, vp, ci, vp, vp, vp, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ci, vp, vp, vp, vp, vp, vp)(("mmm_regress_exposures", L))
    keep = []

    def call(h=True, e=c.e, qz=c.qz, cols=c.cols, w=c.w, D=None, P=None, A=None, C=None, strata=None, B=2, b0=0, waves=0, null=()):
        e = np.ascontiguousarray(e, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        qz = None if qz is None else np.ascontiguousarray(qz, dtype=np.float64)
        cl = np.ascontiguousarray(cols, dtype=np.int32)
        D = e.shape[0] if D is None else D
        P = e.shape[1] if P is None else P
        A = (0 if qz is None else qz.shape[1]) if A is None else A
        C = cl.size if C is None else C
        st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32)
        P1, C1, Q1 = max(P, 1), max(C, 1), max(int(np.abs(cl).sum()), 1)
        out = dict(obs=np.full((P1, C1), 7.0), u_obs=np.full((P1, Q1), 7.0), rz_obs=np.full(P1, 7.0), ge=np.full((P1, C1), 7, dtype=np.uint32),
                   ge_max=np.full((P1, C1), 7, dtype=np.uint32), maxstat=np.full((max(B, 1), C1), 7.0))
        arrs = dict(e=e, cols=cl, w=w)
        if qz is not None:
            arrs["qz"] = qz
        keep.append((arrs, out, st))
        p = {k: (None if k in null else v.ctypes.data) for k, v in list(arrs.items()) + list(out.items())}
        rc = plain(ctx.h if h else None, D, P, p["e"], A, p.get("qz"), C, p["cols"], p["w"], None if st is None else st.ctypes.data, B, b0, 5, 0, waves, p["obs"],
                   p["u_obs"], p["rz_obs"], p["ge"], p["ge_max"], p["maxstat"])
        untouched = {k for k, v in out.items() if (v == 7).all()}
        return rc, (L.mmm_last_error(ctx.h) or b"").decode(), untouched

    everything = {"obs", "u_obs", "rz_obs", "ge", "ge_max", "maxstat"}
    rc, _, untouched = call()
    assert rc == 0 and not untouched
    rc, _, untouched = call(B=0)                                         # the identity outputs are written, the counts are not
    assert rc == 0 and untouched == {"ge", "ge_max", "maxstat"}
    rc, _, untouched = call(B=0, null=("ge", "ge_max", "maxstat", "u_obs", "rz_obs"))
    assert rc == 0 and untouched == everything - {"obs"}
    arg = [dict(h=False), dict(D=0), dict(D=-1), dict(P=0), dict(C=0), dict(C=-1), dict(A=-1), dict(cols=(1, 0, 1)), dict(cols=(1, -2, 1)), dict(B=-1), dict(b0=-1),
           dict(b0=2 ** 31 - 2, B=2), dict(waves=3), dict(waves=32), dict(waves=-1), dict(null=("e",)), dict(null=("cols",)), dict(null=("w",)), dict(null=("qz",)),
           dict(null=("obs",)), dict(null=("ge",)), dict(null=("ge_max",)), dict(strata=[0] * 64 + [65]), dict(strata=[-1] + [0] * 64)]
    for kw in arg:
        rc, msg, untouched = call(**kw)
        assert rc == -1 and untouched == everything, (kw, rc, msg)
    for bad in (np.nan, np.inf, -np.inf, 1.0001e70, -1.0001e70):                 # the magnitude bound keeps every sum finite
        for name, src in (("e", c.e), ("qz", c.qz), ("w", c.w)):
            m = src.copy(); m[7, 1] = bad
            rc, msg, untouched = call(**{name: m})
            assert rc == -1 and untouched == everything and "%s entry (7, 1)" % name in msg, (bad, name, msg)
    assert call(strata=[64] + [0] * 64)[0] == 0                          # the bound itself is accepted
    top = c.e.copy(); top[7, 1] = -1e70
    assert call(e=top)[0] == 0
    # too few residual degrees of freedom, with the figures: D - A - cols >= 1 makes D = 1 unreachable
    rc, msg, untouched = call(e=np.zeros((1, 1)), qz=None, cols=(1,), w=np.ones((1, 1)))
    assert rc == -1 and untouched == everything and "1 - 0 - 1" in msg, msg
    rc, msg, untouched = call(e=c.e[:5], qz=c.qz[:5], cols=(1, 3), w=c.w[:5])
    assert rc == -1 and untouched == everything and "covariate 1" in msg and "5 - 2 - 3" in msg, msg
    assert call(e=c.e[:5], qz=c.qz[:5], cols=(1, 2), w=c.w[:5, :3])[0] == 0
    # limits, each with its figure in the message
    rc, msg, untouched = call(e=np.zeros((4097, 1)), qz=None, cols=(1,), w=np.zeros((4097, 1)))
    assert rc == -4 and untouched == everything and "4097" in msg and "4096" in msg, msg
    rc, msg, untouched = call(e=np.zeros((70, 65)), qz=None, cols=(1,), w=np.zeros((70, 1)))
    assert rc == -4 and untouched == everything and "65" in msg and "64" in msg, msg
    rc, msg, untouched = call(e=np.zeros((70, 1)), qz=np.zeros((70, 33)), cols=(1,), w=np.zeros((70, 1)))
    assert rc == -4 and untouched == everything and "33" in msg and "32" in msg, msg
    rc, msg, untouched = call(e=np.zeros((90, 1)), qz=None, cols=(32, 33), w=np.zeros((90, 65)))
    assert rc == -4 and untouched == everything and "65" in msg and "64" in msg, msg


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_python_is_its_composition_done_by_hand(mmm):
    rng = np.random.default_rng(8)
    D, P, B = 50, 4, 60
    E = rng.random((D, P))
    E[rng.permutation(D)[:30], 1] = 0.0
    grp = np.array(["lum", "basal", "her2"])[rng.integers(0, 3, size=D)]
    brca = rng.integers(0, 2, size=D).astype(bool)
    age = np.round(rng.uniform(30, 80, size=D))
    burden = np.exp(rng.standard_normal(D))
    site = rng.integers(0, 2, size=D)
    cov, adj = {"subtype": grp, "brca": brca, "burden": burden}, {"age": age}
    r = mmm.regress_exposures(E, cov, adj, strata=site, permutations=B, seed=13)
    # the inputs by the package's own design (tests/test_regress_cpu.py holds it to one built by hand), the call by the restatement
    names, y, levels, values = mmm.associate._covariates(cov, None, None, D)
    an, ay, al, _ = mmm.associate._covariates(adj, None, None, D)
    d = mmm.regress._design(E, y, levels, names, ay, al, an, True)
    ref = R.regress(d["e"], d["qz"], d["cols"], d["w"], site, B, 0, 13)
    raw = mmm.regress._raw(mmm.default_context(), d["e"], d["qz"], d["cols"], d["w"], site, B, 0, 13)
    for k in KEYS:
        assert _bits(raw[k], getattr(ref, k)), k
    lv = np.unique(grp)
    assert r.permutations == B and r.names == ["subtype", "brca", "burden"] and r.levels[0].tolist() == lv.tolist() and r.levels[2] is None
    assert _bits(r.partial_r2, ref.obs) and _bits(r.p, (1.0 + ref.ge) / (1.0 + B)) and _bits(r.p_adj, (1.0 + ref.ge_max) / (1.0 + B))
    assert r.df.tolist() == [[2, D - 2 - 2], [1, D - 2 - 1], [1, D - 2 - 1]]
    assert np.allclose(r.q, mmm.associate.benjamini_hochberg(r.p), rtol=1e-14, atol=0)
    # the reported columns against a least-squares fit on the ranks
    rk = np.stack([R.midrank(E[:, p]) for p in range(P)], axis=1)
    Z = np.stack([np.ones(D), R.midrank(age)], axis=1)
    for j, col in ((1, brca.astype(float)), (2, R.midrank(burden))):
        M = np.concatenate([Z, col[:, None]], axis=1)
        beta = np.linalg.lstsq(M, rk, rcond=None)[0]
        res = rk - M @ beta
        se = np.sqrt((res * res).sum(axis=0) / (D - 3) * np.linalg.inv(M.T @ M)[-1, -1])
        assert np.allclose(r.coef[:, j], beta[-1], rtol=1e-9, atol=1e-9) and np.allclose(r.t[:, j], beta[-1] / se, rtol=1e-9, atol=1e-9)
        assert np.allclose(r.F[:, j], r.t[:, j] ** 2, rtol=1e-12)
    assert np.isnan(r.t[:, 0]).all() and np.isnan(r.coef[:, 0]).all() and (r.F[:, 0] >= 0).all()
    assert r.significant(0.3) == [(int(i), int(j)) for i, j in np.argwhere(r.p_adj <= 0.3)]
    assert r.significant(0.3, adjusted=False) == [(int(i), int(j)) for i, j in np.argwhere(r.q <= 0.3)]
    rows = r.table()
    assert len(rows) == P * 3 and rows[5] == dict(feature=1, covariate="burden", partial_r2=r.partial_r2[1, 2], F=r.F[1, 2], t=r.t[1, 2], coef=r.coef[1, 2],
                                                  p=r.p[1, 2], p_adj=r.p_adj[1, 2], q=r.q[1, 2])
    # arrays with names and kinds; no adjuster at all equals the rank statistic of associate_exposures
    a = mmm.regress_exposures(E, np.stack([np.unique(grp, return_inverse=True)[1], brca, burden], axis=1), age, kinds=["categorical", "categorical", None],
                              names=["subtype", "brca", "burden"], strata=site, permutations=B, seed=13)
    assert _bits(a.p, r.p) and _bits(a.p_adj, r.p_adj) and _bits(a.partial_r2, r.partial_r2)
    free = mmm.regress_exposures(E, cov, None, permutations=10, seed=1)
    assoc = mmm.associate_exposures(E, cov, permutations=10, seed=1)
    assert np.allclose((D - 1) * free.partial_r2, assoc.statistic, rtol=1e-10, atol=1e-10) and np.allclose(free.t[:, 2] / np.sqrt(free.t[:, 2] ** 2 + D - 2), assoc.rho[:, 2], atol=1e-10)


def test_planted_effects_come_back_on_the_device(mmm):
    """follows from the bitwise equality with the restatement (whose behaviour on these inputs tests/test_regress_cpu.py asserts); asserted anyway"""
    x, cov, age, pairs = R.planted()
    for adjusted in (True, False):
        e, qz, cols, w = R.planted_inputs(adjusted)
        ref = R.planted_reference(adjusted)
        raw = mmm.regress._raw(mmm.default_context(), e, qz, cols, w, None, R.PLANTED_B, 0, 1000 + R.PLANTED_SEED)
        for k in KEYS:
            assert _bits(raw[k], getattr(ref, k)), (adjusted, k)
    r = mmm.regress_exposures(x, cov, {"age": age}, permutations=R.PLANTED_B, seed=1000 + R.PLANTED_SEED)
    assert sorted(r.significant(0.01)) == sorted(pairs) and sorted(r.significant(0.05)) == sorted(pairs)
    assert (r.p_adj[:, 3] > 0.05).all() and r.coef[0, 0] > 0 and r.t[1, 1] > 3
    free = mmm.regress_exposures(x, cov, None, permutations=R.PLANTED_B, seed=1000 + R.PLANTED_SEED)
    assert (free.p_adj[:3, 3] <= 0.001).all()
    # one confounded null cohort, the plain linear model: rejected without the adjuster, not with it, bit for bit the restatement's counts
    xc, v, a = R.confounded(5002)
    for adjusted, adj in ((True, {"age": a}), (False, None)):
        e, qz, cols, w = R.confounded_inputs(5002, adjusted)
        ref = R.regress(e, qz, cols, w, None, R.CONFOUNDED_B, 0, 5002)
        raw = mmm.regress._raw(mmm.default_context(), e, qz, cols, w, None, R.CONFOUNDED_B, 0, 5002)
        for k in KEYS:
            assert _bits(raw[k], getattr(ref, k)), (adjusted, k)
        got = mmm.regress_exposures(xc, {"v": v}, adj, ranks=False, permutations=R.CONFOUNDED_B, seed=5002)
        assert (got.p[0, 0] > 0.05) == adjusted and (adjusted or got.p[0, 0] <= 0.01)
