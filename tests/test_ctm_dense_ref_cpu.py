"""tests/ctm_dense_ref.py against the index-order C oracle (oracle/mmm_oracle.c), and the case table of tests/test_ctm_dense_dispatch_gpu.py
against the rules by which a handle takes the rows-of-counts kernels.  No GPU.

For every case the oracle runs ONE pass of fit! from the case's written (λ, ν); the restatement must reproduce ζ, Σθ, γ, Elnϕ of that
state and props / ll of the oracle's post-solve λ and new γ within max(a-priori bound, F = 4 units), the unit being the gap between the
restatement in float64 index order and in np.longdouble -- the criterion the device is held to.  The worst ratios are printed per
quantity (DESIGN.md sections 4.4 / 4.7 carry them)."""
import mpmath as mp
import numpy as np
import pytest
from scipy.special import digamma

import ctm_dense_ref as R

CASES = R.cases()
NAMES = [c["name"] for c in CASES]
WORST = {}


def _oracle(oracle, c):
    g0 = c["g0"] if c["features"] is not None else np.concatenate([g.ravel() for g in c["g0"]])
    o = oracle.CtmOracle(c["K"], c["alpha"], c["X"], V=None if c["features"] is not None else c["V"], features=c["features"], gamma0=g0)
    return o


@pytest.mark.parametrize("name", NAMES)
def test_oracle_pass_meets_the_restatement(oracle, name):
    c = CASES[NAMES.index(name)]
    s = R.spec_of(c)
    o = _oracle(oracle, c)
    E0 = o.Elnphi.copy()
    o.lam[:] = c["lam"].ravel(); o.nu[:] = c["nu"].ravel()
    ll = o.fit(maxiter=1, tol=0.0)[0]
    ref = R.Reference(s, c["lam"], c["nu"], E0)
    sumth = np.stack([o.sumtheta(d) for d in range(s.D)])
    r = ref.compare_state(o.zeta, o.gamma, o.Elnphi, sumth=sumth)
    ra, ua = ref.compare_after(o.lam, o.gamma, None if s.imm else o.props, ll)
    r.update(ra)
    print("%-16s %s | units %s" % (name, " ".join("%s %.3f" % kv for kv in r.items()),
                                   " ".join("%s %.1e" % kv for kv in list(ref.unit.items()) + list(ua.items()))))
    for q, v in r.items():
        WORST[q] = max(WORST.get(q, 0.0), v)
        assert v <= 1.0, "%s: %s off by %.3g of its bound" % (name, q, v)


def test_case_table_reaches_every_build():
    theta, ll = set(), set()
    for c in CASES:
        b, kmx = R.dense_build(c["K"], c["V"])
        if c["dense"]:
            assert b is not None, c["name"]
            theta |= set(b); ll.add(kmx)
    assert theta == set(R.THETA_BUILDS), sorted(set(R.THETA_BUILDS) - theta)
    assert ll == set(R.LL_BUILDS)
    # K and V at both ends of every class, among the dense cases
    Ks = {k for c in CASES if c["dense"] for k in c["K"]}
    Vs = {v for c in CASES if c["dense"] for v in c["V"]}
    assert {1, 2, 8, 9, 10, 11, 13, 15, 16} <= Ks
    assert {1, 15, 16, 17, 32, 33, 48, 49, 96, 97, 128} <= Vs
    # the ll build's KMX above a modality's own
    assert any(c["dense"] and len({b[0] for b in R.dense_build(c["K"], c["V"])[0]}) > 1 for c in CASES)
    assert any(c["dense"] and len(c["K"]) == 8 for c in CASES) and any(c["features"] is not None for c in CASES)


@pytest.mark.parametrize("name", NAMES)
def test_case_admissibility(name):
    """A case meant to run over rows of counts satisfies every condition of create; one meant to be refused violates exactly one."""
    c = CASES[NAMES.index(name)]
    cond = R.conditions(c["K"], c["V"], c["X"])
    bad = [k for k in R.CONDITIONS if not cond[k]]
    if c["dense"]:
        assert bad == [], (name, bad)
        assert c["D"] <= 330 and (c["D"] * sum(c["K"]) * 8) < 2 ** 32
    else:
        assert bad == [c["violates"]], (name, bad)


def test_density_cases_sit_on_the_threshold():
    half, minus = CASES[NAMES.index("half")], CASES[NAMES.index("half_minus1")]
    for c, want in ((half, 0), (minus, 1)):
        listed = sum(x.shape[0] for doc in c["X"] for x in doc)
        assert c["D"] * sum(c["V"]) - 2 * listed == 2 * want


def test_rows_case_holds_what_it_names():
    c = CASES[NAMES.index("rows")]
    s = R.spec_of(c)
    assert (s.N[0][5] == 0).all() and (s.N[1][5] == 0).all()                     # a document empty in every modality
    assert (s.N[1][1] == 0).all() and (s.N[0][1] > 0).any()                      # ... and in one
    assert (s.N[1][:, 7] == 0).all()                                             # a term no document has
    assert any((x[:, 1] == 0).any() for doc in c["X"] for x in doc)              # a listed count 0
    slots = {(m, (int(t) - 1) >> 4) for doc in c["X"] for m, x in enumerate(doc) for t in x[x[:, 1] == 65535, 0]}
    assert {(1, 1), (1, 0), (0, 2), (0, 1)} <= slots                             # 65,535 in odd and even slots
    full = [d for d in range(s.D) if d != 5]
    assert (s.N[0][full] > 0).all() and R.dense_build(c["K"], c["V"])[0][0] == (8, 3)     # V = 48 fully present over three slots
    assert max(int(x[:, 1].max()) for doc in c["X"] for x in doc if x.size) == 65535


def test_grid_cases_cover_the_listed_sizes():
    got = {(d, b, cu) for d, b, cu in R.GRID_EDGES}
    assert {d for d, _, _ in got} == {1, 3, 4, 5, 31, 32, 33, 64, 65, 129}
    assert {b for _, b, _ in got} == {1, 2} and {cu for _, _, cu in got} == {1, 4}


def test_scipy_digamma_is_as_good_as_the_bound_assumes():
    """elnphi_bound allows the reference's digamma 4 u (|ψ| + 1): held against 40-digit mpmath on Dirichlet parameters from α to a corpus' total."""
    mp.mp.dps = 40
    rng = np.random.default_rng(5)
    xs = np.concatenate([10.0 ** rng.uniform(-1.2, 7, 1500), rng.uniform(1.3, 1.6, 300), [0.1, 1.4616321449683623]])
    worst =max(abs(float(mp.mpf(float(digamma(x))) - mp.digamma(mp.mpf(float(x))))) / (abs(float(mp.digamma(mp.mpf(float(x))))) + 1) for x in xs)
    print("scipy digamma: worst |err| / (|psi| + 1) = %.2e" % worst)
    assert worst <= 4 * R.U


def test_float64_restatement_is_a_rounding_of_the_longdouble_one():
    """The unit: the float64 index-order evaluation stays within the a-priori bounds of the np.longdouble one (it is one more association
    of the same sums), and is not identical to it."""
    c = CASES[NAMES.index("mix8_9")]
    s = R.spec_of(c)
    E0 = np.concatenate([(digamma(g) - digamma(g.sum(axis=1, keepdims=True))).ravel() for g in c["g0"]])
    ref = R.Reference(s, c["lam"], c["nu"], E0)
    for q in ("zeta", "sumth", "gamma"):
        assert 0.0 < ref.unit[q] <= float(np.max(ref.bound[q])), q


def test_zz_report():
    print("\nworst ratio to max(a-priori bound, 4 units), C oracle in index order: " + "  ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
