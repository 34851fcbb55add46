"""The definition of the signature decomposition as its numpy restatement computes it (tests/decompose_ref.py): the running maximum of its
gain IS the non-negative least-squares optimum over the supports of at most s rows (against a brute force that shares no code with the
Gram route), degenerate rows never meet in a subset, exact ties go to the lower row; then the selection rule and the shares on hand-made
paths, the argument checks of the Python layer, and the declarations."""
import itertools
import os
import re

import numpy as np
import pytest

import decompose_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(seed, C, n, noise):
    """C <= 10 rows over V = 24 terms with a scaled duplicate (row C - 2 = 2.5 x row 1), an exact duplicate (row C // 2 = row 0) and an in-span
    row (row 3 = a blend of rows 4 and 5); planted 1-3-member mixtures, with 2 % noise or without"""
    rng = np.random.default_rng(seed)
    cat = DR.catalogue(rng, C, 24)
    sig = np.zeros((n, 24))
    for i in range(n):
        m = 1 + i % 3
        sig[i] = rng.uniform(0.2, 1.0, size=m) @ cat[np.sort(rng.choice(C, size=m, replace=False))]
        if noise:
            sig[i] *= rng.gamma(2500.0, 1.0 / 2500.0, size=24)
    return cat, sig


def _brute_lstsq(cat, x, S):
    """best[s - 1] = the largest ss - |x - A_T w|^2 over the supports T of at most s rows whose least-squares solution (numpy.linalg.lstsq on
    the tall V x |T| matrix) is positive"""
    C = cat.shape[0]
    ss = float(x @ x)
    best = np.zeros(S)
    for t in range(1, S + 1):
        top = best[t - 2] if t > 1 else 0.0
        for T in itertools.combinations(range(C), t):
            A = cat[list(T)].T
            w = np.linalg.lstsq(A, x, rcond=None)[0]
            if (w > 0).all():
                r = x - A @ w
                top = max(top, ss - float(r @ r))
        best[t - 1] = top
    return best


@pytest.mark.parametrize("seed,C,S,noise", [(1, 9, 4, True), (2, 9, 4, False), (3, 10, 3, True), (4, 6, 4, False), (6, 8, 4, True)])
def test_running_maximum_of_the_gain_is_the_nnls_optimum(seed, C, S, noise):
    """Tolerance 1e-12 ss (measured: <= 1e-15 ss): the Gram route squares the condition number of a subset, and the test asserts that every
    admissible subset of its inputs has min_i d_i / g_ii >= 1e-3, so that square is bounded by about 1e6 x 2^-53 relative."""
    cat, sig = _inputs(seed, C, 6, noise)
    G, b, ss = DR.moments(sig, cat)
    stats = {}
    subset, weight, gain, cosine = DR.search(G, b, ss, S, stats)
    assert stats["ratio"] >= 1e-3, stats["ratio"]
    assert stats["sizes_found"][:, 0].all()
    run = np.maximum.accumulate(gain, axis=1)
    worst = 0.0
    for i in range(sig.shape[0]):
        want = _brute_lstsq(cat, sig[i], S)
        err = float(np.abs(run[i] - want).max()) / ss[i]
        worst = max(worst, err)
        assert err <= 1e-12, (i, run[i], want)
    print("C = %d, S = %d, noise %s: max |running gain - brute force| / ss = %.3g, smallest admissible d / g = %.3g" % (C, S, noise, worst, stats["ratio"]))
    # the reconstruction of every reported subset has the squared residual ss - gain and the cosine sqrt(gain / ss)
    for i in range(sig.shape[0]):
        for s in range(S):
            m = subset[i, s][subset[i, s] >= 0]
            if not m.size:
                continue
            rec = weight[i, s, :m.size] @ cat[m]
            assert abs(float((sig[i] - rec) @ (sig[i] - rec)) - (ss[i] - gain[i, s])) <= 1e-12 * ss[i]
            assert abs(float(rec @ sig[i]) / np.sqrt(float(rec @ rec) * ss[i]) - cosine[i, s]) <= 1e-9


def test_running_maximum_against_scipy_nnls():
    nnls = pytest.importorskip("scipy.optimize").nnls
    cat, sig = _inputs(11, 9, 6, True)
    G, b, ss = DR.moments(sig, cat)
    S = 4
    gain = DR.search(G, b, ss, S)[2]
    run = np.maximum.accumulate(gain, axis=1)
    for i in range(sig.shape[0]):
        best = np.zeros(S)
        for t in range(1, S + 1):
            best[t - 1] = max(ss[i] - nnls(cat[list(T)].T, sig[i])[1] ** 2 for T in itertools.combinations(range(9), t))
        assert float(np.abs(run[i] - best).max()) <= 1e-12 * ss[i], (i, run[i], best)


def test_duplicates_and_in_span_rows_are_never_co_members():
    C = 10
    cat, sig = _inputs(21, C, 9, True)
    G, b, ss = DR.moments(sig, cat)
    subset = DR.search(G, b, ss, 4)[0]
    for rows in subset.reshape(-1, 4):
        m = set(rows[rows >= 0].tolist())
        assert not {1, C - 2} <= m and not {0, C // 2} <= m and not {3, 4, 5} <= m, m
    for T in ((1, C - 2), (0, C // 2), (3, 4, 5), (0, 3, 4, 5)):                # and the subsets themselves fail the pivot test, whatever b
        assert not DR.evaluate(G, b[0], T)[0]
    assert DR._solve(G[np.ix_([3, 4], [3, 4])][None], b[0][[3, 4]][None])[3][0] > 1e-3      # (a blend row with ONE of its parts is no such pair)


def test_exact_ties_go_to_the_lower_row():
    rng = np.random.default_rng(5)
    cat = DR.catalogue(rng, 6, 24, degenerate=False)
    cat[4] = cat[2]                                               # rows 2 and 4 are equal: every subset with one has a twin with the other
    sig = np.stack([cat[2], 0.3 * cat[2] + 0.7 * cat[5]]) * rng.gamma(2500.0, 1.0 / 2500.0, size=(2, 24))
    G, b, ss = DR.moments(sig, cat)
    assert np.array_equal(G[2], G[4]) and np.array_equal(b[:, 2], b[:, 4])
    subset, _, gain, _ = DR.search(G, b, ss, 2)
    assert subset[0, 0].tolist() == [2, -1] and subset[1, 1].tolist() == [2, 5]
    assert DR.evaluate(G, b[0], (4,))[1] == gain[0, 0] and DR.evaluate(G, b[1], (4, 5))[1] == gain[1, 1]      # the twins tie exactly


def test_empty_outputs():
    """ss = 0, sizes beyond C and sizes without an admissible subset come out as subset -1, weight 0, gain 0, cosine 0"""
    rng = np.random.default_rng(6)
    cat = DR.catalogue(rng, 2, 24, degenerate=False)
    sig = np.stack([np.zeros(24), cat[0]])
    G, b, ss = DR.moments(sig, cat)
    subset, weight, gain, cosine = DR.search(G, b, ss, 3)
    assert (subset[0] == -1).all() and not weight[0].any() and not gain[0].any() and not cosine[0].any()
    assert (subset[1, 2] == -1).all() and gain[1, 2] == 0.0                   # s = 3 > C = 2
    assert subset[1, 0].tolist() == [0, -1, -1] and cosine[1, 0] == 1.0


def test_selection_rule_and_shares_on_hand_made_paths(mmm):
    dc = mmm.decompose
    pc = np.array([[0.80, 0.97, 0.975],       # the third member adds 0.005 < 0.01: size 2
                   [0.99, 0.95, 0.992],       # size 1 is within the margin already
                   [0.50, 0.40, 0.90],        # cbest = .5 .5 .9: size 3
                   [0.90, 0.90, 0.90],        # flat: size 1
                   [0.00, 0.00, 0.00]])       # nothing admissible
    assert dc.choose_size(pc, 0.01).tolist() == [2, 1, 3, 1, 1]
    assert dc.choose_size(pc, 0.2).tolist() == [1, 1, 3, 1, 1]
    assert dc.choose_size(pc[0], 0.004).tolist() == 3
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="min_gain"):
            dc.choose_size(pc, bad)
    sub = np.full((5, 3, 3), -1, dtype=np.int32); wt = np.zeros((5, 3, 3))
    for i in range(4):
        sub[i, 0, :1] = [4]; sub[i, 1, :2] = [1, 3]; sub[i, 2, :3] = [0, 2, 5]
        wt[i, 0, :1] = [2.0]; wt[i, 1, :2] = [3.0, 1.0]; wt[i, 2, :3] = [1.0, 1.0, 2.0]
    rowsum = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 0.5])
    d = dc.compose(dc.SearchResult(sub, wt, np.zeros((5, 3)), pc), rowsum, 0.01, names=list("ABCDEF"))
    assert d.size.tolist() == [2, 1, 3, 1, 0]
    assert d.members.tolist() == [[1, 3, -1], [4, -1, -1], [0, 2, 5], [4, -1, -1], [-1, -1, -1]]
    assert d.cosine.tolist() == [0.97, 0.99, 0.90, 0.90, 0.0]
    assert d.shares[0].tolist() == [0.6, 0.4, 0.0]                # 3 x 2 : 1 x 4
    assert d.shares[2].tolist() == [0.2, 0.6, 0.2]                # 1 x 1 : 1 x 3 : 2 x 0.5
    assert d.shares[1].tolist() == [1.0, 0.0, 0.0] and not d.shares[4].any()
    assert d.describe() == ["60.0% B + 40.0% D (cosine 0.9700)", "100.0% E (cosine 0.9900)", "20.0% A + 60.0% C + 20.0% F (cosine 0.9000)",
                            "100.0% E (cosine 0.9000)", "no admissible mixture"]
    assert d._replace(names=None).describe()[0] == "60.0% row 1 + 40.0% row 3 (cosine 0.9700)"
    assert d.allowed(6).tolist() == [True, True, True, True, True, True]
    assert d._replace(members=d.members[:2]).allowed(7).tolist() == [False, True, False, True, True, False, False]      # by hand: rows 1, 3 and 4
    with pytest.raises(ValueError, match="row 5"):
        d.allowed(5)
    # where a smaller size attains the same cosine as the chosen one, its members are reported
    pc2 = np.array([[0.5, 0.5, 0.5]])
    assert dc.compose(dc.SearchResult(sub[:1], wt[:1], np.zeros((1, 3)), pc2), rowsum, 0.01).members.tolist() == [[4, -1, -1]]


def test_arguments_are_checked_before_a_device_is_asked_for(mmm, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(mmm._lib, "default_context", no_device)
    monkeypatch.setattr(mmm.decompose, "lib", no_device)
    rng = np.random.default_rng(0)
    cat = rng.dirichlet(np.ones(8), size=5); sig = rng.dirichlet(np.ones(8), size=2)
    f = mmm.decompose_signatures
    with pytest.raises(ValueError, match="2 terms and the catalogue 8"):
        f(sig[:, :2], cat)
    with pytest.raises(ValueError, match="dimensions"):
        f(sig[0], cat)
    with pytest.raises(ValueError, match="negative or non-finite"):
        f(-sig, cat)
    bad = cat.copy(); bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="negative or non-finite"):
        f(sig, bad)
    zero = cat.copy(); zero[3] = 0.0
    with pytest.raises(ValueError, match="row 3 is all zero"):
        f(sig, zero)
    for S in (0, -1, 2.5):
        with pytest.raises(ValueError, match="max_size must be an integer >= 1"):
            f(sig, cat, max_size=S)
    with pytest.raises(ValueError, match="max_size = 7 \\(limit 6\\)"):
        f(sig, cat, max_size=7)
    with pytest.raises(ValueError, match="C = 257 catalogue rows \\(limit 256\\)"):
        f(np.ones((1, 3)), np.ones((257, 3)))
    with pytest.raises(ValueError, match="8809549056 subsets of the largest size \\(limit 2\\^32 - 1\\)"):
        f(np.ones((1, 3)), np.ones((256, 3)), max_size=5)
    for g in (0.0, -0.1, np.nan):
        with pytest.raises(ValueError, match="min_gain"):
            f(sig, cat, min_gain=g)
    with pytest.raises(ValueError, match="names holds 2 entries"):
        f(sig, cat, names=["a", "b"])
    for kind in (mmm.ILDA, mmm.IMMCTM):
        with pytest.raises(TypeError, match="factorised"):
            f(object.__new__(kind), cat)
        with pytest.raises(TypeError, match="factorised"):
            f(sig, object.__new__(kind))
    s = mmm.decompose_search
    G, b, ss = DR.moments(sig, cat)
    with pytest.raises(ValueError, match="G must be"):
        s(G[:, :3], b, ss, 2)
    with pytest.raises(ValueError, match="b must be"):
        s(G, b[:, :3], ss, 2)
    with pytest.raises(ValueError, match="ss must be"):
        s(G, b, ss[:1], 2)
    with pytest.raises(ValueError, match="limit 6"):
        s(G, b, ss, 7)
    with pytest.raises(AssertionError, match="device call"):      # valid arguments do go on to the device
        f(sig, cat)


def test_declarations(mmm):
    hdr = open(os.path.join(ROOT, "include", "mmmusig.h")).read()
    for name, nargs in (("mmm_decompose_search", 11), ("mmm_signature_decompose", 14)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == nargs
        assert name in mmm._lib.declared_symbols() and len(mmm._lib._SIGS[name][1]) == nargs
    assert re.search(r"MMM_OFF_DECOMPOSE_LDS = 1 << 16", hdr) and mmm._lib.OFF["decompose_lds"] == 1 << 16
    assert re.search(r"#define MMM_VERSION 123\b", hdr)
    for name in ("decompose_signatures", "decompose_search", "Decomposition", "SearchResult"):
        assert name in mmm.__all__ and hasattr(mmm, name)
    assert mmm.Decomposition._fields == ("size", "members", "weights", "shares", "cosine", "path_members", "path_weights", "path_cosine", "names")
