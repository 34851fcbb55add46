"""What the power entry's GPU suite rests on, checked on the numpy restatement alone (tests/power_ref.py), the invariants the definition
proves, and the argument checks of `presence_power` that need no device."""
import numpy as np
import pytest

import power_ref as W
import presence_ref as PR

G = len(W.FRACTIONS)
MARGIN = 1e-6           # relative to max(1, crit): the margin tests/test_presence_cpu.py asks of count_ge; the rounding bounds are below 1e-7


def _sorted_null(lv, B):
    """[B, H, TD] the null statistics of the first B replicates, descending"""
    return -np.sort(-lv.rep[0::G + 1, :B].transpose(1, 0, 2), axis=0)


@pytest.mark.parametrize("i", range(len(W.SHAPES) + 1), ids=lambda i: W.corpora()[i].name)
def test_no_comparison_of_the_gpu_cases_is_near_a_tie(i):
    """count_reject compares values that hold a device log with crit, which is one of them; two implementations agree on it as an integer
    where no Λ is near crit and the selection of crit cannot flip.  For every corpus and every (B, α) of power_ref.CASES (m = 0, 1, 4, 7):
    every Λ^l_b equals crit bit for bit (crit itself, and the point mass at 0) or |Λ^l_b - crit| >= 1e-6 max(1, crit); s_m, s_{m+1}, s_{m+2}
    are pairwise bit-equal or separated by as much; every rounding bound 2 (bound(ll0) + bound(ll1)) is below 1e-7.
    Smallest |Λ - crit| / max(1, crit) found off the ties (seeds of power_ref.SEEDS, the corpora's own): 6.6e-5 (C12V96), 6.7e-4 (edge),
    7.0e-4 (C4V5), 1.3e-3 (C6V1536); largest rounding bound 2.9e-8 (C6V1536).
    And what the definition proves: count_reject at φ = 0 is at most max(m, 0); nothing is written for an untestable item."""
    c = W.corpora()[i]
    lv = W.reference_levels(i)
    live = lv.obs.status != 3
    assert live.any() and np.nanmax(lv.rep_bound) < 1e-7
    assert np.isnan(lv.rep[:, :, ~live]).all() and not np.isnan(lv.rep[:, :, live]).any()
    for B, alpha in W.CASES:
        p = W.power(lv, G, alpha, B=B)
        assert p.m == {(24, 0.05): 0, (40, 0.05): 1, (24, 0.2): 4, (40, 0.2): 7}[(B, alpha)]
        cr = np.repeat(p.crit, G + 1, axis=0)[:, None, :][:, :, live]
        rep = p.rep[:, :, live]
        assert np.isfinite(cr).all()
        far = np.abs(rep - cr) >= MARGIN * np.maximum(1.0, cr)
        assert ((rep == cr) | far).all(), (c.name, B, alpha, np.abs(rep - cr)[~((rep == cr) | far)])
        s = _sorted_null(lv, B)[:, :, live]
        for a, b in ((p.m - 1, p.m), (p.m, p.m + 1)):
            if a >= 0 and b < B:
                assert ((s[a] == s[b]) | (s[a] - s[b] >= MARGIN * np.maximum(1.0, s[b]))).all(), (c.name, B, alpha, a)
        assert np.array_equal(s[p.m], p.crit[:, live])
        assert (p.count_reject[0::G + 1] <= max(p.m, 0)).all()
        assert (p.count_reject[:, ~live] == 0).all() and (p.count_zero[:, ~live] == 0).all() and (p.crit[:, ~live] == 0).all()
        print("%s B=%d α=%g: mean power per level %s" % (c.name, B, alpha, (p.count_reject[:, live].mean(axis=1) / B).round(2).tolist()))


def test_a_test_that_cannot_reject_has_infinite_crit_and_zero_counts():
    lv = W.reference_levels(0)
    live = lv.obs.status != 3
    p = W.power(lv, G, 0.05, B=5)                    # floor(0.05 * 6) - 1 = -1
    assert p.m == -1 and np.isinf(p.crit[:, live]).all() and (p.count_reject == 0).all()
    m, cr = W.critical(np.zeros((3, 2)), 0.999999)   # m + 1 > B cannot happen for α < 1: floor(α (B + 1)) <= B
    assert m == 2 and np.array_equal(cr, np.zeros(2))


def test_with_crit_given_the_counts_of_chunks_add():
    lv = W.reference_levels(0)
    crit = W.power(lv, G, 0.2).crit
    whole = W.power(lv, G, 0.2, crit=crit)
    a, b = W.power(lv, G, 0.2, B=15, first=0, crit=crit), W.power(lv, G, 0.2, B=25, first=15, crit=crit)
    assert np.array_equal(whole.count_reject, a.count_reject + b.count_reject) and np.array_equal(whole.count_zero, a.count_zero + b.count_zero)
    assert (whole.count_reject[0::G + 1] == 0).all() and np.isnan(whole.rep[0::G + 1]).all()          # the null levels are not run
    assert np.array_equal(whole.count_reject[1::G + 1], W.power(lv, G, 0.2).count_reject[1::G + 1])


def test_level_zero_at_the_observed_totals_is_the_presence_test_replicate_for_replicate():
    c = W.corpora()[0]
    lv = W.reference_levels(0)
    o = PR.presence(c._replace(seed=W.SEEDS[c.name]), B=24)
    tested = o.status == 0
    assert tested.any() and np.array_equal(np.ascontiguousarray(o.rep[:, tested]).view(np.uint64), np.ascontiguousarray(lv.rep[0, :24][:, tested]).view(np.uint64))
    assert np.array_equal(o.w_null, lv.obs.w_null) and np.array_equal(o.status, lv.obs.status)
    # g = 0 is w0 itself; a fraction moves weight to the target and keeps the sum within rounding
    w0 = lv.obs.w_null[np.flatnonzero(tested)[0]]
    t = int(c.targets[np.flatnonzero(tested)[0] // c.D])
    assert np.array_equal(W.level_weights(w0, t, 0.0), w0)
    w = W.level_weights(w0, t, 0.25)
    assert w[t] == 0.25 * np.cumsum(w0)[-1] and abs(w.sum() - w0.sum()) < 1e-15 and np.array_equal(W.level_weights(w0, t, 1.0) != 0, np.arange(c.C) == t)


def test_arguments_are_checked_before_a_device_is_asked_for(mmm):
    rng = np.random.default_rng(0)
    cat = rng.dirichlet(np.ones(8), size=3)
    X = [np.array([[1, 4], [3, 2]]), np.array([[2, 5]])]
    for bad in ((0.2, 0.1), (0.1, 0.1), (0.0, 0.5), (0.5, 1.5), (-0.1,), ()):
        with pytest.raises(ValueError, match="fractions"):
            mmm.presence_power(X, cat, [0], fractions=bad, seed=1)
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            mmm.presence_power(X, cat, [0], alpha=bad, seed=1)
    for bad in ([0], [100, -3], np.ones((2, 3)), np.ones((1, 2, 2)), [10.5], []):
        with pytest.raises(ValueError, match="n_mutations"):
            mmm.presence_power(X, cat, [0], n_mutations=bad, seed=1)
    with pytest.raises(ValueError, match="critical value"):
        mmm.presence_power(X, cat, [0], B=0, seed=1)
    with pytest.raises(ValueError, match="crit must be"):
        mmm.presence_power(X, cat, [0], B=0, crit=np.zeros((2, 1, 2)))
    with pytest.raises(ValueError, match="without names"):
        mmm.presence_power(X, cat, ["A"], seed=1)
    with pytest.raises(ValueError, match="need a seed"):
        mmm.presence_power(X, cat, [0])
    with pytest.raises(ValueError, match="catalogue rows"):
        mmm.presence_power(X, cat, [3], seed=1)
    with pytest.raises(ValueError, match="2\\^31"):
        mmm.presence_power(X, cat, [0], B=5, b0=2 ** 31 - 3, seed=1)
    with pytest.raises(ValueError, match="term 9"):
        mmm.presence_power([np.array([[9, 1]])], cat, [0], seed=1)
    for kind in (mmm.ILDA, mmm.IMMCTM):
        with pytest.raises(TypeError, match="factorised"):
            mmm.presence_power(X, object.__new__(kind), [0], seed=1)
    assert "presence_power" in mmm.__all__ and "PowerResult" in mmm.__all__ and "mmm_presence_power" in mmm._lib.declared_symbols()


def test_the_two_readings_of_a_power_result(mmm):
    """detectable: the smallest grid fraction reaching the power; needed_mutations: the smallest grid total; inf where none, NaN where untestable"""
    power = np.zeros((2, 3, 1, 3))
    power[0, :, 0, 0] = (0.1, 0.5, 0.9); power[1, :, 0, 0] = (0.85, 0.9, 1.0)
    power[:, :, 0, 1] = 0.3
    power[:, :, 0, 2] = np.nan
    status = np.array([[0, 1, 3]], dtype=np.int8)
    r = mmm.PowerResult(power, None, None, None, None, None, None, None, status, None, np.array([0.05, 0.1, 0.2]), np.array([[100, 100, 100], [900, 800, 700]]), 0.05,
                        10, None, None)
    d = r.detectable(0.8)
    assert d.shape == (2, 1, 3) and d[0, 0, 0] == 0.2 and d[1, 0, 0] == 0.05 and np.isinf(d[:, 0, 1]).all() and np.isnan(d[:, 0, 2]).all()
    n = r.needed_mutations(0.1)
    assert n.shape == (1, 3) and n[0, 0] == 900 and np.isinf(n[0, 1]) and np.isnan(n[0, 2])
    assert r.needed_mutations(0.2, power=0.9)[0, 0] == 100
    with pytest.raises(ValueError, match="grid"):
        r.needed_mutations(0.15)
