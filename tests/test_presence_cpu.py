"""What the presence test's GPU suite rests on, checked on the numpy restatement alone (tests/presence_ref.py), and the argument checks of
`signature_presence` that need no device."""
import numpy as np
import pytest

import presence_ref as PR


@pytest.mark.parametrize("i", range(len(PR.SHAPES) + 1), ids=lambda i: PR.corpora()[i].name)
def test_no_decision_of_the_gpu_corpora_is_near_a_tie(i):
    """status, count_zero and count_ge pass through a clamp at 0 and a comparison of values that hold a device log; two implementations agree
    on them as integers where no such value is near its threshold.  For every corpus of tests/test_presence_gpu.py:
    every Λ_obs is exactly 0 (by the score rule), +inf, or its raw 2 (ll1 - ll0) is >= 1e-6 in absolute value (so is every replicate's: the
    clamp decides count_zero); every |Λ_b - Λ_obs| of a tested item is >= 1e-6 max(1, Λ_obs).  The rounding bounds are below 3e-8.
    Smallest margins found (seeds of presence_ref): |raw| 2.5e-4 (edge), 2.4e-3 (C12V96), 3.0e-3 (C8V200), 3.5e-3 (C6V1536), 3.6e-3 (C40V96),
    8.0e-3 (C4V5); relative gap to Λ_obs 2.1e-3 (edge), 1.7e-2 (C12V96), 2.3e-2 (C6V1536), 3.2e-2 (C40V96), 0.92 (C4V5), 1.0 (C8V200)."""
    c = PR.corpora()[i]
    o = PR.reference(c)
    tested = o.status == 0
    assert tested.any() and set(np.unique(o.status)) <= {0, 1, 2, 3}
    raw = np.concatenate([o.obs_raw[np.isfinite(o.obs_raw)], o.rep_raw[np.isfinite(o.rep_raw)]])
    print("%s: smallest |raw| %.3g over %d fits of A1" % (c.name, np.abs(raw).min(), raw.size))
    assert (np.abs(raw) >= 1e-6).all()
    for j in range(o.status.size):
        assert o.stat[j] == 0 or np.isinf(o.stat[j]) or o.stat[j] >= 1e-6, (j, o.stat[j])
    gap = np.abs(o.rep[:, tested] - o.stat[tested][None, :]) / np.maximum(1.0, o.stat[tested])[None, :]
    print("%s: smallest |Λ_b - Λ_obs| / max(1, Λ_obs) %.3g; largest rounding bound %.3g" % (c.name, gap.min(), np.nanmax(o.rep_bound)))
    assert (gap >= 1e-6).all()
    assert max(np.nanmax(o.rep_bound), o.bound.max()) < 1e-7
    # a replicate is drawn from a null fit that produces every term it can land on: u0 = 0, so fit(A1) runs exactly where s > 1
    assert np.array_equal(o.rep_alt[:, tested], o.rep_s[:, tested] > 1)


def test_skipping_the_alternative_fit_where_the_score_is_at_most_one_is_sound():
    """On every replicate with s <= 1 the definition sets Λ = 0 without fitting A1.  Fitting it anyway (maxiter 5000, tol 1e-9, 8 samples
    without the target, 20 replicates each) gives |2 (ll1 - ll0)| <= 9.3e-6 on the 52 skipped replicates of 100 -- all of them NEGATIVE: the
    larger fit stops a little short of the null optimum it is heading for -- asserted below 1e-4, a margin of 10 x; and a target weight of at
    most 5.0e-6, below the smallest weight any s > 1 replicate gives (2.9e-5)."""
    c, _ = PR.planted_corpus(seed=11, n_with=0, n_without=8)
    o = PR.presence(c._replace(maxiter=5000, B=20, name="kkt"), always_alt=True)
    tested = o.status == 0
    skipped = ~o.rep_alt[:, tested]
    raw, w1t = o.rep_raw[:, tested], o.rep_w1t[:, tested]
    assert 20 <= skipped.sum() <= skipped.size - 20
    print("skipped %d of %d; 2 (ll1 - ll0) there in [%.3g, %.3g]; target weight there <= %.3g, elsewhere >= %.3g"
          % (skipped.sum(), skipped.size, raw[skipped].min(), raw[skipped].max(), w1t[skipped].max(), w1t[~skipped].min()))
    assert np.abs(raw[skipped]).max() < 1e-4
    assert w1t[skipped].max() < w1t[~skipped][w1t[~skipped] > 0].min()


def test_planted_signature_is_found_and_absent_one_is_not():
    """w_t = 0.1 at N = 2000: no replicate of the null fit reaches Λ_obs, p = 1 / (B + 1).  Without the target the p-values are those of a
    conservative test: about half of the samples have Λ_obs = 0 exactly, a point mass at p = 1, and the rest are spread over (0, 1]."""
    c, has = PR.planted_corpus()
    o = PR.presence(c)
    p = (1.0 + o.count_ge) / (c.B + 1.0)
    assert (~has).sum() >= 40
    assert (p[has] == 1.0 / (c.B + 1)).all(), p[has]
    print("mean p without the target %.3f; share with Λ_obs = 0: %.2f" % (p[~has].mean(), (o.status[~has] == 1).mean()))
    assert 0.35 <= p[~has].mean() <= 0.8
    assert (o.status[has] == 0).all() and (o.score[has] > 1).all()


def test_arguments_are_checked_before_a_device_is_asked_for(mmm):
    rng = np.random.default_rng(0)
    cat = rng.dirichlet(np.ones(8), size=3)
    X = [np.array([[1, 4], [3, 2]]), np.array([[2, 5]])]
    named = (["A", "B", "C"], ["t%d" % i for i in range(8)], cat)
    with pytest.raises(ValueError, match="catalogue rows"):
        mmm.signature_presence(X, cat, [3], seed=1)
    with pytest.raises(ValueError, match="catalogue rows"):
        mmm.signature_presence(X, cat, [-1], seed=1)
    with pytest.raises(ValueError, match="empty"):
        mmm.signature_presence(X, cat, [], seed=1)
    with pytest.raises(ValueError, match="without names"):
        mmm.signature_presence(X, cat, ["A"], seed=1)
    with pytest.raises(ValueError, match="lacks"):
        mmm.signature_presence(X, named, ["D"], seed=1)
    with pytest.raises(ValueError, match="need a seed"):
        mmm.signature_presence(X, cat, [0])
    with pytest.raises(ValueError, match="2\\^31"):
        mmm.signature_presence(X, cat, [0], B=5, b0=2 ** 31 - 3, seed=1)
    with pytest.raises(ValueError, match="term 9"):
        mmm.signature_presence([np.array([[9, 1]])], cat, [0], seed=1)
    with pytest.raises(ValueError, match="limit 4096"):
        mmm.signature_presence(X, np.ones((2, 4097)), [0], seed=1)
    for kind in (mmm.ILDA, mmm.IMMCTM):
        with pytest.raises(TypeError, match="factorised"):
            mmm.signature_presence(X, object.__new__(kind), [0], seed=1)
    assert "signature_presence" in mmm.__all__ and "mmm_presence_test" in mmm._lib.declared_symbols()
    r = mmm.PresenceResult(np.array([[0.01, np.nan, 0.5]]), *[None] * 8, 99, None, None)
    assert r.significant(0.05).tolist() == [[True, False, False]]
