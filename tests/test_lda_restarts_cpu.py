"""Host logic of restarts.fit_lda_restarts (no GPU needed): restarts dealt over ranks, the merge, the tie and NaN rules."""
import numpy as np
import pytest

import mmm_pkg

mmm_pkg.load()
from multimodalmusig_jl_amd import restarts as rs  # noqa: E402


def _fake_single(X, K, α, η, seeds, **kw):
    """Stand-in for one rank's batched fit: final ll of seed s = -|s - 6| (NaN for s = 0); the winner is the first maximum."""
    seeds = list(seeds)
    ll = np.array([np.nan if s == 0 else -abs(s - 6.0) for s in seeds])
    i = rs._best(ll)
    return i, np.full((3, K), float(seeds[i])), np.full((K, 2), float(seeds[i])), ll


def _stubbed(monkeypatch):
    real = rs.fit_lda_restarts

    def dispatch(X, K, α, η, seeds, rank=0, nranks=1, allgather=None, **kw):
        if nranks == 1:
            return _fake_single(X, K, α, η, seeds, **kw)
        return real(X, K, α, η, seeds, rank=rank, nranks=nranks, allgather=allgather, **kw)

    monkeypatch.setattr(rs, "fit_lda_restarts", dispatch)
    return real


@pytest.mark.parametrize("nranks", [2, 3])
def test_lda_restarts_dealt_over_ranks_merge(monkeypatch, nranks):
    real = _stubbed(monkeypatch)
    seeds = [3, 9, 0, 7, 5, 8, 5]          # ll -3, -3, NaN, -1, -1, -2, -1: the maximum -1 first at index 3 (seed 7)
    K = 2
    parts = [_fake_single(None, K, None, None, seeds[r::nranks]) for r in range(nranks)]
    dealt = []
    for rank in range(nranks):
        win, lam, gam, ll = real(None, K, 0.1, 0.1, seeds, rank=rank, nranks=nranks, allgather=lambda obj: (dealt.append(obj), parts)[1])
        assert win == 3 and lam[0, 0] == 7.0 and gam[0, 0] == 7.0       # the winner's own rank returned its λ and γ
        np.testing.assert_array_equal(ll, [-3.0, -3.0, np.nan, -1.0, -1.0, -2.0, -1.0])
    for rank, obj in enumerate(dealt):                                    # each rank fitted seeds[rank::nranks]
        np.testing.assert_array_equal(obj[3], parts[rank][3])


def test_lda_restarts_rank_without_seeds(monkeypatch):
    """More ranks than seeds: a rank with nothing to fit still takes part in the allgather."""
    real = _stubbed(monkeypatch)
    seeds = [4, 6]
    parts = [_fake_single(None, 2, None, None, seeds[r::3]) if seeds[r::3] else (None, None, None, np.zeros(0)) for r in range(3)]
    win, lam, _, ll = real(None, 2, 0.1, 0.1, seeds, rank=2, nranks=3, allgather=lambda obj: parts)
    assert win == 1 and lam[0, 0] == 6.0 and ll.tolist() == [-2.0, 0.0]


def test_best_rule_ties_and_nan():
    assert rs._best([-2.0, -1.0, -1.0]) == 1
    assert rs._best([np.nan, -5.0]) == 1
    assert rs._best([-1.0, np.nan, -1.0]) == 0


def test_lda_restarts_needs_allgather():
    with pytest.raises(ValueError, match="allgather"):
        rs.fit_lda_restarts(None, 2, 0.1, 0.1, [1, 2], rank=0, nranks=2)
