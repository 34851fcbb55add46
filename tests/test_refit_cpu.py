"""The definition of mmm_refit_exposures as its numpy restatement computes it (tests/refit_ref.py): the properties that make it a refit
-- EM never lowers the log-likelihood, planted signatures are found again -- and the condition under which its integer outputs can be
compared with another implementation's: every decision of every document of every corpus the GPU tests use is far from a tie."""
import numpy as np
import pytest

import refit_ref as R


def test_ll_is_non_decreasing_along_an_em_run():
    for C, V in ((12, 96), (65, 96)):
        c = R.corpus(C, V)
        P = R.normalise(c.cat)
        for d in range(3):
            n = np.zeros(V)
            np.add.at(n, c.term[c.doc_ptr[d]:c.doc_ptr[d + 1]], c.count[c.doc_ptr[d]:c.doc_ptr[d + 1]].astype(np.float64))
            A = np.flatnonzero(c.allowed[d])
            trace = []
            R.fit(P[A], n, n / n.sum(), 60, 0.0, trace=trace)
            ll = np.asarray(trace)
            assert len(ll) == 60 and ll[-1] > ll[0]
            assert (np.diff(ll) >= -1e-12 * np.abs(ll[:-1])).all(), np.diff(ll).min()      # up to the rounding of the sum itself


def test_a_one_element_set_gives_weight_one():
    c = R.corpus(12, 96)
    P = R.normalise(c.cat)
    n = np.zeros(96); n[[3, 40, 77]] = [5, 1, 9]
    for a in (0, 7):
        w, ll, u, it, q = R.fit(P[[a]], n, n / n.sum(), 25, 0.0)
        assert w.shape == (1,) and w[0] == 1.0 and it == 25 and u == 0
        assert np.array_equal(q, P[a])
    r = R.refit(1, 12, 96, np.asarray([0, 3]), np.asarray([3, 40, 77], np.int32), np.asarray([5, 1, 9], np.int32), c.cat,
                allowed=np.eye(12, dtype=np.uint8)[[2]], penalty=np.asarray([1.0]), maxiter=25, tol=0.0)
    assert r.w[0, 2] == 1.0 and r.active[0].sum() == 1 and (r.order == -1).all() and r.iters[0] == 25


@pytest.mark.parametrize("C,V,N,k", [(12, 96, 3000, 3), (20, 96, 20000, 4)])
def test_planted_active_sets_are_recovered(C, V, N, k):
    for seed in range(3):
        cat, dp, term, count, which = R.planted(C, V, N, k, seed)
        r = R.refit(1, C, V, dp, term, count, cat, penalty=np.asarray([0.5 * np.log(N)]), maxiter=1000, tol=1e-9)
        assert np.array_equal(np.flatnonzero(r.active[0]), which), (seed, np.flatnonzero(r.active[0]), which)
        assert abs(r.w[0].sum() - 1) < 1e-12 and (r.w[0][r.active[0] == 0] == 0).all()
        assert (r.order[0][:C - k] >= 0).all() and (r.order[0][C - k:] == -1).all()


def test_every_decision_of_every_gpu_corpus_is_far_from_a_tie():
    """the condition under which active / order / iters of two implementations are comparable: the two smallest weights differ by at least
    1e-6 relative at every removal, and no Δ lies within 1e-6 (relative) of its penalty.  No document is left out."""
    seen_exact_tie = False
    for c, tol in R.cases():
        r = R.reference(c, tol)
        for d in range(c.D):
            assert len(r.gap_margin[d]) == len(r.pen_margin[d]) == len(r.rounds[d])
            for j, (g, p) in enumerate(zip(r.gap_margin[d], r.pen_margin[d])):
                assert g >= 1e-6 and p >= 1e-6, (c.name, tol, d, j, g, p)
                seen_exact_tie |= c.name == "twin" and np.isinf(g)
        # every corpus holds the edge documents: an empty document, an empty `allowed` row, a one-signature row; where the shape allows, unexplained > 0
        N = np.add.reduceat(np.concatenate([c.count, [0]]), c.doc_ptr[:-1]) * (np.diff(c.doc_ptr) > 0)
        assert (N == 0).any() and (N == 1).any() and (c.allowed.sum(1) == 0).any() and (c.allowed.sum(1) == 1).any()
        assert (np.diff(c.doc_ptr) > np.asarray([np.unique(c.term[a:b]).size for a, b in zip(c.doc_ptr[:-1], c.doc_ptr[1:])])).any()      # duplicates
        assert (c.count == 0).any()
        if c.C >= 2:
            assert (r.unexplained[N > 0][c.allowed[N > 0].sum(1) > 0] > 0).any()
    assert seen_exact_tie      # the twin rows did meet as the two smallest weights: that tie is exact and goes to the lower index
