"""The definition of mmm_extract_signatures as its numpy restatement computes it (tests/extract_ref.py): it is the Lee-Seung update with
fixed rows, EM never lowers the log-likelihood, a planted row is found again, its two stated consequences hold bit for bit, and the stopping
decisions of every case the GPU tests use are far from a tie."""
import numpy as np

import extract_ref as E
import refit_ref as R


def _lee_seung(n, H, F, E0, iters):
    """KL-NMF n ~ E H by multiplicative updates in np.longdouble with naive sums; rows < F of H are held, the others renormalised"""
    ld = np.longdouble
    n, H, Ex = n.astype(ld), H.astype(ld), E0.astype(ld)
    for _ in range(iters):
        M = Ex @ H
        ratio = np.where(M > 0, n / np.where(M > 0, M, 1), 0)
        En = Ex * (ratio @ H.T) / H.sum(axis=1)[None, :]
        Hn = H * (Ex.T @ ratio) / Ex.sum(axis=0)[:, None]
        Hn[:F] = H[:F]
        Hn[F:] = Hn[F:] / Hn[F:].sum(axis=1)[:, None]
        Ex, H = En, Hn
    return Ex / Ex.sum(axis=1)[:, None], H


def test_the_restatement_is_the_lee_seung_update_with_fixed_rows():
    """50 iterations from the same state on three small cases, against the textbook form in longdouble, which shares no code with the
    restatement.  Largest relative difference of an entry of Q or W, measured: 2.32e-14 (F3J1V96D17), 6.15e-14 (F3J2V97D33), 2.49e-14
    (F0J4V130D16), over the entries that are not exactly 0 in both; asserted at 100 x the measured value of each case (rounding accumulates
    differently per case, and two orders of magnitude still sit far below any modelling error)."""
    measured = {"F3J1V96D17": 2.32e-14, "F3J2V97D33": 6.15e-14, "F0J4V130D16": 2.49e-14}
    for c in E.cases():
        if c.name not in measured:
            continue
        ref = E.extract(c.D, c.F, c.J, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, 1, 0, c.seed, 0, None, 50, 0.0)
        n = E.dense(c.D, c.V, c.doc_ptr, c.term, c.count)
        N = n.sum(axis=1)
        A = np.ones((c.D, c.F + c.J))
        if c.F:
            A[:, :c.F] = c.allowed
        live = N > 0
        H0 = np.concatenate([R.normalise(c.cat) if c.F else np.zeros((0, c.V)), E.start_rows(c.J, c.V, 0, c.seed, 0)])
        E0 = (N[:, None] * A / A.sum(axis=1)[:, None])[live]
        W, H = _lee_seung(n[live], H0, c.F, E0, 50)
        pos = ref.w[0][live] > 0
        dw = np.abs(W[pos] - ref.w[0][live][pos]) / ref.w[0][live][pos]
        dq = np.abs(H[c.F:] - ref.sig[0]) / ref.sig[0]
        worst = float(max(dw.max(), dq.max()))
        print("%s: largest relative difference %.3g" % (c.name, worst))
        assert (W[~pos] == 0).all()
        assert worst <= 100 * measured[c.name], (c.name, worst)


def test_ll_is_non_decreasing_along_a_run():
    """the ll of the normalised iterate never drops by more than the a-priori rounding bound of its own evaluation, summed over documents"""
    for name in ("F3J1V96D17", "F3J2V97D33", "F0J4V130D16"):
        c = next(x for x in E.cases() if x.name == name)
        n = E.dense(c.D, c.V, c.doc_ptr, c.term, c.count)
        trace = []

        def on_iter(r, it, w, P):
            S = np.cumsum(w, axis=1)[:, -1]
            q = E.mixtures(np.where(S[:, None] > 0, w / np.where(S > 0, S, 1)[:, None], w), P)
            ll = bound = 0.0
            for d in range(c.D):
                a, b = R.ll_longdouble(n[d], q[d])
                ll += float(a); bound += b
            trace.append((ll, bound))
        E.extract(c.D, c.F, c.J, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, 1, 0, c.seed, 0, None, 60, 0.0, on_iter=on_iter)
        ll = np.asarray([t[0] for t in trace]); bound = np.asarray([t[1] for t in trace])
        assert len(ll) == 60 and ll[-1] > ll[0]
        assert (np.diff(ll) >= -(bound[1:] + bound[:-1])).all(), (name, np.diff(ll).min())


def test_a_planted_row_is_recovered():
    """D = 40, V = 96, three catalogue rows and one hidden row (Dirichlet(0.3)), exposures Dirichlet(0.5), N_d in [200, 3000), J = 1, 4
    restarts, 500 iterations, tol = 0: the best restart's new row has cosine >= 0.99 to the hidden row.  The restatement's own value:
    0.99815 to 0.99816 on the four restarts."""
    (dp, term, count), cat, hidden = E.planted()
    r = E.extract(40, 3, 1, 96, dp, term, count, cat, None, 4, 0, 2026, 0, None, 500, 0.0)
    cos = [float(q[0] @ hidden / np.sqrt((q[0] @ q[0]) * (hidden @ hidden))) for q in r.sig]
    print("cosines of the four restarts:", cos)
    assert (r.iters == 500).all() and cos[int(np.argmax(r.ll))] >= 0.99


def test_without_free_rows_it_is_the_refit_bit_for_bit():
    for c in E.cases():
        if c.F == 0 or c.D > 100:
            continue
        got = E.extract(c.D, c.F, 0, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, 1, 0, 0, 0, None, 25, 0.0)
        want = R.refit(c.D, c.F, c.V, c.doc_ptr, c.term, c.count, c.cat, c.allowed, None, 25, 0.0)
        for a, b in ((got.w[0], want.w), (got.ll_doc[0], want.ll_doc), (got.unexplained[0], want.unexplained), (got.q[0], want.q)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), c.name
        assert got.iters[0] == 25 and (want.iters[(want.w > 0).any(axis=1)] == 25).all()


def test_a_call_is_a_slice_of_the_call_from_zero():
    for name, r0, Rn in (("F3J1V96D17", 2, 1), ("F1J1V5D3", 1, 2), ("init", 2, 1)):
        c = next(x for x in E.cases() if x.name == name)
        whole, part = E.reference(c), E.reference(c, r0, Rn)
        for k in ("sig", "w", "ll", "ll_doc", "unexplained", "iters"):
            assert np.array_equal(getattr(part, k).view(np.uint8), getattr(whole, k)[r0:r0 + Rn].view(np.uint8)), (name, k)
    a, b = E.start_rows(2, 97, 5, 77, 0), E.start_rows(2, 97, 5, 77, 1)
    assert not np.array_equal(a, b) and np.allclose(a.sum(axis=1), 1.0, atol=1e-14)


def test_every_stopping_decision_of_every_gpu_case_is_far_from_a_tie():
    """every md of every iteration of a case with tol > 0 is further than 1e-6 tol from tol; the table holds the degenerate inputs"""
    stopped_early = False
    for c in E.cases():
        r = E.reference(c)
        assert np.isfinite(r.sig).all() and np.isfinite(r.w).all()
        if c.tol > 0:
            for mds, it in zip(r.md, r.iters):
                assert all(abs(m - c.tol) > 1e-6 * c.tol for m in mds), c.name
                stopped_early |= it < c.maxiter
    assert stopped_early
    every = E.cases()
    N = lambda c: E.dense(c.D, c.V, c.doc_ptr, c.term, c.count).sum(axis=1)
    assert any((N(c) == 0).any() for c in every)
    assert any((np.diff(c.doc_ptr) > np.asarray([np.unique(c.term[a:b]).size for a, b in zip(c.doc_ptr[:-1], c.doc_ptr[1:])])).any() for c in every)
    assert any(c.allowed is not None and (c.allowed.sum(axis=1) == 0).any() for c in every)
    assert any(c.J == 0 and (E.reference(c).unexplained[0][N(c) > 0] > 0).any() for c in every)
    assert any(c.init is not None for c in every) and {1, 3} <= {c.R for c in every} and any(c.R == 300 for c in every)
