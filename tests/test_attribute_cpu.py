"""The restatement of mmm_attribute_mutations (tests/attribute_ref.py) against itself, and the host side of `attribute_mutations`: the
argument checks (all made before a device is asked for -- this file runs without one), the sorting of the queries into the CSR and back,
the group reduction and the moments on synthetic accumulators."""
import numpy as np
import pytest

import attribute_ref as A
import refit_ref as R


def test_posterior_rows_sum_to_one_on_explained_terms_and_to_zero_elsewhere():
    for s in A.SHAPES:
        c, r = A.case(*s), A.reference(*s)
        tot = r.post.sum(axis=1)
        doc = np.repeat(np.arange(c.D), np.diff(c.q_ptr))
        ran = r.status[doc] == 0
        explained = tot > 0
        assert (np.abs(tot[explained] - 1.0) <= c.C * 2.0 ** -52).all(), c.name
        assert not explained[~ran].any() and (r.post[~ran] == 0).all(), c.name
        if c.allowed is not None:
            assert (r.post[c.allowed[doc] == 0] == 0).all() and (r.rep_post[:, c.allowed[doc] == 0] == 0).all(), c.name
        rt = r.rep_post.sum(axis=2)
        assert (np.abs(rt[rt > 0] - 1.0) <= c.C * 2.0 ** -52).all(), c.name
        # statuses: document 1 has no queries, document 2 no mutations, document 4 (where the corpus has it) nothing allowed
        assert r.status[1] == 4 and (r.w[1] == 0).all() and r.iters[1] == 0
        if s != (3, 4096):
            assert r.status[2] == 3 and r.status[4] == 3 and r.status[0] == 0 and r.status[3] == 0


def test_the_cases_hold_every_edge_the_gpu_tests_rely_on():
    c, r = A.case(12, 96), A.reference(12, 96)
    doc = np.repeat(np.arange(c.D), np.diff(c.q_ptr))
    n = np.stack([A.dense(c, d) for d in range(c.D)])
    absent = n[doc, c.q_term] == 0
    assert absent[doc == 0].any() and (r.post[absent & (doc == 0)].sum(axis=1) > 0).all()       # a queried term the document lacks still has a posterior
    assert (c.q_mult > 1).any() and (c.q_group == -1).any() and (c.q_group >= 0).any()
    # duplicate queries: the same (document, term) twice gives the same row twice
    q0 = c.q_ptr[0]
    dup = q0 + np.flatnonzero(c.q_term[q0:c.q_ptr[1]] == c.q_term[q0])
    assert dup.size >= 2 and np.array_equal(r.post[dup[0]], r.post[dup[-1]]) and np.array_equal(r.sum_fx[dup[0]], r.sum_fx[dup[-1]])
    # duplicate CSR terms in a queried document
    assert any(np.unique(c.term[a:b]).size < b - a for a, b in zip(c.doc_ptr[:-1], c.doc_ptr[1:]))
    # the last document: its term V - 1 is produced by none of its allowed signatures -- void observed and in every replicate
    e = np.flatnonzero((doc == 5) & (c.q_term == c.V - 1))
    assert e.size and (r.post[e] == 0).all() and (r.void_count[e] == c.B).all() and (r.top_count[e] == 0).all()
    assert int(np.diff(A.case(2, 5).q_ptr).max()) > 4096


def test_a_single_active_signature_gives_exactly_one():
    c = A.case(12, 96)
    al = np.zeros_like(c.allowed); al[:, 3] = 1
    r = A.attribute(c._replace(allowed=al), B=2)
    assert set(np.unique(r.post)) <= {0.0, 1.0} and set(np.unique(r.rep_post)) <= {0.0, 1.0} and (r.post[:, 3] == 1).any()
    assert set(np.unique(r.sum_fx)) <= {0, 2 * A.FX_ONE}


def test_identical_catalogue_rows_tie_and_the_lowest_wins():
    c = A.twin()
    r = A.attribute(c)
    assert np.array_equal(r.post[:, 4], r.post[:, 5]) and np.array_equal(r.rep_post[:, :, 4], r.rep_post[:, :, 5]) and (r.post[:, 4] > 0).any()
    assert (r.top_count[:, 5] == 0).all() and (r.top_count[:, 4] > 0).any()


def test_chunks_add_and_the_fixed_point_identities_hold():
    for s in ((12, 96), (2, 5)):
        c, r = A.case(*s), A.reference(*s)
        a, b = A.attribute(c, B=2), A.attribute(c, B=c.B - 2, b0=2)
        for k in ("sum_fx", "sumsq_fx", "top_count", "void_count"):
            assert np.array_equal(getattr(a, k) + getattr(b, k), getattr(r, k)), k
        assert np.array_equal(np.concatenate([a.group_fx, b.group_fx]), r.group_fx) and np.array_equal(np.concatenate([a.rep_post, b.rep_post]), r.rep_post)
        assert np.array_equal(a.post, r.post) and np.array_equal(a.w, r.w)
        x = np.floor(r.rep_post * A.FX_ONE).astype(np.uint64)
        assert np.array_equal(x.sum(axis=0), r.sum_fx) and np.array_equal((x * x).sum(axis=0), r.sumsq_fx)
        assert np.array_equal(r.top_count.sum(axis=1) + r.void_count, np.where(np.repeat(r.status, np.diff(c.q_ptr)) == 0, c.B, 0))
        g = np.zeros((c.B, c.G, c.C), np.uint64)
        m = c.q_group >= 0
        for bb in range(c.B):
            np.add.at(g[bb], c.q_group[m], x[bb][m] * c.q_mult[m].astype(np.uint64)[:, None])
        assert np.array_equal(g, r.group_fx)


def test_the_planted_case_is_exact_and_holds_a_replicate_that_loses_a_signature():
    c = A.planted()
    r = A.attribute(c)
    assert set(np.unique(r.post)) == {0.0, 1.0} and (r.post.sum(axis=1) == 1).all()
    assert np.array_equal(r.top_count + 0, (r.post * (c.B - r.void_count)[:, None]).astype(np.int32))
    e = int(c.q_ptr[1]) + 3                                   # document 1's query on signature 1's term
    assert 0 < r.void_count[e] < c.B and r.post[e, 1] == 1 and (r.void_count[:e] == 0).all()


# ---- the Python layer, without a device --------------------------------------------------------------------------------------------------------
def test_argument_checks_come_before_any_device(mmm, monkeypatch):
    monkeypatch.setattr(mmm._lib, "default_context", lambda *a: (_ for _ in ()).throw(AssertionError("a device was asked for")))
    c = A.case(12, 96)
    X = A.as_X(c)
    f = mmm.attribute_mutations
    ok = dict(allowed=c.allowed, B=3, seed=1)
    for kw, err in ((dict(ok, seed=None), "seed"), (dict(ok, B=70000), "65535"), (dict(ok, B=-1), "B"), (dict(ok, B=5000, quantiles=True), "4096"),
                    (dict(ok, B=0, quantiles=True), "B > 0"), (dict(ok, q=(0.5, 1.5)), "q must"), (dict(ok, maxiter=0), "maxiter"), (dict(ok, tol=-1.0), "tol"),
                    (dict(ok, queries=[(0, 0)]), "1-based"), (dict(ok, queries=[(0, c.V + 1)]), "1-based"), (dict(ok, queries=[(c.D, 1)]), "sample"),
                    (dict(ok, queries=[(0, 1, 0)]), "mult"), (dict(ok, queries=[(0, 1, 2, 3)]), "query 0"), (dict(ok, queries=[(0, 1.5)]), "query 0"),
                    (dict(ok, queries=[(0, 1)], groups=["a", "b"]), "one label per query"), (dict(ok, allowed=np.ones((2, 3))), "allowed"),
                    (dict(ok, queries=[(0, 1, 2 ** 30), (1, 1, 2 ** 30)], groups=["g", "g"]), "mults of a group")):
        with pytest.raises(ValueError, match=err):
            f(X, c.cat, **kw)
    with pytest.raises(ValueError, match="limit 256"):
        f(X, np.ones((257, c.V)), **ok)
    with pytest.raises(ValueError, match="limit 4096"):
        f([np.asarray([[1, 1]])], np.ones((2, 4097)), **ok)
    with pytest.raises(ValueError, match="limit 4096"):
        f([np.stack([np.arange(4097) % 4096 + 1, np.ones(4097, np.int64)], axis=1)], np.ones((2, 4096)), allowed=np.ones(2), B=0)
    with pytest.raises(TypeError):
        f(X, object.__new__(mmm.ILDA), **ok)
    with pytest.raises(AssertionError, match="a device was asked for"):       # with every check passed the device is next
        f(X, c.cat, **ok)


def test_queries_are_sorted_into_the_csr_and_results_come_back_in_the_callers_order(mmm):
    at = mmm.attribute
    rng = np.random.default_rng(5)
    D, V = 7, 30
    qs = at._queries([(int(d), int(v), int(m)) for d, v, m in zip(rng.integers(0, D, 40), rng.integers(1, V + 1, 40), rng.integers(1, 5, 40))], None, None, None, D, V)
    qs[:, 0][qs[:, 0] == 3] = 4                                # sample 3 stays without queries
    order, q_ptr = at._sort_queries(qs, D)
    s = qs[order]
    assert q_ptr[0] == 0 and q_ptr[-1] == 40 and q_ptr[4] == q_ptr[3] and (np.diff(q_ptr) >= 0).all()
    for d in range(D):
        assert (s[q_ptr[d]:q_ptr[d + 1], 0] == d).all()
    assert all(np.array_equal(s[q_ptr[d]:q_ptr[d + 1]], qs[qs[:, 0] == d]) for d in range(D))     # stable: the caller's order within a sample
    inv = np.empty(40, np.int64); inv[order] = np.arange(40)
    assert np.array_equal(s[inv], qs)
    # queries=None: every non-zero entry with its count, already in CSR order
    c = A.case(12, 96)
    every = at._queries(None, c.doc_ptr, c.term, c.count, c.D, c.V)
    nz = c.count > 0
    assert np.array_equal(every[:, 1], c.term[nz]) and np.array_equal(every[:, 2], c.count[nz]) and (np.diff(every[:, 0]) >= 0).all()
    assert np.array_equal(np.bincount(every[:, 0], minlength=c.D), [int(nz[a:b].sum()) for a, b in zip(c.doc_ptr[:-1], c.doc_ptr[1:])])
    labels, gid = at._group_ids(["TP53", None, "KRAS", "TP53"], 4)
    assert labels == ["TP53", "KRAS"] and gid.tolist() == [0, -1, 1, 0] and at._group_ids(None, 4) == ([], None)


def test_group_reduction_and_moments_on_synthetic_accumulators(mmm):
    at = mmm.attribute
    one = at.FX_ONE
    post = np.asarray([[0.75, 0.25, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    mult = np.asarray([2, 1, 5, 3]); gid = np.asarray([0, 0, 1, -1], np.int32)
    g = at._group_observed(post, mult, gid, 2)
    assert g.dtype == np.uint64 and g.tolist() == [[2 * 3 * one // 4 + one // 2, 2 * one // 4 + one // 2, 0], [0, 0, 0]]
    sh = at._shares(g)
    assert np.allclose(sh[0], [2.0 / 3, 1.0 / 3, 0]) and np.isnan(sh[1]).all()
    gfx = np.zeros((4, 2, 3), np.uint64)
    gfx[:, 0, 0] = [one, 3 * one, one, 3 * one]; gfx[:, 0, 1] = [3 * one, one, 3 * one, one]
    gfx[2:, 1, 2] = 7
    mean, quant = at._group_summary(gfx, (0.0, 0.5, 1.0))
    assert np.array_equal(mean[0], [0.5, 0.5, 0.0]) and np.array_equal(quant[:, 0, 0], [0.25, 0.5, 0.75])
    assert np.array_equal(mean[1], [0, 0, 1.0]) and np.array_equal(quant[:, 1, 2], [1, 1, 1])      # the replicates without mass are left out
    # moments from the fixed-point sums: exact for equal replicates, the textbook value otherwise, NaN without replicates
    x = np.asarray([[one // 2] * 4, [one // 4, one // 2, 3 * one // 4, one // 2], [0, 0, 0, 0]], dtype=np.uint64).T     # [B = 4, Q = 3]
    s, ss = x.sum(axis=0)[:, None], (x * x).sum(axis=0)[:, None]
    mean, sd = at._moments(s, ss, np.asarray([4, 4, 0]))
    assert mean[0, 0] == 0.5 and sd[0, 0] == 0.0 and mean[1, 0] == 0.5 and np.isnan(mean[2, 0]) and np.isnan(sd[2, 0])
    assert abs(sd[1, 0] - np.std([0.25, 0.5, 0.75, 0.5], ddof=1)) < 1e-15
    big = np.full((1, 1), 65535 * one, np.uint64)              # the largest sums a caller can reach: still exact
    assert at._moments(big, np.full((1, 1), 65535 * one * one, np.uint64), np.asarray([65535]))[1][0, 0] == 0.0
