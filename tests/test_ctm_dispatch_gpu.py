"""The size-dependent choices of CTM create (csrc/ctm.hip create_impl), walked from both sides of every threshold.

create_impl picks, from the corpus size, the lane layout of the solve phase (sum K = 10: 8 lanes x 2 coordinates below 75,000 documents on
a 256-CU device, 2 x 5 from there; sum K = 28: 32 x 1 below 9,000, 16 x 2 from there) and the number of persistent waves per SIMD (sum K =
28 as 16 x 2: three below 40,000, four from there).  `mmm_tuning_opts.geometry_cus` scales the thresholds by cus / 256: at a pretended 4-CU
geometry they sit at 1,171.875, 140.625 and 625 documents, so corpora of a few hundred documents reach both sides.

The two sum K = 10 layouts associate a document's sums differently (test_twin_cpu.py::test_solve_layouts_sum_k_10_differ_sum_k_28_do_not
shows it on the order-matched oracle at these very shapes), so that choice must not depend on the number of restarts R: replica r of a
batch is, bit for bit, the single fit of its gamma0 (tests/test_ctm_batch_gpu.py).  The sum K = 28 choices count D * R
and change no bit; here two device handles that took different branches are put next to each other, and each against the oracle."""
import numpy as np
import pytest

import np_ref
from test_ctm_batch_gpu import FIELDS, _inits, _make
from test_ctm_gpu import SNV3, _fit_case, _same_bits, _same_state

pytestmark = pytest.mark.gpu

CUS = 4
R = 4
BIT_KEYS = ("L", "grid_e", "waves_e", "grid_m", "wide", "tdense", "Ls", "cpl")      # (solve_waves only deals the documents out to the waves)


def walk_case(case, D=None):
    """K, V, features, corpus and the R stacked gamma0 of a case of the walk (tests/test_twin_cpu.py runs the oracle on the same ones)."""
    if case == "imm10":         # the IMMCTM of test_ctm_batch_gpu.py's imm10 case
        c = dict(D=320, K=[10], V=[96], means=[1500], feats=SNV3)
    elif case == "mm55":        # sum K = 10 in two modalities: the switch keys on sum K
        c = dict(D=320, K=[5, 5], V=[96, 38], means=[1500, 150], feats=None)
    else:                       # cfg4_shape on either side of its two thresholds
        k = _fit_case("cfg4_shape")
        c = dict(D={"cfg4_lanes": 40, "cfg4_waves": 200}[case], K=k["K"], V=k["V"], means=k["means"], feats=None)
    if D is not None:
        c["D"] = D
    c["X"], _ = np_ref.synth_mm(c["D"], c["V"], c["K"], seed=12, means=c["means"], empty_frac=0.1)
    c["g0"] = _inits(c["K"], c["V"], R, 99, c["feats"])
    return c


# what a SINGLE handle on the case's corpus reports at geometry_cus = 4 (asserted on the device below; the CPU test builds its oracles from it)
GEO4 = {"imm10": dict(L=16, grid_e=4, waves_e=8, grid_m=10, wide=0, tdense=1, Ls=8, cpl=2),
        "mm55": dict(L=16, grid_e=4, waves_e=8, grid_m=10, wide=0, tdense=1, Ls=8, cpl=2),
        "cfg4_lanes": dict(L=32, grid_e=3, waves_e=8, grid_m=2, wide=0, tdense=0, Ls=32, cpl=1),
        "cfg4_waves": dict(L=32, grid_e=4, waves_e=8, grid_m=7, wide=0, tdense=1, Ls=16, cpl=2)}


def _bits(geo, keys=BIT_KEYS):
    return {k: geo[k] for k in keys}


def _flat(g0r):
    return g0r if isinstance(g0r, np.ndarray) else np.concatenate([x.ravel() for x in g0r])


def batch_equals_singles(mmm, c, g0=None, maxiter=30, tol=2e-3, keys=BIT_KEYS):
    """test_batched_fit_is_bitwise_the_single_model_fit for every replica, plus the last pass' per-document evaluation counts and the
    handles' geometry on `keys`.  -> (geometry of the batch, geometry of the singles, passes per replica)"""
    K, V, X, feats = c["K"], c["V"], c["X"], c["feats"]
    g0 = c["g0"] if g0 is None else g0
    n = len(g0)
    batch = _make(mmm, K, V, X, g0, feats, restarts=n)
    assert batch.R == n
    gb = batch.geometry()
    hists = mmm.fit_restarts(batch, maxiter=maxiter, tol=tol)
    iters, gs = [], None
    for r in range(n):
        single = _make(mmm, K, V, X, g0[r], feats)
        assert gs is None or single.geometry() == gs
        gs = single.geometry()
        h = mmm.fit(single, maxiter=maxiter, tol=tol, verbose=False)
        iters.append(len(h))
        assert len(h) == len(hists[r]) == batch.restart_iters[r], "restart %d stops at another pass" % r
        assert np.array_equal(h, hists[r]), "restart %d: ll history differs from the single-model fit (batch %s, single %s)" % (r, gb, gs)
        assert single.converged == bool(batch.restart_converged[r])
        assert single.elbo == batch.restart_elbo[r]
        batch.select(r)
        for f in FIELDS:
            _same_bits(batch._get(f), single._get(f), "restart %d field %s (batch %s, single %s)" % (r, f, gb, gs))
        sb, ss = batch.solver_stats(per_doc=True), single.solver_stats(per_doc=True)
        assert np.array_equal(sb["per_doc_nu"], ss["per_doc_nu"]) and np.array_equal(sb["per_doc_lambda"], ss["per_doc_lambda"]), "restart %d" % r
        assert sb["n_capped"] == ss["n_capped"] == 0
        single.close()
    batch.close()
    assert _bits(gb, keys) == _bits(gs, keys), "a batch of %d and its single handle took different geometries" % n
    # the replicas stop at different passes, so "a stopped replica is left untouched" is part of what was compared
    assert len(set(iters)) > 1, "choose gamma0 with which the restarts stop at different passes (got %s)" % iters
    return gb, gs, iters


# ------------------------------------------------------------------------------------------ a. sum K = 10 across the threshold
@pytest.mark.parametrize("case", ["imm10", "mm55"])
def test_sum_k_10_batch_takes_the_layout_of_its_single(mmm, tuning, case):
    """D = 320 < 1,171.875 <= D * R = 1,280.  The layout follows D alone: batch and singles both run 8 x 2 and agree in every bit.  (Chosen
    from D * R, the batch ran 2 x 5 against the singles' 8 x 2 and every lambda differed.)"""
    tuning(geometry_cus=CUS)
    c = walk_case(case)
    assert c["D"] < 75000 * CUS / 256 <= c["D"] * R
    gb, gs, iters = batch_equals_singles(mmm, c)
    assert _bits(gs) == GEO4[case] and (gb["Ls"], gb["cpl"]) == (8, 2), (gb, gs)
    # ... for any R
    for n in (2, 16):
        b = _make(mmm, c["K"], c["V"], c["X"], _inits(c["K"], c["V"], n, 7, c["feats"]), c["feats"], restarts=n)
        assert _bits(b.geometry()) == GEO4[case], (n, b.geometry())
        b.close()


# ------------------------------------------------------------------------------------------ b. sum K = 10, each layout pinned
@pytest.mark.parametrize("lanes,expect", [(2, (2, 5)), (8, (8, 2)), (16, (10, 1))])
def test_sum_k_10_pinned_layouts_batch_against_singles(mmm, tuning, lanes, expect):
    """solve_lanes pins the layout for batch and singles alike: 2 x 5 and the lock-step build (packed groups of 10 lanes) with replicas on
    grid.y, and 8 x 2 for completeness."""
    tuning(geometry_cus=CUS, solve_lanes=lanes)
    gb, gs, _ = batch_equals_singles(mmm, walk_case("imm10", D=150))
    assert (gb["Ls"], gb["cpl"]) == (gs["Ls"], gs["cpl"]) == expect


def test_sum_k_10_two_by_five_refill_and_document_order_under_a_batch(mmm, tuning):
    """2 x 5 with a wave's range longer than its 32 slots (and at most 64: the case order_range applies to), replicas on grid.y: slot refill
    and the longest-solve-first order of test_solve_phase_document_order_keeps_every_bit under a batch of two."""
    tuning(geometry_cus=CUS, solve_lanes=2)
    c = walk_case("imm10", D=1500)
    gb, gs, _ = batch_equals_singles(mmm, c, g0=c["g0"][:2])
    for geo in (gb, gs):
        assert (geo["Ls"], geo["cpl"]) == (2, 5)
        assert geo["solve_waves"] > 0 and 64 // geo["Ls"] < c["D"] // geo["solve_waves"] and -(-c["D"] // geo["solve_waves"]) <= 64, geo


# ------------------------------------------------------------------------------------------ c., d. sum K = 28 across its two thresholds
def test_sum_k_28_lane_layouts_are_bit_neutral(mmm, tuning):
    """D = 40 <= 140.625 < D * R = 160: the singles take 32 x 1, the batch 16 x 2 (this choice counts the replicas).  Both associate a
    document's sums as the 32-lane butterfly does: every bit equal, device to device."""
    tuning(geometry_cus=CUS)
    c = walk_case("cfg4_lanes")
    assert c["D"] < 9000 * CUS / 256 <= c["D"] * R
    gb, gs, _ = batch_equals_singles(mmm, c, keys=BIT_KEYS[:-2])
    assert _bits(gs) == GEO4["cfg4_lanes"]
    assert (gs["Ls"], gs["cpl"]) == (32, 1) and (gb["Ls"], gb["cpl"]) == (16, 2), (gb, gs)


def test_sum_k_28_wave_counts_are_bit_neutral(mmm, tuning):
    """D = 200 < 625 <= D * R = 800, both beyond the lane threshold: 16 x 2 with three (singles) and four (batch) persistent waves per SIMD."""
    tuning(geometry_cus=CUS)
    c = walk_case("cfg4_waves")
    assert 9000 * CUS / 256 <= c["D"] < 40000 * CUS / 256 <= c["D"] * R
    gb, gs, _ = batch_equals_singles(mmm, c)
    assert _bits(gs) == GEO4["cfg4_waves"]
    # a block of 4 waves x 4 slots holds 16 documents: 13 blocks give every document a slot of its own; resident are CUs x waves per SIMD
    # blocks, 12 with three (the singles: documents wait for a slot) and 16 with four (the batch: all 13 blocks)
    assert gs["solve_waves"] == 4 * min(13, CUS * 3) and gb["solve_waves"] == 4 * min(13, CUS * 4), (gb, gs)


# ------------------------------------------------------------------------------------------ e. a pinned layout at any corpus size
def _heldout_pair(mmm, tuning, case, lanes):
    c = walk_case(case, D=1500)
    tuning(geometry_cus=CUS)
    model = _make(mmm, c["K"], c["V"], c["X"][:200], c["g0"][0], c["feats"])
    mmm.fit(model, maxiter=6, tol=0.0, verbose=False)
    tuning(geometry_cus=CUS, solve_lanes=lanes)
    out = []
    for D in (50, 1500):
        h = mmm.fit_heldout(c["X"][:D], model, maxiter=2)
        assert len(h.ll_history) == 2
        out.append(h)
    return out


def _same_first_documents(a, b, n):
    M = a.M
    _same_bits(a.lam_matrix()[:n], b.lam_matrix()[:n], "lambda"); _same_bits(a.nu_matrix()[:n], b.nu_matrix()[:n], "nu")
    _same_bits(a._get("zeta").reshape(a.D, M)[:n], b._get("zeta").reshape(b.D, M)[:n], "zeta")
    sa, sb = a.solver_stats(per_doc=True), b.solver_stats(per_doc=True)
    assert np.array_equal(sa["per_doc_nu"][:n], sb["per_doc_nu"][:n]) and np.array_equal(sa["per_doc_lambda"][:n], sb["per_doc_lambda"][:n])


@pytest.mark.parametrize("case,lanes", [("imm10", 8), ("imm10", 2), ("cfg4_lanes", 0)])
def test_a_documents_bits_do_not_depend_on_the_corpus_it_is_held_out_with(mmm, tuning, case, lanes):
    """Under frozen topics, mu and Sigma a document's solves read nothing from its companions, so the first 50 documents of fit_heldout
    over 50 and over 1,500 documents (either side of every threshold at 4 CUs) get the same lambda, nu, zeta and evaluation counts --
    provided both handles run the same association.  Sum K = 28 does on its own (32 x 1 and 16 x 2 are bit-neutral); sum K = 10 does with
    `solve_lanes` pinned, which is what the header promises of it.  See the next test for sum K = 10 unpinned."""
    small, large = _heldout_pair(mmm, tuning, case, lanes)
    gs, gl = small.geometry(), large.geometry()
    if lanes:
        assert (gs["Ls"], gs["cpl"]) == (gl["Ls"], gl["cpl"]) == {8: (8, 2), 2: (2, 5)}[lanes]
    else:
        assert (gs["Ls"], gs["cpl"]) == (32, 1) and (gl["Ls"], gl["cpl"]) == (16, 2)
    _same_first_documents(small, large, 50)


def test_sum_k_10_unpinned_the_corpus_size_picks_the_layout(mmm, tuning):
    """The one place where the size of the corpus changes a document's bits: sum K = 10 with `solve_lanes` left at 0 takes 8 x 2 below
    75,000 x cus / 256 documents and 2 x 5 from there, and the two associate a document's sums differently (lambda differs at the 1e-11
    level, tests/test_twin_cpu.py).  A caller who needs the same bits for the same document in corpora of any size pins `solve_lanes`
    (2 or 8) -- the previous test."""
    small, large = _heldout_pair(mmm, tuning, "imm10", 0)
    gs, gl = small.geometry(), large.geometry()
    assert (gs["Ls"], gs["cpl"]) == (8, 2) and (gl["Ls"], gl["cpl"]) == (2, 5), (gs, gl)


# ------------------------------------------------------------------------------------------ f. each branch against the oracle
@pytest.mark.parametrize("case", ["imm10", "mm55", "cfg4_lanes", "cfg4_waves"])
def test_every_branch_of_the_walk_equals_the_order_matched_oracle(mmm, oracle, tuning, case):
    """The single handle and one replica of the batch of cases a, c and d, three passes each against the oracle built from the geometry the
    handle reports: the walk is tied to the independent restatement, not only device to device."""
    tuning(geometry_cus=CUS)
    c = walk_case(case)
    K, V, X, feats, D, MK = c["K"], c["V"], c["X"], c["feats"], c["D"], sum(c["K"])
    r = 2
    batch = _make(mmm, K, V, X, c["g0"], feats, restarts=R).select(r)
    single = _make(mmm, K, V, X, c["g0"][r], feats)
    assert _bits(single.geometry()) == GEO4[case]
    for g in (single, batch):
        geo = g.geometry()
        kw = dict(features=feats) if feats is not None else dict(V=V)
        o = oracle.CtmOracle(K, [0.1] * len(K), X, gamma0=_flat(c["g0"][r]), geometry=geo, **kw)
        for it in range(3):
            mmm._lib.check(mmm.lib().mmm_ctm_iterate(g._h, 1, 1), g.ctx.h, "iterate")
            assert o.twin_pass(True) == 0
            st = g.solver_stats(per_doc=True)
            assert np.array_equal(st["per_doc_nu"], o.nev_nu[:D]) and np.array_equal(st["per_doc_lambda"], o.nev_lambda[:D]), (geo, it)
            _same_state(g, o, D, MK)
        g.close()
