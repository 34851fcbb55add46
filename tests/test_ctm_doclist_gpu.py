"""Stage calls on document lists (mmm_ctm_update_docs; update_ζ!/θ!/ν!/λ!(model, d) and fitdoc!(model, d), MMCTM.jl:127-198, 450-455)
and the per-document field transfers (mmm_ctm_get_doc / mmm_ctm_set_doc).

The contract is bitwise: a listed document gets exactly what the whole-corpus stage writes for it on a handle in the same state, every
other document keeps every bit and counter.  Each shape is checked to reach the build it is meant to (mmm_ctm_geometry)."""
import os
import time

import numpy as np
import pytest

import np_ref
from test_ctm_gpu import SNV3

pytestmark = pytest.mark.gpu

STAGES = ("zeta", "theta", "nu", "lambda", "fitdoc")
ERR_ARG = -1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fn(mmm, stage):
    return {"zeta": mmm.update_ζ, "theta": mmm.update_θ, "nu": mmm.update_ν, "lambda": mmm.update_λ, "fitdoc": mmm.fitdoc}[stage]


def _theta_doc(model):
    """document id of every value of the flat theta field"""
    D, out = model.D, []
    for m in range(model.M):
        dp = np.asarray(model._doc_ptr[m * (D + 1):(m + 1) * (D + 1)], dtype=np.int64)
        out.append(np.repeat(np.repeat(np.arange(D), np.diff(dp)), model.K[m]))
    return np.concatenate(out)


def _state(mmm, model, sum_docs=()):
    st = model.solver_stats(per_doc=True)
    return {"lambda": model.lam_matrix().copy(), "nu": model.nu_matrix().copy(), "zeta": model._get("zeta").reshape(model.D, model.M).copy(),
            "theta": model._get("theta").copy(), "nev_nu": st["per_doc_nu"].copy(), "nev_lambda": st["per_doc_lambda"].copy(),
            "sumtheta": {int(d): mmm.calculate_sumθ(model, int(d)) for d in sum_docs}}


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.int64) if np.asarray(a).dtype == np.float64 else a,
                          np.asarray(b).view(np.int64) if np.asarray(b).dtype == np.float64 else b)


def _check_rows(model, listed, A, B, before, what):
    """listed rows of A == B (the whole-corpus stage), the other rows of A == before"""
    D = model.D
    inl = np.zeros(D, dtype=bool); inl[np.asarray(listed, dtype=np.int64)] = True
    for f in ("lambda", "nu", "zeta", "nev_nu", "nev_lambda"):
        assert _same(A[f][inl], B[f][inl]), "%s: %s of a listed document differs from the whole-corpus stage" % (what, f)
        assert _same(A[f][~inl], before[f][~inl]), "%s: %s of an unlisted document changed" % (what, f)
    td = _theta_doc(model)
    tl = inl[td]
    assert _same(A["theta"][tl], B["theta"][tl]), "%s: theta of a listed document differs" % what
    assert _same(A["theta"][~tl], before["theta"][~tl]), "%s: theta of an unlisted document changed" % what
    for d, v in A["sumtheta"].items():
        assert _same(v, (B if inl[d] else before)["sumtheta"][d]), "%s: sumθ of document %d" % (what, d)


def _mm(mmm, K, V, D, seed, means, feats=None, empty_frac=0.1):
    X, g0 = np_ref.synth_mm(D, V, K, seed=seed, means=means, empty_frac=empty_frac)
    if feats is None:
        return lambda: mmm.MMCTM(K, [0.1] * len(K), V, X, γ0=g0)
    GM = sum(K[m] * int(np.asarray(feats[m]).max(axis=0).sum()) for m in range(len(K)))
    gflat = np.random.default_rng(seed).integers(1, 101, size=GM).astype(np.float64)
    return lambda: mmm.IMMCTM(K, [0.1] * len(K), feats, X, γ0=gflat)


CTX5 = [np.array([[(t // 384) % 4 + 1, (t // 96) % 4 + 1, (t // 16) % 6 + 1, (t // 4) % 4 + 1, t % 4 + 1] for t in range(1536)])]

# name: (tuning, corpus, expected geometry subset)
SHAPES = {
    "k10_lanes2": (dict(solve_lanes=2), dict(K=[10], V=[96], D=200, seed=71, means=[1500]), {"Ls": 2, "cpl": 5}),
    "k10_lanes8": (dict(solve_lanes=8), dict(K=[10], V=[96], D=200, seed=72, means=[1500]), {"Ls": 8, "cpl": 2}),
    "k14": ({}, dict(K=[7, 7], V=[96, 48], D=200, seed=73, means=[2000, 60]), {"L": 16, "Ls": 16, "cpl": 1}),
    "k28_lanes16": (dict(solve_lanes=16), dict(K=[10, 10, 8], V=[96, 38, 32], D=200, seed=74, means=[2000, 150, 100]), {"Ls": 16, "cpl": 2}),
    "k28_lanes32": (dict(solve_lanes=32), dict(K=[10, 10, 8], V=[96, 38, 32], D=200, seed=75, means=[2000, 150, 100]), {"Ls": 32, "cpl": 1}),
    "k12_packed": ({}, dict(K=[6, 6], V=[40, 24], D=150, seed=76, means=[600, 80]), {"L": 16, "Ls": 12}),
    "k44_64lanes": ({}, dict(K=[22, 22], V=[96, 48], D=120, seed=77, means=[2500, 300]), {"L": 64, "Ls": 64}),
    "k80_big": ({}, dict(K=[40, 40], V=[60, 40], D=60, seed=78, means=[900, 300]), {"wide": 1, "Ls": 64, "cpl": 4}),
    # lock-step solve builds at 4 waves per SIMD (OCC = 4): a pretended 4-CU device, on which the handle's whole-corpus solve launch is
    # more than three waves per SIMD (the `small` test of launch_phase) -- sum K = 10, 14 and 28 one coordinate per lane
    "k10_lockstep_occ4": (dict(geometry_cus=4, disable=("ctm_cpl", "ctm_packed")), dict(K=[10], V=[96], D=200, seed=85, means=[1500]),
                          {"L": 16, "Ls": 16, "cpl": 1, "occ4": True}),
    "k14_occ4": (dict(geometry_cus=4), dict(K=[7, 7], V=[96, 48], D=200, seed=86, means=[2000, 60]), {"L": 16, "Ls": 16, "cpl": 1, "occ4": True}),
    "k28_lockstep_occ4": (dict(geometry_cus=4, disable=("ctm_cpl",)), dict(K=[10, 10, 8], V=[96, 38, 32], D=200, seed=87, means=[2000, 150, 100]),
                          {"L": 32, "Ls": 32, "cpl": 1, "occ4": True}),
    "imm1536_wide": ({}, dict(K=[12], V=[1536], D=60, seed=79, means=[4000], feats=CTX5), {"wide": 1}),
    "imm_k6": ({}, dict(K=[6], V=[96], D=150, seed=80, means=[1500], feats=SNV3), {"L": 16, "Ls": 6}),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_list_stage_is_bitwise_the_whole_corpus_stage(mmm, tuning, shape):
    """Two handles advanced identically by two fused passes (theta then held implicitly).  On one, stage(S); on the other, the
    whole-corpus stage.  Rows in S are equal; rows outside S are as they were.  Every stage, three lists: one document, a random
    unsorted third of the corpus, the whole corpus permuted."""
    tune, corpus, expect = SHAPES[shape]
    tuning(**tune)
    corpus = dict(corpus)
    make = _mm(mmm, corpus.pop("K"), corpus.pop("V"), corpus.pop("D"), corpus.pop("seed"), corpus.pop("means"), corpus.pop("feats", None))
    probe = make()
    geo = probe.geometry()
    expect = dict(expect)
    occ4 = expect.pop("occ4", False)
    for k, v in expect.items():
        assert geo[k] == v, (shape, geo)
    D = probe.D
    if occ4:      # blocks of the whole-corpus lock-step solve launch (4 waves, 64 / Ls documents each) x 4 waves > 3 waves x 4 SIMDs x 4 CUs
        assert geo["solve_waves"] == 0 and -(-D // (4 * (64 // geo["Ls"]))) * 4 > 3 * 4 * 4, geo
    rng = np.random.default_rng(D)
    lists = {"one": [int(rng.integers(D))], "third": [int(x) for x in rng.choice(D, D // 3, replace=False)], "all": [int(x) for x in rng.permutation(D)]}
    assert lists["third"] != sorted(lists["third"])
    for stage in STAGES:
        for lname, S in lists.items():
            A, B, C0 = make(), make(), make()
            for h in (A, B, C0):
                mmm.fit(h, maxiter=2, tol=0.0, verbose=False)
            probe_docs = sorted(set(S[:3]) | set(int(x) for x in rng.choice(D, 3, replace=False)))
            before = _state(mmm, C0, probe_docs)      # (from a third twin: A's theta stays implicit until the list call)
            _fn(mmm, stage)(A, S)
            _fn(mmm, stage)(B)
            _check_rows(A, S, _state(mmm, A, probe_docs), _state(mmm, B, probe_docs), before, "%s %s %s" % (shape, stage, lname))


def _config3(mmm):
    terms1, samples, snv = mmm.read_counts_tsv(os.path.join(GOLD, "brca-eu_snv_counts.tsv"))
    terms2, samples2, sv = mmm.read_counts_tsv(os.path.join(GOLD, "brca-eu_sv_counts.tsv"))
    X = mmm.format_counts_mmctm([{s: snv[:, i] for i, s in enumerate(samples)}, {s: sv[:, i] for i, s in enumerate(samples)}], samples)
    rng = np.random.default_rng(2)
    g0 = [rng.integers(1, 101, size=(7, 96)).astype(np.float64), rng.integers(1, 101, size=(7, 48)).astype(np.float64)]
    return mmm.MMCTM([7, 7], [0.1, 0.1], [96, 48], X, γ0=g0)


def test_reference_loop_of_fitdoc_equals_the_stage_sequence(mmm):
    """The reference's `for d in 1:D fitdoc!(model, d) end` (MMCTM.jl:462-464) then update_μ!, update_Σ!, update_γ! on config 3 equals
    fitdoc!(model) over every document then the same updates: every bit of the E-step state and of μ, Σ; γ to rounding (atomics)."""
    a, b = _config3(mmm), _config3(mmm)
    mmm.fit(a, maxiter=2, tol=0.0, verbose=False); mmm.fit(b, maxiter=2, tol=0.0, verbose=False)
    for d in range(a.D):
        mmm.fitdoc(a, d)
    mmm.fitdoc(b)
    for g in (a, b):
        mmm.update_μ(g); mmm.update_Σ(g); mmm.update_γ(g)
    for f in ("lambda", "nu", "zeta", "theta", "mu", "Sigma", "invSigma"):
        assert _same(a._get(f), b._get(f)), f
    # (the stage update_γ! adds the statistics with global atomics -- k_ctm_gamma_from_theta -- so its sums are not associated the same
    # way from run to run, whatever the θ it reads; that θ is bitwise the same above)
    for f in ("gamma", "Elnphi"):
        np.testing.assert_allclose(a._get(f), b._get(f), rtol=1e-12, atol=0, err_msg=f)
    sa, sb = a.solver_stats(per_doc=True), b.solver_stats(per_doc=True)
    assert _same(sa["per_doc_nu"], sb["per_doc_nu"]) and _same(sa["per_doc_lambda"], sb["per_doc_lambda"])


def test_list_call_on_a_batch_replica(mmm):
    """R = 3: a list call on replica 1 equals the same call on a single handle built from replica 1's γ0 and advanced alike; replicas
    0 and 2 keep every bit."""
    K, V = [5, 4], [40, 24]
    X, _ = np_ref.synth_mm(90, V, K, seed=81, means=[600, 80], empty_frac=0.1)
    rng = np.random.default_rng(5)
    g0 = [[rng.integers(1, 101, size=(K[m], V[m])).astype(np.float64) for m in range(2)] for _ in range(3)]
    batch = mmm.MMCTM(K, [0.1, 0.1], V, X, γ0=g0, restarts=3)
    mmm.fit_restarts(batch, maxiter=2, tol=0.0)
    assert list(batch.restart_iters) == [2, 2, 2]
    single = mmm.MMCTM(K, [0.1, 0.1], V, X, γ0=g0[1])
    mmm.fit(single, maxiter=2, tol=0.0, verbose=False)
    assert single.geometry() == batch.geometry()
    fields = ("lambda", "nu", "zeta", "theta")
    keep = {}
    for r in (0, 2):
        batch.select(r)
        keep[r] = {f: batch._get(f) for f in fields}
    S = [int(x) for x in rng.choice(90, 30, replace=False)]
    batch.select(1)
    mmm.fitdoc(batch, S); mmm.update_ν(batch, S[:5])
    mmm.fitdoc(single, S); mmm.update_ν(single, S[:5])
    for f in fields:
        assert _same(batch._get(f), single._get(f)), f
    sa, sb = batch.solver_stats(per_doc=True), single.solver_stats(per_doc=True)
    assert _same(sa["per_doc_nu"], sb["per_doc_nu"]) and _same(sa["per_doc_lambda"], sb["per_doc_lambda"])
    for r in (0, 2):
        batch.select(r)
        for f in fields:
            assert _same(batch._get(f), keep[r][f]), "replica %d: %s changed" % (r, f)


FID = {"lambda": 6, "nu": 7, "zeta": 8, "props": 9, "theta": 10}


def _get_doc(mmm, g, f, d, n):
    out = np.empty(n)
    return mmm.lib().mmm_ctm_get_doc(g._h, FID[f], d, out, n), out


def test_per_document_fields(mmm):
    """get_doc = the slice of the whole field; set_doc changes that document only (theta: also when it was held implicitly);
    model.λ[d] = v followed by update_ν!(model, d) = the whole-field upload route."""
    K, V, D = [5, 4], [40, 24], 80
    X, g0 = np_ref.synth_mm(D, V, K, seed=82, means=[600, 80], empty_frac=0.2)
    make = lambda: mmm.MMCTM(K, [0.1, 0.1], V, X, γ0=g0)
    g = make()
    mmm.fit(g, maxiter=2, tol=0.0, verbose=False)
    mmm.update_props(g)
    td = _theta_doc(g)
    empty = [d for d in range(D) if X[d][1].shape[0] == 0]
    assert empty
    for d in [0, 7, D - 1, empty[0]]:
        for f, w in (("lambda", 9), ("nu", 9), ("props", 9), ("zeta", 2)):
            rc, v = _get_doc(mmm, g, f, d, w)
            assert rc == 0 and _same(v, g._get(f)[d * w:(d + 1) * w]), (f, d)
        n = int((td == d).sum())
        rc, v = _get_doc(mmm, g, "theta", d, n)
        assert rc == 0 and _same(v, g._get("theta")[td == d]), d
        assert _get_doc(mmm, g, "theta", d, n + 1)[0] == ERR_ARG
    assert _get_doc(mmm, g, "lambda", D, 9)[0] == ERR_ARG and _get_doc(mmm, g, "lambda", -1, 9)[0] == ERR_ARG
    assert mmm.lib().mmm_ctm_get_doc(g._h, 0, 0, np.empty(9), 9) == ERR_ARG       # mu has no per-document part
    # set_doc: only that document changes
    rng = np.random.default_rng(3)
    for f, w in (("lambda", 9), ("nu", 9), ("props", 9), ("zeta", 2)):
        before = g._get(f).copy()
        v = rng.uniform(0.5, 2.0, w)
        assert mmm.lib().mmm_ctm_set_doc(g._h, FID[f], 11, v, w) == 0
        after = g._get(f)
        assert _same(after[11 * w:12 * w], v)
        before[11 * w:12 * w] = v
        assert _same(after, before), f
    # theta after fused passes (held implicitly): set_doc leaves every other document's theta as materialising it gives
    a, b = make(), make()
    mmm.fit(a, maxiter=2, tol=0.0, verbose=False); mmm.fit(b, maxiter=2, tol=0.0, verbose=False)
    n = int((td == 11).sum())
    v = rng.uniform(0.0, 1.0, n)
    assert mmm.lib().mmm_ctm_set_doc(a._h, FID["theta"], 11, v, n) == 0
    ta, tb = a._get("theta"), b._get("theta")
    assert _same(ta[td == 11], v) and _same(ta[td != 11], tb[td != 11])
    # the view leaves: θ[d][m] and props[d][m] round trip through the per-document calls
    th0, th1 = np.asarray(a.θ[11][0]), np.asarray(a.θ[11][1])
    a.θ[11][1] = th1 * 0.5
    assert _same(np.asarray(a.θ[11][1]), th1 * 0.5) and _same(np.asarray(a.θ[11][0]), th0)
    assert _same(a._get("theta")[td != 11], tb[td != 11])
    p0 = np.asarray(a.props[11][0])
    a.props[11][1] = np.full(4, 0.25)
    assert _same(np.asarray(a.props[11][1]), np.full(4, 0.25)) and _same(np.asarray(a.props[11][0]), p0)
    # model.λ[d] = v then update_ν!(model, d) == the whole-field route
    a, b = make(), make()
    mmm.fit(a, maxiter=2, tol=0.0, verbose=False); mmm.fit(b, maxiter=2, tol=0.0, verbose=False)
    v = a.λ[5] + 0.25
    a.λ[5] = v
    flat = b._get("lambda"); flat[5 * 9:6 * 9] = v; b._set("lambda", flat)
    mmm.update_ν(a, 5); mmm.update_ν(b, 5)
    assert _same(a._get("nu"), b._get("nu")) and _same(a._get("lambda"), b._get("lambda"))
    assert _same(a.solver_stats(per_doc=True)["per_doc_nu"], b.solver_stats(per_doc=True)["per_doc_nu"])


def test_refusals_leave_the_state_unchanged(mmm):
    K, V, D = [5, 4], [40, 24], 60
    X, g0 = np_ref.synth_mm(D, V, K, seed=83, means=[600, 80], empty_frac=0.1)
    g = mmm.MMCTM(K, [0.1, 0.1], V, X, γ0=g0)
    mmm.fit(g, maxiter=2, tol=0.0, verbose=False)
    before = _state(mmm, g)
    L = mmm.lib()
    for stage, docs, n in ((4, [3, 5, 3], 3), (4, [-1], 1), (4, [D], 1), (5, [1], 1), (-1, [1], 1), (4, [1], -1)):
        arr = np.ascontiguousarray(docs, dtype=np.int32)
        assert L.mmm_ctm_update_docs(g._h, stage, arr.ctypes.data, n) == ERR_ARG, (stage, docs, n)
    assert L.mmm_ctm_update_docs(g._h, 4, None, 2) == ERR_ARG
    assert L.mmm_ctm_update_doc(g._h, 4, D) == ERR_ARG
    assert L.mmm_ctm_update_docs(g._h, 4, None, 0) == 0
    assert L.mmm_ctm_update_docs(g._h, 2, np.zeros(1, dtype=np.int32).ctypes.data, 0) == 0
    after = _state(mmm, g)
    for f in ("lambda", "nu", "zeta", "theta", "nev_nu", "nev_lambda"):
        assert _same(after[f], before[f]), f


def test_one_document_cost_does_not_grow_with_D(mmm, tuning):
    """A config-4-shaped handle at D = 50,000 and one over its first 2,000 documents, with the same globals and the same state of the
    listed document: the one-document fitdoc! gives the same bits, and its median wall time at 50k is at most 1.5x the one at 2k."""
    K, V = [10, 10, 8], [96, 38, 32]
    tuning(solve_lanes=16)
    X, g0 = np_ref.synth_mm(50000, V, K, seed=20261007)
    big = mmm.MMCTM(K, [0.1] * 3, V, X, γ0=g0)
    small = mmm.MMCTM(K, [0.1] * 3, V, X[:2000], γ0=g0)
    assert big.geometry()["Ls"] == small.geometry()["Ls"] == 16
    mmm._lib.check(mmm.lib().mmm_ctm_iterate(big._h, 2, 1), big.ctx.h, "iterate")
    for f in ("mu", "Sigma", "invSigma", "Elnphi"):
        small._set(f, big._get(f))
    d = 1234
    small.λ[d] = big.λ[d]
    small.ν[d] = big.ν[d]
    mmm.fitdoc(big, d); mmm.fitdoc(small, d)
    assert _same(big.λ[d], small.λ[d]) and _same(big.ν[d], small.ν[d]) and _same(big.ζ[d], small.ζ[d])
    for m in range(3):
        assert _same(np.asarray(big.θ[d][m]), np.asarray(small.θ[d][m]))

    def med(g, n=30):
        for _ in range(3):
            mmm.fitdoc(g, d)
        t = []
        for _ in range(n):
            t0 = time.perf_counter(); mmm.fitdoc(g, d); t.append(time.perf_counter() - t0)
        return float(np.median(t))
    tb, ts = med(big), med(small)
    print("one-document fitdoc!: D = 50,000 %.1f us, D = 2,000 %.1f us (ratio %.2f)" % (tb * 1e6, ts * 1e6, tb / ts))
    assert tb <= 1.5 * ts, (tb, ts)
