"""Sharded fits with several ranks on one card, on every build, model and shard edge -- against independent references on the FULL corpus.

Three groups of ranks are spawned, once each (worlds of 2, 3 and 4 processes, module-scoped fixtures); every rank has its own context on
device 0 and the xGMI mailboxes to its peers (tests/sharded_ref.py run_ranks).  Each group runs an ordered list of named scenarios on one
communicating context and ends with a small known fit, which shows that no earlier scenario left the ranks' sequence numbers out of
step.  Every test function asserts on ONE scenario of one group: the route the launches took (Model.last_pass(), geometry()), the same
bits on every rank, and the global state against the reference.

References and bounds (none is derived from the sharded output):
  LDA     np_ref.lda_iteration on the full corpus.  One pass: rtol 1e-11 on λ, β, Elnβ (atol 1e-13), γ, ll -- test_lda_gpu.py
          test_single_sweep_matches_oracle; three passes: rtol 1e-9 -- its fused-pass test.  The all-reduced statistics of pass 1 are sums
          of non-negative terms n ϕ: they hold (γ_n + γ_ϕ) x their value, n = documents listing the term + tree depth + ranks
          (sharded_ref.sum_roundings), γ_ϕ the roundings of a ϕ the device forms (elbo_ref.phi_roundings), floor 4 units in the last place.
  ILDA    ilda_ref on the full corpus, rtol 1e-9 (Elnβ 1e-8, atol 1e-13): test_ilda_dispatch_gpu.py.  The factor statistics of pass 1, λ_i - η_i,
          hold (γ_n + γ_ϕ) x their value like LDA's (n: the documents and terms of the feature value); the seven ELBO terms hold elbo_ref's bound.
  CTM     the index-order C oracle on the full corpus at the bounds of test_ctm_gpu.py's fused-pass test (γ, μ, Σ 1e-5; ll 1e-6; ELBO 1e-5),
          and μ, Σ recomputed in numpy from the λ, ν gathered from all ranks at its stage bounds (μ 1e-11, Σ 1e-9 / 1e-12): the Gaussian
          M-step divides by the GLOBAL number of documents, the shards are uneven.  The γ sums of pass 1 are formed from θ = softmax Elnϕ₀ (the
          constructor's λ is 0: no solve enters), so they are restated in np.longdouble from γ0 and hold (γ_n + γ_θ) x their value, floor 4 ulp
          (sharded_ref.ctm_gamma_pass1); the seven ELBO terms hold elbo_ref's bound on the state gathered from all ranks.
  ELBO    elbo_ref on the state gathered from all ranks, max(γ_n A, 4 units) per term with one more rounding per rank.
  whole fits  every rank the same bits, the pass count of the unsharded device fit, ll rtol 1e-11, β 1e-9 (test_p2p_gpu.py).

Shards: explicit uneven bounds, so that a local D or N in place of the global one shows; the 41-document edge corpora are cut
[0, 41, 41] (last rank empty), [0, 0, 40, 41] (first rank empty, last rank one document, which carries tokens) and [0, 20, 20, 24, 41] (a
middle rank empty, the next holding four documents without a token; in the MMCTM corpus the last rank's second modality is empty throughout).
_shards asserts these local D and N."""
import numpy as np
import pytest

import sharded_ref as S
from ilda_ref import dist

pytestmark = pytest.mark.gpu

ONE, RUN, RUN_ELN = 1e-11, 1e-9, 1e-8
EDGE_BOUNDS = {2: [0, 41, 41], 3: [0, 0, 40, 41], 4: [0, 20, 20, 24, 41]}


# ------------------------------------------------------------------------------------------------------------ scenario tables
def lda(name, K, V, D, kind="lda_passes", **kw):
    return dict(name=name, kind=kind, K=K, V=V, D=D, **kw)


def _cap(K, V, extra):
    """resident_cap that leaves `extra` ll blocks beside the merged launch's reduce blocks"""
    return ((V + 15) & ~15) * K // 16 + extra


KNOWN = lda("known_fit", 10, 96, 120, kind="lda_fit", maxiter=14, tol=0.0, plain=True, seed=9, mean_n=500, expect=("merged", "p2p", "packed"), packed=True)

EDGES = [
    lda("edge_lda_folded", 10, 96, 41, expect=("merged", "p2p", "packed"), packed=True),
    lda("edge_lda_split", 10, 90, 41, tuning={"disable": ("lda_merged",)}, expect=("split", "p2p")),
    dict(name="edge_ilda", kind="ilda", K=5, V=90, D=41, J=[8, 4, 4], eta=[0.1, 0.3, 0.2], seed=3),
    dict(name="edge_mmctm", kind="ctm", K=[5, 4], V=[40, 24], D=41, alpha=[0.1, 0.1], means=[600, 80], empty_modality=((24, 41, 1),)),
]

# ---- two ranks: the folded merged launch on every padded topic count.  Above 20 topics the 96-term shape cannot run here: two ranks'
#      launches of 6 K + 1 blocks each do not fit one card together (sharded_ref.check_residency); V = 40 / 48 reaches those builds
SWEEP = []
for _K in (2, 4, 5, 7, 9, 11, 13, 17, 22, 27):
    for _V in ((90, 96) if _K <= 17 else (40, 48)):
        _t = {"lda_build": "sparse"}
        if _K >= 13:
            _t["resident_cap"] = _cap(_K, _V, 6)
        SWEEP.append(lda("sweep_K%d_V%d" % (_K, _V), _K, _V, 53, bounds=[0, 37, 53], tuning=_t, expect=("merged", "p2p"), KP=S.pick_kp(_K)))
WORLD2 = SWEEP + EDGES + [KNOWN]

# ---- three ranks: builds, routes, payloads, the stopping rule, the stage API, inference, ILDA, CTM
U60 = [0, 9, 35, 60]
STOP = dict(D=120, maxiter=40, tol=2.1e-3, plain=True, seed=9, mean_n=500)
ROUTES = [
    lda("block_stats", 10, 96, 60, bounds=U60, expect=("merged", "p2p", "packed"), packed=True, geo={"single_step": 1, "block_stats": 1, "dense": 0}, moved=1),
    lda("block_stats_V90", 10, 90, 60, bounds=U60, tuning={"disable": ("lda_count_rows",)}, expect=("merged", "p2p", "packed"), packed=True,
        geo={"single_step": 1, "block_stats": 1, "row_bytes": 8 * 90}, moved=1),
    lda("slabs", 10, 96, 60, bounds=U60, tuning={"disable": ("lda_block_stats",)}, expect=("merged", "p2p", "packed"), packed=True,
        geo={"single_step": 1, "block_stats": 0}, moved=1),
    lda("unpacked", 5, 40, 60, bounds=U60, expect=("merged", "p2p"), not_expect=("packed",), geo={"single_step": 1}),
    lda("late_prologue", 10, 96, 60, bounds=U60, tuning={"disable": ("lda_early_prologue",)}, expect=("merged", "p2p", "packed"), packed=True, moved=0),
    lda("rows_of_counts", 10, 96, 60, bounds=U60, mean_n=3000, expect=("merged", "p2p", "packed"), packed=True, geo={"single_step": 1, "row_bytes": 2 * 16 * 6}),
    lda("rows_of_counts_32bit", 10, 96, 60, bounds=U60, mean_n=3000, tuning={"disable": ("lda_rows16",)}, expect=("merged", "p2p", "packed"), packed=True,
        geo={"single_step": 1, "row_bytes": 4 * 16 * 6}),
    lda("dense_rows", 10, 96, 60, bounds=U60, mean_n=3000, tuning={"lda_build": "dense"}, expect=("merged", "p2p"), not_expect=("packed",),
        geo={"dense": 1, "row_bytes": 2 * 16 * 6}),
    lda("dense_rows_32bit", 10, 90, 60, bounds=U60, mean_n=3000, tuning={"lda_build": "dense", "disable": ("lda_rows16",)}, expect=("merged", "p2p"),
        geo={"dense": 1, "row_bytes": 4 * 16 * 6}),
    lda("grid_stride", 10, 96, 60, bounds=U60, tuning={"grid_blocks": 3}, expect=("merged", "p2p"), not_expect=("packed",), geo={"single_step": 0, "grid_e": 3}),
    # the reduce blocks join the ll sweep where a rank's documents outnumber its two ll blocks' 128: ranks 1 and 2, not rank 0
    lda("ll_join", 10, 96, 300, bounds=[0, 40, 170, 300], mean_n=3000, tuning={"lda_build": "dense", "resident_cap": 62}, expect=("merged", "p2p"),
        join=(False, True, True)),
    lda("split_disabled", 10, 96, 60, bounds=U60, tuning={"disable": ("lda_merged",)}, expect=("split", "p2p")),
    lda("split_residency", 10, 90, 60, bounds=U60, tuning={"resident_cap": 30}, expect=("split", "p2p")),
    lda("split_V260", 4, 260, 60, bounds=U60, mean_n=900, expect=("split", "p2p")),
    # the widest payload of the folded exchange on one card: 32 x 96 + 1 = 3,073 doubles through lda_reduce_block and k_lda_mstep<true>
    lda("split_K32", 32, 96, 60, bounds=U60, tuning={"lda_build": "sparse", "resident_cap": 64}, expect=("split", "p2p"), KP=32),
    lda("unfolded_sparse", 10, 96, 60, bounds=U60, tuning={"disable": ("p2p_folded",)}, expect=("split", "ll_cells"), not_expect=("p2p",)),
    lda("unfolded_dense", 10, 90, 60, bounds=U60, mean_n=3000, tuning={"lda_build": "dense", "disable": ("p2p_folded",)}, expect=("split", "ll_cells"),
        not_expect=("p2p",), geo={"dense": 1}),
    lda("wide_K10", 10, 96, 60, bounds=U60, tuning={"lda_build": "wide"}, expect=("wide",), not_expect=("p2p", "big"), geo={"wide": 1}),
    lda("wide_K40", 40, 90, 60, bounds=U60, expect=("wide", "big"), not_expect=("p2p",), geo={"wide": 1}),
    # 85 x 96 + 1 = 8,161 doubles: the largest LDA payload the mailboxes take (stand-alone k_p2p_allreduce; no build below the wide path
    # holds 85 topics)
    lda("payload_8161", 85, 96, 60, bounds=U60, expect=("wide", "big"), geo={"wide": 1}),
    lda("payload_8257", 86, 96, 60, bounds=U60, kind="lda_overflow", geo={"wide": 1}),
    lda("after_overflow", 7, 90, 60, bounds=U60, expect=("merged", "p2p")),
    lda("stop_folded", 10, 96, kind="lda_fit", expect=("merged", "p2p"), bounds=[0, 17, 75, 120], **STOP),
    lda("stop_split", 10, 96, kind="lda_fit", tuning={"disable": ("lda_merged",)}, expect=("split", "p2p"), bounds=[0, 17, 75, 120], **STOP),
    lda("stop_unfolded", 10, 96, kind="lda_fit", tuning={"disable": ("p2p_folded",)}, expect=("split", "ll_cells"), bounds=[0, 17, 75, 120], **STOP),
    lda("after_stop", 9, 90, 60, bounds=U60, expect=("merged", "p2p")),
    lda("stage_api", 7, 90, 60, bounds=U60, kind="lda_stage", empty=(1, 59)),
    lda("infer", 7, 90, 60, bounds=U60, kind="lda_infer", D_train=80, maxiter=40, tol=1e-4, empty=(3,)),
    dict(name="ilda_sj16_I3", kind="ilda", K=5, V=90, D=60, bounds=U60, J=[8, 4, 4], eta=[0.1, 0.3, 0.2], seed=1, maxiter=40, tol=2.1e-3, plain=True),
    dict(name="ilda_sj17_I3", kind="ilda", K=5, V=90, D=60, bounds=U60, J=[9, 4, 4], eta=[0.1, 0.3, 0.2], seed=2),
    dict(name="ilda_sj12_I2", kind="ilda", K=6, V=77, D=60, bounds=U60, J=[7, 5], eta=[0.2, 0.4], seed=4),
    dict(name="ilda_sj40_I2", kind="ilda", K=6, V=130, D=60, bounds=U60, J=[30, 10], eta=[0.2, 0.4], seed=5),
]
CTM = [
    dict(name="mmctm_slab", kind="ctm", K=[5, 4], V=[40, 24], D=60, bounds=U60, alpha=[0.1, 0.1], means=[600, 80], geo={"wide": 0, "tdense": 0}),
    dict(name="mmctm_sigma_off", kind="ctm", K=[5, 4], V=[40, 24], D=60, bounds=U60, alpha=[0.1, 0.1], means=[600, 80], flags=0),
    dict(name="mmctm_auto_alpha", kind="ctm", K=[5, 4], V=[40, 24], D=60, bounds=U60, alpha=[0.1, 0.1], means=[600, 80], flags=3),
    dict(name="immctm_dense_I3", kind="ctm", K=[6], V=[96], D=60, bounds=U60, alpha=[0.1], means=[900], imm=3, empty_frac=0.0,
         tuning={"ctm_build": "dense"}, geo={"tdense": 1}),
    dict(name="immctm_I1", kind="ctm", K=[6], V=[96], D=60, bounds=U60, alpha=[0.1], means=[900], imm=1, empty_frac=0.0),
    dict(name="mmctm_wide", kind="ctm", K=[5, 4], V=[40, 24], D=60, bounds=U60, alpha=[0.1, 0.1], means=[600, 80], tuning={"ctm_build": "wide"}, geo={"wide": 1}),
]
MM = dict(K=[5, 4], V=[40, 24], alpha=[0.1, 0.1], means=[600, 80])
CTM += [
    # a modality of 40 topics takes the wide path by itself; sum K = 65 the generic kernels of csrc/ctm_big.cuh.  Their statistics are
    # 2 ΣK + ΣK² + Σ K_m V_m + 16 doubles: the shapes of test_ctm_wide_gpu.py (40 + 40 topics over 96 + 48 terms: 12,336) do not fit a mailbox
    # call, so the vocabularies here are small (5,536 and 6,001 doubles)
    dict(name="mmctm_k40", kind="ctm", K=[40], V=[96], D=60, bounds=U60, alpha=[0.1], means=[3000], geo={"wide": 1}),
    dict(name="mmctm_big", kind="ctm", K=[33, 32], V=[30, 20], D=60, bounds=U60, alpha=[0.1, 0.1], means=[600, 300], geo={"Ls": 64, "cpl": 4}, big=True),
    dict(name="mmctm_doclist", kind="ctm_stage", D=60, bounds=U60, **MM),
    dict(name="mmctm_heldout", kind="ctm_heldout", D=60, D_train=70, bounds=U60, maxiter=3, plain=True, **MM),
    dict(name="mmctm_batch", kind="ctm_batch", D=60, bounds=U60, R=2, maxiter=30, tol=2e-3, **MM),
    # 20 restarts x 411 doubles = 8,220: beyond the mailbox, and there is no RCCL communicator
    dict(name="mmctm_batch_overflow", kind="ctm_batch", D=60, bounds=U60, R=20, maxiter=3, tol=0.0, **MM),
    dict(name="mmctm_after_overflow", kind="ctm", D=60, bounds=U60, **MM),
]
WORLD3 = ROUTES + CTM + EDGES + [KNOWN]

# ---- four ranks: the edges, balanced shards from shard_documents, the stage API once more
WORLD4 = [
    lda("balanced_V90", 9, 90, 83, expect=("merged", "p2p", "packed"), packed=True, balanced=True),
    lda("balanced_split", 9, 90, 83, tuning={"disable": ("lda_merged",)}, expect=("split", "p2p"), balanced=True),
    lda("stage_api", 7, 90, 41, kind="lda_stage"),
] + EDGES + [KNOWN]

TABLES = {2: WORLD2, 3: WORLD3, 4: WORLD4}


def _names(world, kinds=None, pred=None):
    return [sc["name"] for sc in TABLES[world] if (kinds is None or sc["kind"] in kinds) and (pred is None or pred(sc))]


def _sc(world, name):
    return next(sc for sc in TABLES[world] if sc["name"] == name)


# ------------------------------------------------------------------------------------------------------------------ fixtures
def _group(world):
    out = S.run_ranks(world, TABLES[world], bounds={41: EDGE_BOUNDS[world]})
    print("\n%d ranks: %.1f s in all; per scenario on rank 0: %s" % (world, out["seconds"]["total"], "  ".join(
        "%s %.2f" % kv for kv in (out["seconds"]["ranks"][0].items() if out["seconds"]["ranks"] else ()))))
    return out


@pytest.fixture(scope="module")
def world2():
    return _group(2)


@pytest.fixture(scope="module")
def world3():
    return _group(3)


@pytest.fixture(scope="module")
def world4():
    return _group(4)


@pytest.fixture
def groups(request):
    return lambda world: request.getfixturevalue("world%d" % world)


_REF = {}


def _cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _ranks(out, name):
    """the scenario's results per rank; a group in which some rank failed fails every test of it, with what the ranks recorded"""
    assert not out["errors"], "\n".join(out["errors"])
    assert len(out["ranks"]) == out["world"] and all(name in r for r in out["ranks"]), name
    return [r[name] for r in out["ranks"]]


def _same_bits(rs, fields):
    for f in fields:
        for r in rs[1:]:
            a, b = rs[0][f], r[f]
            same = all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, list) else np.array_equal(a, b)
            assert same, "%s differs between rank 0 and another rank" % f


def _geo(sc, rs):
    for r in rs:
        for k, v in sc.get("geo", {}).items():
            assert r["geometry"][k] == v, (sc["name"], k, r["geometry"])
        if "KP" in sc:
            assert r["geometry"]["KP"] == sc["KP"], r["geometry"]


def _kinds(sc, rs, keys):
    for r in rs:
        for key in keys:
            kind = set(r[key])
            want = set(sc.get("expect", ()))
            if key == "kind1":
                want -= {"ll_cells", "ll_join"}        # a handle's first pass evaluates no ll (it lags one pass): no ll blocks, nothing to hand over
            assert want <= kind and not (set(sc.get("not_expect", ())) & kind), (sc["name"], key, sorted(kind))


def _tokens(x):
    return int(sum(np.asarray(y).reshape(-1, 2)[:, 1].sum() for y in x)) if isinstance(x, (list, tuple)) else int(np.asarray(x).reshape(-1, 2)[:, 1].sum())


def _shards(out, sc, rs, X):
    b = [r["shard"] for r in rs]
    assert b[0][0] == 0 and b[-1][1] == sc["D"] and all(b[i][1] == b[i + 1][0] for i in range(len(b) - 1)), b
    if sc["D"] == 41:          # the edges, as every group cuts them: (documents, tokens > 0) per rank
        N = [sum(_tokens(x) for x in X[d0:d1]) for d0, d1 in b]
        got = [(d1 - d0, n > 0) for (d0, d1), n in zip(b, N)]
        want = {2: [(41, True), (0, False)], 3: [(0, False), (40, True), (1, True)], 4: [(20, True), (0, False), (4, False), (17, True)]}[out["world"]]
        assert got == want, (sc["name"], got)
        assert sum(1 for n in N if n > 0) >= 2 or out["world"] == 2      # more than one rank contributes to every sum
    return b


# ------------------------------------------------------------------------------------------------------------------- LDA
def _lda_passes(out, sc):
    rs = _ranks(out, sc["name"])
    _geo(sc, rs); _kinds(sc, rs, ("kind1", "kind3"))
    if "moved" in sc:
        assert all(r["geometry"]["prologue_moved"] == sc["moved"] for r in rs), [r["geometry"] for r in rs]
    if "join" in sc:
        assert tuple("ll_join" in r["kind3"] for r in rs) == tuple(sc["join"]), [r["kind3"] for r in rs]
    _same_bits(rs, ("lam1", "Elnbeta1", "beta1", "lam3", "Elnbeta3", "beta3", "ll"))
    X, ref = _cached(("lda", sc["name"]), lambda: S.lda_reference(sc))
    b = _shards(out, sc, rs, X)
    # the harness's restatement of the launch that waits (sharded_ref.merged_blocks, which check_residency sums) against the device's own count
    for r, (d0, d1) in zip(rs, b):
        want = S.merged_blocks(sc, d1 - d0)
        assert (r["blocks3"] > 0) == (want > 0) and r["blocks3"] <= want and r["blocks1"] <= want, (sc["name"], r["blocks1"], r["blocks3"], want)
        if sc.get("packed") or "packed" in sc.get("not_expect", ()) or not ({"merged"} & set(r["kind3"])):
            assert r["blocks3"] == want, (sc["name"], r["blocks3"], want)
    r0 = rs[0]
    assert len(r0["ll"]) == 3
    n = S.sum_roundings(X, sc["V"], out["world"])
    w = {}
    for tag, p, tol in (("1", 0, ONE), ("3", 2, RUN)):
        w["λ" + tag] = dist(r0["lam" + tag], ref[p]["lam"]); w["β" + tag] = dist(r0["beta" + tag], ref[p]["beta"])
        w["Elnβ" + tag] = dist(r0["Elnbeta" + tag], ref[p]["Elnbeta"], atol=1e-13)
        w["γ" + tag] = max([dist(r["gamma" + tag], ref[p]["gamma"][:, d0:d1]) for r, (d0, d1) in zip(rs, b) if d1 > d0] or [0.0])
        w["ll" + tag] = dist(r0["ll"][p], ref[p]["ll"])
        for k in ("λ", "β", "Elnβ", "γ", "ll"):
            assert w[k + tag] <= tol, "%s: %s after pass %s is %.3g from the reference (bound %g)" % (sc["name"], k, tag, w[k + tag], tol)
    # the all-reduced statistics of pass 1, Σ_d n_dv ϕ_dvk: a sum of non-negative terms, so its error is at most (γ_n + the relative error of
    # a ϕ) x its value -- n from the kernels (sharded_ref.sum_roundings), ϕ's roundings from elbo_ref.phi_roundings at the constructor state
    import elbo_ref as R
    from scipy.special import digamma as psi
    _, lam0 = S.lda_corpus(sc)
    Eb0 = psi(lam0) - psi(lam0.sum(axis=0, keepdims=True)); Et0 = psi(1.0) - psi(float(sc["K"]))
    nphi = R.phi_roundings(np.array([Et0]), Eb0, sc["K"])
    stat = ref[0]["lam"] - S.ETA
    room = (S.gam(n)[:, None] + S.gam(nphi)) * stat + 4 * np.spacing(ref[0]["lam"])
    ratio = float((np.abs(r0["lam1"] - ref[0]["lam"]) / room).max())
    print("\n%-22s %s   statistics of pass 1: %.2f of (γ_n + γ_ϕ) Σ, n up to %d, ϕ %d roundings" % (
        sc["name"], " ".join("%s %.1e" % kv for kv in w.items()), ratio, n.max(), nphi))
    assert ratio <= 1.0, (sc["name"], ratio)
    return rs


@pytest.mark.parametrize("name", _names(2, ("lda_passes",)))
def test_two_ranks_lda_passes(world2, name):
    _lda_passes(world2, _sc(2, name))


@pytest.mark.parametrize("name", _names(3, ("lda_passes",)))
def test_three_ranks_lda_passes(world3, name):
    _lda_passes(world3, _sc(3, name))


@pytest.mark.parametrize("name", _names(4, ("lda_passes",)))
def test_four_ranks_lda_passes(world4, name):
    _lda_passes(world4, _sc(4, name))


def test_every_padded_topic_count_ran_folded():
    assert sorted({sc["KP"] for sc in SWEEP}) == list(S.KPS)
    assert all(S.merged_blocks(sc, 37) > 0 for sc in SWEEP)


def _lda_fit(out, sc, stops):
    rs = _ranks(out, sc["name"])
    _kinds(sc, rs, ("kind",))
    _same_bits(rs, ("ll", "lam", "beta", "converged", "elbo"))
    r0, p = rs[0], out["plain"][sc["name"]]
    n = len(r0["ll"])
    assert n == len(p["ll"]) and r0["converged"] == p["converged"], (n, len(p["ll"]))
    if stops:
        # the rule fired on the device inside an enqueued chunk (12 passes, then 8 at a time): at least one no-op pass followed it
        assert r0["converged"] and 10 < n < sc["maxiter"] and (n + 1) not in (12, 20, 28, 36), n
    else:
        assert n == sc["maxiter"] and not r0["converged"]
    np.testing.assert_allclose(r0["ll"], p["ll"], rtol=1e-11)
    np.testing.assert_allclose(r0["beta"], p["beta"], rtol=1e-9)
    np.testing.assert_allclose(r0["elbo"], p["elbo"], rtol=1e-10)
    X, ref = _cached(("lda", sc["name"]), lambda: S.lda_reference(sc, passes=n))
    np.testing.assert_allclose(r0["ll"], [r["ll"] for r in ref], rtol=RUN)
    np.testing.assert_allclose(r0["lam"], ref[-1]["lam"], rtol=1e-5)
    print("\n%-22s %d passes, ll %.1e from the unsharded fit, %.1e from the reference" % (
        sc["name"], n, dist(r0["ll"], p["ll"]), dist(r0["ll"], [r["ll"] for r in ref])))


@pytest.mark.parametrize("name", ["stop_folded", "stop_split", "stop_unfolded"])
def test_stopping_rule_inside_a_chunk(world3, name):
    _lda_fit(world3, _sc(3, name), stops=True)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_known_fit_after_everything_else(groups, world):
    """the last scenario of every group: the context is still usable and its sequence numbers line up"""
    assert TABLES[world][-1] is KNOWN
    _lda_fit(groups(world), KNOWN, stops=False)


def test_payload_above_the_mailbox_fails_alike_and_at_once(world3):
    sc = _sc(3, "payload_8257")
    rs = _ranks(world3, sc["name"])
    _geo(sc, rs)
    for r in rs:
        assert S.NO_RCCL in r["error"], r["error"]
        assert r["seconds"] < 5.0, "the refusal took %.1f s: some rank waited" % r["seconds"]
    order = [s["name"] for s in WORLD3]
    assert order.index("after_overflow") == order.index("payload_8257") + 1        # ... and the next model on the context fits (its own test)


@pytest.mark.parametrize("world", [3, 4])
def test_stage_api_on_every_rank(groups, world):
    import elbo_ref as R
    import np_ref
    out = groups(world)
    sc = _sc(world, "stage_api")
    rs = _ranks(out, sc["name"])
    X, lam0 = S.lda_corpus(sc)
    b = _shards(out, sc, rs, X)
    _same_bits(rs, ("lam", "Elnbeta", "beta", "ll", "elbo", "terms"))
    K, V, D = sc["K"], sc["V"], sc["D"]
    ref = np_ref.lda_iteration(X, K, S.ALPHA, S.ETA, lam0, [np.full((K, x.shape[0]), 1.0 / K) for x in X])
    gamma = np.concatenate([r["gamma"] for r in rs], axis=1); Elntheta = np.concatenate([r["Elntheta"] for r in rs], axis=1)
    phi = np.concatenate([r["phi"] for r in rs], axis=0)
    r0 = rs[0]
    w = {"γ": dist(gamma, ref["gamma"]), "Elnθ": dist(Elntheta, ref["Elntheta"], atol=1e-13), "λ": dist(r0["lam"], ref["lam"]),
         "Elnβ": dist(r0["Elnbeta"], ref["Elnbeta"], atol=1e-13), "β": dist(r0["beta"], ref["beta"]), "ll": dist(r0["ll"], ref["ll"]),
         "ϕ": dist(phi, np.concatenate([p.T for p in ref["phi"]], axis=0), atol=1e-300)}
    print("\nstage API, %d ranks: %s" % (world, " ".join("%s %.1e" % kv for kv in w.items())))
    assert max(w.values()) <= ONE, w
    # the ELBO of the state the ranks hold together, term by term
    st = dict(K=K, V=V, D=D, alpha=S.ALPHA, eta=S.ETA, X=X, lam=r0["lam"], Elnbeta=r0["Elnbeta"], gamma=gamma, Elntheta=Elntheta, phi=phi, features=None)
    t = R.lda_terms(st)
    n = R.lda_roundings(K, V, max(d1 - d0 for d0, d1 in b), max(x.shape[0] for x in X)) + world
    ratio = R.ratios(r0["terms"], t, n)
    print("ELBO terms in units of the bound: %s" % " ".join("%s %.3f" % kv for kv in zip(R.LDA_TERMS, ratio)))
    assert np.all(ratio <= 1.0), ratio
    assert r0["elbo"] == r0["terms"][0] + r0["terms"][1] + r0["terms"][2] + r0["terms"][3] - r0["terms"][4] - r0["terms"][5] - r0["terms"][6]


def test_frozen_topic_inference_on_a_sharded_corpus(world3):
    import lda_infer_ref as I
    sc = _sc(3, "infer")
    rs = _ranks(world3, sc["name"])
    X, _ = S.lda_corpus(sc)
    b = _shards(world3, sc, rs, X)
    tp = rs[0]["topics"]
    for r in rs[1:]:
        assert all(np.array_equal(r["topics"][k], tp[k]) for k in tp)
    for tag, unsmoothed in (("heldout", 0), ("transform", 1)):
        _same_bits(rs, (tag + "_ll", tag + "_converged"))
        ref = I.infer(X, sc["K"], S.ALPHA, tp["beta"], tp["Elnbeta"], tp["lam"], unsmoothed, sc["maxiter"], sc["tol"])
        ll = rs[0][tag + "_ll"]
        assert len(ll) == len(ref.ll) and rs[0][tag + "_converged"] == ref.converged and 10 < len(ll) < sc["maxiter"], (len(ll), len(ref.ll))
        w = {"ll": dist(ll, ref.ll)}
        w["θ"] = max(dist(r[tag + "_theta"], ref.theta[:, d0:d1]) for r, (d0, d1) in zip(rs, b) if d1 > d0)
        w["γ"] = max(dist(r[tag + "_gamma"], ref.gamma[:, d0:d1]) for r, (d0, d1) in zip(rs, b) if d1 > d0)
        print("\n%s on three ranks, %d passes: %s" % (tag, len(ll), " ".join("%s %.1e" % kv for kv in w.items())))
        assert w["ll"] <= 1e-10 and w["θ"] <= 1e-9 and w["γ"] <= 1e-9, w           # the bounds of test_lda_infer_dispatch_gpu.py


# ------------------------------------------------------------------------------------------------------------------ ILDA
def _ilda(out, sc):
    import ilda_ref
    import elbo_ref as R
    rs = _ranks(out, sc["name"])
    c = S.ilda_case(sc)
    b = _shards(out, sc, rs, c["X"])
    for r in rs:
        for key in ("kind1", "kind3"):      # the split launches, never merged and never folded under a communicator
            assert "split" in r[key] and not ({"merged", "p2p", "wide"} & set(r[key])), (key, r[key])
    _same_bits(rs, ("lam1", "Elnbeta1", "beta1", "lam3", "Elnbeta3", "beta3", "ll", "elbo", "terms"))
    assert (sum(c["J"]) <= 16) == (sum(sc["J"]) <= 16) and c["J"] == sc["J"]
    m = ilda_ref.model_of(c)
    r0, w = rs[0], {}
    ll = []
    for p in range(3):
        ll.append(m.one_pass())
        if p in (0, 2):
            tag = str(p + 1)
            for i in range(m.I):
                w["λ" + tag] = max(w.get("λ" + tag, 0.0), dist(r0["lam" + tag][i], m.lam[i])); w["β" + tag] = max(w.get("β" + tag, 0.0), dist(r0["beta" + tag][i], m.beta[i]))
                w["Elnβ" + tag] = max(w.get("Elnβ" + tag, 0.0), dist(r0["Elnbeta" + tag][i], m.Elnbeta[i], atol=1e-13))
            w["γ" + tag] = max([dist(r["gamma" + tag], m.gamma[:, d0:d1]) for r, (d0, d1) in zip(rs, b) if d1 > d0] or [0.0])
            if p == 0:
                # the all-reduced statistics folded onto the feature values, λ_i - η_i: sums of non-negative terms n ϕ, held to (γ_n + γ_ϕ) x value
                n, nphi = S.ilda_stat_pass1(c, out["world"])
                ratio = 0.0
                for i in range(m.I):
                    room = (S.gam(n[i])[:, None] + S.gam(nphi)) * (m.lam[i] - c["eta"][i]) + 4 * np.spacing(m.lam[i])
                    ratio = max(ratio, float((np.abs(r0["lam1"][i] - m.lam[i]) / room).max()))
    w["ll"] = dist(r0["ll"], ll)
    e, t = m.elbo_terms()
    w["ELBO"] = dist(r0["elbo"], e)
    # the seven terms against elbo_ref on the state the ranks hold together after the third pass, test_elbo_gpu.py's bound + one rounding per rank
    st = dict(K=c["K"], V=c["V"], D=c["D"], alpha=c["alpha"], eta=np.asarray(c["eta"], dtype=np.float64), X=c["X"], features=c["features"],
              lam=r0["lam3"], Elnbeta=r0["Elnbeta3"], gamma=np.concatenate([r["gamma3"] for r in rs], axis=1),
              Elntheta=np.concatenate([r["Elntheta3"] for r in rs], axis=1), phi=np.concatenate([r["phi3"] for r in rs], axis=0))
    nr = R.lda_roundings(c["K"], c["V"], max(d1 - d0 for d0, d1 in b), max(x.shape[0] for x in c["X"]), I=len(c["J"]), Jmax=max(c["J"])) + out["world"]
    tr = R.ratios(r0["terms"], R.lda_terms(st), nr)
    print("\n%-16s %s   statistics of pass 1: %.2f of (γ_n + γ_ϕ) Σ; ELBO terms / bound: %s" % (
        sc["name"], " ".join("%s %.1e" % kv for kv in w.items()), ratio, " ".join("%.3f" % x for x in tr)))
    for k, v in w.items():
        assert v <= (RUN_ELN if k.startswith("Elnβ") else RUN), (sc["name"], k, v)
    assert ratio <= 1.0, (sc["name"], ratio)
    assert np.all(tr <= 1.0), (sc["name"], tr)
    assert r0["elbo"] == r0["terms"][0] + r0["terms"][1] + r0["terms"][2] + r0["terms"][3] - r0["terms"][4] - r0["terms"][5] - r0["terms"][6]
    if sc.get("tol"):
        _same_bits(rs, ("fit_ll", "fit_lam", "fit_converged", "fit_elbo"))
        p = out["plain"][sc["name"]]
        n = len(r0["fit_ll"])
        assert n == len(p["fit_ll"]) and r0["fit_converged"] == p["fit_converged"] and r0["fit_converged"] and 10 < n < sc["maxiter"], (n, len(p["fit_ll"]))
        np.testing.assert_allclose(r0["fit_ll"], p["fit_ll"], rtol=1e-11)
        np.testing.assert_allclose(r0["fit_elbo"], p["fit_elbo"], rtol=1e-10)


@pytest.mark.parametrize("name", _names(3, ("ilda",)))
def test_three_ranks_ilda(world3, name):
    _ilda(world3, _sc(3, name))


@pytest.mark.parametrize("world", [2, 4])
def test_ilda_shard_edges(groups, world):
    _ilda(groups(world), _sc(world, "edge_ilda"))


# ------------------------------------------------------------------------------------------------------------------- CTM
def _ctm(out, sc, oracle):
    rs = _ranks(out, sc["name"])
    X, g0f, feats = S.ctm_corpus(sc)
    b = _shards(out, sc, rs, X)
    if sc["D"] == 41 and out["world"] == 4:      # one modality empty on a whole rank, the other not
        assert _tokens([x[1] for x in X[b[3][0]:b[3][1]]]) == 0 and _tokens([x[0] for x in X[b[3][0]:b[3][1]]]) > 0
    _geo(sc, rs)
    glob = ["mu", "Sigma", "invSigma", "gamma", "Elnphi", "alpha"]
    _same_bits(rs, [f + t for f in glob for t in (("1",) if sc["kind"] == "ctm_stage" else ("1", "3"))] + ["ll", "elbo", "terms"])
    K, M, MK, D = sc["K"], len(sc["K"]), sum(sc["K"]), sc["D"]
    flags = sc.get("flags", 1)
    sigma, auto = bool(flags & 1) or feats is not None, bool(flags & 2)
    o = oracle.CtmOracle(K, sc["alpha"], X, V=None if feats is not None else sc["V"], features=feats, gamma0=g0f)
    r0, w, ll = rs[0], {}, []
    stage = sc["kind"] == "ctm_stage"
    for n, tag in (((1, "1"),) if stage else ((1, "1"), (2, "3"))):
        ll.append(o.fit(maxiter=n, tol=0.0, update_sigma=sigma, auto_alpha=auto))
        lam = np.concatenate([r["lambda" + tag].reshape(-1, MK) for r in rs]); nu = np.concatenate([r["nu" + tag].reshape(-1, MK) for r in rs])
        assert lam.shape == (D, MK)
        w["γ" + tag] = dist(r0["gamma" + tag], o.gamma)
        w["μ" + tag] = dist(r0["mu" + tag], o.mu, atol=1e-7)
        w["Σ" + tag] = dist(r0["Sigma" + tag], o.Sigma, atol=1e-7)
        w["λ" + tag] = float(np.median(np.abs(lam - o.lam.reshape(D, MK)).max(axis=1)))
        for k in ("γ", "μ", "Σ"):
            assert w[k + tag] <= 1e-5, (sc["name"], k + tag, w)
        assert w["λ" + tag] <= 1e-7, w              # (test_ctm_gpu.py _robust_close: most documents' solves land within 1e-7)
        if auto:
            w["α" + tag] = dist(r0["alpha" + tag], o.alpha)
            assert w["α" + tag] <= 1e-3, w          # (test_fit_autoalpha_matches_oracle)
        # update_props! (MMCTM.jl:145-154) of the λ every rank holds: the softmax per modality, at the stage test's bound
        props = np.concatenate([r["props" + tag].reshape(-1, MK) for r in rs])
        want, off = np.empty_like(props), 0
        for k in K:
            e = np.exp(lam[:, off:off + k].astype(np.longdouble) - lam[:, off:off + k].max(axis=1, keepdims=True))
            want[:, off:off + k] = (e / e.sum(axis=1, keepdims=True)).astype(np.float64); off += k
        w["props|λ" + tag] = dist(props, want)
        assert w["props|λ" + tag] <= 1e-11, w
        # the Gaussian M-step from the λ, ν all ranks hold together: the mean and the covariance over the GLOBAL D documents
        LD = np.longdouble
        mu = lam.astype(LD).sum(axis=0) / LD(D)
        w["μ|λ" + tag] = dist(r0["mu" + tag], mu.astype(np.float64), atol=1e-14)
        assert w["μ|λ" + tag] <= 1e-11, w
        if sigma:
            df = lam.astype(LD) - mu[None, :]
            Sg = (np.diag(nu.astype(LD).sum(axis=0)) + df.T @ df) / LD(D)
            w["Σ|λν" + tag] = dist(r0["Sigma" + tag].reshape(MK, MK), Sg.astype(np.float64), atol=1e-12)
            prod = r0["Sigma" + tag].reshape(MK, MK) @ r0["invSigma" + tag].reshape(MK, MK)
            w["ΣΣ⁻¹" + tag] = float(np.abs(prod - np.eye(MK)).max())
            assert w["Σ|λν" + tag] <= 1e-9 and w["ΣΣ⁻¹" + tag] <= 1e-8, w
        else:
            assert np.array_equal(r0["Sigma" + tag].reshape(MK, MK), np.eye(MK))
    # the γ sums of the first pass (all-reduced inside the statistics): sums of non-negative terms n θ with θ = softmax Elnϕ₀, free of the
    # LD_MMA solves -- in np.longdouble from γ0 and the full corpus, held to (γ_n + γ_θ) x value with a floor of 4 units in the last place
    val, stat, n, nth = S.ctm_gamma_pass1(sc, X, g0f, feats, out["world"])
    room = (S.gam(n) + S.gam(nth)) * stat.astype(np.float64) + 4 * np.spacing(val.astype(np.float64))
    w["γ₁/bound"] = float((np.abs(r0["gamma1"].astype(np.longdouble) - val).astype(np.float64) / room).max())
    assert w["γ₁/bound"] <= 1.0, (sc["name"], w["γ₁/bound"])
    # the seven ELBO terms against elbo_ref on the state the ranks hold together (globals of rank 0; λ, ν, ζ and the θ the ELBO was formed
    # from, rank after rank), test_elbo_gpu.py's bound with one more rounding per rank
    import elbo_ref as R
    last = "1" if stage else "3"
    lay = R.CtmLayout(K, sc["V"], X, features=feats)
    theta = np.concatenate([r["theta"][int(sum(k * sum(np.asarray(x[j]).reshape(-1, 2).shape[0] for x in X[d0:d1]) for j, k in enumerate(K[:m]))):][
        :K[m] * sum(np.asarray(x[m]).reshape(-1, 2).shape[0] for x in X[d0:d1])] for m in range(M) for r, (d0, d1) in zip(rs, b)])
    st = dict(alpha=r0["alpha" + last], mu=r0["mu" + last], invSigma=r0["invSigma" + last].reshape(MK, MK), gamma=r0["gamma" + last],
              Elnphi=r0["Elnphi" + last], lam=lam, nu=nu, zeta=np.concatenate([r["zeta" + last].reshape(-1, M) for r in rs]), theta=theta)
    tr = R.ratios(r0["terms"], R.ctm_terms(lay, st), R.ctm_roundings(lay) + out["world"])
    w["terms/bound"] = float(tr.max())
    assert np.all(tr <= 1.0), (sc["name"], tr)
    assert r0["elbo"] == r0["terms"][0] + r0["terms"][1] + r0["terms"][2] + r0["terms"][3] - r0["terms"][4] - r0["terms"][5] - r0["terms"][6]
    ll_o = np.concatenate(ll)
    assert r0["ll"].shape == ll_o.shape == ((1 if stage else 3), M)
    w["ll"] = dist(r0["ll"], ll_o)
    w["ELBO"] = dist(r0["elbo"], o.elbo()[0])
    print("\n%-18s %s" % (sc["name"], " ".join("%s %.1e" % kv for kv in w.items())))
    assert w["ll"] <= 1e-6 and w["ELBO"] <= 1e-5, w


@pytest.mark.parametrize("name", _names(3, ("ctm", "ctm_stage")))
def test_three_ranks_ctm(world3, oracle, name):
    _ctm(world3, _sc(3, name), oracle)


def _heldout_oracle(oracle, sc, topics, Xn, g0f, tag, flags):
    """The index-order oracle's inference of the FULL held-out corpus under the globals the ranks loaded (tests/test_inference_gpu.py); what
    transform does not load stays the constructor's, from the γ0 the ranks were given."""
    on = oracle.CtmOracle(sc["K"], sc["alpha"], Xn, V=sc["V"], gamma0=g0f)
    if tag == "heldout":                                                    # MMCTM.jl:558-563
        on.mu[:] = topics["mu"]; on.Sigma[:] = topics["Sigma"]; on.invSigma[:] = topics["invSigma"]
        on.gamma[:] = topics["gamma"]; on.Elnphi[:] = topics["Elnphi"]; on.phi[:] = topics["phi"]
    else:                                                                   # MMCTM.jl:516-521: invΣ stays the identity
        on.phi[:] = topics["phi"]
        if not flags & 2:
            on.mu[:] = topics["mu"]; on.Sigma[:] = topics["Sigma"]
    return on, on.infer(flags, sc["maxiter"], 0.0)


def test_ctm_heldout_on_a_sharded_corpus(world3, oracle):
    """N_m and D are global at create time: the ll rows are the full corpus's, Σ of fit_gaussian divides by all 60 documents."""
    sc = _sc(3, "mmctm_heldout")
    rs = _ranks(world3, sc["name"])
    Xn, g0f, _ = S.ctm_corpus(sc)
    _shards(world3, sc, rs, Xn)
    D, MK = sc["D"], sum(sc["K"])
    tp, plain = rs[0]["topics"], world3["plain"][sc["name"]]
    for r in rs[1:]:
        assert all(np.array_equal(r["topics"][k], tp[k]) for k in tp)
    LD = np.longdouble
    for tag, flags in S.HELDOUT_MODES:
        _same_bits(rs, [tag + "_" + f for f in ("ll", "mu", "Sigma", "invSigma", "elbo")])
        on, ll_o = _heldout_oracle(oracle, sc, tp, Xn, g0f, tag, flags)
        r0 = rs[0]
        lam = np.concatenate([r[tag + "_lambda"].reshape(-1, MK) for r in rs]); nu = np.concatenate([r[tag + "_nu"].reshape(-1, MK) for r in rs])
        w = {"ll₁": dist(r0[tag + "_ll"][0], ll_o[0]), "ll": dist(r0[tag + "_ll"], ll_o), "ll|unsharded": dist(r0[tag + "_ll"], plain[tag + "_ll"]),
             "λ|unsharded": float(np.abs(lam - plain[tag + "_lambda"].reshape(D, MK)).max()), "ELBO": dist(r0[tag + "_elbo"], on.elbo()[0]), "ELBO|unsharded": dist(r0[tag + "_elbo"], plain[tag + "_elbo"])}
        assert r0[tag + "_ll"].shape == ll_o.shape == (sc["maxiter"], len(sc["K"]))
        assert w["ll₁"] <= 1e-6 and w["ll"] <= 1e-5 and w["ll|unsharded"] <= 1e-5 and w["ELBO"] <= 1e-5 and w["ELBO|unsharded"] <= 1e-5, (tag, w)    # test_inference_gpu.py's bounds
        if flags & 2:
            mu = lam.astype(LD).sum(axis=0) / LD(D)
            df = lam.astype(LD) - mu[None, :]
            Sg = (np.diag(nu.astype(LD).sum(axis=0)) + df.T @ df) / LD(D)
            w["μ|λ"] = dist(r0[tag + "_mu"], mu.astype(np.float64), atol=1e-14)
            w["Σ|λν"] = dist(r0[tag + "_Sigma"].reshape(MK, MK), Sg.astype(np.float64), atol=1e-12)
            assert w["μ|λ"] <= 1e-11 and w["Σ|λν"] <= 1e-9, (tag, w)
        else:
            assert np.array_equal(r0[tag + "_mu"], tp["mu"]) and np.array_equal(r0[tag + "_Sigma"], tp["Sigma"])
        print("\n%-16s %s" % (tag, " ".join("%s %.1e" % kv for kv in w.items())))


def test_ctm_batch_on_a_communicating_context(world3):
    """mmm_ctm_create_batch takes a communicator: each replica must be, bit for bit, the sharded single fit of its γ0 (the contract of
    test_ctm_batch_gpu.py), on every rank."""
    sc = _sc(3, "mmctm_batch")
    rs = _ranks(world3, sc["name"])
    iters = []
    for r in range(sc["R"]):
        for rk in rs:
            assert not rk["error"], rk["error"]
            b, s1 = rk["batch%d" % r], rk["single%d" % r]
            for f in S.BATCH_FIELDS + ("ll", "elbo", "converged"):
                assert np.array_equal(b[f], s1[f]), "restart %d, field %s: the batch differs from the single fit" % (r, f)
        for f in ("mu", "Sigma", "gamma", "ll", "elbo"):
            assert all(np.array_equal(rk["batch%d" % r][f], rs[0]["batch%d" % r][f]) for rk in rs), (r, f)
        iters.append(len(rs[0]["batch%d" % r]["ll"]))
    print("\nbatch of %d on three ranks: %s passes" % (sc["R"], iters))
    assert all(10 < n <= sc["maxiter"] for n in iters)


def test_ctm_batch_beyond_the_mailbox_fails_alike_and_at_once(world3):
    sc = _sc(3, "mmctm_batch_overflow")
    MK, GT = sum(sc["K"]), sum(k * v for k, v in zip(sc["K"], sc["V"]))
    assert (sc["R"] - 1) * (2 * MK + MK * MK + GT + 16) <= S.P2P_CAP < sc["R"] * (2 * MK + MK * MK + GT + 16)
    for r in _ranks(world3, sc["name"]):
        assert S.NO_RCCL in r["error"], r["error"]
        assert r["seconds"] < 5.0, "the refusal took %.1f s: some rank waited" % r["seconds"]
    order = [s["name"] for s in WORLD3]
    assert order.index("mmctm_after_overflow") == order.index("mmctm_batch_overflow") + 1


@pytest.mark.parametrize("world", [2, 4])
def test_mmctm_shard_edges(groups, oracle, world):
    _ctm(groups(world), _sc(world, "edge_mmctm"), oracle)


# --------------------------------------------------------------------------------------------------------------- the harness
def test_groups_fit_one_card_and_end_with_the_known_fit():
    for world, table in TABLES.items():
        names = [sc["name"] for sc in table]
        assert len(set(names)) == len(names) and table[-1] is KNOWN
        blocks = S.check_residency(world, table, {41: EDGE_BOUNDS[world]})
        assert max(blocks.values()) <= S.CU_BUDGET
    assert {tuple(b) for b in EDGE_BOUNDS.values()} == {(0, 41, 41), (0, 0, 40, 41), (0, 20, 20, 24, 41)}
