"""Harness and references of tests/test_sharded_gpu.py: several ranks on ONE card, each a process with its own context on device 0 and the
xGMI mailboxes between them (Context.init_p2p over gloo), run the same ordered list of named scenarios on their shards of a corpus; the
parent compares what every rank returns with an independent restatement evaluated on the FULL corpus (np_ref for LDA, ilda_ref for ILDA,
the index-order C oracle for MMCTM / IMMCTM, elbo_ref for the ELBO terms).

A scenario is a plain dict (it is pickled to the ranks): `kind` names the function below that runs it, `name` the key of its results.
Shards come from `bounds` (documents [bounds[r], bounds[r + 1]) on rank r) or, without it, from `shard_documents`.

One card is one set of compute units.  The launch that folds the exchange into the LDA reduction (k_lda_reduce_ll_mstep) is made of blocks
of 1,024 threads that wait for each other AND for the peers' blocks, one block per CU (its 126 VGPRs allow no second one); the library
sizes it for a device of its own (residency_cap), so on one card the ranks' launches together must fit the 256 CUs.  `merged_blocks` is that
arithmetic; `check_residency` refuses a scenario list that would not fit before anything is spawned."""
import ctypes as C
import datetime
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, ETA = 0.1, 0.1
CUS = 256                     # compute units of the card
CU_BUDGET = 232               # ... of which the ranks' waiting launches may hold this many together
P2P_CAP = 8192                # doubles per mailbox call (csrc/mmm_internal.h kP2PCap)
KPS = (2, 4, 6, 8, 10, 12, 16, 20, 24, 32)
NO_RCCL = "no RCCL communicator"
EMPTY = np.zeros((0, 2), dtype=np.int64)


def pick_kp(K):
    return next((o for o in KPS if K <= o), (K + 1) & ~1)


# ------------------------------------------------------------------------------------------------------------------ corpora
def lda_corpus(sc):
    """(X, λ0) of an LDA scenario: np_ref.synth_lda, the documents listed in `empty` (and, of a 41-document corpus, documents 20 .. 23) emptied."""
    import np_ref
    X, lam0 = np_ref.synth_lda(sc["D"], sc["V"], sc["K"], seed=sc.get("seed", 5), mean_n=sc.get("mean_n", 300))
    for d in edge_empty(sc):
        X[d] = EMPTY
    return X, lam0


def edge_empty(sc):
    """Documents without a token: those the scenario lists; of the edge corpora (D = 41) documents 20 .. 23, which the four-rank bounds give
    to one rank alone.  Document 40, the only one of the last rank of [0, 0, 40, 41], carries tokens."""
    return tuple(sc.get("empty", ())) + ((20, 21, 22, 23) if sc["D"] == 41 else ())


def ilda_case(sc):
    """An ilda_ref case dict: feature table `J` over V terms (random_table), corpus, λ0."""
    import ilda_ref
    rng = np.random.Generator(np.random.PCG64([20261020, sc.get("seed", 1)]))
    c = ilda_ref._case(rng, sc["name"], ilda_ref.random_table(rng, sc["V"], sc["J"]), sc["K"], sc["D"], sc.get("mean_n", 200), eta=sc["eta"])
    for d in edge_empty(sc):
        c["X"][d] = EMPTY
    return c


SNV3 = np.array([[t // 16 + 1, (t // 4) % 4 + 1, t % 4 + 1] for t in range(96)])


def ctm_corpus(sc):
    """(X, γ0 flat, features or None) of a CTM scenario.  `imm`: one modality over the 96 SNV terms, factorised into `imm` features."""
    import np_ref
    X, g0 = np_ref.synth_mm(sc["D"], sc["V"], sc["K"], seed=sc.get("seed", 4), means=sc["means"], empty_frac=sc.get("empty_frac", 0.1))
    M = len(sc["K"])
    for d in edge_empty(sc):
        X[d] = [EMPTY for _ in range(M)]
    for d0, d1, m in sc.get("empty_modality", ()):
        for d in range(d0, d1):
            X[d][m] = EMPTY
    feats = None
    if sc.get("imm"):
        feats = [SNV3[:, :sc["imm"]] if sc["imm"] > 1 else (SNV3[:, :1] - 1) * 16 + (SNV3[:, 1:2] - 1) * 4 + SNV3[:, 2:3]]
        GM = sum(sc["K"][m] * int(np.asarray(feats[m]).max(axis=0).sum()) for m in range(M))
        g0f = np.random.default_rng(sc.get("seed", 4)).integers(1, 101, size=GM).astype(np.float64)
    else:
        g0f = np.concatenate([g.ravel() for g in g0])
    return X, g0f, feats


def shard_of(sc, world, rank, X, override=None):
    """[d0, d1) of `rank`: the scenario's own bounds, else the call's bounds for a corpus of this many documents, else shard_documents."""
    b = sc.get("bounds") or (override or {}).get(len(X))
    if b is not None and not sc.get("balanced"):
        assert len(b) == world + 1 and b[0] == 0 and b[-1] == len(X) and all(b[i] <= b[i + 1] for i in range(world)), (sc["name"], b)
        return int(b[rank]), int(b[rank + 1])
    import mmm_pkg
    return mmm_pkg.load().shard_documents(X, world, rank)


# ----------------------------------------------------------------------------------------------------------- residency on one card
def merged_blocks(sc, Dloc):
    """Blocks of the merged reduce + ll + M-step launch of an LDA scenario on a rank with Dloc documents (csrc/lda.hip fused_passes): the
    reduce blocks (two logical ones per block when the scenario says `packed`) and the ll blocks, cut to the residency cap.  0: not merged."""
    t = sc.get("tuning", {})
    V, K = sc["V"], sc["K"]
    KP = pick_kp(K)
    if t.get("lda_build") == "wide" or KP > 32 or (KP >= 32 and t.get("lda_build", "auto") == "auto"):
        return 0
    unfolded = "p2p_folded" in t.get("disable", ())        # split launches whose reduce blocks wait for their own ll blocks' cells (k_lda_reduce_ll)
    if not unfolded and ("lda_merged" in t.get("disable", ()) or V > 256):
        return 0
    Vp = V if unfolded else (V + 15) & ~15
    nred = (Vp * K + 15) // 16
    cap = min(CUS - 4, t.get("resident_cap") or CUS)
    if cap < nred + 1:
        return 0
    L = 16 if KP <= 15 else (32 if KP <= 31 else 64)
    per_wave = 64 // L
    n_ll = max(1, min(-(-Dloc // per_wave), 512))
    nredp = nred // (2 if sc.get("packed") else 1)
    return nredp + min(n_ll, cap - nredp)


def check_residency(world, scenarios, bounds=None):
    """Every LDA scenario's waiting launches of all ranks together within CU_BUDGET; returns {name: blocks}."""
    out = {}
    for sc in scenarios:
        if not sc["kind"].startswith("lda"):
            continue
        D = sc["D"]
        b = sc.get("bounds") or (bounds or {}).get(D)
        sizes = [b[r + 1] - b[r] for r in range(world)] if b is not None and not sc.get("balanced") else [-(-D // world) + 8] * world
        tot = sum(merged_blocks(sc, n) for n in sizes)
        assert tot <= CU_BUDGET, "%s: %d blocks of %d ranks wait for each other on a card of %d CUs" % (sc["name"], tot, world, CUS)
        out[sc["name"]] = tot
    return out


# ------------------------------------------------------------------------------------------------------------------- the ranks
def _ll_history(pkg, g, n=64):
    buf = np.zeros(n * getattr(g, "M", 1)); cnt = C.c_int()
    fn = pkg.lib().mmm_lda_ll_history if isinstance(g, pkg.LDA) else pkg.lib().mmm_ctm_ll_history
    pkg._lib.check(fn(g._h, buf.ctypes.data, n, C.byref(cnt)), g.ctx.h, "ll_history")
    return buf[:cnt.value * getattr(g, "M", 1)].copy()


def _iterate(pkg, g, n, flags=1):
    if isinstance(g, pkg.LDA):
        pkg._lib.check(pkg.lib().mmm_lda_iterate(g._h, n), g.ctx.h, "iterate")
    else:
        pkg._lib.check(pkg.lib().mmm_ctm_iterate(g._h, n, flags), g.ctx.h, "iterate")


def _lda_model(pkg, ctx, sc, X, lam0):
    ctx.set_tuning(**sc.get("tuning", {}))
    try:
        return pkg.LDA(sc["K"], ALPHA, ETA, sc["V"], X, λ0=lam0, ctx=ctx)
    finally:
        ctx.set_tuning()


def _lda_state(g, tag, out):
    out["lam" + tag] = g.λ; out["Elnbeta" + tag] = g.Elnβ; out["beta" + tag] = g.β; out["gamma" + tag] = g.γ
    out["kind" + tag] = sorted(g.last_pass()); out["blocks" + tag] = g.last_pass_blocks()


def run_lda_passes(pkg, ctx, sc, X, lam0):
    """iterate(1), then two more passes: the state after the first and after the third, the three ll values, what the launches were."""
    g = _lda_model(pkg, ctx, sc, X, lam0)
    out = {"geometry": g.geometry()}
    _iterate(pkg, g, 1); _lda_state(g, "1", out)
    _iterate(pkg, g, 2); _lda_state(g, "3", out)
    out["ll"] = _ll_history(pkg, g)
    out["geometry"] = g.geometry()
    g.close()
    return out


def run_lda_fit(pkg, ctx, sc, X, lam0):
    g = _lda_model(pkg, ctx, sc, X, lam0)
    ll = pkg.fit(g, maxiter=sc["maxiter"], tol=sc["tol"], verbose=False)
    out = {"ll": ll, "lam": g.λ, "beta": g.β, "converged": g.converged, "elbo": g.elbo, "kind": sorted(g.last_pass()), "geometry": g.geometry()}
    g.close()
    return out


def run_lda_overflow(pkg, ctx, sc, X, lam0):
    """A payload beyond the mailbox on a context without an RCCL communicator: the call that needs the exchange must fail at once."""
    g = _lda_model(pkg, ctx, sc, X, lam0)
    out = {"geometry": g.geometry(), "error": "", "seconds": 0.0}
    t0 = time.monotonic()
    try:
        _iterate(pkg, g, 1)
        g.λ
    except pkg.MmmError as e:
        out["error"] = str(e)
    out["seconds"] = time.monotonic() - t0
    ctx.synchronize()
    g.close()
    return out


def run_lda_stage(pkg, ctx, sc, X, lam0):
    """The reference's functions one at a time on every rank (from_sums all-reduces V K doubles, the ll one, the ELBO five)."""
    g = _lda_model(pkg, ctx, sc, X, lam0)
    out = {"geometry": g.geometry()}
    pkg.update_γ(g); out["gamma"] = g.γ; out["Elntheta"] = g.Elnθ
    pkg.update_ϕ(g); out["phi"] = g.phi_flat()
    pkg.update_λ(g); out["lam"] = g.λ
    pkg.update_Elnβ(g); out["Elnbeta"] = g.Elnβ
    pkg.update_β(g); out["beta"] = g.β
    pkg.update_θ(g)
    out["ll"] = pkg.calculate_loglikelihood(g)
    e, t = pkg.calculate_elbo(g, terms=True)
    out["elbo"] = e; out["terms"] = t
    g.close()
    return out


def run_lda_infer(pkg, ctx, sc, X, lam0, topics):
    """Frozen-topic inference of this rank's held-out documents under topics every rank loads: transform (unsmoothed) and fit_heldout."""
    out = {}
    for tag, unsmoothed in (("heldout", 0), ("transform", 1)):
        g = _lda_model(pkg, ctx, sc, X, lam0)
        g.λ = topics["lam"]; g.Elnβ = topics["Elnbeta"]; g.β = topics["beta"]
        ll = np.zeros(sc["maxiter"]); ni = C.c_int(); cv = C.c_int()
        pkg._lib.check(pkg.lib().mmm_lda_infer(g._h, unsmoothed, sc["maxiter"], sc["tol"], ll.ctypes.data, C.byref(ni), C.byref(cv)), ctx.h, "infer")
        out[tag + "_ll"] = ll[:ni.value].copy(); out[tag + "_converged"] = bool(cv.value)
        out[tag + "_theta"] = g.θ; out[tag + "_gamma"] = g.γ
        g.close()
    return out


def _ilda_factors(g, name):
    flat = g._get(name)
    return [flat[g._ioff[i]:g._ioff[i + 1]].reshape(g.J[i], g.K, order="F").copy() for i in range(g.I)]


def run_ilda(pkg, ctx, sc, c, d0, d1):
    def model():
        return pkg.ILDA(c["K"], c["alpha"], c["eta"], c["features"], c["X"][d0:d1], λ0=c["lam0"], ctx=ctx)
    out = {}
    g = model()
    out["geometry"] = g.geometry()
    for n, tag in ((1, "1"), (2, "3")):
        _iterate(pkg, g, n)
        out["lam" + tag] = _ilda_factors(g, "ilambda"); out["Elnbeta" + tag] = _ilda_factors(g, "iElnbeta"); out["beta" + tag] = _ilda_factors(g, "ibeta")
        out["gamma" + tag] = g.γ; out["kind" + tag] = sorted(g.last_pass())
    out["ll"] = _ll_history(pkg, g)
    e, t = pkg.calculate_elbo(g, terms=True)
    out["elbo"] = e; out["terms"] = t
    out["Elntheta3"] = g.Elnθ; out["phi3"] = g.phi_flat()          # the state the ELBO was formed from
    g.close()
    if sc.get("tol"):
        g = model()
        ll = pkg.fit(g, maxiter=sc["maxiter"], tol=sc["tol"], verbose=False)
        out.update(fit_ll=ll, fit_lam=_ilda_factors(g, "ilambda"), fit_converged=g.converged, fit_elbo=g.elbo)
        g.close()
    return out


def _ctm_model(pkg, ctx, sc, X, g0f, feats):
    ctx.set_tuning(**sc.get("tuning", {}))
    try:
        if feats is not None:
            return pkg.IMMCTM(sc["K"], sc["alpha"], feats, X, γ0=g0f, ctx=ctx)
        off = np.concatenate([[0], np.cumsum([k * v for k, v in zip(sc["K"], sc["V"])])])
        g0 = [g0f[off[m]:off[m + 1]].reshape(sc["K"][m], sc["V"][m]) for m in range(len(sc["K"]))]
        return pkg.MMCTM(sc["K"], sc["alpha"], sc["V"], X, γ0=g0, ctx=ctx)
    finally:
        ctx.set_tuning()


def _ctm_state(pkg, g, tag, out):
    for f in ("mu", "Sigma", "invSigma", "gamma", "Elnphi", "lambda", "nu", "zeta", "props", "alpha"):
        out[f + tag] = g._get(f)


def run_ctm(pkg, ctx, sc, X, g0f, feats):
    """One fused pass and two more (update_sigma as the scenario says): the global state and this rank's λ, ν, props after the first and
    the third, the per-modality ll rows, the ELBO."""
    g = _ctm_model(pkg, ctx, sc, X, g0f, feats)
    flags = sc.get("flags", 1)
    out = {"geometry": g.geometry()}
    _iterate(pkg, g, 1, flags); _ctm_state(pkg, g, "1", out)
    _iterate(pkg, g, 2, flags); _ctm_state(pkg, g, "3", out)
    out["ll"] = _ll_history(pkg, g).reshape(-1, g.M)
    e, t = pkg.calculate_elbo(g, terms=True)
    out["elbo"] = e; out["terms"] = t
    out["theta"] = g._get("theta")            # the θ the ELBO was formed from (rebuilt on demand after fused passes)
    g.close()
    return out


def run_ctm_stage(pkg, ctx, sc, X, g0f, feats):
    """fitdoc! on a document list (this rank's documents, last first, in one set of launches), then the M-step one reference function at a
    time: update_μ / update_Σ all-reduce the moments, update_γ the γ sums, the ll its numerators, the ELBO five sums."""
    g = _ctm_model(pkg, ctx, sc, X, g0f, feats)
    out = {"geometry": g.geometry()}
    docs = list(range(g.D))[::-1]
    if docs:
        pkg.fitdoc(g, docs)
    pkg.update_μ(g); pkg.update_Σ(g); pkg.update_γ(g); pkg.update_props(g)
    _ctm_state(pkg, g, "1", out)
    out["ll"] = pkg.calculate_loglikelihoods(g).reshape(1, -1)
    e, t = pkg.calculate_elbo(g, terms=True)
    out["elbo"] = e; out["terms"] = t
    out["theta"] = g._get("theta")
    g.close()
    return out


CTM_GLOBALS = ("mu", "Sigma", "invSigma", "gamma", "Elnphi", "phi")
HELDOUT_MODES = (("heldout", 0), ("transform", 1), ("transform_gauss", 3))          # MMM_INFER_UNSMOOTHED = 1, MMM_INFER_FIT_GAUSSIAN = 2


def ctm_train(pkg, ctx, sc):
    """The trained globals every rank loads: four passes on the training corpus on a context that does not communicate."""
    Xt, g0f, feats = ctm_corpus(dict(sc, D=sc["D_train"], seed=sc.get("seed", 4) + 100))
    t = _ctm_model(pkg, ctx, sc, Xt, g0f, feats)
    pkg.fit(t, maxiter=4, tol=0.0, verbose=False)
    out = {f: t._get(f) for f in CTM_GLOBALS}
    t.close()
    return out


def run_ctm_heldout(pkg, ctx, sc, X, g0f, feats, topics):
    """fit_heldout (MMCTM.jl:554-586) and transform without / with fit_gaussian (:511-552) of this rank's held-out documents: the steps of
    multimodalmusig.jl_amd/inference.py on the communicating context, three passes each."""
    from ctypes import byref, c_int
    out = {}
    for tag, flags in HELDOUT_MODES:
        g = _ctm_model(pkg, ctx, sc, X, g0f, feats)
        if tag == "heldout":
            for f in CTM_GLOBALS:
                g._set(f, topics[f])
        else:
            g._set("phi", topics["phi"])
            if not flags & 2:
                g._set("mu", topics["mu"]); g._set("Sigma", topics["Sigma"])
        ll = np.zeros(sc["maxiter"] * g.M); ni = c_int(); cv = c_int()
        pkg._lib.check(pkg.lib().mmm_ctm_infer(g._h, flags, sc["maxiter"], 0.0, ll.ctypes.data, byref(ni), byref(cv)), ctx.h, "mmm_ctm_infer")
        out[tag + "_ll"] = ll[:ni.value * g.M].reshape(ni.value, g.M).copy()
        for f in ("mu", "Sigma", "invSigma", "lambda", "nu", "props"):
            out[tag + "_" + f] = g._get(f)
        out[tag + "_elbo"] = pkg.calculate_elbo(g)
        g.close()
    return out


def _batch_inits(sc):
    rng = np.random.default_rng(sc.get("seed", 4) + 7)
    return [[rng.integers(1, 101, size=(k, v)).astype(np.float64) for k, v in zip(sc["K"], sc["V"])] for _ in range(sc["R"])]


BATCH_FIELDS = ("mu", "Sigma", "invSigma", "gamma", "Elnphi", "lambda", "nu", "zeta", "props", "theta")


def run_ctm_batch(pkg, ctx, sc, X):
    """R restarts in one handle on the communicating context (nrep x s_stats doubles per exchange), then each restart as a single handle."""
    g0 = _batch_inits(sc)
    out = {"error": ""}
    batch = pkg.MMCTM(sc["K"], sc["alpha"], sc["V"], X, γ0=g0, restarts=sc["R"], ctx=ctx)
    t0 = time.monotonic()
    try:
        hists = pkg.fit_restarts(batch, maxiter=sc["maxiter"], tol=sc["tol"])
    except pkg.MmmError as e:
        out["error"] = str(e)
        out["seconds"] = time.monotonic() - t0
        ctx.synchronize()
        batch.close()
        return out
    for r in range(sc["R"]):
        batch.select(r)
        out["batch%d" % r] = dict({f: batch._get(f) for f in BATCH_FIELDS}, ll=hists[r], elbo=batch.restart_elbo[r], converged=bool(batch.restart_converged[r]))
    batch.close()
    for r in range(sc["R"]):
        single = pkg.MMCTM(sc["K"], sc["alpha"], sc["V"], X, γ0=g0[r], ctx=ctx)
        h = pkg.fit(single, maxiter=sc["maxiter"], tol=sc["tol"], verbose=False)
        out["single%d" % r] = dict({f: single._get(f) for f in BATCH_FIELDS}, ll=h, elbo=single.elbo, converged=single.converged)
        single.close()
    return out


def run_scenario(pkg, ctx, world, rank, sc, override, plain):
    """-> the results of this rank: {field: array}.  plain["ctx"]: a second context of the rank, which does not communicate."""
    kind = sc["kind"]
    if kind.startswith("lda"):
        X, lam0 = lda_corpus(sc)
        d0, d1 = shard_of(sc, world, rank, X, override)
        if kind == "lda_passes":
            out = run_lda_passes(pkg, ctx, sc, X[d0:d1], lam0)
        elif kind == "lda_fit":
            out = run_lda_fit(pkg, ctx, sc, X[d0:d1], lam0)
        elif kind == "lda_overflow":
            out = run_lda_overflow(pkg, ctx, sc, X[d0:d1], lam0)
        elif kind == "lda_stage":
            out = run_lda_stage(pkg, ctx, sc, X[d0:d1], lam0)
        elif kind == "lda_infer":
            # the topics: trained unsharded by every rank for itself, on a context that does not communicate (the same bits everywhere)
            Xt, lt = lda_corpus(dict(sc, D=sc["D_train"], seed=sc.get("seed", 5) + 100, empty=()))
            t = _lda_model(pkg, plain["ctx"], sc, Xt, lt)
            pkg.fit(t, maxiter=15, tol=0.0, verbose=False)
            topics = {"lam": t.λ, "Elnbeta": t.Elnβ, "beta": t.β}
            t.close()
            out = run_lda_infer(pkg, ctx, sc, X[d0:d1], lam0, topics)
            out["topics"] = topics
        else:
            raise KeyError(kind)
    elif kind == "ilda":
        c = ilda_case(sc)
        d0, d1 = shard_of(sc, world, rank, c["X"], override)
        out = run_ilda(pkg, ctx, sc, c, d0, d1)
    elif kind.startswith("ctm"):
        X, g0f, feats = ctm_corpus(sc)
        d0, d1 = shard_of(sc, world, rank, X, override)
        if kind == "ctm":
            out = run_ctm(pkg, ctx, sc, X[d0:d1], g0f, feats)
        elif kind == "ctm_stage":
            out = run_ctm_stage(pkg, ctx, sc, X[d0:d1], g0f, feats)
        elif kind == "ctm_heldout":
            topics = ctm_train(pkg, plain["ctx"], sc)
            out = run_ctm_heldout(pkg, ctx, sc, X[d0:d1], g0f, feats, topics)
            out["topics"] = topics
        elif kind == "ctm_batch":
            out = run_ctm_batch(pkg, ctx, sc, X[d0:d1])
        else:
            raise KeyError(kind)
    else:
        raise KeyError(kind)
    out["shard"] = (d0, d1)
    return out


def run_plain(pkg, ctx, sc):
    """The unsharded device fit of a scenario that asks for one (`plain`), on a context that does not communicate."""
    kind = sc["kind"]
    if kind == "lda_fit":
        X, lam0 = lda_corpus(sc)
        return run_lda_fit(pkg, ctx, sc, X, lam0)
    if kind == "lda_passes":
        X, lam0 = lda_corpus(sc)
        return run_lda_passes(pkg, ctx, sc, X, lam0)
    if kind == "ilda":
        c = ilda_case(sc)
        return run_ilda(pkg, ctx, sc, c, 0, sc["D"])
    if kind == "ctm":
        X, g0f, feats = ctm_corpus(sc)
        return run_ctm(pkg, ctx, sc, X, g0f, feats)
    if kind == "ctm_heldout":
        X, g0f, feats = ctm_corpus(sc)
        return run_ctm_heldout(pkg, ctx, sc, X, g0f, feats, ctm_train(pkg, ctx, sc))
    raise KeyError(kind)


def _worker(rank, world, port, scenarios, override, q):
    res = {"rank": rank, "results": {}, "plain": {}, "seconds": {}, "error": None}
    dist = None
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ["MMM_P2P_TIMEOUT_S"] = "20"
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        import mmm_pkg
        pkg = mmm_pkg.load()

        def allgather(b):
            out = [None] * world
            dist.all_gather_object(out, b)
            return out

        def allmin(v):
            out = [None] * world
            dist.all_gather_object(out, int(v))
            return min(out)

        t0 = time.monotonic()
        ctx = pkg.Context(0)
        ctx.init_p2p(world, rank, allgather, allmin)
        assert ctx.transport == "p2p"
        res["seconds"]["<set-up>"] = time.monotonic() - t0
        plain = {"ctx": pkg.Context(0)}
        name = "<set-up>"
        try:
            for sc in scenarios:
                name = sc["name"]
                t0 = time.monotonic()
                res["results"][name] = run_scenario(pkg, ctx, world, rank, sc, override, plain)
                res["seconds"][name] = time.monotonic() - t0
            # the unsharded fits, on rank 0 alone, while the peers wait on the host (the barrier below)
            for sc in scenarios:
                if rank == 0 and sc.get("plain"):
                    name = "plain " + sc["name"]
                    res["plain"][sc["name"]] = run_plain(pkg, plain["ctx"], sc)
        except BaseException as e:      # noqa: BLE001 -- recorded; this rank issues no further GPU call, its peers meet the library's time limit
            res["error"] = "rank %d, scenario %s: %s\n%s" % (rank, name, e, traceback.format_exc())
    except BaseException as e:          # noqa: BLE001
        res["error"] = "rank %d, set-up: %s\n%s" % (rank, e, traceback.format_exc())
    # the mailboxes must outlive every peer's last store: nobody tears down before all ranks are here (bounded by the group's time-out)
    try:
        if dist is not None and dist.is_initialized():
            dist.barrier()
    except BaseException as e:          # noqa: BLE001
        res["error"] = (res["error"] or "") + "\nrank %d: barrier: %s" % (rank, e)
    q.put(res)
    try:
        if dist is not None and dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
    except BaseException:               # noqa: BLE001
        pass


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def run_ranks(world, scenarios, bounds=None):
    """Spawn `world` ranks (at most 4) on device 0, run the scenarios in order on each, and return
    {"ranks": [per rank {scenario: {field: array}}], "plain": {scenario: unsharded fit of rank 0}, "errors": [...], "seconds": {...}}.
    bounds: {number of documents: [b_0 .. b_world]} -- the shards of every corpus of that size, in place of shard_documents.
    Every wait is bounded: the library's 20 s in a kernel, gloo's 120 s, the queue and the joins here.  Nothing is started twice."""
    import queue as _queue

    import torch.multiprocessing as mp
    assert 2 <= world <= 4
    check_residency(world, scenarios, bounds)
    mctx = mp.get_context("spawn")
    q = mctx.Queue()
    port = _free_port()
    procs = [mctx.Process(target=_worker, args=(r, world, port, scenarios, bounds, q)) for r in range(world)]
    t0 = time.monotonic()
    for p in procs:
        p.start()
    got, errors = [], []
    deadline = time.monotonic() + 420
    while len(got) < world and time.monotonic() < deadline:
        try:
            got.append(q.get(timeout=5))
        except _queue.Empty:
            if not any(p.is_alive() for p in procs) and q.empty():
                break
    for p in procs:
        p.join(timeout=60)
    for r, p in enumerate(procs):
        if p.is_alive():
            errors.append("rank %d did not end" % r)
            p.terminate(); p.join(timeout=30)
        elif p.exitcode != 0:
            errors.append("rank %d ended with exit code %s" % (r, p.exitcode))
    if len(got) < world:
        errors.append("%d of %d ranks reported" % (len(got), world))
    got.sort(key=lambda r: r["rank"])
    errors += [r["error"] for r in got if r["error"]]
    return {"world": world, "ranks": [r["results"] for r in got], "plain": got[0]["plain"] if got else {}, "errors": errors,
            "seconds": {"total": time.monotonic() - t0, "ranks": [r["seconds"] for r in got]}}


# --------------------------------------------------------------------------------------------------------------- references
def lda_reference(sc, passes=3):
    """np_ref.lda_iteration on the full corpus from the constructor state (γ = 1, ϕ = 1 / K): per pass λ, Elnβ, β, γ, ll."""
    import np_ref
    X, lam0 = lda_corpus(sc)
    K = sc["K"]
    lam = lam0.copy()
    phi = [np.full((K, x.shape[0]), 1.0 / K) for x in X]
    out = []
    for _ in range(passes):
        r = np_ref.lda_iteration(X, K, ALPHA, ETA, lam, phi)
        lam, phi = r["lam"], r["phi"]
        out.append(r)
    return X, out


def gam(n):
    u = 2.0 ** -53
    return n * u / (1.0 - n * u)


def docs_per_term(X, V):
    n = np.zeros(V)
    for x in X:
        n[np.unique(np.asarray(x, dtype=np.int64).reshape(-1, 2)[:, 0]) - 1] += 1
    return n


def tree_roundings(world, grid_e=CUS * 2):
    """roundings of a cross-document sum beyond one per document: the reduction over the E-step blocks' partials (64 slab lanes, two 8-way
    stages), one per rank"""
    return np.ceil(grid_e / 64.0) + 16 + world


def _softmax0(E):
    e = np.exp(E.astype(np.longdouble) - E.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def ctm_gamma_pass1(sc, X, g0f, feats, world):
    """The γ sums of the FIRST pass of a CTM handle (MMCTM.jl:224-242, IMMCTM.jl:199-223) in np.longdouble.  The constructor's λ is 0, so the θ
    they are formed from is softmax_k Elnϕ₀[k, v] for every document -- no LD_MMA solve enters: γ₁ = α + θ_kv Σ_d n_dv (IMMCTM: folded onto
    the values of every feature).  -> (value, statistic = value - α, n, roundings of a θ), flat in the header's γ layout; n counts one
    addition per document listing the term (and per term of a feature value), the tree and the ranks."""
    import elbo_ref as R
    from scipy.special import digamma as psi
    LD = np.longdouble
    vals, stats, ns, nth, off = [], [], [], 0.0, 0
    for m, K in enumerate(sc["K"]):
        Xm = [x[m] for x in X]
        V = sc["V"][m]
        Nv = np.zeros(V, dtype=LD)
        for x in Xm:
            np.add.at(Nv, np.asarray(x, dtype=np.int64).reshape(-1, 2)[:, 0] - 1, np.asarray(x, dtype=np.int64).reshape(-1, 2)[:, 1].astype(LD))
        docs = docs_per_term(Xm, V)
        if feats is None:
            G0 = g0f[off:off + K * V].reshape(K, V); off += K * V
            E = psi(G0) - psi(G0.sum(axis=1, keepdims=True))
            st = _softmax0(E) * Nv[None, :]
            n = np.broadcast_to(docs[None, :], (K, V))
            extra = 0
        else:
            F = np.asarray(feats[m], dtype=np.int64) - 1; J = [int(j) + 1 for j in F.max(axis=0)]; SJ = sum(J)
            G0 = g0f[off:off + K * SJ].reshape(K, SJ); off += K * SJ
            jo = np.concatenate([[0], np.cumsum(J)])
            E = np.zeros((K, V))
            for i in range(len(J)):
                Gi = G0[:, jo[i]:jo[i + 1]]
                E += (psi(Gi) - psi(Gi.sum(axis=1, keepdims=True)))[:, F[:, i]]
            th = _softmax0(E) * Nv[None, :]
            st = np.zeros((K, SJ), dtype=LD); n = np.zeros((K, SJ))
            for i in range(len(J)):
                for j in range(J[i]):
                    sel = F[:, i] == j
                    st[:, jo[i] + j] = th[:, sel].sum(axis=1); n[:, jo[i] + j] = docs[sel].sum() + sel.sum()
            extra = len(J) - 1
        nth = max(nth, R.phi_roundings(np.zeros(1), E, K) + extra)
        a = sc["alpha"][m]
        vals.append((st + LD(a)).ravel()); stats.append(st.ravel()); ns.append(n.ravel() + tree_roundings(world))
    return np.concatenate(vals), np.concatenate(stats), np.concatenate(ns), nth


def ilda_stat_pass1(c, world):
    """(n per feature [J_i], roundings of a ϕ) of the first pass's ILDA statistics λ_i[j, k] - η_i = Σ_{v: f_i(v) = j} Σ_d n_dv ϕ_dvk."""
    import elbo_ref as R
    from scipy.special import digamma as psi
    F = np.asarray(c["features"], dtype=np.int64) - 1
    docs = docs_per_term(c["X"], c["V"])
    E = sum((psi(l) - psi(l.sum(axis=0, keepdims=True)))[F[:, i], :] for i, l in enumerate(c["lam0"]))
    nphi = R.phi_roundings(np.array([psi(1.0) - psi(float(c["K"]))]), E, c["K"]) + len(c["J"]) - 1
    n = [np.array([docs[F[:, i] == j].sum() + (F[:, i] == j).sum() for j in range(J)]) + tree_roundings(world) for i, J in enumerate(c["J"])]
    return n, nphi


def sum_roundings(X, V, world, grid_e=CUS * 2):
    """n of a cross-document sum of non-negative terms as the kernels form it (the bound is γ_n x value, tests/elbo_ref.py): one addition per
    document that lists the term, the reduction tree over the E-step blocks' partials (64 slab lanes, two 8-way stages), one per rank."""
    per_term = np.zeros(V)
    for x in X:
        per_term[np.asarray(x, dtype=np.int64).reshape(-1, 2)[:, 0] - 1] += 1
    return per_term + np.ceil(grid_e / 64.0) + 16 + world
