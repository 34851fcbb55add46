"""Choosing the number of signatures by held-out mutations -- the question the reference leaves outside the package (`LDA(7, ...)`,
`MMCTM([7, 7], ...)`, `run_mmctm.jl -k`: K is always given).

Every document's mutations are dealt into F folds on the GPU (`mmm_split_counts`: one Philox word per mutation), for every candidate K
the restarts of a batch are fitted on F - 1 folds and every restart is scored on the fold it did not see where its tables lie
(`mmm_lda_score_replicas`), and the candidate with the best held-out log-likelihood per mutation -- or the smallest within one standard
error of it -- is picked.  The definitions, down to the order of every sum, are in include/mmmusig.h: the same
arguments give the same bits on every run.
"""
import time
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import MmmError, check, lib
from .bootstrap import _is_nested, _modality_csr
from .models import LDA, fit
from .utils import PackedCorpus, pack_lda, pack_mm

MAX_FOLDS = 64

ScoreResult = namedtuple("ScoreResult", "ll ll_doc n_doc cosine_doc cosine")
ScoreResult.__doc__ = """ll: log-likelihood per mutation over the documents with N_d > 0 (= calculate_loglikelihood(X, θ, β)); ll_doc, n_doc,
cosine_doc: [D] per-document log-likelihood, mutations and cosine between the counts and their reconstruction; cosine: the mean of
cosine_doc over the documents with N_d > 0."""

KPick = namedtuple("KPick", "mean se best pick")
KPick.__doc__ = """mean, se: [len(Ks)] mean and standard error of every candidate's scores; best: the K with the highest mean (ties to the
lowest K); pick: the smallest K whose mean is within one standard error (best's) of it."""

KSelection = namedtuple("KSelection", "Ks heldout heldout_all mean se best pick train_ll stability cosine")
KSelection.__doc__ = """Ks: the candidates; heldout: [nK, reps * F] held-out log-likelihood per mutation of the restart with the best TRAINING
log-likelihood, repetition-major; heldout_all: [nK, reps * F, R] of every restart; mean, se, best, pick: `pick_k(Ks, heldout)`; with full_fit
(else None) train_ll: [nK] best final log-likelihood on all of X, stability: list over K of the [K] `restart_consensus` stability,
cosine: [nK] mean reconstruction cosine of the best restart on X."""

MMSelection = namedtuple("MMSelection", "Ks heldout picks")
MMSelection.__doc__ = """Ks: the candidates (per-modality K lists); heldout: [nK, reps * F, M] held-out log-likelihood per mutation of every
modality under the seeded stage-2 model; picks: list over the modalities of `pick_k` over the candidates' K[m] (None unless asked for)."""


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _split_csr(ctx, D, doc_ptr, count, F, rep, seed, stream):
    """mmm_split_counts on one CSR corpus (doc_ptr relative to its first entry) -> int32 [F, nnz]"""
    F, rep, seed, stream = int(F), int(rep), int(seed), int(stream)
    if not 1 <= F <= MAX_FOLDS:
        raise ValueError("folds must be 1..%d" % MAX_FOLDS)
    if not 0 <= seed < 2 ** 64 or not 0 <= stream < 2 ** 31 or not 0 <= rep < 2 ** 31:
        raise ValueError("seed must fit 64 bits (unsigned), stream and rep 31 bits")
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    out = np.zeros((F, count.size), dtype=np.int32)
    check(lib().mmm_split_counts(ctx.h, int(D), doc_ptr, _ptr(count), F, rep, seed, stream, _ptr(out)), ctx.h, "mmm_split_counts")
    return out


def split_counts(X, folds, seed, rep=0, ctx=None):
    """Every document's mutations dealt into `folds` folds, on the GPU: a list of `folds` corpora of X's shape -- same rows, same terms, the
    counts of the fold; rows that come out 0 are KEPT; the folds of an entry sum to its count.  `rep` numbers repeated splits of one seed.
    X as LDA takes it (list of W_d x 2 matrices, 1-based terms) or MMCTM-nested (X[d][m]): modality m is split with stream = m."""
    ctx = ctx or _lib.default_context()
    D = len(X)
    if _is_nested(X):
        M = X.M if isinstance(X, PackedCorpus) else len(X[0])
        doc_ptr, term, count = pack_mm(X, M)
        per_mod = []
        for m in range(M):
            dp, c, e0 = _modality_csr(doc_ptr, count, D, m)
            per_mod.append((dp, term[e0:e0 + c.size] + 1, _split_csr(ctx, D, dp, c, folds, rep, seed, m)))
        return [[[np.stack([t[dp[d]:dp[d + 1]], r[f, dp[d]:dp[d + 1]]], axis=1).astype(np.int64) for dp, t, r in per_mod] for d in range(D)]
                for f in range(int(folds))]
    doc_ptr, term, count = pack_lda(X)
    r = _split_csr(ctx, D, doc_ptr, count, folds, rep, seed, 0)
    t = term + 1
    return [[np.stack([t[doc_ptr[d]:doc_ptr[d + 1]], r[f, doc_ptr[d]:doc_ptr[d + 1]]], axis=1).astype(np.int64) for d in range(D)]
            for f in range(int(folds))]


def _minus(x, p):
    x = np.asarray(x, dtype=np.int64).reshape(-1, 2); p = np.asarray(p, dtype=np.int64).reshape(-1, 2)
    if x.shape != p.shape or not np.array_equal(x[:, 0], p[:, 0]) or (p[:, 1] > x[:, 1]).any():
        raise ValueError("holdout: the fold is no part of X (rows, terms or counts do not fit)")
    return np.stack([x[:, 0], x[:, 1] - p[:, 1]], axis=1)


def holdout(X, parts, f):
    """(X_train, X_test) for fold f of `parts = split_counts(X, ...)`: X_test is the fold, X_train = X - fold f (rows kept, counts
    subtracted).  LDA or MMCTM nesting."""
    test = parts[int(f)]
    if len(test) != len(X):
        raise ValueError("holdout: the fold has %d documents, X %d" % (len(test), len(X)))
    if _is_nested(X):
        return [[_minus(xm, pm) for xm, pm in zip(x, p)] for x, p in zip(X, test)], test
    return [_minus(x, p) for x, p in zip(X, test)], test


def score_exposures(X, θ, β, ctx=None):
    """Held-out score of the documents X (LDA nesting) under exposures θ (K x D) and signatures β (V x K) -> ScoreResult(ll, ll_doc, n_doc,
    cosine_doc, cosine) (`mmm_mixture_score`).  ll equals `calculate_loglikelihood(X, θ, β)` bit for bit."""
    ctx = ctx or _lib.default_context()
    doc_ptr, term, count = pack_lda(X)
    th = np.ascontiguousarray(np.asarray(θ, dtype=np.float64).T); be = np.ascontiguousarray(np.asarray(β, dtype=np.float64).T)   # [k + K d], [k V + v]
    D = len(X)
    if th.ndim != 2 or be.ndim != 2 or th.shape[0] != D or th.shape[1] != be.shape[0]:
        raise ValueError("θ must be K x D and β V x K for the D = %d documents of X" % D)
    ll_doc = np.zeros(D); n_doc = np.zeros(D); cos_doc = np.zeros(D); total = np.zeros(4)
    check(lib().mmm_mixture_score(ctx.h, D, th.shape[1], be.shape[1], doc_ptr, _ptr(term), _ptr(count), th.ravel(), be.ravel(), _ptr(ll_doc), _ptr(n_doc),
                                  _ptr(cos_doc), total), ctx.h, "mmm_mixture_score")
    return ScoreResult(float(total[0]), ll_doc, n_doc, cos_doc, float(total[3]))


def score_restarts(model, X, per_document=False):
    """Every restart of a fitted LDA (a restart batch or an ordinary model: one restart) scored on the documents X -- the model's D
    documents, usually the held-out fold -- where its tables lie (`mmm_lda_score_replicas`): total [R, 4] = (ll per mutation, Σ ll, Σ N,
    mean cosine) per restart; with per_document=True also ll_doc and cosine_doc, [R, D] each.  Restart r's row equals
    `score_exposures(X, θ, β)` on its downloaded θ, β bit for bit.  The model, its selected restart included, is left as it was."""
    if not isinstance(model, LDA):
        raise TypeError("score_restarts takes an LDA (a restart batch or an ordinary model)")
    doc_ptr, term, count = pack_lda(X)
    if len(X) != model.D:
        raise ValueError("X has %d documents, the model %d" % (len(X), model.D))
    R, D = model.R, model.D
    total = np.zeros((R, 4))
    ll_doc = np.zeros((R, D)) if per_document else None
    cos_doc = np.zeros((R, D)) if per_document else None
    check(lib().mmm_lda_score_replicas(model._h, doc_ptr, _ptr(term), _ptr(count), total, _ptr(ll_doc), _ptr(cos_doc)), model.ctx.h, "score_restarts")
    return (total, ll_doc, cos_doc) if per_document else total


def pick_k(Ks, scores):
    """Ks: the candidate K values; scores: [len(Ks), n] (n folds x repetitions, higher is better) -> KPick(mean, se, best, pick).  se =
    sd(ddof=1) / sqrt(n), 0 for n = 1; best: the K with the highest mean, ties to the lowest K (a NaN mean never wins); pick: the smallest K
    with mean >= mean[best] - se[best] -- the one-standard-error rule."""
    Ks = [int(k) for k in Ks]
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] != len(Ks) or s.shape[1] < 1 or not Ks:
        raise ValueError("scores must be [len(Ks), n] with n >= 1")
    n = s.shape[1]
    mean = s.mean(axis=1)
    se = s.std(axis=1, ddof=1) / np.sqrt(n) if n > 1 else np.zeros(len(Ks))
    m = np.where(np.isnan(mean), -np.inf, mean)
    order = sorted(range(len(Ks)), key=lambda i: Ks[i])
    ib = max(order, key=lambda i: (m[i], -Ks[i]))
    bound = m[ib] - (0.0 if np.isnan(se[ib]) else se[ib])
    ip = next(i for i in order if m[i] >= bound)
    return KPick(mean, se, Ks[ib], Ks[ip])


def _restart_seeds(seed, K, rep, f, R):
    """the R initialisation seeds of candidate K, repetition rep, fold f (f = folds: the fit on all of X)"""
    return [int(s) for s in np.random.default_rng([int(seed), int(K), int(rep), int(f)]).integers(1, 2 ** 62, size=int(R))]


def _batch_refused(e):
    s = str(e)
    return "status -4" in s and "mmm_lda_create_batch" in s


def _fit_score_lda(K, α, η, V, Xtr, Xte, seeds, maxiter, tol, ctx, consensus=False, clock=None):
    """R restarts fitted on Xtr and scored on Xte -> (training ll [R], total [R, 4], stability or None).  A batch handle; shapes that
    batches refuse: R single handles one after the other, scored with score_exposures."""
    from .ctm import fit_restarts
    from .match import restart_consensus, signature_consensus
    from .restarts import _best
    R = len(seeds)
    lam0 = [np.random.default_rng(s).integers(1, 101, size=(V, K)).astype(np.float64) for s in seeds]     # as fit_lda_restarts
    t0 = time.perf_counter()
    try:
        model = LDA(K, α, η, V, Xtr, λ0=lam0, restarts=R, ctx=ctx)
    except MmmError as e:
        if not _batch_refused(e):
            raise
        model = None
    stab = None
    if model is not None:
        try:
            fit_restarts(model, maxiter=maxiter, tol=tol)
            ctx.synchronize()
            t1 = time.perf_counter()
            train = np.array(model.restart_ll, dtype=np.float64)
            total = score_restarts(model, Xte)
            t2 = time.perf_counter()
            if consensus:
                stab = restart_consensus(model, ref=_best(train), q=()).stability
        finally:
            model.close()
        if clock is not None:
            clock["fit"] = clock.get("fit", 0.0) + (t1 - t0); clock["score"] = clock.get("score", 0.0) + (t2 - t1)
        return train, total, stab
    train, total, lams = np.zeros(R), np.zeros((R, 4)), []
    for r in range(R):
        t0 = time.perf_counter()
        one = LDA(K, α, η, V, Xtr, λ0=lam0[r], ctx=ctx)
        try:
            fit(one, maxiter=maxiter, tol=tol, verbose=False)
            train[r] = one.ll
            θ, β = one.θ, one.β
            t1 = time.perf_counter()
            s = score_exposures(Xte, θ, β, ctx=ctx)
            total[r] = (s.ll, float(s.ll_doc[s.n_doc > 0].sum()), float(s.n_doc.sum()), s.cosine)
            t2 = time.perf_counter()
            if consensus:
                lams.append(np.ascontiguousarray(one.λ.T))
        finally:
            one.close()
        if clock is not None:
            clock["fit"] = clock.get("fit", 0.0) + (t1 - t0); clock["score"] = clock.get("score", 0.0) + (t2 - t1)
    if consensus:
        stab = signature_consensus(np.stack(lams), _best(train), q=(), ctx=ctx).stability
    return train, total, stab


def select_num_signatures(X, Ks, α, η, folds=4, reps=1, restarts=16, seed=0, maxiter=1000, tol=1e-4, full_fit=True, ctx=None, clock=None):
    """Held-out selection of the number of LDA signatures -> KSelection.

    For every repetition rep < reps the mutations of X are split into `folds` folds (`split_counts(X, folds, seed, rep)`); for every candidate
    K and fold f an `LDA(K, α, η, V, X_train, λ0=..., restarts=R)` is fitted on X minus the fold with `fit_restarts(maxiter, tol)` -- restart
    i initialised as `default_rng(s_i).integers(1, 101, (V, K))`, the s_i drawn from `default_rng([seed, K, rep, f])` -- and every restart
    is scored on the fold with `score_restarts`.  The fold's score is the held-out log-likelihood per mutation of the restart with the best
    TRAINING log-likelihood: the held-out fold never chooses among restarts.  `pick_k` then gives best and pick.  With full_fit one more
    batch per K is fitted on all of X: its best final log-likelihood, the `restart_consensus` stability of its topics and its mean
    reconstruction cosine are reported beside the held-out figures (a K whose extra signature is unstable across restarts shows there).
    V is the vocabulary of X (its largest term).  `clock`: a dict that receives the seconds spent in "split", "fit" and "score"."""
    from .restarts import _best
    ctx = ctx or _lib.default_context()
    Ks = [int(k) for k in Ks]
    F, reps, R = int(folds), int(reps), int(restarts)
    if not Ks or min(Ks) < 1 or reps < 1 or R < 1:
        raise ValueError("Ks must hold K >= 1, reps and restarts must be >= 1")
    if not 2 <= F <= MAX_FOLDS:
        raise ValueError("folds must be 2..%d: a model is fitted on the other folds" % MAX_FOLDS)
    doc_ptr, term, count = pack_lda(X)
    D = len(X)
    V = int(term.max()) + 1 if term.size else 0
    heldout = np.zeros((len(Ks), reps * F)); heldout_all = np.zeros((len(Ks), reps * F, R))
    for rep in range(reps):
        t0 = time.perf_counter()
        parts = _split_csr(ctx, D, doc_ptr, count, F, rep, seed, 0)
        if clock is not None:
            clock["split"] = clock.get("split", 0.0) + (time.perf_counter() - t0)
        for f in range(F):
            Xtr = PackedCorpus(D, doc_ptr, term, count - parts[f])
            Xte = PackedCorpus(D, doc_ptr, term, parts[f])
            for i, K in enumerate(Ks):
                train, total, _ = _fit_score_lda(K, α, η, V, Xtr, Xte, _restart_seeds(seed, K, rep, f, R), maxiter, tol, ctx, clock=clock)
                heldout_all[i, rep * F + f] = total[:, 0]
                heldout[i, rep * F + f] = total[_best(train), 0]
    p = pick_k(Ks, heldout)
    train_ll = stability = cosine = None
    if full_fit:
        Xall = PackedCorpus(D, doc_ptr, term, count)
        train_ll, cosine, stability = np.zeros(len(Ks)), np.zeros(len(Ks)), []
        for i, K in enumerate(Ks):
            train, total, stab = _fit_score_lda(K, α, η, V, Xall, Xall, _restart_seeds(seed, K, reps, F, R), maxiter, tol, ctx, consensus=True, clock=clock)
            b = _best(train)
            train_ll[i], cosine[i] = train[b], total[b, 3]
            stability.append(stab)
    return KSelection(Ks, heldout, heldout_all, p.mean, p.se, p.best, p.pick, train_ll, stability, cosine)


def select_num_signatures_mmctm(counts, Ks, α, V, folds=4, reps=1, restarts=16, seed=0, maxiter=1000, tol=1e-4, stage2_tol=1e-5, pick=False, ctx=None, **kw):
    """Held-out scores of candidate MMCTM shapes -> MMSelection(Ks, heldout [nK, reps * F, M], picks).  Ks: a list of per-modality K lists.
    Per repetition the mutations of `counts` (counts[d][m]) are split into `folds` folds (`split_counts`: modality m with stream = m); per
    candidate and fold the driver of scripts/run_mmctm.jl runs on the training counts -- `fit_seed_models(train, K, α, V, seeds, maxiter, tol)`
    with `restarts` seeds drawn from `default_rng([seed, i, rep, f])` (i: the candidate's index), then `seed_and_fit_restart(..., maxiter,
    stage2_tol)` -- and every modality of the fold is scored with `score_exposures` on the seeded model's props and ϕ.  pick=True:
    `pick_k` per modality over the candidates' K[m] (which must then differ from candidate to candidate).  A composition of existing
    pieces: no device code of its own."""
    from .restarts import fit_seed_models, seed_and_fit_restart
    ctx = ctx or _lib.default_context()
    Ks = [[int(k) for k in K] for K in Ks]
    F, reps, R = int(folds), int(reps), int(restarts)
    if not Ks or reps < 1 or R < 1 or not 2 <= F <= MAX_FOLDS:
        raise ValueError("Ks must not be empty, reps and restarts >= 1, folds 2..%d" % MAX_FOLDS)
    M, D = len(Ks[0]), len(counts)
    if any(len(K) != M for K in Ks) or len(V) != M:
        raise ValueError("every candidate and V must have one entry per modality")
    heldout = np.zeros((len(Ks), reps * F, M))
    for rep in range(reps):
        parts = split_counts(counts, F, seed, rep=rep, ctx=ctx)
        for f in range(F):
            train, test = holdout(counts, parts, f)
            for i, K in enumerate(Ks):
                seeds = [int(s) for s in np.random.default_rng([int(seed), i, rep, f]).integers(1, 2 ** 62, size=R)]
                opt_gamma, _, _ = fit_seed_models(train, K, α, V, seeds, ctx=ctx, maxiter=maxiter, tol=tol, **kw)
                model = seed_and_fit_restart(train, K, α, V, opt_gamma, ctx=ctx, maxiter=maxiter, tol=stage2_tol, **kw)
                try:
                    props, ϕ = model._get("props").reshape(D, model.MK), model.ϕ      # [d][modality-major ΣK], as bootstrap_exposures reads it
                    off = np.concatenate([[0], np.cumsum(K)])
                    for m in range(M):
                        θ = props[:, off[m]:off[m + 1]].T                                                                # K_m x D
                        β = np.stack([np.asarray(ϕ[m][k], dtype=np.float64) for k in range(K[m])], axis=1)             # V_m x K_m
                        heldout[i, rep * F + f, m] = score_exposures([test[d][m] for d in range(D)], θ, β, ctx=ctx).ll
                finally:
                    model.close()
    picks = None
    if pick:
        picks = []
        for m in range(M):
            km = [K[m] for K in Ks]
            if len(set(km)) != len(km):
                raise ValueError("pick=True: the candidates' K of modality %d must differ (%r)" % (m, km))
            picks.append(pick_k(km, heldout[:, :, m]))
    return MMSelection(Ks, heldout, picks)
