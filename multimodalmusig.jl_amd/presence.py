"""Is signature t really present in this sample, and with what p-value? -- the question that follows a refit (SBS3 for an HRD call, APOBEC, a
therapy signature) and that neither the BIC decision of `refit_exposures` nor its intervals on the chosen set answer.

Per (target, sample) the likelihood-ratio statistic Λ = 2 (ll(allowed ∪ {t}) - ll(allowed ∖ {t})) is computed from two constrained EM fits.
The tested weight sits on the boundary of the simplex, where the χ² reference distribution is wrong, so the null distribution is the
parametric bootstrap: B count vectors are drawn from the sample's own null fit and each is refitted with and without the signature.  All of
it -- the draws, both fits and the comparison -- runs in one call (`mmm_presence_test`); the replicates' counts never leave the device's
LDS, and the larger fit is skipped wherever the score Σ_v r_v P[t][v] <= 1 already proves that the target's weight is 0.  The definition,
down to the order of every sum, is in include/mmmusig.h.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .bootstrap import _is_nested, _modality_csr
from .ctm import MMCTM
from .models import LDA
from .refit import MAX_CATALOGUE, RefitResult, _allowed, _catalogue
from .simulate import MAX_TERMS, _seeds
from .utils import PackedCorpus, pack_lda, pack_mm

_PresenceResult = namedtuple("PresenceResult", "p stat score exposure_alt exposures_null count_ge count_zero status iters B replicates names")


class PresenceResult(_PresenceResult):
    """All arrays [T, D] (target, sample) unless said otherwise.  p = (1 + count_ge) / (B + 1), NaN where the pair is untestable (and with
    B = 0); stat: Λ_obs (+inf where only the target can produce one of the sample's mutations); score: s = Σ_v r_v P[t][v] under the null
    fit -- s <= 1 means the null optimum is the optimum with the target too; exposure_alt: the target's weight in the larger fit (0 where
    that fit was not needed); exposures_null: [T, C, D] the weights of the fit without the target; count_ge, count_zero: replicates with
    Λ_b >= Λ_obs, with Λ_b = 0; status: 0 tested by replicates, 1 Λ_obs = 0 (p = 1, none run), 2 Λ_obs = +inf (p = 1 / (B + 1), none run),
    3 untestable (no mutations, or nothing allowed besides the target); iters: EM iterations of all the pair's fits; replicates:
    [B, T, D] Λ_b with keep_replicates (NaN where none were run), else None; names: the targets' names where the catalogue has names."""
    __slots__ = ()

    def significant(self, alpha=0.05):
        """[T, D] bool: p <= alpha (False where untestable)"""
        with np.errstate(invalid="ignore"):
            return np.nan_to_num(self.p, nan=np.inf) <= float(alpha)


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _targets(targets, names, C):
    """-> (int32 [T] indices, their names or None)"""
    if isinstance(targets, (str, int, np.integer)):
        targets = [targets]
    targets = list(targets)
    if not targets:
        raise ValueError("targets is empty")
    if all(isinstance(t, str) for t in targets):
        if names is None:
            raise ValueError("targets holds names but the catalogue came without names")
        unknown = [t for t in targets if t not in names]
        if unknown:
            raise ValueError("targets names a signature the catalogue lacks: %r" % unknown[0])
        idx = [names.index(t) for t in targets]
    else:
        if any(isinstance(t, str) or int(t) != t for t in targets):
            raise ValueError("targets must be all names or all indices")
        idx = [int(t) for t in targets]
        if any(not 0 <= i < C for i in idx):
            raise ValueError("targets must be catalogue rows in [0, %d)" % C)
    return np.asarray(idx, dtype=np.int32), ([names[i] for i in idx] if names is not None else None)


def _raw(ctx, D, V, doc_ptr, term, count, cat, targets, allowed=None, B=0, b0=0, seed=0, stream=0, maxiter=1000, tol=1e-9, keep=False, catalogue_in_lds=True):
    """mmm_presence_test on one CSR corpus (0-based terms) -> dict of its outputs, item-major ([T D] / [T D, C] / [B, T D]).
    catalogue_in_lds=False (tests): the replicate launch reads the catalogue through L2 even where an item's rows fit LDS."""
    cat = np.ascontiguousarray(cat, dtype=np.float64)
    C = cat.shape[0]
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    term = np.ascontiguousarray(term, dtype=np.int32); count = np.ascontiguousarray(count, dtype=np.int32)
    targets = np.ascontiguousarray(targets, dtype=np.int32)
    T = targets.size
    if allowed is not None:
        allowed = np.ascontiguousarray(allowed, dtype=np.uint8)
        if allowed.shape != (D, C):
            raise ValueError("allowed must be [D, C] = [%d, %d], got %r" % (D, C, allowed.shape))
    TD = T * D
    out = dict(w_null=np.zeros((TD, C)), stat=np.zeros(TD), score=np.zeros(TD), w_alt=np.zeros(TD), count_ge=np.zeros(TD, dtype=np.int32),
               count_zero=np.zeros(TD, dtype=np.int32), status=np.zeros(TD, dtype=np.int8), iters=np.zeros(TD, dtype=np.int64),
               rep_stat=np.zeros((B, TD)) if keep else None)
    before = None
    if not catalogue_in_lds:
        before = ctx.get_tuning()
        t = _lib.TuningOpts.from_buffer_copy(before)
        t.disable |= _lib.OFF["refit_lds"]
        check(lib().mmm_ctx_set_tuning(ctx.h, _lib.C.byref(t)), ctx.h, "mmm_ctx_set_tuning")
    try:
        rc = lib().mmm_presence_test(ctx.h, int(D), C, int(V), doc_ptr, _ptr(term), _ptr(count), cat.ravel(), _ptr(allowed), T, _ptr(targets), int(B), int(b0),
                                     int(seed), int(stream), int(maxiter), float(tol),
                                     *[_ptr(out[k]) for k in ("w_null", "stat", "score", "w_alt", "count_ge", "count_zero", "status", "iters", "rep_stat")])
    finally:
        if before is not None:
            check(lib().mmm_ctx_set_tuning(ctx.h, _lib.C.byref(before)), ctx.h, "mmm_ctx_set_tuning")
    check(rc, ctx.h, "mmm_presence_test")
    return out


def _table(catalogue, targets, modality):
    """-> (names or None, cat [C, V], int32 [T] targets, their names or None), within the limits of the presence kernels"""
    names, cat = _catalogue(catalogue, modality)
    C, V = cat.shape
    if C < 1 or V < 1:
        raise ValueError("the catalogue must have at least one signature and one term")
    if C > MAX_CATALOGUE:
        raise ValueError("C = %d catalogue signatures (limit %d)" % (C, MAX_CATALOGUE))
    if V > MAX_TERMS:
        raise ValueError("V = %d terms (limit %d)" % (V, MAX_TERMS))
    tg, tnames = _targets(targets, names, C)
    return names, cat, tg, tnames


def _corpus(X, modality, allowed, names, C, V):
    """-> (D, doc_ptr, term, count, allowed [D, C] uint8 or None) of X as the presence kernels take it"""
    D = len(X)
    if _is_nested(X):
        if modality is None:
            raise ValueError("an MMCTM-nested X holds one corpus per modality: pass modality=m")
        M = X.M if isinstance(X, PackedCorpus) else len(X[0])
        if not 0 <= int(modality) < M:
            raise ValueError("modality %d of %d" % (int(modality), M))
        dp_all, term_all, count_all = pack_mm(X, M)
        doc_ptr, count, e0 = _modality_csr(dp_all, count_all, D, int(modality))
        term = term_all[e0:e0 + count.size]
    else:
        doc_ptr, term, count = pack_lda(X)
    if term.size and int(term.max()) >= V:
        raise ValueError("X holds term %d, the catalogue has %d terms" % (int(term.max()) + 1, V))
    if isinstance(allowed, RefitResult):
        if allowed.active.shape != (C, D):
            raise ValueError("the RefitResult holds %r chosen sets, not C x D = %d x %d" % (allowed.active.shape, C, D))
        al = np.ascontiguousarray(allowed.active.T, dtype=np.uint8)
    else:
        al = _allowed(allowed, names, D, C)
    return D, doc_ptr, term, count, al


def signature_presence(X, catalogue, targets, allowed=None, B=1000, seed=None, stream=0, b0=0, maxiter=1000, tol=1e-9, modality=None, keep_replicates=False,
                       ctx=None):
    """Per-sample test of H0: the weight of signature t is 0, for every t of `targets` and every sample of X -> PresenceResult.

    X and catalogue as `refit_exposures` takes them (C <= 256; here also V <= 4096).  targets: catalogue rows, as indices or -- where the
    catalogue has names -- as names.  allowed: as in `refit_exposures`, or a `RefitResult`, whose chosen sets are then used: refit first,
    then test what was kept (is it significant?) or what was dropped (was it dropped for lack of evidence?).  A target is always ADDED to
    the set for the larger fit and REMOVED from it for the null fit, whether the sample's set holds it or not.
    B: parametric-bootstrap replicates per tested pair; p = (1 + #{Λ_b >= Λ_obs}) / (B + 1).  Pairs whose Λ_obs is exactly 0 (p = 1) or +inf
    (p = 1 / (B + 1)) take no replicates.  Replicates b0 .. b0 + B - 1 of the sequence that (seed, stream) fixes: the counts of chunked
    calls add.  seed is required when B > 0.  The replicates are the vectors `simulate_counts(exposures_null, P, N, B, seed, stream)` gives
    for the T x D pairs as one corpus (P: the row-normalised catalogue), so a `goodness_of_fit` of the null fits under the same seed and
    stream sees the same draws and is correlated with this test: give the two different streams.  The test is conservative: under H0
    about half of the replicates (and of the samples) have Λ = 0 exactly, a point mass at p = 1.
    keep_replicates: return the [B, T, D] statistics Λ_b.  ILDA / IMMCTM catalogues: TypeError (factorised tables)."""
    names, cat, tg, tnames = _table(catalogue, targets, modality)
    C, V = cat.shape
    B = int(B)
    if B > 0 and seed is None:
        raise ValueError("B > 0 replicates need a seed")
    B, b0, seed, stream = _seeds(B, b0, 0 if seed is None else seed, stream)
    D, doc_ptr, term, count, al = _corpus(X, modality, allowed, names, C, V)
    T = tg.size
    ctx = ctx or (catalogue.ctx if isinstance(catalogue, (LDA, MMCTM)) else _lib.default_context())      # every argument is checked before a device is asked for
    r = _raw(ctx, D, V, doc_ptr, term, count, cat, tg, al, B, b0, seed, stream, maxiter, tol, keep=bool(keep_replicates))
    status = r["status"].reshape(T, D)
    count_ge = r["count_ge"].reshape(T, D)
    p = (1.0 + count_ge) / (B + 1.0) if B else np.full((T, D), np.nan)
    p = np.where(status == 3, np.nan, p)
    return PresenceResult(p, r["stat"].reshape(T, D), r["score"].reshape(T, D), r["w_alt"].reshape(T, D), r["w_null"].reshape(T, D, C).transpose(0, 2, 1).copy(),
                          count_ge, r["count_zero"].reshape(T, D), status, r["iters"].reshape(T, D), B,
                          r["rep_stat"].reshape(B, T, D) if keep_replicates else None, tnames)
