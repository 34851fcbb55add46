"""Signature assignment (refitting): the exposures of every sample to a FIXED catalogue of signatures, with the signatures a sample does
not need removed -- the step the reference leaves outside the package and, for many users, the only one they run (COSMIC SBS / DBS / ID
against a set of tumours).

Per sample the mixture weights are fitted by EM under the catalogue rows it may use, then the signature with the smallest weight is
removed and the rest refitted for as long as that costs less log-likelihood than the penalty (backward elimination, smallest contribution
first: deconstructSigs, MutationalPatterns' strict refit and SigProfilerAssignment all answer the question this way).  All rounds of all
samples run in one launch (`mmm_refit_exposures`); weights outside the chosen set are exactly 0.  The definition, down to the order of
every sum and every tie rule, is in include/mmmusig.h: the same arguments give the same bits on every run.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .bootstrap import _is_nested, _modality_csr, _resample_csr, replicate_summary
from .ctm import MMCTM
from .match import _reject_factorised, _signatures_of, _values
from .models import LDA
from .utils import PackedCorpus, pack_lda, pack_mm

MAX_CATALOGUE = 256       # catalogue rows a refit takes (a wave holds two weight vectors and two lists of them in LDS)

RefitResult = namedtuple("RefitResult", "exposures active order cost ll_doc unexplained iters counts intervals names")
RefitResult.__doc__ = """exposures: [C, D] weights of every sample, exactly 0 outside its chosen set; active: [C, D] bool; order, cost: [D, C] the
signatures removed from every sample in the order of their removal (-1 padded) and the log-likelihood each removal cost; ll_doc: [D]
Σ_v n_v log q_v under the final weights; unexplained: [D] mutations in terms none of the sample's signatures produces; iters: [D] EM
iterations of all the sample's fits; counts: [C, D] = exposures x N_d; intervals: with bootstrap=B a `RefitIntervals`, else None; names: the
catalogue's signature names where it came with them, else None."""

RefitIntervals = namedtuple("RefitIntervals", "mean sd quantiles q B")
RefitIntervals.__doc__ = """mean, sd: [C, D]; quantiles: [len(q), C, D] of the exposures of B multinomial resamples of every sample, refitted
on the sample's CHOSEN set (no further elimination)."""


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _raw(ctx, D, V, doc_ptr, term, count, cat, allowed=None, penalty=None, maxiter=1000, tol=1e-9, outputs="all", catalogue_in_lds=True):
    """mmm_refit_exposures on one CSR corpus (0-based terms) -> dict of w, active, order, cost [D, C], ll_doc, unexplained, iters [D].
    outputs="w": only w is asked for.  catalogue_in_lds=False (tests): the launch reads the catalogue through L2 even where it fits LDS."""
    cat = np.ascontiguousarray(cat, dtype=np.float64)
    C = cat.shape[0]
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    term = np.ascontiguousarray(term, dtype=np.int32); count = np.ascontiguousarray(count, dtype=np.int32)
    if allowed is not None:
        allowed = np.ascontiguousarray(allowed, dtype=np.uint8)
        if allowed.shape != (D, C):
            raise ValueError("allowed must be [D, C] = [%d, %d], got %r" % (D, C, allowed.shape))
    if penalty is not None:
        penalty = np.ascontiguousarray(penalty, dtype=np.float64)
        if penalty.shape != (D,):
            raise ValueError("penalty must hold one value per document")
    out = {"w": np.zeros((D, C))}
    if outputs == "all":
        out.update(active=np.zeros((D, C), dtype=np.uint8), order=np.full((D, C), -1, dtype=np.int32), cost=np.zeros((D, C)), ll_doc=np.zeros(D),
                   unexplained=np.zeros(D), iters=np.zeros(D, dtype=np.int64))
    before = None
    if not catalogue_in_lds:
        before = ctx.get_tuning()
        t = _lib.TuningOpts.from_buffer_copy(before)
        t.disable |= _lib.OFF["refit_lds"]
        check(lib().mmm_ctx_set_tuning(ctx.h, _lib.C.byref(t)), ctx.h, "mmm_ctx_set_tuning")
    try:
        rc = lib().mmm_refit_exposures(ctx.h, int(D), C, int(V), doc_ptr, _ptr(term), _ptr(count), cat.ravel(), _ptr(allowed), _ptr(penalty), int(maxiter),
                                       float(tol), _ptr(out["w"]), *[_ptr(out.get(k)) for k in ("active", "order", "cost", "ll_doc", "unexplained", "iters")])
    finally:
        if before is not None:
            check(lib().mmm_ctx_set_tuning(ctx.h, _lib.C.byref(before)), ctx.h, "mmm_ctx_set_tuning")
    check(rc, ctx.h, "mmm_refit_exposures")
    return out


def _catalogue(catalogue, modality):
    """-> (names or None, [C, V] array) from an array, the (names, terms, S) of read_signatures_tsv or a fitted LDA / MMCTM"""
    _reject_factorised(catalogue, "refit_exposures")
    if isinstance(catalogue, (LDA, MMCTM)):
        return None, _signatures_of(catalogue, modality, "catalogue")
    if isinstance(catalogue, tuple) and len(catalogue) == 3 and not np.isscalar(catalogue[0]) and len(catalogue[0]) and isinstance(catalogue[0][0], str):
        names, _, S = catalogue
        S = _values(S, "catalogue", (2,))
        if len(names) != S.shape[0]:
            raise ValueError("the catalogue has %d names and %d rows" % (len(names), S.shape[0]))
        return list(names), S
    return None, _values(catalogue, "catalogue", (2,))


def _allowed(allowed, names, D, C):
    if allowed is None:
        return None
    if len(allowed) and all(isinstance(a, str) for a in allowed):
        if names is None:
            raise ValueError("allowed holds names but the catalogue came without names")
        unknown = [a for a in allowed if a not in names]
        if unknown:
            raise ValueError("allowed names a signature the catalogue lacks: %r" % unknown[0])
        mask = np.zeros(C, dtype=np.uint8)
        mask[[names.index(a) for a in allowed]] = 1
        return np.ascontiguousarray(np.broadcast_to(mask, (D, C)))
    a = np.asarray(allowed)
    if a.shape == (C,):
        return np.ascontiguousarray(np.broadcast_to(a != 0, (D, C)), dtype=np.uint8)
    if a.shape == (D, C):
        return np.ascontiguousarray(a != 0, dtype=np.uint8)
    raise ValueError("allowed must be a length-C mask, a list of names or a D x C mask (C = %d, D = %d), got shape %r" % (C, D, a.shape))


def refit_exposures(X, catalogue, penalty="bic", allowed=None, maxiter=1000, tol=1e-9, modality=None, bootstrap=0, seed=None, q=(0.025, 0.5, 0.975),
                    ctx=None):
    """Exposures of the samples X to the signatures of `catalogue`, sparse per sample -> RefitResult.

    X as LDA takes it (a list of W_d x 2 matrices, 1-based terms, or a PackedCorpus), or MMCTM-nested (X[d][m]) with `modality=m`.
    catalogue: a [C, V] array (one row per signature, rows need not be normalised), the (names, terms, S) `read_signatures_tsv` returns
    (the names are kept), or a fitted LDA / MMCTM (the columns of β; ϕ of `modality`).  C <= 256.
    penalty: the log-likelihood a removal may cost -- "bic": 0.5 log N_d per sample; a float: the same for every sample; None: no
    elimination, the plain fit under the allowed signatures.  Under "bic" a sample with ONE mutation has the penalty 0.5 log 1 = 0: a
    signature leaves it only where the removal does not lower the log-likelihood at all (Δ < 0), so such a sample may keep several
    signatures; pass a float to decide otherwise.  allowed: a length-C mask or a list of names (shared by all samples), a D x C
    mask, or None.  maxiter, tol: of every EM fit (stop when no weight moves by tol or more).
    bootstrap=B: intervals on the CHOSEN sets -- every sample's counts are resampled B times (`mmm_resample_counts`, `seed`), the B x D
    replicate samples are refitted in ONE call with the sample's chosen set as `allowed` and no penalty, and summarised by
    `mmm_replicate_summary` at the quantiles q.  No model handle is created.  ILDA / IMMCTM catalogues: TypeError (factorised tables)."""
    ctx = ctx or (catalogue.ctx if isinstance(catalogue, (LDA, MMCTM)) else _lib.default_context())
    names, cat = _catalogue(catalogue, modality)
    C, V = cat.shape
    if C < 1 or V < 1:
        raise ValueError("the catalogue must have at least one signature and one term")
    if C > MAX_CATALOGUE:
        raise ValueError("C = %d catalogue signatures (limit %d)" % (C, MAX_CATALOGUE))
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
        stream = int(modality)
    else:
        doc_ptr, term, count = pack_lda(X)
        stream = 0
    if term.size and int(term.max()) >= V:
        raise ValueError("X holds term %d, the catalogue has %d terms" % (int(term.max()) + 1, V))
    N = np.zeros(D)
    np.add.at(N, np.repeat(np.arange(D), np.diff(doc_ptr)), count.astype(np.float64))
    if penalty is None:
        pen = None
    elif isinstance(penalty, str):
        if penalty != "bic":
            raise ValueError("penalty must be \"bic\", a float or None")
        pen = 0.5 * np.log(np.maximum(N, 1.0))
    else:
        if not (np.isfinite(float(penalty)) and float(penalty) >= 0):
            raise ValueError("penalty must be finite and >= 0")
        pen = np.full(D, float(penalty))
    al = _allowed(allowed, names, D, C)
    r = _raw(ctx, D, V, doc_ptr, term, count, cat, al, pen, maxiter, tol)
    intervals = None
    B = int(bootstrap)
    if B < 0:
        raise ValueError("bootstrap must be >= 0")
    if B:
        if seed is None:
            raise ValueError("bootstrap=B needs a seed")
        nnz = int(doc_ptr[-1])
        rc = _resample_csr(ctx, D, doc_ptr, count, B, 0, seed, stream)
        dps = np.concatenate([(doc_ptr[:-1][None, :] + nnz * np.arange(B, dtype=np.int64)[:, None]).ravel(), [B * nnz]])
        rb = _raw(ctx, B * D, V, dps, np.tile(term, B), rc.ravel(), cat, np.tile(r["active"], (B, 1)), None, maxiter, tol, outputs="w")
        mean, sd, quant = replicate_summary(rb["w"].reshape(B, D, C), q, ctx=ctx)
        intervals = RefitIntervals(mean.T.copy(), sd.T.copy(), quant.transpose(0, 2, 1).copy(), tuple(float(v) for v in np.atleast_1d(q)), B)
    expo = r["w"].T.copy()
    return RefitResult(expo, r["active"].T.astype(bool), r["order"], r["cost"], r["ll_doc"], r["unexplained"], r["iters"], expo * N[None, :], intervals,
                       names)
