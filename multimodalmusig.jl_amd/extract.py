"""Extraction of NEW signatures beside a fixed catalogue ("fit and extract"): the well-known catalogue signatures are held, only the few rows
the catalogue lacks are learned -- the step between the two modes the package had, fully de novo (LDA / MMCTM: every topic free) and fully
fixed (`refit_exposures`: every row given).  Without a catalogue it is plain KL-NMF / pLSA extraction.

All restarts run in one launch (`mmm_extract_signatures`), one workgroup per restart; the restart with the largest log-likelihood is
returned, the others say how stable its new rows are (`consensus=True`).  The definition, down to the order of every sum, is in
include/mmmusig.h: the same arguments give the same bits on every run.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .bootstrap import _is_nested
from .match import _values, signature_consensus
from .refit import _allowed, _catalogue
from .utils import pack_lda

MAX_ROWS = 256            # fixed + new rows
MAX_NEW = 32              # new rows
W_ALL_LIMIT = 1 << 24     # doubles of w [R, D, K] that are downloaded for all restarts; beyond it the best restart runs again alone

_Extraction = namedtuple("Extraction", "signatures exposures ll best ll_all iters all_signatures unexplained names stability fixed")


class Extraction(_Extraction):
    """signatures: [J, V] the new rows of the best restart (each sums to 1); exposures: [D, K] its weights, fixed rows first; ll: its
    log-likelihood; best: its index (the largest ll, ties to the lowest); ll_all, iters: [R] of every restart; all_signatures: [R, J, V];
    unexplained: [D] mutations in terms no row of the sample produces; names: the K row names, the catalogue's first, then "NEW1", ...;
    stability: with consensus=True [J] the mean cosine of the other restarts' matched rows, else None; fixed: the [F, V] catalogue rows as
    given."""
    __slots__ = ()

    def catalogue(self):
        """(names, None, [K, V] table), fixed rows first, in the form `read_signatures_tsv` returns: `refit_exposures`,
        `signature_presence` and `decompose_signatures` take it unchanged"""
        return list(self.names), None, np.concatenate([self.fixed, self.signatures], axis=0)


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _raw(ctx, D, V, doc_ptr, term, count, cat, J, allowed=None, R=1, r0=0, seed=0, stream=0, init=None, maxiter=1000, tol=1e-7, waves=0,
         outputs=("w", "ll_doc", "unexplained")):
    """mmm_extract_signatures on one CSR corpus (0-based terms) -> dict of sig [R, J, V], ll [R], iters [R] and, where asked for, w [R, D, K],
    ll_doc, unexplained [R, D].  cat: [F, V] or None."""
    F = 0 if cat is None else int(np.shape(cat)[0])
    cat = None if F == 0 else np.ascontiguousarray(cat, dtype=np.float64)
    K = F + int(J)
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    term = np.ascontiguousarray(term, dtype=np.int32); count = np.ascontiguousarray(count, dtype=np.int32)
    if allowed is not None:
        allowed = np.ascontiguousarray(allowed, dtype=np.uint8)
        if allowed.shape != (D, F):
            raise ValueError("allowed must be [D, F] = [%d, %d], got %r" % (D, F, allowed.shape))
    if init is not None:
        init = np.ascontiguousarray(init, dtype=np.float64)
        if init.shape != (R, J, V):
            raise ValueError("init must be [R, J, V] = [%d, %d, %d], got %r" % (R, J, V, init.shape))
    out = {"sig": np.zeros((R, J, V)), "ll": np.zeros(R), "iters": np.zeros(R, dtype=np.int32)}
    if "w" in outputs:
        out["w"] = np.zeros((R, D, K))
    for k in ("ll_doc", "unexplained"):
        if k in outputs:
            out[k] = np.zeros((R, D))
    # an empty array still needs an address: NULL says "not given"
    one = np.zeros(1)
    addr = lambda a: a.ctypes.data if a.size else one.ctypes.data
    rc = lib().mmm_extract_signatures(ctx.h, int(D), F, int(J), int(V), doc_ptr, _ptr(term), _ptr(count), _ptr(cat), _ptr(allowed), int(R), int(r0),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), None if init is None else addr(init), int(maxiter), float(tol), int(waves),
                                      addr(out["sig"]), addr(out["w"]) if "w" in out else None, addr(out["ll"]),
                                      addr(out["ll_doc"]) if "ll_doc" in out else None, addr(out["unexplained"]) if "unexplained" in out else None,
                                      addr(out["iters"]))
    check(rc, ctx.h, "mmm_extract_signatures")
    return out


def extract_signatures(X, catalogue=None, n_new=1, restarts=64, seed=0, allowed=None, init=None, maxiter=1000, tol=1e-7, consensus=False, names=None,
                       ctx=None):
    """New signatures of the samples X beside the FIXED rows of `catalogue` -> Extraction.

    X as LDA takes it (a list of W_d x 2 matrices, 1-based terms, or a PackedCorpus).  catalogue: as `refit_exposures` takes it (an [F, V]
    array, the (names, terms, S) of `read_signatures_tsv`, a fitted LDA), or None: every row is new and the number of terms is the largest
    term of X.  n_new: J <= 32 new rows, F + J <= 256.  restarts: R random starts (Philox words of
    (seed, restart index): restart r of any call with the same seed starts from the same rows), or the rows of init [R, J, V].  allowed: which
    FIXED rows a sample may use -- a length-F mask or a list of names (shared), a D x F mask, or None; new rows are always allowed.
    maxiter, tol: a restart stops when no weight and no entry of a new row moves by tol or more.  consensus=True (J >= 1, R >= 2): the
    restarts' new rows are matched to the best restart's and `stability` holds their mean cosine (`mmm_signature_consensus`).  names: of the
    fixed rows, where the catalogue came without.  Compare J = 0, 1, 2, ... by `ll` to choose the number of new rows."""
    if _is_nested(X):
        raise ValueError("an MMCTM-nested X holds one corpus per modality: pass one modality's corpus")
    J, R = int(n_new), int(restarts)
    if catalogue is None:
        cat_names, cat = None, None
        F = 0
    else:
        cat_names, cat = _catalogue(catalogue, None)
        F = cat.shape[0]
    if names is not None:
        if len(names) != F or not all(isinstance(s, str) for s in names):
            raise ValueError("names must hold one string per fixed row (%d)" % F)
        cat_names = list(names)
    if J < 0 or J > MAX_NEW:
        raise ValueError("n_new = %d new signatures (0 .. %d)" % (J, MAX_NEW))
    if F + J < 1 or F + J > MAX_ROWS:
        raise ValueError("F + n_new = %d rows (1 .. %d)" % (F + J, MAX_ROWS))
    if R < 1:
        raise ValueError("restarts must be >= 1")
    if int(maxiter) < 1 or not float(tol) >= 0:
        raise ValueError("maxiter must be >= 1 and tol >= 0")
    if consensus and (J < 1 or R < 2):
        raise ValueError("consensus=True needs n_new >= 1 and restarts >= 2")
    doc_ptr, term, count = pack_lda(X)
    D = len(doc_ptr) - 1
    if cat is None:
        V = int(term.max()) + 1 if term.size else 1
        if init is not None and np.ndim(init) == 3:
            V = max(V, np.shape(init)[2])
    else:
        V = cat.shape[1]
        if V < 1:
            raise ValueError("the catalogue must have at least one term")
    if term.size and int(term.max()) >= V:
        raise ValueError("X holds term %d, the catalogue has %d terms" % (int(term.max()) + 1, V))
    al = _allowed(allowed, cat_names, D, F) if F else None
    if init is not None:
        init = _values(init, "init", (3,))
        if init.shape != (R, J, V):
            raise ValueError("init must be [restarts, n_new, V] = [%d, %d, %d], got %r" % (R, J, V, init.shape))
        if J and not (init.sum(axis=2) > 0).all():
            raise ValueError("init holds a row that sums to 0")
    ctx = ctx or _lib.default_context()
    K = F + J
    all_w = R * D * K <= W_ALL_LIMIT
    r = _raw(ctx, D, V, doc_ptr, term, count, cat, J, al, R, 0, seed, 0, init, maxiter, tol, outputs=("w", "unexplained") if all_w else ())
    best = int(np.argmax(r["ll"]))                      # ties: the lowest r
    if all_w:
        w, unex = r["w"][best], r["unexplained"][best]
    else:                                               # restart `best` alone: a slice of the same call, bit for bit
        one = _raw(ctx, D, V, doc_ptr, term, count, cat, J, al, 1, best, seed, 0, None if init is None else init[best:best + 1], maxiter, tol,
                   outputs=("w", "unexplained"))
        w, unex = one["w"][0], one["unexplained"][0]
    stability = None
    if consensus:
        stability = signature_consensus(r["sig"], best, q=(), ctx=ctx).stability
    fixed_names = cat_names if cat_names is not None else ["FIXED%d" % (i + 1) for i in range(F)]
    return Extraction(r["sig"][best].copy(), w.copy(), float(r["ll"][best]), best, r["ll"], r["iters"], r["sig"], unex.copy(),
                      list(fixed_names) + ["NEW%d" % (j + 1) for j in range(J)], stability, np.zeros((0, V)) if cat is None else cat)
