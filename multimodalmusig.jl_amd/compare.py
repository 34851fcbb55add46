"""Did the exposures change between a tumour's two mutation sets -- clonal and subclonal, early and late, primary and relapse, before and after
therapy -- for which signatures, and with what p-value?

Refitting the two tables separately and looking at the difference has no null distribution: a set of 40 mutations shows large differences
by chance alone.  Here the honest test is also exact.  Under H0 the two sets are draws from one mixture, so given the pooled counts the
partition into sets of sizes N_a and N_b is a uniform random subset, whatever was fitted.  A replicate deals N_a of the N pooled mutations
to set a (`mmm_deal_counts`' dealing: one Philox word per mutation, the N_a smallest keys), refits both sets under the sample's allowed
signatures and compares T = ll_a + ll_b and every |w^a_c - w^b_c| with the observed values; the maximum over the sample's signatures gives
single-step Westfall-Young adjusted p-values per signature.  All of it runs in one call (`mmm_compare_exposures`); the replicates' counts
never leave the device's LDS.  The definition, down to the order of every sum, is in include/mmmusig.h.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .associate import benjamini_hochberg
from .bootstrap import _is_nested, _modality_csr
from .ctm import MMCTM
from .models import LDA
from .refit import MAX_CATALOGUE, RefitResult, _allowed, _catalogue
from .simulate import MAX_TERMS, _seeds
from .utils import PackedCorpus, pack_lda, pack_mm

MAX_SAMPLES = 2 ** 28          # the sample shares a Philox counter word with the dealing's tag

_ComparisonResult = namedtuple("ComparisonResult", "p stat exposures_a exposures_b exposures_pooled delta p_signature p_adjusted count_ge count_sig count_max "
                               "status unexplained iters B replicates names")


class ComparisonResult(_ComparisonResult):
    """p [D] = (1 + count_ge) / (B + 1): the permutation p-value of the sample's statistic T = ll_a + ll_b, NaN where the sample is untestable
    (and with B = 0); stat [D] = max(2 (T_obs - ll_pooled), 0), the likelihood-ratio form of T; exposures_a, exposures_b, exposures_pooled
    [C, D]: the weights of the three fits (exactly 0 outside the sample's allowed set); delta [C, D] = |exposures_a - exposures_b|;
    p_signature [C, D] = (1 + count_sig) / (B + 1) per signature, unadjusted; p_adjusted [C, D] = (1 + count_max) / (B + 1): adjusted over
    the signatures of the sample by the permutation distribution of the largest difference (single-step max-T); both NaN outside the
    allowed set; count_ge [D], count_sig, count_max [C, D]: the replicates at least as extreme as the observed value; status [D]: 0
    tested, 3 untestable (one of the sets is empty, or nothing is allowed); unexplained [D]: pooled mutations on terms none of the
    allowed signatures produces (they drop out of every log-likelihood alike); iters [D]: EM iterations of all the sample's fits;
    replicates: [B, D] 2 (T_b - ll_pooled) with keep_replicates (NaN where untestable), else None; names: the catalogue's names or None."""
    __slots__ = ()

    @property
    def q(self):
        """[D] Benjamini-Hochberg q-values of p over the tested samples (NaN elsewhere)"""
        q = np.full(self.p.shape, np.nan)
        ok = ~np.isnan(self.p)
        if ok.any():
            q[ok] = benjamini_hochberg(self.p[ok])
        return q

    def changed(self, alpha=0.05):
        """indices of the samples with p <= alpha"""
        with np.errstate(invalid="ignore"):
            return np.flatnonzero(np.nan_to_num(self.p, nan=np.inf) <= float(alpha))

    def changed_signatures(self, alpha=0.05):
        """the (sample, signature) pairs with p_adjusted <= alpha, signatures by name where the catalogue has names"""
        with np.errstate(invalid="ignore"):
            c, d = np.nonzero(np.nan_to_num(self.p_adjusted, nan=np.inf) <= float(alpha))
        order = np.lexsort((c, d))
        return [(int(d[i]), self.names[c[i]] if self.names is not None else int(c[i])) for i in order]


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _corpus(X, modality, what):
    """-> (D, doc_ptr, term, count), 0-based terms"""
    D = len(X)
    if _is_nested(X):
        if modality is None:
            raise ValueError("an MMCTM-nested %s holds one corpus per modality: pass modality=m" % what)
        M = X.M if isinstance(X, PackedCorpus) else len(X[0])
        if not 0 <= int(modality) < M:
            raise ValueError("modality %d of %d" % (int(modality), M))
        dp_all, term_all, count_all = pack_mm(X, M)
        doc_ptr, count, e0 = _modality_csr(dp_all, count_all, D, int(modality))
        return D, doc_ptr, term_all[e0:e0 + count.size], count
    return (D,) + tuple(pack_lda(X))


def _deal_raw(ctx, D, doc_ptr, count, n_a, B, b0=0, seed=0, stream=0, key_bits=32):
    """mmm_deal_counts on one CSR corpus -> int32 [B, nnz].  key_bits below 32: the header's test hook."""
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    n_a = np.ascontiguousarray(n_a, dtype=np.int32)
    out = np.zeros((int(B), count.size), dtype=np.int32)
    check(lib().mmm_deal_counts(ctx.h, int(D), doc_ptr, _ptr(count), _ptr(n_a), int(B), int(b0), int(seed), int(stream), int(key_bits), _ptr(out)), ctx.h,
          "mmm_deal_counts")
    return out


def deal_counts(X, n_a, B, seed, stream=0, b0=0, ctx=None, V=None):
    """B random subsets of every sample's mutations, of FIXED size: [B, D, V] counts, replicate b of sample d holding n_a[d] of the sample's
    mutations, every subset of that size equally likely (`split_counts` deals into folds of RANDOM size, another distribution).  X as LDA
    takes it; the mutations are numbered in term order of the dense count vector (duplicate terms summed), as `compare_exposures` numbers
    the pooled mutations, so `deal_counts(pooled, N_a, B, seed, stream, b0)` gives the set-a vectors of its replicates b0 .. b0 + B - 1; set b
    is the rest.  V: the number of terms (default: the largest term of X).  Integer throughout and reproducible: chunked calls are slices
    of one big call."""
    D, doc_ptr, term, count = _corpus(X, None, "X")
    top = int(term.max()) + 1 if term.size else 0
    V = max(top, 1) if V is None else int(V)
    if V < top:
        raise ValueError("X holds term %d, V = %d" % (top, V))
    n_a = np.asarray(n_a)
    if n_a.shape != (D,) or (n_a != np.floor(n_a)).any():
        raise ValueError("n_a must hold one integer per sample")
    B, b0, seed, stream = _seeds(B, b0, seed, stream)
    if stream >= 2 ** 31:
        raise ValueError("stream must be below 2^31")
    if D > MAX_SAMPLES:
        raise ValueError("D = %d samples (limit 2^28)" % D)
    dense = np.zeros((D, V), dtype=np.int64)
    np.add.at(dense, (np.repeat(np.arange(D), np.diff(doc_ptr)), term), count)
    N = dense.sum(axis=1)
    if (N >= 2 ** 31).any():
        raise ValueError("a sample holds 2^31 or more mutations")
    if ((n_a < 0) | (n_a > N)).any():
        raise ValueError("n_a[%d] is outside [0, N_d]" % int(np.flatnonzero((n_a < 0) | (n_a > N))[0]))
    ctx = ctx or _lib.default_context()
    d_idx, v_idx = np.nonzero(dense)                 # row-major: per sample the terms ascending, without duplicates
    dp = np.concatenate([[0], np.cumsum((dense > 0).sum(axis=1))]).astype(np.int64)
    r = _deal_raw(ctx, D, dp, dense[d_idx, v_idx], n_a, B, b0, seed, stream)
    out = np.zeros((B, D, V), dtype=np.int64)
    out[:, d_idx, v_idx] = r
    return out


def _raw(ctx, D, V, a, b, cat, allowed=None, B=0, b0=0, seed=0, stream=0, maxiter=1000, tol=1e-9, keep=False, key_bits=32, catalogue_in_lds=True):
    """mmm_compare_exposures on two CSR corpora a, b = (doc_ptr, term, count) (0-based terms) -> dict of its outputs ([D] / [D, C] / [B, D]).
    key_bits below 32: the header's test hook.  catalogue_in_lds=False (tests): the replicate launch reads the catalogue through L2 even
    where a sample's rows fit LDS."""
    cat = np.ascontiguousarray(cat, dtype=np.float64)
    C = cat.shape[0]
    pa, ta, ca = np.ascontiguousarray(a[0], dtype=np.int64), np.ascontiguousarray(a[1], dtype=np.int32), np.ascontiguousarray(a[2], dtype=np.int32)
    pb, tb, cb = np.ascontiguousarray(b[0], dtype=np.int64), np.ascontiguousarray(b[1], dtype=np.int32), np.ascontiguousarray(b[2], dtype=np.int32)
    if allowed is not None:
        allowed = np.ascontiguousarray(allowed, dtype=np.uint8)
        if allowed.shape != (D, C):
            raise ValueError("allowed must be [D, C] = [%d, %d], got %r" % (D, C, allowed.shape))
    out = dict(w_a=np.zeros((D, C)), w_b=np.zeros((D, C)), w_pool=np.zeros((D, C)), stat=np.zeros(D), count_ge=np.zeros(D, dtype=np.int32),
               count_sig=np.zeros((D, C), dtype=np.int32), count_max=np.zeros((D, C), dtype=np.int32), status=np.zeros(D, dtype=np.int8),
               unexplained=np.zeros(D), iters=np.zeros(D, dtype=np.int64), rep_stat=np.zeros((B, D)) if keep else None)
    before = None
    if not catalogue_in_lds:
        before = ctx.get_tuning()
        t = _lib.TuningOpts.from_buffer_copy(before)
        t.disable |= _lib.OFF["refit_lds"]
        check(lib().mmm_ctx_set_tuning(ctx.h, _lib.C.byref(t)), ctx.h, "mmm_ctx_set_tuning")
    try:
        rc = lib().mmm_compare_exposures(ctx.h, int(D), C, int(V), pa, _ptr(ta), _ptr(ca), pb, _ptr(tb), _ptr(cb), cat.ravel(), _ptr(allowed), int(B), int(b0),
                                         int(seed), int(stream), int(key_bits), int(maxiter), float(tol),
                                         *[_ptr(out[k]) for k in ("w_a", "w_b", "w_pool", "stat", "count_ge", "count_sig", "count_max", "status", "unexplained",
                                                                  "iters", "rep_stat")])
    finally:
        if before is not None:
            check(lib().mmm_ctx_set_tuning(ctx.h, _lib.C.byref(before)), ctx.h, "mmm_ctx_set_tuning")
    check(rc, ctx.h, "mmm_compare_exposures")
    return out


def compare_exposures(X_a, X_b, catalogue, allowed=None, B=1000, seed=None, stream=0, b0=0, maxiter=1000, tol=1e-9, modality=None, keep_replicates=False,
                      ctx=None):
    """Per-sample exact permutation test of H0: the two mutation sets of the sample are draws from ONE mixture of the catalogue's signatures
    -> ComparisonResult.

    X_a, X_b: the two tables over the same samples, each as `refit_exposures` takes X; catalogue as there (C <= 256; here also V <= 4096).
    allowed: as in `refit_exposures`, or a `RefitResult`, whose chosen sets are then used.  Recommended: the refit of the POOLED table -- a
    selection made on the pooled counts is the same under every permutation of the mutations between the two sets, so the test stays
    exact; a selection made on one of the two sets, or on each separately, has seen the partition and the p-values are no longer exact.
    B: permutations per sample; p = (1 + #{T_b >= T_obs}) / (B + 1), and likewise per signature for |w^a_c - w^b_c| (`p_signature`) and
    for its maximum over the sample's signatures (`p_adjusted`).  Replicates b0 .. b0 + B - 1 of the sequence that (seed, stream) fixes:
    the counts of chunked calls add.  seed is required when B > 0.  A replicate's set a is `deal_counts(pooled, N_a, ...)` under the same
    seed and stream.  keep_replicates: return the [B, D] statistics.  A sample with an empty set or with nothing allowed is untestable:
    status 3, p NaN.  ILDA / IMMCTM catalogues: TypeError (factorised tables)."""
    names, cat = _catalogue(catalogue, modality)
    C, V = cat.shape
    if C < 1 or V < 1:
        raise ValueError("the catalogue must have at least one signature and one term")
    if C > MAX_CATALOGUE:
        raise ValueError("C = %d catalogue signatures (limit %d)" % (C, MAX_CATALOGUE))
    if V > MAX_TERMS:
        raise ValueError("V = %d terms (limit %d)" % (V, MAX_TERMS))
    B = int(B)
    if B > 0 and seed is None:
        raise ValueError("B > 0 replicates need a seed")
    B, b0, seed, stream = _seeds(B, b0, 0 if seed is None else seed, stream)
    if stream >= 2 ** 31:
        raise ValueError("stream must be below 2^31")
    if int(maxiter) < 1 or not float(tol) >= 0:
        raise ValueError("maxiter must be >= 1 and tol >= 0")
    D, pa, ta, ca = _corpus(X_a, modality, "X_a")
    Db, pb, tb, cb = _corpus(X_b, modality, "X_b")
    if Db != D:
        raise ValueError("X_a holds %d samples, X_b %d" % (D, Db))
    if D > MAX_SAMPLES:
        raise ValueError("D = %d samples (limit 2^28)" % D)
    for t, what in ((ta, "X_a"), (tb, "X_b")):
        if t.size and int(t.max()) >= V:
            raise ValueError("%s holds term %d, the catalogue has %d terms" % (what, int(t.max()) + 1, V))
    if isinstance(allowed, RefitResult):
        if allowed.active.shape != (C, D):
            raise ValueError("the RefitResult holds %r chosen sets, not C x D = %d x %d" % (allowed.active.shape, C, D))
        al = np.ascontiguousarray(allowed.active.T, dtype=np.uint8)
    else:
        al = _allowed(allowed, names, D, C)
    ctx = ctx or (catalogue.ctx if isinstance(catalogue, (LDA, MMCTM)) else _lib.default_context())      # every argument is checked before a device is asked for
    r = _raw(ctx, D, V, (pa, ta, ca), (pb, tb, cb), cat, al, B, b0, seed, stream, maxiter, tol, keep=bool(keep_replicates))
    status = r["status"]
    on = (np.ones((D, C), dtype=bool) if al is None else al != 0) & (status == 0)[:, None]

    def pval(count, mask):
        p = (1.0 + count) / (B + 1.0) if B else np.full(count.shape, np.nan)
        return np.where(mask, p, np.nan)

    wa, wb = r["w_a"].T.copy(), r["w_b"].T.copy()
    return ComparisonResult(pval(r["count_ge"], status == 0), r["stat"], wa, wb, r["w_pool"].T.copy(), np.abs(wa - wb), pval(r["count_sig"], on).T.copy(),
                            pval(r["count_max"], on).T.copy(), r["count_ge"], r["count_sig"].T.copy(), r["count_max"].T.copy(), status, r["unexplained"], r["iters"], B,
                            r["rep_stat"] if keep_replicates else None, names)
