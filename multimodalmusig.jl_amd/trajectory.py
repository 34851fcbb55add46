"""Where along a tumour's ordered mutations do the exposures change, how many times, and is that more than chance?

The mutations of a tumour are ordered -- by cancer cell fraction, by inferred timing -- and cut into bins (`bin_by_order`).  `exposure_trajectory`
fits every run of consecutive bins once (the segment table), picks the change points by optimal partitioning under a penalty per change
point, and tests the best single cut by the exact permutation of `compare_exposures`: under H0 the exposures are constant along the
timeline, so given the pooled counts the assignment of the mutations to the bins is uniform.  A replicate deals every prefix of the
timeline from ONE set of keys, refits both sides of every cut and keeps the best; the counts never leave the device's LDS.  All of it runs
in one call (`mmm_exposure_trajectory`).  The definition, down to the order of every sum, is in include/mmmusig.h.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .associate import benjamini_hochberg
from .compare import MAX_SAMPLES, _corpus, _ptr
from .ctm import MMCTM
from .models import LDA
from .refit import MAX_CATALOGUE, RefitResult, _allowed, _catalogue
from .simulate import MAX_TERMS, _seeds

MAX_BINS = 128                 # MMM_TRAJECTORY_MAX_BINS

_TrajectoryResult = namedtuple("TrajectoryResult", "p stat cut p_cut n_changepoints changepoints p_changepoint exposures_segment exposures_bin best gain count_ge "
                               "count_cut status unexplained iters B replicates names seg_ll bin_ptr")


class TrajectoryResult(_TrajectoryResult):
    """p [D] = (1 + count_ge) / (B + 1): the permutation p-value of the best single cut of the sample's timeline, corrected for the search
    over the cuts; NaN unless status is 0 (and with B = 0).  stat [D] = max(2 (G_max - ll_0T), 0); cut [D]: the bin the second part starts
    with (-1 where there is no scan).  p_cut [D][T_d]: per cut (1 + count_cut) / (B + 1), adjusted over the cuts by the permutation
    distribution of the best one (single-step max-T); NaN where t is no cut.  n_changepoints [D], changepoints [D, max_changepoints] (the
    first bin of every later segment, -1 beyond): the optimal partitioning under the penalty.  p_changepoint [D, max_changepoints]: with
    changepoint_tests, the scan p-value of every chosen change point inside its window (NaN beyond, and without the tests).
    exposures_segment [D][n_changepoints + 1, C]; exposures_bin [D][T_d, C]; best [D, max_changepoints + 1]: the selection curve F_m(T);
    gain [D][T_d] = G_t - ll_0T per cut.  status [D]: 0 tested, 1 timeline shorter than 2 min_len (partitioned, not tested), 3 no mutation or
    nothing allowed.  unexplained [D]: mutations on terms none of the allowed signatures produces; iters [D]: EM iterations of the table's and
    the replicates' fits; replicates: [B, D] 2 (G_max,b - ll_0T) with keep_replicates, else None; names: the catalogue's names or None;
    seg_ll: the segment table as the C entry lays it out; bin_ptr [D + 1]."""
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

    def segments(self, d):
        """the chosen segments of sample d -> a list of (first_bin, end_bin, exposures [C]), end_bin exclusive"""
        d = int(d)
        T = int(self.bin_ptr[d + 1] - self.bin_ptr[d])
        k = int(self.n_changepoints[d])
        if self.status[d] == 3:
            return []
        b = [0] + [int(t) for t in self.changepoints[d, :k]] + [T]
        return [(b[i], b[i + 1], self.exposures_segment[d][i]) for i in range(k + 1)]


def bin_by_order(terms, key, bin_size=100, descending=True):
    """Cut every sample's mutations into a timeline of bins of `bin_size` mutations along an ordering key (the cancer cell fraction: clonal
    first with descending=True).  terms, key: per sample the term (1-based, as the corpora hold them) and the key of every mutation.  The
    order is stable (equal keys keep their input order); the last bin takes the remainder.  -> a [D] list of [T_d] lists of W x 2
    (term, count) matrices, as `exposure_trajectory` takes a timeline.  Pure numpy."""
    bin_size = int(bin_size)
    if bin_size < 1:
        raise ValueError("bin_size must be >= 1")
    if len(terms) != len(key):
        raise ValueError("terms holds %d samples, key %d" % (len(terms), len(key)))
    out = []
    for d, (t, k) in enumerate(zip(terms, key)):
        t = np.asarray(t, dtype=np.int64).ravel()
        k = np.asarray(k, dtype=np.float64).ravel()
        if t.shape != k.shape:
            raise ValueError("sample %d: %d terms, %d keys" % (d, t.size, k.size))
        if np.isnan(k).any():
            raise ValueError("sample %d: a key is NaN" % d)
        if t.size and t.min() < 1:
            raise ValueError("sample %d: terms are 1-based" % d)
        o = np.argsort(-k if descending else k, kind="stable")
        bins = []
        for s in range(0, t.size, bin_size):
            v, c = np.unique(t[o[s:s + bin_size]], return_counts=True)
            bins.append(np.stack([v, c], axis=1).astype(np.int64))
        out.append(bins)
    return out


def _timeline(timeline, modality):
    """-> (D, nbins, bin_ptr, doc_ptr, term, count), 0-based terms"""
    if isinstance(timeline, np.ndarray):
        if timeline.ndim != 3:
            raise ValueError("a dense timeline is [D, T, V], got %r" % (timeline.shape,))
        if (timeline < 0).any() or (timeline != np.floor(timeline)).any():
            raise ValueError("a dense timeline holds counts: integers >= 0")
        D, T, _ = timeline.shape
        flat = [np.stack([np.flatnonzero(r) + 1, r[np.flatnonzero(r)]], axis=1).astype(np.int64) for r in timeline.reshape(D * T, -1)]
        sizes = [T] * D
    else:
        sizes = [len(s) for s in timeline]
        flat = [b for s in timeline for b in s]
        D = len(sizes)
    bin_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if max(sizes, default=0) > MAX_BINS:
        raise ValueError("a timeline of %d bins (limit %d)" % (max(sizes), MAX_BINS))
    if not flat:
        return D, 0, bin_ptr, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)
    nb, dp, term, count = _corpus(flat, modality, "timeline")
    return D, nb, bin_ptr, dp, term, count


def _raw(ctx, D, V, nbins, doc_ptr, term, count, bin_ptr, cat, allowed=None, min_len=1, max_cp=8, penalty=None, B=0, b0=0, seed=0, stream=0, maxiter=1000,
         tol=1e-9, keep=False, key_bits=32, bins=True, catalogue_in_lds=True):
    """mmm_exposure_trajectory on a CSR corpus of bins (0-based terms) -> dict of its outputs.  key_bits below 32: the header's test hook.
    catalogue_in_lds=False (tests): the replicate launch reads the catalogue through L2 even where a sample's rows fit LDS."""
    cat = np.ascontiguousarray(cat, dtype=np.float64)
    C = cat.shape[0]
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64); bin_ptr = np.ascontiguousarray(bin_ptr, dtype=np.int64)
    term = np.ascontiguousarray(term, dtype=np.int32); count = np.ascontiguousarray(count, dtype=np.int32)
    penalty = np.ascontiguousarray(np.zeros(D) if penalty is None else penalty, dtype=np.float64)
    if penalty.shape != (D,):
        raise ValueError("penalty must hold one value per sample")
    if allowed is not None:
        allowed = np.ascontiguousarray(allowed, dtype=np.uint8)
        if allowed.shape != (D, C):
            raise ValueError("allowed must be [D, C] = [%d, %d], got %r" % (D, C, allowed.shape))
    T = np.diff(bin_ptr)
    S = int((T * (T + 1) // 2).sum())
    M = int(max_cp)
    # what the entry leaves where it writes nothing (no bins at all): every sample untestable
    out = dict(seg_ll=np.full(S, np.nan), best=np.full((D, M + 1), np.nan), n_cp=np.zeros(D, dtype=np.int32), cp=np.full((D, M), -1, dtype=np.int32),
               w_seg=np.zeros((D, M + 1, C)), w_bin=np.zeros((nbins, C)) if bins else None, gain_cut=np.full(nbins, np.nan), cut=np.full(D, -1, dtype=np.int32),
               stat=np.zeros(D), count_ge=np.zeros(D, dtype=np.int32), count_cut=np.zeros(nbins, dtype=np.int32), status=np.full(D, 3, dtype=np.int8),
               unexplained=np.zeros(D), iters=np.zeros(D, dtype=np.int64), rep_stat=np.full((B, D), np.nan) if keep else None)
    before = None
    if not catalogue_in_lds:
        before = ctx.get_tuning()
        t = _lib.TuningOpts.from_buffer_copy(before)
        t.disable |= _lib.OFF["refit_lds"]
        check(lib().mmm_ctx_set_tuning(ctx.h, _lib.C.byref(t)), ctx.h, "mmm_ctx_set_tuning")
    try:
        rc = lib().mmm_exposure_trajectory(ctx.h, int(D), C, int(V), int(nbins), doc_ptr, _ptr(term), _ptr(count), bin_ptr, cat.ravel(), _ptr(allowed), int(min_len), M,
                                           penalty, int(B), int(b0), int(seed), int(stream), int(key_bits), int(maxiter), float(tol),
                                           *[out[k].ctypes.data if out[k] is not None else None
                                             for k in ("seg_ll", "best", "n_cp", "cp", "w_seg", "w_bin", "gain_cut", "cut", "stat", "count_ge", "count_cut", "status",
                                                       "unexplained", "iters", "rep_stat")])
    finally:
        if before is not None:
            check(lib().mmm_ctx_set_tuning(ctx.h, _lib.C.byref(before)), ctx.h, "mmm_ctx_set_tuning")
    check(rc, ctx.h, "mmm_exposure_trajectory")
    return out


def exposure_trajectory(timeline, catalogue, allowed=None, min_len=1, max_changepoints=8, penalty="bic", B=1000, seed=None, stream=0, b0=0, maxiter=1000,
                        tol=1e-9, modality=None, keep_replicates=False, changepoint_tests=True, ctx=None):
    """Change points of the exposures along every sample's timeline of bins, and the exact permutation test of the best single cut
    -> TrajectoryResult.

    timeline: a [D] list of [T_d] lists of documents as `refit_exposures` takes them (`bin_by_order` makes one), or a dense [D, T, V] array
    of counts; T_d <= 128.  catalogue as in `refit_exposures` (C <= 256; here also V <= 4096).  allowed: as there, or a `RefitResult`, whose
    chosen sets are then used.  Recommended: the refit of the POOLED table (all bins of a sample summed) -- a selection made on the pooled
    counts is the same under every permutation of the mutations along the timeline, so the test stays exact.
    min_len: the shortest segment, in bins.  max_changepoints: the most change points a sample may get.  penalty: what a change point must
    gain in log-likelihood -- "bic": 0.5 (|A_d| + 1) log N_d, half a log N for each of the |A_d| - 1 free weights of the new segment, for
    the location of the change point and for one extra parameter that keeps the rule on the conservative side of the search over
    locations; a float: the same for every sample; a [D] array.
    B: permutations per sample; p = (1 + #{G_max,b >= G_max}) / (B + 1), where G_t = ll(bins before t) + ll(bins from t on) and the maximum
    runs over the cuts t in [min_len, T - min_len]: the search over the cuts is part of every replicate, so p is corrected for it, and
    p_cut holds the per-cut values adjusted the same way.  Replicates b0 .. b0 + B - 1 of the sequence that (seed, stream) fixes: the counts of
    chunked calls add.  seed is required when B > 0.  A replicate's prefix at cut t is `deal_counts(pooled, C_t, ...)` under the same seed
    and stream.  keep_replicates: return the [B, D] statistics.
    changepoint_tests: one second call tests every chosen change point on its WINDOW, the bins between the neighbouring change points
    (or the ends of the timeline), the windows stacked as samples in the order (sample, k): p_changepoint[d][k] is the window's scan
    p-value, corrected for the search inside the window.  It is CONDITIONAL on the neighbouring change points: they were chosen on the
    same data, so it is a guide to which change points carry the partition, not an unconditional level.  Needs B > 0.
    A sample without mutations or with nothing allowed has status 3, one with fewer than 2 min_len bins status 1: p NaN.  With ONE allowed
    signature every partition has the same likelihood up to rounding and the outputs of the sample say nothing.  ILDA / IMMCTM catalogues:
    TypeError (factorised tables)."""
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
    L, M = int(min_len), int(max_changepoints)
    if L < 1 or M < 0:
        raise ValueError("min_len must be >= 1 and max_changepoints >= 0")
    D, nbins, bin_ptr, dp, term, count = _timeline(timeline, modality)
    if D > MAX_SAMPLES:
        raise ValueError("D = %d samples (limit 2^28)" % D)
    if term.size and int(term.max()) >= V:
        raise ValueError("the timeline holds term %d, the catalogue has %d terms" % (int(term.max()) + 1, V))
    if isinstance(allowed, RefitResult):
        if allowed.active.shape != (C, D):
            raise ValueError("the RefitResult holds %r chosen sets, not C x D = %d x %d" % (allowed.active.shape, C, D))
        al = np.ascontiguousarray(allowed.active.T, dtype=np.uint8)
    else:
        al = _allowed(allowed, names, D, C)
    nA = np.full(D, C) if al is None else (al != 0).sum(axis=1)
    Nbin = np.add.reduceat(np.concatenate([count, [0]]).astype(np.int64), dp[:-1]) * (dp[:-1] != dp[1:]) if nbins else np.zeros(0, np.int64)
    N = np.array([Nbin[bin_ptr[d]:bin_ptr[d + 1]].sum() for d in range(D)], dtype=np.int64)
    if isinstance(penalty, str):
        if penalty != "bic":
            raise ValueError("penalty must be \"bic\", a float or one value per sample")
        pen = 0.5 * (nA + 1.0) * np.log(np.maximum(N, 1).astype(np.float64))
    else:
        pen = np.broadcast_to(np.asarray(penalty, dtype=np.float64), (D,)).copy() if np.ndim(penalty) == 0 else np.asarray(penalty, dtype=np.float64)
        if pen.shape != (D,):
            raise ValueError("penalty must be \"bic\", a float or one value per sample")
    if not (np.isfinite(pen) & (pen >= 0)).all():
        raise ValueError("a penalty is negative or not finite")
    if changepoint_tests and M > 0 and B == 0:
        changepoint_tests = False
    ctx = ctx or (catalogue.ctx if isinstance(catalogue, (LDA, MMCTM)) else _lib.default_context())      # every argument is checked before a device is asked for
    r = _raw(ctx, D, V, nbins, dp, term, count, bin_ptr, cat, al, L, M, pen, B, b0, seed, stream, maxiter, tol, keep=bool(keep_replicates))
    status = r["status"]

    def pval(cnt, mask):
        p = (1.0 + cnt) / (B + 1.0) if B else np.full(cnt.shape, np.nan)
        return np.where(mask, p, np.nan)

    sl = [slice(int(bin_ptr[d]), int(bin_ptr[d + 1])) for d in range(D)]
    p_cut_flat = pval(r["count_cut"], ~np.isnan(r["gain_cut"]))
    p_cp = np.full((D, M), np.nan)
    if changepoint_tests and M > 0 and int(r["n_cp"].sum()):
        # the windows as samples of a second call: bins between the neighbouring change points
        rows, wal, wpen, where = [], [], [], []
        for d in range(D):
            k = int(r["n_cp"][d])
            b = [0] + [int(t) for t in r["cp"][d, :k]] + [int(bin_ptr[d + 1] - bin_ptr[d])]
            for j in range(k):
                rows.append(np.arange(bin_ptr[d] + b[j], bin_ptr[d] + b[j + 2]))
                wal.append(None if al is None else al[d]); wpen.append(pen[d]); where.append((d, j))
        wbp = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
        pick = np.concatenate(rows)
        wdp = np.concatenate([[0], np.cumsum(np.diff(dp)[pick])]).astype(np.int64)
        ent = np.concatenate([np.arange(dp[b], dp[b + 1]) for b in pick]) if pick.size else np.zeros(0, np.int64)
        w = _raw(ctx, len(rows), V, int(pick.size), wdp, term[ent], count[ent], wbp, cat, None if al is None else np.stack(wal), L, 0, np.asarray(wpen), B, b0, seed,
                 stream, maxiter, tol, bins=False)
        pw = pval(w["count_ge"], w["status"] == 0)
        for i, (d, j) in enumerate(where):
            p_cp[d, j] = pw[i]
    return TrajectoryResult(pval(r["count_ge"], status == 0), r["stat"], r["cut"], [p_cut_flat[s] for s in sl], r["n_cp"], r["cp"], p_cp,
                            [r["w_seg"][d, :int(r["n_cp"][d]) + 1] for d in range(D)], [r["w_bin"][s] for s in sl], r["best"], [r["gain_cut"][s] for s in sl],
                            r["count_ge"], [r["count_cut"][s] for s in sl], status, r["unexplained"], r["iters"], B, r["rep_stat"] if keep_replicates else None, names,
                            r["seg_ll"], bin_ptr)
