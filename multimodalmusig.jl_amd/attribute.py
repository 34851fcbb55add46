"""Which signature caused this mutation? -- the per-mutation signature probabilities that SigProfilerAssignment, MutationalPatterns and
deconstructSigs write, and the question behind every driver analysis ("was this PIK3CA E545K an APOBEC mutation?", "what share of the
cohort's POLE-hotspot mutations came from SBS10?").

Per queried (sample, term) pair the posterior of signature c is w_c P[c][v] / Σ_c' w_c' P[c'][v] under the sample's fit over its allowed
signatures.  The point value is one division; the number a user needs is its uncertainty -- in a 150-mutation exome a posterior of 0.6 is
worth little.  So the sample's counts are resampled B times (the replicates of `resample_counts` and of `refit_exposures(bootstrap=B)`
under the same seed, deliberately), every replicate is refitted and its posteriors are accumulated as exact integers, all in one call
(`mmm_attribute_mutations`): the replicates' counts never leave the device's LDS.  Queries can carry a group label (a gene, a hotspot), and
the per-replicate group totals give intervals on "the share of this group's mutations that signature c caused".  The definition, down to the
order of every sum, is in include/mmmusig.h.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .bootstrap import _is_nested, replicate_summary
from .ctm import MMCTM
from .models import LDA
from .presence import _corpus
from .refit import MAX_CATALOGUE, _catalogue, refit_exposures
from .simulate import MAX_SUMMARY_B, MAX_TERMS, _seeds

FX_ONE = 1 << 24           # the fixed point of the accumulators: x = floor(ρ 2^24)
MAX_CALL_B = 4096          # replicates of one mmm_attribute_mutations call
MAX_TOTAL_B = 65535        # replicates whose Σ x² still fits the 64-bit sum: 65,536 x 2^48 = 2^64
MAX_ROW = 4096             # CSR entries of a queried sample
REPLICATE_BYTES = 256 << 20      # host budget for the kept posteriors of one chunk of samples (quantiles=True)

_FIELDS = ("posterior top exposures mean sd p_top void quantiles group_share group_mean group_quantiles groups names queries status iters B q "
           "replicates")
_AttributionResult = namedtuple("AttributionResult", _FIELDS)


class AttributionResult(_AttributionResult):
    """Q queries in the caller's order, C signatures, D samples, G groups.  posterior: [Q, C], exactly 0 outside the sample's allowed set, a
    row of zeros where none of them produces the term; top: [Q] the signature with the largest posterior (-1 for a row of zeros);
    exposures: [C, D] the fitted weights; status: [D] 0 processed, 3 no mutations or nothing allowed, 4 no queries; iters: [D] EM iterations
    of all the sample's fits (the observed fit runs once per call).  queries: [Q, 3] (sample, 1-based term, mult) as given.
    With B > 0 -- mean, sd: [Q, C] over the B - void replicates in which some allowed signature produces the term (NaN where there is none;
    from the exact fixed-point sums, resolution 2^-24); p_top: [Q, C] the fraction of the B replicates in which c had the largest posterior;
    void: [Q] replicates in which the term had no mass.  quantiles: [len(q), Q, C] with quantiles=True (void replicates enter as 0), else None;
    replicates: [B, Q, C] with keep_replicates=True, else None.
    groups: the G labels in the order of their first appearance; group_share: [G, C] Σ mult floor(ρ 2^24) over the group's queries,
    normalised over c (NaN for a group without mass); group_mean, group_quantiles: [G, C] and [len(q), G, C] of that share over the
    replicates.  names: the catalogue's names or None."""
    __slots__ = ()

    def _name(self, c):
        return self.names[c] if self.names is not None else "signature %d" % c

    def describe(self, i):
        """one line of text for query i, e.g. "sample 12, term 37: 71.3 % SBS2 [55.0, 84.1]" (the interval: the outer quantiles)"""
        i = int(i)
        d, v = int(self.queries[i, 0]), int(self.queries[i, 1])
        c = int(self.top[i])
        if c < 0:
            return "sample %d, term %d: no allowed signature produces it" % (d, v)
        s = "sample %d, term %d: %.1f %% %s" % (d, v, 100.0 * self.posterior[i, c], self._name(c))
        if self.quantiles is not None and self.quantiles.shape[0] >= 2:
            s += " [%.1f, %.1f]" % (100.0 * self.quantiles[0, i, c], 100.0 * self.quantiles[-1, i, c])
        elif self.B:
            s += " (sd %.1f, top in %.0f %% of %d replicates)" % (100.0 * self.sd[i, c], 100.0 * self.p_top[i, c], self.B)
        return s


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _raw(ctx, D, V, doc_ptr, term, count, cat, allowed, q_ptr, q_term, q_mult=None, q_group=None, G=0, B=0, b0=0, seed=0, stream=0, maxiter=1000, tol=1e-9,
         keep=False):
    """mmm_attribute_mutations on one CSR corpus (0-based terms) and one query CSR -> dict of its outputs."""
    cat = np.ascontiguousarray(cat, dtype=np.float64)
    C = cat.shape[0]
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    term = np.ascontiguousarray(term, dtype=np.int32); count = np.ascontiguousarray(count, dtype=np.int32)
    q_ptr = np.ascontiguousarray(q_ptr, dtype=np.int64)
    q_term = np.ascontiguousarray(q_term, dtype=np.int32)
    q_mult = None if q_mult is None else np.ascontiguousarray(q_mult, dtype=np.int32)
    q_group = None if q_group is None else np.ascontiguousarray(q_group, dtype=np.int32)
    if allowed is not None:
        allowed = np.ascontiguousarray(allowed, dtype=np.uint8)
        if allowed.shape != (D, C):
            raise ValueError("allowed must be [D, C] = [%d, %d], got %r" % (D, C, allowed.shape))
    Q = int(q_term.size)
    B, G = int(B), int(G)
    out = dict(w=np.zeros((D, C)), post=np.zeros((Q, C)), status=np.zeros(D, dtype=np.int8), iters=np.zeros(D, dtype=np.int64),
               sum_fx=np.zeros((Q, C), dtype=np.uint64), sumsq_fx=np.zeros((Q, C), dtype=np.uint64), top_count=np.zeros((Q, C), dtype=np.int32),
               void_count=np.zeros(Q, dtype=np.int32), group_fx=np.zeros((max(B, 0), max(G, 0), C), dtype=np.uint64),
               rep_post=np.zeros((max(B, 0), Q, C)) if keep else None)
    rc = lib().mmm_attribute_mutations(ctx.h, int(D), C, int(V), doc_ptr, _ptr(term), _ptr(count), cat.ravel(), _ptr(allowed), q_ptr, _ptr(q_term), _ptr(q_mult),
                                       _ptr(q_group), G, B, int(b0), int(seed), int(stream), int(maxiter), float(tol),
                                       *[_ptr(out[k]) for k in ("w", "post", "status", "iters", "sum_fx", "sumsq_fx", "top_count", "void_count", "group_fx",
                                                                "rep_post")])
    check(rc, ctx.h, "mmm_attribute_mutations")
    return out


def _queries(queries, doc_ptr, term, count, D, V):
    """-> int64 [Q, 3] (sample, 0-based term, mult) in the caller's order; None: every non-zero entry of the corpus, mult = its count"""
    if queries is None:
        e = np.flatnonzero(count > 0)
        d = np.searchsorted(doc_ptr, e, side="right") - 1
        return np.stack([d.astype(np.int64), term[e].astype(np.int64), count[e].astype(np.int64)], axis=1).reshape(-1, 3)
    rows = []
    for i, t in enumerate(queries):
        t = tuple(t)
        if len(t) not in (2, 3) or any(int(x) != x for x in t):
            raise ValueError("query %d must be (sample, term) or (sample, term, mult) of integers, got %r" % (i, t))
        d, v, m = int(t[0]), int(t[1]), int(t[2]) if len(t) == 3 else 1
        if not 0 <= d < D:
            raise ValueError("query %d names sample %d of %d" % (i, d, D))
        if not 1 <= v <= V:
            raise ValueError("query %d names term %d; terms are 1-based like X, the catalogue has %d" % (i, v, V))
        if m < 1:
            raise ValueError("query %d has mult %d (>= 1)" % (i, m))
        rows.append((d, v - 1, m))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def _group_ids(groups, Q):
    """labels (None: no group) -> (labels in the order of their first appearance, int32 [Q] ids with -1 for None)"""
    if groups is None:
        return [], None
    groups = list(groups)
    if len(groups) != Q:
        raise ValueError("groups must hold one label per query (%d), got %d" % (Q, len(groups)))
    labels, ids = [], np.full(Q, -1, dtype=np.int32)
    index = {}
    for i, g in enumerate(groups):
        if g is None:
            continue
        if g not in index:
            index[g] = len(labels); labels.append(g)
        ids[i] = index[g]
    return labels, ids


def _sort_queries(qs, D):
    """the queries as a CSR over samples -> (order, q_ptr): sorted = qs[order], a stable sort by sample; result[order] = sorted result"""
    order = np.argsort(qs[:, 0], kind="stable")
    q_ptr = np.concatenate([[0], np.cumsum(np.bincount(qs[:, 0], minlength=D))]).astype(np.int64)
    return order, q_ptr


def _group_observed(post, mult, gid, G):
    """Σ mult floor(ρ 2^24) per (group, signature) as exact integers -> uint64 [G, C]"""
    out = np.zeros((G, post.shape[1]), dtype=np.uint64)
    if G and gid is not None:
        x = np.floor(post * FX_ONE).astype(np.uint64) * mult.astype(np.uint64)[:, None]
        m = gid >= 0
        np.add.at(out, gid[m], x[m])
    return out


def _shares(fx):
    """[..., C] integer totals -> their shares over the last axis, NaN where the total is 0"""
    fx = np.asarray(fx, dtype=np.float64)
    tot = fx.sum(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(tot > 0, fx / tot, np.nan)


def _group_summary(group_fx, q):
    """group_fx uint64 [B, G, C] -> (mean [G, C], quantiles [len(q), G, C]) of the per-replicate shares; replicates in which a group has no
    mass are left out of that group's summary"""
    qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    B, G, C = group_fx.shape
    if B == 0 or G == 0:
        return np.full((G, C), np.nan), np.full((qa.size, G, C), np.nan)
    s = _shares(group_fx)
    mean = np.full((G, C), np.nan); quant = np.full((qa.size, G, C), np.nan)
    for g in range(G):
        ok = ~np.isnan(s[:, g, 0])
        if ok.any():
            mean[g] = s[ok, g].mean(axis=0)
            quant[:, g] = np.quantile(s[ok, g], qa, axis=0)
    return mean, quant


def _moments(sum_fx, sumsq_fx, n):
    """mean and sd (n - 1 in the denominator; 0 for n = 1, NaN for n = 0) of ρ from the fixed-point sums over n [Q] replicates.  The numerator
    n Σx² - (Σx)² is formed in exact integer arithmetic, so equal replicates give sd = 0 exactly."""
    n = np.asarray(n, dtype=np.int64)
    nf = n.astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(nf > 0, sum_fx.astype(np.float64) / nf / FX_ONE, np.nan)
    sd = np.where(nf > 0, 0.0, np.nan) * np.ones(sum_fx.shape)
    qi, ci = np.nonzero((sum_fx > 0) & (n[:, None] > 1))
    if qi.size:
        s = sum_fx[qi, ci].astype(object); ss = sumsq_fx[qi, ci].astype(object); k = n[qi].astype(object)
        num = (k * ss - s * s).astype(np.float64)
        kf = n[qi].astype(np.float64)
        sd[qi, ci] = np.sqrt(num / (kf * (kf - 1.0))) / FX_ONE
    return mean, sd


def attribute_mutations(X, catalogue, queries=None, groups=None, allowed=None, B=0, seed=None, q=(0.025, 0.5, 0.975), quantiles=False, modality=None,
                        maxiter=1000, tol=1e-9, keep_replicates=False, ctx=None):
    """Posterior of every catalogue signature for the queried mutations of the samples X, with bootstrap uncertainty -> AttributionResult.

    X, catalogue and modality as `signature_presence` takes them (C <= 256, V <= 4096; a queried sample has at most 4096 rows).  ILDA /
    IMMCTM catalogues: TypeError (factorised tables).
    allowed: a mask, a list of names or a `RefitResult` (its chosen sets); None: `refit_exposures(X, catalogue, "bic")` runs first and its
    chosen sets are used.  No elimination runs here.
    queries: None = every non-zero entry of X, with mult = its count; else a sequence of (sample, term) or (sample, term, mult), samples
    0-based, terms 1-based like X, in any order -- a term need not occur in the sample, and a pair may be asked twice.  groups: one label per
    query (a gene, a hotspot; None = no group).
    B: bootstrap replicates (needs seed; at most 65,535 -- beyond that Σ x² no longer fits its 64-bit sum and sd could not be formed).  The
    replicates are those of `resample_counts(X, B, seed)` and of `refit_exposures(bootstrap=B, seed=seed)`, on purpose: intervals on the
    exposures and on the posteriors then describe the same resamples.  More than 4096 replicates go through several calls, whose sums add.
    quantiles=True: per-query quantiles at q (B <= 4096).  The samples are then taken in chunks whose kept posteriors stay within a fixed
    host budget, and each chunk is reduced by `mmm_replicate_summary`.  keep_replicates: return the [B, Q, C] posteriors themselves.
    Every argument is checked before a device is asked for."""
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
    if B > MAX_TOTAL_B:
        raise ValueError("B = %d replicates: beyond %d the 64-bit sum of squares overflows and sd cannot be formed" % (B, MAX_TOTAL_B))
    B, _, seed, _ = _seeds(B, 0, 0 if seed is None else seed, 0)
    if (quantiles or keep_replicates) and B > MAX_SUMMARY_B:
        raise ValueError("quantiles / keep_replicates hold every replicate: B <= %d" % MAX_SUMMARY_B)
    if (quantiles or keep_replicates) and B == 0:
        raise ValueError("quantiles / keep_replicates need B > 0 replicates")
    qa = tuple(float(v) for v in np.atleast_1d(q))
    if any(not 0.0 <= v <= 1.0 for v in qa):
        raise ValueError("q must lie in [0, 1]")
    if int(maxiter) < 1 or not float(tol) >= 0.0:
        raise ValueError("maxiter must be >= 1 and tol >= 0")
    D, doc_ptr, term, count, al = _corpus(X, modality, allowed, names, C, V)
    stream = int(modality) if _is_nested(X) else 0           # the stream refit_exposures(bootstrap=B) draws the modality with
    qs = _queries(queries, doc_ptr, term, count, D, V)
    Q = qs.shape[0]
    labels, gid = _group_ids(groups, Q)
    G = len(labels)
    rows = np.diff(doc_ptr)
    long = [int(d) for d in np.unique(qs[:, 0]) if rows[d] > MAX_ROW]
    if long:
        raise ValueError("queried sample %d has %d rows (limit %d)" % (long[0], int(rows[long[0]]), MAX_ROW))
    if G and int(np.bincount(gid[gid >= 0], weights=qs[gid >= 0, 2], minlength=G).max()) >= 2 ** 31:
        raise ValueError("the mults of a group must sum to less than 2^31")
    ctx = ctx or (catalogue.ctx if isinstance(catalogue, (LDA, MMCTM)) else _lib.default_context())      # every argument is checked before a device is asked for
    if allowed is None:
        al = np.ascontiguousarray(refit_exposures(X, catalogue, "bic", maxiter=maxiter, tol=tol, modality=modality, ctx=ctx).active.T, dtype=np.uint8)
    order, q_ptr = _sort_queries(qs, D)
    sq = qs[order]
    sg = None if gid is None else gid[order]
    q_term, q_mult = sq[:, 1].astype(np.int32), sq[:, 2].astype(np.int32)

    # ---- chunks of samples (only where the replicates are kept) x chunks of replicates
    keep = bool(quantiles or keep_replicates)
    nq_doc = np.diff(q_ptr)
    chunks = []
    if keep:
        cap = max(1, REPLICATE_BYTES // (8 * C * max(B, 1)))
        lo = 0
        while lo < D:
            hi = lo + 1
            while hi < D and q_ptr[hi + 1] - q_ptr[lo] <= cap:
                hi += 1
            chunks.append((lo, hi)); lo = hi
    else:
        chunks.append((0, D))
    W = np.zeros((D, C)); post = np.zeros((Q, C)); status = np.full(D, 4, dtype=np.int8); iters = np.zeros(D, dtype=np.int64)
    sum_fx = np.zeros((Q, C), dtype=np.uint64); sumsq_fx = np.zeros((Q, C), dtype=np.uint64)
    top_count = np.zeros((Q, C), dtype=np.int64); void = np.zeros(Q, dtype=np.int64)
    group_fx = np.zeros((B, G, C), dtype=np.uint64)
    quant = np.zeros((len(qa), Q, C)) if quantiles else None
    reps = np.zeros((B, Q, C)) if keep_replicates else None
    for lo, hi in chunks:
        a, b = int(q_ptr[lo]), int(q_ptr[hi])
        if a == b:
            continue
        qp = np.zeros(D + 1, dtype=np.int64)
        qp[lo + 1:hi + 1] = q_ptr[lo + 1:hi + 1] - a
        qp[hi + 1:] = b - a
        b0 = 0
        while True:
            nb = min(B - b0, MAX_CALL_B)
            r = _raw(ctx, D, V, doc_ptr, term, count, cat, al, qp, q_term[a:b], q_mult[a:b], None if sg is None else sg[a:b], G, nb, b0, seed, stream, maxiter,
                     tol, keep=keep)
            if b0 == 0:
                post[a:b] = r["post"]
                docs = np.arange(lo, hi)[nq_doc[lo:hi] > 0]
                W[docs] = r["w"][docs]; status[docs] = r["status"][docs]
            iters += r["iters"]
            sum_fx[a:b] += r["sum_fx"]; sumsq_fx[a:b] += r["sumsq_fx"]; top_count[a:b] += r["top_count"]; void[a:b] += r["void_count"]
            if nb:
                group_fx[b0:b0 + nb] += r["group_fx"]
            if keep:
                if quantiles:
                    quant[:, a:b] = replicate_summary(r["rep_post"], qa, ctx=ctx)[2]
                if keep_replicates:
                    reps[:, a:b] = r["rep_post"]
            b0 += nb
            if b0 >= B:
                break
    inv = np.empty(Q, dtype=np.int64)
    inv[order] = np.arange(Q)
    un = lambda x: x[inv]
    post_u = un(post)
    top = np.where(post_u.max(axis=1) > 0, post_u.argmax(axis=1), -1) if Q else np.zeros(0, dtype=np.int64)
    mean = sd = p_top = void_u = None
    if B:
        mean, sd = _moments(un(sum_fx), un(sumsq_fx), B - un(void))
        p_top = un(top_count) / float(B)
        void_u = un(void)
    gshare = _shares(_group_observed(post, q_mult, sg, G)) if G else np.zeros((0, C))
    gmean, gquant = _group_summary(group_fx, qa) if B else (None, None)
    out_q = qs.copy(); out_q[:, 1] += 1
    return AttributionResult(post_u, top, W.T.copy(), mean, sd, p_top, void_u, None if quant is None else quant[:, inv], gshare, gmean, gquant, labels, names, out_q,
                             status, iters, B, qa, None if reps is None else reps[:, inv])


def mutation_table(result, path=None):
    """The per-mutation table assignment tools write: one row per query with sample, term, mult, the top signature, its posterior (and, with
    replicates, its sd and p_top) and the posterior of every signature -> (header, rows).  path: also written there as TSV."""
    C = result.posterior.shape[1]
    sig = list(result.names) if result.names is not None else ["signature_%d" % c for c in range(C)]
    header = ["sample", "term", "mult", "top", "posterior"] + (["sd", "p_top"] if result.B else []) + sig
    rows = []
    for i in range(result.posterior.shape[0]):
        c = int(result.top[i])
        row = [int(result.queries[i, 0]), int(result.queries[i, 1]), int(result.queries[i, 2]), sig[c] if c >= 0 else "", float(result.posterior[i, c]) if c >= 0 else 0.0]
        if result.B:
            row += [float(result.sd[i, c]) if c >= 0 else float("nan"), float(result.p_top[i, c]) if c >= 0 else 0.0]
        rows.append(row + [float(x) for x in result.posterior[i]])
    if path is not None:
        with open(path, "w") as fh:
            fh.write("\t".join(header) + "\n")
            for row in rows:
                fh.write("\t".join(repr(x) if isinstance(x, float) else str(x) for x in row) + "\n")
    return header, rows
