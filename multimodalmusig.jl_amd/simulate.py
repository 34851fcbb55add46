"""Model simulation and per-sample goodness of fit -- beyond the reference, which can fit exposures but cannot say whether a sample is
explained by the signatures it was given.

`simulate_counts` draws count vectors from every sample's own mixture θ_d x β on the GPU (`mmm_simulate_counts`: Philox4x32-10 counters,
integer thresholds): synthetic cohorts from (exposures, signatures, totals).  `goodness_of_fit` is the parametric bootstrap built on it
(`mmm_fit_check`): B replicates per sample are drawn from its fitted mixture where they are scored, and the sample's reconstruction
cosine and chi-square are placed among theirs -- a p-value that, unlike the raw cosine, does not depend on the number of mutations.  The
definitions, down to the order of every sum, are in include/mmmusig.h: the same arguments give the same bits on
every run.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .bootstrap import _is_nested, _modality_csr, replicate_summary
from .ctm import IMMCTM, MMCTM
from .match import _modality
from .models import ILDA, LDA
from .utils import PackedCorpus, pack_lda, pack_mm

MAX_TERMS = 4096          # V a block keeps in LDS (pi, the threshold row and its histograms)
MAX_SUMMARY_B = 4096      # replicates mmm_replicate_summary takes

_FitCheck = namedtuple("FitCheck", "cosine chi2 p_cosine p_chi2 n_doc B cosine_rep chi2_rep z_cosine z_chi2")


class FitCheck(_FitCheck):
    """cosine, chi2: [D] the statistics of every sample against its mixture (chi2 = +inf where a sample has a mutation in a term its mixture
    cannot produce); p_cosine = (1 + #{replicates with cosine <= the sample's}) / (B + 1), p_chi2 = (1 + #{replicates with chi2 >= the
    sample's}) / (B + 1): small = worse explained than the model's own draws; n_doc: [D] mutations; cosine_rep, chi2_rep: [B, D] with
    keep_replicates (or summary), else None; z_cosine, z_chi2: [D] (observed - mean) / sd over the replicates with summary=True, else None."""
    __slots__ = ()

    def flagged(self, alpha=0.01, statistic="chi2"):
        """indices of the samples with p <= alpha under `statistic` ("chi2" or "cosine")"""
        if statistic not in ("chi2", "cosine"):
            raise ValueError("statistic must be \"chi2\" or \"cosine\"")
        return np.flatnonzero((self.p_chi2 if statistic == "chi2" else self.p_cosine) <= float(alpha))


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _seeds(B, b0, seed, stream):
    B, b0, seed, stream = int(B), int(b0), int(seed), int(stream)
    if B < 0 or b0 < 0 or b0 + B > 2 ** 31 - 1:
        raise ValueError("B and b0 must be >= 0 with b0 + B <= 2^31 - 1")
    if not 0 <= seed < 2 ** 64 or not 0 <= stream < 2 ** 32:
        raise ValueError("seed must fit 64 bits and stream 32 bits, both unsigned")
    return B, b0, seed, stream


def _tables(θ, β, D=None):
    """θ K x D, β V x K -> (props [D, K] = props[k + K d], phi [K, V] = phi[k V + v])"""
    th = np.ascontiguousarray(np.asarray(θ, dtype=np.float64).T); be = np.ascontiguousarray(np.asarray(β, dtype=np.float64).T)
    if th.ndim != 2 or be.ndim != 2 or th.shape[1] != be.shape[0] or be.shape[0] < 1 or be.shape[1] < 1 or (D is not None and th.shape[0] != D):
        raise ValueError("θ must be K x D and β V x K%s" % ("" if D is None else " for the D = %d documents of X" % D))
    if be.shape[1] > MAX_TERMS:
        raise ValueError("V = %d terms (limit %d)" % (be.shape[1], MAX_TERMS))
    return th, be


def _of_model(model, modality, what):
    """-> (ctx, doc_ptr, term, count, θ K x D, β V x K, stream) of a fitted LDA, or of modality m of a fitted MMCTM"""
    if isinstance(model, ILDA):
        raise TypeError("%s: the topics of an ILDA are factorised over the features (ILDA.jl:6-9); no V x K signatures to draw from" % what)
    if isinstance(model, IMMCTM):
        raise TypeError("%s: the topics of an IMMCTM are factorised over the features (IMMCTM.jl:13); no K x V signatures to draw from" % what)
    if isinstance(model, LDA):
        doc_ptr, term, count = pack_lda(model.X)
        return model.ctx, doc_ptr, term, count, model.θ, model.β, 0
    m = _modality(model, modality)
    D = model.D
    dp_all, term_all, count_all = pack_mm(model.X, model.M)
    doc_ptr, count, e0 = _modality_csr(dp_all, count_all, D, m)
    off = int(sum(model.K[:m]))
    θ = model._get("props").reshape(D, model.MK)[:, off:off + model.K[m]].T
    β = np.stack([np.asarray(model.ϕ[m][k], dtype=np.float64) for k in range(model.K[m])], axis=1)
    return model.ctx, doc_ptr, term_all[e0:e0 + count.size], count, θ, β, m


def _totals(doc_ptr, count):
    N = np.zeros(len(doc_ptr) - 1, dtype=np.int64)
    np.add.at(N, np.repeat(np.arange(N.size), np.diff(doc_ptr)), count.astype(np.int64))
    return N


def _simulate(ctx, th, be, N, B, b0, seed, stream):
    """mmm_simulate_counts -> int32 [B, D, V]"""
    D, V = th.shape[0], be.shape[1]
    N = np.asarray(N)
    if N.shape != (D,) or (N < 0).any() or (N >= 2 ** 31).any() or not np.array_equal(N, np.floor(N)):
        raise ValueError("N must hold one total per document, integer and in [0, 2^31)")
    n_doc = np.ascontiguousarray(N, dtype=np.int32)
    out = np.zeros((B, D, V), dtype=np.int32)
    check(lib().mmm_simulate_counts(ctx.h, D, th.shape[1], V, _ptr(th), _ptr(be), _ptr(n_doc), B, b0, seed, stream, _ptr(out)), ctx.h,
          "mmm_simulate_counts")
    return out


def simulate_counts(θ, β=None, N=None, B=1, seed=0, b0=0, stream=0, as_corpus=False, modality=None, ctx=None):
    """B synthetic count tables drawn from the mixtures θ_d x β on the GPU -> int32 [B, D, V]: sample d of replicate b holds N[d]
    categorical draws from p = β θ[:, d] / Σ.  θ: K x D exposures, β: V x K signatures, as `score_exposures` takes them (columns need not be
    normalised; entries >= 0 and finite), N: [D] totals.  Replicates b0 .. b0 + B - 1 of the sequence that (seed, stream) fixes: chunked
    calls are slices of one big call, and the draws share no random word with `resample_counts` or `split_counts` of the same seed.
    as_corpus=True: a list of B corpora in the LDA nesting (W_d x 2 matrices, 1-based terms, zero rows dropped) that `LDA(...)` accepts.
    `simulate_counts(model, N=None, ...)`: a fitted LDA draws from its own θ and β with its samples' totals; an MMCTM with `modality=m`
    from its props and ϕ[m] with stream = m (`stream` must then be 0).  ILDA / IMMCTM: TypeError (factorised tables).  V <= 4096."""
    if isinstance(θ, (LDA, MMCTM, IMMCTM)):
        if β is not None:
            raise TypeError("simulate_counts(model, ...) takes no β")
        mctx, doc_ptr, _, count, θ, β, mstream = _of_model(θ, modality, "simulate_counts")
        if mstream and stream:
            raise ValueError("an MMCTM draws modality m with stream = m; stream must be 0")
        stream = stream or mstream
        ctx = ctx or mctx
        if N is None:
            N = _totals(doc_ptr, count)
    elif β is None or N is None:
        raise TypeError("simulate_counts(θ, β, N, ...) needs β and N")
    ctx = ctx or _lib.default_context()
    B, b0, seed, stream = _seeds(B, b0, seed, stream)
    th, be = _tables(θ, β)
    out = _simulate(ctx, th, be, N, B, b0, seed, stream)
    if not as_corpus:
        return out
    corpora = []
    for b in range(B):
        docs = []
        for d in range(out.shape[1]):
            t = np.flatnonzero(out[b, d])
            docs.append(np.stack([t + 1, out[b, d, t]], axis=1).astype(np.int64))
        corpora.append(docs)
    return corpora


def goodness_of_fit(X, θ=None, β=None, B=1000, seed=0, stream=0, keep_replicates=False, summary=False, modality=None, ctx=None):
    """Per-sample goodness of fit of the samples X under exposures θ (K x D) and signatures β (V x K) by a parametric bootstrap on the GPU
    -> FitCheck.

    For every sample the reconstruction cosine (the `cosine_doc` of `score_exposures`, on the dense count vector) and the Pearson chi-square
    Σ_v (n_v - N π_v)² / (N π_v) against its mixture π = β θ_d / Σ are computed; B count vectors of the same total are drawn from π
    (`simulate_counts` with the same seed and stream gives exactly these), scored the same way where they are drawn, and
    p = (1 + #{replicates at least as extreme}) / (B + 1).  The raw cosine is not comparable across samples, since its distribution under
    the model depends on the number of mutations; the p-values are.  A sample with no mutations has both statistics 0 and p = 1.

    p-values from exposures that were FITTED ON THE SAME COUNTS are conservative: the fit has already moved π towards the sample, so the
    sample lies closer to its mixture than a fresh draw from it does, p is biased upwards and a flag is under- rather than over-called.
    Calibrated p-values need exposures that did not see the counts (a held-out part, or known exposures as in a simulation).

    keep_replicates: return the [B, D] statistics of the replicates.  summary=True: z = (observed - mean) / sd over the replicates
    (`mmm_replicate_summary`; B <= 4096, ValueError beyond).  `goodness_of_fit(model, ...)`: a fitted LDA is checked on its own X, θ, β;
    an MMCTM with `modality=m` on its props and ϕ[m], with stream = m (`stream` must then be 0).  ILDA / IMMCTM: TypeError.  V <= 4096."""
    if isinstance(X, (LDA, MMCTM, IMMCTM)):
        if θ is not None or β is not None:
            raise TypeError("goodness_of_fit(model, ...) takes no θ or β")
        mctx, doc_ptr, term, count, θ, β, mstream = _of_model(X, modality, "goodness_of_fit")
        if mstream and stream:
            raise ValueError("an MMCTM draws modality m with stream = m; stream must be 0")
        stream = stream or mstream
        ctx = ctx or mctx
    else:
        if θ is None or β is None:
            raise TypeError("goodness_of_fit(X, θ, β, ...) needs θ and β")
        if _is_nested(X):
            if modality is None:
                raise ValueError("an MMCTM-nested X holds one corpus per modality: pass modality=m")
            M = X.M if isinstance(X, PackedCorpus) else len(X[0])
            if not 0 <= int(modality) < M:
                raise ValueError("modality %d of %d" % (int(modality), M))
            dp_all, term_all, count_all = pack_mm(X, M)
            doc_ptr, count, e0 = _modality_csr(dp_all, count_all, len(X), int(modality))
            term = term_all[e0:e0 + count.size]
        else:
            doc_ptr, term, count = pack_lda(X)
    ctx = ctx or _lib.default_context()
    B, _, seed, stream = _seeds(B, 0, seed, stream)
    if summary and not 1 <= B <= MAX_SUMMARY_B:
        raise ValueError("summary=True takes 1 <= B <= %d replicates, got %d" % (MAX_SUMMARY_B, B))
    D = len(doc_ptr) - 1
    th, be = _tables(θ, β, D)
    V = be.shape[1]
    if term.size and int(term.max()) >= V:
        raise ValueError("X holds term %d, β has %d terms" % (int(term.max()) + 1, V))
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    term = np.ascontiguousarray(term, dtype=np.int32); count = np.ascontiguousarray(count, dtype=np.int32)
    cos_obs = np.zeros(D); chi_obs = np.zeros(D); cos_le = np.zeros(D, dtype=np.int32); chi_ge = np.zeros(D, dtype=np.int32)
    keep = bool(keep_replicates or summary)
    cos_rep = np.zeros((B, D)) if keep else None
    chi_rep = np.zeros((B, D)) if keep else None
    check(lib().mmm_fit_check(ctx.h, D, th.shape[1], V, doc_ptr.ctypes.data, _ptr(term), _ptr(count), _ptr(th), _ptr(be), B, 0, seed, stream,
                              cos_obs.ctypes.data, chi_obs.ctypes.data, cos_le.ctypes.data, chi_ge.ctypes.data, _ptr(cos_rep), _ptr(chi_rep)), ctx.h, "mmm_fit_check")
    z_cos = z_chi = None
    if summary:
        with np.errstate(all="ignore"):
            mean, sd, _ = replicate_summary(np.concatenate([cos_rep, chi_rep], axis=1), q=(), ctx=ctx) if D else (np.zeros(0), np.zeros(0), None)
            z_cos = (cos_obs - mean[:D]) / sd[:D]
            z_chi = (chi_obs - mean[D:]) / sd[D:]
    return FitCheck(cos_obs, chi_obs, (1.0 + cos_le) / (B + 1.0), (1.0 + chi_ge) / (B + 1.0), _totals(doc_ptr, count), B, cos_rep if keep else None,
                    chi_rep if keep else None, z_cos, z_chi)
