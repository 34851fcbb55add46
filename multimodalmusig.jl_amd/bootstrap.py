"""Bootstrap confidence intervals of the exposures under trained topics -- a capability beyond the reference, which offers point
estimates only (`θ` of LDA, `props` of MMCTM).

Every sample's counts are resampled multinomially B times on the GPU (`mmm_resample_counts`), the B x D replicate documents are stacked
into one corpus and inferred under the frozen topics by the existing path (`transform`: LDA.jl:233-263, MMCTM.jl:511-552 with
`fit_gaussian=false`), and the B exposures of every (signature, sample) cell are reduced to mean / sd / quantiles on the GPU
(`mmm_replicate_summary`).  The definitions -- Philox4x32-10 counters, the integer inverse-CDF draw, the quantile rule -- are in
include/mmmusig.h; the same arguments give the same bits on every run.
"""
import warnings
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .ctm import IMMCTM, MMCTM
from .inference import _lda_infer, transform
from .models import ILDA, LDA
from .utils import PackedCorpus, pack_lda, pack_mm

BootstrapResult = namedtuple("BootstrapResult", "mean sd quantiles q B n_iter converged replicates")
BootstrapResult.__doc__ = """mean, sd: ΣK x D; quantiles: len(q) x ΣK x D; n_iter, converged: one entry per chunk of `batch` replicates;
replicates: B x ΣK x D with return_replicates=True, else None."""


def _resample_csr(ctx, D, doc_ptr, count, B, b0, seed, stream):
    """mmm_resample_counts on one CSR corpus (doc_ptr relative to its first entry) -> int32 [B, nnz]"""
    B, b0, seed, stream = int(B), int(b0), int(seed), int(stream)
    if not 0 <= seed < 2 ** 64 or not 0 <= stream < 2 ** 32:
        raise ValueError("seed must fit 64 bits and stream 32 bits, both unsigned")
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    out = np.zeros((max(B, 0), count.size), dtype=np.int32)
    check(lib().mmm_resample_counts(ctx.h, int(D), doc_ptr, count.ctypes.data if count.size else None, B, b0, seed, stream,
                                    out.ctypes.data if out.size else None), ctx.h, "mmm_resample_counts")
    return out


def _is_nested(X):
    """MMCTM nesting X[d][m] (a list of per-modality matrices) as opposed to LDA's X[d] (one W_d x 2 matrix)"""
    if isinstance(X, PackedCorpus):
        return X.M is not None
    return len(X) > 0 and isinstance(X[0], (list, tuple)) and len(X[0]) > 0 and np.ndim(X[0][0]) == 2


def _modality_csr(doc_ptr, count, D, m):
    """modality m of a pack_mm corpus as a CSR corpus of its own: (relative doc_ptr, counts, first entry)"""
    dp = doc_ptr[m * (D + 1):(m + 1) * (D + 1)]
    return dp - dp[0], count[int(dp[0]):int(dp[-1])], int(dp[0])


def resample_counts(X, B, seed, b0=0, stream=0, ctx=None):
    """B multinomial resamples of every document of X, drawn on the GPU (replicates b0 .. b0 + B - 1 of the sequence that `seed` fixes:
    chunked calls are slices of one big call).  X as LDA takes it (list of W_d x 2 matrices, 1-based terms); returns a list of B corpora of
    the same shape: same rows, same terms, resampled counts -- rows that drew 0 are KEPT (unlike make_count_matrix), every document keeps
    its total.  For an MMCTM-nested X (X[d][m]) modality m is drawn with stream = m (`stream` must then be 0)."""
    ctx = ctx or _lib.default_context()
    if int(B) < 0:
        raise ValueError("B must be >= 0")
    D = len(X)
    if _is_nested(X):
        if stream != 0:
            raise ValueError("an MMCTM-nested X draws modality m with stream = m; stream must be 0")
        M = X.M if isinstance(X, PackedCorpus) else len(X[0])
        doc_ptr, term, count = pack_mm(X, M)
        per_mod = []
        for m in range(M):
            dp, c, e0 = _modality_csr(doc_ptr, count, D, m)
            per_mod.append((dp, term[e0:e0 + c.size] + 1, _resample_csr(ctx, D, dp, c, B, b0, seed, m)))
        return [[[np.stack([t[dp[d]:dp[d + 1]], r[b, dp[d]:dp[d + 1]]], axis=1).astype(np.int64) for dp, t, r in per_mod] for d in range(D)]
                for b in range(int(B))]
    doc_ptr, term, count = pack_lda(X)
    r = _resample_csr(ctx, D, doc_ptr, count, B, b0, seed, stream)
    t = term + 1
    return [[np.stack([t[doc_ptr[d]:doc_ptr[d + 1]], r[b, doc_ptr[d]:doc_ptr[d + 1]]], axis=1).astype(np.int64) for d in range(D)]
            for b in range(int(B))]


def _stack_lda(ctx, D, doc_ptr, term, count, nb, b0, seed):
    """the stacked corpus of replicates b0 .. b0 + nb - 1 (replicate-major: document b D + d), in CSR form"""
    nnz = int(doc_ptr[-1])
    r = _resample_csr(ctx, D, doc_ptr, count, nb, b0, seed, 0)
    dp = np.concatenate([(doc_ptr[:-1][None, :] + nnz * np.arange(nb, dtype=np.int64)[:, None]).ravel(), [nb * nnz]])
    return PackedCorpus(nb * D, dp, np.tile(term, nb), r.ravel())


def _stack_mm(ctx, D, M, doc_ptr, term, count, nb, b0, seed):
    dps, terms, counts, base = [], [], [], 0
    for m in range(M):
        dp, c, e0 = _modality_csr(doc_ptr, count, D, m)
        nnz = c.size
        r = _resample_csr(ctx, D, dp, c, nb, b0, seed, m)
        dps.append(np.concatenate([(dp[:-1][None, :] + nnz * np.arange(nb, dtype=np.int64)[:, None]).ravel(), [nb * nnz]]) + base)
        base += nb * nnz
        terms.append(np.tile(term[e0:e0 + nnz], nb)); counts.append(r.ravel())
    return PackedCorpus(nb * D, np.concatenate(dps), np.concatenate(terms), np.concatenate(counts), M=M)


def replicate_summary(x, q=(0.025, 0.5, 0.975), ctx=None):
    """mean, sd (B - 1 in the denominator; 0 when B = 1) and the q-quantiles (Julia's default `quantile`, numpy's "linear") over the first
    axis of x (B x ...), computed on the GPU (`mmm_replicate_summary`; 1 <= B <= 4096).  A cell with a NaN replicate gives NaN.
    Returns (mean, sd, quantiles) of shapes x.shape[1:], x.shape[1:], (len(q),) + x.shape[1:]."""
    ctx = ctx or _lib.default_context()
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim < 1 or x.shape[0] < 1:
        raise ValueError("replicate_summary needs at least one replicate")
    B, shape = x.shape[0], x.shape[1:]
    n = int(np.prod(shape, dtype=np.int64))
    qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
    mean = np.zeros(n); sd = np.zeros(n); quant = np.zeros((qa.size, n))
    check(lib().mmm_replicate_summary(ctx.h, B, n, x.ctypes.data if n else None, int(qa.size), qa.ctypes.data if qa.size else None,
                                      mean.ctypes.data, sd.ctypes.data, quant.ctypes.data if qa.size else None), ctx.h, "mmm_replicate_summary")
    return mean.reshape(shape), sd.reshape(shape), quant.reshape((qa.size,) + shape)


def bootstrap_exposures(model, X, B, seed, q=(0.025, 0.5, 0.975), batch=None, maxiter=None, tol=None, init_seed=None, return_replicates=False,
                        verbose=False):
    """Non-parametric bootstrap of the exposures of the documents X under the trained topics of `model` (a fitted LDA or MMCTM; a restart
    batch uses its selected restart).  Returns BootstrapResult(mean, sd, quantiles, q, B, n_iter, converged, replicates).

    The counts of every document are resampled B times (`resample_counts`: modality m of an MMCTM corpus with stream = m).  Replicates are
    inferred `batch` at a time (default: all B at once): the `batch` resampled corpora are stacked into ONE corpus of batch x D documents
    (replicate-major: document b D + d) and given to the frozen-topic path, exactly as `transform(model, X_stacked, maxiter, tol)` (LDA;
    defaults 1000 / 1e-4) or `transform(model, X_stacked, maxiter, tol, fit_gaussian=False)` (MMCTM; defaults as `transform`, including
    the reference's tol = 1e4) would -- the replicates equal that composition bit for bit.  `init_seed` is `transform`'s `seed`.

    The stopping rule is the existing one and therefore acts on the log-likelihood of the STACKED corpus: all replicates of a chunk run
    the same number of passes.  With batch < B different chunks may stop at different passes; `n_iter` and `converged` are per chunk.

    The exposures are θ (K x D) for LDA and the props of every modality for MMCTM (ΣK x D, modality-major rows, the order of `propdf` in
    scripts/run_mmctm.jl:216-240).  mean / sd / quantiles are taken over all B replicates in one `mmm_replicate_summary` call.  The trained
    model is not touched.  ILDA / IMMCTM: TypeError (the reference defines no `transform` for them)."""
    if isinstance(model, ILDA):
        raise TypeError("transform(::ILDA) is a MethodError in the reference (ILDA.jl:293): no bootstrap of ILDA exposures")
    if isinstance(model, IMMCTM):
        raise TypeError("transform is not defined for IMMCTM (IMMCTM.jl has no such method): no bootstrap of IMMCTM exposures")
    if not isinstance(model, (LDA, MMCTM)):
        raise TypeError("bootstrap_exposures takes a fitted LDA or MMCTM")
    B = int(B)
    if B < 1:
        raise ValueError("B must be >= 1")
    batch = B if batch is None else int(batch)
    if batch < 1:
        raise ValueError("batch must be >= 1")
    D, ctx = len(X), model.ctx
    is_lda = isinstance(model, LDA)
    if is_lda:
        doc_ptr, term, count = pack_lda(X)
        SK = model.K
        maxiter = 1000 if maxiter is None else int(maxiter)
        tol = 1e-4 if tol is None else tol
    else:
        doc_ptr, term, count = pack_mm(X, model.M)
        SK = model.MK
        maxiter = 1000 if maxiter is None else int(maxiter)
    reps = np.empty((B, SK, D))
    n_iter, converged = [], []
    for b0 in range(0, B, batch):
        nb = min(batch, B - b0)
        if is_lda:
            Xs = _stack_lda(ctx, D, doc_ptr, term, count, nb, b0, seed)
            new = LDA(model.K, model.α, model.η, model.V, Xs, seed=init_seed, ctx=ctx)         # the steps of transform (LDA.jl:233-263)
            try:
                new.β = model.β
                hist = _lda_infer(new, True, maxiter, tol, verbose)
                expo = new._get("theta")
                n_iter.append(len(hist)); converged.append(bool(new.converged))
            finally:
                new.close()
        else:
            Xs = _stack_mm(ctx, D, model.M, doc_ptr, term, count, nb, b0, seed)
            new = transform(model, Xs, maxiter=maxiter, tol=tol, fit_gaussian=False, verbose=verbose, seed=init_seed)
            try:
                expo = new._get("props")
                n_iter.append(len(new.ll_history)); converged.append(bool(new.converged))
            finally:
                new.close()
        reps[b0:b0 + nb] = expo.reshape(nb, D, SK).transpose(0, 2, 1)
    if not all(converged):
        warnings.warn("bootstrap_exposures: %d of %d chunks did not converge within maxiter = %d passes" % (len(converged) - sum(converged), len(converged), maxiter))
    mean, sd, quant = replicate_summary(reps, q, ctx=ctx)
    return BootstrapResult(mean, sd, quant, tuple(float(v) for v in np.atleast_1d(q)), B, n_iter, converged, reps if return_replicates else None)
