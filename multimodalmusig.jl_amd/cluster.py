"""Groups of samples by their exposures: consensus k-means (Monti et al. 2003; ConsensusClusterPlus) -- the cohort-level step after a fit,
which the MMCTM paper takes to find subgroups of tumours from their signature probabilities.

For every candidate number of groups k, `replicates` k-means runs on random subsamples go through one launch (`mmm_cluster_samples`, one
workgroup per run); an all-pairs pass counts how often two samples were drawn together and how often they then shared a group.  From the
counts: the consensus matrix, PAC (the proportion of ambiguously clustered pairs, Senbabaoglu et al. 2014) per k, the k with the smallest
PAC, one final partition by average linkage of 1 - consensus, and a per-sample confidence.  The definition, down to the order of every sum,
is in include/mmmusig.h: the same arguments give the same bits on every run.

PAC prefers coarse, clean splits: where two groups merge cleanly, a smaller k can score 0 although more groups exist.  Read `pac` over all
ks, not only its minimum, and pass `k=` where the finer split is wanted.

The linkage runs on the host in numpy: D merges, each a minimum over a D x D matrix.  Measured per k on one host core: 0.07 s at
D = 560, 0.6 s at D = 1200, 2.8 s at D = 2000 (from about D = 1500 it takes seconds), 53 s at D = 4096; `labels_by_k` runs it for every k, so pass
few ks where D is in the thousands.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .ctm import IMMCTM, MMCTM
from .models import ILDA, LDA

MAX_SAMPLES = 4096
MAX_FEATURES = 256
MAX_KS = 16
MAX_GROUPS = 32

_SampleClusters = namedtuple("SampleClusters", "ks pac k labels labels_by_k consensus together item_consensus cluster_consensus iters inertia skipped "
                                               "unsettled replicates")


class SampleClusters(_SampleClusters):
    """ks: [nk] the candidate numbers of groups; pac: [nk] ambiguous / valid pairs (NaN where no pair was ever drawn together); k: the chosen
    number (the smallest pac, ties to the smaller k, or the `k=` argument); labels: [D] the final groups at k, numbered by their smallest
    member; labels_by_k: [nk, D] the same for every k; consensus: [nk, D, D] same / together, 0 where never together, and together:
    [nk, D, D] (both None with counts=False); item_consensus: [D] a sample's mean consensus at k with the other members of its group (NaN for a
    group of one); cluster_consensus: [k] the mean over a group's pairs (NaN for a group of one); iters, inertia: [nk, B] of every run;
    skipped: [nk] runs whose subsample had fewer than k members; unsettled: [nk] runs that reached maxiter; replicates: B."""
    __slots__ = ()

    def flagged(self, threshold=0.8):
        """indices of the samples whose item consensus is below `threshold`"""
        return np.flatnonzero(self.item_consensus < float(threshold))


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _raw(ctx, x, ks, B, b0=0, keep=0, seed=0, stream=0, maxiter=100, pac_lo=100, pac_hi=900, waves=0, placement=0,
         outputs=("together", "same", "ambiguous", "valid")):
    """mmm_cluster_samples on x [D, P] -> dict of labels [nk, B, D] int8, iters [nk, B] int32, inertia [nk, B] and, where asked for, together,
    same [nk, D, D] uint32, ambiguous, valid [nk] int64"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be [D, P], got %r" % (x.shape,))
    D, P = x.shape
    ks = np.ascontiguousarray(ks, dtype=np.int32)
    if ks.ndim != 1:
        raise ValueError("ks must be a list of numbers of groups")
    nk, B = ks.size, int(B)
    out = {"labels": np.zeros((nk, max(B, 0), D), dtype=np.int8), "iters": np.zeros((nk, max(B, 0)), dtype=np.int32), "inertia": np.zeros((nk, max(B, 0)))}
    for name in ("together", "same"):
        if name in outputs:
            out[name] = np.zeros((nk, D, D), dtype=np.uint32)
    for name in ("ambiguous", "valid"):
        if name in outputs:
            out[name] = np.zeros(nk, dtype=np.int64)
    # an empty array still needs an address: NULL says "not given"
    one = np.zeros(1)
    addr = lambda a: a.ctypes.data if a.size else one.ctypes.data
    opt = lambda name: addr(out[name]) if name in out else None
    rc = lib().mmm_cluster_samples(ctx.h, int(D), int(P), addr(x), int(nk), addr(ks), B, int(b0), int(keep), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(maxiter),
                                   int(pac_lo), int(pac_hi), int(waves), int(placement), addr(out["labels"]), addr(out["iters"]), addr(out["inertia"]),
                                   opt("together"), opt("same"), opt("ambiguous"), opt("valid"))
    check(rc, ctx.h, "mmm_cluster_samples")
    return out


def _keep(subsample):
    """the 32-bit threshold of a subsampling fraction: 1.0 -> 0 (every sample), else floor(subsample 2^32) clipped to [1, 2^32 - 1]"""
    s = float(subsample)
    if not 0.0 < s <= 1.0:
        raise ValueError("subsample must be in (0, 1]")
    return 0 if s == 1.0 else int(min(max(np.floor(s * 4294967296.0), 1.0), 4294967295.0))


def _per_mille(pac):
    try:
        lo, hi = (float(v) for v in pac)
    except (TypeError, ValueError):
        raise ValueError("pac must be a pair (lower, upper) of consensus bounds")
    if not 0.0 <= lo < hi <= 1.0:
        raise ValueError("pac = (lower, upper) needs 0 <= lower < upper <= 1")
    lo, hi = int(round(lo * 1000.0)), int(round(hi * 1000.0))
    if not lo < hi:
        raise ValueError("pac bounds are taken per mille: %r leaves no interval" % (pac,))
    return lo, hi


def _features(E, modalities):
    """-> (ctx of the model or None, [D, P] features before the metric)"""
    if isinstance(E, (LDA, ILDA)):
        if modalities is not None:
            raise ValueError("modalities is for an MMCTM / IMMCTM")
        th = np.asarray(E.θ, dtype=np.float64)                 # K x D
        return E.ctx, np.ascontiguousarray((th / th.sum(axis=0, keepdims=True)).T)
    if isinstance(E, (MMCTM, IMMCTM)):
        ms = list(range(E.M)) if modalities is None else [int(m) for m in np.atleast_1d(modalities)]
        if not ms or len(set(ms)) != len(ms) or not all(0 <= m < E.M for m in ms):
            raise ValueError("modalities must be distinct indices below %d" % E.M)
        props = E._get("props").reshape(E.D, E.MK)
        off = np.concatenate([[0], np.cumsum(E.K)]).astype(int)
        return E.ctx, np.ascontiguousarray(np.concatenate([props[:, off[m]:off[m + 1]] for m in ms], axis=1))
    if modalities is not None:
        raise ValueError("modalities is for an MMCTM / IMMCTM")
    x = np.array(E, dtype=np.float64, ndmin=1)
    if x.ndim != 2:
        raise ValueError("E must be a [D, P] array or a fitted model")
    return None, x


def _transform(x, metric):
    if metric not in ("hellinger", "euclidean"):
        raise ValueError("metric must be \"hellinger\" or \"euclidean\"")
    if not np.isfinite(x).all():
        raise ValueError("E holds an entry that is not finite")
    if metric == "euclidean":
        if (np.abs(x) > 1e150).any():
            raise ValueError("E holds an entry beyond 1e150 in magnitude")
        return np.ascontiguousarray(x)
    if (x < 0).any():
        raise ValueError("metric=\"hellinger\" takes non-negative features")
    s = x.sum(axis=1, keepdims=True)
    if not (s > 0).all():
        raise ValueError("metric=\"hellinger\" takes rows with a positive sum")
    return np.ascontiguousarray(np.sqrt(x / s))


def average_linkage(dist, k):
    """Average-linkage (UPGMA) agglomeration of the symmetric [D, D] matrix `dist` down to k groups -> labels [D], the groups numbered by their
    smallest member.  The closest pair of groups is taken in row-major order (the lowest (i, j), groups standing at their smallest member);
    merged distances by the Lance-Williams update with size weights, (n_i d_ih + n_j d_jh) / (n_i + n_j)."""
    M = np.array(dist, dtype=np.float64)
    D = M.shape[0]
    if M.shape != (D, D) or not 1 <= int(k) <= max(D, 1):
        raise ValueError("average_linkage needs a [D, D] matrix and 1 <= k <= D")
    np.fill_diagonal(M, np.inf)
    size = np.ones(D)
    rep = np.arange(D)                                 # the slot every sample stands in
    for _ in range(D - int(k)):
        i, j = divmod(int(np.argmin(M)), D)            # the first minimum in row-major order of a symmetric matrix has i < j
        row = (size[i] * M[i] + size[j] * M[j]) / (size[i] + size[j])
        row[i] = np.inf; row[j] = np.inf
        M[i] = row; M[:, i] = row
        M[j] = np.inf; M[:, j] = np.inf
        size[i] += size[j]
        rep[rep == j] = i
    _, labels = np.unique(rep, return_inverse=True)    # slots are smallest members: ascending slot = ascending smallest member
    return labels.astype(np.int64)


def _item_consensus(cons, labels):
    D = labels.size
    item = np.full(D, np.nan)
    groups = int(labels.max()) + 1 if D else 0
    clus = np.full(groups, np.nan)
    for g in range(groups):
        idx = np.flatnonzero(labels == g)
        if idx.size < 2:
            continue
        sub = cons[np.ix_(idx, idx)]
        off = sub.sum(axis=1) - np.diag(sub)
        item[idx] = off / (idx.size - 1)
        clus[g] = off.sum() / (idx.size * (idx.size - 1))
    return item, clus


def _pick(pac, ks):
    """index of the smallest pac, ties to the smaller k; NaN counts as +inf"""
    return min(range(len(ks)), key=lambda i: (np.inf if np.isnan(pac[i]) else pac[i], ks[i]))


def cluster_samples(E, ks=range(2, 9), replicates=1000, subsample=0.8, seed=0, metric="hellinger", maxiter=100, pac=(0.1, 0.9), k=None, modalities=None,
                    counts=True, ctx=None):
    """Consensus clustering of the samples by their exposures on the GPU -> SampleClusters.

    E: a [D, P] array of features per sample; a fitted LDA / ILDA (its normalised θ); a fitted MMCTM / IMMCTM (the signature probabilities of
    `modalities`, default all, side by side).  ks: the candidate numbers of groups (<= 16 of them, each in 1 .. min(32, D)).  replicates: B
    k-means runs per k, each on a subsample in which every sample is kept with probability `subsample` (1.0: all samples, the runs differ by
    their starts only), started by k-means++ from Philox words of (seed, replicate index) and run for at most `maxiter` iterations.
    metric: "hellinger" clusters the square roots of the row-normalised features (non-negative rows), "euclidean" the features as given.
    pac = (lower, upper): a pair of samples is ambiguous when its consensus lies strictly between the bounds (taken per mille).  k: the
    number of groups of `labels`, one of ks; None: the smallest PAC.  counts=False leaves `consensus` and `together` out of the result.
    D <= 4096, P <= 256."""
    mctx, x = _features(E, modalities)
    x = _transform(x, metric)
    D, P = x.shape
    if not 1 <= D <= MAX_SAMPLES or not 1 <= P <= MAX_FEATURES:
        raise ValueError("D = %d samples (1 .. %d), P = %d features (1 .. %d)" % (D, MAX_SAMPLES, P, MAX_FEATURES))
    try:
        ks = list(ks)
        kl = [int(v) for v in ks]
    except (TypeError, ValueError):
        raise ValueError("ks must be a list of numbers of groups")
    if not 1 <= len(kl) <= MAX_KS or len(set(kl)) != len(kl) or any(v != w for v, w in zip(kl, ks)):
        raise ValueError("ks must hold 1 .. %d distinct integers" % MAX_KS)
    if min(kl) < 1 or max(kl) > min(MAX_GROUPS, D):
        raise ValueError("every k must be in 1 .. min(%d, D = %d)" % (MAX_GROUPS, D))
    B = int(replicates)
    if B < 1 or B > 2 ** 31 - 1:
        raise ValueError("replicates must be in 1 .. 2^31 - 1")
    if len(kl) * B * D >= 2 ** 31:
        raise ValueError("len(ks) x replicates x D = %d labels (limit 2^31 - 1)" % (len(kl) * B * D))
    keep = _keep(subsample)
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 bits, unsigned")
    if int(maxiter) < 1:
        raise ValueError("maxiter must be >= 1")
    lo, hi = _per_mille(pac)
    if k is not None and int(k) not in kl:
        raise ValueError("k = %r is not one of ks" % (k,))
    ctx = ctx or mctx or _lib.default_context()
    r = _raw(ctx, x, kl, B, 0, keep, seed, 0, maxiter, lo, hi)
    tog, same = r["together"], r["same"]
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.where(r["valid"] > 0, r["ambiguous"] / r["valid"].astype(np.float64), np.nan)
        cons = np.where(tog > 0, same / np.maximum(tog, 1).astype(np.float64), 0.0)
    pick = kl.index(int(k)) if k is not None else _pick(p, kl)
    by_k = np.stack([average_linkage(1.0 - cons[i], kl[i]) for i in range(len(kl))])
    item, clus = _item_consensus(cons[pick], by_k[pick])
    skipped = ((r["labels"] >= 0).sum(axis=2) == 0).sum(axis=1)
    return SampleClusters(np.array(kl), p, kl[pick], by_k[pick].copy(), by_k, cons if counts else None, tog if counts else None, item, clus, r["iters"],
                          r["inertia"], skipped, (r["iters"] == int(maxiter)).sum(axis=1), B)
