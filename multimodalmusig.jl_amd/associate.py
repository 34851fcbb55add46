"""Exposures against sample covariates: which signatures differ between groups of samples, which go with a clinical or genomic covariate --
the cohort-level step after `cluster_samples`, which the MMCTM paper takes on its clusters.

Every (feature, covariate) pair gets a rank statistic -- the tie-corrected Kruskal-Wallis H of a categorical covariate, (D - 1) rho^2 with
Spearman's rho of a numeric one -- and a permutation p-value: the covariate rows are permuted jointly `permutations` times in one launch
(`mmm_associate_exposures`, one workgroup per permutation).  That is exact under the heavy ties of sparse exposures (entries that are exactly
0), the joint permutation gives Westfall-Young max-T adjusted p-values that respect the correlation between signatures, and permuting only
inside `strata` holds a confounder such as the tumour type fixed.  The definition, down to the order of every rounded operation, is in
include/mmmusig.h: the same arguments give the same bits on every run.

The adjustment runs within a covariate (over the features): statistics of covariates with different numbers of levels are not on one scale.
Missing covariate values are not handled: drop or impute them before the call."""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .cluster import _features

MAX_SAMPLES = 4096
MAX_FEATURES = 256
MAX_COLUMNS = 256

_ExposureAssociations = namedtuple("ExposureAssociations", "statistic rho mean_rank p p_adj q permutations names levels")


class ExposureAssociations(_ExposureAssociations):
    """statistic: [P, C] (D - 1) t -- Kruskal-Wallis H (categorical) or (D - 1) rho^2 (numeric); rho: [P, C] Spearman's coefficient, signed, NaN
    for a categorical covariate; mean_rank: list over the covariates of [P, G] mean midranks of the feature per level (NaN for a level without
    members; None for a numeric covariate); p: [P, C] (1 + ge) / (1 + B); p_adj: [P, C] the max-T adjusted (1 + ge_max) / (1 + B), within a
    covariate; q: [P, C] Benjamini-Hochberg over all P C raw p-values; permutations: B; names: the covariates' names; levels: per covariate the
    array of its levels (None for a numeric one)."""
    __slots__ = ()

    def significant(self, alpha=0.05, adjusted=True):
        """(feature, covariate) index pairs with p_adj (adjusted=True) or q (False) at most alpha, in row-major order"""
        v = self.p_adj if adjusted else self.q
        return [(int(i), int(j)) for i, j in np.argwhere(v <= float(alpha))]

    def table(self):
        """one row per (feature, covariate): dicts of feature, covariate, statistic, rho, p, p_adj, q"""
        P, C = self.p.shape
        return [dict(feature=i, covariate=self.names[j], statistic=float(self.statistic[i, j]), rho=float(self.rho[i, j]), p=float(self.p[i, j]),
                     p_adj=float(self.p_adj[i, j]), q=float(self.q[i, j])) for i in range(P) for j in range(C)]


def _raw(ctx, x, levels, y, strata, B, b0=0, seed=0, stream=0, waves=0, outputs=("zc_obs", "maxstat")):
    """mmm_associate_exposures on x [D, P], y [D, C] -> dict of obs [P, C], ge, ge_max [P, C] uint32 and, where asked for, zc_obs [P, Q] int64,
    maxstat [B, C]"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    levels = np.ascontiguousarray(levels, dtype=np.int32)
    if x.ndim != 2 or y.ndim != 2 or levels.ndim != 1 or y.shape != (x.shape[0], levels.size):
        raise ValueError("x must be [D, P], y [D, C] and levels [C], got %r, %r, %r" % (x.shape, y.shape, levels.shape))
    D, P = x.shape
    C, B = levels.size, int(B)
    Q = int(np.where(levels > 0, levels, 1).sum())
    st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32)
    if st is not None and st.shape != (D,):
        raise ValueError("strata must be [D]")
    out = {"obs": np.zeros((P, C)), "ge": np.zeros((P, C), dtype=np.uint32), "ge_max": np.zeros((P, C), dtype=np.uint32)}
    if "zc_obs" in outputs:
        out["zc_obs"] = np.zeros((P, max(Q, 0)), dtype=np.int64)
    if "maxstat" in outputs:
        out["maxstat"] = np.zeros((max(B, 0), C))
    # an empty array still needs an address: NULL says "not given"
    one = np.zeros(1)
    addr = lambda a: a.ctypes.data if a.size else one.ctypes.data
    opt = lambda name: addr(out[name]) if name in out else None
    rc = lib().mmm_associate_exposures(ctx.h, int(D), int(P), addr(x), int(C), addr(levels), addr(y), None if st is None else addr(st), B, int(b0),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(waves), addr(out["obs"]), opt("zc_obs"), addr(out["ge"]),
                                       addr(out["ge_max"]), opt("maxstat"))
    check(rc, ctx.h, "mmm_associate_exposures")
    return out


def benjamini_hochberg(p):
    """Benjamini-Hochberg adjusted p-values of the array p (any shape): q_(i) = min over j >= i of p_(j) m / j, capped at 1"""
    p = np.asarray(p, dtype=np.float64)
    flat = p.ravel()
    m = flat.size
    order = np.argsort(flat, kind="stable")
    scaled = flat[order] * m / np.arange(1, m + 1)
    q = np.empty(m)
    q[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return q.reshape(p.shape)


def _missing(col):
    if col.dtype.kind == "f":
        return bool(np.isnan(col).any())
    if col.dtype.kind == "O":
        return any(v is None or (isinstance(v, float) and v != v) for v in col)
    return False


def _covariates(covariates, kinds, names, D):
    """-> (names, y [D, C] float64, levels [C] int32, the level values per covariate)"""
    if isinstance(covariates, dict):
        if names is not None:
            raise ValueError("names is for an array of covariates; a dict carries its own")
        names = [str(k) for k in covariates]
        cols = [np.asarray(v) for v in covariates.values()]
    else:
        arr = np.asarray(covariates)
        if arr.ndim == 1:
            arr = arr[:, None]
        if arr.ndim != 2:
            raise ValueError("covariates must be a [D, C] array or a dict of columns")
        cols = [arr[:, j] for j in range(arr.shape[1])]
        if names is None:
            names = ["covariate%d" % j for j in range(len(cols))]
        names = [str(n) for n in names]
    C = len(cols)
    if C < 1:
        raise ValueError("no covariate given")
    if len(names) != C:
        raise ValueError("%d names for %d covariates" % (len(names), C))
    if kinds is None:
        kinds = [None] * C
    elif isinstance(kinds, dict):
        unknown = set(kinds) - set(names)
        if unknown:
            raise ValueError("kinds names unknown covariates: %s" % sorted(unknown))
        kinds = [kinds.get(n) for n in names]
    else:
        kinds = list(kinds)
        if len(kinds) != C:
            raise ValueError("%d kinds for %d covariates" % (len(kinds), C))
    y = np.zeros((D, C))
    levels = np.zeros(C, dtype=np.int32)
    values = []
    for j, (name, col, kind) in enumerate(zip(names, cols, kinds)):
        if col.ndim != 1 or col.shape[0] != D:
            raise ValueError("covariate %r has shape %r, not (%d,)" % (name, col.shape, D))
        if kind not in (None, "numeric", "categorical"):
            raise ValueError("kind of covariate %r must be \"numeric\" or \"categorical\"" % name)
        if _missing(col):
            raise ValueError("covariate %r holds a missing value (NaN or None); missing values are not handled" % name)
        if kind is None:
            kind = "numeric" if col.dtype.kind == "f" else "categorical"
        if kind == "numeric":
            try:
                v = col.astype(np.float64)
            except (TypeError, ValueError):
                raise ValueError("covariate %r is not numeric" % name)
            if not np.isfinite(v).all():
                raise ValueError("covariate %r holds an entry that is not finite" % name)
            y[:, j] = v
            values.append(None)
        else:
            try:
                lv, codes = np.unique(col, return_inverse=True)
            except TypeError:
                raise ValueError("the levels of covariate %r cannot be ordered" % name)
            y[:, j] = codes.reshape(-1)
            levels[j] = lv.size
            values.append(lv)
    return names, y, levels, values


def associate_exposures(E, covariates, kinds=None, names=None, strata=None, permutations=10000, seed=0, modalities=None, ctx=None):
    """Permutation tests of exposures against sample covariates on the GPU -> ExposureAssociations.

    E: a [D, P] array of features per sample; a fitted LDA / ILDA (its normalised θ); a fitted MMCTM / IMMCTM (the signature probabilities of
    `modalities`, default all, side by side) -- the features `cluster_samples` takes.  covariates: a [D, C] array or a dict name -> column.
    Boolean, integer and string columns are categorical (levels from np.unique), float columns numeric; kinds (a list, or a dict by name, of
    "numeric" / "categorical" / None) overrides that.  `SampleClusters.labels` is a valid column as it stands.  strata: [D] labels of any
    type; the rows are permuted inside a stratum only, which conditions on it.  permutations: B joint permutations of the covariate rows, drawn
    from Philox words of (seed, permutation index).  D <= 4096, P <= 256, at most 256 columns (one per numeric covariate, one per level)."""
    mctx, x = _features(E, modalities)
    D, P = x.shape
    if not 1 <= D <= MAX_SAMPLES or not 1 <= P <= MAX_FEATURES:
        raise ValueError("D = %d samples (1 .. %d), P = %d features (1 .. %d)" % (D, MAX_SAMPLES, P, MAX_FEATURES))
    if not np.isfinite(x).all():
        raise ValueError("E holds an entry that is not finite")
    names, y, levels, values = _covariates(covariates, kinds, names, D)
    Q = int(np.where(levels > 0, levels, 1).sum())
    if Q > MAX_COLUMNS:
        raise ValueError("the covariates take %d columns (one per numeric covariate, one per level; limit %d)" % (Q, MAX_COLUMNS))
    st = None
    if strata is not None:
        sa = np.asarray(strata)
        if sa.shape != (D,):
            raise ValueError("strata must hold one label per sample")
        if _missing(sa):
            raise ValueError("strata holds a missing value (NaN or None)")
        st = np.unique(sa, return_inverse=True)[1].reshape(-1).astype(np.int32)
    try:
        B = int(permutations)
    except (TypeError, ValueError):
        raise ValueError("permutations must be an integer")
    if B != permutations or not 1 <= B <= 2 ** 31 - 1:
        raise ValueError("permutations must be an integer in 1 .. 2^31 - 1")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 bits, unsigned")
    ctx = ctx or mctx or _lib.default_context()
    r = _raw(ctx, x, levels, y, st, B, 0, seed, 0, 0, outputs=("zc_obs",))
    # the descriptive columns, on the host from the returned integers
    col0 = np.concatenate([[0], np.cumsum(np.where(levels > 0, levels, 1))]).astype(int)
    rho = np.full((P, len(names)), np.nan)
    mean_rank = []
    rx2 = np.stack([_midranks2(x[:, p]) for p in range(P)], axis=1)
    ssx = ((rx2 - (D + 1)) ** 2).sum(axis=0).astype(np.float64)
    for j in range(len(names)):
        if levels[j] == 0:
            ssy = float(((_midranks2(y[:, j]) - (D + 1)) ** 2).sum())
            with np.errstate(invalid="ignore", divide="ignore"):
                rho[:, j] = np.where((ssx > 0) & (ssy > 0), r["zc_obs"][:, col0[j]] / np.sqrt(ssx * ssy), np.nan)
            mean_rank.append(None)
        else:
            n_g = np.bincount(y[:, j].astype(int), minlength=int(levels[j])).astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                # Zc = sum of doubled ranks over the level - (D + 1) n_g; the mean midrank is half the mean doubled rank
                mean_rank.append(np.where(n_g > 0, (r["zc_obs"][:, col0[j]:col0[j + 1]] / n_g + (D + 1)) / 2.0, np.nan))
    p = (1.0 + r["ge"]) / (1.0 + B)
    return ExposureAssociations((D - 1) * r["obs"], rho, mean_rank, p, (1.0 + r["ge_max"]) / (1.0 + B), benjamini_hochberg(p), B, names, values)


def _midranks2(v):
    """doubled midranks 2 #{less} + #{equal} + 1 of a vector, by sorting"""
    v = np.asarray(v, dtype=np.float64) + 0.0              # -0.0 + 0.0 = 0.0: one value for np.unique, as in an IEEE comparison
    u, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    less = np.cumsum(cnt) - cnt
    return (2 * less + cnt + 1)[inv.reshape(-1)].astype(np.int64)
