"""Exposures against sample covariates with continuous confounders held fixed: which signatures go with a clinical or genomic covariate
*after* age, purity, ploidy or mutation burden -- what `strata`, which can only condition on a discrete variable, cannot answer.

Every (feature, covariate) pair gets the partial R^2 of the covariate in the linear model feature ~ adjusters + covariate and a permutation
p-value by the Freedman-Lane scheme (Freedman & Lane 1983; Winkler et al. 2014): the reduced model's residuals are permuted (inside `strata`
if given), the fitted part is added back and the full model is refitted.  By Frisch-Waugh that refit is, per permutation, one product of the
orthonormal design columns with the permuted residuals, which `mmm_regress_exposures` runs for all permutations in one launch (one workgroup
per permutation).  The joint permutation gives Westfall-Young max-T adjusted p-values across the features.  With `ranks=True` (the default)
the features, the numeric tested covariates and the numeric adjusters are replaced by their midranks: partial Spearman, exact under the zeros
of sparse exposures and consistent with `associate_exposures`, whose statistic it equals when there is no adjuster.  The definition, down to
the order of every rounded operation, is in include/mmmusig.h: the same arguments give the same bits on every run.

Missing values, interaction terms and generalised linear models are not handled."""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .associate import _covariates, _midranks2, _missing, benjamini_hochberg
from .cluster import _features

MAX_SAMPLES = 4096
MAX_FEATURES = 64
MAX_ADJUST_COLUMNS = 32
MAX_COLUMNS = 64
COLLINEAR = 1e-8          # a column whose residual on the earlier ones is below this share of its own norm is refused
EXPLAINED = 1e-20         # a feature whose residual norm^2 is below this share of its centred norm^2 gets an exact-zero residual column
CONSTANT = 1e-28          # a feature whose centred norm^2 is below this share of its norm^2 is constant

_ExposureRegressions = namedtuple("ExposureRegressions", "partial_r2 F t coef df p p_adj q permutations names levels")


class ExposureRegressions(_ExposureRegressions):
    """partial_r2: [P, C] the share of the feature's variance left by the adjusters that the covariate explains; F: [P, C] the partial F,
    (r2 / df1) / ((1 - r2) / df2); t: [P, C] the signed t-statistic (t^2 = F) of a covariate with one column, NaN otherwise; coef: [P, C] the
    covariate's coefficient in the full model, per unit of the covariate on the scale the model was fitted on (ranks under ranks=True; level 1
    against level 0 for a two-level covariate), NaN for more than one column; df: [C, 2] (df1, df2) = (columns of the covariate, D - A - df1);
    p: [P, C] (1 + ge) / (1 + B); p_adj: [P, C] the max-T adjusted (1 + ge_max) / (1 + B), within a covariate; q: [P, C] Benjamini-Hochberg
    over all P C raw p-values; permutations: B; names: the tested covariates' names; levels: per covariate the array of its levels (None for a
    numeric one)."""
    __slots__ = ()

    def significant(self, alpha=0.05, adjusted=True):
        """(feature, covariate) index pairs with p_adj (adjusted=True) or q (False) at most alpha, in row-major order"""
        v = self.p_adj if adjusted else self.q
        return [(int(i), int(j)) for i, j in np.argwhere(v <= float(alpha))]

    def table(self):
        """one row per (feature, covariate): dicts of feature, covariate, partial_r2, F, t, coef, p, p_adj, q"""
        P, C = self.p.shape
        return [dict(feature=i, covariate=self.names[j], partial_r2=float(self.partial_r2[i, j]), F=float(self.F[i, j]), t=float(self.t[i, j]),
                     coef=float(self.coef[i, j]), p=float(self.p[i, j]), p_adj=float(self.p_adj[i, j]), q=float(self.q[i, j])) for i in range(P) for j in range(C)]


def _raw(ctx, e, qz, cols, w, strata, B, b0=0, seed=0, stream=0, waves=0, outputs=("u_obs", "rz_obs", "maxstat")):
    """mmm_regress_exposures on e [D, P], qz [D, A] (or None), w [D, Q] -> dict of obs [P, C], ge, ge_max [P, C] uint32 and, where asked for,
    u_obs [P, Q], rz_obs [P], maxstat [B, C]"""
    e = np.ascontiguousarray(e, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    if e.ndim != 2 or w.ndim != 2 or cols.ndim != 1 or w.shape[0] != e.shape[0]:
        raise ValueError("e must be [D, P], w [D, Q] and cols [C], got %r, %r, %r" % (e.shape, w.shape, cols.shape))
    D, P = e.shape
    qz = None if qz is None else np.ascontiguousarray(qz, dtype=np.float64).reshape(D, -1)
    A = 0 if qz is None else qz.shape[1]
    C, B, Q = cols.size, int(B), w.shape[1]
    if int(cols.sum()) != Q:
        raise ValueError("cols sums to %d, w has %d columns" % (int(cols.sum()), Q))
    st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32)
    if st is not None and st.shape != (D,):
        raise ValueError("strata must be [D]")
    out = {"obs": np.zeros((P, C)), "ge": np.zeros((P, C), dtype=np.uint32), "ge_max": np.zeros((P, C), dtype=np.uint32)}
    if "u_obs" in outputs:
        out["u_obs"] = np.zeros((P, Q))
    if "rz_obs" in outputs:
        out["rz_obs"] = np.zeros(P)
    if "maxstat" in outputs:
        out["maxstat"] = np.zeros((max(B, 0), C))
    # an empty array still needs an address: NULL says "not given"
    one = np.zeros(1)
    addr = lambda a: a.ctypes.data if a.size else one.ctypes.data
    opt = lambda name: addr(out[name]) if name in out else None
    rc = lib().mmm_regress_exposures(ctx.h, int(D), int(P), addr(e), int(A), None if A == 0 else addr(qz), int(C), addr(cols), addr(w),
                                     None if st is None else addr(st), B, int(b0), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(waves), addr(out["obs"]),
                                     opt("u_obs"), opt("rz_obs"), addr(out["ge"]), addr(out["ge_max"]), opt("maxstat"))
    check(rc, ctx.h, "mmm_regress_exposures")
    return out


def _midranks(v):
    return _midranks2(v) / 2.0


def _columns(y, levels, ranks):
    """per covariate its block of model columns: the values (or their midranks) of a numeric one, the indicators of the levels 1 .. G-1 of a
    categorical one"""
    blocks = []
    for j in range(y.shape[1]):
        G = int(levels[j])
        if G == 0:
            blocks.append((_midranks(y[:, j]) if ranks else y[:, j].copy())[:, None])
        else:
            blocks.append(np.stack([(y[:, j] == g).astype(np.float64) for g in range(1, G)], axis=1) if G > 1 else np.zeros((y.shape[0], 0)))
    return blocks


def _residual(Q, v):
    """v minus its projection on the orthonormal columns of Q, applied twice (the second pass removes what rounding left)"""
    for _ in range(2):
        if Q.shape[1]:
            v = v - Q @ (Q.T @ v)
    return v


def _design(x, y, levels, names, ay, alevels, anames, ranks=True):
    """The inputs of mmm_regress_exposures by Gram-Schmidt applied twice -> dict of e [D, P], qz [D, A], cols [C] int32, w [D, Q] and
    scale [C] (the norm of a one-column covariate's residual on the adjusters, NaN otherwise).  x [D, P] features; y, levels, names: the
    tested covariates as `associate._covariates` returns them; ay, alevels, anames: the adjusters likewise (ay may have no column).  The
    adjustment space is the intercept, the numeric adjusters and G - 1 indicators per categorical adjuster, in that order of columns."""
    D, P = x.shape
    qz = np.full((D, 1), 1.0 / np.sqrt(D))
    for name, block in zip(anames, _columns(ay, alevels, ranks)):
        for k in range(block.shape[1]):
            v = block[:, k]
            r = _residual(qz, v)
            if not np.linalg.norm(r) > COLLINEAR * np.linalg.norm(v):
                raise ValueError("adjuster %r is a linear combination of the intercept and the adjusters before it" % name)
            qz = np.concatenate([qz, (r / np.linalg.norm(r))[:, None]], axis=1)
    A = qz.shape[1]
    ws, cols, scale = [], [], []
    for name, block in zip(names, _columns(y, levels, ranks)):
        if block.shape[1] == 0:
            raise ValueError("covariate %r has a single level: it is a linear combination of the adjusters" % name)
        wc = np.zeros((D, 0))
        for k in range(block.shape[1]):
            v = block[:, k]
            r = _residual(np.concatenate([qz, wc], axis=1), v)
            if not np.linalg.norm(r) > COLLINEAR * np.linalg.norm(v):
                raise ValueError("covariate %r is a linear combination of the adjusters%s" % (name, " and its own earlier levels" if k else ""))
            wc = np.concatenate([wc, (r / np.linalg.norm(r))[:, None]], axis=1)
        if D - A - wc.shape[1] < 1:
            raise ValueError("covariate %r leaves D - A - columns = %d - %d - %d residual degrees of freedom (at least 1 is needed)" % (name, D, A, wc.shape[1]))
        ws.append(wc)
        cols.append(wc.shape[1])
        scale.append(float(np.linalg.norm(_residual(qz, block[:, 0]))) if wc.shape[1] == 1 else np.nan)
    xr = np.stack([_midranks(x[:, p]) for p in range(P)], axis=1) if ranks else x
    e = _residual(qz, xr)
    cen = xr - xr.mean(axis=0)[None, :]
    cen2, raw2, res2 = (cen * cen).sum(axis=0), (xr * xr).sum(axis=0), (e * e).sum(axis=0)
    e[:, (cen2 <= CONSTANT * raw2) | (res2 <= EXPLAINED * cen2)] = 0.0          # constant, or explained by the adjusters: p = 1
    return dict(e=np.ascontiguousarray(e), qz=qz, cols=np.array(cols, dtype=np.int32), w=np.concatenate(ws, axis=1), scale=np.array(scale))


def regress_exposures(E, covariates, adjust, kinds=None, adjust_kinds=None, names=None, strata=None, ranks=True, permutations=10000, seed=0, modalities=None,
                      ctx=None):
    """Freedman-Lane permutation tests of exposures against covariates given adjusters, on the GPU -> ExposureRegressions.

    E: a [D, P] array of features per sample; a fitted LDA / ILDA (its normalised θ); a fitted MMCTM / IMMCTM (the signature probabilities of
    `modalities`, default all, side by side) -- the features `associate_exposures` takes.  covariates: the tested covariates, a [D, C] array or
    a dict name -> column, read as in `associate_exposures` (boolean, integer and string columns categorical, float columns numeric; `kinds`
    overrides).  adjust: the confounders to hold fixed, in the same forms (`adjust_kinds` overrides; None = none, the intercept alone).  A
    categorical column of G levels enters as G - 1 indicators.  ranks=True replaces the features, the numeric tested covariates and the numeric
    adjusters by their midranks (partial Spearman); ranks=False is the plain linear model on the values given.  strata: [D] labels of any
    type; the residuals are permuted inside a stratum only.  permutations: B joint permutations, drawn from Philox words of (seed, permutation
    index).  A tested covariate or an adjuster that is a linear combination of the columns before it is refused by name.  D <= 4096, P <= 64,
    at most 32 adjustment columns (the intercept included) and 64 tested columns; every covariate must leave a residual degree of freedom."""
    mctx, x = _features(E, modalities)
    D, P = x.shape
    if not 1 <= D <= MAX_SAMPLES or not 1 <= P <= MAX_FEATURES:
        raise ValueError("D = %d samples (1 .. %d), P = %d features (1 .. %d)" % (D, MAX_SAMPLES, P, MAX_FEATURES))
    if not np.isfinite(x).all():
        raise ValueError("E holds an entry that is not finite")
    names, y, levels, values = _covariates(covariates, kinds, names, D)
    if adjust is None or (isinstance(adjust, dict) and not adjust):
        if adjust_kinds:
            raise ValueError("adjust_kinds without adjusters")
        anames, ay, alevels = [], np.zeros((D, 0)), np.zeros(0, dtype=np.int32)
    else:
        an = None
        if not isinstance(adjust, dict):
            shape = np.shape(adjust)
            an = ["adjust%d" % j for j in range(1 if len(shape) == 1 else shape[1])] if len(shape) in (1, 2) else None
        anames, ay, alevels, _ = _covariates(adjust, adjust_kinds, an, D)
    if not isinstance(ranks, (bool, np.bool_)):
        raise ValueError("ranks must be True or False")
    A = 1 + int(np.where(alevels > 0, alevels - 1, 1).sum())
    Q = int(np.where(levels > 0, np.maximum(levels - 1, 1), 1).sum())
    if A > MAX_ADJUST_COLUMNS:
        raise ValueError("the adjusters take %d columns (the intercept, one per numeric adjuster, one per level but the first; limit %d)" % (A, MAX_ADJUST_COLUMNS))
    if Q > MAX_COLUMNS:
        raise ValueError("the covariates take %d columns (one per numeric covariate, one per level but the first; limit %d)" % (Q, MAX_COLUMNS))
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
    d = _design(x, y, levels, names, ay, alevels, anames, bool(ranks))
    ctx = ctx or mctx or _lib.default_context()
    r = _raw(ctx, d["e"], d["qz"], d["cols"], d["w"], st, B, 0, seed, 0, 0, outputs=("u_obs", "rz_obs"))
    return _report(r, d, D, B, names, values)


def _report(r, d, D, B, names, values):
    """the reported columns, on the host from the returned statistics"""
    cols = d["cols"].astype(np.int64)
    A = d["qz"].shape[1]
    df = np.stack([cols, D - A - cols], axis=1)
    r2 = r["obs"]
    with np.errstate(invalid="ignore", divide="ignore"):
        F = (r2 / df[None, :, 0]) / ((1.0 - r2) / df[None, :, 1])
    col0 = np.concatenate([[0], np.cumsum(cols)]).astype(int)
    t = np.full(r2.shape, np.nan)
    coef = np.full(r2.shape, np.nan)
    for j in range(len(names)):
        if cols[j] == 1:
            u = r["u_obs"][:, col0[j]]
            with np.errstate(invalid="ignore"):
                t[:, j] = np.sign(u) * np.sqrt(F[:, j])
            coef[:, j] = u / d["scale"][j]
    p = (1.0 + r["ge"]) / (1.0 + B)
    return ExposureRegressions(r2, F, t, coef, df, p, (1.0 + r["ge_max"]) / (1.0 + B), benjamini_hochberg(p), B, names, values)
