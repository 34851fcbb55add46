"""A censored outcome against the exposures together: do the signatures predict survival, how well, and is that better than chance -- the
multivariable question after `survival_association`, which tests one signature at a time, and `classify_exposures`, which takes a binary
label only (dichotomising survival at a time point throws the censoring away and is wrong for samples censored before the cut).

The answer has the design of `classify_exposures`: the cross-validated concordance index (Harrell's C) of a ridge-penalised, stratified Cox
regression (Breslow ties) with a permutation p-value.  The penalty is chosen by the same cross-validation, so the whole scan over the
penalties is permuted: `p_best` covers the choice.  The B permutations x R repeats x F folds x L penalties Newton fits run in one launch
(`mmm_cox_exposures`, one workgroup per permutation).  Every scan and sum has a written order, so the same arguments give the same bits on
every run; the definition is in include/mmmusig.h.  Efron ties, time-varying covariates, L1 or elastic-net
penalties, nested cross-validation, left truncation and missing values are not handled."""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .classify import _column, _integer, best_penalty, standardise
from .cluster import _features
from .survival import _outcome

MAX_SAMPLES = 4096
MAX_FEATURES = 64
MAX_FOLDS = 255
MAX_REPEATS = 64
MAX_PENALTIES = 32
OPTIONAL = ("scores", "u2_obs", "coef", "full_iters", "maxstat")

_ExposureCoxModel = namedtuple("ExposureCoxModel", "c_index c_index_repeats p best p_best penalty penalties coef hazard_ratio names oof_risk events mean scale "
                                                   "n_pairs permutations modalities")


class ExposureCoxModel(_ExposureCoxModel):
    """c_index [L]: the cross-validated concordance index per penalty (the mean over the repeats); c_index_repeats [R, L]; p [L]: (1 + ge) /
    (1 + B) per penalty; best: the index of the largest C, the largest penalty winning ties; p_best: (1 + gemax[best]) / (1 + B), corrected
    for the choice of the penalty; penalty: penalties[best]; coef [P]: the fit on all samples at `best`, log hazard ratios per standard
    deviation of a feature; hazard_ratio: exp(coef); names: the features' names; oof_risk [D]: the out-of-fold linear predictor of every sample
    at `best`, the mean over the repeats (higher = more hazard); events: dict of the fits that stopped at maxiter or lost a pivot, under the
    identity and among the permutations (counted, not raised); mean, scale [P]: the standardisation; n_pairs: the comparable pairs;
    permutations: B."""
    __slots__ = ()

    def predict_risk(self, E_new):
        """the linear predictor (log relative hazard) of new samples: features as in `cox_exposures`, standardised by the kept mean and scale"""
        _, x = _features(E_new, self.modalities)
        if x.shape[1] != self.coef.size:
            raise ValueError("E_new has %d features, the model %d" % (x.shape[1], self.coef.size))
        return ((x - self.mean) / self.scale) @ self.coef

    def risk_groups(self, n=2):
        """[D] int: n quantile groups of `oof_risk` (0 = the lowest risk), to hand to `kaplan_meier(time, event, groups=...)`.  They are for the
        picture, not for a second test: the cut was not part of the permuted procedure, so a log-rank p-value between these groups is not
        valid; `p_best` is the test."""
        n = _integer(n, "n", 2, self.oof_risk.size)
        edges = np.quantile(self.oof_risk, np.arange(1, n) / n)
        return np.searchsorted(edges, self.oof_risk, side="left").astype(np.int64)

    def table(self):
        """one row per penalty (dicts of penalty, c_index, p, best), then one per coefficient of the chosen fit (dicts of feature, coef,
        hazard_ratio)"""
        rows = [dict(penalty=float(v), c_index=float(self.c_index[l]), p=float(self.p[l]), best=l == self.best) for l, v in enumerate(self.penalties)]
        return rows + [dict(feature=n, coef=float(c), hazard_ratio=float(h)) for n, c, h in zip(self.names, self.coef, self.hazard_ratio)]


def make_folds(event, strata, folds, repeats, seed):
    """fold [R, D] uint8: the deal of `classify.make_folds` with the cell (stratum, event).  Per repeat r the generator is
    np.random.default_rng([seed, r]); the cells (stratum ascending, then censored, event) are visited in order, a cell's members (ascending)
    are put in the order of one `permutation` draw and dealt round-robin into the folds, the deal continuing from cell to cell."""
    from .classify import make_folds as deal
    return deal(np.asarray(event).astype(np.uint8), strata, folds, repeats, seed)


def comparable_pairs(time, event, strata=None):
    """the number of comparable pairs of Harrell's C: event sample i with every j of its stratum that has time_j > time_i, or time_j = time_i
    and event_j = 0"""
    t, e = np.asarray(time, dtype=np.float64), np.asarray(event).astype(bool)
    s = np.zeros(t.size, dtype=np.int64) if strata is None else np.asarray(strata)
    n = 0
    for code in np.unique(s):
        m = s == code
        ts, tc = np.sort(t[m]), np.sort(t[m & ~e])
        te = t[m & e]
        n += int((ts.size - np.searchsorted(ts, te, side="right")).sum() + (np.searchsorted(tc, te, side="right") - np.searchsorted(tc, te, side="left")).sum())
    return n


def _raw(ctx, x, time, event, strata, fold, F, lambdas, maxiter, tol, B, b0=0, seed=0, stream=0, waves=0, outputs=OPTIONAL):
    """mmm_cox_exposures on x [D, P], time, event [D], fold [R, D] -> dict of s_obs [L] int64, n_pairs [1] int64, ge, gemax [L] uint32, events [4]
    uint32 and, where asked for, scores [R, L, D], u2_obs [R, L] int64, coef [L, P], full_iters [L, 2] int32, maxstat [B] int64"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    time = np.ascontiguousarray(time, dtype=np.float64)
    event = np.ascontiguousarray(event, dtype=np.uint8)
    fold = np.ascontiguousarray(fold, dtype=np.uint8)
    lam = np.ascontiguousarray(lambdas, dtype=np.float64).reshape(-1)
    if x.ndim != 2 or time.shape != (x.shape[0],) or event.shape != time.shape or fold.ndim != 2 or fold.shape[1] != x.shape[0]:
        raise ValueError("x must be [D, P], time and event [D], fold [R, D], got %r, %r, %r, %r" % (x.shape, time.shape, event.shape, fold.shape))
    D, P = x.shape
    R, L, B = fold.shape[0], lam.size, int(B)
    st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32)
    if st is not None and st.shape != (D,):
        raise ValueError("strata must be [D]")
    out = {"s_obs": np.zeros(L, dtype=np.int64), "n_pairs": np.zeros(1, dtype=np.int64), "ge": np.zeros(L, dtype=np.uint32), "gemax": np.zeros(L, dtype=np.uint32),
           "events": np.zeros(4, dtype=np.uint32)}
    if "scores" in outputs:
        out["scores"] = np.zeros((R, L, D))
    if "u2_obs" in outputs:
        out["u2_obs"] = np.zeros((R, L), dtype=np.int64)
    if "coef" in outputs:
        out["coef"] = np.zeros((L, P))
    if "full_iters" in outputs:
        out["full_iters"] = np.zeros((L, 2), dtype=np.int32)
    if "maxstat" in outputs:
        out["maxstat"] = np.zeros(max(B, 0), dtype=np.int64)
    # an empty array still needs an address: NULL says "not given"
    one = np.zeros(1)
    addr = lambda a: a.ctypes.data if a.size else one.ctypes.data
    opt = lambda name: addr(out[name]) if name in out else None
    rc = lib().mmm_cox_exposures(ctx.h, int(D), int(P), addr(x), addr(time), addr(event), None if st is None else addr(st), int(R), int(F), addr(fold), int(L),
                                 addr(lam), int(maxiter), float(tol), B, int(b0), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(waves), opt("scores"),
                                 opt("u2_obs"), addr(out["s_obs"]), addr(out["n_pairs"]), opt("coef"), opt("full_iters"), addr(out["ge"]), addr(out["gemax"]),
                                 opt("maxstat"), addr(out["events"]))
    check(rc, ctx.h, "mmm_cox_exposures")
    return out


def cox_exposures(E, time, event, strata=None, penalties=(0.1, 1.0, 10.0, 100.0), folds=5, repeats=5, permutations=1000, seed=0, maxiter=30, tol=1e-8,
                  modalities=None, ctx=None):
    """Cross-validated concordance index of a ridge Cox regression of a censored outcome on the exposures, with permutation p-values, on the
    GPU -> ExposureCoxModel.

    E: a [D, P] array of features per sample; a fitted LDA / ILDA (its normalised θ); a fitted MMCTM / IMMCTM (the signature probabilities of
    `modalities`, default all, side by side) -- the features `cluster_samples` takes; they are standardised over all D samples (unsupervised:
    nothing of the outcome leaks).  time: [D] >= 0; event: [D], 1 (or True) where the event was seen at `time`, 0 where the sample was
    censored there.  strata: [D] labels of any type; every stratum has its own baseline hazard, the feature rows are permuted inside a stratum
    only and the folds are balanced inside it.  penalties: the ridge penalties lambda of 1/2 lambda |w|^2 added to the negative log partial
    likelihood.  folds, repeats: F-fold cross-validation, repeated R times with other folds.  permutations: B joint permutations of the
    feature rows against (time, event, folds, stratum), drawn from Philox words of (seed, index).  D <= 4096, P <= 64, F <= min(255, the
    number of events), R <= 64, at most 32 penalties."""
    mctx, x = _features(E, modalities)
    D, P = x.shape
    if not 2 <= D <= MAX_SAMPLES or not 1 <= P <= MAX_FEATURES:
        raise ValueError("D = %d samples (2 .. %d), P = %d features (1 .. %d)" % (D, MAX_SAMPLES, P, MAX_FEATURES))
    if not np.isfinite(x).all():
        raise ValueError("E holds an entry that is not finite")
    t, ev = _outcome(time, event, D)
    st = None
    if strata is not None:
        st = _column(strata, "strata", D)[1].astype(np.int32)
    try:
        lam = np.array([float(v) for v in np.atleast_1d(penalties)], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("penalties must be numbers")
    if not 1 <= lam.size <= MAX_PENALTIES or not (np.isfinite(lam).all() and (lam > 0).all()):
        raise ValueError("penalties must be 1 .. %d positive finite numbers" % MAX_PENALTIES)
    F = _integer(folds, "folds", 2, MAX_FOLDS)
    nev = int(ev.sum())
    if F > nev:
        raise ValueError("folds = %d exceeds the number of events (%d)" % (F, nev))
    R = _integer(repeats, "repeats", 1, MAX_REPEATS)
    B = _integer(permutations, "permutations", 1, 2 ** 31 - 1)
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 bits, unsigned")
    maxiter = _integer(maxiter, "maxiter", 1, 2 ** 31 - 1)
    if not float(tol) >= 0.0:
        raise ValueError("tol must be >= 0")
    n_pairs = comparable_pairs(t, ev, st)
    if n_pairs == 0:
        raise ValueError("no comparable pair: no event sample has a later time, or a censored sample at its own time, in its stratum")
    fold = make_folds(ev, st, F, R, seed)
    for r in range(R):
        for f in range(F):
            if not ev[fold[r] != f].any():
                raise ValueError("the training set of repeat %d, fold %d holds no event: use fewer folds or coarser strata" % (r, f))
    z, mean, scale = standardise(x)
    ctx = ctx or mctx or _lib.default_context()
    r = _raw(ctx, z, t, ev, st, fold, F, lam, maxiter, float(tol), B, 0, seed, 0, 0, outputs=("scores", "u2_obs", "coef", "full_iters"))
    den = 2.0 * n_pairs
    best = best_penalty(r["s_obs"], lam)
    e4 = r["events"]
    events = dict(identity_maxiter=int(e4[0]), identity_pivot=int(e4[1]), permutations_maxiter=int(e4[2]), permutations_pivot=int(e4[3]))
    coef = r["coef"][best].copy()
    return ExposureCoxModel(r["s_obs"] / (R * den), r["u2_obs"] / den, (1.0 + r["ge"]) / (1.0 + B), best, float((1.0 + r["gemax"][best]) / (1.0 + B)), float(lam[best]),
                            lam, coef, np.exp(coef), ["signature%d" % j for j in range(P)], r["scores"][:, best, :].mean(axis=0), events, mean, scale,
                            int(r["n_pairs"][0]), B, modalities)
