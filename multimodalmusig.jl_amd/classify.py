"""A binary label against the exposures together: how well do the signatures predict BRCA1/2 status, HR deficiency or response, and is that
better than chance -- the multivariable question after `associate_exposures` and `survival_association`, which test one signature at a time.

The answer is the cross-validated AUC of a ridge-penalised logistic regression with a permutation p-value
(`sklearn.model_selection.permutation_test_score` has the same design for one penalty).  The penalty is chosen by the same cross-validation,
so the whole scan over the penalties is permuted: `p_best` covers the choice.  The B permutations x R repeats x F folds x L penalties Newton
fits run in one launch (`mmm_classify_exposures`, one workgroup per permutation).  Every sum has a written order, so the same arguments give
the same bits on every run; the definition is in include/mmmusig.h.  Missing values, more than two classes, class
weights, L1 penalties and nested cross-validation are not handled."""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .associate import _missing
from .cluster import _features

MAX_SAMPLES = 4096
MAX_FEATURES = 63
MAX_FOLDS = 255
MAX_REPEATS = 64
MAX_PENALTIES = 32
OPTIONAL = ("scores", "u2_obs", "coef", "full_iters", "maxstat")

_ExposureClassifier = namedtuple("ExposureClassifier", "auc auc_repeats p best p_best penalty penalties intercept coef names oof_score events mean scale classes "
                                                       "permutations modalities")


class ExposureClassifier(_ExposureClassifier):
    """auc [L]: the cross-validated AUC per penalty (the mean over the repeats); auc_repeats [R, L]; p [L]: (1 + ge) / (1 + B) per penalty;
    best: the index of the largest AUC, the largest penalty winning ties; p_best: (1 + gemax[best]) / (1 + B), corrected for the choice of the
    penalty; penalty: penalties[best]; intercept, coef [P]: the fit on all samples at `best`, in standardised units; names: the features'
    names; oof_score [D]: the out-of-fold score of every sample at `best`, the mean over the repeats; events: dict of the fits that stopped at
    maxiter or lost a pivot, under the identity and among the permutations (counted, not raised); mean, scale [P]: the standardisation;
    classes: the two label values, the second is the positive one; permutations: B."""
    __slots__ = ()

    def predict_score(self, E_new):
        """the linear score (log-odds of the positive class) of new samples: features as in `classify_exposures`, standardised by the kept mean and scale"""
        _, x = _features(E_new, self.modalities)
        if x.shape[1] != self.coef.size:
            raise ValueError("E_new has %d features, the classifier %d" % (x.shape[1], self.coef.size))
        return self.intercept + ((x - self.mean) / self.scale) @ self.coef

    def predict_proba(self, E_new):
        """the probability of the positive class, classes[1]"""
        return 1.0 / (1.0 + np.exp(-self.predict_score(E_new)))

    def table(self):
        """one row per penalty (dicts of penalty, auc, p, best), then one per coefficient of the chosen fit (dicts of feature, coef)"""
        rows = [dict(penalty=float(v), auc=float(self.auc[l]), p=float(self.p[l]), best=l == self.best) for l, v in enumerate(self.penalties)]
        return rows + [dict(feature="intercept", coef=float(self.intercept))] + [dict(feature=n, coef=float(c)) for n, c in zip(self.names, self.coef)]


def standardise(x):
    """-> (z, mean, scale): mean 0 and population sd 1 per column over all samples; a constant column becomes 0 (scale 1)"""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    const = x.max(axis=0) == x.min(axis=0)
    scale = np.where(const, 1.0, x.std(axis=0))
    z = np.where(const[None, :], 0.0, (x - mean) / scale)
    return np.ascontiguousarray(z), mean, scale


def make_folds(y, strata, folds, repeats, seed):
    """fold [R, D] uint8.  Per repeat r the generator is np.random.default_rng([seed, r]); the cells (stratum ascending, then class 0, 1) are
    visited in order, a cell's members (ascending) are put in the order of one `permutation` draw and dealt round-robin into the folds, the
    deal continuing from cell to cell: inside a cell the folds differ by at most one member."""
    y = np.asarray(y)
    D = y.size
    s = np.zeros(D, dtype=np.int64) if strata is None else np.asarray(strata)
    out = np.zeros((repeats, D), dtype=np.uint8)
    for r in range(repeats):
        rng = np.random.default_rng([int(seed), r])
        nxt = 0
        for code in np.unique(s):
            for c in (0, 1):
                mem = np.flatnonzero((s == code) & (y == c))
                mem = mem[rng.permutation(mem.size)]
                out[r, mem] = (nxt + np.arange(mem.size)) % folds
                nxt += mem.size
    return out


def _raw(ctx, x, y, strata, fold, F, lambdas, maxiter, tol, B, b0=0, seed=0, stream=0, waves=0, outputs=OPTIONAL):
    """mmm_classify_exposures on x [D, P], y [D], fold [R, D] -> dict of s_obs [L] int64, ge, gemax [L] uint32, events [4] uint32 and, where
    asked for, scores [R, L, D], u2_obs [R, L] int64, coef [L, P + 1], full_iters [L, 2] int32, maxstat [B] int64"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.uint8)
    fold = np.ascontiguousarray(fold, dtype=np.uint8)
    lam = np.ascontiguousarray(lambdas, dtype=np.float64).reshape(-1)
    if x.ndim != 2 or y.shape != (x.shape[0],) or fold.ndim != 2 or fold.shape[1] != x.shape[0]:
        raise ValueError("x must be [D, P], y [D], fold [R, D], got %r, %r, %r" % (x.shape, y.shape, fold.shape))
    D, P = x.shape
    R, L, B = fold.shape[0], lam.size, int(B)
    st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32)
    if st is not None and st.shape != (D,):
        raise ValueError("strata must be [D]")
    out = {"s_obs": np.zeros(L, dtype=np.int64), "ge": np.zeros(L, dtype=np.uint32), "gemax": np.zeros(L, dtype=np.uint32), "events": np.zeros(4, dtype=np.uint32)}
    if "scores" in outputs:
        out["scores"] = np.zeros((R, L, D))
    if "u2_obs" in outputs:
        out["u2_obs"] = np.zeros((R, L), dtype=np.int64)
    if "coef" in outputs:
        out["coef"] = np.zeros((L, P + 1))
    if "full_iters" in outputs:
        out["full_iters"] = np.zeros((L, 2), dtype=np.int32)
    if "maxstat" in outputs:
        out["maxstat"] = np.zeros(max(B, 0), dtype=np.int64)
    # an empty array still needs an address: NULL says "not given"
    one = np.zeros(1)
    addr = lambda a: a.ctypes.data if a.size else one.ctypes.data
    opt = lambda name: addr(out[name]) if name in out else None
    rc = lib().mmm_classify_exposures(ctx.h, int(D), int(P), addr(x), addr(y), None if st is None else addr(st), int(R), int(F), addr(fold), int(L), addr(lam),
                                      int(maxiter), float(tol), B, int(b0), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(waves), opt("scores"), opt("u2_obs"),
                                      addr(out["s_obs"]), opt("coef"), opt("full_iters"), addr(out["ge"]), addr(out["gemax"]), opt("maxstat"), addr(out["events"]))
    check(rc, ctx.h, "mmm_classify_exposures")
    return out


def _column(col, name, D):
    col = np.asarray(col)
    if col.ndim != 1 or col.shape[0] != D:
        raise ValueError("%s has shape %r, not (%d,)" % (name, col.shape, D))
    if _missing(col):
        raise ValueError("%s holds a missing value (NaN or None); missing values are not handled" % name)
    try:
        lv, codes = np.unique(col, return_inverse=True)
    except TypeError:
        raise ValueError("the values of %s cannot be ordered" % name)
    return lv, codes.reshape(-1)


def _integer(v, name, lo, hi):
    try:
        n = int(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be an integer" % name)
    if n != v or not lo <= n <= hi:
        raise ValueError("%s must be an integer in %d .. %d" % (name, lo, hi))
    return n


def best_penalty(s_obs, penalties):
    """the index of the largest s_obs; among equals the largest penalty wins"""
    s = np.asarray(s_obs)
    ties = np.flatnonzero(s == s.max())
    return int(ties[np.argmax(np.asarray(penalties)[ties])])


def classify_exposures(E, labels, strata=None, penalties=(0.1, 1.0, 10.0, 100.0), folds=5, repeats=5, permutations=1000, seed=0, maxiter=30, tol=1e-8,
                       modalities=None, ctx=None):
    """Cross-validated AUC of a ridge logistic regression of a binary label on the exposures, with permutation p-values, on the GPU ->
    ExposureClassifier.

    E: a [D, P] array of features per sample; a fitted LDA / ILDA (its normalised θ); a fitted MMCTM / IMMCTM (the signature probabilities of
    `modalities`, default all, side by side) -- the features `cluster_samples` takes; they are standardised over all D samples (unsupervised:
    nothing of the label leaks).  labels: [D], exactly two values by np.unique, the second is the positive class.  strata: [D] labels of any
    type; the feature rows are permuted inside a stratum only and the folds are balanced inside it.  penalties: the ridge penalties lambda of
    1/2 lambda |w|^2 (sklearn's C = 1 / lambda).  folds, repeats: F-fold cross-validation, repeated R times with other folds.
    permutations: B joint permutations of the feature rows against (label, folds, stratum), drawn from Philox words of (seed, index).
    D <= 4096, P <= 63, F <= min(255, n_1, n_0), R <= 64, at most 32 penalties."""
    mctx, x = _features(E, modalities)
    D, P = x.shape
    if not 2 <= D <= MAX_SAMPLES or not 1 <= P <= MAX_FEATURES:
        raise ValueError("D = %d samples (2 .. %d), P = %d features (1 .. %d)" % (D, MAX_SAMPLES, P, MAX_FEATURES))
    if not np.isfinite(x).all():
        raise ValueError("E holds an entry that is not finite")
    classes, y = _column(labels, "labels", D)
    if classes.size != 2:
        raise ValueError("labels takes %d distinct values, not two" % classes.size)
    y = y.astype(np.uint8)
    n1, n0 = int(y.sum()), int(D - y.sum())
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
    if F > min(n1, n0):
        raise ValueError("folds = %d exceeds the smaller class (%d positive, %d negative samples)" % (F, n1, n0))
    R = _integer(repeats, "repeats", 1, MAX_REPEATS)
    B = _integer(permutations, "permutations", 1, 2 ** 31 - 1)
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 bits, unsigned")
    maxiter = _integer(maxiter, "maxiter", 1, 2 ** 31 - 1)
    if not float(tol) >= 0.0:
        raise ValueError("tol must be >= 0")
    fold = make_folds(y, st, F, R, seed)
    for r in range(R):
        for f in range(F):
            if len(set(y[fold[r] != f].tolist())) != 2:
                raise ValueError("the training set of repeat %d, fold %d lacks a class: use fewer folds or coarser strata" % (r, f))
    z, mean, scale = standardise(x)
    ctx = ctx or mctx or _lib.default_context()
    r = _raw(ctx, z, y, st, fold, F, lam, maxiter, float(tol), B, 0, seed, 0, 0, outputs=("scores", "u2_obs", "coef", "full_iters"))
    den = 2.0 * n1 * n0
    best = best_penalty(r["s_obs"], lam)
    ev = r["events"]
    events = dict(identity_maxiter=int(ev[0]), identity_pivot=int(ev[1]), permutations_maxiter=int(ev[2]), permutations_pivot=int(ev[3]))
    return ExposureClassifier(r["s_obs"] / (R * den), r["u2_obs"] / den, (1.0 + r["ge"]) / (1.0 + B), best, float((1.0 + r["gemax"][best]) / (1.0 + B)),
                              float(lam[best]), lam, float(r["coef"][best, 0]), r["coef"][best, 1:].copy(), ["signature%d" % j for j in range(P)],
                              r["scores"][:, best, :].mean(axis=0), events, mean, scale, classes, B, modalities)
