"""Exposures against survival: do the groups of `cluster_samples` differ in survival, which signature's exposure goes with hazard, and above
which exposure does a tumour count as "high" -- the questions after `associate_exposures`, whose ranks cannot take a censored time.

Every test is a permutation test in the log-rank (Savage) scores a_i = event_i - H(t_i), H the Nelson-Aalen estimate: the log-rank test of a
group covariate, the Cox score test of a ranked exposure (trend), and the maximally selected log-rank statistic over every cutpoint of an
exposure, whose p-value is corrected for the scan by permuting the whole scan.  The outcome rows are permuted jointly `permutations` times in
one launch (`mmm_survival_association`, one workgroup per permutation): exact for exposures that are mostly zeros and for small groups, with
Westfall-Young max-T adjustment over the signatures, and with a confounder held fixed by permuting inside `strata` only.  The scores are
quantised to integers (2^-24), so the same arguments give the same bits on every run; the definition is in include/mmmusig.h (DESIGN.md
section 4.20).  Missing values are not handled: drop or impute them before the call."""
import math
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .associate import _midranks2, _missing, benjamini_hochberg
from .cluster import _features

MAX_SAMPLES = 4096
MAX_FEATURES = 256
MAX_LEVELS = 256
MAX_STRATA = 64
SCALE = 16777216.0

GroupTest = namedtuple("GroupTest", "name chi2 p levels observed expected n")
GroupTest.__doc__ = """chi2: the statistic (with two levels the log-rank chi-square with the permutation variance, else the sum of the one-against-rest
statistics); p: (1 + ge) / (1 + B); levels: the level values; observed, expected: events per level, seen and expected under no difference
(within strata); n: samples per level."""
KMCurve = namedtuple("KMCurve", "times survival at_risk median")
KMCurve.__doc__ = """the product-limit estimate: times: the distinct event times, ascending; survival: S just after each; at_risk: the samples at risk
just before each; median: the first time with S <= 0.5, None where the curve does not reach it."""
_SurvivalAssociations = namedtuple("SurvivalAssociations", "z p p_adj q cut_value n_high z_cut p_cut p_cut_adj groups permutations")


class SurvivalAssociations(_SurvivalAssociations):
    """Per signature ([P] each): z: the signed root of the trend statistic, positive when higher exposure goes with more events than expected;
    p: (1 + ge) / (1 + B); p_adj: the max-T adjusted p over the signatures; q: Benjamini-Hochberg over the P raw p-values; cut_value: the
    selected cutpoint, "high" means exposure > cut_value (NaN where no cut is allowed); n_high: the samples above it; z_cut: the signed root of
    the statistic at that cut, positive when the high group has more events than expected; p_cut: its p-value corrected for the scan over the
    cuts; p_cut_adj: corrected over the signatures as well.  The cut columns are None with cutpoints=False.  groups: a GroupTest per group
    covariate.  permutations: B."""
    __slots__ = ()

    def significant(self, alpha=0.05, adjusted=True):
        """the signatures with p_adj (adjusted=True) or q (False) at most alpha"""
        v = self.p_adj if adjusted else self.q
        return [int(i) for i in np.flatnonzero(v <= float(alpha))]

    def table(self):
        """one row per signature (dicts of feature, z, p, p_adj, q and, with cutpoints, cut_value, n_high, z_cut, p_cut, p_cut_adj), then one per
        group covariate (dicts of group, chi2, p)"""
        rows = []
        for i in range(self.p.size):
            row = dict(feature=i, z=float(self.z[i]), p=float(self.p[i]), p_adj=float(self.p_adj[i]), q=float(self.q[i]))
            if self.p_cut is not None:
                row.update(cut_value=float(self.cut_value[i]), n_high=int(self.n_high[i]), z_cut=float(self.z_cut[i]), p_cut=float(self.p_cut[i]),
                           p_cut_adj=float(self.p_cut_adj[i]))
            rows.append(row)
        return rows + [dict(group=g.name, chi2=g.chi2, p=g.p) for g in self.groups]


def _strata_members(D, strata):
    if strata is None:
        return [np.arange(D)]
    lv, s = np.unique(np.asarray(strata), return_inverse=True)
    return [np.flatnonzero(s.reshape(-1) == c) for c in range(lv.size)]


def survival_scores(time, event, strata=None):
    """The log-rank scores of mmm_survival_association, on the host -> (a [D] float64, A [D] int32).  Per stratum, over its distinct event
    times u_j ascending: d_j events at u_j, n_j samples with time >= u_j, H_i = the running sum of d_j / n_j up to time_i, a_i = event_i - H_i,
    A_i = rint(a_i 2^24).  strata: [D] labels of any type, or None."""
    time = np.asarray(time, dtype=np.float64) + 0.0
    event = np.asarray(event)
    if time.ndim != 1 or event.shape != time.shape or (strata is not None and np.shape(strata) != time.shape):
        raise ValueError("time, event and strata must be [D]")
    if not np.isfinite(time).all() or (time < 0).any():
        raise ValueError("time holds an entry that is not finite or is negative")
    if not np.isin(event, (0, 1)).all():
        raise ValueError("event must hold 0 or 1")
    ev = event.astype(np.int64)
    a = np.zeros(time.size)
    for mem in _strata_members(time.size, strata):
        t, e = time[mem], ev[mem]
        u, dj = np.unique(t[e == 1], return_counts=True)
        if u.size == 0:
            continue
        ts = np.sort(t)
        nj = t.size - np.searchsorted(ts, u, side="left")
        H = np.cumsum(dj.astype(np.float64) / nj.astype(np.float64))              # a sequential sum, ascending
        k = np.searchsorted(u, t, side="right")
        a[mem] = e - np.where(k > 0, H[np.maximum(k, 1) - 1], 0.0)
    return a, np.rint(a * SCALE).astype(np.int32)


def _raw(ctx, x, levels, groups, time, event, strata, m_lo, B, b0=0, seed=0, stream=0, waves=0, outputs=("z_trend", "u_group", "maxstat")):
    """mmm_survival_association on x [D, P], groups [D, C] (or None) -> dict of obs_trend [P], obs_group [C], ge_trend, gemax_trend [P], ge_group
    [C], with m_lo >= 1 obs_cut, cut_at, ge_cut, gemax_cut [P] and, where asked for, z_trend [P], u_group [Q] int64, maxstat [B, 2]"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    levels = np.ascontiguousarray(levels, dtype=np.int32).reshape(-1)
    time = np.ascontiguousarray(time, dtype=np.float64)
    event = np.ascontiguousarray(event, dtype=np.uint8)
    if x.ndim != 2 or time.shape != (x.shape[0],) or event.shape != time.shape:
        raise ValueError("x must be [D, P], time and event [D], got %r, %r, %r" % (x.shape, time.shape, event.shape))
    D, P = x.shape
    C, B = levels.size, int(B)
    g = None
    if C:
        g = np.ascontiguousarray(groups, dtype=np.int32)
        if g.shape != (D, C):
            raise ValueError("groups must be [D, C]")
    st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32)
    if st is not None and st.shape != (D,):
        raise ValueError("strata must be [D]")
    Q = int(levels.sum())
    out = {"obs_trend": np.zeros(P), "obs_group": np.zeros(C), "ge_trend": np.zeros(P, dtype=np.uint32), "gemax_trend": np.zeros(P, dtype=np.uint32),
           "ge_group": np.zeros(C, dtype=np.uint32)}
    if m_lo >= 1:
        out.update(obs_cut=np.zeros(P), cut_at=np.zeros(P, dtype=np.int32), ge_cut=np.zeros(P, dtype=np.uint32), gemax_cut=np.zeros(P, dtype=np.uint32))
    if "z_trend" in outputs:
        out["z_trend"] = np.zeros(P, dtype=np.int64)
    if "u_group" in outputs:
        out["u_group"] = np.zeros(max(Q, 0), dtype=np.int64)
    if "maxstat" in outputs:
        out["maxstat"] = np.zeros((max(B, 0), 2))
    # an empty array still needs an address: NULL says "not given"
    one = np.zeros(1)
    addr = lambda a: a.ctypes.data if a.size else one.ctypes.data
    opt = lambda name: addr(out[name]) if name in out else None
    rc = lib().mmm_survival_association(ctx.h, int(D), int(P), addr(x), int(C), addr(levels) if C else None, addr(g) if C else None, addr(time), addr(event),
                                        None if st is None else addr(st), int(m_lo), B, int(b0), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(waves),
                                        addr(out["obs_trend"]), opt("z_trend"), addr(out["obs_group"]), opt("u_group"), opt("obs_cut"), opt("cut_at"),
                                        addr(out["ge_trend"]), addr(out["gemax_trend"]), opt("ge_cut"), opt("gemax_cut"), addr(out["ge_group"]), opt("maxstat"))
    check(rc, ctx.h, "mmm_survival_association")
    return out


def _codes(col, name, D):
    col = np.asarray(col)
    if col.ndim != 1 or col.shape[0] != D:
        raise ValueError("%s has shape %r, not (%d,)" % (name, col.shape, D))
    if _missing(col):
        raise ValueError("%s holds a missing value (NaN or None); missing values are not handled" % name)
    try:
        lv, codes = np.unique(col, return_inverse=True)
    except TypeError:
        raise ValueError("the labels of %s cannot be ordered" % name)
    return lv, codes.reshape(-1).astype(np.int32)


def _groups(groups, D):
    """-> (names, codes [D, C] int32, levels [C] int32, the level values per covariate)"""
    if groups is None:
        return [], np.zeros((D, 0), dtype=np.int32), np.zeros(0, dtype=np.int32), []
    if isinstance(groups, dict):
        names, cols = [str(k) for k in groups], [np.asarray(v) for v in groups.values()]
    else:
        arr = np.asarray(groups)
        if arr.ndim == 1:
            arr = arr[:, None]
        if arr.ndim != 2:
            raise ValueError("groups must be a [D, C] array or a dict of label columns")
        names, cols = ["group%d" % j for j in range(arr.shape[1])], [arr[:, j] for j in range(arr.shape[1])]
    values, codes = [], np.zeros((D, len(cols)), dtype=np.int32)
    for j, (name, col) in enumerate(zip(names, cols)):
        lv, codes[:, j] = _codes(col, "group covariate %r" % name, D)
        values.append(lv)
    return names, codes, np.array([v.size for v in values], dtype=np.int32), values


def _outcome(time, event, D):
    t, e = np.asarray(time), np.asarray(event)
    for name, col in (("time", t), ("event", e)):
        if col.ndim != 1 or col.shape[0] != D:
            raise ValueError("%s has shape %r, not (%d,)" % (name, col.shape, D))
        if _missing(col):
            raise ValueError("%s holds a missing value (NaN or None); missing values are not handled" % name)
    try:
        t = t.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError("time is not numeric")
    if not np.isfinite(t).all() or (t < 0).any():
        raise ValueError("time holds an entry that is not finite or is negative")
    try:
        ok = np.isin(e, (0, 1)).all()
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("event must hold 0 (censored) or 1 (the event was seen)")
    return t, e.astype(np.uint8)


def _centred(f, A, members):
    """T - E of the integer column f under the identity, for a sign"""
    return float(sum(float((f[m] * A[m]).sum()) - float(f[m].sum()) * float(A[m].sum()) / m.size for m in members))


def survival_association(E, time, event, groups=None, strata=None, cutpoints=True, min_fraction=0.1, permutations=10000, seed=0, modalities=None, ctx=None):
    """Permutation tests of exposures and sample groups against a censored survival outcome on the GPU -> SurvivalAssociations.

    E: a [D, P] array of features per sample; a fitted LDA / ILDA (its normalised θ); a fitted MMCTM / IMMCTM (the signature probabilities of
    `modalities`, default all, side by side) -- the features `cluster_samples` takes.  time: [D] >= 0; event: [D], 1 (or True) where the event
    was seen at `time`, 0 where the sample was censored there.  groups: a [D, C] array or a dict name -> column of labels of any type, coded
    by np.unique; `SampleClusters.labels` is a valid column as it stands.  strata: [D] labels of any type (at most 64 distinct); the outcome
    rows are permuted inside a stratum only and every test is the stratified one.  cutpoints: also scan every cutpoint of every signature
    that leaves at least max(1, ceil(min_fraction D)) samples on either side.  permutations: B joint permutations of the outcome rows, drawn
    from Philox words of (seed, permutation index).  D <= 4096, P <= 256, at most 256 levels over all group covariates."""
    mctx, x = _features(E, modalities)
    D, P = x.shape
    if not 1 <= D <= MAX_SAMPLES or not 1 <= P <= MAX_FEATURES:
        raise ValueError("D = %d samples (1 .. %d), P = %d features (1 .. %d)" % (D, MAX_SAMPLES, P, MAX_FEATURES))
    if not np.isfinite(x).all():
        raise ValueError("E holds an entry that is not finite")
    t, ev = _outcome(time, event, D)
    names, codes, levels, values = _groups(groups, D)
    if int(levels.sum()) > MAX_LEVELS:
        raise ValueError("the group covariates have %d levels (limit %d)" % (int(levels.sum()), MAX_LEVELS))
    st = None
    if strata is not None:
        lv, st = _codes(strata, "strata", D)
        if lv.size > MAX_STRATA:
            raise ValueError("strata has %d distinct labels (limit %d)" % (lv.size, MAX_STRATA))
    m_lo = 0
    if cutpoints:
        if not 0.0 <= float(min_fraction) <= 0.5:
            raise ValueError("min_fraction must lie in 0 .. 0.5")
        m_lo = min(max(1, int(math.ceil(float(min_fraction) * D))), max(1, D // 2))
    try:
        B = int(permutations)
    except (TypeError, ValueError):
        raise ValueError("permutations must be an integer")
    if B != permutations or not 1 <= B <= 2 ** 31 - 1:
        raise ValueError("permutations must be an integer in 1 .. 2^31 - 1")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 bits, unsigned")
    ctx = ctx or mctx or _lib.default_context()
    r = _raw(ctx, x, levels, codes, t, ev, st, m_lo, B, 0, seed, 0, 0, outputs=("z_trend", "u_group"))
    # the descriptive columns, on the host from the returned integers
    A = survival_scores(t, ev, st)[1].astype(np.int64)
    members = _strata_members(D, st)
    rx = np.stack([_midranks2(x[:, p]) for p in range(P)], axis=1)
    z = np.array([np.sign(_centred(rx[:, p], A, members)) for p in range(P)]) * np.sqrt(r["obs_trend"])
    p = (1.0 + r["ge_trend"]) / (1.0 + B)
    cut = dict(cut_value=None, n_high=None, z_cut=None, p_cut=None, p_cut_adj=None)
    if m_lo:
        at = r["cut_at"].astype(np.int64)
        cut_value, sign = np.full(P, np.nan), np.zeros(P)
        for j in np.flatnonzero(at > 0):
            order = np.lexsort((np.arange(D), x[:, j] + 0.0))
            cut_value[j] = x[order[at[j] - 1], j]
            low = np.zeros(D, dtype=np.int64)
            low[order[:at[j]]] = 1
            sign[j] = -np.sign(_centred(low, A, members))
        cut = dict(cut_value=cut_value, n_high=np.where(at > 0, D - at, 0), z_cut=sign * np.sqrt(r["obs_cut"]), p_cut=(1.0 + r["ge_cut"]) / (1.0 + B),
                   p_cut_adj=(1.0 + r["gemax_cut"]) / (1.0 + B))
    tests, q0 = [], 0
    for c, name in enumerate(names):
        G = int(levels[c])
        observed = np.bincount(codes[:, c], weights=ev, minlength=G)
        tests.append(GroupTest(name, float(r["obs_group"][c]) / (2.0 if G == 2 else 1.0), float((1.0 + r["ge_group"][c]) / (1.0 + B)), values[c], observed,
                               observed - r["u_group"][q0:q0 + G] / SCALE, np.bincount(codes[:, c], minlength=G)))
        q0 += G
    return SurvivalAssociations(z, p, (1.0 + r["gemax_trend"]) / (1.0 + B), benjamini_hochberg(p), cut["cut_value"], cut["n_high"], cut["z_cut"], cut["p_cut"],
                                cut["p_cut_adj"], tests, B)


def kaplan_meier(time, event, groups=None):
    """The product-limit survival curves that go with the report, on the host.  groups=None -> one KMCurve; else a dict label -> KMCurve of the
    samples with that label.  At the distinct event times u_j, ascending: S_j = S_{j-1} (1 - d_j / n_j) from S_0 = 1."""
    t, ev = _outcome(time, event, np.asarray(time).shape[0] if np.asarray(time).ndim == 1 else -1)

    def curve(t, e):
        u, dj = np.unique(t[e == 1] + 0.0, return_counts=True)
        nj = t.size - np.searchsorted(np.sort(t), u, side="left")
        S = np.cumprod(1.0 - dj / nj.astype(np.float64)) if u.size else np.zeros(0)
        below = np.flatnonzero(S <= 0.5)
        return KMCurve(u, S, nj.astype(np.int64), float(u[below[0]]) if below.size else None)

    if groups is None:
        return curve(t, ev)
    lv, codes = _codes(groups, "groups", t.size)
    return {(v.item() if hasattr(v, "item") else v): curve(t[codes == k], ev[codes == k]) for k, v in enumerate(lv)}
