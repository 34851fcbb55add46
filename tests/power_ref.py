"""numpy restatement of mmm_presence_power (include/mmmusig.h) and the cases its tests share.

Built from the restatements that already exist: `presence_ref.presence` (B = 0) for the observed phase, `presence_ref.sets` / `dense` /
`statistic` for every replicate's Λ with its longdouble value and rounding bound, `simulate_ref.mixture` / `thresholds` / `simulate_doc`
for the draws.  It shares nothing with the kernels.  The statistics of a corpus are computed once for the largest B of the cases (replicate
b of a level does not depend on B) and every (B, α) case is cut from them."""
import functools
from collections import namedtuple

import numpy as np

import presence_ref as PR
import refit_ref as R
import simulate_ref as S

# ---- the cases of tests/test_power_cpu.py and tests/test_power_gpu.py --------------------------------------------------------------------------
SHAPES = ((4, 5), (12, 96), (6, 1536))              # and the edge corpus
FRACTIONS = (0.07, 1.0)                             # G = 2: one small fraction, and every draw from the target
FIXED_TOTAL = 50                                    # H = 2: the observed totals, and this one for every sample
CASES = ((24, 0.05), (40, 0.05), (24, 0.2), (40, 0.2))        # (B, α): m = floor(α (B + 1)) - 1 = 0, 1, 4, 7
B_MAX = 40
# the draw seed per corpus, recorded here because tests/test_power_cpu.py asserts that under it no comparison is near a tie (the corpora's
# own seeds were the first tried and pass); stream as the corpus has it
SEEDS = {"C4V5": 20264, "C12V96": 20272, "C6V1536": 20266, "edge": 77}

Levels = namedtuple("Levels", "obs n_level rep rep_ld rep_bound rep_iters")
Levels.__doc__ = """obs: presence_ref.RefOut of the observed phase (B = 0); n_level [H, D] int32; rep, rep_ld, rep_bound [L, B, TD]: Λ, its longdouble
value and rounding bound (NaN for untestable items); rep_iters [L, B, TD] int64."""

Power = namedtuple("Power", "m crit count_reject count_zero iters rep rep_ld rep_bound")
Power.__doc__ = """m; crit [H, TD] (0 for untestable items); count_reject, count_zero [L, TD] int32; iters [TD] int64 (the observed fits and every
level's that ran); rep, rep_ld, rep_bound [L, B, TD] (NaN where nothing ran)."""


def corpora():
    return [PR.corpus(C, V) for C, V in SHAPES] + [PR.edge_corpus()]


def n_levels(c, obs):
    """[2, D]: the observed totals (1 for an empty sample, which is untestable anyway) and FIXED_TOTAL"""
    return np.stack([np.maximum(obs.N, 1), np.full(c.D, FIXED_TOTAL)]).astype(np.int32)


def level_weights(w0, t, phi):
    """the generating weights [C] of a level: w0 itself at φ = 0, else (1 - φ) w0 with φ W0 on the target, W0 the sequential sum of w0"""
    if phi == 0:
        return w0.copy()
    w = (1.0 - np.float64(phi)) * w0
    w[t] = np.float64(phi) * np.cumsum(w0)[-1]
    return w


def levels(c, fractions, n_level, B, seed, stream, b0=0, skip_null=False):
    """Λ of replicate b0 .. b0 + B - 1 of every level l = h (1 + G) + g and every testable item"""
    obs = PR.presence(c, B=0)
    P = R.normalise(c.cat)
    phis = (0.0,) + tuple(fractions)
    H, G1, TD = n_level.shape[0], len(phis), obs.status.size
    L = H * G1
    rep, rep_ld, rep_bound = (np.full((L, B, TD), np.nan) for _ in range(3))
    rep_iters = np.zeros((L, B, TD), np.int64)
    for j in range(TD):
        if obs.status[j] == 3:
            continue
        d, t, A0, A1 = PR.sets(c, j)
        for l in range(L):
            h, g = divmod(l, G1)
            if g == 0 and skip_null:
                continue
            _, Tv, _ = S.thresholds(S.mixture(level_weights(obs.w_null[j], t, phis[g]), P))
            draws = S.simulate_doc(Tv, int(n_level[h, d]), l * TD + j, b0 + np.arange(B), seed, stream)
            for b in range(B):
                st = PR.statistic(P, A0, A1, t, draws[b], c.maxiter, c.tol)
                rep[l, b, j], rep_ld[l, b, j], rep_bound[l, b, j], rep_iters[l, b, j] = st.lam, st.lam_ld, st.bound, st.iters
    return Levels(obs, n_level, rep, rep_ld, rep_bound, rep_iters)


def critical(null, alpha):
    """null [B, ...] -> (m, s_{m+1} over the first axis; +inf where m < 0 or m + 1 > B)"""
    B = null.shape[0]
    m = int(np.floor(np.float64(alpha) * np.float64(B + 1))) - 1
    if m < 0 or m + 1 > B:
        return m, np.full(null.shape[1:], np.inf)
    return m, -np.sort(-null, axis=0)[m]


def power(lv, G, alpha, B=None, first=0, crit=None):
    """the outputs of one call over the replicates [first, first + B) of lv; crit [H, TD]: given, the null levels are not run"""
    B = lv.rep.shape[1] - first if B is None else B
    G1 = G + 1
    L, _, TD = lv.rep.shape
    H = L // G1
    live = lv.obs.status != 3
    rep, rep_ld, rep_bound = (x[:, first:first + B].copy() for x in (lv.rep, lv.rep_ld, lv.rep_bound))
    its = lv.rep_iters[:, first:first + B].copy()
    m = int(np.floor(np.float64(alpha) * np.float64(B + 1))) - 1
    if crit is not None:
        for x in (rep, rep_ld, rep_bound):
            x[0::G1] = np.nan
        its[0::G1] = 0
        cr = np.asarray(crit, dtype=np.float64)
    else:
        cr = np.zeros((H, TD))
        cr[:, live] = critical(rep[0::G1][:, :, live].transpose(1, 0, 2), alpha)[1]
    with np.errstate(invalid="ignore"):
        rej = (rep > np.repeat(cr, G1, axis=0)[:, None, :]).sum(axis=1).astype(np.int32)
        zero = (rep == 0).sum(axis=1).astype(np.int32)
    rej[:, ~live] = 0
    if crit is not None:
        rej[0::G1] = 0
    return Power(m, cr, rej, zero, lv.obs.iters + its.sum(axis=(0, 1)), rep, rep_ld, rep_bound)


@functools.lru_cache(maxsize=None)
def reference_levels(i):
    """the B_MAX replicates of every level of corpus i of corpora(), computed once per process"""
    c = corpora()[i]
    obs = PR.presence(c, B=0)
    return levels(c, FRACTIONS, n_levels(c, obs), B_MAX, SEEDS[c.name], c.stream)


def reference(i, B, alpha):
    return power(reference_levels(i), len(FRACTIONS), alpha, B=B)
