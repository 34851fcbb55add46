"""What is "signature t not detected" worth in this sample? -- the detection power of `signature_presence`, per (target, sample), over a
grid of spiked-in fractions and mutation totals: the limit-of-detection curve of a signature assignment.

For every pair the sample's own null fit is taken as the truth, the target is mixed in at the fraction φ of the mutations, count vectors
of the level's total are drawn from that mixture, and each is put through the presence test's statistic.  The critical value is the one the
presence test itself applies at this B: the (m + 1)-th largest of the B statistics drawn at φ = 0, m = floor(α (B + 1)) - 1, so that
"Λ > crit" is "p <= α".  Draws, both fits, the selection and the comparisons run on the device in one call (`mmm_presence_power`); a
replicate's counts never leave LDS and a block stages a pair's catalogue rows once for all levels.  The definition, down to the order of
every sum, is in include/mmmusig.h.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .ctm import MMCTM
from .models import LDA
from .presence import _corpus, _ptr, _table
from .simulate import _seeds

MAX_LEVELS = 64

_PowerResult = namedtuple("PowerResult", "power size crit count_reject count_zero stat score exposures_null status iters fractions n_mutations alpha B "
                                         "replicates names")


class PowerResult(_PowerResult):
    """power [H, G, T, D] = count_reject / B at total h and fraction g, NaN where the pair is untestable (status 3); size [H, T, D]: the same
    at φ = 0, the attained size of the test (<= α by construction; NaN with `crit` given, where the null levels are not run); crit [H, T, D]:
    the critical value, +inf where the test cannot reject at this B; count_reject [H, G, T, D], count_zero [H, 1 + G, T, D] (fraction 0
    first): replicates with Λ > crit, with Λ = 0; stat, score [T, D], exposures_null [T, C, D], status, iters [T, D]: the observed phase of
    `signature_presence` (iters with every level's fits); fractions [G]; n_mutations [H, D]; alpha; B; replicates: [H, 1 + G, B, T, D] with
    keep_replicates, else None; names: the targets' names where the catalogue has names."""
    __slots__ = ()

    def detectable(self, power=0.8):
        """[H, T, D]: the smallest fraction of the grid whose power reaches `power`, inf where none does (NaN where untestable)"""
        with np.errstate(invalid="ignore"):
            ok = self.power >= float(power)
        f = np.where(ok, np.asarray(self.fractions)[None, :, None, None], np.inf).min(axis=1)
        return np.where(self.status[None] == 3, np.nan, f)

    def needed_mutations(self, fraction, power=0.8):
        """[T, D]: the smallest total of the grid at which the power at `fraction` (a fraction of the grid) reaches `power`, inf where none
        does (NaN where untestable)"""
        g = np.flatnonzero(np.asarray(self.fractions) == float(fraction))
        if g.size != 1:
            raise ValueError("fraction %r is not on the grid %r" % (fraction, list(self.fractions)))
        with np.errstate(invalid="ignore"):
            ok = self.power[:, g[0]] >= float(power)
        n = np.where(ok, self.n_mutations[:, None, :].astype(np.float64), np.inf).min(axis=0)
        return np.where(self.status == 3, np.nan, n)


def _fractions(fractions):
    f = np.atleast_1d(np.asarray(fractions, dtype=np.float64))
    if f.ndim != 1 or not 1 <= f.size <= MAX_LEVELS:
        raise ValueError("fractions must hold 1 .. %d values" % MAX_LEVELS)
    if not (np.all(f > 0) and np.all(f <= 1) and np.all(np.diff(f) > 0)):
        raise ValueError("fractions must increase strictly within (0, 1], got %r" % (f.tolist(),))
    return np.ascontiguousarray(f)


def _levels(n_mutations, D):
    """-> int32 [H, D] or None (the observed totals)"""
    if n_mutations is None:
        return None
    n = np.asarray(n_mutations)
    if n.ndim == 1:
        n = np.repeat(n[:, None], D, axis=1)
    if n.ndim != 2 or n.shape[1] != D or not 1 <= n.shape[0] <= MAX_LEVELS:
        raise ValueError("n_mutations must be None, a list of 1 .. %d totals or an [H, D] array (D = %d), got shape %r" % (MAX_LEVELS, D, np.shape(n_mutations)))
    if n.size and (np.any(n != np.floor(n)) or n.min() < 1 or n.max() >= 2 ** 31):
        raise ValueError("n_mutations must be whole numbers in [1, 2^31)")
    return np.ascontiguousarray(n, dtype=np.int32)


def _raw(ctx, D, V, doc_ptr, term, count, cat, targets, fractions, n_level=None, alpha=0.05, allowed=None, B=0, b0=0, seed=0, stream=0, crit=None, maxiter=1000,
         tol=1e-9, keep=False):
    """mmm_presence_power on one CSR corpus (0-based terms) -> dict of its outputs, level- and item-major ([T D], [T D, C], [H, T D], [L, T D],
    [L, B, T D])"""
    cat = np.ascontiguousarray(cat, dtype=np.float64)
    C = cat.shape[0]
    doc_ptr = np.ascontiguousarray(doc_ptr, dtype=np.int64)
    term = np.ascontiguousarray(term, dtype=np.int32); count = np.ascontiguousarray(count, dtype=np.int32)
    targets = np.ascontiguousarray(targets, dtype=np.int32)
    fractions = np.ascontiguousarray(fractions, dtype=np.float64)
    T, G = targets.size, fractions.size
    TD = T * D
    if allowed is not None:
        allowed = np.ascontiguousarray(allowed, dtype=np.uint8)
        if allowed.shape != (D, C):
            raise ValueError("allowed must be [D, C] = [%d, %d], got %r" % (D, C, allowed.shape))
    H = 1
    if n_level is not None:
        n_level = np.ascontiguousarray(n_level, dtype=np.int32)
        H = n_level.shape[0]
        if n_level.shape != (H, D):
            raise ValueError("n_level must be [H, D], got %r" % (n_level.shape,))
    if crit is not None:
        crit = np.ascontiguousarray(crit, dtype=np.float64)
        if crit.shape != (H, TD):
            raise ValueError("crit must be [H, T D] = [%d, %d], got %r" % (H, TD, crit.shape))
    Lv = H * (1 + G)
    out = dict(w_null=np.zeros((TD, C)), stat=np.zeros(TD), score=np.zeros(TD), w_alt=np.zeros(TD), status=np.zeros(TD, dtype=np.int8),
               iters=np.zeros(TD, dtype=np.int64), crit=np.zeros((H, TD)), count_reject=np.zeros((Lv, TD), dtype=np.int32),
               count_zero=np.zeros((Lv, TD), dtype=np.int32), rep_stat=np.zeros((Lv, B, TD)) if keep else None)
    rc = lib().mmm_presence_power(ctx.h, int(D), C, int(V), doc_ptr, _ptr(term), _ptr(count), cat.ravel(), _ptr(allowed), T, _ptr(targets), G, _ptr(fractions), H,
                                  _ptr(n_level), float(alpha), int(B), int(b0), int(seed), int(stream), int(maxiter), float(tol), _ptr(crit),
                                  *[_ptr(out[k]) for k in ("w_null", "stat", "score", "w_alt", "status", "iters", "crit", "count_reject", "count_zero", "rep_stat")])
    check(rc, ctx.h, "mmm_presence_power")
    return out


def presence_power(X, catalogue, targets, fractions=(0.02, 0.05, 0.1, 0.2), n_mutations=None, alpha=0.05, allowed=None, B=1000, seed=None, stream=0, b0=0,
                   crit=None, maxiter=1000, tol=1e-9, modality=None, keep_replicates=False, ctx=None):
    """Detection power of `signature_presence` at level α for every t of `targets` and every sample of X -> PowerResult.

    X, catalogue, targets, allowed, maxiter, tol, modality as `signature_presence` takes them.  fractions: the grid of spiked-in fractions
    φ, strictly increasing in (0, 1]: the target is given the share φ of the sample's null exposures and the others are scaled by 1 - φ.
    n_mutations: None (every sample at its observed total), a list of H totals applied to every sample, or an [H, D] array.
    Pairs with Λ_obs = 0 and Λ_obs = +inf take part like any other; untestable pairs give NaN.
    B: replicates per level and pair, b0 .. b0 + B - 1 of the sequence (seed, stream) fixes; seed is required.  The level φ = 0 at the
    observed totals draws exactly the replicates of `signature_presence` under the same seed and stream, and every level can be reproduced
    with `simulate_counts`.  The critical value of (total, pair) is taken from the B null replicates of this call: rejection is
    p = (1 + #{Λ_null >= Λ}) / (B + 1) <= α, so B < 1 / α - 1 can never reject (crit = +inf, power 0).
    crit: [H, T, D] critical values of an earlier call; the null levels are then not run (size is NaN) and the counts of calls over
    (b0, B) chunks add.  keep_replicates: return the [H, 1 + G, B, T, D] statistics."""
    names, cat, tg, tnames = _table(catalogue, targets, modality)
    C, V = cat.shape
    fr = _fractions(fractions)
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie in (0, 1), got %r" % alpha)
    B = int(B)
    if B < 1 and crit is None:
        raise ValueError("B = 0 replicates leave no critical value: give B >= 1 or crit")
    if B > 0 and seed is None:
        raise ValueError("B > 0 replicates need a seed")
    B, b0, seed, stream = _seeds(B, b0, 0 if seed is None else seed, stream)
    D, doc_ptr, term, count, al = _corpus(X, modality, allowed, names, C, V)
    nl = _levels(n_mutations, D)
    T, G = tg.size, fr.size
    H = 1 if nl is None else nl.shape[0]
    if H * (1 + G) * T * D >= 2 ** 31:
        raise ValueError("H (1 + G) T D = %d level pairs (limit 2^31 - 1)" % (H * (1 + G) * T * D))
    if crit is not None:
        crit = np.asarray(crit, dtype=np.float64)
        if crit.shape != (H, T, D) or np.isnan(crit).any():
            raise ValueError("crit must be [H, T, D] = [%d, %d, %d] without NaN, got shape %r" % (H, T, D, crit.shape))
        crit = np.ascontiguousarray(crit.reshape(H, T * D))
    ctx = ctx or (catalogue.ctx if isinstance(catalogue, (LDA, MMCTM)) else _lib.default_context())      # every argument is checked before a device is asked for
    r = _raw(ctx, D, V, doc_ptr, term, count, cat, tg, fr, nl, alpha, al, B, b0, seed, stream, crit, maxiter, tol, keep=bool(keep_replicates))
    status = r["status"].reshape(T, D)
    cr = r["count_reject"].reshape(H, 1 + G, T, D)
    dead = np.broadcast_to(status == 3, (H, 1 + G, T, D))
    share = np.where(dead, np.nan, cr / float(B)) if B else np.full((H, 1 + G, T, D), np.nan)
    size = np.full((H, T, D), np.nan) if crit is not None else share[:, 0]
    if nl is None:
        nl = np.bincount(np.repeat(np.arange(D), np.diff(doc_ptr)), weights=np.maximum(count, 0), minlength=D).astype(np.int64)[None, :]
    return PowerResult(share[:, 1:].copy(), size.copy(), r["crit"].reshape(H, T, D), cr[:, 1:].copy(), r["count_zero"].reshape(H, 1 + G, T, D), r["stat"].reshape(T, D),
                       r["score"].reshape(T, D), r["w_null"].reshape(T, D, C).transpose(0, 2, 1).copy(), status, r["iters"].reshape(T, D), fr, nl, alpha, B,
                       r["rep_stat"].reshape(H, 1 + G, B, T, D) if keep_replicates else None, tnames)
