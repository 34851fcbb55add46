"""Decomposition of signatures into sparse non-negative mixtures of catalogue signatures -- the step between extraction and assignment.

`match_signatures` names a de-novo signature by ONE catalogue row.  A signature that is a blend of two or three catalogue signatures (the
rule for flat or co-occurring processes: SBS2 + SBS13, SBS1 + SBS5) has no good one-to-one match.  Here every signature gets, for every
size s up to `max_size`, the subset of exactly s catalogue rows whose non-negative combination reconstructs it best -- found by EXHAUSTIVE
search on the GPU (`mmm_signature_decompose`), not by a greedy add / remove path: the answer is the optimum, so it is a definition.  The
smallest size within `min_gain` of the best cosine is reported, with the mixture in probability terms ("60 % of row 2, 40 % of row 13") and
a mask for `refit_exposures(..., allowed=...)` / `signature_presence`.  The definition, down to the order of every operation and the tie
rule, is in include/mmmusig.h: the same arguments give the same bits on every run.
"""
from collections import namedtuple
from math import comb

import numpy as np

from . import _lib
from ._lib import check, lib
from .ctm import MMCTM
from .match import _reject_factorised, _signatures_of
from .models import LDA
from .refit import _catalogue

MAX_SIZE = 6              # members of a subset
MAX_CATALOGUE = 256       # catalogue rows
MAX_SUBSETS = 2 ** 32     # binom(C, min(max_size, C)) must stay below this

SearchResult = namedtuple("SearchResult", "subset weight gain cosine")
SearchResult.__doc__ = """Per signature i and size s = 1 .. S: subset [n, S, S] the best admissible subset of exactly s rows (ascending, -1 padded),
weight [n, S, S] its weights (0 padded), gain [n, S] and cosine [n, S] = sqrt(min(gain / ss, 1)); all -1 / 0 where no subset of the size is
admissible."""

_Decomposition = namedtuple("Decomposition", "size members weights shares cosine path_members path_weights path_cosine names")


class Decomposition(_Decomposition):
    """size: [..., K] members of the chosen mixture of every signature (0: nothing admissible); members: [..., K, S] its catalogue rows
    ascending, -1 padded; weights: [..., K, S] their weights (signature ~ sum_j weights_j cat[members_j]); shares: [..., K, S] = w_j a_j /
    sum w a with a_c = sum_v cat[c][v], the mixture in probability terms; cosine: [..., K] of the chosen reconstruction; path_members,
    path_weights: [..., K, S, S] and path_cosine: [..., K, S] the best subset of EVERY size (`SearchResult`); names: the catalogue's names or
    None."""
    __slots__ = ()

    def allowed(self, C):
        """[C] bool mask of every catalogue row some signature's chosen mixture uses: the `allowed=` of refit_exposures / signature_presence"""
        C = int(C)
        m = np.asarray(self.members).ravel()
        m = m[m >= 0]
        if m.size and int(m.max()) >= C:
            raise ValueError("the decomposition uses catalogue row %d, C = %d" % (int(m.max()), C))
        mask = np.zeros(C, dtype=bool)
        mask[m] = True
        return mask

    def describe(self):
        """one string per signature, e.g. "60.0% SBS2 + 40.0% SBS13 (cosine 0.9871)"; rows are named "row c" where the catalogue has no names"""
        mem = np.asarray(self.members); sh = np.asarray(self.shares); cs = np.asarray(self.cosine)
        S = mem.shape[-1]
        out = []
        for m, s, c in zip(mem.reshape(-1, S), sh.reshape(-1, S), cs.ravel()):
            parts = ["%.1f%% %s" % (100.0 * s[j], self.names[m[j]] if self.names is not None else "row %d" % m[j]) for j in range(S) if m[j] >= 0]
            out.append("%s (cosine %.4f)" % (" + ".join(parts), c) if parts else "no admissible mixture")
        return out


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _check_limits(C, S):
    if int(S) != S or S < 1:
        raise ValueError("max_size must be an integer >= 1, got %r" % (S,))
    if S > MAX_SIZE:
        raise ValueError("max_size = %d (limit %d)" % (S, MAX_SIZE))
    if C < 1:
        raise ValueError("the catalogue must have at least one row")
    if C > MAX_CATALOGUE:
        raise ValueError("C = %d catalogue rows (limit %d)" % (C, MAX_CATALOGUE))
    most = comb(C, min(S, C))
    if most >= MAX_SUBSETS:
        raise ValueError("C = %d, max_size = %d: %d subsets of the largest size (limit 2^32 - 1)" % (C, S, most))


class _route:
    """in_lds=False (tests): G and b are read through L2 even where they fit LDS; the tuning is put back afterwards"""

    def __init__(self, ctx, in_lds):
        self.ctx, self.in_lds, self.before = ctx, in_lds, None

    def __enter__(self):
        if not self.in_lds:
            self.before = self.ctx.get_tuning()
            t = _lib.TuningOpts.from_buffer_copy(self.before)
            t.disable |= _lib.OFF["decompose_lds"]
            check(lib().mmm_ctx_set_tuning(self.ctx.h, _lib.C.byref(t)), self.ctx.h, "mmm_ctx_set_tuning")

    def __exit__(self, *exc):
        if self.before is not None:
            check(lib().mmm_ctx_set_tuning(self.ctx.h, _lib.C.byref(self.before)), self.ctx.h, "mmm_ctx_set_tuning")
        return False


def _outputs(n, S):
    return np.full((n, S, S), -1, dtype=np.int32), np.zeros((n, S, S)), np.zeros((n, S)), np.zeros((n, S))


def decompose_search(G, b, ss, max_size, ctx=None, in_lds=True):
    """Stage 2 alone on caller moments (`mmm_decompose_search`): G [C, C] = cat cat^T, b [n, C] = sig cat^T, ss [n] = |sig|^2 -> SearchResult.
    1 <= max_size <= 6, C <= 256, binom(C, min(max_size, C)) < 2^32."""
    G = np.ascontiguousarray(G, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64); ss = np.ascontiguousarray(ss, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError("G must be [C, C], got shape %r" % (G.shape,))
    C = G.shape[0]
    if b.ndim != 2 or b.shape[1] != C:
        raise ValueError("b must be [n, C] with C = %d, got shape %r" % (C, b.shape))
    n = b.shape[0]
    if ss.shape != (n,):
        raise ValueError("ss must be [n] = [%d], got shape %r" % (n, ss.shape))
    _check_limits(C, max_size)
    S = int(max_size)
    ctx = ctx or _lib.default_context()
    subset, weight, gain, cosine = _outputs(n, S)
    with _route(ctx, in_lds):
        rc = lib().mmm_decompose_search(ctx.h, n, C, S, _ptr(G), _ptr(b), _ptr(ss), _ptr(subset), _ptr(weight), _ptr(gain), _ptr(cosine))
    check(rc, ctx.h, "mmm_decompose_search")
    return SearchResult(subset, weight, gain, cosine)


def _raw(ctx, sig, cat, S, moments=False, in_lds=True):
    """mmm_signature_decompose on sig [n, V], cat [C, V] -> SearchResult (and with moments=True the device's (G, b, ss))"""
    n, V = sig.shape
    C = cat.shape[0]
    subset, weight, gain, cosine = _outputs(n, S)
    G = np.zeros((C, C)) if moments else None; b = np.zeros((n, C)) if moments else None; ss = np.zeros(n) if moments else None
    with _route(ctx, in_lds):
        rc = lib().mmm_signature_decompose(ctx.h, n, C, V, _ptr(sig), _ptr(cat), S, _ptr(subset), _ptr(weight), _ptr(gain), _ptr(cosine), _ptr(G), _ptr(b), _ptr(ss))
    check(rc, ctx.h, "mmm_signature_decompose")
    r = SearchResult(subset, weight, gain, cosine)
    return (r, (G, b, ss)) if moments else r


def choose_size(path_cosine, min_gain):
    """The selection rule on path_cosine [..., S] -> the chosen sizes [...] (1-based).  With cbest[s] = max_{t <= s} cosine[t]: the smallest s
    with cbest[S] - cbest[s] < min_gain -- the smallest size within a margin of the best, the idea of `pick_k`."""
    pc = np.asarray(path_cosine, dtype=np.float64)
    if not (np.isfinite(min_gain) and min_gain > 0):
        raise ValueError("min_gain must be finite and > 0, got %r" % (min_gain,))
    cbest = np.maximum.accumulate(pc, axis=-1)
    within = cbest[..., -1:] - cbest < min_gain
    return np.argmax(within, axis=-1) + 1                      # (the last size is always within the margin)


def compose(path, rowsum, min_gain, names=None):
    """Decomposition of a SearchResult `path` (leading shape [n]) under the catalogue's row sums a_c = sum_v cat[c][v]: the size by
    `choose_size`; members and weights from the smallest t attaining cbest[size]; shares_j = w_j a_j / sum w a."""
    sub = np.asarray(path.subset); wt = np.asarray(path.weight); pc = np.asarray(path.cosine, dtype=np.float64)
    rowsum = np.asarray(rowsum, dtype=np.float64)
    n, S = pc.shape
    size = choose_size(pc, min_gain)
    cbest = np.maximum.accumulate(pc, axis=-1)
    members = np.full((n, S), -1, dtype=np.int32); weights = np.zeros((n, S)); shares = np.zeros((n, S)); cosine = np.zeros(n)
    for i in range(n):
        s = int(size[i])
        t = int(np.argmax(pc[i, :s] == cbest[i, s - 1]))       # the smallest t (0-based) attaining cbest[s]
        members[i] = sub[i, t]; weights[i] = wt[i, t]; cosine[i] = pc[i, t]
        used = members[i] >= 0
        mass = np.where(used, weights[i] * rowsum[np.where(used, members[i], 0)], 0.0)
        if mass.sum() > 0:
            shares[i] = mass / mass.sum()
    nmem = (members >= 0).sum(axis=1).astype(np.int32)
    return Decomposition(nmem, members, weights, shares, cosine, sub, wt, pc, list(names) if names is not None else None)


def decompose_signatures(sig, catalogue, max_size=3, min_gain=0.01, modality=None, names=None, ctx=None):
    """Every signature as a sparse non-negative mixture of catalogue signatures -> Decomposition.

    sig: a [K, V] or [R, K, V] array or a fitted LDA / MMCTM (the columns of β; ϕ of `modality`), as `match_signatures` takes it; ILDA /
    IMMCTM: TypeError (factorised tables).  catalogue: as `refit_exposures` takes it -- a [C, V] array (rows need not be normalised, none all
    zero), the (names, terms, S) of `read_signatures_tsv`, or a fitted model; C <= 256.  max_size: the largest number of catalogue rows in a
    mixture, 1 .. 6, with binom(C, max_size) < 2^32 (C = 86: every size; C = 256: up to 4).
    For every size s <= max_size the best subset of exactly s rows is found by exhaustive search on the GPU (path_members, path_weights,
    path_cosine); the chosen size is the smallest whose best cosine so far is within `min_gain` of the best over all sizes.  names: the
    catalogue's row names for `describe()` (default: those the catalogue came with).  `result.allowed(C)` is the mask of all chosen rows."""
    _reject_factorised(sig, "decompose_signatures")
    own_ctx = sig.ctx if isinstance(sig, (LDA, MMCTM)) else None
    s = _signatures_of(sig, modality, "sig")
    cat_names, cat = _catalogue(catalogue, modality)
    C, V = cat.shape
    if s.shape[-1] != V:
        raise ValueError("the signatures have %d terms and the catalogue %d" % (s.shape[-1], V))
    if V < 1 or s.shape[-2] < 1:
        raise ValueError("K and V must be >= 1")
    _check_limits(C, max_size)
    if not (cat > 0).any(axis=1).all():
        raise ValueError("catalogue row %d is all zero" % int(np.argmin((cat > 0).any(axis=1))))
    if not (np.isfinite(min_gain) and min_gain > 0):
        raise ValueError("min_gain must be finite and > 0, got %r" % (min_gain,))
    if names is None:
        names = cat_names
    elif len(names) != C:
        raise ValueError("names holds %d entries, the catalogue has %d rows" % (len(names), C))
    ctx = ctx or own_ctx or _lib.default_context()
    lead = s.shape[:-1]
    path = _raw(ctx, np.ascontiguousarray(s.reshape(-1, V)), cat, int(max_size))
    d = compose(path, cat.sum(axis=1), min_gain, names)
    S = int(max_size)
    return Decomposition(d.size.reshape(lead), d.members.reshape(lead + (S,)), d.weights.reshape(lead + (S,)), d.shares.reshape(lead + (S,)),
                         d.cosine.reshape(lead), d.path_members.reshape(lead + (S, S)), d.path_weights.reshape(lead + (S, S)),
                         d.path_cosine.reshape(lead + (S,)), d.names)
