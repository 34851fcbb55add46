"""Matching signatures to a catalogue and across the restarts of a batch -- the step the reference's README leaves to the user ("compute
the cosine distance between the inferred and COSMIC signatures, then use a linear sum assignment solver to find the optimal set of unique
matches"), and the same operation applied to a restart sweep: topic labels are arbitrary per restart, so every restart's topics are
matched to one reference restart's before anything is said across restarts.

Cosine, assignment (shortest augmenting paths, Crouse 2016) and the consensus (mean / sd / quantiles of the aligned topic probabilities,
stability per signature) run on the GPU (`mmm_signature_*`, `mmm_*_match_replicas`, `mmm_*_replica_consensus`); the handle forms read the
restarts' tables where they lie.  The definitions, down to the order of every sum and every tie rule, are in include/mmmusig.h: the same
arguments give the same bits on every run.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from .ctm import IMMCTM, MMCTM
from .models import ILDA, LDA

MAX_CATALOGUE = 1024      # catalogue rows an assignment takes (one wave's LDS holds its column arrays)
MAX_REPLICAS = 4096       # restarts a consensus takes (mmm_replicate_summary sorts a column in LDS)

SignatureMatch = namedtuple("SignatureMatch", "assign cosine similarity")
SignatureMatch.__doc__ = """assign: [..., K] 0-based catalogue row of every signature (distinct within a set); cosine: [..., K] the cosine to
it; similarity: [..., K, C] all cosines (None from `match_restarts`, which leaves them on the device)."""

ConsensusResult = namedtuple("ConsensusResult", "ref assign cosine stability mean sd quantiles q")
ConsensusResult.__doc__ = """ref: the reference restart; assign, cosine: [R, K] every restart's topics in ref's labelling and the cosines;
stability: [K] mean cosine of the other restarts' matched topics; mean, sd: [K, V] and quantiles: [len(q), K, V] of the aligned topic
probabilities over the restarts."""


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _values(x, name, ndims):
    """a caller array as C-contiguous float64 with one of the given numbers of dimensions, every entry finite and >= 0"""
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.ndim not in ndims:
        raise ValueError("%s must have %s dimensions, got shape %r" % (name, " or ".join(str(n) for n in ndims), a.shape))
    if a.size and not (np.isfinite(a).all() and (a >= 0).all()):
        raise ValueError("%s holds a negative or non-finite entry" % name)
    return a


def _reject_factorised(model, what):
    if isinstance(model, ILDA):
        raise TypeError("%s: the topics of an ILDA are factorised over the features (ILDA.jl:6-9); no V x K signatures to match" % what)
    if isinstance(model, IMMCTM):
        raise TypeError("%s: the topics of an IMMCTM are factorised over the features (IMMCTM.jl:13); no K x V signatures to match" % what)


def _signatures_of(x, modality, name):
    """[K, V] / [R, K, V] array from an array or a fitted model (LDA: the columns of β; MMCTM: ϕ of `modality`; the selected restart)"""
    _reject_factorised(x, "match_signatures")
    if isinstance(x, LDA):
        return np.ascontiguousarray(x.β.T)
    if isinstance(x, MMCTM):
        m = _modality(x, modality)
        return np.stack([np.asarray(x.ϕ[m][k], dtype=np.float64) for k in range(x.K[m])])
    return _values(x, name, (2, 3))


def _modality(model, modality):
    if modality is None:
        raise ValueError("an MMCTM has one set of signatures per modality: pass modality=m")
    m = int(modality)
    if not 0 <= m < model.M:
        raise ValueError("modality %d of %d" % (m, model.M))
    return m


def cosine_similarity(A, B, ctx=None):
    """Cosine of every row of A ([..., K, V]) to every row of B ([C, V]) -> [..., K, C], on the GPU (`mmm_signature_cosine`).  Entries must
    be finite and >= 0; rows need not be normalised; a zero row gives 0 against everything."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    if A.ndim < 2:
        raise ValueError("A must be [..., K, V], got shape %r" % (A.shape,))
    A = _values(A, "A", (A.ndim,))
    B = _values(B, "B", (2,))
    K, V = A.shape[-2:]
    C = B.shape[0]
    if B.shape[1] != V:
        raise ValueError("A has %d terms and B %d" % (V, B.shape[1]))
    if K < 1 or C < 1 or V < 1:
        raise ValueError("K, C and V must be >= 1")
    R = int(np.prod(A.shape[:-2], dtype=np.int64))
    ctx = ctx or _lib.default_context()
    S = np.zeros(A.shape[:-1] + (C,))
    check(lib().mmm_signature_cosine(ctx.h, R, K, C, V, _ptr(A), _ptr(B), _ptr(S)), ctx.h, "mmm_signature_cosine")
    return S


def _check_match_shape(K, C, V, Vc):
    if Vc != V:
        raise ValueError("the signatures have %d terms and the catalogue %d" % (V, Vc))
    if K < 1 or V < 1:
        raise ValueError("K and V must be >= 1")
    if K > C:
        raise ValueError("K = %d signatures cannot be matched one to one to C = %d catalogue rows" % (K, C))


def match_signatures(sig, catalogue, modality=None, ctx=None):
    """The one-to-one match of signatures to catalogue rows that maximises the summed cosine.  `sig`: a [K, V] or [R, K, V] array or a fitted
    model (LDA: the columns of β; MMCTM: ϕ of `modality`; a batch model: its selected restart); `catalogue`: [C, V] (or a model, likewise),
    K <= C <= 1024.  Returns SignatureMatch(assign, cosine, similarity) (`mmm_signature_match`)."""
    own_ctx = sig.ctx if isinstance(sig, (LDA, MMCTM)) else None
    s = _signatures_of(sig, modality, "sig")
    c = _signatures_of(catalogue, modality, "catalogue")
    if c.ndim != 2:
        raise ValueError("catalogue must be [C, V], got shape %r" % (c.shape,))
    K, V = s.shape[-2:]
    C = c.shape[0]
    _check_match_shape(K, C, V, c.shape[1])
    R = 1 if s.ndim == 2 else s.shape[0]
    ctx = ctx or own_ctx or _lib.default_context()
    assign = np.zeros((R, K), dtype=np.int32); matched = np.zeros((R, K)); S = np.zeros((R, K, C))
    check(lib().mmm_signature_match(ctx.h, R, K, C, V, _ptr(s), _ptr(c), _ptr(assign), _ptr(matched), _ptr(S)), ctx.h, "mmm_signature_match")
    if s.ndim == 2:
        return SignatureMatch(assign[0], matched[0], S[0])
    return SignatureMatch(assign, matched, S)


def _handle_call(model, modality, what):
    """(C function, leading arguments, K, V) of the handle form for `model`"""
    _reject_factorised(model, what)
    if isinstance(model, LDA):
        return "lda", (model._h,), model.K, model.V
    if isinstance(model, MMCTM):
        m = _modality(model, modality)
        return "ctm", (model._h, m), model.K[m], model.V[m]
    raise TypeError("%s takes an LDA or MMCTM (a restart batch or an ordinary model)" % what)


def match_restarts(model, modality=None, catalogue=None):
    """Every restart's topics matched to `catalogue` ([C, V]) or, without one, to the SELECTED restart's own topics -> SignatureMatch with
    assign, cosine of shape [R, K] (similarity None).  The restarts' tables (λ of an LDA, γ of `modality` of an MMCTM) are read where they
    lie on the device (`mmm_lda_match_replicas` / `mmm_ctm_match_replicas`): only the catalogue goes up and the R x K results come down."""
    kind, lead, K, V = _handle_call(model, modality, "match_restarts")
    cat, C = None, K
    if catalogue is not None:
        cat = _values(catalogue, "catalogue", (2,))
        C = cat.shape[0]
        _check_match_shape(K, C, V, cat.shape[1])
    R = model.R
    assign = np.zeros((R, K), dtype=np.int32); matched = np.zeros((R, K))
    check(getattr(lib(), "mmm_%s_match_replicas" % kind)(*lead, C, _ptr(cat), _ptr(assign), _ptr(matched)), model.ctx.h, "match_restarts")
    return SignatureMatch(assign, matched, None)


def _best_restart(model, modality):
    if getattr(model, "restart_ll", None) is None:
        raise ValueError("restart_consensus(ref=None) takes the restart with the best final log-likelihood: run fit_restarts(model) first, or pass ref")
    if isinstance(model, LDA):
        from .restarts import _best
        return _best(model.restart_ll)
    from .ctm import pick_optimal_modality_models
    return pick_optimal_modality_models(model)[modality]


def restart_consensus(model, modality=None, ref=None, q=(0.025, 0.5, 0.975)):
    """What the restart sweep says about the topics themselves: every restart's topics are matched to restart `ref`'s (default: the restart
    with the best final log-likelihood -- `fit_restarts` must have run), normalised to probabilities and summarised per (signature, term)
    over the R restarts -> ConsensusResult(ref, assign, cosine, stability, mean, sd, quantiles, q).  stability[k] is the mean cosine of the
    other restarts' topics matched to ref's topic k: near 1 when every local optimum holds that signature.  On the device throughout
    (`mmm_lda_replica_consensus` / `mmm_ctm_replica_consensus`); R <= 4096."""
    kind, lead, K, V = _handle_call(model, modality, "restart_consensus")
    R = model.R
    if ref is None:
        ref = _best_restart(model, lead[1] if kind == "ctm" else None)
    ref = int(ref)
    if not 0 <= ref < R:
        raise ValueError("ref = %d is not one of the %d restarts" % (ref, R))
    qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
    if qa.size and not ((qa >= 0).all() and (qa <= 1).all()):
        raise ValueError("q must lie in [0, 1]")
    assign = np.zeros((R, K), dtype=np.int32); matched = np.zeros((R, K)); stab = np.zeros(K)
    mean = np.zeros((K, V)); sd = np.zeros((K, V)); quant = np.zeros((qa.size, K, V))
    check(getattr(lib(), "mmm_%s_replica_consensus" % kind)(*lead, ref, int(qa.size), _ptr(qa), _ptr(assign), _ptr(matched), _ptr(stab), _ptr(mean), _ptr(sd),
                                                          _ptr(quant)), model.ctx.h, "restart_consensus")
    return ConsensusResult(ref, assign, matched, stab, mean, sd, quant, tuple(float(v) for v in qa))


def signature_consensus(sig, ref, q=(0.025, 0.5, 0.975), ctx=None):
    """`restart_consensus` on a caller array sig [R, K, V] (`mmm_signature_consensus`)."""
    s = _values(sig, "sig", (3,))
    R, K, V = s.shape
    ref = int(ref)
    if not 0 <= ref < R:
        raise ValueError("ref = %d is not one of the %d replicas" % (ref, R))
    if K < 1 or V < 1:
        raise ValueError("K and V must be >= 1")
    qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
    if qa.size and not ((qa >= 0).all() and (qa <= 1).all()):
        raise ValueError("q must lie in [0, 1]")
    ctx = ctx or _lib.default_context()
    assign = np.zeros((R, K), dtype=np.int32); matched = np.zeros((R, K)); stab = np.zeros(K)
    mean = np.zeros((K, V)); sd = np.zeros((K, V)); quant = np.zeros((qa.size, K, V))
    check(lib().mmm_signature_consensus(ctx.h, R, K, V, _ptr(s), ref, int(qa.size), _ptr(qa), _ptr(assign), _ptr(matched), _ptr(stab), _ptr(mean), _ptr(sd),
                                        _ptr(quant)), ctx.h, "mmm_signature_consensus")
    return ConsensusResult(ref, assign, matched, stab, mean, sd, quant, tuple(float(v) for v in qa))
