"""numpy restatement of the held-out selection definitions of include/mmmusig.h (mmm_split_counts, mmm_mixture_score): the fold of every
mutation from its own Philox4x32-10 word, and the per-document score in np.longdouble.  The device must equal `split` integer for integer
and the score to the rounding of its double sums."""
import numpy as np

from bootstrap_ref import philox4x32_10

SPLIT_BIT = 0x80000000


def fold_words(N, d, rep, seed, stream=0):
    """the N random words of document d: word i % 4 of the block with counter (i / 4, d, rep, 0x80000000 | stream)"""
    nblk = (N + 3) // 4
    z = np.zeros(nblk, np.uint64)
    w = philox4x32_10(np.arange(nblk, dtype=np.uint64), z + np.uint64(d), z + np.uint64(rep), z + np.uint64(SPLIT_BIT | int(stream)),
                      int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return np.stack(w, axis=1).ravel()[:N]


def split_doc(count, d, F, rep, seed, stream=0):
    """[F, W] counts of one document's folds; count: the document's counts in CSR order"""
    count = np.asarray(count, dtype=np.int64)
    out = np.zeros((F, count.size), dtype=np.int64)
    N = int(count.sum())
    if N == 0:
        return out
    fold = ((fold_words(N, d, rep, seed, stream) * np.uint64(F)) >> np.uint64(32)).astype(np.int64)
    entry = np.searchsorted(np.cumsum(count), np.arange(N, dtype=np.int64), side="right")       # cum[e-1] <= i < cum[e]
    np.add.at(out, (fold, entry), 1)
    return out


def split(X, F, seed, rep=0, stream=0):
    """X: list of (W_d x 2) matrices [1-based term, count] -> list of F corpora of the same shape (zero rows kept)"""
    docs = [np.asarray(x, dtype=np.int64).reshape(-1, 2) for x in X]
    per_doc = [split_doc(x[:, 1], d, F, rep, seed, stream) for d, x in enumerate(docs)]
    return [[np.stack([x[:, 0], p[f]], axis=1).astype(np.int64) for x, p in zip(docs, per_doc)] for f in range(F)]


def split_mm(X, F, seed, rep=0):
    """MMCTM nesting X[d][m]: modality m is split with stream = m"""
    M = len(X[0])
    per_mod = [split([X[d][m] for d in range(len(X))], F, seed, rep=rep, stream=m) for m in range(M)]
    return [[[per_mod[m][f][d] for m in range(M)] for d in range(len(X))] for f in range(F)]


def counts_matrix(parts):
    """[F, nnz] counts of a list of LDA-nested corpora (documents concatenated)"""
    return np.stack([np.concatenate([np.asarray(x).reshape(-1, 2)[:, 1] for x in part]) for part in parts])


def score(X, theta, beta):
    """theta K x D, beta V x K -> (ll_doc, n_doc, cos_doc) in np.longdouble; duplicate terms of a document are separate entries"""
    th = np.asarray(theta, dtype=np.longdouble); be = np.asarray(beta, dtype=np.longdouble)
    D = len(X)
    ll = np.zeros(D, np.longdouble); n_doc = np.zeros(D, np.longdouble); cos = np.zeros(D, np.longdouble)
    for d, x in enumerate(X):
        x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
        p = be @ th[:, d]                                   # [V]
        n = x[:, 1].astype(np.longdouble)
        pe = p[x[:, 0] - 1]
        pos = n > 0
        ll[d] = (n[pos] * np.log(pe[pos])).sum() if pos.any() else 0
        n_doc[d] = n.sum()
        nn, pp = (n * n).sum(), (p * p).sum()
        cos[d] = (n * pe).sum() / (np.sqrt(nn) * np.sqrt(pp)) if nn > 0 and pp > 0 else 0
    return ll, n_doc, cos
