"""numpy restatement of the bootstrap definitions of include/mmmusig.h (mmm_resample_counts, mmm_replicate_summary): Philox4x32-10, the
integer inverse-CDF draw, the replicate-major stacking and the summary formulas.  The device must equal `resample` bit for bit."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint64 arrays holding 32-bit values in and out (Salmon et al., SC'11)"""
    c = [np.asarray(x, np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def resample_doc(count, d, b, seed, stream=0):
    """the resampled counts of one (document, replicate) pair; count: the document's counts in CSR order"""
    count = np.asarray(count, dtype=np.int64)
    N = int(count.sum())
    if N == 0:
        return np.zeros(count.size, dtype=np.int64)
    nblk = (N + 3) // 4
    z = np.zeros(nblk, np.uint64)
    w = philox4x32_10(np.arange(nblk, dtype=np.uint64), z + np.uint64(d), z + np.uint64(b), z + np.uint64(stream), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    u = np.stack(w, axis=1).ravel()[:N]
    r = (u * np.uint64(N)) >> np.uint64(32)
    e = np.searchsorted(np.cumsum(count).astype(np.uint64), r, side="right")
    return np.bincount(e, minlength=count.size).astype(np.int64)


def resample(X, B, seed, b0=0, stream=0):
    """X: list of (W_d x 2) matrices [1-based term, count].  Returns a list of B corpora of the same shape (zero rows kept)."""
    out = []
    for b in range(B):
        out.append([np.stack([np.asarray(x).reshape(-1, 2)[:, 0], resample_doc(np.asarray(x).reshape(-1, 2)[:, 1], d, b0 + b, seed, stream)], axis=1)
                    .astype(np.int64) for d, x in enumerate(X)])
    return out


def resample_mm(X, B, seed, b0=0):
    """MMCTM nesting X[d][m]: modality m is drawn with stream = m"""
    M = len(X[0])
    per_mod = [resample([X[d][m] for d in range(len(X))], B, seed, b0=b0, stream=m) for m in range(M)]
    return [[[per_mod[m][b][d] for m in range(M)] for d in range(len(X))] for b in range(B)]


def counts_matrix(reps):
    """[B, nnz] counts of a list of LDA-nested replicate corpora (documents concatenated)"""
    return np.stack([np.concatenate([x[:, 1] for x in rep]) if rep else np.zeros(0, np.int64) for rep in reps])


def stack(reps):
    """replicate-major stacked corpus: document b D + d"""
    return [doc for rep in reps for doc in rep]


def summary(x, q):
    """mean, sd (B - 1; 0 for B = 1) and quantiles over axis 0 by the formulas of the header"""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    mean = np.zeros(x.shape[1:])
    for b in range(B):
        mean = mean + x[b]
    mean = mean / B
    ss = np.zeros(x.shape[1:])
    for b in range(B):
        ss = ss + (x[b] - mean) ** 2
    sd = np.sqrt(ss / (B - 1)) if B > 1 else np.zeros(x.shape[1:])
    s = np.sort(x, axis=0)
    quant = []
    for qq in np.atleast_1d(q):
        h = (B - 1) * float(qq)
        lo = int(np.floor(h))
        hi = min(lo + 1, B - 1)
        quant.append(s[lo] + (h - lo) * (s[hi] - s[lo]))
    return mean, sd, np.stack(quant) if len(quant) else np.zeros((0,) + x.shape[1:])
