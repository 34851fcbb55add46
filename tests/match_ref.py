"""numpy / pure-Python restatement of the signature-matching definitions of include/mmmusig.h (mmm_signature_cosine, mmm_signature_match,
mmm_signature_consensus).  Given S, the device's assignment must equal `lsap` exactly; the cosine and the row sums are compared within
the rounding bounds the tests derive (their orders of summation may differ from the device's)."""
import itertools
import math

import numpy as np


def cosine_exact(sig, cat):
    """S[k][c] with each of the three sums taken exactly (math.fsum): one rounding per sum"""
    sig = np.asarray(sig, dtype=np.float64); cat = np.asarray(cat, dtype=np.float64)
    K, C = sig.shape[0], cat.shape[0]
    S = np.zeros((K, C))
    ss = [math.fsum(float(x) * float(x) for x in row) for row in sig]         # (a product of two doubles is rounded once; fsum adds those exactly)
    cc = [math.fsum(float(x) * float(x) for x in row) for row in cat]
    for k in range(K):
        for c in range(C):
            if ss[k] == 0.0 or cc[c] == 0.0:
                continue
            dot = math.fsum(float(a) * float(b) for a, b in zip(sig[k], cat[c]))
            S[k, c] = dot / (math.sqrt(ss[k]) * math.sqrt(cc[c]))
    return S


def cosine(sig, cat):
    """the same with numpy's sums (for data, not for bounds): [..., K, V] x [C, V] -> [..., K, C]"""
    sig = np.asarray(sig, dtype=np.float64); cat = np.asarray(cat, dtype=np.float64)
    ns = np.sqrt((sig * sig).sum(axis=-1)); nc = np.sqrt((cat * cat).sum(axis=-1))
    den = ns[..., :, None] * nc[None, :]
    dot = sig @ cat.T
    return np.where(den > 0, dot / np.where(den > 0, den, 1.0), 0.0)


def lsap(S):
    """The injective k -> c that maximises sum_k S[k][a(k)]: shortest augmenting paths (Crouse 2016, Algorithm 1) on W = -S with the
    evaluation order of the header.  The vector expressions are elementwise: per column exactly ((minval + W[i][c]) - u[i]) - v[c]."""
    S = np.asarray(S, dtype=np.float64)
    K, C = S.shape
    assert 1 <= K <= C
    W = -S
    u = np.zeros(K); v = np.zeros(C)
    col4row = np.full(K, -1, dtype=np.int64); row4col = np.full(C, -1, dtype=np.int64); path = np.full(C, -1, dtype=np.int64)
    for cur in range(K):
        spc = np.full(C, np.inf)
        scanned = np.zeros(C, dtype=bool)
        rows = []
        minval = np.float64(0.0)
        i, sink = cur, -1
        while sink < 0:
            rows.append(i)
            red = ((minval + W[i]) - u[i]) - v
            better = ~scanned & (red < spc)                      # strictly smaller only
            spc[better] = red[better]; path[better] = i
            cand = np.where(scanned, np.inf, spc)
            j = int(np.argmin(cand))                             # the first minimum: ties to the lowest column
            minval = cand[j]
            scanned[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
        u[cur] += minval
        for i in rows[1:]:
            u[i] += minval - spc[col4row[i]]
        v[scanned] -= minval - spc[scanned]
        j = sink
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, int(col4row[i])
            if i == cur:
                break
    return col4row.astype(np.int32)


def brute_force_value(S):
    """the largest sum_k S[k][a(k)] over all injections (small K, C only)"""
    S = np.asarray(S, dtype=np.float64)
    K, C = S.shape
    return max(sum(S[k, p[k]] for k in range(K)) for p in itertools.permutations(range(C), K))


def match(sig, cat):
    """(assign [R, K], matched [R, K], S [R, K, C]) of sig [R, K, V] against cat [C, V]"""
    S = cosine(sig, cat)
    assign = np.stack([lsap(S[r]) for r in range(S.shape[0])])
    matched = np.take_along_axis(S, assign[..., None].astype(np.int64), axis=2)[..., 0]
    return assign, matched, S


def align_normalise(sig, assign):
    """P[r][assign[r][k]][v] = sig[r][k][v] / sum_v sig[r][k][v], the sum in index order; a zero row stays zero"""
    sig = np.asarray(sig, dtype=np.float64)
    R, K, V = sig.shape
    P = np.zeros((R, K, V))
    for r in range(R):
        for k in range(K):
            s = np.cumsum(sig[r, k])[-1]                         # (cumsum adds one after the other)
            P[r, assign[r, k]] = sig[r, k] / s if s != 0.0 else 0.0
    return P


def stability(assign, matched, ref):
    """per reference signature: the mean over r != ref, added in replica order, of the matched cosine of the signature assigned to it"""
    R, K = assign.shape
    acc = np.zeros(K)
    for r in range(R):
        if r == ref:
            continue
        for k in range(K):
            acc[assign[r, k]] += matched[r, k]
    return acc / (R - 1) if R > 1 else np.ones(K)
