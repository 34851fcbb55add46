"""numpy restatement of the simulation / goodness-of-fit definitions of include/mmmusig.h (mmm_simulate_counts, mmm_fit_check): the
mixture and its integer thresholds, the Philox4x32-10 word of every draw, and the two statistics with the order of every sum.  The device
must equal all of it bit for bit: only +, -, x, /, sqrt, floor and comparisons occur, each rounded once (numpy never fuses a product into a
sum)."""
import numpy as np

from bootstrap_ref import philox4x32_10

SIM_BIT = 0x80000000          # high bit of the THIRD counter word: a simulation (the resampler and the split keep b, rep < 2^31)
TWO32 = 4294967296.0
_LANES = np.arange(64)
PLANTED_SEED, DRAW_SEED, PLANTED_B = 1, 2024, 199      # the planted corpus of the CPU and GPU tests: `planted` seed, draw seed, replicates


def mixture(props_d, phi):
    """p_v = sum_k props[k] phi[k, v], k ascending, product and sum rounded separately; props_d [K], phi [K, V]"""
    phi = np.asarray(phi, dtype=np.float64)
    p = np.zeros(phi.shape[1])
    for k in range(phi.shape[0]):
        p = p + np.float64(props_d[k]) * phi[k]
    return p


def thresholds(p):
    """-> (pi [V] float64, T [V] uint64 in [0, 2^32], S).  cum is the strictly sequential inclusive sum (np.cumsum accumulates in index
    order), pi_v = p_v / S, T_v = floor((cum_v / S) 2^32)."""
    p = np.asarray(p, dtype=np.float64)
    cum = np.cumsum(p)
    S = cum[-1]
    with np.errstate(all="ignore"):
        pi = p / S
        T = np.floor((cum / S) * TWO32)
    return pi, (T.astype(np.uint64) if np.isfinite(S) and S > 0 else np.zeros(p.size, np.uint64)), S


def words(N, d, b, seed, stream=0):
    """[len(b), N] random words of the replicates b (global indices) of document d: draw i is word i % 4 of the block with counter
    (i / 4, d, 0x80000000 | b, stream) under the key (seed low, seed high)"""
    b = np.atleast_1d(np.asarray(b, dtype=np.uint64))
    nblk = (int(N) + 3) // 4
    c0 = np.arange(nblk, dtype=np.uint64)[None, :]
    z = np.zeros((b.size, nblk), np.uint64)
    w = philox4x32_10(z + c0, z + np.uint64(d), z + (b[:, None] | np.uint64(SIM_BIT)), z + np.uint64(stream), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return np.stack(w, axis=-1).reshape(b.size, 4 * nblk)[:, :int(N)]


def land(T, u):
    """the term of every word of u: the first v with T_v > u"""
    return np.searchsorted(np.asarray(T, dtype=np.uint64), np.asarray(u, dtype=np.uint64), side="right")


def simulate_doc(T, N, d, b, seed, stream=0):
    """[len(b), V] draws per term of the replicates b of document d under the thresholds T"""
    b = np.atleast_1d(b)
    V = len(T)
    out = np.zeros((b.size, V), dtype=np.int64)
    if int(N) == 0:
        return out
    v = land(T, words(N, d, b, seed, stream))
    np.add.at(out, (np.repeat(np.arange(b.size), int(N)), v.ravel()), 1)
    return out


def simulate(props, phi, n_doc, B, b0=0, seed=0, stream=0):
    """props [D, K] (props[k + K d]), phi [K, V] -> int64 [B, D, V]"""
    props = np.asarray(props, dtype=np.float64); phi = np.asarray(phi, dtype=np.float64)
    D, V = props.shape[0], phi.shape[1]
    out = np.zeros((B, D, V), dtype=np.int64)
    for d in range(D):
        if int(n_doc[d]) == 0 or B == 0:
            continue
        _, T, _ = thresholds(mixture(props[d], phi))
        out[:, d, :] = simulate_doc(T, n_doc[d], d, b0 + np.arange(B), seed, stream)
    return out


def wave_sum(x):
    """sum over the last axis as the header orders it: 64 partial sums, partial l over l, l + 64, ... ascending (from 0.0), then the
    butterfly l ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1"""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[-1]
    pad = (-V) % 64
    if pad:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,))], axis=-1)
    x = x.reshape(x.shape[:-1] + (-1, 64))
    part = np.zeros(x.shape[:-2] + (64,))
    for s in range(x.shape[-2]):
        part = part + x[..., s, :]
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[..., _LANES ^ off]
    return part[..., 0]


def statistics(n, pi, N):
    """n [..., V] integer counts of total N, pi [V] -> (cosine [...], chi2 [...])"""
    n = np.asarray(n, dtype=np.float64); pi = np.asarray(pi, dtype=np.float64)
    if int(N) == 0:
        return np.zeros(n.shape[:-1]), np.zeros(n.shape[:-1])
    with np.errstate(all="ignore"):
        num, nn, pp = wave_sum(n * pi), wave_sum(n * n), wave_sum(pi * pi)
        cos = np.where((nn > 0) & (pp > 0), num / (np.sqrt(nn) * np.sqrt(pp)), 0.0)
        e = np.float64(N) * pi
        dd = n - e
        t = np.where(pi > 0, (dd * dd) / e, np.where(n > 0, np.inf, 0.0))
    return cos, wave_sum(t)


def dense(V, term, count):
    n = np.zeros(V, dtype=np.int64)
    np.add.at(n, np.asarray(term, dtype=np.int64), np.asarray(count, dtype=np.int64))
    return n


def fit_check(doc_ptr, term, count, props, phi, B, b0=0, seed=0, stream=0):
    """-> dict(cos_obs, chi_obs [D], cos_le, chi_ge [D] int32, cos_rep, chi_rep [B, D], n_doc [D])"""
    props = np.asarray(props, dtype=np.float64); phi = np.asarray(phi, dtype=np.float64)
    D, V = props.shape[0], phi.shape[1]
    r = dict(cos_obs=np.zeros(D), chi_obs=np.zeros(D), cos_le=np.zeros(D, np.int32), chi_ge=np.zeros(D, np.int32), cos_rep=np.zeros((B, D)),
             chi_rep=np.zeros((B, D)), n_doc=np.zeros(D, np.int64))
    for d in range(D):
        n = dense(V, term[doc_ptr[d]:doc_ptr[d + 1]], count[doc_ptr[d]:doc_ptr[d + 1]])
        N = int(n.sum())
        r["n_doc"][d] = N
        if N == 0:
            r["cos_le"][d] = r["chi_ge"][d] = B
            continue
        pi, T, _ = thresholds(mixture(props[d], phi))
        r["cos_obs"][d], r["chi_obs"][d] = statistics(n, pi, N)
        if B:
            c, x = statistics(simulate_doc(T, N, d, b0 + np.arange(B), seed, stream), pi, N)
            r["cos_rep"][:, d], r["chi_rep"][:, d] = c, x
            r["cos_le"][d] = int((c <= r["cos_obs"][d]).sum()); r["chi_ge"][d] = int((x >= r["chi_obs"][d]).sum())
    return r


def csr(docs):
    """docs: list of (terms, counts) -> (doc_ptr int64, term int32, count int32)"""
    dp = np.concatenate([[0], np.cumsum([len(t) for t, _ in docs])]).astype(np.int64)
    term = np.concatenate([np.asarray(t, np.int32) for t, _ in docs] + [np.zeros(0, np.int32)]).astype(np.int32)
    count = np.concatenate([np.asarray(c, np.int32) for _, c in docs] + [np.zeros(0, np.int32)]).astype(np.int32)
    return dp, term, count


def planted(seed, K=5, V=96, n_clean=12, n_bad=12, share=0.25):
    """The corpus of the issue's prototype: K Dirichlet(0.1) signatures over V terms; n_clean documents drawn exactly from their own mixture
    (Dirichlet(0.5) exposures, totals spread geometrically over 135 .. 3000) and n_bad of which `share` of the mutations comes from a
    signature the table lacks (totals over 1000 .. 3000: a quarter of 135 mutations is too little for either statistic to see every
    time).  The props are the TRUE exposures, so the p-values of the clean half are calibrated.
    -> (doc_ptr, term, count, props [D, K], phi [K, V], bad [D] bool)"""
    rng = np.random.default_rng(seed)
    phi = rng.dirichlet(np.full(V, 0.1), size=K)
    extra = rng.dirichlet(np.full(V, 0.1))
    D = n_clean + n_bad
    props = rng.dirichlet(np.full(K, 0.5), size=D)
    totals = np.concatenate([np.geomspace(135, 3000, n_clean), np.geomspace(1000, 3000, n_bad)]).round().astype(np.int64)
    bad = np.arange(D) >= n_clean
    docs = []
    for d in range(D):
        p = props[d] @ phi
        n_x = int(round(share * totals[d])) if bad[d] else 0
        n = rng.multinomial(totals[d] - n_x, p / p.sum()) + rng.multinomial(n_x, extra)
        t = np.flatnonzero(n)
        docs.append((t, n[t]))
    return csr(docs) + (props, phi, bad)


def edge_corpus(V, K, seed=0):
    """Unnormalised props and phi with leading, interior and trailing zero-probability terms (where V leaves room), and documents whose
    totals sit on the Philox-block and 64-lane-step edges; document 1 is empty, document 2 holds a duplicate term, document 3 (V >= 5) an
    observed count on a zero-probability term.  -> (doc_ptr, term, count, props [D, K], phi [K, V], zero [V] bool)"""
    rng = np.random.default_rng([seed, V, K])
    phi = rng.gamma(0.3, size=(K, V)) * 3.0 + 1e-3
    zero = np.zeros(V, dtype=bool)
    if V >= 5:
        zero[[0, V // 2, V - 1]] = True
        if V >= 64:
            zero[[1, 62, 63, V - 2]] = True
        phi[:, zero] = 0.0
    totals = [5000 + V % 7, 0, 1, 3, 4, 5, 255, 256, 257]
    D = len(totals)
    props = rng.gamma(0.7, size=(D, K)) * 2.5 + 1e-3
    if K > 1:
        props[4, 0] = 0.0
    live = np.flatnonzero(~zero)
    docs = []
    for d, N in enumerate(totals):
        if N == 0:
            docs.append((np.zeros(0, np.int32), np.zeros(0, np.int32)))
            continue
        p = mixture(props[d], phi)
        odd = d == 3 and zero.any()                  # one count the model cannot produce
        n = rng.multinomial(N - 1 if odd else N, p / p.sum())
        if odd:
            n[np.flatnonzero(zero)[1]] += 1
        t = np.flatnonzero(n); c = n[t]
        if d == 0:                                   # a term in two entries (the total is kept) and an entry with a zero count
            j = int(np.argmax(c))
            t = np.concatenate([t, t[j:j + 1], live[:1]]); c = np.concatenate([c, [1], [0]]); c[j] -= 1
        docs.append((t[::-1].copy(), c[::-1].copy()))      # entries need not be sorted
    return csr(docs) + (props, phi, zero)
