"""Independent numpy/scipy restatement of LDA frozen-topic inference, written from src/LDA.jl of the reference (line numbers below are
that file's), NOT from oracle/mmm_oracle.c: dense loops over documents, the reference's nested layout (ϕ[d] K x W_d, γ / θ K x D, the
tables V x K), every sum in np.longdouble and rounded to double once.  tests/test_lda_infer_ref_cpu.py holds the C oracle to it,
tests/test_lda_infer_dispatch_gpu.py the device.  `cases()` is the fixed list both files walk: every E-step build that `mmm_lda_infer`
can launch (csrc/lda.hip frozen_passes), each with the geometry the handle must report."""
import collections

import numpy as np
from scipy.special import digamma, gammaln

LD = np.longdouble


def _d(x):
    return np.asarray(x, dtype=np.float64)


class Lda:
    """`mutable struct LDA` in its constructor state (LDA.jl:24-54) on documents X, and the functions frozen-topic inference calls.
    X[d]: (W_d, 2) [term (1-based), count].  beta / Elnbeta / lam: V x K, assigned by the caller (LDA.jl:237, :269-271)."""

    def __init__(self, K, alpha, V, X, eta=None):
        self.K, self.alpha, self.V = int(K), float(alpha), int(V)
        self.eta = None if eta is None else float(eta)
        self.X = [np.asarray(x, dtype=np.int64).reshape(-1, 2) for x in X]
        self.D = len(self.X)                                                                         # :32
        self.N = np.array([int(x[:, 1].sum()) for x in self.X], dtype=np.int64)                      # :33
        self.lam = None; self.beta = None; self.Elnbeta = None                                       # :36-39, replaced by the caller's
        self.gamma = np.ones((self.K, self.D))                                                       # :41
        self.theta = None                                                                            # :42 (undef)
        self.update_Elntheta()                                                                       # :43-44
        self.phi = [np.full((self.K, x.shape[0]), 1.0 / self.K) for x in self.X]                     # :46-49
        self.converged = False                                                                       # :51

    def update_Elntheta(self):                                                                       # :78-80
        g = self.gamma
        self.Elntheta = digamma(g) - digamma(_d(g.astype(LD).sum(axis=0, keepdims=True)))

    def update_gamma(self):                                                                          # :82-90
        g = np.full((self.K, self.D), self.alpha, dtype=LD)
        for d in range(self.D):
            g[:, d] += (self.phi[d].astype(LD) * self.X[d][:, 1].astype(LD)[None, :]).sum(axis=1)   # ϕ[d] * X[d][:, 2]
        self.gamma = _d(g)
        self.update_Elntheta()

    def update_phi(self):                                                                            # :69-76
        for d in range(self.D):
            v = self.X[d][:, 0] - 1
            e = np.exp(self.Elntheta[:, d].astype(LD)[:, None] + self.Elnbeta[v, :].T.astype(LD))
            self.phi[d] = _d(e / e.sum(axis=0, keepdims=True))

    def unsmoothed_update_phi(self):                                                                 # :226-231
        for d in range(self.D):
            v = self.X[d][:, 0] - 1
            e = np.exp(self.Elntheta[:, d].astype(LD))[:, None] * self.beta[v, :].T.astype(LD)
            self.phi[d] = _d(e / e.sum(axis=0, keepdims=True))

    def update_theta(self):                                                                          # :92-94
        g = self.gamma.astype(LD)
        self.theta = _d(g / g.sum(axis=0, keepdims=True))

    def loglikelihood(self):                                                                         # :174-188
        ll = LD(0); N = 0
        for d in range(self.D):
            n = self.X[d][:, 1]
            N += int(n.sum())
            v = self.X[d][:, 0] - 1
            p = (self.beta[v, :].astype(LD) * self.theta[:, d].astype(LD)[None, :]).sum(axis=1)     # dot(θ[:, d], β[v, :])
            ll += (n.astype(LD) * np.log(p)).sum()
        return float(ll / N)

    def elbo_terms(self):
        """(elbo, the seven terms in the order of calculate_elbo, :162-172)."""
        K, D, V, eta, al = self.K, self.D, self.V, self.eta, self.alpha
        t = np.zeros(7, dtype=LD)
        t[0] = K * (LD(gammaln(V * eta)) - V * LD(gammaln(eta))) + (LD(eta) - 1) * self.Elnbeta.astype(LD).sum()             # :114-118
        t[1] = D * (LD(gammaln(K * al)) - K * LD(gammaln(al))) + (LD(al) - 1) * self.Elntheta.astype(LD).sum()                # :120-124
        for d in range(D):
            n = self.X[d][:, 1].astype(LD)
            v = self.X[d][:, 0] - 1
            p = self.phi[d].astype(LD)
            t[2] += (p * self.Elntheta[:, d].astype(LD)[:, None] * n[None, :]).sum()                 # :126-132
            t[3] += (p.T * self.Elnbeta[v, :].astype(LD) * n[:, None]).sum()                         # :134-140
            t[6] += np.where(p > 0, p * np.log(np.where(p > 0, p, LD(1))), LD(0)).sum()              # :154-160, log(0^0) = 0
        l = self.lam                                                                                 # :142-146
        t[4] = gammaln(l).astype(LD).sum() - gammaln(_d(l.astype(LD).sum(axis=0))).astype(LD).sum() - ((l.astype(LD) - 1) * self.Elnbeta.astype(LD)).sum()
        g = self.gamma                                                                               # :148-152
        t[5] = gammaln(g).astype(LD).sum() - gammaln(_d(g.astype(LD).sum(axis=0))).astype(LD).sum() - ((g.astype(LD) - 1) * self.Elntheta.astype(LD)).sum()
        e = t[0] + t[1] + t[2] + t[3] - t[4] - t[5] - t[6]
        return float(e), _d(t)


Run = collections.namedtuple("Run", "ll gamma theta phi converged ratio model")


def stop_ratio(ll):
    """|ll[-2] - ll[-1]| / |ll[-1]| (common.jl:53-56); nan while there is one value."""
    return abs(ll[-2] - ll[-1]) / abs(ll[-1]) if len(ll) > 1 else float("nan")


def infer(X, K, alpha, beta, Elnbeta, lam, unsmoothed, maxiter, tol, phi0=None, eta=None):
    """The loop of `transform` (unsmoothed; LDA.jl:233-263) or of `fit_heldout` (:265-295) on documents X under the given V x K tables.
    phi0: start from this ϕ (list of K x W_d) instead of the constructor's 1/K.  Returns Run(ll history, γ, θ, ϕ, converged, the stop ratio
    of every pass, the model -- whose elbo_terms() is calculate_elbo when lam, Elnbeta and eta were given)."""
    beta = _d(beta)
    m = Lda(K, alpha, beta.shape[0], X, eta=eta)
    m.beta = beta.copy()                                                                             # :237 / :270
    m.Elnbeta = None if Elnbeta is None else _d(Elnbeta).copy()                                      # :271
    m.lam = None if lam is None else _d(lam).copy()                                                  # :269
    if phi0 is not None:
        m.phi = [_d(p).copy() for p in phi0]
        assert [p.shape for p in m.phi] == [(m.K, x.shape[0]) for x in m.X]
    ll, ratio = [], []
    for _ in range(maxiter):                                                                         # :241 / :274
        m.update_gamma()
        if unsmoothed:
            m.unsmoothed_update_phi()
        else:
            m.update_phi()
        m.update_theta()
        ll.append(m.loglikelihood())
        ratio.append(stop_ratio(ll))
        if len(ll) > 10 and ratio[-1] < tol:                                                         # :252 / :286
            m.converged = True
            break
    return Run(np.array(ll), m.gamma, m.theta, m.phi, m.converged, np.array(ratio), m)


def phi_rows(phi):
    """ϕ as one [nnz, K] array, the documents' blocks one after the other (the flat layout of the device and of the oracle)."""
    K = phi[0].shape[0] if phi else 0
    return np.concatenate([p.T for p in phi], axis=0) if phi else np.zeros((0, K))


def phi_docs(flat, X):
    """The inverse: [nnz, K] -> list of K x W_d."""
    out, a = [], 0
    for x in X:
        w = np.asarray(x).reshape(-1, 2).shape[0]
        out.append(np.ascontiguousarray(flat[a:a + w].T)); a += w
    return out


def dist(a, b, atol=0.0):
    """max over entries of (|a - b| - atol) / |b|: the smallest rtol with which assert_allclose(a, b, rtol, atol) passes."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(np.abs(a - b) <= atol, 0.0, (np.abs(a - b) - atol) / np.abs(b))
    return float(r.max())


# ------------------------------------------------------------------------------------------------------ cases
ALPHA, ETA = 0.1, 0.1
TRAIN_D, TRAIN_PASSES = 120, 15
PASSES = 12


def heldout_corpus(seed, D, V, K, mean_n, conc):
    """D documents drawn from a K-topic mixture over V terms (conc: Dirichlet concentration of the topics; 1.0 gives documents that list
    most terms, 0.1 sparse ones), then the edge documents every case carries: document 0 holds an entry with count 0, document 1 is
    empty and the last document has one entry.  (A corpus of one document is that document 0 alone.)"""
    rng = np.random.Generator(np.random.PCG64([seed, D, V, K]))
    beta = rng.dirichlet(np.full(V, conc), size=K)
    X = []
    for d in range(D):
        th = rng.dirichlet(np.full(K, 0.5))
        c = rng.multinomial(20 + rng.poisson(mean_n), th @ beta)
        idx = np.nonzero(c)[0]
        X.append(np.stack([idx + 1, c[idx]], axis=1).astype(np.int64))
    assert X[0].shape[0] >= 3
    X[0][1, 1] = 0
    if D >= 3:
        X[1] = np.zeros((0, 2), dtype=np.int64)
        X[D - 1] = np.array([[7 % V + 1, 5]], dtype=np.int64)
    return X


def _geo(L, KP, single_step, wide, row_bytes, waves_e, grid_e, dense=0):
    return dict(L=L, KP=KP, single_step=single_step, wide=wide, row_bytes=row_bytes, waves_e=waves_e, grid_e=grid_e, dense=dense)


# name, V, K, D, tuning, (mean_n, conc), what mmm_lda_geometry / mmm_lda_row_bytes must report on a 256-CU device.  row_bytes: 2 * 16 * SLs
# rows of 16-bit counts, 4 * 16 * SL rows of 32-bit counts, 8 V padded (term, count) pairs, 0 the CSR reader (or the wide path).
DENSE, SPARSE = (400, 1.0), (150, 0.1)
_SPECS = [
    # ---- single-step (L = 16, KP <= 12, V <= 96, the grid covers every document), rows of 16-bit counts where the corpus is dense enough
    ("s16_k6_v96_d70", 96, 6, 70, {}, DENSE, _geo(16, 6, 1, 0, 192, 4, 5)),
    ("s16_k7_v96_d37", 96, 7, 37, {}, DENSE, _geo(16, 8, 1, 0, 192, 4, 3)),
    ("s16_k10_v96_d70", 96, 10, 70, {}, DENSE, _geo(16, 10, 1, 0, 192, 4, 5)),
    ("s16_k12_v96_d3", 96, 12, 3, {}, DENSE, _geo(16, 12, 1, 0, 768, 4, 1)),
    ("s16_k1_v50_d37", 50, 1, 37, {}, DENSE, _geo(16, 2, 1, 0, 192, 4, 3)),
    ("s16_k2_v50_d1", 50, 2, 1, {}, DENSE, _geo(16, 2, 1, 0, 192, 4, 1)),
    ("s16_k7_v50_d70", 50, 7, 70, {}, DENSE, _geo(16, 8, 1, 0, 192, 4, 5)),
    ("s16_k1_v33_d3", 33, 1, 3, {}, DENSE, _geo(16, 2, 1, 0, 264, 4, 1)),
    ("s16_k2_v33_d37", 33, 2, 37, {}, DENSE, _geo(16, 2, 1, 0, 128, 4, 3)),
    ("s16_k7_v33_d70", 33, 7, 70, {}, DENSE, _geo(16, 8, 1, 0, 128, 4, 5)),
    # ---- single-step, the other corpus forms
    ("s32_k10_v96_norows16", 96, 10, 70, {"disable": ("lda_rows16",)}, DENSE, _geo(16, 10, 1, 0, 384, 4, 5)),
    ("s32_k10_v96_bigcount", 96, 10, 70, {}, DENSE, _geo(16, 10, 1, 0, 384, 4, 5)),
    ("pairs_k10_v96", 96, 10, 70, {"disable": ("lda_count_rows",)}, DENSE, _geo(16, 10, 1, 0, 768, 4, 5)),
    # ---- single-step, pinned waves per block: 1 and 3 leave table entries beyond the register-held part, 12 is the most
    ("w1_k10_v96", 96, 10, 70, {"waves_per_block": 1}, DENSE, _geo(16, 10, 1, 0, 192, 1, 18)),
    ("w3_k10_v96", 96, 10, 70, {"waves_per_block": 3}, DENSE, _geo(16, 10, 1, 0, 192, 3, 6)),
    ("w12_k10_v96", 96, 10, 70, {"waves_per_block": 12}, DENSE, _geo(16, 10, 1, 0, 192, 12, 2)),
    # ---- grid-stride, L = 16: 3 blocks of 8 waves = 96 documents per step
    ("gs_k10_d97", 96, 10, 97, {"grid_blocks": 3}, DENSE, _geo(16, 10, 0, 0, 192, 8, 3)),
    ("gs_k10_d200", 96, 10, 200, {"grid_blocks": 3}, DENSE, _geo(16, 10, 0, 0, 192, 8, 3)),
    ("gs_k10_d240", 96, 10, 240, {"grid_blocks": 3}, DENSE, _geo(16, 10, 0, 0, 192, 8, 3)),
    ("gs_k10_d200_pairs", 96, 10, 200, {"grid_blocks": 3, "disable": ("lda_count_rows",)}, DENSE, _geo(16, 10, 0, 0, 768, 8, 3)),
    # ---- K = 13..15: KP = 16 at L = 16, never single-step
    ("k13_v96", 96, 13, 70, {}, DENSE, _geo(16, 16, 0, 0, 192, 4, 5)),
    ("k15_v96_g2_pairs", 96, 15, 70, {"grid_blocks": 2, "disable": ("lda_count_rows",)}, SPARSE, _geo(16, 16, 0, 0, 768, 4, 2)),
    ("k13_v130_g2", 130, 13, 70, {"grid_blocks": 2}, DENSE, _geo(16, 16, 0, 0, 0, 2, 2)),
    ("k15_v130", 130, 15, 70, {}, DENSE, _geo(16, 16, 0, 0, 0, 2, 9)),
    # ---- the CSR reader: documents of more than 96 and more than 192 distinct terms; a document that lists a term twice
    ("csr_v300_k5", 300, 5, 60, {}, (480, 1.0), _geo(16, 6, 0, 0, 0, 3, 5)),
    ("csr_dup_v24_k6", 24, 6, 40, {}, DENSE, _geo(16, 6, 1, 0, 0, 4, 3)),
    # ---- L = 32 (two documents per wave step)
    ("l32_k16_v96", 96, 16, 150, {}, DENSE, _geo(32, 16, 0, 0, 768, 4, 19)),
    ("l32_k20_v50", 50, 20, 150, {}, DENSE, _geo(32, 20, 0, 0, 400, 7, 11)),
    ("l32_k24_v96_d3", 96, 24, 3, {}, DENSE, _geo(32, 24, 0, 0, 768, 2, 1)),
    ("l32_k25_v96", 96, 25, 150, {"lda_build": "sparse"}, DENSE, _geo(32, 32, 0, 0, 768, 1, 75)),
    ("l32_k31_v50", 50, 31, 150, {"lda_build": "sparse"}, DENSE, _geo(32, 32, 0, 0, 400, 4, 19)),
    ("l32_k20_v96_g2", 96, 20, 150, {"grid_blocks": 2}, DENSE, _geo(32, 20, 0, 0, 768, 3, 2)),
    ("l32_k24_v50_d3_g2", 50, 24, 3, {"grid_blocks": 2}, DENSE, _geo(32, 24, 0, 0, 400, 6, 2)),
    # ---- L = 64 (one document per wave, two prefetched chunks)
    ("l64_k32_v30", 30, 32, 40, {"lda_build": "sparse"}, DENSE, _geo(64, 32, 0, 0, 240, 8, 5)),
    ("l64_k32_v120", 120, 32, 40, {"lda_build": "sparse"}, DENSE, _geo(64, 32, 0, 0, 960, 1, 40)),
    # ---- the wide path: tables by term through L2; k_lda_estep_wide up to 32 padded topics, k_lda_estep_big beyond
    ("wide_k5_v24", 24, 5, 40, {"lda_build": "wide"}, DENSE, _geo(16, 6, 0, 1, 0, 4, 10)),
    ("wide_k33_v50", 50, 33, 40, {}, DENSE, _geo(64, 34, 0, 1, 0, 3, 10)),
    ("wide_k48_v96", 96, 48, 60, {}, DENSE, _geo(64, 48, 0, 1, 0, 1, 15)),
    ("wide_k64_v50", 50, 64, 40, {}, DENSE, _geo(64, 64, 0, 1, 0, 1, 10)),
    ("wide_k65_v96", 96, 65, 40, {}, DENSE, _geo(64, 66, 0, 1, 0, 1, 10)),
    ("wide_k129_v96", 96, 129, 40, {}, DENSE, _geo(64, 130, 0, 1, 0, 1, 10)),
    ("wide_k256_v96", 96, 256, 37, {}, DENSE, _geo(64, 256, 0, 1, 0, 1, 10)),
    # ---- a device pretended to have 2 CUs: whatever build results (asserted): the handle is a dense-row one (D > 96), whose frozen passes run
    #      the grid-stride build over its rows of counts, two blocks, four steps per wave
    ("cus2_k10_d200", 96, 10, 200, {"geometry_cus": 2}, DENSE, _geo(16, 10, 0, 0, 192, 8, 2, dense=1)),
]

# one representative of single-step, grid-stride L = 16, L = 32 and the wide path at K = 48 (the property tests)
REPRESENTATIVES = ("s16_k10_v96_d70", "gs_k10_d200", "l32_k20_v96_g2", "wide_k48_v96")


# corpus draws of the held-out documents: a case whose stopped run (tol = 1e-4) has a stop ratio within 5 % of the tolerance after the 10th
# pass, in either mode, takes its next draw (tests/test_lda_infer_ref_cpu.py asserts the margin)
_DRAW = {"s16_k7_v96_d37": 1, "s16_k10_v96_d70": 3, "s32_k10_v96_bigcount": 5, "pairs_k10_v96": 2, "gs_k10_d97": 10, "gs_k10_d200": 1, "k13_v96": 8,
         "k15_v96_g2_pairs": 2, "k13_v130_g2": 8, "l32_k16_v96": 2, "l32_k24_v96_d3": 7, "l32_k25_v96": 13, "l32_k24_v50_d3_g2": 1, "l64_k32_v30": 5,
         "wide_k129_v96": 25, "wide_k256_v96": 7, "l32_k20_v96_g2": 2, "l64_k32_v120": 3, "wide_k33_v50": 20, "wide_k48_v96": 11, "wide_k64_v50": 9,
         "wide_k65_v96": 10, "cus2_k10_d200": 2}


def _case(n, draw=None):
    import np_ref
    name, V, K, D, tune, (mean_n, conc), geo = _SPECS[n]
    draw = _DRAW.get(name, 0) if draw is None else draw
    Xt, lam0 = np_ref.synth_lda(TRAIN_D, V, K, seed=500 + n, mean_n=300)
    Xn = heldout_corpus(900 + n + 1000 * draw, D, V, K, mean_n, conc)
    if name == "s32_k10_v96_bigcount":           # one count that no 16-bit slot holds
        Xn[5][0, 1] = 65536
    if name == "csr_dup_v24_k6":                 # every term, then the first once more: 25 rows, no padded row of V slots holds them
        Xn[4] = np.stack([np.concatenate([np.arange(1, V + 1), [1]]), np.concatenate([np.arange(2, V + 2), [9]])], axis=1).astype(np.int64)
    return dict(name=name, V=V, K=K, D=D, alpha=ALPHA, eta=ETA, tuning=dict(tune), mean_n=mean_n, Xt=Xt, lam0=lam0, Xn=Xn, geometry=geo)


def cases():
    """The fixed list of the walk.  Each case: name, trained shape (V, K), training corpus and λ0 (np_ref.synth_lda, TRAIN_D documents),
    held-out corpus Xn (D documents), tuning keywords of the held-out handle and the geometry that handle must report."""
    return [_case(n) for n in range(len(_SPECS))]


def has_edge_documents(c):
    """An empty document, a one-entry document and a document holding an entry with count 0 (one document: the last of these alone)."""
    X = c["Xn"]
    zero = any((x[:, 1] == 0).any() for x in X)
    if c["D"] == 1:
        return zero
    return zero and any(x.shape[0] == 0 for x in X) and any(x.shape[0] == 1 for x in X)
