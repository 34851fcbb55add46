"""Independent numpy/scipy restatement of ILDA, written from src/ILDA.jl of the reference (line numbers below are that file's), NOT from
oracle/mmm_oracle.c: dense loops over documents, the reference's nested layout (λ[i] J_i x K, ϕ[d] K x W_d, γ / θ K x D), every sum in
np.longdouble and rounded to double once.  tests/test_ilda_ref_cpu.py holds the C oracle to it, tests/test_ilda_dispatch_gpu.py the device.
`draw_cases` is the fixed list of feature tables and corpora both files walk."""
import numpy as np
from scipy.special import digamma, gammaln

LD = np.longdouble
TERMS = ("ElnPβ", "ElnPθ", "ElnPZ", "ElnPX", "ElnQβ", "ElnQθ", "ElnQZ")


def _d(x):
    return np.asarray(x, dtype=np.float64)


def _dirichlet_mean_log(a):
    """digamma.(a) .- digamma.(sum(a, dims=1)) (ILDA.jl:82, :101-103); the column sums in extended precision."""
    return digamma(a) - digamma(_d(a.astype(LD).sum(axis=0, keepdims=True)))


class Ilda:
    """`mutable struct ILDA` and its functions.  features: V x I, 1-based values; J = column maxima (ILDA.jl:35).  X[d]: (W_d, 2)
    [term (1-based), count].  lam0: list over features of J_i x K matrices (the reference draws rand(1:100), :38)."""

    def __init__(self, K, alpha, eta, features, X, lam0):
        self.K, self.alpha = int(K), float(alpha)
        self.features = np.asarray(features, dtype=np.int64)
        self.V, self.I = self.features.shape
        self.J = [int(j) for j in self.features.max(axis=0)]
        self.eta = np.full(self.I, float(eta)) if np.ndim(eta) == 0 else _d(eta).copy()                 # :59-63
        self.X = [np.asarray(x, dtype=np.int64).reshape(-1, 2) for x in X]
        self.D = len(self.X)
        self.lam = [_d(l).copy() for l in lam0]
        assert [l.shape for l in self.lam] == [(j, self.K) for j in self.J]
        self.Elnbeta = [None] * self.I
        self.update_Elnbeta()                                                                        # :39-42
        self.gamma = np.ones((self.K, self.D))                                                       # :44
        self.update_Elntheta()                                                                       # :45-46
        self.phi = [np.full((self.K, x.shape[0]), 1.0 / self.K) for x in self.X]                     # :48-51
        self.beta = None; self.theta = None
        self.converged = False

    # ---- the five updates ------------------------------------------------------------------------------------
    def _rows(self, tabs, d):
        """[tabs[i][features[v, i], :] for the terms v of document d]: list over features of W_d x K."""
        v = self.X[d][:, 0] - 1
        return [tabs[i][self.features[v, i] - 1, :] for i in range(self.I)]

    def update_phi(self):                                                                            # :65-79
        for d in range(self.D):
            a = np.repeat(self.Elntheta[:, d].astype(LD)[:, None], self.X[d].shape[0], axis=1)
            for r in self._rows(self.Elnbeta, d):
                a = a + r.T.astype(LD)
            e = np.exp(a)
            self.phi[d] = _d(e / e.sum(axis=0, keepdims=True))

    def update_Elntheta(self):                                                                       # :81-83
        self.Elntheta = _dirichlet_mean_log(self.gamma)

    def update_gamma(self):                                                                          # :85-93
        g = np.full((self.K, self.D), self.alpha, dtype=LD)
        for d in range(self.D):
            g[:, d] += (self.phi[d].astype(LD) * self.X[d][:, 1].astype(LD)[None, :]).sum(axis=1)
        self.gamma = _d(g)
        self.update_Elntheta()

    def update_theta(self):                                                                          # :95-97
        g = self.gamma.astype(LD)
        self.theta = _d(g / g.sum(axis=0, keepdims=True))

    def update_Elnbeta(self):                                                                        # :99-105
        for i in range(self.I):
            self.Elnbeta[i] = _dirichlet_mean_log(self.lam[i])

    def update_lambda(self):                                                                         # :107-126
        lam = [np.full((self.J[i], self.K), self.eta[i], dtype=LD) for i in range(self.I)]
        for d in range(self.D):
            v = self.X[d][:, 0] - 1
            nphi = self.phi[d].T.astype(LD) * self.X[d][:, 1].astype(LD)[:, None]                    # W x K
            for i in range(self.I):
                np.add.at(lam[i], self.features[v, i] - 1, nphi)                                     # repeated rows accumulate
        self.lam = [_d(l) for l in lam]
        self.update_Elnbeta()

    def update_beta(self):                                                                           # :128-130
        self.beta = [_d(l.astype(LD) / l.astype(LD).sum(axis=0, keepdims=True)) for l in self.lam]

    # ---- log-likelihood and ELBO --------------------------------------------------------------------------------
    def loglikelihood(self):                                                                         # :209-236
        ll = LD(0); N = 0
        for d in range(self.D):
            n = self.X[d][:, 1]
            N += int(n.sum())
            p = np.repeat(self.theta[:, d].astype(LD)[None, :], n.size, axis=0)                      # W x K
            for r in self._rows(self.beta, d):
                p = p * r.astype(LD)
            ll += (n.astype(LD) * np.log(p.sum(axis=1))).sum()
        return float(ll / N)

    def ElnQbeta_of(self, i):
        """One feature's term of calculate_ElnQβ (:177-178)."""
        l = self.lam[i]
        q = gammaln(l).astype(LD).sum() - gammaln(_d(l.astype(LD).sum(axis=0))).astype(LD).sum()
        return float(q - ((l.astype(LD) - 1) * self.Elnbeta[i].astype(LD)).sum())

    def elbo_terms(self):
        """(elbo, the seven terms in the order of calculate_elbo, :197-207)."""
        K, D = self.K, self.D
        t = np.zeros(7, dtype=LD)
        for i in range(self.I):                                                                      # :132-141
            J, eta = self.J[i], self.eta[i]
            t[0] += K * (LD(gammaln(J * eta)) - J * LD(gammaln(eta))) + (LD(eta) - 1) * self.Elnbeta[i].astype(LD).sum()
        t[1] = D * (LD(gammaln(K * self.alpha)) - K * LD(gammaln(self.alpha))) + (LD(self.alpha) - 1) * self.Elntheta.astype(LD).sum()   # :143-147
        for d in range(D):
            n = self.X[d][:, 1].astype(LD)
            p = self.phi[d].astype(LD)
            t[2] += (p * self.Elntheta[:, d].astype(LD)[:, None] * n[None, :]).sum()                 # :149-155
            for r in self._rows(self.Elnbeta, d):                                                    # :157-172
                t[3] += (p.T * n[:, None] * r.astype(LD)).sum()
            t[6] += np.where(p > 0, p * np.log(np.where(p > 0, p, LD(1))), LD(0)).sum()              # :189-195, log(0^0) = 0
        t[4] = self.ElnQbeta_of(self.I - 1)                                                          # :174-181: `lnq =` inside the loop, the last feature's term survives
        g = self.gamma                                                                               # :183-187
        t[5] = gammaln(g).astype(LD).sum() - gammaln(_d(g.astype(LD).sum(axis=0))).astype(LD).sum() - ((g.astype(LD) - 1) * self.Elntheta.astype(LD)).sum()
        e = t[0] + t[1] + t[2] + t[3] - t[4] - t[5] - t[6]
        return float(e), _d(t)

    # ---- drivers ------------------------------------------------------------------------------------------------
    def one_pass(self):
        """The body of fit! (:250-257); returns the pass's log-likelihood."""
        self.update_gamma(); self.update_phi(); self.update_lambda(); self.update_beta(); self.update_theta()
        return self.loglikelihood()

    @staticmethod
    def _stop(ll, tol):                                                                              # :263 ; common.jl:53-56
        return len(ll) > 10 and abs(ll[-2] - ll[-1]) / abs(ll[-1]) < tol

    def fit(self, maxiter=1000, tol=1e-4):                                                           # :246-272
        ll = []
        for _ in range(maxiter):
            ll.append(self.one_pass())
            if self._stop(ll, tol):
                self.converged = True
                break
        self.elbo, _ = self.elbo_terms()
        self.ll = ll[-1]
        self.ll_history = np.array(ll)
        return self.ll_history

    def fit_heldout(self, X, maxiter=100):                                                           # :323-353
        new = Ilda(self.K, self.alpha, self.eta, self.features, X, [np.ones_like(l) for l in self.lam])
        new.J = list(self.J)                       # the held-out constructor re-derives J from the same table
        new.lam = [l.copy() for l in self.lam]; new.beta = [b.copy() for b in self.beta]; new.Elnbeta = [e.copy() for e in self.Elnbeta]
        ll = []
        for _ in range(maxiter):
            new.update_gamma(); new.update_phi(); new.update_theta()
            ll.append(new.loglikelihood())
            if self._stop(ll, 1e-4):
                new.converged = True
                break
        new.elbo, _ = new.elbo_terms()
        new.ll = ll[-1]
        new.ll_history = np.array(ll)
        return new


# ------------------------------------------------------------------------------------------------------ cases
SNV3 = np.array([[t // 16 + 1, (t // 4) % 4 + 1, t % 4 + 1] for t in range(96)])


def full_product(J):
    """Every combination of feature values once, first feature slowest (the SNV / pentanucleotide layout)."""
    grids = np.meshgrid(*[np.arange(1, j + 1) for j in J], indexing="ij")
    return np.stack([g.ravel() for g in grids], axis=1)


def random_table(rng, V, J, used=None):
    """V terms with drawn feature values; the maximum of every feature is carried by some term (so J is the column maxima).  used[i]:
    the values feature i may take (default all)."""
    f = np.empty((V, len(J)), dtype=np.int64)
    for i, j in enumerate(J):
        pool = np.arange(1, j + 1) if used is None or used[i] is None else np.asarray(used[i])
        f[:, i] = rng.choice(pool, size=V)
        f[(7 * i + 3) % V, i] = j
    return f


def corpus(rng, D, V, K, mean_n, conc=0.1):
    """Documents drawn from a K-topic mixture over V terms: X[d] lists the terms that occurred, with counts."""
    beta = rng.dirichlet(np.full(V, conc), size=max(K, 2))
    X = []
    for d in range(D):
        th = rng.dirichlet(np.full(beta.shape[0], 0.5))
        c = rng.multinomial(20 + rng.poisson(mean_n), th @ beta)
        idx = np.nonzero(c)[0]
        X.append(np.stack([idx + 1, c[idx]], axis=1).astype(np.int64))
    return X


def _case(rng, name, features, K, D, mean_n, eta=None, alpha=0.1):
    features = np.asarray(features, dtype=np.int64)
    V, I = features.shape
    J = [int(j) for j in features.max(axis=0)]
    if eta is None:
        eta = [float(x) for x in np.round(rng.uniform(0.05, 0.6, size=I), 3)]
    X = corpus(rng, D, V, K, mean_n)
    lam0 = [rng.integers(1, 101, size=(j, K)).astype(np.float64) for j in J]
    return dict(name=name, V=V, I=I, J=J, K=K, D=D, mean_n=mean_n, eta=list(eta), alpha=alpha, features=features, X=X, lam0=lam0)


N_DRAWN = 12
NAMED = ("identity", "identity_small", "I8", "bigJ", "sj512", "penta", "v257", "sj16", "sj17", "tiny", "holes", "K1", "K33", "K65", "K100",
         "dup", "empty")


def draw_cases(seed=20261016):
    """The fixed case list: the named cases (each reaches a branch of the ILDA dispatch that the SNV3 table does not), then N_DRAWN
    drawn ones (I in 1..5, J_i in 2..8, V in 5..400, K in 1..24, D in 3..700).  Deterministic in `seed`."""
    out = []
    for n, name in enumerate(NAMED):
        rng = np.random.Generator(np.random.PCG64([seed, n]))
        if name == "identity":                       # one feature whose value is the term: ILDA == LDA; sum J > 16
            c = _case(rng, name, np.arange(1, 78)[:, None], 6, 120, 300)
        elif name == "identity_small":               # the same with sum J <= 16 (merged launch)
            c = _case(rng, name, np.arange(1, 14)[:, None], 4, 90, 80)
        elif name == "I8":                           # the most features a handle takes
            c = _case(rng, name, random_table(rng, 150, [2, 3, 2, 3, 3, 2, 3, 2]), 7, 80, 400)
        elif name == "bigJ":                         # a feature with more than 64 values, most of them carried by no term
            used0 = np.concatenate([rng.choice(np.arange(1, 200), size=110, replace=False), [200]])
            c = _case(rng, name, random_table(rng, 587, [200, 5], used=[used0, None]), 5, 60, 900)
        elif name == "sj512":                        # sum J at the limit
            c = _case(rng, name, random_table(rng, 700, [300, 200, 12]), 4, 50, 1200)
        elif name == "penta":                        # 1536 pentanucleotide contexts: tables beyond LDS
            c = _case(rng, name, full_product([6, 4, 4, 4, 4]), 10, 64, 3000)
        elif name == "v257":                         # V just above 256, small tables
            c = _case(rng, name, random_table(rng, 260, [6, 5, 5]), 6, 70, 500)
        elif name in ("sj16", "sj17"):               # the same table and corpus but for one extra value of feature 0
            rng = np.random.Generator(np.random.PCG64([seed, 1000]))
            f = random_table(rng, 90, [8, 4, 4])
            c = _case(rng, name, f, 5, 110, 350, eta=[0.1, 0.3, 0.2])
            if name == "sj17":
                f = f.copy(); f[41, 0] = 9
                lam0 = [np.vstack([c["lam0"][0], rng.integers(1, 101, size=(1, 5)).astype(np.float64)])] + c["lam0"][1:]
                c.update(features=f, J=[9, 4, 4], lam0=lam0)
        elif name == "tiny":                         # fewer terms than feature values
            c = _case(rng, name, np.array([[1, 3], [3, 1], [2, 2], [1, 1], [3, 3]]), 3, 40, 30)
        elif name == "holes":                        # value 3 of feature 0 is carried by no term; V = 77 is no multiple of 16
            f = SNV3[SNV3[:, 0] != 3][:77]
            c = _case(rng, name, f, 5, 100, 400)
        elif name in ("K1", "K33", "K65", "K100"):   # rolled topic loops / the big statistics kernel on SNV3
            c = _case(rng, name, SNV3, int(name[1:]), 48, 1500)
        elif name == "dup":                          # a document that lists a term twice (the reference treats the rows separately)
            c = _case(rng, name, SNV3[:40], 4, 30, 200)
            c["X"][7] = np.vstack([c["X"][7], c["X"][7][:1]])
        elif name == "empty":                        # empty documents first and last
            c = _case(rng, name, SNV3[::2], 5, 45, 250)
            c["X"][0] = np.zeros((0, 2), dtype=np.int64); c["X"][-1] = np.zeros((0, 2), dtype=np.int64)
        c["name"] = name
        out.append(c)
    rng = np.random.Generator(np.random.PCG64([seed, 2000]))
    for n in range(N_DRAWN):
        I = int(rng.integers(1, 6))
        J = [int(j) for j in rng.integers(2, 9, size=I)]
        V = int(rng.integers(max(5, I), 401))
        K = int(rng.integers(1, 25))
        D = int(rng.integers(3, 701))
        mean_n = int(rng.integers(V // 4 + 2, V + 3))
        out.append(_case(rng, "drawn%02d" % n, random_table(rng, V, J), K, D, mean_n))
    return out


def model_of(case, eta=None):
    return Ilda(case["K"], case["alpha"], case["eta"] if eta is None else eta, case["features"], case["X"], case["lam0"])


# ------------------------------------------------------------------------------------------------------ helpers of the two test files
def dist(a, b, atol=0.0):
    """max over entries of (|a - b| - atol) / |b|: the smallest rtol with which assert_allclose(a, b, rtol, atol) passes."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    if a.size == 0:
        return 0.0
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(np.abs(a - b) <= atol, 0.0, (np.abs(a - b) - atol) / np.abs(b))
    return float(r.max())


def oracle_of(orc, c, eta=None, features=None, lam0=None):
    lam0 = c["lam0"] if lam0 is None else lam0
    return orc.IldaOracle(c["K"], c["alpha"], c["eta"] if eta is None else eta, c["features"] if features is None else features, c["X"],
                          lambda0=np.concatenate([l.ravel(order="F") for l in lam0]))


def heldout_docs(c):
    rng = np.random.Generator(np.random.PCG64([77, c["V"]]))
    X = corpus(rng, 25, c["V"], c["K"], c["mean_n"] // 2 + 5)
    X[3] = np.zeros((0, 2), dtype=np.int64)
    return X
