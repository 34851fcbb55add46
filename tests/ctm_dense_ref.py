"""Independent numpy restatement of what one fused CTM pass computes outside its LD_MMA solves, written from src/MMCTM.jl and
src/IMMCTM.jl of the reference (the line numbers below are those files'), NOT from oracle/ or the package, of which nothing is imported:
dense [D, V_m] count matrices, every sum in np.longdouble (`dt=LD`) or, for the unit of the GPU bounds, in float64 and index order
(`dt=np.float64`).  tests/test_ctm_dense_ref_cpu.py holds the C oracle to it, tests/test_ctm_dense_dispatch_gpu.py the device kernels
that run over rows of 16-bit counts (k_ctm_theta_dense<KMX, SL>, k_ctm_loglik_dense<KMX>; csrc/ctm_estep.cuh, csrc/ctm_mstep.cuh).

Within one pass fit! (MMCTM.jl:457-479) runs fitdoc! as ζ, θ, ν, λ and then μ, Σ, γ, props, ϕ, ll.  So after ONE pass from a state (λ, ν)
the test wrote, ζ depends only on that state, γ only on that λ and the starting Elnϕ -- neither on the solves -- and props / ll are functions
of the post-solve λ and the new γ, both of which can be read back.

Besides the restatement: `dense_build` (the two rules by which a handle takes the rows-of-counts kernels), `conditions` (what create asks
of a corpus for them), a count generator with exact presence control, the a-priori error bounds, and the fixed case table both files walk."""
import numpy as np
from scipy.special import digamma, polygamma

LD = np.longdouble
U = 2.0 ** -53                 # unit roundoff of float64
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble has no extended precision on this machine"

EXP_ULP = 0.506                # the table exp (ar_exp) against 40-digit mpmath, DESIGN.md section 2
LOG_ABS = 2.4e-15              # the table log (dev_log_tab), absolute, same place
DIGAMMA_ERR = 9e-16            # the device digamma, |err| / (|psi| + 1), same place
F = 4.0                        # another association of the same sums against the index-order one: the factor of test_ctm_gauss_gpu.py


# ---------------------------------------------------------------------------------------------------------- sums
def _sum(x, axis, dt):
    """Sum along `axis`: np.longdouble, or float64 in index order (one rounding per addition, as a literal loop)."""
    x = np.asarray(x, dtype=dt)
    if dt is LD or x.shape[axis] == 0:
        return x.sum(axis=axis)
    return np.add.accumulate(x, axis=axis).take(-1, axis=axis)


def _offsets(K):
    return np.concatenate([[0], np.cumsum(K)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------- the model's layouts
class Spec:
    """What defines a model: K, α, V (MMCTM) or features (IMMCTM; features[m]: V_m x I_m, 1-based values, J = column maxima), and the corpus
    X[d][m]: (W, 2) [term (1-based), count].  Flat layouts are the C ABI's: γ / Elnϕ of an MMCTM [m][k][v], of an IMMCTM [m][k][i][j]."""

    def __init__(self, K, alpha, V, X, features=None):
        self.K = [int(k) for k in K]; self.M = len(self.K); self.MK = int(sum(self.K)); self.koff = _offsets(self.K)
        self.X = X; self.D = len(X)
        self.features = None if features is None else [np.asarray(f, dtype=np.int64) for f in features]
        self.imm = features is not None
        if self.imm:
            self.V = [int(f.shape[0]) for f in self.features]
            self.I = [int(f.shape[1]) for f in self.features]
            self.J = [[int(j) for j in f.max(axis=0)] for f in self.features]                     # IMMCTM.jl:42
            self.alpha = [np.full(self.I[m], float(alpha[m])) if np.ndim(alpha[m]) == 0 else np.asarray(alpha[m], float) for m in range(self.M)]
            self.gsize = [self.K[m] * int(sum(self.J[m])) for m in range(self.M)]
        else:
            self.V = [int(v) for v in V]
            self.alpha = [float(a) for a in alpha]
            self.gsize = [self.K[m] * self.V[m] for m in range(self.M)]
        self.goff = _offsets(self.gsize)
        # dense counts: every listed row of a term adds (update_γ! and the ll both walk the rows, MMCTM.jl:230-240, :390-397)
        self.N = []
        for m in range(self.M):
            n = np.zeros((self.D, self.V[m]), dtype=np.int64)
            for d in range(self.D):
                x = np.asarray(X[d][m], dtype=np.int64).reshape(-1, 2)
                np.add.at(n[d], x[:, 0] - 1, x[:, 1])
            self.N.append(n)

    def unflatten(self, flat, m):
        """γ or Elnϕ of modality m from the flat layout: MMCTM [K_m, V_m]; IMMCTM list over features of [K_m, J_i]."""
        a = np.asarray(flat)[self.goff[m]:self.goff[m + 1]]
        if not self.imm:
            return a.reshape(self.K[m], self.V[m])
        a = a.reshape(self.K[m], int(sum(self.J[m])))
        jo = _offsets(self.J[m])
        return [a[:, jo[i]:jo[i + 1]] for i in range(self.I[m])]

    def flatten(self, per_m):
        out = []
        for m in range(self.M):
            out.append(np.concatenate(per_m[m], axis=1).ravel() if self.imm else np.asarray(per_m[m]).ravel())
        return np.concatenate(out)


# ---------------------------------------------------------------------------------------------------------- the restatement
def update_zeta(s, lam, nu, dt=LD):
    """update_ζ!, MMCTM.jl:172-181: ζ[d][m] = sum(exp.(λ[d][block m] .+ 0.5 ν[d][block m])) -> [D, M]."""
    lam = np.asarray(lam, dtype=dt); nu = np.asarray(nu, dtype=dt)
    e = np.exp(lam + dt(0.5) * nu)
    return np.stack([_sum(e[:, s.koff[m]:s.koff[m + 1]], 1, dt) for m in range(s.M)], axis=1)


def update_theta(s, lam, Elnphi_flat, m, dt=LD):
    """update_θ! for modality m and EVERY term (a document's θ columns are those of its terms), MMCTM.jl:183-198: exp(λ_k + Elnϕ_k[v]);
    IMMCTM.jl:152-172: exp(λ_k) Π_i exp(Elnϕ_k[i][feature_i(v)]); then ./= sum over k -> [D, K_m, V_m]."""
    lam = np.asarray(lam, dtype=dt)[:, s.koff[m]:s.koff[m + 1]]
    E = s.unflatten(Elnphi_flat, m)
    if s.imm:
        th = np.repeat(np.exp(lam)[:, :, None], s.V[m], axis=2)
        for i in range(s.I[m]):
            th = th * np.exp(E[i].astype(dt))[:, s.features[m][:, i] - 1][None, :, :]
    else:
        th = np.exp(lam[:, :, None] + E.astype(dt)[None, :, :])
    return th / _sum(th, 1, dt)[:, None, :]


def calculate_sumtheta(s, theta_m, m, dt=LD):
    """calculate_sumθ, MMCTM.jl:110-117: sum(θ[d][m] .* X[d][m][:, 2]', dims=2) -> [D, K_m]."""
    return _sum(theta_m * s.N[m].astype(dt)[:, None, :], 2, dt)


def update_gamma(s, thetas, dt=LD):
    """update_γ!, MMCTM.jl:224-242: γ[m][k][v] = α[m] + Σ_d θ[d][m][k, w] n; IMMCTM.jl:199-223: γ[m][k][i][feature_i(v)] gets the same
    addends.  -> list over m (MMCTM [K_m, V_m]; IMMCTM list over i of [K_m, J_i])."""
    out = []
    for m in range(s.M):
        nth = _sum(thetas[m] * s.N[m].astype(dt)[:, None, :], 0, dt)            # [K_m, V_m]: Nθ summed over the documents
        if not s.imm:
            out.append(dt(s.alpha[m]) + nth)
            continue
        gi = []
        for i in range(s.I[m]):
            g = np.full((s.K[m], s.J[m][i]), s.alpha[m][i], dtype=dt)
            for j in range(s.J[m][i]):
                sel = s.features[m][:, i] - 1 == j
                g[:, j] = g[:, j] + _sum(nth[:, sel], 1, dt)
            gi.append(g)
        out.append(gi)
    return out


def update_Elnphi(s, gamma, dt=LD):
    """update_Elnϕ!, MMCTM.jl:214-222 / IMMCTM.jl:188-197: digamma.(γ) .- digamma(sum(γ)), the sum over a topic's terms (feature values).
    digamma itself is scipy's float64 one for both `dt` (its error is part of `elnphi_bound`)."""
    def one(g):
        return digamma(np.asarray(g, dtype=np.float64)) - digamma(np.asarray(_sum(g, 1, dt), dtype=np.float64))[:, None]
    return [[one(g) for g in gm] if s.imm else one(gm) for gm in gamma]


def update_phi(s, gamma_flat, m, dt=LD):
    """update_ϕ!, MMCTM.jl:244-250: ϕ[m][k] = γ[m][k] ./ sum(γ[m][k]); for an IMMCTM what calculate_loglikelihoods forms, IMMCTM.jl:417-420
    with :376-378: Π_i γ[m][k][i][feature_i(v)] / sum(γ[m][k][i]) -> [K_m, V_m]."""
    g = s.unflatten(gamma_flat, m)
    if not s.imm:
        g = g.astype(dt)
        return g / _sum(g, 1, dt)[:, None]
    p = np.ones((s.K[m], s.V[m]), dtype=dt)
    for i in range(s.I[m]):
        gi = g[i].astype(dt)
        p = p * (gi / _sum(gi, 1, dt)[:, None])[:, s.features[m][:, i] - 1]
    return p


def update_props(s, lam, dt=LD):
    """update_props!, MMCTM.jl:145-154: exp.(η) ./ sum(exp.(η)) per modality block, as written (no maximum subtracted) -> [D, ΣK]."""
    e = np.exp(np.asarray(lam, dtype=dt))
    return np.concatenate([e[:, s.koff[m]:s.koff[m + 1]] / _sum(e[:, s.koff[m]:s.koff[m + 1]], 1, dt)[:, None] for m in range(s.M)], axis=1)


def calculate_loglikelihoods(s, props, gamma_flat, dt=LD):
    """calculate_loglikelihoods, MMCTM.jl:384-448 / IMMCTM.jl:362-428: per modality Σ_d [N_d > 0] Σ_w n log(Σ_k props_k ϕ_k[v]) / Σ_d N_d
    (a document's ll / N_d is multiplied by N_d again, :409-414) -> [M]."""
    out = np.zeros(s.M, dtype=dt)
    for m in range(s.M):
        phi = update_phi(s, gamma_flat, m, dt)
        pw = _sum(np.asarray(props, dtype=dt)[:, s.koff[m]:s.koff[m + 1], None] * phi[None, :, :], 1, dt)       # [D, V_m]
        n = s.N[m].astype(dt)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(s.N[m] > 0, n * np.log(pw), dt(0))                  # an unlisted term is no row of X
        out[m] = _sum(_sum(t, 1, dt), 0, dt) / dt(int(s.N[m].sum()))
    return out


def pass_from_state(s, lam, nu, Elnphi_flat, dt=LD):
    """What one pass makes of the written state without its solves: ζ [D, M], Σθ [D, ΣK], γ and Elnϕ (flat)."""
    thetas = [update_theta(s, lam, Elnphi_flat, m, dt) for m in range(s.M)]
    sumth = np.concatenate([calculate_sumtheta(s, thetas[m], m, dt) for m in range(s.M)], axis=1)
    gamma = update_gamma(s, thetas, dt)
    return dict(zeta=update_zeta(s, lam, nu, dt), sumth=sumth, gamma=s.flatten(gamma), Elnphi=s.flatten(update_Elnphi(s, gamma, dt)))


def after_solves(s, lam_post, gamma_flat, dt=LD):
    """props and ll of the state read back after the pass."""
    props = update_props(s, lam_post, dt)
    return dict(props=props, ll=calculate_loglikelihoods(s, props, gamma_flat, dt))


# ---------------------------------------------------------------------------------------------------------- a-priori bounds
# Every summand of ζ, the θ n statistics, Σθ and the softmax denominators is positive, so a float64 evaluation in ANY association is off
# by a relative γ_n = n u / (1 - n u) with n the number of roundings on the longest path to the result (Higham, Accuracy and Stability,
# sections 3.1 and 4.2; zeros added for padding lanes, slots and documents do not round).  The table exp is off by EXP_ULP ulp <= 2
# EXP_ULP u relative, and its argument carries one rounding: exp(x (1 + ε)) = exp(x) (1 + x ε).
_EXPR = 2.0 * EXP_ULP


def _gam(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U) + n * 2.0 ** -63           # + the np.longdouble reference's own roundings


def zeta_bound(s, lam, nu):
    """ζ_dm = Σ_k exp(λ_k + ν_k / 2): per term the rounding of the argument (|λ + ν/2| u) and the table exp, then K_m - 1 additions.
    Relative, [D, M]."""
    arg = np.abs(np.asarray(lam) + 0.5 * np.asarray(nu))
    return np.stack([_gam(_EXPR + arg[:, s.koff[m]:s.koff[m + 1]].max(axis=1) + s.K[m] - 1) for m in range(s.M)], axis=1)


def _theta_roundings(s, lam, Elnphi_flat, m):
    """Roundings of one θ_kv n_v of document d, [D]: a_k = exp(λ_k - max λ) (argument |λ_k - max| u, table exp), B_kv = exp(Elnϕ) (table
    exp; IMMCTM: the argument is a float64 sum of I_m table entries, (I_m - 1) Σ_i |Elnϕ_i| u), e_k = a_k B_kv (1), all of it once in the
    numerator and once in the denominator s = Σ_k e_k (K_m - 1 additions), 1 / s (1), n / s (1); e_k r enters the sums fused."""
    lam = np.asarray(lam)[:, s.koff[m]:s.koff[m + 1]]
    spread = lam.max(axis=1) - lam.min(axis=1)
    bextra = 0.0
    if s.imm and s.I[m] > 1:
        E = s.unflatten(Elnphi_flat, m)
        bextra = (s.I[m] - 1) * float(sum(np.abs(e).max() for e in E))
    de = 2.0 * _EXPR + spread + bextra + 1.0
    return 2.0 * de + s.K[m] + 1.0


def gamma_bound(s, lam, Elnphi_flat):
    """γ = α + Σ_d θ n: the worst document's term roundings plus one addition per document that has the term (per feature value: per
    document and term that has it).  Relative, flat like γ."""
    out = []
    for m in range(s.M):
        c = float(_theta_roundings(s, lam, Elnphi_flat, m).max())
        P = (s.N[m] > 0).sum(axis=0)                                             # [V_m] summands besides α
        if not s.imm:
            out.append(np.repeat(_gam(c + P)[None, :], s.K[m], axis=0))
            continue
        gi = []
        for i in range(s.I[m]):
            Pj = np.array([P[s.features[m][:, i] - 1 == j].sum() for j in range(s.J[m][i])])
            gi.append(np.repeat(_gam(c + Pj)[None, :], s.K[m], axis=0))
        out.append(gi)
    return s.flatten(out)


def sumtheta_bound(s, lam, Elnphi_flat):
    """Σθ_dk = Σ_v θ_kv n_v: the term's roundings (+ 2 where θ is stored and multiplied by n afterwards) plus one addition per listed term.
    Relative, [D, ΣK]."""
    out = []
    for m in range(s.M):
        c = _theta_roundings(s, lam, Elnphi_flat, m) + 2.0 + (s.N[m] > 0).sum(axis=1)
        out.append(np.repeat(_gam(c)[:, None], s.K[m], axis=1))
    return np.concatenate(out, axis=1)


def elnphi_bound(s, gamma_flat, gbound_flat):
    """Elnϕ = ψ(γ) - ψ(Σγ), absolute, flat: first order in the error of γ (ψ' γ times its relative bound; Σγ adds V_m - 1 additions), two
    digamma evaluations at DIGAMMA_ERR (|ψ| + 1) on the device and at 4 u (|ψ| + 1) in scipy's, one subtraction."""
    out = []
    for m in range(s.M):
        g = s.unflatten(gamma_flat, m); b = s.unflatten(gbound_flat, m)

        def one(g, b):
            S = g.sum(axis=1, keepdims=True)
            bS = (g * b).sum(axis=1, keepdims=True) / S + _gam(g.shape[1] - 1)
            e = polygamma(1, g) * g * b + polygamma(1, S) * S * bS
            e = e + (DIGAMMA_ERR + 4 * U) * (np.abs(digamma(g)) + np.abs(digamma(S)) + 2.0)
            return e + 2 * U * np.abs(digamma(g) - digamma(S))
        out.append([one(gi, bi) for gi, bi in zip(g, b)] if s.imm else one(g, b))
    return s.flatten(out)


def props_bound(s, lam_post):
    """props_k = exp(η_k - max) / Σ: the device's exp is the library's (1 ulp <= 2 u) on an argument with one rounding, numerator and
    denominator, K_m - 1 additions, one division.  Relative, [D, ΣK]."""
    out = []
    for m in range(s.M):
        x = np.asarray(lam_post)[:, s.koff[m]:s.koff[m + 1]]
        off = x.max(axis=1, keepdims=True) - x
        out.append(_gam((2.0 + off) + (2.0 + off.max(axis=1, keepdims=True)) + s.K[m]))
    return np.concatenate(out, axis=1)


def ll_bound(s, lam_post, gamma_flat, ll_ref):
    """ll_m, absolute, [M]: p = Σ_k props_k ϕ_kv carries props' bound, ϕ's (γ / Σγ: V_m roundings; IMMCTM Σ_i (J_i + 1)) and K_m fused
    additions; log adds LOG_ABS; the sum of the n log p (all of one sign) is off by its depth: a lane adds at most V_m of them, then one
    per document it meets, then the lanes, waves and blocks (64 more at the most, generously); one division by N_m."""
    pb = props_bound(s, lam_post)
    out = np.zeros(s.M)
    for m in range(s.M):
        dphi = float(s.V[m]) if not s.imm else float(sum(j + 1 for j in s.J[m]))
        dp = pb[:, s.koff[m]:s.koff[m + 1]].max(axis=1) + _gam(dphi + s.K[m])                  # [D]
        Nd = s.N[m].sum(axis=1).astype(np.float64)
        depth = s.V[m] + s.D + 64 + 1
        out[m] = float((Nd * (dp + LOG_ABS)).sum() / Nd.sum() + _gam(depth) * abs(float(ll_ref[m])))
    return out


def rel_gap(a, b):
    """max |a - b| / |b| over the entries (0 where both are 0)."""
    a = np.asarray(a, dtype=LD); b = np.asarray(b, dtype=LD)
    if a.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a == b, LD(0), np.abs(a - b) / np.abs(b))
    return float(r.max())


def ratio_rel(dev, ref, bound, unit):
    """Worst |dev - ref| / |ref| over the entries in units of max(a-priori bound, F unit); NaN / inf in `dev` -> inf."""
    dev = np.asarray(dev, dtype=np.float64)
    if not np.all(np.isfinite(dev)):
        return float("inf")
    ref = np.asarray(ref, dtype=LD).reshape(dev.shape); bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), dev.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dev.astype(LD) == ref, LD(0), np.abs(dev.astype(LD) - ref) / np.abs(ref))
    return float((r / np.maximum(bound, F * unit)).max()) if dev.size else 0.0


def ratio_abs(dev, ref, bound, unit):
    dev = np.asarray(dev, dtype=np.float64)
    if not np.all(np.isfinite(dev)):
        return float("inf")
    ref = np.asarray(ref, dtype=LD).reshape(dev.shape); bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), dev.shape)
    return float((np.abs(dev.astype(LD) - ref) / np.maximum(bound, F * unit)).max()) if dev.size else 0.0


class Reference:
    """The restatement of one written state, evaluated once: np.longdouble values, the a-priori bounds and the units (the gap of the float64
    index-order evaluation to the np.longdouble one).  `compare_*` return the worst ratio per quantity; a ratio <= 1 passes."""

    def __init__(self, s, lam, nu, Elnphi_flat):
        self.s, self.lam, self.nu, self.E0 = s, np.asarray(lam), np.asarray(nu), np.asarray(Elnphi_flat)
        self.ld = pass_from_state(s, lam, nu, Elnphi_flat, LD)
        f64 = pass_from_state(s, lam, nu, Elnphi_flat, np.float64)
        self.unit = {q: rel_gap(f64[q], self.ld[q]) for q in ("zeta", "sumth", "gamma")}
        self.unit["Elnphi"] = float(np.abs(f64["Elnphi"] - self.ld["Elnphi"]).max())
        self.bound = dict(zeta=zeta_bound(s, lam, nu), sumth=sumtheta_bound(s, lam, Elnphi_flat), gamma=gamma_bound(s, lam, Elnphi_flat))
        self.bound["Elnphi"] = elnphi_bound(s, np.asarray(self.ld["gamma"], dtype=np.float64), self.bound["gamma"])

    def compare_state(self, zeta, gamma, Elnphi, sumth=None, docs=None):
        r = dict(zeta=ratio_rel(np.reshape(zeta, (self.s.D, self.s.M)), self.ld["zeta"], self.bound["zeta"], self.unit["zeta"]),
                 gamma=ratio_rel(gamma, self.ld["gamma"], self.bound["gamma"], self.unit["gamma"]),
                 Elnphi=ratio_abs(Elnphi, self.ld["Elnphi"], self.bound["Elnphi"], self.unit["Elnphi"]))
        if sumth is not None:
            docs = np.arange(self.s.D) if docs is None else np.asarray(docs)
            r["sumth"] = ratio_rel(np.reshape(sumth, (len(docs), self.s.MK)), self.ld["sumth"][docs], self.bound["sumth"][docs], self.unit["sumth"])
        return r

    def compare_after(self, lam_post, gamma_dev, props, ll):
        """props and ll against the restatement of the λ and γ that were read back"""
        s = self.s
        lam_post = np.reshape(lam_post, (s.D, s.MK))
        ld = after_solves(s, lam_post, gamma_dev, LD); f64 = after_solves(s, lam_post, gamma_dev, np.float64)
        up = rel_gap(f64["props"], ld["props"]); ul = float(np.abs(f64["ll"] - ld["ll"]).max())
        r = dict(ll=ratio_abs(ll, ld["ll"], ll_bound(s, lam_post, gamma_dev, ld["ll"]), ul))
        if props is not None:         # (an IMMCTM has no props field, IMMCTM.jl:1-27: its ll forms them on the fly, :365)
            r["props"] = ratio_rel(np.reshape(props, (s.D, s.MK)), ld["props"], props_bound(s, lam_post), up)
        return r, dict(props=up, ll=ul)


# ---------------------------------------------------------------------------------------------------------- which build a handle takes
def dense_build(K, V):
    """The two rules of create: KMX from K_m (<= 8 -> 8, <= 10 -> 10, <= 16 -> 16), SL from V_m (<= 32 -> 2, <= 48 -> 3, <= 96 -> 6,
    <= 128 -> 8), admitted while KMX SL <= 64 (the statistics stay in registers).  -> (the (KMX, SL) of k_ctm_theta_dense per modality,
    the KMX of k_ctm_loglik_dense = the largest of them), or (None, None) where a modality has no build."""
    builds = []
    for k, v in zip(K, V):
        kmx = 8 if k <= 8 else 10 if k <= 10 else 16 if k <= 16 else 0
        sl = 2 if v <= 32 else 3 if v <= 48 else 6 if v <= 96 else 8 if v <= 128 else 0
        if kmx == 0 or sl == 0 or kmx * sl > 64:
            return None, None
        builds.append((kmx, sl))
    return builds, max(b[0] for b in builds)


THETA_BUILDS = ((8, 2), (8, 3), (8, 6), (8, 8), (10, 2), (10, 3), (10, 6), (16, 2), (16, 3))
LL_BUILDS = (8, 10, 16)
CONDITIONS = ("density", "no_duplicate", "count16", "K16", "V128", "registers")


def conditions(K, V, X):
    """What create asks of a corpus before a handle runs over rows of counts, each as a bool: at least half of the D ΣV cells listed
    (2 listed >= cells), no document lists a term twice, every count < 65,536, K_m <= 16, V_m <= 128, KMX SL <= 64."""
    D, M = len(X), len(K)
    listed = sum(np.asarray(X[d][m]).reshape(-1, 2).shape[0] for d in range(D) for m in range(M))
    dup = any(len(set(np.asarray(X[d][m]).reshape(-1, 2)[:, 0].tolist())) != np.asarray(X[d][m]).reshape(-1, 2).shape[0] for d in range(D) for m in range(M))
    cmax = max([int(np.asarray(X[d][m]).reshape(-1, 2)[:, 1].max()) for d in range(D) for m in range(M) if np.asarray(X[d][m]).size] + [0])
    k16, v128 = all(k <= 16 for k in K), all(v <= 128 for v in V)
    regs = True
    if k16 and v128:
        regs = dense_build(K, V)[0] is not None
    return dict(density=2 * listed >= D * int(sum(V)), no_duplicate=not dup, count16=cmax < 65536, K16=k16, V128=v128, registers=regs)


# ---------------------------------------------------------------------------------------------------------- corpora and states
def draw_counts(rng, D, V, listed, mean=12, empty_docs=(), absent_terms=()):
    """[D, V] counts with EXACTLY `listed` nonzero cells, drawn among the cells outside `empty_docs` (rows) and `absent_terms` (columns);
    a listed cell holds 1 + Poisson(mean)."""
    ok = np.ones((D, V), dtype=bool)
    ok[list(empty_docs), :] = False
    ok[:, list(absent_terms)] = False
    cells = np.flatnonzero(ok.ravel())
    assert 0 <= listed <= cells.size, (listed, cells.size)
    n = np.zeros(D * V, dtype=np.int64)
    pick = rng.choice(cells, size=listed, replace=False)
    n[pick] = 1 + rng.poisson(mean, size=listed)
    return n.reshape(D, V)


def rows_of(rng, n):
    """[W, 2] rows [term (1-based), count] of one document's nonzero counts, in drawn order (nothing may depend on sorted terms)."""
    idx = rng.permutation(np.flatnonzero(n))
    return np.stack([idx + 1, n[idx]], axis=1).astype(np.int64).reshape(-1, 2)


def state(rng, D, MK):
    """(λ, ν) to write: λ spread over ±6 (the subtraction of the maximum matters), ν in 0.05 ... 2."""
    return rng.uniform(-6.0, 6.0, size=(D, MK)), rng.uniform(0.05, 2.0, size=(D, MK))


SNV3 = np.array([[t // 16 + 1, (t // 4) % 4 + 1, t % 4 + 1] for t in range(96)])


def _case(name, group, K, V, D, dens=0.8, features=None, tune=None, seed=0, edit=None, dense=True, violates=None, mean=12, empty=None, absent=None):
    """One case: corpus with exactly round(dens D V_m) listed cells per modality (dens: one number or one per modality), γ0 drawn like the
    reference's constructor (integers 1 ... 100), the state to write.  `edit(X, N)` changes single rows afterwards."""
    rng = np.random.Generator(np.random.PCG64([20261019, seed]))
    M = len(K)
    dens = [dens] * M if np.ndim(dens) == 0 else list(dens)
    empty = empty or {}; absent = absent or {}
    N = [draw_counts(rng, D, V[m], int(round(dens[m] * (D - len(empty.get(m, ()))) * (V[m] - len(absent.get(m, ()))))), mean,
                     empty.get(m, ()), absent.get(m, ())) for m in range(M)]
    X = [[rows_of(rng, N[m][d]) for m in range(M)] for d in range(D)]
    if edit is not None:
        edit(X)
    if features is None:
        g0 = [rng.integers(1, 101, size=(K[m], V[m])).astype(np.float64) for m in range(M)]
    else:
        g0 = rng.integers(1, 101, size=sum(K[m] * int(np.asarray(features[m]).max(axis=0).sum()) for m in range(M))).astype(np.float64)
    lam, nu = state(rng, D, int(sum(K)))
    return dict(name=name, group=group, K=list(K), V=list(V), D=D, X=X, features=features, g0=g0, lam=lam, nu=nu, alpha=[0.1] * M,
                tune=dict(tune or {}), dense=dense, violates=violates)


def _add_row(X, d, m, term, count):
    X[d][m] = np.vstack([X[d][m], [[term, count]]]).astype(np.int64)


def _set_count(X, d, m, term, count):
    """term (1-based) of document d gets `count`: its row is changed, or added where the document did not list it"""
    x = X[d][m]
    hit = np.flatnonzero(x[:, 0] == term)
    if hit.size:
        x[hit[0], 1] = count
    else:
        _add_row(X, d, m, term, count)


def _drop_rows(X, m, k):
    """k listed rows fewer in modality m (the last row of the first documents that have more than one)"""
    for d in range(len(X)):
        if k == 0:
            break
        if X[d][m].shape[0] > 1:
            X[d][m] = X[d][m][:-1]
            k -= 1
    assert k == 0


# grid edges.  k_ctm_theta_dense: 8 waves x 4 document groups per block, wave w of block b starts at document (8 b + w) 4 and advances by
# stride = gridDim.x 32.  k_ctm_loglik_dense: 4 waves per block, grid_s = min(ceil(D / 4), 4 CUs - 1) blocks, nslots = 4 grid_s waves,
# wave slot s takes documents (s + step nslots) 4 ...: geometry_cus = 1 -> 3 blocks, nslots 4 = 48 documents per step; geometry_cus = 4 ->
# at most 15 blocks, 240 documents per step.
GRID_EDGES = (
    # (D, grid_blocks, geometry_cus)
    (1, 1, 1),      # theta: wave 0 holds 1 document of its first group, waves 1-7 none; ll: grid_s = 1, slot 0 one document, slots 1-3 none
    (3, 2, 4),      # theta: block 1 has no document at all (starts at 32); wave 0 of block 0 three lanes of groups short
    (4, 1, 4),      # theta: exactly one full wave step of wave 0; ll: one slot, full
    (5, 1, 1),      # theta: wave 1 with one document; ll: grid_s = 2, slot 1 with one document, slots 2-7 none
    (31, 1, 1),     # theta: stride 32, one step, the last group of wave 7 one document short; ll: grid_s 3, 12 slots, 48 per step, slots 8-11 none
    (32, 1, 4),     # theta: one step exactly full, the next step (base + 32 >= D) beyond D for every wave; ll: grid_s 8, 32 slots, 8 full
    (33, 1, 1),     # theta: wave 0 takes a second step with one document, the next step of waves 1-7 is entirely beyond D; ll: 48 per step, one step
    (33, 2, 4),     # theta: stride 64, block 1 wave 0 holds document 32 alone; ll: grid_s 9, slot 8 one document
    (64, 2, 1),     # theta: two blocks, one full step each, nothing beyond; ll: 48 per step: slots 0-3 take a second step (48 ... 63), 4-11 do not
    (65, 1, 1),     # theta: stride 32: wave 0 three steps, the third with one document (64); ll: second step slots 0-3 full, slot 4 one document
    (65, 2, 4),     # theta: stride 64: block 0 wave 0 a second step with one document; ll: grid_s 15, 60 slots, 240 per step, slots 17-59 none
    (129, 1, 1),    # theta: stride 32: five steps for wave 0, the fifth one document; ll: three steps, slot 8's third holds document 128 alone
    (129, 2, 1),    # theta: stride 64: three steps for block 0 wave 0, the third one document, the next step of block 1 beyond D
)


def _grid_case(D, gb, cus, seed):
    return _case("grid_D%d_b%d_c%d" % (D, gb, cus), "grid", [2, 9], [17, 40], D, dens=0.75, tune=dict(grid_blocks=gb, geometry_cus=cus), seed=seed)


def _rows_edit(X):
    # modality 0 (V = 48, three slots, fully present): 65,535 in slot 2 (term 40 -> 0-based 39: 39 >> 4 = 2, even) and slot 1 (term 20 -> 19 >> 4 = 1, odd)
    _set_count(X, 2, 0, 40, 65535); _set_count(X, 3, 0, 20, 65535)
    # modality 1 (V = 24, two slots): 65,535 in an odd slot (term 18 -> 17 >> 4 = 1) and in an even one (term 4 -> 3 >> 4 = 0)
    _set_count(X, 2, 1, 18, 65535); _set_count(X, 3, 1, 4, 65535)
    # a listed entry with count 0 (term 9 of document 6, dropped from the draw first)
    X[6][1] = X[6][1][X[6][1][:, 0] != 9]
    _add_row(X, 6, 1, 9, 0)


def _c65536(X):
    _set_count(X, 4, 0, 18, 65536)


def _dup(X):
    _add_row(X, 3, 0, int(X[3][0][0, 0]), 5)


_HALF = dict(K=[5], V=[24], D=40)           # 960 cells: 480 listed is exactly half


def cases():
    """The fixed case table, by group: "build" (every θ build with K and V at both ends of its class), "mixed" (the ll build's KMX above a
    modality's own, M = 8, the IMMCTM), "rows", "refused" (tdense = 0: each violates exactly one of CONDITIONS), "half", "grid"."""
    c = []
    sd = iter(range(1000))
    # ---- builds: K in {1, 2, 8} {9, 10} {11, 13, 15, 16} x V in {1, 15, 16, 17, 32} {33, 48} {49, 96} {97, 128}
    c.append(_case("b8x2", "build", [1, 2, 8, 8, 2], [1, 15, 16, 17, 32], 37, dens=[1.0, 0.7, 0.8, 0.7, 0.9], seed=next(sd)))
    c.append(_case("b8x3", "build", [1, 8, 2], [33, 48, 48], 35, seed=next(sd)))
    c.append(_case("b8x6", "build", [2, 8, 1], [49, 96, 96], 34, seed=next(sd)))
    c.append(_case("b8x8", "build", [1, 8, 2], [97, 128, 128], 33, seed=next(sd)))
    c.append(_case("b10x2", "build", [9, 10, 9, 10, 9], [1, 15, 16, 17, 32], 37, dens=[1.0, 0.7, 0.8, 0.7, 0.9], seed=next(sd)))
    c.append(_case("b10x3", "build", [9, 10], [33, 48], 35, seed=next(sd)))
    c.append(_case("b10x6", "build", [10, 9], [49, 96], 34, seed=next(sd)))
    c.append(_case("b16x2a", "build", [11, 16, 13], [1, 32, 15], 37, dens=[1.0, 0.8, 0.7], seed=next(sd)))
    c.append(_case("b16x2b", "build", [13, 15, 16], [16, 17, 15], 35, seed=next(sd)))
    c.append(_case("b16x3", "build", [11, 16, 13, 15], [33, 48, 48, 33], 34, seed=next(sd)))
    # ---- the ll build's KMX above a modality's own; M = 8; the IMMCTM over the SNV3 features
    c.append(_case("mix2_16", "mixed", [2, 16], [40, 24], 45, seed=next(sd)))
    c.append(_case("mix8_9", "mixed", [8, 9], [96, 17], 45, seed=next(sd)))
    c.append(_case("mix1_10_11", "mixed", [1, 10, 11], [20, 96, 48], 45, seed=next(sd)))
    c.append(_case("M8", "mixed", [1, 2, 3, 4, 5, 6, 7, 8], [5, 16, 17, 31, 32, 33, 48, 20], 41, seed=next(sd)))
    c.append(_case("imm_snv3", "mixed", [10], [96], 61, dens=0.7, features=[SNV3], mean=20, seed=next(sd)))
    # ---- rows: documents empty in one modality (1, 8) and in all (5), a term no document has (term 8 of modality 1, 0-based 7), a listed
    # count 0, 65,535 in odd and even slots, SL = 3 with V = 48 fully present (slot 3 of every lane is padding)
    c.append(_case("rows", "rows", [5, 4], [48, 24], 37, dens=[1.0, 0.8], empty={0: (5,), 1: (1, 5, 8)}, absent={1: (7,)}, edit=_rows_edit, seed=next(sd)))
    # ---- refusals (tdense = 0, the slab kernels), each one condition away from a dense handle
    c.append(_case("c65536", "refused", [5, 4], [40, 24], 37, edit=_c65536, dense=False, violates="count16", seed=next(sd)))
    c.append(_case("K17", "refused", [17, 4], [40, 24], 37, dense=False, violates="K16", seed=next(sd)))
    c.append(_case("V129", "refused", [5, 4], [129, 24], 37, dense=False, violates="V128", seed=next(sd)))
    c.append(_case("dup", "refused", [5, 4], [40, 24], 37, edit=_dup, dense=False, violates="no_duplicate", seed=next(sd)))
    c.append(_case("half_minus1", "refused", dens=0.5, edit=lambda X: _drop_rows(X, 0, 1), dense=False, violates="density", seed=next(sd), **_HALF))
    c.append(_case("K9_V97", "refused", [9], [97], 33, dense=False, violates="registers", seed=next(sd)))       # (10, 8): 80 statistics
    c.append(_case("K11_V49", "refused", [11], [49], 33, dense=False, violates="registers", seed=next(sd)))     # (16, 6): 96
    # ---- density at exactly half: dense
    c.append(_case("half", "half", dens=0.5, seed=next(sd), **_HALF))
    # ---- grid edges
    for D, gb, cus in GRID_EDGES:
        c.append(_grid_case(D, gb, cus, next(sd)))
    return c


def spec_of(c):
    return Spec(c["K"], c["alpha"], c["V"], c["X"], features=c["features"])


def heldout_docs(c, D=29):
    """Held-out documents for case c, dense like it (85 % of the cells listed), one of them empty."""
    rng = np.random.Generator(np.random.PCG64([77, c["D"]]))
    N = [draw_counts(rng, D, v, int(round(0.85 * (D - 1) * v)), 10, empty_docs=(4,)) for v in c["V"]]
    return [[rows_of(rng, N[m][d]) for m in range(len(c["V"]))] for d in range(D)]
