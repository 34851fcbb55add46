"""Independent restatement of the seven ELBO terms of LDA, ILDA, MMCTM and IMMCTM, written from the formulas of the reference
(src/LDA.jl:114-172, src/ILDA.jl:132-207, src/MMCTM.jl:264-370, src/IMMCTM.jl:247-262 and :316-330; the line numbers below are those
files'), NOT from oracle/ or the package, of which nothing is imported.  Plain numpy in np.longdouble, lgamma from mpmath at 40 digits.

The ELBO is a pure function of the state a handle holds, and every input can be written and read back.  So `lda_terms` / `ctm_terms`
take a *state* (a dict of arrays in the flat layouts of include/mmmusig.h) and return, per term and in the order of
`calculate_elbo(..., terms=True)`,

    value   the np.longdouble value,
    A       Σ |summand|, the scale an absolute bound needs (ElnQθ and ElnQϕ pass through zero),
    f64     the same term evaluated in float64 in index order (the "unit" run: |f64 - value| measures the reference, not the device).

`bound(terms, n)` is max(γ_n A, F |f64 - value|) with γ_n = n u / (1 - n u), u = 2^-53, F = 4 (the margin of ctm_dense_ref.py: library
exp, log and lgamma are a few units each); `lda_roundings` / `ctm_roundings` derive n, the number of roundings on the longest path of a
term through the device kernels, from the sizes of a case.  No accuracy figure is assumed for the device's lgamma, log or exp.

Also here: the case tables both test files walk, `lda_state` / `ctm_state` that draw a WRITTEN state -- fields deliberately not
consistent with one another (γ does not follow from ϕ, ζ not from λ and ν), so that each term depends on its own inputs only and a
swapped pointer shows -- with values at the edges the kernels care about, and the arithmetic by which a case reaches a kernel."""
import collections
import math

import mpmath
import numpy as np

import ctm_dense_ref as CR

LD = np.longdouble
U = 2.0 ** -53
F = 4.0
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble has no extended precision on this machine"

LDA_TERMS = ("ElnPβ", "ElnPθ", "ElnPZ", "ElnPX", "ElnQβ", "ElnQθ", "ElnQZ")
CTM_TERMS = ("ElnPϕ", "ElnPη", "ElnPZ", "ElnPX", "ElnQϕ", "ElnQη", "ElnQZ")

Terms = collections.namedtuple("Terms", "value A f64")


# ---------------------------------------------------------------------------------------------------------- arithmetic
def _mp(x):
    """np.longdouble (or float) -> mpf without losing the low bits"""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(LD(x) - LD(hi)))


def _ld(m):
    hi = float(m)
    return LD(hi) + LD(float(m - hi))


def lgamma(x, dt=LD):
    """lgamma of every entry: dt = LD -> mpmath at 40 digits, rounded to np.longdouble; dt = float64 -> the C library's."""
    x = np.asarray(x)
    if dt is not LD:
        return np.array([math.lgamma(float(v)) for v in x.ravel()], dtype=np.float64).reshape(x.shape)
    out = np.empty(x.shape, dtype=LD)
    with mpmath.workdps(40):
        flat = out.reshape(-1)
        for i, v in enumerate(x.ravel()):
            flat[i] = _ld(mpmath.loggamma(_mp(v)))
    return out


def _tot(x, dt):
    """Σ of every entry: np.longdouble, or float64 in index order (one rounding per addition, as a literal loop)."""
    x = np.asarray(x, dtype=dt).ravel()
    if x.size == 0:
        return dt(0)
    return x.sum() if dt is LD else np.add.accumulate(x)[-1]


def _abs(x):
    return float(np.abs(np.asarray(x, dtype=np.float64)).sum())


def _xlogx(p, dt):
    """log(p ^ p) with 0^0 = 1 (LDA.jl:157, MMCTM.jl:365)"""
    p = np.asarray(p, dtype=dt)
    return np.where(p > 0, p * np.log(np.where(p > 0, p, dt(1))), dt(0))


def gam(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def bound(t, n):
    """max(γ_n A_t, F unit_t) per term, absolute"""
    unit = np.abs((np.asarray(t.f64, dtype=LD) - t.value).astype(np.float64))
    return np.maximum(gam(n) * np.asarray(t.A), F * unit)


def ratios(dev, t, n, extra=None):
    """|dev - value| / bound per term; `extra`: an absolute allowance added to the bound (the error of a θ or ϕ the device formed).
    A bound of exactly 0 (an empty sum) demands equality."""
    dev = np.asarray(dev, dtype=np.float64)
    if not np.all(np.isfinite(dev)):
        return np.full(7, np.inf)
    b = bound(t, n) + (0.0 if extra is None else np.asarray(extra, dtype=np.float64))
    gap = np.abs(dev.astype(LD) - t.value).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(gap == 0.0, 0.0, gap / b)


with mpmath.workdps(40):
    L2PI_LD = _ld(mpmath.log(2 * mpmath.pi))


def total(t):
    v = t.value
    return v[0] + v[1] + v[2] + v[3] - v[4] - v[5] - v[6]


def cholesky_logdet(S, dt):
    """log det of a symmetric positive definite matrix by Cholesky in `dt` (numpy's slogdet is float64 only)"""
    A = np.array(S, dtype=dt)
    n = A.shape[0]
    ld = dt(0)
    for j in range(n):
        piv = np.sqrt(A[j, j])
        ld = ld + dt(2) * np.log(piv)
        A[j:, j] = A[j:, j] / piv
        if j + 1 < n:
            A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - np.outer(A[j + 1:, j], A[j + 1:, j])
    return ld


# ---------------------------------------------------------------------------------------------------------- LDA / ILDA
def _lda_eval(st, dt):
    """The seven terms of an LDA (ILDA when st has `features`) state in dtype `dt`, and Σ |summand| of each.
    st: K, V, D, alpha, eta (scalar; ILDA: [I]), X[d] (W_d x 2, 1-based terms), lam / Elnbeta [V, K] (ILDA: lists of [J_i, K]),
    gamma / Elntheta [K, D], phi [nnz, K] (document blocks one after the other; np.longdouble allowed)."""
    K, V, D = st["K"], st["V"], st["D"]
    ilda = st.get("features") is not None
    v = [dt(0)] * 7; A = [0.0] * 7
    al = dt(st["alpha"])
    Elnth = np.asarray(st["Elntheta"], dtype=dt); gamma = np.asarray(st["gamma"], dtype=dt)

    def dirichlet_q(lam, Eln):
        """Σ lgamma(λ) - Σ_k lgamma(Σ_v λ) - Σ (λ - 1) Elnβ over a [n, K] table (LDA.jl:142-146); columns are the Dirichlets"""
        lam = np.asarray(lam, dtype=dt); Eln = np.asarray(Eln, dtype=dt)
        a = lgamma(lam, dt); cs = np.array([_tot(lam[:, k], dt) for k in range(lam.shape[1])], dtype=dt)
        b = lgamma(cs, dt); c = (lam - dt(1)) * Eln
        return _tot(a, dt) - _tot(b, dt) - _tot(c, dt), _abs(a) + _abs(b) + _abs(c)

    if ilda:
        feats = np.asarray(st["features"], dtype=np.int64); I = feats.shape[1]
        J = [int(j) for j in feats.max(axis=0)]; eta = np.asarray(st["eta"], dtype=dt)
        for i in range(I):                                                                    # ILDA.jl:132-141
            c = dt(K) * (lgamma(dt(J[i]) * eta[i], dt) - dt(J[i]) * lgamma(eta[i], dt))
            s = (eta[i] - dt(1)) * _tot(st["Elnbeta"][i], dt)
            v[0] = v[0] + c + s
            A[0] += K * (abs(float(lgamma(dt(J[i]) * eta[i], dt))) + J[i] * abs(float(lgamma(eta[i], dt)))) + abs(float(eta[i]) - 1) * _abs(st["Elnbeta"][i])
        # ILDA.jl:174-181: `lnq =` inside the loop over features keeps the LAST feature only; the device reproduces that on purpose
        v[4], A[4] = dirichlet_q(st["lam"][I - 1], st["Elnbeta"][I - 1])
        Eeff = sum(np.asarray(st["Elnbeta"][i], dtype=dt)[feats[:, i] - 1, :] for i in range(I))   # [V, K]   ILDA.jl:157-172
    else:
        eta = dt(st["eta"])
        lv, le = lgamma(dt(V) * eta, dt), lgamma(eta, dt)
        v[0] = dt(K) * (lv - dt(V) * le) + (eta - dt(1)) * _tot(st["Elnbeta"], dt)            # LDA.jl:114-118
        A[0] = K * (abs(float(lv)) + V * abs(float(le))) + abs(float(eta) - 1) * _abs(st["Elnbeta"])
        v[4], A[4] = dirichlet_q(st["lam"], st["Elnbeta"])
        Eeff = np.asarray(st["Elnbeta"], dtype=dt)
    lk, la = lgamma(dt(K) * al, dt), lgamma(al, dt)
    v[1] = dt(D) * (lk - dt(K) * la) + (al - dt(1)) * _tot(Elnth, dt)                         # LDA.jl:120-124
    A[1] = D * (abs(float(lk)) + K * abs(float(la))) + abs(float(al) - 1) * _abs(Elnth)
    phi = np.asarray(st["phi"], dtype=dt)
    e = 0
    for d in range(D):
        x = np.asarray(st["X"][d], dtype=np.int64).reshape(-1, 2)
        W = x.shape[0]
        p = phi[e:e + W]; n = x[:, 1].astype(dt)[:, None]; e += W
        z = p * Elnth[:, d][None, :] * n                                                      # LDA.jl:126-132
        xx = p * Eeff[x[:, 0] - 1, :] * n                                                     # LDA.jl:134-140
        q = _xlogx(p, dt)                                                                     # LDA.jl:154-160
        v[2] = v[2] + _tot(z, dt); v[3] = v[3] + _tot(xx, dt); v[6] = v[6] + _tot(q, dt)
        A[2] += _abs(z); A[3] += _abs(xx); A[6] += _abs(q)
    a = lgamma(gamma, dt); cs = np.array([_tot(gamma[:, d], dt) for d in range(D)], dtype=dt)   # LDA.jl:148-152
    b = lgamma(cs, dt); c = (gamma - dt(1)) * Elnth
    v[5] = _tot(a, dt) - _tot(b, dt) - _tot(c, dt); A[5] = _abs(a) + _abs(b) + _abs(c)
    return np.array(v, dtype=dt), np.array(A)


def lda_terms(st):
    v, A = _lda_eval(st, LD)
    f, _ = _lda_eval(st, np.float64)
    return Terms(v, A, f)


def lda_grid_s(D, cus):
    """blocks of 4 waves of the LDA stage kernels (lda_create_impl): min(ceil(D / 4), 4 CUs') at least 1"""
    return max(1, min((D + 3) // 4, 4 * cus))


def lda_roundings(K, V, D, Wmax, cus=256, I=0, Jmax=0):
    """n per term: the roundings on the longest path through k_lda_elbo_docs(_big) / k_lda_elbo_topics / k_ilda_elbo_topics, k_sum_columns
    and lda_elbo_finish.  A library call (lgamma, log) counts as one rounding.
      tail    a document's five values: 6 butterfly steps, one addition per document step of the wave, 3 for the block's 4 waves, then
              k_sum_columns (ceil(grid_s / 64) additions per lane + 6 butterfly steps)
      tokens  a lane meets ceil(W / 64) listed terms, K products each: ϕ Elnθ n is 2 roundings + 1 addition, ϕ log ϕ the same
      slots   K > 64: lane l holds topics l + 64 s, one addition per slot"""
    gs = lda_grid_s(D, cus)
    steps = -(-D // (gs * 4)); tok = -(-Wmax // 64); slots = -(-K // 64)
    tail = 6 + steps + 3 + (-(-gs // 64)) + 6
    rows = -(-(Jmax if I else V) // 256)
    n = np.zeros(7)
    # ElnPβ: a thread adds K rows Elnβ values (ILDA: per feature), block_sum_256 (6 + 3), host: V η, 2 lgamma, V lgamma, -, K (..), η - 1, *, +
    n[0] = K * rows + 9 + 8 + (3 * I + 6 * I if I else 0)
    n[1] = slots + tail + 8                       # Σ Elnθ over the slots, the tail; host as ElnPβ
    n[2] = 3 * tok * K + tail
    n[3] = 3 * tok * K + tail + max(I - 1, 0)     # ILDA: the effective table is a float64 sum of I entries
    # ElnQβ per topic: rows x (lgamma, λ - 1, * Elnβ, -, +), block sum 9, Σλ (rows + 9) into lgamma (1), -, then one addition per topic
    n[4] = 5 * rows + 9 + rows + 9 + 2 + K
    n[5] = 5 * slots + 6 + (slots + 6 + 1) + 1 + (tail - 6)
    n[6] = 3 * tok * K + tail
    return n


def phi_roundings(Elntheta, Elnbeta, K):
    """Relative error of a ϕ the device forms as exp(Elnθ) exp(Elnβ) / Σ_k (LDA.jl:69-76) in roundings: as ctm_dense_ref._theta_roundings
    (the arguments carry one rounding each, |x| u after exp; two table exp; the product; numerator and denominator; K - 1 additions; the
    division)."""
    de = 2.0 * CR._EXPR + float(np.abs(Elntheta).max()) + float(np.abs(Elnbeta).max()) + 1.0
    return 2.0 * de + K + 1.0


def lda_phi(X, Elntheta, Elnbeta):
    """update_ϕ! (LDA.jl:69-76) in np.longdouble, NOT rounded: [nnz, K]"""
    out = []
    Elntheta = np.asarray(Elntheta, dtype=LD); Elnbeta = np.asarray(Elnbeta, dtype=LD)
    for d, x in enumerate(X):
        x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
        a = Elntheta[:, d][None, :] + Elnbeta[x[:, 0] - 1, :]
        e = np.exp(a - a.max(axis=1, keepdims=True))
        out.append(e / e.sum(axis=1, keepdims=True))
    K = Elntheta.shape[0]
    return np.concatenate(out, axis=0) if out else np.zeros((0, K), dtype=LD)


def stale_allowance(t, eps, qz_scale):
    """What an error of relative size eps in θ (ϕ) adds to the bounds: eps A for the terms linear in it (ElnPZ, ElnPX), eps Σ n |p| (|log p|
    + 1) for ElnQZ."""
    out = np.zeros(7)
    out[2] = eps * t.A[2]; out[3] = eps * t.A[3]; out[6] = eps * qz_scale
    return out


# ---------------------------------------------------------------------------------------------------------- MMCTM / IMMCTM
class CtmLayout:
    """The flat layouts of a CTM state: K, V (IMMCTM: features[m] V_m x I_m, 1-based), X[d][m]."""

    def __init__(self, K, V, X, features=None):
        self.s = CR.Spec(K, [0.0] * len(K), V, X, features=features)          # layouts only (α travels with the state)
        s = self.s
        self.K, self.M, self.MK, self.D, self.V, self.imm = s.K, s.M, s.MK, s.D, s.V, s.imm
        self.W = np.array([[np.asarray(X[d][m]).reshape(-1, 2).shape[0] for m in range(s.M)] for d in range(s.D)], dtype=np.int64).reshape(s.D, s.M)
        self.nnz = self.W.sum(axis=0) if s.D else np.zeros(s.M, dtype=np.int64)
        self.toff = CR._offsets([int(self.nnz[m]) * s.K[m] for m in range(s.M)])
        self.nalpha = int(sum(s.I)) if s.imm else s.M

    def theta_dm(self, theta, d, m):
        """[W_dm, K_m] block of a flat θ"""
        e0 = int(self.W[:d, m].sum()); W = int(self.W[d, m]); Km = self.K[m]
        return np.asarray(theta)[self.toff[m] + e0 * Km:self.toff[m] + (e0 + W) * Km].reshape(W, Km)

    def effective(self, Elnphi, m, dt):
        """[K_m, V_m] table Σ_i Elnϕ[m][k][i][f_vi] that ElnPX walks (IMMCTM.jl:296-314); an MMCTM's is Elnϕ itself"""
        E = self.s.unflatten(Elnphi, m)
        if not self.imm:
            return np.asarray(E, dtype=dt)
        f = self.s.features[m]
        return sum(np.asarray(E[i], dtype=dt)[:, f[:, i] - 1] for i in range(self.s.I[m]))


def theta_from(lay, lam, Elnphi, dt=LD):
    """update_θ! of every document from (λ, Elnϕ) in np.longdouble (or float64 in index order), NOT rounded, in the flat layout (MMCTM.jl:183-198, IMMCTM.jl:152-172;
    the restatement of ctm_dense_ref.py, which forms θ for every term, read at the listed ones)."""
    out = []
    lam = np.reshape(lam, (lay.D, lay.MK))
    for m in range(lay.M):
        th = CR.update_theta(lay.s, lam, Elnphi, m, dt)                     # [D, K_m, V_m]
        for d in range(lay.D):
            x = np.asarray(lay.s.X[d][m], dtype=np.int64).reshape(-1, 2)
            out.append(th[d][:, x[:, 0] - 1].T.ravel())
    return np.concatenate(out) if out else np.zeros(0, dtype=dt)


def theta_roundings(lay, lam, Elnphi):
    lam = np.reshape(lam, (lay.D, lay.MK))
    return max(float(CR._theta_roundings(lay.s, lam, Elnphi, m).max()) if lay.D else 0.0 for m in range(lay.M))


def _ctm_eval(lay, st, dt):
    """st: alpha (flat: [M], IMMCTM [Σ I_m]), mu [MK], invSigma [MK, MK], gamma / Elnphi (flat), lam / nu [D, MK], zeta [D, M], theta (flat)."""
    s = lay.s; M, MK, D = lay.M, lay.MK, lay.D
    v = [dt(0)] * 7; A = [0.0] * 7
    alpha = np.asarray(st["alpha"], dtype=dt)
    ao = 0
    for m in range(M):                                                         # MMCTM.jl:271-284 / :338-350, IMMCTM.jl:247-262 / :316-330
        G = s.unflatten(st["gamma"], m); E = s.unflatten(st["Elnphi"], m)
        blocks = [(G[i], E[i], alpha[ao + i]) for i in range(s.I[m])] if lay.imm else [(G, E, alpha[m])]
        ao += s.I[m] if lay.imm else 0
        for k in range(s.K[m]):
            for g, e, al in blocks:                                            # one Dirichlet per (m, k[, i])
                g = np.asarray(g[k], dtype=dt); e = np.asarray(e[k], dtype=dt); n = g.shape[0]
                la, ln = lgamma(al, dt), lgamma(dt(n) * al, dt)
                se = _tot(e, dt)
                v[0] = v[0] + (-(dt(n) * la - ln) + (al - dt(1)) * se)         # -logmvbeta(fill(α, n)) + (α - 1) Σ Elnϕ
                A[0] += n * abs(float(la)) + abs(float(ln)) + abs(float(al) - 1) * _abs(e)
                lg = lgamma(g, dt); ls = lgamma(_tot(g, dt), dt); ge = (g - dt(1)) * e
                v[4] = v[4] + (-(_tot(lg, dt) - ls) + _tot(ge, dt))            # -logmvbeta(γ) + Σ (γ - 1) Elnϕ
                A[4] += _abs(lg) + abs(float(ls)) + _abs(ge)
    S = np.asarray(st["invSigma"], dtype=dt).reshape(MK, MK); mu = np.asarray(st["mu"], dtype=dt)
    lam = np.asarray(st["lam"], dtype=dt).reshape(D, MK); nu = np.asarray(st["nu"], dtype=dt).reshape(D, MK)
    zeta = np.asarray(st["zeta"], dtype=dt).reshape(D, M)
    logdet = cholesky_logdet(S, dt)
    l2pi = L2PI_LD if dt is LD else np.log(dt(2) * np.pi)
    Eeff = [lay.effective(st["Elnphi"], m, dt) for m in range(M)]
    theta = np.asarray(st["theta"], dtype=dt)
    for d in range(D):
        diff = lam[d] - mu
        tr = nu[d] * np.diag(S)
        quad = diff[:, None] * S * diff[None, :]
        v[1] = v[1] + dt(0.5) * (logdet - dt(MK) * l2pi - _tot(tr, dt) - _tot(quad, dt))      # MMCTM.jl:286-300
        A[1] += 0.5 * (abs(float(logdet)) + MK * float(l2pi) + _abs(tr) + _abs(quad))
        lognu = np.log(nu[d])
        v[5] = v[5] + dt(-0.5) * (_tot(lognu, dt) + dt(MK) * (l2pi + dt(1)))                   # MMCTM.jl:352-358
        A[5] += 0.5 * (_abs(lognu) + MK * (float(l2pi) + 1))
        Ee = np.exp(lam[d] + dt(0.5) * nu[d])
        for m in range(M):                                                                    # MMCTM.jl:302-316
            x = np.asarray(s.X[d][m], dtype=np.int64).reshape(-1, 2)
            n = x[:, 1].astype(dt); N = _tot(n, dt)
            th = lay.theta_dm(theta, d, m).astype(dt)                                         # [W, K_m]
            sl = slice(s.koff[m], s.koff[m + 1])
            lin = th * n[:, None] * lam[d, sl][None, :]                                       # λ . sumθ
            ndz = (N / zeta[d, m]) * Ee[sl]
            nlz = N * np.log(zeta[d, m])
            v[2] = v[2] + _tot(lin, dt) - _tot(ndz, dt) + N - nlz
            A[2] += _abs(lin) + _abs(ndz) + float(N) + abs(float(nlz))
            px = n[:, None] * th * Eeff[m][:, x[:, 0] - 1].T                                  # MMCTM.jl:318-336
            qz = n[:, None] * _xlogx(th, dt)                                                  # MMCTM.jl:360-370
            v[3] = v[3] + _tot(px, dt); v[6] = v[6] + _tot(qz, dt)
            A[3] += _abs(px); A[6] += _abs(qz)
    return np.array(v, dtype=dt), np.array(A)


def ctm_terms(lay, st):
    v, A = _ctm_eval(lay, st, LD)
    f, _ = _ctm_eval(lay, st, np.float64)
    return Terms(v, A, f)


def qz_scale_ctm(lay, st):
    """Σ n |θ| (|log θ| + 1): the first-order sensitivity of ElnQZ to a relative error of θ"""
    tot = 0.0
    th = np.asarray(st["theta"], dtype=np.float64)
    for m in range(lay.M):
        for d in range(lay.D):
            x = np.asarray(lay.s.X[d][m], dtype=np.int64).reshape(-1, 2)
            p = lay.theta_dm(th, d, m)
            with np.errstate(divide="ignore", invalid="ignore"):
                tot += float((x[:, 1][:, None] * np.where(p > 0, p * (np.abs(np.log(np.where(p > 0, p, 1.0))) + 1.0), 0.0)).sum())
    return tot


def qz_scale_lda(st):
    p = np.asarray(st["phi"], dtype=np.float64)
    return float(np.where(p > 0, p * (np.abs(np.log(np.where(p > 0, p, 1.0))) + 1.0), 0.0).sum())


def ctm_grid_s(D, cus):
    """blocks of 4 waves of the CTM stage kernels (mmm_ctm_create_batch): min(ceil(D / 4), 4 CUs' - 1), at least 1"""
    return max(1, min((D + 3) // 4, 4 * cus - 1))


def ctm_roundings(lay, cus=256):
    """n per term through k_ctm_elbo_docs<TAB_LDS> / k_ctm_elbo_docs_big, k_ctm_elbo_topics, k_sum_columns and elbo_finish (a library
    call counts as one rounding; `tail` as in lda_roundings; slots = ceil(ΣK / 64) coordinates per lane in the _big kernel).
      tokens  one accumulator per lane runs over every modality: Σ_m ceil(W_m / 64) K_m products of 2 roundings + 1 addition
      blocks  k_ctm_elbo_topics adds one Dirichlet per (m, k[, i]) to P and Q: its own path (ceil(n / 256) x 4 per thread, wave and block sum
              6 + 3, lgamma(Σγ) on a sum of ceil(n / 256) + 9 roundings, 7 for the closing arithmetic) plus one addition per block
      ElnPη   λ - μ (1), the ΣK-long fma chain of invΣ (λ - μ), ν invΣ_ii + diff Sd (3), the slots -- and the chain once more for what the
              products carry in (the issue's "twice"); logdet: a pivot has passed through up to ΣK eliminations of 2 roundings, log, ΣK
              additions (3 ΣK + 2); host: 5"""
    D, MK, M = lay.D, lay.MK, lay.M
    gs = ctm_grid_s(D, cus)
    steps = -(-D // (gs * 4)) if D else 0
    slots = -(-MK // 64)
    tail = 6 + steps + 3 + (-(-gs // 64)) + 6
    Wmax = lay.W.max(axis=0) if D else np.zeros(M, dtype=np.int64)
    tok = int(sum(-(-int(Wmax[m]) // 64) * lay.K[m] for m in range(M)))
    s = lay.s
    nb = int(sum(lay.K[m] * (s.I[m] if lay.imm else 1) for m in range(M)))
    nmax = max(max(s.J[m]) for m in range(M)) if lay.imm else max(lay.V)
    rows = -(-nmax // 256)
    Imax = max(s.I) if lay.imm else 1
    n = np.zeros(7)
    n[0] = rows + 9 + 7 + nb
    n[1] = 2 * MK + 4 + slots + tail + 3 * MK + 2 + 5
    n[2] = 6 * slots + 4 + 3 * tok + 1 + tail
    n[3] = 3 * tok + tail + (Imax - 1)
    n[4] = 4 * rows + 9 + rows + 9 + 1 + 7 + nb
    n[5] = 2 * slots + tail + 4
    n[6] = 3 * tok + tail
    return n


def elbo_docs_lds(lay, wide):
    """dynamic LDS of the k_ctm_elbo_docs launch in bytes (elbo_enqueue): invΣ, the table when it is staged, 64 doubles per wave"""
    GT = int(sum(lay.K[m] * lay.V[m] for m in range(lay.M)))
    return 8 * (lay.MK * lay.MK + (0 if wide else GT) + 4 * 64)


def ctm_is_wide(lay, forced=False):
    """mmm_ctm_create_batch: the table and one slab beyond 160 KB of LDS with a single wave left, a modality of more than 32 topics,
    ΣK > 64, or ctm_build = wide.  estep_lds(F_SLAB) = 8 (GT + waves G L + waves max_m K_m V_m), L = 16 / 32 / 64 lanes per document, G = 64 / L,
    waves halved from 8 while it is above 150 KB."""
    GT = int(sum(lay.K[m] * lay.V[m] for m in range(lay.M)))
    slab = max(lay.K[m] * lay.V[m] for m in range(lay.M))
    waves = 8
    lds = lambda w: 8 * (GT + w * 64 + w * slab)
    while waves > 1 and lds(waves) > 150 * 1024:
        waves >>= 1
    return bool(forced or lds(waves) > 160 * 1024 or max(lay.K) > 32 or lay.MK > 64)


# ---------------------------------------------------------------------------------------------------------- written states
SPECIAL = (1e-3, 1.0 + 1e-9, 1.0 - 1e-9, 2.0 + 1e-9, 2.0 - 1e-9, 1e6)       # α-sized, both sides of lgamma's zeros, large


def _plant(a, vals, step=3):
    """vals at every `step`-th entry of the flat array (as many as fit), in place"""
    f = a.reshape(-1)
    for i, x in enumerate(vals):
        if i * step < f.size:
            f[i * step] = x
    return a


def _docs(rng, V, lens, dup=False, big_count=False):
    X = []
    for W in lens:
        t = rng.choice(V, size=W, replace=W > V) + 1
        c = rng.integers(1, 20, size=W)
        X.append(np.stack([t, c], axis=1).astype(np.int64).reshape(-1, 2))
    for x in X:
        if dup and x.shape[0] >= 2:
            x[1, 0] = x[0, 0]; dup = False                      # a term listed twice in one document
    for x in X:
        if big_count and x.shape[0] >= 1:
            x[-1, 1] = 70000; big_count = False
    return X


def _lens(D, pattern):
    return [pattern[d % len(pattern)] for d in range(D)]


LEN_EDGES = (0, 1, 63, 64, 65, 130)          # around the 64-lane token stride

# name, K, V, D, lens: K in {1, 2, 63, 64 | 65, 128, 129, 256}, V around the 256 stride of k_lda_elbo_topics, D in {1, 3, 16, 17} under
# geometry_cus = 1 (grid_s <= 4 blocks of 4 waves; D = 17 takes a second document step with one live wave)
LDA_CASES = (
    dict(name="k1_v1_d1", K=1, V=1, D=1, lens=(1,)),
    dict(name="k2_v96_d3", K=2, V=96, D=3, lens=(0, 1, 63)),
    dict(name="k10_v96_d17", K=10, V=96, D=17, lens=LEN_EDGES),
    dict(name="k63_v255_d16", K=63, V=255, D=16, lens=(64, 65, 130, 0, 1, 63)),
    dict(name="k64_v256_d17", K=64, V=256, D=17, lens=LEN_EDGES),
    dict(name="k65_v257_d17", K=65, V=257, D=17, lens=LEN_EDGES),
    dict(name="k128_v96_d3", K=128, V=96, D=3, lens=(65, 0, 64)),
    dict(name="k129_v96_d16", K=129, V=96, D=16, lens=(1, 63, 65, 0)),
    dict(name="k256_v96_d1", K=256, V=96, D=1, lens=(130,)),
    dict(name="ilda_snv3", K=5, V=96, D=17, lens=LEN_EDGES, J=(6, 4, 4), eta=(0.1, 0.1, 0.1)),
    dict(name="ilda_i2_eta", K=7, V=24, D=3, lens=(24, 0, 65), J=(6, 4), eta=(0.3, 1.7)),
)


def full_product(J):
    """V = Π J_i terms, every combination of feature values once, 1-based [V, I]"""
    grids = np.meshgrid(*[np.arange(1, j + 1) for j in J], indexing="ij")
    return np.stack([g.ravel() for g in grids], axis=1).astype(np.int64)


def lda_case(name):
    return next(c for c in LDA_CASES if c["name"] == name)


def lda_state(rng, case):
    K, V, D = case["K"], case["V"], case["D"]
    X = _docs(rng, V, _lens(D, case["lens"]), dup=True, big_count=True)
    nnz = sum(x.shape[0] for x in X)
    st = dict(K=K, V=V, D=D, X=X, alpha=1e-3, eta=0.37, features=None)
    phi = rng.dirichlet(np.full(K, 0.3), size=nnz).reshape(nnz, K)
    phi[::5, rng.integers(0, K)] = 0.0                                    # dev_xlogx(0)
    phi[phi < 1e-300] = 0.0
    st["phi"] = phi
    st["gamma"] = _plant(rng.gamma(2.0, 3.0, size=(D, K)) + 0.01, SPECIAL).T.copy()          # [K, D]; the specials along a document
    st["Elntheta"] = -rng.gamma(2.0, 2.0, size=(K, D))
    if case.get("J"):
        J = case["J"]
        st["features"] = full_product(J) if int(np.prod(J)) == V else None
        assert st["features"] is not None, "an ILDA case takes the full product of its feature values"
        st["eta"] = np.asarray(case["eta"], dtype=np.float64)
        st["lam"] = [_plant(rng.gamma(1.5, 20.0, size=(j, K)) + 0.05, SPECIAL, step=5) for j in J]
        st["Elnbeta"] = [-rng.gamma(2.0, 3.0, size=(j, K)) for j in J]
    else:
        st["lam"] = _plant(rng.gamma(1.5, 20.0, size=(V, K)) + 0.05, SPECIAL, step=5)
        st["Elnbeta"] = -rng.gamma(2.0, 3.0, size=(V, K))
    return st


# K, V (or features), pattern of listed terms per (document, modality); D in {1, 12, 13} under geometry_cus = 1 (grid_s <= 3 blocks of 4
# waves: document 12 is a wave's second step).  ΣK in {1, 2, 14, 28, 63, 64 | 65, 128, 256}; M in {1, 3, 8}.
SNV3 = (6, 4, 4)
CTM_CASES = (
    dict(name="k1", K=[1], V=[5], D=1, lens=((1,),)),
    dict(name="k2", hot=True, K=[2], V=[9], D=12, lens=((0,), (1,), (9,))),
    dict(name="k7_7", K=[7, 7], V=[96, 48], D=13, lens=((64, 0), (0, 0), (65, 1), (1, 48), (0, 5))),
    dict(name="k7_7_wide", K=[7, 7], V=[96, 48], D=13, lens=((64, 0), (0, 0), (65, 1), (1, 48), (0, 5)), build="wide", twin="k7_7"),
    dict(name="k28", hot=True, K=[10, 10, 8], V=[30, 20, 16], D=12, lens=((30, 0, 16), (1, 20, 0), (0, 0, 0), (65, 64, 1))),
    dict(name="k63", K=[31, 32], V=[20, 24], D=13, lens=((20, 24), (0, 1), (64, 65))),
    dict(name="k64_lds48", K=[32, 32], V=[40, 40], D=13, lens=((40, 1), (0, 0), (65, 64), (1, 0))),
    dict(name="k65", hot=True, K=[33, 32], V=[12, 10], D=13, lens=((12, 10), (0, 0), (64, 65), (1, 0))),
    dict(name="k128", K=[40, 40, 48], V=[9, 8, 7], D=12, lens=((9, 8, 7), (0, 1, 65), (64, 0, 0))),
    dict(name="k256", K=[32] * 8, V=[6] * 8, D=1, lens=((6, 0, 1, 65, 64, 2, 3, 4),)),
    dict(name="m8_k1", K=[1] * 8, V=[4] * 8, D=12, lens=((4, 0, 1, 2, 3, 4, 0, 65), (0,) * 8)),
    dict(name="k33_4", K=[33, 4], V=[10, 8], D=12, lens=((10, 8), (0, 1), (65, 0))),
    dict(name="wide_tab", K=[16, 8], V=[700, 260], D=12, lens=((130, 64), (0, 0), (1, 65), (65, 0))),
    dict(name="imm_snv3", K=[5], J=[SNV3], D=13, lens=((96,), (0,), (65,), (1,), (64,))),
    dict(name="imm_2mod", hot=True, K=[4, 3], J=[(3, 2, 2), (5, 2)], D=12, lens=((12, 10), (0, 0), (1, 65), (64, 0))),
)


def ctm_case(name):
    return next(c for c in CTM_CASES if c["name"] == name)


def ctm_layout(rng, case):
    K = case["K"]; M = len(K)
    feats = [full_product(j) for j in case["J"]] if case.get("J") else None
    V = [int(f.shape[0]) for f in feats] if feats else case["V"]
    pat = case["lens"]
    X = []
    per_m = [_docs(rng, V[m], [pat[d % len(pat)][m] for d in range(case["D"])], dup=(m == 0), big_count=(m == M - 1)) for m in range(M)]
    for d in range(case["D"]):
        X.append([per_m[m][d] for m in range(M)])
    return CtmLayout(K, V, X, features=feats)


def spd(rng, n, lo=0.1, hi=100.0):
    """symmetric positive definite with eigenvalues spread geometrically over [lo, hi]: κ₂ = hi / lo = 1e3 (<= 1e4)"""
    if n == 1:
        return np.array([[2.0]])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    S = (Q * np.geomspace(lo, hi, n)[None, :]) @ Q.T
    return 0.5 * (S + S.T)


def ctm_state(rng, case, lay=None):
    lay = lay or ctm_layout(rng, case)
    s = lay.s; D, MK, M = lay.D, lay.MK, lay.M
    G = int(s.goff[-1])
    unequal = (0.05, 0.7, 0.3, 1.9, 0.011, 1.0, 0.5, 2.5)
    st = dict(alpha=np.array([unequal[i % 8] for i in range(lay.nalpha)]))
    st["mu"] = 10.0 + rng.standard_normal(MK)
    st["invSigma"] = spd(rng, MK)
    st["gamma"] = _plant(rng.gamma(2.0, 10.0, size=G) + 0.05, SPECIAL, step=7)
    st["Elnphi"] = -rng.gamma(2.0, 2.0, size=G)
    st["lam"] = rng.uniform(-6.0, 6.0, size=(D, MK))
    # ν over [1e-6, 5]; the cases marked `hot` reach 50, where exp(λ + ν / 2) of one coordinate dwarfs the rest of ElnPZ (so not everywhere:
    # a bound scaled by that summand would hide the other documents)
    hi = 50.0 if case.get("hot") else 5.0
    st["nu"] = _plant(np.exp(rng.uniform(np.log(1e-6), np.log(hi), size=(D, MK))), (1e-6, hi), step=2)
    st["zeta"] = _plant(np.exp(rng.uniform(np.log(1e-3), np.log(1e6), size=(D, M))), (1e-3, 1e6), step=1)
    th = []
    for m in range(M):
        p = rng.dirichlet(np.full(lay.K[m], 0.4), size=int(lay.nnz[m])).reshape(int(lay.nnz[m]), lay.K[m])
        p[::4, rng.integers(0, lay.K[m])] = 0.0                  # exact zeros
        p[p < 1e-300] = 0.0
        th.append(p.ravel())
    st["theta"] = np.concatenate(th) if th else np.zeros(0)
    return lay, st


def with_theta(st, theta):
    out = dict(st); out["theta"] = theta
    return out


def with_phi(st, phi):
    out = dict(st); out["phi"] = phi
    return out


# ---------------------------------------------------------------------------------------------------------- handles that have run passes
# After n fused passes ϕ (θ) is not stored: materialise_phi / materialise_theta form it on demand from the ring slots of pass n - 1.  A case
# is a corpus, the tuning that selects an E-step build, and the geometry the handle must report.  N_PASSES = 3, tol = 0.
N_PASSES = 3

PASS_LDA = (
    dict(name="single_step", K=10, V=96, D=64, tune={}, geo=dict(single_step=1, wide=0, dense=0, L=16)),
    dict(name="dense_row", K=10, V=96, D=130, tune=dict(lda_build="dense"), geo=dict(dense=1, wide=0, L=16)),
    dict(name="grid_stride", K=10, V=96, D=130, tune=dict(grid_blocks=3), geo=dict(single_step=0, grid_e=3, wide=0, dense=0)),
    dict(name="wide", K=10, V=96, D=64, tune=dict(lda_build="wide"), geo=dict(wide=1)),
    dict(name="k65", K=65, V=96, D=40, tune={}, geo=dict(wide=1, L=64, KP=66)),
)

PASS_CTM = (
    dict(name="lds", K=[5, 4], V=[40, 24], D=48, means=[600, 80], tune={}, geo=dict(wide=0, tdense=0)),
    dict(name="rows_of_counts", K=[5, 4], V=[24, 16], D=48, means=[600, 300], tune=dict(ctm_build="dense"), geo=dict(wide=0, tdense=1)),
    dict(name="wide", K=[5, 4], V=[40, 24], D=48, means=[600, 80], tune=dict(ctm_build="wide"), geo=dict(wide=1, tdense=0)),
    dict(name="k65", K=[33, 32], V=[12, 10], D=20, means=[200, 100], tune={}, geo=dict(wide=1, L=64, cpl=4)),
    dict(name="imm_snv3", K=[5], J=[SNV3], D=40, means=[800], tune={}, geo=dict(wide=0)),
)


def _multinomial_docs(rng, D, V, K, mean_n, conc, empty=()):
    beta = rng.dirichlet(np.full(V, conc), size=K)
    X = []
    for d in range(D):
        th = rng.dirichlet(np.full(K, 0.5))
        c = rng.multinomial(0 if d in empty else 50 + rng.poisson(mean_n), th @ beta)
        idx = np.nonzero(c)[0]
        X.append(np.stack([idx + 1, c[idx]], axis=1).astype(np.int64).reshape(-1, 2))
    return X


def pass_lda(case, seed=11):
    """(X, λ0 [V, K]) of an after-passes LDA case: multinomial documents over K planted topics, no term listed twice"""
    rng = np.random.default_rng(seed)
    X = _multinomial_docs(rng, case["D"], case["V"], min(case["K"], 10), 400, 0.3)
    return X, rng.integers(1, 101, size=(case["V"], case["K"])).astype(np.float64)


def pass_ctm(case, seed=12):
    """(layout, α, flat γ0) of an after-passes CTM case; document 1 is empty in the last modality"""
    rng = np.random.default_rng(seed)
    feats = [full_product(j) for j in case["J"]] if case.get("J") else None
    V = [int(f.shape[0]) for f in feats] if feats else case["V"]
    M = len(case["K"])
    per_m = [_multinomial_docs(rng, case["D"], V[m], min(case["K"][m], 6), case["means"][m], 1.0, empty=(1,) if m == M - 1 and M > 1 else ())
             for m in range(M)]
    X = [[per_m[m][d] for m in range(M)] for d in range(case["D"])]
    lay = CtmLayout(case["K"], V, X, features=feats)
    alpha = [np.array([0.1, 0.4, 0.25][:len(j)]) for j in case["J"]] if feats else [0.05, 0.7][:M]
    g0 = rng.integers(1, 101, size=int(lay.s.goff[-1])).astype(np.float64)
    return lay, alpha, g0


def nested_gamma(lay, flat):
    """flat γ0 -> what MMCTM(γ0=...) takes (list over m of [K_m, V_m]); an IMMCTM takes the flat array"""
    return flat if lay.imm else [np.asarray(flat)[lay.s.goff[m]:lay.s.goff[m + 1]].reshape(lay.K[m], lay.V[m]) for m in range(lay.M)]


def rows_of_counts_ok(lay):
    """what create asks of a corpus for the rows-of-counts θ phase when ctm_build = dense forces it: every modality <= 16 topics and <= 128
    terms, no term listed twice in a document, counts below 65536, at least half of the D x V_m cells present"""
    cells = sum(lay.D * v for v in lay.V); present = int(lay.nnz.sum())
    nodup = all(len(set(np.asarray(lay.s.X[d][m]).reshape(-1, 2)[:, 0])) == lay.W[d, m] for d in range(lay.D) for m in range(lay.M))
    small = all(int(np.asarray(lay.s.X[d][m]).reshape(-1, 2)[:, 1].max(initial=0)) < 65536 for d in range(lay.D) for m in range(lay.M))
    return max(lay.K) <= 16 and max(lay.V) <= 128 and nodup and small and 2 * present >= cells and lay.MK <= 64


def lda_written(name):
    """(case, written state) of an LDA / ILDA case: the draw both test files use"""
    c = lda_case(name)
    return c, lda_state(np.random.default_rng([x["name"] for x in LDA_CASES].index(name)), c)


def ctm_written(name):
    """(case, layout, written state) of a CTM case; a case with a `twin` draws its twin's state (another build on the same numbers)"""
    c = ctm_case(name)
    lay, st = ctm_state(np.random.default_rng(100 + [x["name"] for x in CTM_CASES].index(c.get("twin", name))), c)
    return c, lay, st


def lda_case_roundings(c, cus=1):
    return lda_roundings(c["K"], c["V"], c["D"], max(c["lens"]), cus=cus, I=len(c.get("J", ())), Jmax=max(c.get("J", (0,))))
