"""Inputs and references for the Gaussian M-step of the CTM (update_μ! / update_Σ! / inv(Σ), MMCTM.jl:200-212; `ctm_gauss_mstep` in
csrc/ctm_mstep.cuh with its three Gauss-Jordan inversions).  numpy only (mpmath is used by the tests that check this file), no GPU.

* `state(n, kind, seed)`: document states (λ, ν) on which the inversions swap rows at about half of the columns ("pivot"), the states
  fits produce ("typical"), a mean far from zero ("shifted") and exactly singular Σ ("singular0", "singular_mid").
* `sigma_ref`: the reference's centred Σ in np.longdouble; `sigma_bound`: what float64 may lose on the device's raw-moment form.
* `lu_longdouble`: inverse and log|det| by LU + Newton-Schulz in np.longdouble; `gauss_jordan`: the device's elimination in float64.
* `cases()`: the sizes the GPU tests run, one per build and per boundary between builds.
* `twin(...)`: `orc_twin_moments` + `orc_twin_gauss` (oracle/mmm_twin.c) on a state, for any ΣK <= 256."""
import ctypes as C

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                 # unit roundoff of float64
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble has no extended precision on this machine"

KINDS = ("pivot", "typical", "shifted", "singular0", "singular_mid")


# the draw of the "pivot" state per size: the first seed at which the elimination swaps rows at column 0 and in the last three columns
# (the conditions tests/test_gauss_ref_cpu.py asserts); 0 where not listed
_PIVOT_DRAW = {3: 2, 64: 5, 256: 4}


def state(n, kind, seed=None, shift=100.0):
    """(lam [D, n], nu [D, n]) with D = 2 n + 3: odd and no multiple of 32, so the last 32-document tile of k_ctm_moments is short.

    pivot: coordinates of scales 1 ... 30 (geometric, shuffled) that share a common factor, ν = 1e-6 -- Σ is far from diagonally
        dominant, the largest entry of a column is rarely on the diagonal (swaps at about half of the columns, κ₂ 5e3 ... 4e5).
    typical: scales 1, no common factor, ν ~ U(0.05, 0.5): diag(Σν) plus a scatter of similar scale.
    shifted: pivot with `shift` added to every coordinate (|μ| >> the spread of λ: the raw-moment form cancels).
    singular0: typical, coordinate 0 constant (0.5) with ν = 0 -- row and column 0 of Σ are exactly zero (every product and sum of the
        raw-moment form that involves coordinate 0 is exact or cancels exactly: D is odd, 0.5 D is exact).
    singular_mid: typical, coordinates 0 and 1 are +1 in document 0, -1 in document 1, 0 elsewhere, ν = 0 on both; the other coordinates
        of document 1 stay within 0.25 of document 0's.  The leading block is [[a, a], [a, a]], a = 2 / D, rows 0 and 1 are identical and
        every other entry of column 0 is below a: column 0 takes row 0 as its pivot, and its elimination leaves column 1 exactly zero at
        and below the diagonal (a - a·(a / a), x - x·1)."""
    assert kind in KINDS
    draw = "pivot" if kind == "shifted" else kind
    if seed is None:
        seed = _PIVOT_DRAW.get(n, 0) if draw == "pivot" else 0
    rng = np.random.default_rng([n, KINDS.index(draw), seed])
    D = 2 * n + 3
    if kind in ("pivot", "shifted"):
        s = rng.permutation(np.geomspace(1.0, 30.0, n))
        z = np.sqrt(0.8) * rng.standard_normal((D, 1)) + np.sqrt(0.2) * rng.standard_normal((D, n))
        lam = 0.1 * s * z
        nu = np.full((D, n), 1e-6)
        if kind == "shifted":
            lam = lam + float(shift)
        return np.ascontiguousarray(lam), nu
    lam = rng.standard_normal((D, n))
    nu = rng.uniform(0.05, 0.5, size=(D, n))
    if kind == "singular0":
        lam[:, 0] = 0.5; nu[:, 0] = 0.0
    elif kind == "singular_mid":
        assert n >= 2
        lam[1, 2:] = lam[0, 2:] - 0.25 * rng.uniform(-1.0, 1.0, size=n - 2)
        lam[:, :2] = 0.0; lam[0, :2] = 1.0; lam[1, :2] = -1.0
        nu[:, :2] = 0.0
    return np.ascontiguousarray(lam), nu


def sigma_ref(lam, nu, mu):
    """update_Σ! as the reference writes it (MMCTM.jl:204-210): (diag(Σ_d ν_d) + Σ_d (λ_d - μ)(λ_d - μ)') / D, in np.longdouble."""
    lam = np.asarray(lam, dtype=LD); nu = np.asarray(nu, dtype=LD); mu = np.asarray(mu, dtype=LD)
    D = lam.shape[0]
    diff = lam - mu
    S = np.zeros((lam.shape[1],) * 2, dtype=LD)
    for d in range(D):
        S += np.outer(diff[d], diff[d])
    S[np.diag_indices_from(S)] += nu.sum(axis=0)
    return S / LD(D)


def sigma_bound(lam, nu, mu):
    """Elementwise a-priori bound on |Σ_device - Σ_exact| for the raw-moment evaluation in float64, Σ_exact being the centred formula at
    the SAME μ (Σ_d (λ-μ)(λ-μ)' = Σλλ' - μ Σλ' - Σλ μ' + D μμ' holds for every μ, so μ's own rounding is not part of it).

    The device forms, with u = 2^-53 and γ_k = k u / (1 - k u) (Higham, Accuracy and Stability, §3.1, §4.2):
      k_ctm_moments + k_reduce_partials
        S_i  = Σ_d λ_di          D terms, some fixed tree (4 chains per tile, tiles, blocks, 64/8/8 slabs; added zeros do not round):
                                 |ΔS_i| <= γ_{D-1} B_i,  B_i = Σ_d |λ_di|
        N_i  = Σ_d ν_di          |ΔN_i| <= γ_{D-1} N_i
        LL_ij = Σ_d λ_di λ_dj    D products (one rounding each; the fused ones round less) and D-1 additions:
                                 |ΔLL_ij| <= γ_D A_ij,  A_ij = Σ_d |λ_di λ_dj|
      ctm_gauss_mstep
        t1 = μ_i S_j, t2 = μ_j S_i   one product each:  |Δt1| <= γ_D |μ_i| B_j,  |Δt2| <= γ_D |μ_j| B_i   (|S| <= B)
        t3 = (D μ_i) μ_j             two products:      |Δt3| <= γ_2 D |μ_i μ_j|
        v  = ((LL - t1) - t2) + t3 [+ N_i on the diagonal]   at most 4 additions/differences: a further factor (1 + γ_4) on every term
        Σ_ij = v / D                 one division: a further factor (1 + u)
    With T_ij = A_ij + |μ_i| B_j + |μ_j| B_i + D |μ_i μ_j| + [i = j] N_i every term carries at most D + 5 roundings, hence
        |Σ_device - Σ_exact|_ij <= γ_{D+5} T_ij / D.
    (The issue names A, D|μμ|, N, D and u; the cross terms |μ_i| B_j belong to the same operations and are kept.)  The comparison value
    `sigma_ref` is itself rounded, in np.longdouble (u' = 2^-64 <= 2^-11 u) on sums the same T bounds: the bound returned is
    (γ_{D+5} + γ'_{D+5}) T / D.  A derived bound: no constant in it comes from a measurement."""
    lam = np.asarray(lam, dtype=LD); nu = np.asarray(nu, dtype=LD); mu = np.asarray(mu, dtype=LD)
    D = lam.shape[0]
    al = np.abs(lam); am = np.abs(mu)
    A = al.T @ al
    B = al.sum(axis=0)
    T = A + np.outer(am, B) + np.outer(B, am) + D * np.outer(am, am)
    T[np.diag_indices_from(T)] += nu.sum(axis=0)
    k = D + 5
    g = k * U / (1.0 - k * U) + k * 2.0 ** -64 / (1.0 - k * 2.0 ** -64)
    return np.asarray(LD(g) * T / LD(D), dtype=np.float64)


def lu_longdouble(S, max_steps=8):
    """(S^-1, log|det S|) in np.longdouble: LU with partial pivoting (vectorised rank-1 updates), triangular solves for every column at
    once, then Newton-Schulz steps X <- X + X (I - S X) until max|I - S X| <= n 2^-60.  The residual is itself formed in np.longdouble, so
    for an ill-conditioned S it stalls near n 2^-64 max(|S||X|) before it reaches that; the loop also ends when a step no longer halves
    it.  tests/test_gauss_ref_cpu.py holds the result to n 2^-60 κ₂ of mpmath's at 50 digits."""
    S = np.asarray(S, dtype=LD)
    n = S.shape[0]
    lu = S.copy()
    perm = np.arange(n)
    logdet = LD(0)
    for c in range(n):
        p = c + int(np.argmax(np.abs(lu[c:, c])))
        if p != c:
            lu[[c, p]] = lu[[p, c]]; perm[[c, p]] = perm[[p, c]]
        if lu[c, c] == 0:
            raise np.linalg.LinAlgError("singular matrix")
        logdet += np.log(np.abs(lu[c, c]))
        lu[c + 1:, c] /= lu[c, c]
        lu[c + 1:, c + 1:] -= np.outer(lu[c + 1:, c], lu[c, c + 1:])
    X = np.eye(n, dtype=LD)[perm]
    for c in range(n):                       # L y = P
        X[c + 1:] -= np.outer(lu[c + 1:, c], X[c])
    for c in range(n - 1, -1, -1):           # U x = y
        X[c] /= lu[c, c]
        X[:c] -= np.outer(lu[:c, c], X[c])
    eye = np.eye(n, dtype=LD)
    prev = np.inf
    for _ in range(max_steps):
        R = eye - S @ X
        res = float(np.abs(R).max())
        if res <= n * 2.0 ** -60 or res > 0.5 * prev:
            break
        X = X + X @ R
        prev = res
    return X, logdet


def gauss_jordan(S):
    """The device's elimination (block_inverse_wide / _pipelined / _big; orc_twin_gauss), restated in float64: per column the pivot is the
    largest |entry| at or below the diagonal, ties to the lowest row; the pivot row is swapped up and scaled, the column's multipliers are
    taken after the swap, every other row is eliminated.  Returns (inverse, pivot row per column, list of the columns at which rows were
    swapped, first column whose pivot was exactly zero or None)."""
    A = np.array(S, dtype=np.float64)
    n = A.shape[0]
    Ai = np.eye(n)
    piv_rows = np.zeros(n, dtype=np.int64)
    swaps = []
    zero_at = None
    with np.errstate(all="ignore"):
        for c in range(n):
            p = c + int(np.argmax(np.abs(A[c:, c])))          # argmax: the first of equal maxima
            if A[p, c] == 0.0 and zero_at is None:
                zero_at = c
            piv_rows[c] = p
            if p != c:
                swaps.append(c)
            piv = A[p, c]
            for Mx in (A, Ai):
                top = Mx[c].copy()
                Mx[c] = Mx[p] / piv
                if p != c:
                    Mx[p] = top
            rows = np.arange(n) != c
            f = A[rows, c].copy()
            A[rows] -= np.outer(f, A[c])
            A[rows, c] = 0.0
            Ai[rows] -= np.outer(f, Ai[c])
    return Ai, piv_rows, swaps, zero_at


# ΣK -> its split into modalities (K_m <= 64, at most 8 modalities)
_SPLITS = {1: [1], 2: [1, 1], 3: [2, 1], 10: [10], 28: [10, 10, 8], 31: [16, 15], 32: [32], 33: [17, 16], 63: [32, 31], 64: [64],
           65: [33, 32], 128: [64, 64], 256: [64, 64, 64, 64]}


def cases():
    """The fixed list of (ΣK, K): small sizes (1, 2, 3, 10); 28, the config 4 size; 31 | 32, the last sizes of the pipelined build, whose
    11 rows per thread are all in use at 32; 33, 63, 64: the wide build, 64 a full wave in the pivot search; 65, 128, 256: the big build,
    256 its limit."""
    return [(n, list(K)) for n, K in _SPLITS.items()]


def corpus(n, K):
    """A tiny valid corpus for the case: D = 2 n + 3 documents, two terms per modality, one token of one term per document and modality."""
    D = 2 * n + 3
    V = [2] * len(K)
    X = [[np.array([[1 + (d + m) % 2, 1]], dtype=np.int64) for m in range(len(K))] for d in range(D)]
    return X, V


def twin(oracle, n, K, lam, nu, grid_m):
    """`orc_twin_moments` + `orc_twin_gauss` on the state, moments over `grid_m` blocks -> (rc, μ, Σ, Σ^-1, oracle model).  rc = -2: an exactly zero
    pivot.  (The oracle model is built without a launch geometry -- its E-step is not run here -- so that ΣK > 64 is accepted.)"""
    X, V = corpus(n, K)
    o = oracle.CtmOracle(K, [0.1] * len(K), X, V=V, seed=1)
    o.s.grid_m = int(grid_m)
    o.lam[:] = np.asarray(lam, dtype=np.float64).ravel(); o.nu[:] = np.asarray(nu, dtype=np.float64).ravel()
    mom = np.zeros(2 * n + n * n)
    L = oracle.lib()
    L.orc_twin_moments(C.byref(o.s), mom)
    with np.errstate(all="ignore"):
        rc = L.orc_twin_gauss(C.byref(o.s), mom, 1)
    return rc, o.mu.copy(), o.Sigma.reshape(n, n, order="F").copy(), o.invSigma.reshape(n, n, order="F").copy(), o


def inv_error_bound(oracle, S, F=4.0):
    """What a float64 inverse of the float64 matrix S may be off by, entrywise maximum: F max(e_LU, e_numpy, n 2^-52 max|X|) with X the
    np.longdouble inverse, e_LU the error of the literal oracle's LU inverse (`orc_inv_logdet`, the restatement of the reference's `inv`)
    and e_numpy the error of numpy's, both on the same S.  Gauss-Jordan with partial pivoting has the first-order forward-error bound
    of LU inversion up to a modest constant, and single draws scatter by a few times: F = 4.  Returns (bound, X, log|det S|, unit) with
    unit = bound / F."""
    n = S.shape[0]
    X, ld = lu_longdouble(S)
    rc, Xlu, _, _ = oracle.inv_logdet(S)
    assert rc == 0
    e_lu = float(np.abs(Xlu.astype(LD) - X).max())
    e_np = float(np.abs(np.linalg.inv(S).astype(LD) - X).max())
    unit = max(e_lu, e_np, n * 2.0 ** -52 * float(np.abs(X).max()))
    return F * unit, X, ld, unit
