"""tests/gauss_ref.py against mpmath, its input states against the conditions they are built for, and the order-matched oracle's
Gaussian M-step (orc_twin_moments + orc_twin_gauss, the CPU restatement the device must equal bit for bit) against both.  No GPU.

How often the suite's other inputs make the inversions swap rows (counted with `gauss_ref.gauss_jordan`, float64, on the CPU): the Σ of
test_ctm_gpu.py::test_estep_mstep_against_oracle -- mm2 0 of 14 columns in each of its three M-steps, mm3 0 of 28, imm 0, 0, 1 of 10 -- and
the twenty shapes of ::test_random_shapes_bit_identical_to_oracle: 2 swaps in 1071 columns over three passes each.  On the "pivot" states
of gauss_ref: 5 of 10, 20 of 32, 34 of 64, 162 of 256 (asserted below: at least a quarter of the columns, column 0 and one of the last
three).

Worst ratio of the twin's |invΣ - longdouble inverse| to the unit of gauss_ref.inv_error_bound (the larger of the literal oracle's LU
error, numpy's, and n 2^-52 max|X|), kinds pivot / typical / shifted(100), bound F = 4: pipelined sizes 1.30 / 0.26 / 0.85 (the 1.30 at
ΣK = 2), wide sizes 0.36 / 0.06 / 0.18, big sizes 0.11 / 0.07 / 0.24; Σ at most 0.104 of gauss_ref.sigma_bound (test_zz_worst_ratios
prints the table)."""
import mpmath as mp
import numpy as np
import pytest

import gauss_ref as G

LD = G.LD
CASES = G.cases()
ACC_KINDS = ("pivot", "typical", "shifted")
RATIOS = {}            # (build, kind) -> worst ratio to the unit of the F-bound; (n, kind) -> Σ ratio to sigma_bound


def _mpf(x):
    """an np.longdouble as an mpf, exactly (two float64 pieces)"""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


def _build(n):
    return "pipelined" if n <= 32 else ("wide" if n <= 64 else "big")


def _grid_m(n):
    return max(1, (2 * n + 3 + 31) // 32)


@pytest.fixture(scope="module")
def twins(oracle):
    """(n, kind) -> (lam, nu, rc, μ, Σ, Σ^-1) of the order-matched oracle, computed once"""
    cache = {}

    def get(n, K, kind):
        if (n, kind) not in cache:
            lam, nu = G.state(n, kind)
            rc, mu, S, Si, _ = G.twin(oracle, n, K, lam, nu, _grid_m(n))
            cache[(n, kind)] = (lam, nu, rc, mu, S, Si)
        return cache[(n, kind)]
    return get


@pytest.mark.parametrize("kind", ["pivot", "shifted"])
@pytest.mark.parametrize("n", [2, 10, 33])
def test_helper_against_mpmath(n, kind):
    """sigma_ref and lu_longdouble against mpmath at 50 digits."""
    mp.mp.dps = 50
    lam, nu = G.state(n, kind)
    D = lam.shape[0]
    mu = lam.sum(axis=0) / D
    S = G.sigma_ref(lam, nu, mu)
    diff = [[mp.mpf(float(lam[d, i])) - mp.mpf(float(mu[i])) for i in range(n)] for d in range(D)]
    Smp = mp.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):
            s = mp.fsum(diff[d][i] * diff[d][j] for d in range(D))
            if i == j:
                s += mp.fsum(mp.mpf(float(x)) for x in nu[:, i])
            Smp[i, j] = Smp[j, i] = s / D
    smax = max(abs(Smp[i, j]) for i in range(n) for j in range(n))
    eS = max(abs(_mpf(S[i, j]) - Smp[i, j]) for i in range(n) for j in range(n))
    assert eS <= n * mp.mpf(2) ** -60 * smax, float(eS / smax)
    S64 = np.asarray(S, dtype=np.float64)
    X, ld = G.lu_longdouble(S64)
    A = mp.matrix(S64.tolist())
    Xmp = A ** -1
    kappa = float(np.linalg.cond(S64))
    xmax = max(abs(Xmp[i, j]) for i in range(n) for j in range(n))
    eX = max(abs(_mpf(X[i, j]) - Xmp[i, j]) for i in range(n) for j in range(n))
    eld = abs(_mpf(ld) - mp.log(abs(mp.det(A))))
    print("n = %d %s: κ₂ %.1e, Σ rel %.1e, inverse rel %.1e, log det abs %.1e (allowed %.1e)"
          % (n, kind, kappa, float(eS / smax), float(eX / xmax), float(eld), n * 2.0 ** -60 * kappa))
    assert eX <= n * mp.mpf(2) ** -60 * kappa * xmax
    assert eld <= n * mp.mpf(2) ** -60 * kappa


@pytest.mark.parametrize("n,K", CASES)
def test_pivot_states_make_the_elimination_swap(twins, n, K):
    """What the "pivot" states are for: row swaps at a quarter of the columns or more, one at column 0, one in the last three
    columns, and a condition number that leaves a float64 inverse meaningful."""
    lam, nu, rc, mu, S, Si = twins(n, K, "pivot")
    assert rc == 0
    _, piv, swaps, zero_at = G.gauss_jordan(S)
    assert zero_at is None
    kappa = np.linalg.cond(S)
    print("ΣK = %d: swaps at %d of %d columns, κ₂ = %.1e" % (n, len(swaps), n, kappa))
    assert kappa <= 1e6
    if n >= 2:
        assert 0 in swaps
        assert swaps[-1] >= n - 3
    if n >= 10:
        assert len(swaps) >= n / 4
    # ... and what fits produce does not: the states called typical swap (almost) nowhere
    St = twins(n, K, "typical")[4]
    assert len(G.gauss_jordan(St)[2]) <= max(1, n // 16)


@pytest.mark.parametrize("n", [2, 32, 33, 65])
def test_singular_states_meet_an_exact_zero_pivot(twins, n):
    K = dict(CASES)[n]
    for kind, col in (("singular0", 0), ("singular_mid", 1)):
        lam, nu, rc, mu, S, Si = twins(n, K, kind)
        assert rc == -2, kind
        piv, zero_at = G.gauss_jordan(S)[1::2]
        assert zero_at == col, (kind, zero_at)
        if kind == "singular0":
            assert not S[0].any() and not S[:, 0].any()
        else:
            assert S[0, 0] == S[0, 1] == S[1, 1] == 2.0 / (2 * n + 3) and np.array_equal(S[0], S[1]) and piv[0] == 0


@pytest.mark.parametrize("kind", ACC_KINDS)
@pytest.mark.parametrize("n,K", CASES)
def test_twin_is_the_elimination_and_is_accurate(oracle, twins, n, K, kind):
    """The order-matched oracle runs the algorithm under test -- from its own Σ, `gauss_jordan` gives its inverse (so: its pivot sequence;
    another sequence rounds differently) -- and is as accurate as float64 allows: μ and Σ within the a-priori bounds of the sums they
    are, Σ^-1 within F = 4 units of gauss_ref.inv_error_bound of the np.longdouble inverse."""
    lam, nu, rc, mu, S, Si = twins(n, K, kind)
    assert rc == 0
    D = lam.shape[0]
    X_gj = G.gauss_jordan(S)[0]
    assert np.all(np.abs(Si - X_gj) <= 4 * np.spacing(np.maximum(np.abs(Si), np.abs(X_gj)))), np.abs(Si - X_gj).max()
    # μ_i = fl(fl(Σ_d λ_di) / D): D - 1 additions and a division
    mu_ref = np.asarray(lam, dtype=LD).sum(axis=0) / LD(D)
    assert np.all(np.abs(mu.astype(LD) - mu_ref) <= (D + 1) * G.U * np.abs(lam).sum(axis=0) / D)
    rS = float((np.abs(S.astype(LD) - G.sigma_ref(lam, nu, mu)) / G.sigma_bound(lam, nu, mu)).max())
    bound, X, ld, unit = G.inv_error_bound(oracle, S)
    err = float(np.abs(Si.astype(LD) - X).max())
    RATIOS[(n, kind)] = (rS, err / unit)
    print("ΣK = %d %s: Σ at %.3f of its bound, Σ^-1 off by %.2e = %.2f units (bound 4)" % (n, kind, rS, err, err / unit))
    assert rS <= 1.0
    assert err <= bound


@pytest.mark.parametrize("n", [10, 32, 33, 64, 65, 256])
def test_oracle_logdet_against_longdouble(oracle, twins, n):
    """The ELBO's 0.5 D log det Σ^-1 (MMCTM.jl:286-300) is the literal oracle's LU log det; on the Σ^-1 of the pivot states it agrees with
    the np.longdouble one far inside the rtol = 1e-9 at which the device's ELBO terms are compared with the oracle's."""
    K = dict(CASES)[n]
    Si = twins(n, K, "pivot")[5]
    rc, _, ld_o, _ = oracle.inv_logdet(Si)
    assert rc == 0
    ld = G.lu_longdouble(Si)[1]
    print("ΣK = %d: log det Σ^-1 = %.6f, oracle off by %.1e relative" % (n, float(ld), abs(ld_o - float(ld)) / abs(float(ld))))
    assert abs(ld_o - float(ld)) <= 1e-11 * abs(float(ld))


def test_zz_worst_ratios():
    """Runs last: the worst ratios per build, as DESIGN.md section 4.6 quotes them."""
    print("\ncases run: %d of %d" % (len(RATIOS), len(CASES) * len(ACC_KINDS)))
    for b in ("pipelined", "wide", "big"):
        for kind in ACC_KINDS:
            v = [RATIOS[(n, kind)] for n, _ in CASES if _build(n) == b and (n, kind) in RATIOS]
            if v:
                print("  %-9s %-8s Σ / bound %.3f   Σ^-1 / unit %.2f" % (b, kind, max(x[0] for x in v), max(x[1] for x in v)))
    assert all(v[1] <= 4.0 for v in RATIOS.values())
