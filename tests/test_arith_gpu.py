"""The scalar functions and lane collectives whose bits decide where an LD_MMA solve stops (csrc/mmm_arith.h, dev_math.h),
evaluated on the device through mmm_debug_math and compared BIT FOR BIT with the host: the same header compiled by gcc
(oracle/mmm_twin.c), IEEE division / square root of numpy, and the summation trees written out in Python."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dev(mmm, ctx, op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    bp = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    mmm._lib.check(mmm.lib().mmm_debug_math(ctx.h, op, a.size, a, None if bp is None else bp.ctypes.data, out), ctx.h, "debug_math")
    return out


def _bits_equal(x, y):
    x = np.ascontiguousarray(x, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
    bad = x.view(np.int64) != y.view(np.int64)
    bad &= ~(np.isnan(x) & np.isnan(y))
    assert not bad.any(), "%d of %d values differ; first: %r vs %r" % (bad.sum(), x.size, x[bad][:3], y[bad][:3])


@pytest.fixture(scope="module")
def ctx(mmm):
    return mmm.Context(0)


def test_exp_log_digamma_bits(mmm, oracle, ctx):
    rng = np.random.default_rng(11)
    L = oracle.lib()
    xs = np.concatenate([rng.uniform(-40, 40, 200000), rng.uniform(-745, 709, 20000), rng.normal(0, 1e-4, 2000), [0.0, -0.0, 710.0, -746.0, 1e-320]])
    ref = np.empty_like(xs); L.orc_ar_exp_vec(xs.size, xs, ref)
    _bits_equal(_dev(mmm, ctx, 0, xs), ref)
    np.testing.assert_allclose(ref[:200000], np.exp(xs[:200000]), rtol=3e-16)
    xs = np.concatenate([rng.uniform(1e-7, 30, 200000), 10.0 ** rng.uniform(-300, 300, 20000), 1.0 + rng.normal(0, 1e-6, 2000)])
    ref = np.empty_like(xs); L.orc_ar_log_vec(xs.size, xs, ref)
    _bits_equal(_dev(mmm, ctx, 1, xs), ref)
    np.testing.assert_allclose(ref, np.log(xs), rtol=4e-16, atol=1e-18)
    xs = np.concatenate([rng.uniform(1e-3, 200, 100000), 10.0 ** rng.uniform(-7, 8, 20000)])
    ref = np.empty_like(xs); L.orc_ar_digamma_vec(xs.size, xs, ref)
    _bits_equal(_dev(mmm, ctx, 2, xs), ref)


def test_table_exp_log_bits_and_accuracy(mmm, oracle, ctx):
    """ar_exp_tab / ar_log_tab (the exp / log of the LD_MMA objectives: 128-entry tables, no division): the device evaluates them from LDS,
    the CPU restatement from a static array of the same generated numbers -- bit for bit, including the ends of the range (v_ldexp_f64 against
    the host's ldexp on subnormal results) -- and they are as accurate as their header claims (exp < 1 ulp; log: absolute 2.5e-15 up to x = 30)."""
    import mpmath as mp
    rng = np.random.default_rng(21)
    L = oracle.lib()
    xs = np.concatenate([rng.uniform(-40, 40, 200000), rng.uniform(-760, 712, 40000), rng.normal(0, 1e-4, 2000), rng.uniform(-745.2, -707, 20000),
                         [0.0, -0.0, 709.7, 709.78, 709.79, 710.0, 1e5, -1e5, 1e300, -1e300, np.inf, -np.inf, np.nan, -745.0, -745.13, -745.14, -746.0, -750.0, 1e-320]])
    ref = np.empty_like(xs); L.orc_ar_exptab_vec(xs.size, xs, ref)
    _bits_equal(_dev(mmm, ctx, 9, xs), ref)
    with np.errstate(over="ignore"):
        np.testing.assert_allclose(ref[:200000], np.exp(xs[:200000]), rtol=2.3e-16)
    assert ref[-19 + 2] > 1e308 and np.isinf(ref[-19 + 4]) and np.isinf(ref[-19 + 8]) and ref[-19 + 9] == 0.0 and np.isnan(ref[-19 + 12]) and ref[-19 + 11] == 0.0
    mp.mp.dps = 40
    worst = 0.0
    for x, y in zip(xs[:3000], ref[:3000]):                 # against 40-digit values: < 1 ulp
        t = mp.exp(mp.mpf(float(x)))
        worst = max(worst, float(abs(mp.mpf(float(y)) - t) / t) / 2.0 ** -52)
    assert worst < 1.0, worst
    xs = np.concatenate([rng.uniform(1e-7, 30, 200000), 10.0 ** rng.uniform(-300, 300, 20000), 1.0 + rng.normal(0, 1e-6, 2000), [1.0, 2.0, 0.5, 1e-7]])
    ref = np.empty_like(xs); L.orc_ar_logtab_vec(xs.size, xs, ref)
    _bits_equal(_dev(mmm, ctx, 10, xs), ref)
    assert np.max(np.abs(ref[:200000] - np.log(xs[:200000]))) < 2.5e-15
    worst = max(float(abs(mp.mpf(float(y)) - mp.log(mp.mpf(float(x))))) for x, y in zip(xs[:3000], ref[:3000]))
    assert worst < 2.5e-15, worst


def test_division_and_sqrt_are_ieee(mmm, ctx):
    """dev_div / dev_sqrt (the compiler's sequences without range handling) are correctly rounded in the range the MMA step
    algebra works in -- the host side of the parity tests uses plain `/` and sqrt()."""
    rng = np.random.default_rng(12)
    a = rng.normal(0, 1, 300000) * 10.0 ** rng.uniform(-12, 12, 300000)
    b = rng.normal(0, 1, 300000) * 10.0 ** rng.uniform(-12, 12, 300000)
    b[b == 0] = 1.0
    _bits_equal(_dev(mmm, ctx, 3, a, b), a / b)
    x = np.abs(a)
    _bits_equal(_dev(mmm, ctx, 4, x), np.sqrt(x))
    _bits_equal(_dev(mmm, ctx, 4, np.zeros(64)), np.zeros(64))


def _tree(v):
    v = list(v)
    while len(v) > 1:
        v = [v[2 * i] + v[2 * i + 1] for i in range(len(v) // 2)]
    return v[0]


def test_lane_sums_are_balanced_trees(mmm, ctx):
    """group_sum<L> = balanced tree over adjacent pairs (what oracle/mmm_twin.c writes); wave_sum = xor-butterfly 32,16,...,1."""
    rng = np.random.default_rng(13)
    x = rng.normal(0, 1, 64 * 50) * 10.0 ** rng.uniform(-8, 8, 64 * 50)
    for op, L in ((5, 16), (6, 32), (7, 64)):
        ref = np.repeat([_tree(x[i:i + L]) for i in range(0, x.size, L)], L)
        _bits_equal(_dev(mmm, ctx, op, x), ref)
    ref = []
    for i in range(0, x.size, 64):
        t = x[i:i + 64].copy()
        off = 32
        while off:
            t = t + t[np.arange(64) ^ off]
            off >>= 1
        ref.append(t)
    _bits_equal(_dev(mmm, ctx, 8, x), np.concatenate(ref))


# ---- the functions that exist on the device only (dev_math.h), operations 11 .. 22 of mmm_debug_math: each against the claim its comment makes

OP_DIGAMMA, OP_RCP, OP_SQRT_POS, OP_LOG_POS, OP_LOG_TAB, OP_DIGAMMA_TAB, OP_XLOGX = 11, 12, 13, 14, 15, 16, 17
OP_WAVE_MAX, OP_WAVE_MAX_DPP, OP_ROWS_SUM4, OP_BCAST, OP_READLANE_SUM = 18, 19, 20, 21, 22


def _ulp_distance(x, y):
    """number of doubles between x and y (finite, same sign)"""
    x = np.ascontiguousarray(x, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
    assert np.isfinite(x).all() and np.isfinite(y).all() and (np.signbit(x) == np.signbit(y)).all()
    return np.abs(x.view(np.int64) - y.view(np.int64))


def _scaled(rng, n, e_lo, e_hi):
    """m 2^e, m uniform in [1, 2), e uniform in e_lo .. e_hi"""
    return np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(e_lo, e_hi + 1, n))


def _three(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def _worst_ulp_mp(xs, ys, fn):
    """largest |y - fn(x)| in units of the spacing of doubles at fn(x), fn evaluated to 40 digits"""
    import mpmath as mp
    mp.mp.dps = 40
    worst = 0.0
    for x, y in zip(xs, ys):
        t = fn(mp.mpf(float(x)))
        worst = max(worst, float(abs(mp.mpf(float(y)) - t) / mp.mpf(float(np.spacing(abs(float(t)))))))
    return worst


def test_rcp_within_one_ulp(mmm, ctx):
    """dev_rcp, the LDA E-step's only quotient: "1/x to <= 1 ulp" over +-[2^-1000, 2^1000], exact powers of two and their neighbours included"""
    rng = np.random.default_rng(31)
    pw = _three(np.ldexp(1.0, np.arange(-1000, 1001)))
    x = np.concatenate([_scaled(rng, 200000, -1000, 999), pw])
    x = np.concatenate([x, -x])
    got = _dev(mmm, ctx, OP_RCP, x)
    d = _ulp_distance(got, 1.0 / x)
    print("\ndev_rcp: largest distance to 1.0 / x %d ulp (%d of %d values differ)" % (d.max(), (d > 0).sum(), x.size))
    assert d.max() <= 1, (x[np.argmax(d)], d.max())


def test_division_and_sqrt_over_the_exponent_range(mmm, ctx):
    """dev_sqrt_pos, dev_sqrt and dev_div are correctly rounded wherever every intermediate of their sequences is normal: operands (and the
    quotient) anywhere in [2^-900, 2^900], not only in the 1e-12 .. 1e12 of the MMA step; perfect squares and their neighbours."""
    rng = np.random.default_rng(32)
    k = rng.integers(1, 1 << 26, 20000).astype(np.float64)
    sq = np.ldexp(k * k, 2 * rng.integers(-449, 420, 20000))          # k^2 < 2^52 is exact; 4^j keeps it a perfect square, within [2^-898, 2^890]
    pw = np.ldexp(1.0, np.arange(-900, 901))
    x = np.concatenate([_scaled(rng, 200000, -900, 899), _three(sq), pw, np.nextafter(pw[:-1], np.inf), np.nextafter(pw[1:], 0.0)])
    assert x.min() >= np.ldexp(1.0, -900) and x.max() <= np.ldexp(1.0, 900)
    ref = np.sqrt(x)
    assert np.array_equal(ref[200000 + 20000:200000 + 40000] ** 2, sq)
    _bits_equal(_dev(mmm, ctx, OP_SQRT_POS, x), ref)
    _bits_equal(_dev(mmm, ctx, 4, x), ref)
    ea, eb = rng.integers(-900, 900, 400000), rng.integers(-900, 900, 400000)
    keep = np.abs(ea - eb) <= 898                                      # the quotient of the mantissas lies in (1/2, 2)
    ea, eb = ea[keep][:200000], eb[keep][:200000]
    a = np.ldexp(rng.uniform(1.0, 2.0, ea.size), ea) * rng.choice([-1.0, 1.0], ea.size)
    b = np.ldexp(rng.uniform(1.0, 2.0, ea.size), eb) * rng.choice([-1.0, 1.0], ea.size)
    q = a / b
    assert ea.size > 100000 and np.abs(q).min() >= np.ldexp(1.0, -900) and np.abs(q).max() <= np.ldexp(1.0, 900)
    _bits_equal(_dev(mmm, ctx, 3, a, b), q)


def _log_arguments(rng):
    """the argument sets of test_exp_log_digamma_bits' log part; 1 +- 2^-k; both sides of sqrt(1/2) 2^e, where dev_log_pos' reduction switches"""
    k = np.arange(1, 53)
    c = np.ldexp(0.70710678118654752440, np.arange(-1020, 1021, 40))
    edges = np.concatenate([1.0 + np.ldexp(1.0, -k), 1.0 - np.ldexp(1.0, -k), _three(c)])
    sets = [rng.uniform(1e-7, 30, 200000), 10.0 ** rng.uniform(-300, 300, 20000), 1.0 + rng.normal(0, 1e-6, 2000)]
    return edges, sets


def test_log_pos_below_two_ulp(mmm, ctx):
    """dev_log_pos (the ll term of lda_chunk; dev_log_tab's subnormal branch): "error < 2 ulp", on 3000 points against 40-digit values.  Over the
    whole sets against numpy's log, whose own error is below 1 ulp: below 3."""
    import mpmath as mp
    rng = np.random.default_rng(33)
    edges, sets = _log_arguments(rng)
    n_each = (3000 - edges.size) // 3
    pts = np.concatenate([edges] + [s[:n_each] for s in sets])
    assert 2900 < pts.size <= 3000
    worst = _worst_ulp_mp(pts, _dev(mmm, ctx, OP_LOG_POS, pts), mp.log)
    xs = np.concatenate(sets)
    ref = np.log(xs)
    wide = np.max(np.abs(_dev(mmm, ctx, OP_LOG_POS, xs) - ref) / np.spacing(np.abs(ref)))
    print("\ndev_log_pos: %.3f ulp against mpmath on %d points, %.3f ulp against numpy's log on %d" % (worst, pts.size, wide, xs.size))
    assert worst < 2.0, worst
    assert wide < 3.0, wide


def test_log_tab_every_input(mmm, oracle, ctx):
    """dev_log_tab, the log of every dense log-likelihood sweep.  Normal x > 0: the bits of ar_log_tab (the twin).  Everything else as log():
    +-0 -> -inf, x < 0 -> NaN, subnormals within 2 ulp (through dev_log_pos), NaN of either sign -> NaN, +inf -> +inf -- a NaN or infinite
    probability must not come out of a sweep as a finite log-likelihood."""
    import mpmath as mp
    rng = np.random.default_rng(34)
    L = oracle.lib()
    edges, sets = _log_arguments(rng)
    xs = np.concatenate(sets + [edges, [1.0, 2.0, 0.5, 1e-7, 2.2250738585072014e-308, np.finfo(np.float64).max]])
    ref = np.empty_like(xs); L.orc_ar_logtab_vec(xs.size, xs, ref)
    _bits_equal(_dev(mmm, ctx, OP_LOG_TAB, xs), ref)
    got = _dev(mmm, ctx, OP_LOG_TAB, np.array([0.0, -0.0]))
    assert np.isneginf(got).all(), got
    neg = np.concatenate([-xs[:2000], -(10.0 ** rng.uniform(-323, -308, 100)), [-5e-324, -np.finfo(np.float64).max, -np.inf]])
    got = _dev(mmm, ctx, OP_LOG_TAB, neg)
    assert np.isnan(got).all(), (neg[~np.isnan(got)][:3], got[~np.isnan(got)][:3])
    sub = np.concatenate([10.0 ** rng.uniform(-323, -308, 1000), [5e-324, 1e-323, 2.2250738585072009e-308]])
    worst = _worst_ulp_mp(sub, _dev(mmm, ctx, OP_LOG_TAB, sub), mp.log)
    print("\ndev_log_tab on %d subnormal and smallest normal arguments: %.3f ulp against mpmath" % (sub.size, worst))
    assert worst < 2.0, worst
    nans = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001, 0x7fffffffffffffff, 0xffffffffffffffff],
                    dtype=np.uint64).view(np.float64)                              # NaN of either sign, quiet or signalling, any payload
    got = _dev(mmm, ctx, OP_LOG_TAB, nans)
    assert np.isnan(nans).all() and np.isnan(got).all(), got
    got = _dev(mmm, ctx, OP_LOG_TAB, np.array([np.inf]))
    assert got[0] == np.inf, got


def test_digamma_tab_bits(mmm, oracle, ctx):
    """ar_digamma_pos_tab on the device (the LDA dense-row prologue) against the twin, bit for bit, on the arguments at which tests/test_twin_cpu.py
    measures the twin against mpmath: every boundary of the log table +- 1 ulp seen through x + 7, and 10^-1.5 .. 10^5."""
    rng = np.random.default_rng(35)
    L = oracle.lib()
    y = _three(np.ldexp(1.0 + np.repeat(np.arange(128), 16) / 128.0, np.tile(np.arange(2, 18), 128)))
    xs = np.concatenate([y[y - 7.0 > 1e-3] - 7.0, 10.0 ** rng.uniform(-1.5, 5, 100000)])
    ref = np.empty_like(xs); L.orc_ar_digammatab_vec(xs.size, xs, ref)
    _bits_equal(_dev(mmm, ctx, OP_DIGAMMA_TAB, xs), ref)


def _digamma_restated(x):
    """dev_digamma's general branch for x < 0 in numpy, operation by operation (libm's tan and log, IEEE division, no fma)"""
    x = np.asarray(x, dtype=np.float64)
    psi = 0.0 - np.pi / np.tan(np.pi * x)
    x = 1.0 - x
    n = np.where(x < 7.0, 7.0 - np.floor(x), 0.0)
    for v in range(1, 7):
        psi = psi - np.where(v < n, 1.0 / (x + v), 0.0)
    psi = psi - np.where(n > 0, 1.0 / x, 0.0)
    x = x + n
    t = 1.0 / x
    s = np.log(x) - 0.5 * t
    t = t * t
    p = np.full_like(x, -0.4432598039215686)
    for c in (0.08333333333333333, -0.021092796092796094, 0.007575757575757576, -0.004166666666666667, 0.003968253968253968, -0.008333333333333333,
              0.08333333333333333):
        p = p * t + c
    return psi + (s - t * p)


def test_digamma_general_branch(mmm, oracle, ctx):
    """dev_digamma outside (0, 1e40), where it does not go to ar_digamma_pos: x >= 1e40 at the project's digamma bound (1e-13 relative to mpmath);
    +inf, NaN, 0; x < 0 through the reflection, measured as |err| / (|psi(x)| + |pi cot(pi x)| + 1) -- psi has a zero in every unit interval
    and the reflection term carries the error -- against a numpy restatement of the same algorithm: the restatement stays below 1e-13 and the
    device below four times the restatement's own value (tan, log and up to seven reciprocals may each differ from libm by an ulp or two).
    Inside (0, 1e40), beyond the range already checked: the bits of the twin's ar_digamma_pos."""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(36)
    xs = 10.0 ** rng.uniform(40, 307, 1000)
    got = _dev(mmm, ctx, OP_DIGAMMA, xs)
    rel = max(abs(float((mp.mpf(float(y)) - mp.digamma(mp.mpf(float(x)))) / mp.digamma(mp.mpf(float(x))))) for x, y in zip(xs, got))
    print("\ndev_digamma, x >= 1e40: %.3g relative to mpmath" % rel)
    assert rel <= 1e-13, rel
    got = _dev(mmm, ctx, OP_DIGAMMA, np.array([np.inf, np.nan, 0.0]))
    assert got[0] == np.inf and np.isnan(got[1]) and got[2] == -np.inf, got
    xs = rng.uniform(-50, 0, 6000)
    xs = xs[np.abs(xs - np.rint(xs)) >= 1.0 / 16][:3000]
    assert xs.size == 3000
    got = _dev(mmm, ctx, OP_DIGAMMA, xs)
    res = _digamma_restated(xs)
    e_dev = e_res = 0.0
    for x, y, z in zip(xs, got, res):
        xm = mp.mpf(float(x))
        t = mp.digamma(xm)
        scale = abs(t) + abs(mp.pi * mp.cot(mp.pi * xm)) + 1
        e_dev = max(e_dev, float(abs(mp.mpf(float(y)) - t) / scale))
        e_res = max(e_res, float(abs(mp.mpf(float(z)) - t) / scale))
    print("dev_digamma, -50 < x < 0: device %.3g, numpy restatement %.3g (|err| / (|psi| + |pi cot pi x| + 1))" % (e_dev, e_res))
    assert e_res <= 1e-13, e_res
    assert e_dev <= 4.0 * e_res, (e_dev, e_res)
    xs = np.concatenate([10.0 ** rng.uniform(-300, -7, 20000), 10.0 ** rng.uniform(8, 39.9, 20000)])
    ref = np.empty_like(xs); oracle.lib().orc_ar_digamma_vec(xs.size, xs, ref)
    _bits_equal(_dev(mmm, ctx, OP_DIGAMMA, xs), ref)


def test_xlogx(mmm, ctx):
    """dev_xlogx of the ELBO's E ln q(z) sums: 0 -> 0 (the reference's 0^0 = 1 in log(x^x)), x log x at the bounds this file holds log to
    (4e-16 relative, 1e-18 absolute near x = 1) against mpmath, and NaN -> NaN: log(x^x) of a NaN is a NaN in the reference."""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(37)
    assert (_dev(mmm, ctx, OP_XLOGX, np.zeros(64)).view(np.int64) == 0).all()
    xs = np.concatenate([10.0 ** rng.uniform(-300, 300, 2400), 1.0 + rng.normal(0, 1e-6, 500), rng.uniform(1e-7, 1.0, 96), [1e-300, 1e300, 1.0, 0.5]])
    got = _dev(mmm, ctx, OP_XLOGX, xs)
    worst = 0.0
    for x, y in zip(xs, got):
        t = mp.mpf(float(x)) * mp.log(mp.mpf(float(x)))
        worst = max(worst, float(abs(mp.mpf(float(y)) - t) / (mp.mpf(1e-18) + mp.mpf(4e-16) * abs(t))))
    print("\ndev_xlogx: largest error %.3f of the bound 1e-18 + 4e-16 |x log x|" % worst)
    assert worst <= 1.0, worst
    got = _dev(mmm, ctx, OP_XLOGX, np.array([np.nan, np.copysign(np.nan, -1.0)]))
    assert np.isnan(got).all(), got


def _per_wave(fn, x):
    return np.concatenate([np.full(64, fn(x[i:i + 64])) for i in range(0, x.size, 64)])


def test_wave_max_both_builds(mmm, ctx):
    """wave_max (xor butterfly) and wave_max_dpp (four DPP stages inside the 16-lane rows, then the row swaps; the pivot search of every
    Gauss-Jordan build): the largest of each 64 values in every lane.  The pivot pattern -- the sentinel -1 everywhere but in lane w of wave w --
    makes a stage that misses one source lane fail exactly one wave; NaN lanes are dropped as by fmax."""
    rng = np.random.default_rng(38)
    rand = rng.normal(0, 1, 64 * 50) * 10.0 ** rng.uniform(-8, 8, 64 * 50)
    equal = np.concatenate([np.full(64, 3.7), np.full(64, -2.5e-300)])
    inf = np.concatenate([np.where(np.arange(64) == 41, np.inf, rand[:64]), np.full(64, -np.inf), np.where(np.arange(64) == 17, -1e308, -np.inf),
                          np.where(np.arange(64) == 62, 0.0, -np.abs(rand[64:128])), np.where(np.arange(64) == 33, -0.0, -np.abs(rand[64:128]) - 1e-300)])
    val = np.abs(rng.normal(0, 1, 64)) * 10.0 ** rng.uniform(-300, 300, 64)
    pivot = np.full((64, 64), -1.0); pivot[np.arange(64), np.arange(64)] = val
    two = pivot.copy(); two[np.arange(64), (np.arange(64) * 7 + 13) % 64] = val
    assert ((np.arange(64) * 7 + 13) % 64 != np.arange(64)).all()
    x = np.concatenate([rand, equal, inf, pivot.ravel(), two.ravel()])
    ref = _per_wave(np.max, x)
    for op in (OP_WAVE_MAX, OP_WAVE_MAX_DPP):
        got = _dev(mmm, ctx, op, x)
        assert np.array_equal(got, ref), (op, np.flatnonzero(got != ref)[:5] // 64)
        zero = ref == 0.0
        assert np.array_equal(np.signbit(got[zero]), np.signbit(ref[zero]))       # (each of these waves holds one zero)
    neg0 = np.full(64, -0.0)
    for op in (OP_WAVE_MAX, OP_WAVE_MAX_DPP):
        got = _dev(mmm, ctx, op, neg0)
        assert (got == 0.0).all() and np.signbit(got).all(), got
    # quiet NaNs in a few lanes: dropped (fmax); a wave of nothing but NaN gives NaN
    xn = rand[:64 * 20].copy()
    xn[rng.choice(xn.size, 60, replace=False)] = np.nan
    xn[64 * 3:64 * 4] = -1.0; xn[64 * 3 + 9] = np.nan; xn[64 * 3 + 40] = 2.5          # the pivot pattern with a NaN beside it
    xn[64 * 5:64 * 6] = np.nan; xn[64 * 5 + 63] = -7.0                                 # one number among 63 NaNs
    xn = np.concatenate([xn, np.full(64, np.nan)])
    ref = _per_wave(np.fmax.reduce, xn)
    assert np.isnan(ref[-64:]).all() and not np.isnan(ref[:-64]).any()
    for op in (OP_WAVE_MAX, OP_WAVE_MAX_DPP):
        got = _dev(mmm, ctx, op, xn)
        assert np.array_equal(got, ref, equal_nan=True), (op, np.flatnonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:5] // 64)


def test_rows_sum4_association(mmm, ctx):
    """rows_sum4: lane i ends with (x[j] + x[j + 32]) + (x[j + 16] + x[j + 48]), j = i % 16 -- "(row 0 + row 2) + (row 1 + row 3)" -- in all 64 lanes;
    sixteen decades of spread, so that another association changes bits"""
    rng = np.random.default_rng(39)
    x = rng.normal(0, 1, 64 * 50) * 10.0 ** rng.uniform(-8, 8, 64 * 50)
    w = x.reshape(-1, 4, 16)
    ref = np.tile((w[:, 0] + w[:, 2]) + (w[:, 1] + w[:, 3]), (1, 4)).ravel()
    other = np.tile((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]), (1, 4)).ravel()
    assert (ref.view(np.int64) != other.view(np.int64)).mean() > 0.2                   # the data can tell the associations apart
    _bits_equal(_dev(mmm, ctx, OP_ROWS_SUM4, x), ref)


def test_readlane_sum_and_broadcast(mmm, ctx):
    """wave_readlane: s = 0; s += lane j's value for j = 0 .. 63 (k_align_normalise's index-order sum), the same bits in every lane.
    wave_bcast: out[i] = x[64 (i / 64) + lane] for a fixed lane and for an index that varies from lane to lane."""
    rng = np.random.default_rng(40)
    x = rng.normal(0, 1, 64 * 50) * 10.0 ** rng.uniform(-8, 8, 64 * 50)
    ref = []
    for i in range(0, x.size, 64):
        s = 0.0
        for j in range(64):
            s = s + float(x[i + j])
        ref.append(s)
    _bits_equal(_dev(mmm, ctx, OP_READLANE_SUM, x), np.repeat(ref, 64))
    base = 64 * (np.arange(x.size) // 64)
    lane = np.arange(x.size) % 64
    for idx in (np.zeros(x.size, dtype=np.int64), np.full(x.size, 37), np.full(x.size, 63), (lane * 5 + 3) % 64, 63 - lane, rng.integers(0, 64, x.size)):
        _bits_equal(_dev(mmm, ctx, OP_BCAST, x, idx.astype(np.float64)), x[base + idx])
