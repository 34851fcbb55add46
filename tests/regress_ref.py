"""numpy restatement of mmm_regress_exposures (include/mmmusig.h) and the cases its tests share.

Written from the header text: its own Philox4x32-10, np.lexsort for the two orders that make pi, every dot product as 16 explicit per-stripe
sequential loops over the slots (vectorised over the cells and over a batch of replicates, which changes no cell's order), the 16 stripe sums
added in ascending order from 0.0, rz, num and t in explicit loops from 0.0 -- every product, division and sum a separate numpy operation.  It
shares no code with the package.  `design` builds the inputs of the call (qz, e, w) with np.linalg.qr for the tests that hold the definition
to outside facts.

The header's limits make D = 1 unreachable (D - A - cols[c] >= 1 with cols[c] >= 1 needs D >= 2), so the table starts at D = 2 with A = 0 and
D = 1 is one of the refusals the device test checks."""
import functools
from collections import namedtuple

import numpy as np

BITS = 0xF0000000
M32 = np.uint64(0xFFFFFFFF)

RgOut = namedtuple("RgOut", "obs u_obs rz_obs ge ge_max maxstat")
RgOut.__doc__ = "obs [P, C], u_obs [P, Q], rz_obs [P] float64; ge, ge_max [P, C] uint32; maxstat [B, C] float64"


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def keys(D, bgs, seed, stream=0):
    """key_d, d < D, of the replicates with the GLOBAL indices bgs -> [len(bgs), D]"""
    bgs = np.asarray(bgs, np.uint64).reshape(-1)
    nb = (D + 3) // 4
    blk = np.broadcast_to(np.arange(nb, dtype=np.uint64)[None, :], (bgs.size, nb))
    z = np.zeros((bgs.size, nb), np.uint64)
    w = philox4x32_10(blk, z + np.uint64(BITS), z + bgs[:, None], z + np.uint64(stream), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return np.stack(w, axis=2).reshape(bgs.size, 4 * nb)[:, :D]


def permutations(D, strata, bgs, seed, stream=0):
    """pi [len(bgs), D]: pi(slot_j) = e_j"""
    s = np.zeros(D, np.int64) if strata is None else np.asarray(strata, np.int64)
    d = np.arange(D)
    slot = np.lexsort((d, s))                            # the last key is the primary one
    k = keys(D, bgs, seed, stream)
    pi = np.empty(k.shape, np.int64)
    for r in range(k.shape[0]):
        pi[r, slot] = np.lexsort((d, k[r], s))
    return pi


def permutation(D, strata, bg, seed, stream=0):
    return permutations(D, strata, [bg], seed, stream)[0]


def stripe_dot(F, G):
    """dot(F[.][r], G[..., ., p]) for every (r, p) in the stripe order: F [D, R], G [..., D, P] -> [..., R, P]"""
    D = F.shape[0]
    sums = []
    for s in range(16):
        acc = np.zeros(G.shape[:-2] + (F.shape[1], G.shape[-1]))
        for i in range(s, D, 16):
            prod = F[i][:, None] * G[..., i, None, :]
            acc = acc + prod
        sums.append(acc)
    tot = np.zeros_like(sums[0])
    for s in range(16):
        tot = tot + sums[s]
    return tot


def statistic(qz, w, col0, ss, Ep):
    """Ep [..., D, P]: the residual rows the slots received -> t [..., P, C], u [..., P, Q], rz [..., P]"""
    A = qz.shape[1]
    a = stripe_dot(qz, Ep)                               # [..., A, P]
    u = stripe_dot(w, Ep)                                # [..., Q, P]
    fit = np.zeros(Ep.shape[:-2] + (Ep.shape[-1],))
    for j in range(A):
        sq = a[..., j, :] * a[..., j, :]
        fit = fit + sq
    rz = ss - fit
    C = len(col0) - 1
    t = np.zeros(Ep.shape[:-2] + (Ep.shape[-1], C))
    for c in range(C):
        num = np.zeros_like(rz)
        for q in range(col0[c], col0[c + 1]):
            sq = u[..., q, :] * u[..., q, :]
            num = num + sq
        with np.errstate(invalid="ignore", divide="ignore"):
            t[..., c] = np.where(rz > 0, num / rz, 0.0)
    return t, np.swapaxes(u, -1, -2), rz


def regress(e, qz, cols, w, strata, B, b0, seed, stream=0, batch=256):
    e = np.asarray(e, np.float64)
    D, P = e.shape
    qz = np.zeros((D, 0)) if qz is None else np.asarray(qz, np.float64).reshape(D, -1)
    w = np.asarray(w, np.float64)
    col0 = [0] + [int(v) for v in np.cumsum(cols)]
    C = len(cols)
    ss = np.zeros(P)
    for p in range(P):
        ss[p] = stripe_dot(e[:, p:p + 1], e[:, p:p + 1])[0, 0]
    obs, u_obs, rz_obs = statistic(qz, w, col0, ss, e)
    ge, gm, ms = np.zeros((P, C), np.uint32), np.zeros((P, C), np.uint32), np.zeros((B, C))
    for lo in range(0, B, batch):
        hi = min(B, lo + batch)
        pi = permutations(D, strata, b0 + np.arange(lo, hi, dtype=np.int64), seed, stream)
        t, _, _ = statistic(qz, w, col0, ss, e[pi])      # slot i receives e[pi(i)]
        M = t.max(axis=-2)                               # [n, C]
        ge += (t >= obs[None]).sum(axis=0).astype(np.uint32)
        gm += (M[:, None, :] >= obs[None]).sum(axis=0).astype(np.uint32)
        ms[lo:hi] = M
    return RgOut(obs, u_obs, rz_obs, ge, gm, ms)


# ---- forming the inputs: midranks and an orthonormal design by QR ----------------------------------------------------------------------------
def midrank(v):
    """midranks #{less} + (#{equal} + 1) / 2, IEEE comparisons, by counting"""
    v = np.asarray(v, np.float64)
    return (v[None, :] < v[:, None]).sum(axis=1) + ((v[None, :] == v[:, None]).sum(axis=1) + 1) / 2.0


def indicators(codes):
    """G - 1 indicator columns of the levels 1 .. G-1 of integral codes 0 .. G-1"""
    codes = np.asarray(codes).astype(int)
    return np.stack([(codes == g).astype(np.float64) for g in range(1, codes.max() + 1)], axis=1)


def design(x, Z, covs):
    """x [D, P] features; Z [D, A] adjuster columns with the intercept first, or None; covs: a list of [D, k] column blocks, one per tested
    covariate -> e [D, P], qz [D, A], cols, w [D, Q]"""
    x = np.asarray(x, np.float64)
    D = x.shape[0]
    qz = np.zeros((D, 0)) if Z is None else np.linalg.qr(np.asarray(Z, np.float64))[0]
    res = lambda m: m - qz @ (qz.T @ m)
    e = res(res(x))
    ws = [np.linalg.qr(res(res(np.asarray(b, np.float64).reshape(D, -1))))[0] for b in covs]
    return e, qz, [b.shape[1] for b in ws], np.concatenate(ws, axis=1)


def orthobasis(rng, D, n):
    """n orthonormal columns of a random [D, n] matrix"""
    return np.linalg.qr(rng.standard_normal((D, n)))[0]


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name e qz cols w strata B b0 seed")


def draw(D, P, A, cols, seed):
    """residuals that are orthogonal to qz only up to rounding, a design that is orthonormal: what a caller would pass"""
    rng = np.random.default_rng(seed)
    Q = int(sum(cols))
    basis = orthobasis(rng, D, min(D, A + Q))
    if basis.shape[1] < A + Q:                           # more columns than samples cannot be orthonormal: the formulas are the contract
        basis = np.concatenate([basis, rng.standard_normal((D, A + Q - basis.shape[1])) / np.sqrt(D)], axis=1)
    qz, w = basis[:, :A], basis[:, A:]
    x = rng.standard_normal((D, P))
    e = x - qz @ (qz.T @ x)
    return e, qz, w


def cases():
    out = []

    def add(name, D, P, A, cols, B, strata=None, b0=0, seed=None, inputs=None):
        e, qz, w = inputs if inputs is not None else draw(D, P, A, cols, 300 + len(out))
        out.append(Case(name, e, qz if A else None, tuple(cols), w, None if strata is None else np.asarray(strata, np.int32), B, b0, 11 + len(out) if seed is None else seed))

    add("D2", 2, 2, 0, [1], 5, b0=2)
    for D in (15, 16, 17, 63, 64, 65, 257):
        add("D%d" % D, D, 3, 2, [1, 2, 1], 5, b0=D)
    add("D4096", 4096, 2, 1, [1], 4)                     # the rows do not fit LDS
    add("P1", 20, 1, 1, [1], 6)
    add("P33", 20, 33, 1, [1, 2, 1], 6)
    add("P64", 40, 64, 3, [1], 4)
    add("A0", 12, 2, 0, [1, 2, 1], 8)
    add("A32", 70, 3, 32, [1, 2, 1], 5)
    add("Q64", 100, 3, 2, [31, 33], 3)
    add("ones64", 80, 5, 1, [1] * 64, 3)
    add("full", 257, 64, 32, [31, 33], 2)                # every limit but D at once: 4 x 4 tiles, rows in memory
    # contents: an all-zero residual column, a w column of zeros, residuals that are not orthogonal to qz, a fully explained feature
    D = 40
    e, qz, w = draw(D, 4, 2, [1, 2, 1], 78)
    e[:, 1] = 0.0
    w[:, 2] = 0.0
    e[:, 2] += 0.75 * qz[:, 1] + 0.25 * qz[:, 0]         # the formula, not the intent, is the contract
    e[:, 3] = 1.5 * qz[:, 0] - 0.5 * qz[:, 1]            # rz is rounding noise of either sign
    add("contents", D, 4, 2, [1, 2, 1], 40, inputs=(e, qz, w))
    # rz <= 0 for certain: the same column twice in qz counts the fitted part of feature 0 twice
    e, qz, w = draw(D, 3, 2, [1, 2], 79)
    qz[:, 1] = qz[:, 0]
    e[:, 0] = 3.0 * qz[:, 0] + 0.125 * e[:, 0]
    add("rzneg", D, 3, 2, [1, 2], 20, inputs=(e, qz, w))
    add("onestratum", 30, 3, 2, [1, 2], 10, strata=np.full(30, 5))
    add("allalone", 30, 3, 2, [1, 2], 10, strata=np.arange(30)[::-1])
    add("sizes", 64, 3, 2, [1, 2], 12, strata=[2] + [0, 0] + [1] * 61)
    add("unordered", 41, 3, 1, [1, 1, 2], 12, strata=np.random.default_rng(9).integers(0, 4, size=41)[::-1] * 10)
    add("many", 5, 2, 1, [1, 2], 3000)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, b0, B):
    c = next(v for v in cases() if v.name == name)
    return regress(c.e, c.qz, c.cols, c.w, c.strata, B, b0, c.seed)


def reference(c, b0=None, B=None):
    """computed once per (case, b0, B) and shared; do not modify the result"""
    return _reference(c.name, c.b0 if b0 is None else b0, c.B if B is None else B)


# ---- planted and confounded inputs ---------------------------------------------------------------------------------------------------------------
PLANTED_SEED, PLANTED_B = 4, 999
CONFOUNDED_D, CONFOUNDED_B = 60, 199


def planted(seed=PLANTED_SEED):
    """D = 120, P = 6, adjuster age.  age drives the features 0 .. 2; feature 0 is shifted between the two groups of grp, feature 1 goes with num;
    batch (three levels) is noise; conf = 1.5 age + noise goes with the features 0 .. 2 only through age -> x, dict of tested columns, age, the
    planted (feature, covariate) pairs"""
    rng = np.random.default_rng(seed)
    D = 120
    age = rng.standard_normal(D)
    grp = rng.integers(0, 2, size=D)
    num = rng.standard_normal(D)
    batch = rng.integers(0, 3, size=D)
    conf = 1.5 * age + rng.standard_normal(D)
    x = rng.standard_normal((D, 6))
    x[:, :3] += age[:, None]
    x[:, 0] += 1.6 * grp
    x[:, 1] += 1.2 * num
    return x, {"grp": grp, "num": num, "batch": batch, "conf": conf}, age, [(0, 0), (1, 1)]


def planted_inputs(adjusted=True, seed=PLANTED_SEED):
    """the call's inputs under ranks=True: midranks of the features, of the numeric tested columns and of age"""
    x, cov, age, _ = planted(seed)
    D = x.shape[0]
    rx = np.stack([midrank(x[:, p]) for p in range(x.shape[1])], axis=1)
    Z = np.stack([np.ones(D), midrank(age)], axis=1) if adjusted else np.ones((D, 1))
    blocks = [indicators(cov["grp"]), midrank(cov["num"])[:, None], indicators(cov["batch"]), midrank(cov["conf"])[:, None]]
    return design(rx, Z, blocks)


@functools.lru_cache(maxsize=None)
def planted_reference(adjusted=True):
    e, qz, cols, w = planted_inputs(adjusted)
    return regress(e, qz, cols, w, None, PLANTED_B, 0, 1000 + PLANTED_SEED)


def confounded(seed):
    """a null cohort of D = 60: the adjuster drives the feature and the tested covariate, which are independent given it -> x [D, 1], v, age"""
    rng = np.random.default_rng(seed)
    age = rng.standard_normal(CONFOUNDED_D)
    x = (age + rng.standard_normal(CONFOUNDED_D))[:, None]
    v = age + rng.standard_normal(CONFOUNDED_D)
    return x, v, age


def confounded_inputs(seed, adjusted=True):
    """the plain linear model on the values (ranks=False)"""
    x, v, age = confounded(seed)
    Z = np.stack([np.ones(CONFOUNDED_D), age], axis=1) if adjusted else np.ones((CONFOUNDED_D, 1))
    return design(x, Z, [v[:, None]])
