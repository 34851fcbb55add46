"""The definitions of mmm_simulate_counts / mmm_fit_check as their numpy restatement computes them (tests/simulate_ref.py): the integer
thresholds, the draws, the separation of their random words from the resampler's and the split's, and -- on the planted corpus the GPU test
then uses -- that the p-values tell a contaminated sample from a clean one.  The header and the binding declare both entries."""
import os
import re

import numpy as np

import bootstrap_ref
import select_ref
import simulate_ref as S
from simulate_ref import DRAW_SEED, PLANTED_B, PLANTED_SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thresholds_are_monotone_end_at_two_to_32_and_stay_across_zero_terms():
    pi, T, S_ = S.thresholds(np.asarray([0, 0, 0.5, 0, 0.25, 0.25, 0, 0]))
    assert T.tolist() == [0, 0, 2 ** 31, 2 ** 31, 3 * 2 ** 30, 2 ** 32, 2 ** 32, 2 ** 32] and S_ == 1.0
    assert pi.tolist() == [0, 0, 0.5, 0, 0.25, 0.25, 0, 0]
    _, T, _ = S.thresholds(np.asarray([1.0, 1e-20, 1e-20]))
    assert T.tolist() == [2 ** 32] * 3
    rng = np.random.default_rng(3)
    for V in (1, 5, 96, 1536):
        p = rng.gamma(0.3, size=V) * 7.0
        p[rng.random(V) < 0.3] = 0.0
        p[V // 2] = 1.0
        _, T, _ = S.thresholds(p)
        assert (np.diff(T.astype(np.int64)) >= 0).all() and int(T[-1]) == 2 ** 32
        Tprev = np.concatenate([[0], T[:-1]])
        assert (T[p == 0] == Tprev[p == 0]).all()


def test_the_extreme_words_land_on_terms_with_positive_probability():
    for p in ([0, 0, 0.5, 0, 0.25, 0.25, 0, 0], [1.0, 1e-20, 1e-20], [0.0, 3.0], [2.0, 0.0], [1e-300, 1.0, 0.0]):
        p = np.asarray(p, dtype=np.float64)
        _, T, _ = S.thresholds(p)
        v = S.land(T, np.asarray([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.uint64))
        assert (p[v] > 0).all(), (p, v)
    assert S.land(S.thresholds(np.asarray([0, 0, 0.5, 0, 0.25, 0.25, 0, 0]))[1], [0, 2 ** 31 - 1, 2 ** 31, 3 * 2 ** 30 - 1, 3 * 2 ** 30, 2 ** 32 - 1]).tolist() == \
        [2, 2, 4, 4, 5, 5]
    assert S.land(S.thresholds(np.asarray([1.0, 1e-20, 1e-20]))[1], [0, 2 ** 32 - 1]).tolist() == [0, 0]


def test_every_simulated_row_sums_to_its_total_and_a_zero_term_is_never_drawn():
    dp, term, count, props, phi, zero = S.edge_corpus(96, 3)
    n_doc = np.asarray([int(count[dp[d]:dp[d + 1]].sum()) for d in range(len(dp) - 1)])
    out = S.simulate(props, phi, n_doc, 5, b0=7, seed=11, stream=2)
    assert out.shape == (5, len(n_doc), 96) and np.array_equal(out.sum(axis=2), np.tile(n_doc, (5, 1)))
    assert zero.sum() >= 3 and not out[:, :, zero].any() and (out >= 0).all()
    assert np.array_equal(out[2:4], S.simulate(props, phi, n_doc, 2, b0=9, seed=11, stream=2))         # a slice of the big call
    assert not np.array_equal(out[0, 0], out[1, 0])


def test_words_differ_from_the_resamplers_and_the_splits():
    seed, d, b, stream, N = 5, 3, 2, 1, 64
    nblk = N // 4
    z = np.zeros(nblk, np.uint64)
    ours = S.words(N, d, b, seed, stream)[0]
    theirs = np.stack(bootstrap_ref.philox4x32_10(np.arange(nblk, dtype=np.uint64), z + np.uint64(d), z + np.uint64(b), z + np.uint64(stream), seed, 0),
                      axis=1).ravel()           # the block of bootstrap_ref.resample_doc(count, d, b, seed, stream)
    split = select_ref.fold_words(N, d, b, seed, stream)
    assert ours.shape == theirs.shape == split.shape == (N,)
    assert not np.intersect1d(ours, theirs).size and not np.intersect1d(ours, split).size and not np.intersect1d(theirs, split).size
    cnt = np.full(8, 8)
    rs = bootstrap_ref.resample_doc(cnt, d, b, seed, stream)
    mine = S.simulate_doc(S.thresholds(cnt.astype(np.float64))[1], N, d, b, seed, stream)[0]
    assert rs.sum() == mine.sum() == N and not np.array_equal(rs, mine)
    # the counter differs in the high bit of the third word only: the same block once that bit is set by hand
    same = np.stack(bootstrap_ref.philox4x32_10(np.arange(nblk, dtype=np.uint64), z + np.uint64(d), z + np.uint64(b | 0x80000000), z + np.uint64(stream), seed, 0),
                    axis=1).ravel()
    assert np.array_equal(ours, same)


def test_statistics_by_hand():
    pi = np.asarray([0.5, 0.25, 0.25, 0.0])
    cos, chi = S.statistics(np.asarray([[2, 1, 1, 0], [4, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0]]), pi, 4)
    assert abs(cos[0] - 1.0) < 4e-16 and chi[0] == 0.0          # n = N pi: the cosine is 1 to the rounding of two square roots
    assert chi[1] == 4.0 and abs(cos[1] - 0.5 / np.sqrt(0.375)) < 1e-15
    assert np.isinf(chi[2]) and chi[2] > 0 and cos[3] == 0.0
    assert S.statistics(np.zeros(4), pi, 0) == (0.0, 0.0)
    x = np.random.default_rng(0).random(130)
    assert abs(S.wave_sum(x) - x.sum()) < 1e-12 and S.wave_sum(np.arange(65.0)) == 2080.0


def test_planted_contamination_is_flagged_and_clean_samples_are_not():
    """what tests/test_simulate_gpu.py relies on when it asks the device for the same flags: with B = 199 every contaminated document has
    both counts 0 (p = 1 / 200) and at most 2 of the 12 clean ones have p_chi2 <= 0.05"""
    dp, term, count, props, phi, bad = S.planted(PLANTED_SEED)
    assert bad.sum() == 12 and (~bad).sum() == 12 and props.shape == (24, 5) and phi.shape == (5, 96)
    r = S.fit_check(dp, term, count, props, phi, PLANTED_B, seed=DRAW_SEED)
    assert not r["cos_le"][bad].any() and not r["chi_ge"][bad].any()
    p_chi = (1.0 + r["chi_ge"]) / (PLANTED_B + 1.0)
    assert (p_chi[~bad] <= 0.05).sum() <= 2
    assert np.isfinite(r["chi_rep"]).all() and (r["cos_rep"] > 0).all() and (r["cos_rep"] <= 1).all()
    # the raw cosine does not separate them: some contaminated sample reconstructs better than some clean one
    assert r["cos_obs"][bad].max() > r["cos_obs"][~bad].min()


def test_header_and_binding_declare_both_entries(mmm):
    hdr = open(os.path.join(ROOT, "include", "mmmusig.h")).read()
    for name in ("mmm_simulate_counts", "mmm_fit_check"):
        assert re.search(r"\bint %s\(mmm_ctx\* ctx," % name, hdr), name
        assert name in mmm._lib.declared_symbols()
    assert "0x80000000 | b" in hdr and "#define MMM_VERSION 123" in hdr
    assert {"simulate_counts", "goodness_of_fit", "FitCheck"} <= set(mmm.__all__)
