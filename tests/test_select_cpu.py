"""The held-out selection definitions without a GPU: the properties of the numpy restatement of the split (tests/select_ref.py) that the
device is then held to integer for integer (tests/test_select_gpu.py), the one-standard-error rule and the hold-out arithmetic."""
import numpy as np
import pytest

import bootstrap_ref as br
import np_ref
import select_ref as sr


def _corpus():
    X, _ = np_ref.synth_lda(40, 96, 6, seed=31, mean_n=400)
    X = [x.copy() for x in X]
    X[3][2, 1] = 0                       # an entry with count 0, added by hand
    return X


def test_restated_split_partitions_every_entry():
    X = _corpus()
    c = np.concatenate([x[:, 1] for x in X])
    for F in (1, 2, 3, 16):
        parts = sr.split(X, F, 20260101)
        C = sr.counts_matrix(parts)
        assert C.shape == (F, c.size) and (C >= 0).all()
        assert np.array_equal(C.sum(axis=0), c)                                    # the folds of an entry sum to its count, exactly
        for part in parts:
            assert all(np.array_equal(p[:, 0], x[:, 0]) for p, x in zip(part, X))  # rows and terms kept, zero rows included
    assert np.array_equal(sr.counts_matrix(sr.split(X, 1, 5))[0], c)               # F = 1 returns the counts
    # the folds are near-equal shares: fold sizes of the whole corpus within 5 binomial standard deviations of N / F
    C = sr.counts_matrix(sr.split(X, 4, 20260101)).sum(axis=1)
    N = c.sum()
    assert np.abs(C - N / 4).max() < 5 * np.sqrt(N * 0.25 * 0.75)


def test_restated_split_is_deterministic_and_every_argument_enters():
    X = _corpus()[:6]
    base = sr.counts_matrix(sr.split(X, 3, 0x1234567800000005))
    assert np.array_equal(base, sr.counts_matrix(sr.split(X, 3, 0x1234567800000005)))
    for other in (sr.split(X, 3, 0x1234567800000006), sr.split(X, 3, 0x1234567900000005), sr.split(X, 3, 0x1234567800000005, rep=1),
                  sr.split(X, 3, 0x1234567800000005, stream=1)):
        assert not np.array_equal(base, sr.counts_matrix(other))


def test_split_words_are_not_the_resamplers():
    """the stream bit: at the same seed, document, replicate and stream a split draws other words than a resample"""
    N, d, seed = 1000, 3, 77
    nblk = (N + 3) // 4
    z = np.zeros(nblk, np.uint64)
    res = np.stack(br.philox4x32_10(np.arange(nblk, dtype=np.uint64), z + np.uint64(d), z, z, seed & 0xFFFFFFFF, seed >> 32), axis=1).ravel()[:N]
    spl = sr.fold_words(N, d, 0, seed, 0)
    assert (res == spl).mean() < 0.01
    # and the counter that differs is the fourth, in its high bit alone
    same = np.stack(br.philox4x32_10(np.arange(nblk, dtype=np.uint64), z + np.uint64(d), z, z + np.uint64(0x80000000), seed & 0xFFFFFFFF, seed >> 32),
                    axis=1).ravel()[:N]
    assert np.array_equal(same, spl)


def test_pick_k(mmm):
    pick_k = mmm.pick_k
    # a plateau: K = 4 has the highest mean, K = 3 lies within its standard error, K = 2 does not
    s = [[-2.10, -2.12, -2.11, -2.13], [-1.900, -1.910, -1.890, -1.900], [-1.800, -1.810, -1.790, -1.800], [-1.795, -1.805, -1.785, -1.825]]
    p = pick_k([1, 2, 3, 4], s)
    assert np.allclose(p.mean, np.mean(s, axis=1)) and np.allclose(p.se, np.std(s, axis=1, ddof=1) / 2)
    assert p.best == 3 and p.pick == 3
    s[3] = [-1.790, -1.800, -1.780, -1.820]                 # mean -1.7975 > -1.8, se 0.0085: K = 3 is within it
    p = pick_k([1, 2, 3, 4], s)
    assert p.best == 4 and p.pick == 3
    s[3] = [-1.700, -1.701, -1.699, -1.700]                 # a clear gain: nothing smaller is within a standard error
    p = pick_k([1, 2, 3, 4], s)
    assert p.best == 4 and p.pick == 4
    # ties go to the lowest K, whatever the order the candidates are given in
    p = pick_k([5, 2, 3], [[1.0, 1.0], [1.0, 1.0], [0.5, 0.5]])
    assert p.best == 2 and p.pick == 2
    # n = 1: se = 0, pick = best
    p = pick_k([2, 3, 4], [[-3.0], [-2.0], [-2.5]])
    assert np.array_equal(p.se, np.zeros(3)) and p.best == 3 and p.pick == 3
    # a NaN mean never wins
    p = pick_k([2, 3], [[np.nan, 1.0], [0.0, 0.1]])
    assert p.best == 3 and p.pick == 3
    with pytest.raises(ValueError):
        pick_k([2, 3], [[1.0, 2.0]])


def test_holdout_arithmetic(mmm):
    X = _corpus()[:5]
    parts = sr.split(X, 3, 9)
    for f in range(3):
        train, test = mmm.holdout(X, parts, f)
        assert all(np.array_equal(t, p) for t, p in zip(test, parts[f]))
        for x, tr, te in zip(X, train, test):
            assert np.array_equal(tr[:, 0], x[:, 0]) and np.array_equal(tr[:, 1] + te[:, 1], x[:, 1]) and (tr[:, 1] >= 0).all()
        others = sum(np.concatenate([p[:, 1] for p in parts[g]]) for g in range(3) if g != f)
        assert np.array_equal(np.concatenate([t[:, 1] for t in train]), others)    # the training corpus is the other folds
    Xm, _ = np_ref.synth_mm(4, [24, 12], [3, 2], seed=3, means=[200, 60])
    pm = sr.split_mm(Xm, 2, 9)
    train, test = mmm.holdout(Xm, pm, 1)
    for d in range(4):
        for m in range(2):
            assert np.array_equal(train[d][m][:, 1] + test[d][m][:, 1], Xm[d][m][:, 1]) and np.array_equal(test[d][m], pm[1][d][m])
    with pytest.raises(ValueError):
        mmm.holdout(X, sr.split(X[:4], 3, 9), 0)
    bad = [[p.copy() for p in part] for part in parts]
    bad[0][1][0, 1] = X[1][0, 1] + 1                                                # more than the entry holds
    with pytest.raises(ValueError):
        mmm.holdout(X, bad, 0)
