"""The bootstrap definitions without a GPU: the Philox known answers, the properties of the numpy restatement (tests/bootstrap_ref.py) that
the device is then held to bit for bit (tests/test_bootstrap_gpu.py), and the two entry points in the built library."""
import numpy as np

import bootstrap_ref as br
import np_ref


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = br.philox4x32_10(*[np.array([c], np.uint64) for c in ctr], *key)
        assert _hex(w[0] for w in got) == want
    # vectorised over the counter: element i equals the scalar call
    got = br.philox4x32_10(np.arange(5, dtype=np.uint64), np.full(5, 7, np.uint64), np.full(5, 3, np.uint64), np.zeros(5, np.uint64), 11, 12)
    one = br.philox4x32_10(*[np.array([c], np.uint64) for c in (4, 7, 3, 0)], 11, 12)
    assert [int(w[4]) for w in got] == [int(w[0]) for w in one]


def _corpus():
    X, _ = np_ref.synth_lda(40, 96, 6, seed=31, mean_n=400)
    X = [x.copy() for x in X]
    X[3][2, 1] = 0                       # an entry with count 0, added by hand
    return X


def test_resampling_restatement_is_a_multinomial_resampling():
    X = _corpus()
    B, seed = 256, 20260101
    reps = br.resample(X, B, seed)
    C = br.counts_matrix(reps)                                                     # [B, nnz]
    c = np.concatenate([x[:, 1] for x in X])
    dp = np.concatenate([[0], np.cumsum([x.shape[0] for x in X])])
    for rep in reps[:3]:
        for x, r in zip(X, rep):
            assert np.array_equal(x[:, 0], r[:, 0])                                # same rows, same terms
    # every replicate keeps every N_d
    N = np.array([x[:, 1].sum() for x in X])
    assert np.array_equal(np.add.reduceat(C, dp[:-1], axis=1), np.broadcast_to(N, (B, len(X))))
    # a zero count never receives a draw
    assert c[dp[3] + 2] == 0 and not C[:, dp[3] + 2].any()
    assert C.min() >= 0
    # streams differ
    assert not np.array_equal(br.counts_matrix(br.resample(X, 4, seed, stream=1)), C[:4])
    # chunked calls are slices of the big call
    assert np.array_equal(br.counts_matrix(br.resample(X, 8, seed, b0=64)), C[64:72])
    # the replicate means sit where a multinomial puts them: |mean_e - c_e| <= 6 standard errors for every entry (a cap, not a
    # measurement: the restatement gives 4.05 on exactly this input)
    Ne = np.repeat(N, np.diff(dp)).astype(np.float64)
    p = c / Ne
    live = c > 0
    se = np.sqrt(Ne * p * (1 - p) / B)
    z = np.abs(C.mean(axis=0) - c)[live & (se > 0)] / se[live & (se > 0)]
    print("max |z| over %d entries: %.3f" % (z.size, z.max()))
    assert z.max() <= 6.0
    assert np.array_equal(C[:, live & (se == 0)], np.broadcast_to(c[live & (se == 0)], (B, int((live & (se == 0)).sum()))))


def test_summary_restatement_matches_numpy():
    rng = np.random.default_rng(5)
    x = rng.random((37, 11))
    q = [0.0, 0.025, 0.5, 0.975, 1.0]
    mean, sd, quant = br.summary(x, q)
    np.testing.assert_allclose(mean, x.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(sd, x.std(axis=0, ddof=1), rtol=1e-12)
    np.testing.assert_allclose(quant, np.quantile(x, q, axis=0), rtol=0, atol=1e-15)
    assert np.array_equal(quant[0], x.min(axis=0)) and np.array_equal(quant[-1], x.max(axis=0))
    m1, s1, q1 = br.summary(x[:1], [0.3])
    assert np.array_equal(m1, x[0]) and not s1.any() and np.array_equal(q1[0], x[0])


def test_stack_is_replicate_major():
    X = _corpus()[:5]
    reps = br.resample(X, 3, 9)
    S = br.stack(reps)
    assert len(S) == 15 and all(S[b * 5 + d] is reps[b][d] for b in range(3) for d in range(5))


def test_library_exports_the_bootstrap_entry_points(mmm):
    mmm.build()
    L = mmm.lib()
    assert hasattr(L, "mmm_resample_counts") and hasattr(L, "mmm_replicate_summary")
    assert {"mmm_resample_counts", "mmm_replicate_summary"} <= set(mmm._lib.declared_symbols())
    assert callable(mmm.bootstrap_exposures) and callable(mmm.resample_counts)
