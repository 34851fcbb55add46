"""Signature matching on the device against the restatement of its definitions (tests/match_ref.py): the cosine within the rounding
bound of its three sums, the assignment EXACTLY the restatement's on the device's own similarities, planted permutations recovered,
bits independent of R and of the chunking, the handle forms equal to the array form on the downloaded tables, and the consensus."""
import os

import numpy as np
import pytest

import match_ref as mr
import np_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53


def _bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rows(rng, n, V, scale=True):
    """n unnormalised non-negative rows over V terms, row scales spanning 1e-3 .. 1e6"""
    x = rng.dirichlet(np.full(V, 0.3), size=n) if V > 1 else rng.random((n, 1)) + 0.1
    return x * (10.0 ** rng.uniform(-3, 6, size=(n, 1))) if scale else x


# ------------------------------------------------------------------------------------------------------------ 1. cosine
@pytest.mark.parametrize("V", [1, 7, 96, 1536, 5000])
def test_cosine_is_the_definition(mmm, V):
    rng = np.random.default_rng(100 + V)
    sig = _rows(rng, 5, V); cat = _rows(rng, 9, V)
    sig[3] = 0.0; cat[6] = 0.0                                    # zero rows: S = 0 against everything, never NaN
    bound = (2 * V + 8) * U
    for s, c in ((sig, cat), (sig[:1], cat[:1]), (cat, sig)):     # (K = C = 1 among them; the cosine alone takes K > C)
        got = mmm.cosine_similarity(s, c)
        want = mr.cosine_exact(s, c)
        err = float(np.abs(got - want).max())
        print("V = %d, K = %d, C = %d: max |S - exact| = %.3g (bound %.3g)" % (V, s.shape[0], c.shape[0], err, bound))
        assert got.shape == want.shape and np.isfinite(got).all() and err <= bound
        assert not got[(s == 0).all(axis=1)].any() and not got[:, (c == 0).all(axis=1)].any()
    stacked = mmm.cosine_similarity(np.stack([sig, sig[::-1]]), cat)              # leading axes are replicas
    assert _bits(stacked[0], mmm.cosine_similarity(sig, cat)) and _bits(stacked[1], stacked[0][::-1])


# ------------------------------------------------------------------------------------------------------------ 2. assignment
def _assign_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "random":
        return _rows(rng, 3 * 12, 40).reshape(3, 12, 40), _rows(rng, 12, 40)
    if name == "rectangular":
        return _rows(rng, 3 * 7, 96).reshape(3, 7, 96), _rows(rng, 86, 96)
    if name == "ties":                                            # every catalogue row three times: exact ties, the lowest column must win
        base = _rows(rng, 5, 24)
        return _rows(rng, 4 * 6, 24).reshape(4, 6, 24), np.concatenate([base, base, base])[rng.permutation(15)]
    if name == "ties_coarse":                                     # 0 / 1 entries: many equal cosines between different rows too
        return rng.integers(0, 2, size=(4, 8, 6)).astype(np.float64), rng.integers(0, 2, size=(11, 6)).astype(np.float64)
    if name == "K1":
        return _rows(rng, 3, 30).reshape(3, 1, 30), _rows(rng, 5, 30)
    if name == "K256":
        return _rows(rng, 2 * 256, 64).reshape(2, 256, 64), _rows(rng, 256, 64)
    if name == "C1024":
        return _rows(rng, 2 * 200, 32).reshape(2, 200, 32), _rows(rng, 1024, 32)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["random", "rectangular", "ties", "ties_coarse", "K1", "K256", "C1024"])
def test_assignment_equals_the_restatement_exactly(mmm, name):
    sig, cat = _assign_case(name)
    m = mmm.match_signatures(sig, cat)
    R, K, _ = sig.shape
    assert m.assign.shape == (R, K) and m.assign.dtype == np.int32 and m.similarity.shape == (R, K, cat.shape[0])
    for r in range(R):
        want = mr.lsap(m.similarity[r])
        assert np.array_equal(m.assign[r], want), "%s replica %d: device %r, restatement %r" % (name, r, m.assign[r], want)
        assert len(set(m.assign[r].tolist())) == K
        assert _bits(m.cosine[r], m.similarity[r][np.arange(K), m.assign[r]])
    one = mmm.match_signatures(sig[0], cat)                       # a [K, V] input gives unbatched outputs
    assert _bits(one.assign, m.assign[0]) and _bits(one.cosine, m.cosine[0]) and _bits(one.similarity, m.similarity[0])


def test_identical_catalogue_rows_go_to_the_lowest(mmm):
    row = np.arange(1.0, 9.0)
    m = mmm.match_signatures(row[None, :], np.stack([row[::-1], row, row, row]))
    s = m.similarity[0]
    assert m.assign.tolist() == [1] and s[1] == s[2] == s[3] and s[0] < s[1]


# ------------------------------------------------------------------------------------------------------------ 3. planted permutations
def test_planted_permutations_are_recovered(mmm):
    rng = np.random.default_rng(20260302)
    R, K, V = 256, 10, 96
    base = rng.dirichlet(np.full(V, 0.1), size=K)
    perms = np.stack([rng.permutation(K) for _ in range(R)])
    sig = np.stack([base[perms[r]] * rng.uniform(0.5, 200.0, size=(K, 1)) * rng.gamma(50.0, 1.0 / 50.0, size=(K, V)) for r in range(R)])
    m = mmm.match_signatures(sig, base)
    ok = (m.assign == perms).all(axis=1)
    print("recovered %d of %d permutations, smallest matched cosine %.3f" % (int(ok.sum()), R, float(m.cosine.min())))
    assert ok.all()


# ------------------------------------------------------------------------------------------------------------ 4. R and chunking
def test_a_replica_does_not_depend_on_R_or_on_the_chunking(mmm):
    rng = np.random.default_rng(41)
    R, K, Cn, V = 300, 120, 128, 32                               # 300 x 120 x 128 similarities: more than one device chunk of S
    sig = _rows(rng, R * K, V).reshape(R, K, V); cat = _rows(rng, Cn, V)
    full = mmm.match_signatures(sig, cat)
    again = mmm.match_signatures(sig, cat)
    assert all(_bits(a, b) for a, b in zip(full, again))
    for r in (0, 1, 150, 272, 273, 299):
        one = mmm.match_signatures(sig[r:r + 1], cat)
        assert _bits(one.assign[0], full.assign[r]) and _bits(one.cosine[0], full.cosine[r]) and _bits(one.similarity[0], full.similarity[r]), r
    R = 70000                                                     # more replicas than one launch takes
    sig = _rows(rng, R * 2, 5).reshape(R, 2, 5); cat = _rows(rng, 3, 5)
    full = mmm.match_signatures(sig, cat)
    for r in (0, 65534, 65535, 65536, 69999):
        one = mmm.match_signatures(sig[r], cat)
        assert _bits(one.assign, full.assign[r]) and _bits(one.cosine, full.cosine[r]) and _bits(one.similarity, full.similarity[r]), r
    empty = mmm.match_signatures(np.zeros((0, 2, 5)), cat)        # R = 0 writes nothing
    assert empty.assign.shape == (0, 2) and empty.similarity.shape == (0, 2, 3)


# ------------------------------------------------------------------------------------------------------------ 5. handle forms
def _brca(mmm):
    _, samples, snv = mmm.read_counts_tsv(os.path.join(GOLD, "brca-eu_snv_counts.tsv"))
    _, samples2, sv = mmm.read_counts_tsv(os.path.join(GOLD, "brca-eu_sv_counts.tsv"))
    assert samples == samples2
    return samples, {s: snv[:, i] for i, s in enumerate(samples)}, {s: sv[:, i] for i, s in enumerate(samples)}


def _tables(model, field):
    """the tables of every restart, downloaded restart by restart ([R, K, V]); the selection is put back"""
    keep = model.selected
    out = []
    for r in range(model.R):
        model.select(r)
        out.append(field(model))
    model.select(keep)
    return np.stack(out)


def _check_handle(mmm, model, tabs, modality, V):
    R, K = tabs.shape[:2]
    for sel in sorted({0, R - 1, R // 3}):
        model.select(sel)
        got = mmm.match_restarts(model, modality=modality)
        want = mmm.match_signatures(tabs, tabs[sel])
        assert got.similarity is None and _bits(got.assign, want.assign) and _bits(got.cosine, want.cosine), sel
        assert np.array_equal(got.assign[sel], np.arange(K))
        err = float(np.abs(got.cosine[sel] - 1.0).max())
        print("selected restart %d: max |cosine to itself - 1| = %.3g (bound %.3g)" % (sel, err, (2 * V + 8) * U))
        assert err <= (2 * V + 8) * U
        ref = mr.match(tabs, tabs[sel])[0]                        # the restatement on its own similarities: equal unless a near-tie flips
        print("restarts whose assignment equals the restatement's on numpy's similarities: %d of %d" % (int((ref == got.assign).all(axis=1).sum()), R))
    cat = _rows(np.random.default_rng(8), 86, V)
    got = mmm.match_restarts(model, modality=modality, catalogue=cat)
    want = mmm.match_signatures(tabs, cat)
    assert _bits(got.assign, want.assign) and _bits(got.cosine, want.cosine)


def test_lda_handle_forms(mmm):
    samples, snv, _ = _brca(mmm)
    X = mmm.format_counts_lda(snv, samples)
    model = mmm.LDA(7, 0.1, 0.1, X, restarts=64, seed=5)
    with pytest.raises(ValueError, match="fit_restarts"):
        mmm.restart_consensus(model)
    mmm.fit_restarts(model)
    iters = np.asarray(model.restart_iters)
    print("passes per restart: min %d, max %d, distinct values mod 3: %r" % (iters.min(), iters.max(), sorted(set((iters % 3).tolist()))))
    assert len(set((iters % 3).tolist())) > 1                     # the restarts stand in different ring slots: a wrong slot would show
    tabs = _tables(model, lambda m: np.ascontiguousarray(m.λ.T))
    assert tabs.shape == (64, 7, 96)
    _check_handle(mmm, model, tabs, None, 96)
    model.close()


def test_mmctm_handle_forms(mmm):
    samples, snv, sv = _brca(mmm)
    X = mmm.format_counts_mmctm([snv, sv], samples)
    model = mmm.MMCTM([7, 7], [0.1, 0.1], [96, 48], X, restarts=32, seed=9)
    mmm.fit_restarts(model, maxiter=12, tol=1e-3)
    with pytest.raises(ValueError, match="modality"):
        mmm.match_restarts(model)
    for m, V in ((0, 96), (1, 48)):
        tabs = _tables(model, lambda mod: np.stack([mod.γ[m][k] for k in range(7)]))
        assert tabs.shape == (32, 7, V)
        _check_handle(mmm, model, tabs, m, V)
    own = mmm.match_signatures(model, np.stack([model.ϕ[1][k] for k in range(7)]), modality=1)      # a model as `sig`: its ϕ
    assert np.array_equal(own.assign, np.arange(7))
    model.close()


def test_ordinary_handles_and_factorised_models(mmm):
    X, _ = np_ref.synth_lda(30, 96, 5, seed=12, mean_n=400)
    g = mmm.LDA(5, 0.1, 0.1, 96, X, seed=2)
    mmm.fit(g, maxiter=7, tol=0.0, verbose=False)                 # 7 passes: the ring stands at slot 1
    lam = np.ascontiguousarray(g.λ.T)
    got = mmm.match_restarts(g)
    assert got.assign.shape == (1, 5) and np.array_equal(got.assign[0], np.arange(5)) and np.abs(got.cosine - 1).max() <= (2 * 96 + 8) * U
    cat = _rows(np.random.default_rng(1), 9, 96)
    want = mmm.match_signatures(lam, cat)
    got = mmm.match_restarts(g, catalogue=cat)
    assert _bits(got.assign[0], want.assign) and _bits(got.cosine[0], want.cosine)
    by_beta = mmm.match_signatures(g, cat)                            # a model as `sig`: the columns of β
    assert np.array_equal(by_beta.assign, want.assign)
    c = mmm.restart_consensus(g, ref=0)                           # one replica: its own probabilities, sd 0, stability 1
    np.testing.assert_allclose(c.mean, lam / lam.sum(axis=1, keepdims=True), rtol=0, atol=4 * 96 * U)
    assert not c.sd.any() and np.array_equal(c.stability, np.ones(5)) and _bits(c.quantiles[1], c.mean)
    feats = np.stack([np.arange(96) // 16 + 1, np.arange(96) % 16 + 1], axis=1)
    il = mmm.ILDA(4, 0.1, [0.1, 0.1], feats, X, seed=1)
    Xm, _ = np_ref.synth_mm(10, [96], [3], seed=2, means=[300])
    im = mmm.IMMCTM([3], [0.1], [feats], Xm, seed=1)
    for fn in (mmm.match_restarts, lambda m: mmm.restart_consensus(m, ref=0), lambda m: mmm.match_signatures(m, cat)):
        with pytest.raises(TypeError):
            fn(il)
        with pytest.raises(TypeError):
            fn(im)
    L = mmm.lib()                                                 # the C entries refuse them too
    a = np.zeros(8, np.int32); md = np.zeros(8)
    assert L.mmm_lda_match_replicas(il._h, 0, None, a.ctypes.data, md.ctypes.data) == -4
    assert L.mmm_ctm_match_replicas(im._h, 0, 0, None, a.ctypes.data, md.ctypes.data) == -4


# ------------------------------------------------------------------------------------------------------------ 6. consensus
Q5 = (0.0, 0.025, 0.5, 0.975, 1.0)


def _check_consensus(mmm, got, tabs, ref, V):
    assign, matched, _ = mr.match(tabs, tabs[ref])
    dev = mmm.match_signatures(tabs, tabs[ref])                   # the assignment is defined on the device's similarities
    assert got.ref == ref and _bits(got.assign, dev.assign) and _bits(got.cosine, dev.cosine)
    print("restarts whose assignment equals the restatement's on numpy's similarities: %d of %d" % (int((assign == got.assign).all(axis=1).sum()), len(tabs)))
    P = mr.align_normalise(tabs, got.assign)
    mean, sd, quant = mmm.replicate_summary(P, Q5)
    bound = 4 * V * U
    for name, a, b in (("mean", got.mean, mean), ("sd", got.sd, sd), ("quantiles", got.quantiles, quant)):
        err = float(np.abs(a - b).max())
        print("%s: max |device - summary of the restatement| = %.3g (bound %.3g)" % (name, err, bound))
        assert a.shape == b.shape and err <= bound
    assert np.abs(got.mean.sum(axis=1) - 1.0).max() <= 1e-12
    np.testing.assert_allclose(got.stability, mr.stability(got.assign, got.cosine, ref), rtol=0, atol=len(tabs) * U)
    assert (got.stability > 0).all() and (got.stability <= 1 + 1e-12).all()


def test_restart_consensus(mmm):
    samples, snv, sv = _brca(mmm)
    model = mmm.LDA(7, 0.1, 0.1, mmm.format_counts_lda(snv, samples), restarts=64, seed=6)
    mmm.fit_restarts(model)
    tabs = _tables(model, lambda m: np.ascontiguousarray(m.λ.T))
    best = int(np.argmax(model.restart_ll))
    got = mmm.restart_consensus(model, q=Q5)
    assert got.q == Q5
    _check_consensus(mmm, got, tabs, best, 96)
    _check_consensus(mmm, mmm.restart_consensus(model, ref=3, q=Q5), tabs, 3, 96)
    arr = mmm.signature_consensus(tabs, best, q=Q5)               # the array form on the downloaded tables: the same bits
    assert all(_bits(a, b) for a, b in zip(arr[1:7], got[1:7]))
    print("stability per signature:", np.round(got.stability, 4))
    model.close()
    mm = mmm.MMCTM([7, 7], [0.1, 0.1], [96, 48], mmm.format_counts_mmctm([snv, sv], samples), restarts=32, seed=10)
    mmm.fit_restarts(mm, maxiter=12, tol=1e-3)
    for m, V in ((0, 96), (1, 48)):
        tabs = _tables(mm, lambda mod: np.stack([mod.γ[m][k] for k in range(7)]))
        _check_consensus(mmm, mmm.restart_consensus(mm, modality=m, q=Q5), tabs, mmm.pick_optimal_modality_models(mm)[m], V)
    mm.close()


def test_consensus_of_planted_replicas(mmm):
    rng = np.random.default_rng(77)
    R, K, V = 200, 6, 150
    base = rng.dirichlet(np.full(V, 0.2), size=K)
    perms = np.stack([rng.permutation(K) for _ in range(R)])
    sig = np.stack([base[perms[r]] * rng.uniform(0.5, 50.0, size=(K, 1)) * rng.gamma(200.0, 1.0 / 200.0, size=(K, V)) for r in range(R)])
    got = mmm.signature_consensus(sig, ref=0, q=Q5)
    _check_consensus(mmm, got, sig, 0, V)
    np.testing.assert_allclose(got.mean, base[perms[0]], atol=0.02)
    assert (got.quantiles[0] <= got.quantiles[2]).all() and (got.quantiles[2] <= got.quantiles[4]).all()
    small = sig[:3].copy()
    small[1, 2] = 0.0                                             # a zero signature stays zero: its label's mean sums to 2 / 3
    got = mmm.signature_consensus(small, ref=0, q=(0.0,))
    k = int(got.assign[1, 2])
    assert got.cosine[1, 2] == 0.0 and not got.quantiles[0, k].any() and abs(got.mean[k].sum() - 2.0 / 3.0) <= 1e-12
    assert np.abs(np.delete(got.mean, k, axis=0).sum(axis=1) - 1.0).max() <= 1e-12


def test_limits_and_errors_of_the_c_entries(mmm):
    L, ctx = mmm.lib(), mmm.default_context()

    def err():
        return L.mmm_last_error(ctx.h).decode()

    def match(sig, cat, S=False):
        sig = np.ascontiguousarray(sig, np.float64); cat = np.ascontiguousarray(cat, np.float64)
        R, K, V = sig.shape
        a = np.zeros((R, K), np.int32); m = np.zeros((R, K)); s = np.zeros((R, K, cat.shape[0]))
        return L.mmm_signature_match(ctx.h, R, K, cat.shape[0], V, sig.ctypes.data, cat.ctypes.data, a.ctypes.data, m.ctypes.data, s.ctypes.data if S else None)

    def consensus(sig, ref=0):
        sig = np.ascontiguousarray(sig, np.float64)
        R, K, V = sig.shape
        a = np.zeros((R, K), np.int32); mean = np.zeros((K, V))
        return L.mmm_signature_consensus(ctx.h, R, K, V, sig.ctypes.data, ref, 0, None, a.ctypes.data, None, None, mean.ctypes.data, None, None)
    ones = np.ones((2, 3, 4))
    assert match(ones, np.ones((5, 4))) == 0 and match(ones, np.ones((5, 4)), S=True) == 0
    assert match(ones, np.ones((2, 4))) == -1 and "K <= C" in err()
    assert match(np.ones((1, 2, 2)), np.ones((1025, 2))) == -4 and "1024" in err()
    assert consensus(np.ones((4097, 1, 2))) == -4 and "4096" in err()
    assert consensus(np.ones((4096, 1, 2))) == 0
    for bad in (np.nan, np.inf, -1.0):
        x = ones.copy(); x[1, 2, 3] = bad
        assert match(x, np.ones((5, 4))) == -1 and "sig[23]" in err()
        assert consensus(x) == -1
        c = np.ones((5, 4)); c[4, 0] = bad
        assert match(ones, c) == -1 and "cat[16]" in err()
    assert consensus(ones, ref=2) == -1 and consensus(ones, ref=-1) == -1
    a = np.zeros(6, np.int32)
    assert L.mmm_signature_match(ctx.h, 2, 3, 5, 4, None, ones.ctypes.data, a.ctypes.data, ones.ctypes.data, None) == -1
    assert L.mmm_signature_match(ctx.h, 2, 3, 5, 4, ones.ctypes.data, ones.ctypes.data, None, ones.ctypes.data, None) == -1
    assert L.mmm_signature_cosine(ctx.h, 2, 0, 5, 4, ones.ctypes.data, ones.ctypes.data, ones.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------------------ 7. restart drivers
def test_restart_drivers_return_the_consensus_on_request(mmm):
    from multimodalmusig_jl_amd import restarts as rs
    X, _ = np_ref.synth_lda(60, 96, 4, seed=21, mean_n=600)
    seeds = list(range(40, 52))
    old = rs.fit_lda_restarts(X, 4, 0.1, 0.1, seeds, V=96, maxiter=40)
    new = rs.fit_lda_restarts(X, 4, 0.1, 0.1, seeds, V=96, maxiter=40, consensus=True)
    assert len(old) == 4 and len(new) == 5
    assert old[0] == new[0] and all(_bits(a, b) for a, b in zip(old[1:], new[1:4]))
    cons = new[4]
    assert isinstance(cons, mmm.ConsensusResult) and cons.ref == old[0] and cons.assign.shape == (12, 4) and cons.mean.shape == (4, 96)
    np.testing.assert_allclose(cons.mean.sum(axis=1), 1.0, atol=1e-12)
    assert np.array_equal(cons.assign[cons.ref], np.arange(4))    # the consensus is in the winner's labelling
    with pytest.raises(ValueError, match="one batch"):
        rs.fit_lda_restarts(X, 4, 0.1, 0.1, seeds, V=96, maxiter=40, batch_size=6, consensus=True)
    Xm, _ = np_ref.synth_mm(40, [96, 30], [3, 2], seed=5, means=[400, 60])
    kw = dict(maxiter=8, tol=1e-3)
    old = rs.fit_seed_models(Xm, [3, 2], [0.1, 0.1], [96, 30], [1, 2, 3, 4, 5], **kw)
    new = rs.fit_seed_models(Xm, [3, 2], [0.1, 0.1], [96, 30], [1, 2, 3, 4, 5], consensus=True, **kw)
    assert len(old) == 3 and len(new) == 4 and _bits(old[1], new[1]) and _bits(old[2], new[2])
    assert all(_bits(a, b) for a, b in zip(old[0], new[0]))
    assert [c.mean.shape for c in new[3]] == [(3, 96), (2, 30)] and [c.ref for c in new[3]] == [int(i) for i in np.argmax(new[2], axis=0)]
