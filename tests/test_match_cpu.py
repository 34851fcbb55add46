"""Signature matching without a GPU: the restatement's assignment is optimal (brute force; scipy where it is installed), the Python
layer validates before it touches a device, and the catalogue reader round-trips."""
import numpy as np
import pytest

import match_ref as mr


def _cases(seed=20260301):
    """seeded (K, C) matrices for every 1 <= K <= 6, K <= C <= 8: uniform, cosine-shaped and tie-heavy (entries in {0, 1/4, 1/2, 3/4})"""
    rng = np.random.default_rng(seed)
    for K in range(1, 7):
        for C in range(K, 9):
            yield "uniform", rng.random((K, C))
            a, b = rng.dirichlet(np.full(12, 0.3), size=K), rng.dirichlet(np.full(12, 0.3), size=C)
            yield "cosine", mr.cosine(a, b)
            yield "ties", rng.integers(0, 4, size=(K, C)) / 4.0
            yield "ties", rng.integers(0, 2, size=(K, C)) / 2.0


def test_lsap_is_optimal_against_brute_force():
    n = 0
    for kind, S in _cases():
        a = mr.lsap(S)
        K, C = S.shape
        assert a.shape == (K,) and len(set(a.tolist())) == K and a.min() >= 0 and a.max() < C, (kind, S)
        got = sum(S[k, a[k]] for k in range(K))
        want = mr.brute_force_value(S)
        assert abs(got - want) <= 1e-12, (kind, K, C, got, want)
        n += 1
    assert n == 4 * sum(9 - K for K in range(1, 7))


def test_lsap_prefers_the_lowest_column_on_exact_ties():
    S = np.array([[0.5, 0.5, 0.5], [0.25, 0.25, 0.25]])
    assert mr.lsap(S).tolist() == [0, 1]
    S = np.array([[0.0, 0.75, 0.75, 0.75]])
    assert mr.lsap(S).tolist() == [1]


def test_lsap_value_equals_scipy():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(5)
    mats = [S for _, S in _cases(seed=77)]
    for K, C in ((12, 19), (12, 12), (7, 86), (40, 64)):
        mats.append(rng.random((K, C)))
        mats.append(rng.integers(0, 4, size=(K, C)) / 4.0)
        mats.append(mr.cosine(rng.dirichlet(np.full(96, 0.2), size=K), rng.dirichlet(np.full(96, 0.2), size=C)))
    for S in mats:
        a = mr.lsap(S)
        rows, cols = opt.linear_sum_assignment(S, maximize=True)
        assert abs(S[np.arange(S.shape[0]), a].sum() - S[rows, cols].sum()) <= 1e-12


def test_align_and_stability_restatement():
    rng = np.random.default_rng(9)
    base = rng.dirichlet(np.full(20, 0.2), size=4)
    perms = [rng.permutation(4) for _ in range(5)]
    sig = np.stack([base[p] * rng.uniform(0.5, 9.0, size=(4, 1)) for p in perms])
    assign, matched, _ = mr.match(sig, sig[0])
    for r, p in enumerate(perms):
        assert np.array_equal(perms[0][assign[r]], p)             # replica r's topic k is base[p[k]] = replica 0's topic assign[r][k]
    P = mr.align_normalise(sig, assign)
    np.testing.assert_allclose(P, np.broadcast_to(base[perms[0]], P.shape), rtol=1e-14)
    np.testing.assert_allclose(mr.stability(assign, matched, 0), 1.0, rtol=1e-14)
    assert np.array_equal(mr.stability(assign[:1], matched[:1], 0), np.ones(4))


@pytest.fixture
def no_device(mmm, monkeypatch):
    """any attempt to reach the library or a device fails the test"""
    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were validated")
    from multimodalmusig_jl_amd import _lib, match
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(match, "lib", boom)
    return mmm


def test_python_validation_comes_before_the_device(no_device):
    mmm = no_device
    sig = np.ones((3, 8)); cat = np.ones((5, 8))
    with pytest.raises(ValueError, match="K = 3"):
        mmm.match_signatures(sig, cat[:2])
    with pytest.raises(ValueError, match="terms"):
        mmm.match_signatures(sig, np.ones((5, 7)))
    bad = sig.copy(); bad[1, 2] = -1e-300
    with pytest.raises(ValueError, match="negative or non-finite"):
        mmm.match_signatures(bad, cat)
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="negative or non-finite"):
        mmm.match_signatures(sig, np.where(np.arange(8) == 2, np.inf, cat))
    with pytest.raises(ValueError, match="negative or non-finite"):
        mmm.cosine_similarity(bad, cat)
    with pytest.raises(ValueError, match="terms"):
        mmm.cosine_similarity(sig, np.ones((5, 9)))
    with pytest.raises(ValueError, match="dimensions"):
        mmm.match_signatures(np.ones(8), cat)
    with pytest.raises(ValueError, match=r"\[C, V\]"):
        mmm.match_signatures(sig, np.ones((2, 5, 8)))
    with pytest.raises(ValueError, match="ref = 4"):
        mmm.signature_consensus(np.ones((4, 3, 8)), ref=4)
    with pytest.raises(ValueError, match="q must lie"):
        mmm.signature_consensus(np.ones((4, 3, 8)), ref=0, q=(0.5, 1.5))
    with pytest.raises(TypeError):
        mmm.match_restarts(object())
    from multimodalmusig_jl_amd import restarts as rs
    with pytest.raises(ValueError, match="one batch"):
        rs.fit_lda_restarts([], 3, 0.1, 0.1, [1, 2, 3, 4], V=5, batch_size=2, consensus=True)
    with pytest.raises(ValueError, match="one batch"):
        rs.fit_seed_models([], [3], [0.1], [5], [1, 2, 3, 4], batch_size=2, consensus=True)


def test_read_signatures_tsv_round_trip(mmm, tmp_path):
    rng = np.random.default_rng(3)
    terms = ["A[C>A]A", "A[C>A]C", "A[C>G]T", "T[T>G]T", "C[T>C]G"]
    names = ["SBS1", "SBS5", "SBS40"]
    table = rng.dirichlet(np.full(5, 0.5), size=3)                # [C, V]
    path = tmp_path / "cosmic.tsv"
    with open(path, "w") as fh:
        fh.write("Type\t" + "\t".join(names) + "\n")
        for v, t in enumerate(terms):
            fh.write(t + "\t" + "\t".join(repr(float(table[c, v])) for c in range(3)) + "\n")
    got_names, got_terms, S = mmm.read_signatures_tsv(str(path))
    assert got_names == names and got_terms == terms and S.dtype == np.float64 and S.flags["C_CONTIGUOUS"]
    assert np.array_equal(S, table)
    order = [3, 0, 4, 1]                                          # reordered, one catalogue term not asked for
    _, t2, S2 = mmm.read_signatures_tsv(str(path), terms=[terms[i] for i in order])
    assert t2 == [terms[i] for i in order] and np.array_equal(S2, table[:, order])
    with pytest.raises(ValueError, match="lacks 1 of the 3 terms"):
        mmm.read_signatures_tsv(str(path), terms=[terms[0], "G[T>A]G", terms[1]])
    with open(path, "a") as fh:
        fh.write(terms[0] + "\t0.1\t0.2\t0.3\n")
    with pytest.raises(ValueError, match="listed twice"):
        mmm.read_signatures_tsv(str(path), terms=terms)
