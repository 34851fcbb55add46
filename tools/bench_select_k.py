#!/usr/bin/env python3
"""Held-out selection of the number of signatures on the BRCA-EU SNV table (tests/golden/brca-eu_snv_counts.tsv), Ks = 2..12, F = 4 folds,
R = 64 restarts per batch:
  (a) select_num_signatures: the split on the device, every restart of a batch scored where its tables lie (mmm_lda_score_replicas), with
      the seconds spent in the split, the fits and the scoring clocked separately (its `clock` argument);
  (b) the route without the new entries, with the SAME batches fitted: the split by the numpy restatement of its definition on the host
      (tests/select_ref.py), every restart scored by select(r), a download of θ and β, and calculate_loglikelihood(X_test, θ, β).
Reports (a) / (b) for the scoring step and for the whole call, and whether the two routes give the same held-out figures (they must: the
scores are equal bit for bit).  The fits dominate both routes.
Usage: python tools/bench_select_k.py [--kmin 2] [--kmax 12] [--folds 4] [--R 64] [--rounds 3] [--out profiles/select_k_brca.json]
Host clocks around calls that end in a device synchronise; one warm-up of each route on Ks = [kmin], then the median of --rounds runs.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import mmm_pkg  # noqa: E402
import select_ref as sr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kmin", type=int, default=2)
ap.add_argument("--kmax", type=int, default=12)
ap.add_argument("--folds", type=int, default=4)
ap.add_argument("--R", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()

_, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
ctx = mmm.default_context()
F, R, seed = args.folds, args.R, args.seed
doc_ptr, term, count = mmm.pack_lda(X)
D, V = len(X), int(term.max()) + 1


def route_a(Ks):
    clock = {}
    ctx.synchronize()
    t0 = time.perf_counter()
    res = mmm.select_num_signatures(X, Ks, 0.1, 0.1, folds=F, reps=1, restarts=R, seed=seed, full_fit=False, clock=clock)
    ctx.synchronize()
    return dict(clock, total=time.perf_counter() - t0), res


def route_b(Ks):
    clock = {"split": 0.0, "fit": 0.0, "score": 0.0}
    held = np.zeros((len(Ks), F, R))
    ctx.synchronize()
    t00 = time.perf_counter()
    parts = np.concatenate([sr.split_doc(count[doc_ptr[d]:doc_ptr[d + 1]], d, F, 0, seed) for d in range(D)], axis=1).astype(np.int32)
    clock["split"] = time.perf_counter() - t00
    for f in range(F):
        Xtr = mmm.PackedCorpus(D, doc_ptr, term, count - parts[f]); Xte = mmm.PackedCorpus(D, doc_ptr, term, parts[f])
        for i, K in enumerate(Ks):
            t0 = time.perf_counter()
            lam0 = [np.random.default_rng(s).integers(1, 101, size=(V, K)).astype(np.float64) for s in mmm.select._restart_seeds(seed, K, 0, f, R)]
            model = mmm.LDA(K, 0.1, 0.1, V, Xtr, λ0=lam0, restarts=R)
            mmm.fit_restarts(model)
            ctx.synchronize()
            t1 = time.perf_counter()
            for r in range(R):
                model.select(r)
                held[i, f, r] = mmm.calculate_loglikelihood(Xte, model.θ, model.β)
            t2 = time.perf_counter()
            model.close()
            clock["fit"] += t1 - t0; clock["score"] += t2 - t1
    ctx.synchronize()
    return dict(clock, total=time.perf_counter() - t00), held


Ks = list(range(args.kmin, args.kmax + 1))
route_a(Ks[:1]); route_b(Ks[:1])
runs_a, runs_b = [], []
for _ in range(args.rounds):
    ca, res = route_a(Ks)
    cb, held = route_b(Ks)
    runs_a.append(ca); runs_b.append(cb)
med = lambda runs, k: statistics.median(r[k] for r in runs)
out = {"device": ctx.device_name(), "D": D, "V": V, "nnz": int(count.size), "mutations": int(count.sum()), "Ks": Ks, "folds": F, "R": R, "rounds": args.rounds,
       "a_select_num_signatures_s": {k: med(runs_a, k) for k in ("split", "fit", "score", "total")},
       "b_host_split_select_download_s": {k: med(runs_b, k) for k in ("split", "fit", "score", "total")},
       "a_all_s": runs_a, "b_all_s": runs_b,
       "routes_give_equal_scores": bool(np.array_equal(res.heldout_all, held)),
       "heldout_mean": res.mean.tolist(), "heldout_se": res.se.tolist(), "best": res.best, "pick": res.pick}
for k in ("split", "score", "total"):
    out["a_over_b_" + k] = out["a_select_num_signatures_s"][k] / out["b_host_split_select_download_s"][k]
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
