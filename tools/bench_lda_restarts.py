#!/usr/bin/env python3
"""LDA restarts on BASELINE config 1 (BRCA-EU SNV table, K = 7, alpha = eta = 0.1), fitted to convergence (tol 1e-4, maxiter 1000)
two ways from the same R random inits: one batch handle (LDA(..., restarts=R) + fit_restarts) and R single handles fitted one after
the other (the default single path, merged launch included).
Usage: python tools/bench_lda_restarts.py [--restarts 256] [--seed 0]
Each mode is timed by the host clock around its fits (handles created beforehand), ending in a device synchronise, after a warm-up fit
of the same kind.  Prints one JSON line: per mode wall seconds, fits/s and the pass counts; whether the two modes pick the same winner."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import mmm_pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--restarts", type=int, default=256)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--maxiter", type=int, default=1000)
ap.add_argument("--tol", type=float, default=1e-4)
args = ap.parse_args()
mmm = mmm_pkg.load()
from multimodalmusig_jl_amd import restarts as rs  # noqa: E402

_, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
K, V, R = 7, 96, args.restarts
rng = np.random.default_rng(args.seed)
lams = [rng.integers(1, 101, size=(V, K)).astype(np.float64) for _ in range(R)]
ctx = mmm.default_context()


def batch_fit(n):
    b = mmm.LDA(K, 0.1, 0.1, V, X, λ0=lams[:n], restarts=n)
    ctx.synchronize()
    t0 = time.perf_counter()
    mmm.fit_restarts(b, maxiter=args.maxiter, tol=args.tol)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    out = (dt, b.restart_ll.copy(), b.restart_iters.copy())
    b.close()
    return out


def sequential_fits(n):
    gs = [mmm.LDA(K, 0.1, 0.1, V, X, λ0=lams[i]) for i in range(n)]
    ctx.synchronize()
    t0 = time.perf_counter()
    hists = [mmm.fit(g, maxiter=args.maxiter, tol=args.tol, verbose=False) for g in gs]
    ctx.synchronize()
    dt = time.perf_counter() - t0
    for g in gs:
        g.close()
    return dt, np.array([h[-1] for h in hists]), np.array([len(h) for h in hists])


batch_fit(min(R, 8)); sequential_fits(1)          # warm-up: module load, kernel attributes, pinned buffers
tb, llb, itb = batch_fit(R)
ts, lls, its = sequential_fits(R)
wb, ws = rs._best(llb), rs._best(lls)
res = {
    "tool": "bench_lda_restarts", "config": "1 (BRCA-EU SNV, K=7, alpha=eta=0.1)", "device": ctx.device_name(), "restarts": R,
    "maxiter": args.maxiter, "tol": args.tol,
    "batch": {"wall_s": tb, "fits_per_s": R / tb, "passes_max": int(itb.max()), "passes_mean": float(itb.mean())},
    "sequential": {"wall_s": ts, "fits_per_s": R / ts, "passes_max": int(its.max()), "passes_mean": float(its.mean()),
                   "passes_total": int(its.sum())},
    "speedup": ts / tb,
    "winner": {"batch": wb, "sequential": ws, "agree": wb == ws, "ll_batch": float(llb[wb]), "ll_sequential": float(lls[ws]),
               "max_rel_ll_diff": float(np.max(np.abs(llb - lls) / np.abs(lls)))},
}
print(json.dumps(res))
