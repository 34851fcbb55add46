#!/usr/bin/env python3
"""Parametric-bootstrap goodness of fit of the BRCA-EU SNV table (tests/golden/brca-eu_snv_counts.tsv, 560 samples x 96 terms) under a
K = 10 LDA fitted on the table: B (1000) replicates per sample, B x sum N_d categorical draws and two statistics per replicate.
  (a) the kernel alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_fit_check) in a run of
      its own and hand the summary to the main run with --kernel-stats FILE;
  (b) goodness_of_fit end to end (host clock around the call, which ends in a device synchronise), and simulate_counts end to end (the
      B x D x V table comes to the host);
  (c) the host: numpy.random.Generator.multinomial plus the same two statistics in vectorised numpy, on --host-reps replicates, scaled to B.
Reports the draws per second of (a) beside the resampler's (profiles/bootstrap_resample_kernel_stats.csv: the same Philox block and the same
search per draw), and how many samples the check flags.
Usage: python tools/bench_fitcheck.py [--B 1000] [--rounds 3] [--host-reps 50] [--kernel-stats FILE] [--out profiles/fitcheck_brca.json]
       python tools/bench_fitcheck.py --kernel-only 3
Prints one JSON line."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import mmm_pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1000)
ap.add_argument("--K", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--host-reps", type=int, default=50)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()

_, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
ctx = mmm.default_context()
D, V = len(X), 96
rng = np.random.default_rng(args.seed)
g = mmm.LDA(args.K, 0.1, 0.1, V, X, λ0=rng.integers(1, 101, size=(V, args.K)).astype(np.float64))
mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
θ, β = g.θ, g.β
g.close()
N = np.asarray([x[:, 1].sum() for x in X], dtype=np.int64)


def check():
    return mmm.goodness_of_fit(X, θ, β, B=args.B, seed=args.seed, ctx=ctx)


if args.kernel_only:
    for _ in range(args.kernel_only):
        check()
    sys.exit(0)


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, r


clock(check)
t_b, t_s = [], []
for _ in range(args.rounds):
    t, fc = clock(check)
    t_b.append(t)
    t, _ = clock(lambda: mmm.simulate_counts(θ, β, N, B=min(args.B, 100), seed=args.seed, ctx=ctx))
    t_s.append(t)

# (c) the host: multinomial draws and the same statistics, vectorised over the replicates of a sample
dense = np.zeros((D, V))
for d, x in enumerate(X):
    np.add.at(dense[d], x[:, 0] - 1, x[:, 1])
hrng = np.random.default_rng(args.seed)
nh = min(args.host_reps, args.B)
t0 = time.perf_counter()
le = np.zeros(D, dtype=np.int64); ge = np.zeros(D, dtype=np.int64)
for d in range(D):
    p = β @ θ[:, d]
    pi = p / p.sum()
    e = N[d] * pi
    pn = np.sqrt((pi * pi).sum())

    def stats(n):
        return (n @ pi) / (np.sqrt((n * n).sum(axis=-1)) * pn), (((n - e) ** 2) / e).sum(axis=-1)
    co, xo = stats(dense[d])
    cr, xr = stats(hrng.multinomial(N[d], pi, size=nh).astype(np.float64))
    le[d] = (cr <= co).sum(); ge[d] = (xr >= xo).sum()
t_c = time.perf_counter() - t0

draws = int(N.sum()) * args.B
out = {"device": ctx.device_name(), "D": D, "V": V, "K": args.K, "B": args.B, "mutations": int(N.sum()), "draws": draws, "rounds": args.rounds,
       "b_goodness_of_fit_s": statistics.median(t_b), "b_all_s": t_b, "simulate_counts_reps": min(args.B, 100), "simulate_counts_s": statistics.median(t_s),
       "c_numpy_reps": nh, "c_numpy_s": t_c, "c_numpy_scaled_s": t_c * args.B / nh,
       "flagged_chi2_at_0.01": int(fc.flagged(0.01, "chi2").size), "flagged_cosine_at_0.01": int(fc.flagged(0.01, "cosine").size),
       "cosine_min_median_max": [float(fc.cosine.min()), float(np.median(fc.cosine)), float(fc.cosine.max())],
       "flagged_chi2_with_cosine_above_0.9": int((fc.cosine[fc.flagged(0.01, "chi2")] > 0.9).sum())}
out["c_over_b"] = out["c_numpy_scaled_s"] / out["b_goodness_of_fit_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh) if "k_simulate" in r["Name"]]
    calls = sum(int(r["Calls"]) for r in rows)
    ns = sum(float(r["TotalDurationNs"]) for r in rows)
    out["a_kernel_calls"] = calls
    out["a_kernel_ms"] = ns / calls / 1e6
    out["a_draws_per_s"] = draws / (ns / calls / 1e9)
    ref = os.path.join(ROOT, "profiles", "bootstrap_resample_kernel_stats.csv")
    if os.path.exists(ref):
        with open(ref) as fh:
            rs = [r for r in csv.DictReader(fh) if "k_resample_counts" in r["Name"]]
        if rs and args.B == 1000:                 # its longest launch is the B = 1000 call on the same table: the same number of draws
            out["resampler_kernel_ms"] = float(rs[0]["MaxNs"]) / 1e6
            out["resampler_draws_per_s"] = draws / (float(rs[0]["MaxNs"]) / 1e9)
            out["a_over_resampler"] = out["a_draws_per_s"] / out["resampler_draws_per_s"]
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
