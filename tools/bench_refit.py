#!/usr/bin/env python3
"""Refit of the BRCA-EU SNV table (tests/golden/brca-eu_snv_counts.tsv, 560 samples x 96 terms) to a catalogue of C signatures: ten fitted
on the table itself (LDA K = 10) plus C - 10 Dirichlet(0.3) decoys -- no COSMIC file is shipped, and the decoys are what a published
catalogue is to a tumour type: mostly signatures it does not carry.
  (a) the kernel alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_refit_exposures, BIC
      penalty) in a run of its own and hand the summary to the main run with --kernel-stats FILE;
  (b) refit_exposures end to end (host clock around the call, which ends in a device synchronise);
  (c) the same with bootstrap = --B (1000) on the chosen sets;
  (d) the same definition in vectorised numpy on the host (tests/refit_ref.py), on --host-docs samples, scaled to 560.
Reports the ratios and, from the iteration counts, the double-precision operations per second the kernel sustains (4 |A| V per EM iteration:
a multiply and an add per signature and term in each of the two products).
Usage: python tools/bench_refit.py [--C 86] [--B 1000] [--rounds 3] [--host-docs 16] [--kernel-stats FILE] [--out profiles/refit_brca.json]
       python tools/bench_refit.py --kernel-only 3
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import mmm_pkg  # noqa: E402
import refit_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--C", type=int, default=86)
ap.add_argument("--B", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--host-docs", type=int, default=16)
ap.add_argument("--maxiter", type=int, default=1000)
ap.add_argument("--tol", type=float, default=1e-9)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()

_, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
ctx = mmm.default_context()
doc_ptr, term, count = mmm.pack_lda(X)
D, V = len(X), 96
rng = np.random.default_rng(args.seed)
g = mmm.LDA(10, 0.1, 0.1, V, X, λ0=rng.integers(1, 101, size=(V, 10)).astype(np.float64))
mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
cat = np.concatenate([np.ascontiguousarray(g.β.T), rng.dirichlet(np.full(V, 0.3), size=args.C - 10)])
g.close()
N = np.asarray([x[:, 1].sum() for x in X], dtype=np.float64)
pen = 0.5 * np.log(np.maximum(N, 1.0))


def raw():
    return mmm.refit._raw(ctx, D, V, doc_ptr, term, count, cat, None, pen, args.maxiter, args.tol)


if args.kernel_only:
    for _ in range(args.kernel_only):
        raw()
    sys.exit(0)


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, r


clock(raw)
t_b, t_c = [], []
for _ in range(args.rounds):
    t, res = clock(lambda: mmm.refit_exposures(X, cat, maxiter=args.maxiter, tol=args.tol))
    t_b.append(t)
    t, boot = clock(lambda: mmm.refit_exposures(X, cat, maxiter=args.maxiter, tol=args.tol, bootstrap=args.B, seed=args.seed))
    t_c.append(t)
# (d) the host restatement on the first --host-docs samples; its outputs must be the device's
nh = min(args.host_docs, D)
t0 = time.perf_counter()
ref = R.refit(nh, args.C, V, doc_ptr[:nh + 1], term, count, cat, None, pen[:nh], args.maxiter, args.tol)
t_d = time.perf_counter() - t0
same = bool(np.array_equal(ref.w, res.exposures.T[:nh]) and np.array_equal(ref.order, res.order[:nh]) and np.array_equal(ref.iters, res.iters[:nh]))
share = float(res.iters[:nh].sum()) / float(res.iters.sum())          # the subset's share of the EM iterations: what the scaling goes by

# operations: every fit of a document runs on |A| signatures; the rounds of a document go C, C - 1, ...; the iteration counts are per
# document, so the mean |A| over a document's fits weighs them
nrem = (res.order >= 0).sum(axis=1)
nfit = nrem + (nrem < args.C - 1)                 # every removal is a fit, plus the first, plus the refused last one (none when one is left)
meanA = np.asarray([np.mean([args.C - j for j in range(int(n) + 1)]) for n in nfit])
flops = float((4.0 * meanA * V * res.iters).sum())

out = {"device": ctx.device_name(), "D": D, "V": V, "C": args.C, "mutations": int(count.sum()), "maxiter": args.maxiter, "tol": args.tol, "B": args.B,
       "rounds": args.rounds, "b_refit_exposures_s": statistics.median(t_b), "b_all_s": t_b, "c_bootstrap_s": statistics.median(t_c), "c_all_s": t_c,
       "d_numpy_docs": nh, "d_numpy_s": t_d, "d_numpy_scaled_560_s": t_d / share, "d_subset_share_of_iterations": share,
       "numpy_equals_device_on_subset": same, "em_iterations_total": int(res.iters.sum()), "fits_total": int(nfit.sum() + 0),
       "active_per_sample_mean": float(res.active.sum(axis=0).mean()), "active_per_sample_max": int(res.active.sum(axis=0).max()),
       "unexplained_total": float(res.unexplained.sum()), "approx_flop": flops,
       "bootstrap_documents": args.B * D, "bootstrap_ci_width_mean": float((boot.intervals.quantiles[-1] - boot.intervals.quantiles[0])[res.active].mean())}
out["d_over_b"] = out["d_numpy_scaled_560_s"] / out["b_refit_exposures_s"]
out["c_over_b"] = out["c_bootstrap_s"] / out["b_refit_exposures_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh) if "k_refit" in r["Name"]]
    calls = sum(int(r["Calls"]) for r in rows)
    ns = sum(float(r["TotalDurationNs"]) for r in rows)
    out["a_kernel_calls"] = calls
    out["a_kernel_ms"] = ns / calls / 1e6
    out["a_kernel_gflops"] = flops / (ns / calls)
    out["b_over_a"] = out["b_refit_exposures_s"] / (ns / calls / 1e9)
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
