#!/usr/bin/env python3
"""Extraction of J = 2 new signatures from the BRCA-EU SNV table (tests/golden/brca-eu_snv_counts.tsv, 560 samples x 96 terms) beside F = 10
fixed rows -- the first ten rows of the catalogue tools/bench_refit.py builds (the signatures of an LDA with K = 10 fitted to the table) --
in 256 restarts of 1000 iterations (tol = 0).
  (a) the kernel alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_extract_signatures) in a
      run of its own and hand the summary to the main run with --kernel-stats FILE;
  (b) extract_signatures end to end (host clock around the call, which ends in a device synchronise), warmed up, median of --rounds; and the
      library call alone with the block geometry pinned by --waves (the Python function always takes the library's choice);
  (c) the same definition in vectorised numpy on the host (tests/extract_ref.py): ONE restart of --host-iters iterations, scaled to the
      restarts and iterations of (b); its rows must be the device's.
Reports the ratios and the double-precision operations per second the kernel sustains (per restart and iteration D (4 K + 2 J) V: a multiply
and an add per row and term in q and in g, and per new row and term in the sums over documents).
Usage: python tools/bench_extract.py [--restarts 256] [--maxiter 1000] [--waves 0] [--rounds 5] [--host-iters 100] [--kernel-stats FILE]
                                     [--out profiles/extract_brca.json]
       python tools/bench_extract.py --kernel-only 3
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
import extract_ref as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--F", type=int, default=10)
ap.add_argument("--J", type=int, default=2)
ap.add_argument("--restarts", type=int, default=256)
ap.add_argument("--maxiter", type=int, default=1000)
ap.add_argument("--waves", type=int, default=0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-iters", type=int, default=100)
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
cat = np.ascontiguousarray(g.β.T)[:args.F]                     # the catalogue of tools/bench_refit.py, its first rows
g.close()
F, J, R = cat.shape[0], args.J, args.restarts


def raw(R=R, maxiter=args.maxiter, outputs=()):
    return mmm.extract._raw(ctx, D, V, doc_ptr, term, count, cat, J, None, R, 0, args.seed, 0, None, maxiter, 0.0, args.waves, outputs=outputs)


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


run = lambda: mmm.extract_signatures(X, cat, n_new=J, restarts=R, seed=args.seed, maxiter=args.maxiter, tol=0.0)
clock(run)
ts = []
for _ in range(args.rounds):
    t, ex = clock(run)
    ts.append(t)
# the library call alone, at the pinned geometry (--waves)
clock(raw)
tr = [clock(raw)[0] for _ in range(args.rounds)]
# (c) the host restatement: one restart, fewer iterations; its rows must be the device's at that count
t0 = time.perf_counter()
ref = E.extract(D, F, J, V, doc_ptr, term, count, cat, None, 1, 0, args.seed, 0, None, args.host_iters, 0.0)
t_c = time.perf_counter() - t0
dev = raw(1, args.host_iters, ("w", "unexplained"))
same = bool(np.array_equal(ref.sig, dev["sig"]) and np.array_equal(ref.w, dev["w"]) and np.array_equal(ref.unexplained, dev["unexplained"]))
flop = float(R) * args.maxiter * D * (4.0 * (F + J) + 2.0 * J) * V

out = {"device": ctx.device_name(), "D": D, "V": V, "F": F, "J": J, "restarts": R, "maxiter": args.maxiter, "waves": args.waves, "rounds": args.rounds,
       "mutations": int(count.sum()), "b_end_to_end_s": statistics.median(ts), "b_all_s": ts, "raw_call_at_waves_s": statistics.median(tr), "best": ex.best, "ll_best": ex.ll,
       "ll_spread": float(ex.ll_all.max() - ex.ll_all.min()), "new_row_exposure_mean": ex.exposures[:, F:].mean(axis=0).tolist(),
       "c_numpy_iters": args.host_iters, "c_numpy_one_restart_s": t_c, "c_numpy_scaled_s": t_c * R * args.maxiter / args.host_iters,
       "numpy_equals_device": same, "approx_flop": flop}
out["c_over_b"] = out["c_numpy_scaled_s"] / out["b_end_to_end_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh) if "k_extract<" in r["Name"]]
    calls = sum(int(r["Calls"]) for r in rows)
    ns = sum(float(r["TotalDurationNs"]) for r in rows)
    out["a_kernel_calls"] = calls
    out["a_kernel_ms"] = ns / calls / 1e6
    out["a_kernel_gflops"] = flop / (ns / calls)
    out["a_us_per_restart_iteration_on_one_cu"] = ns / calls / 1e3 / args.maxiter / max(1.0, R / 256.0)
    out["b_over_a"] = out["b_end_to_end_s"] / (ns / calls / 1e9)
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
