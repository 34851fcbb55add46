#!/usr/bin/env python3
"""Cross-validated C-index with permutation p-values on the BRCA-EU exposures: θ of an LDA with K = 10 fitted to
tests/golden/brca-eu_snv_counts.tsv (560 samples); synthetic times whose hazard rises with the first signature, about 35 % of the samples
censored, times rounded to 0.01 so that ties exist; the default arguments of `cox_exposures` (four penalties, 5 folds, 5 repeats) with
B = 10^3 permutations: 1001 x 100 cross-validation fits and 4 all-sample fits in two launches.
  (a) the kernel alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_cox_exposures) in a
      run of its own and hand the summary to the main run with --kernel-stats FILE;
  (b) cox_exposures end to end (host clock around the call, whose library part ends in a device synchronise), warmed up, median of
      --rounds; the library call alone (with the block geometry pinned by --waves) is reported beside it;
  (c) the same definition in numpy on the host (tests/cox_ref.py): --host-permutations permutations, scaled to the permutations of (b) by
      (B + 1) / (host permutations + 1), the identity counting as one; its outputs must be the device's in every bit.
--shape D,P replaces the BRCA inputs by synthetic ones of that size.
Usage: python tools/bench_cox.py [--permutations 1000] [--waves 0] [--rounds 5] [--host-permutations 4] [--shape 2000,30]
                                 [--kernel-stats FILE] [--out profiles/cox_brca.json]
       python tools/bench_cox.py --kernel-only 3
Prints one JSON line; --out appends it to the file (one line per configuration)."""
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
import cox_ref as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--permutations", type=int, default=1000)
ap.add_argument("--waves", type=int, default=0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-permutations", type=int, default=4)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--shape", default=None)
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()
ctx = mmm.default_context()
rng = np.random.default_rng(args.seed)
B, R, F = args.permutations, 5, 5
PEN = (0.1, 1.0, 10.0, 100.0)

if args.shape:
    D, P = (int(v) for v in args.shape.split(","))
    E = rng.random((D, P))
else:
    _, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
    X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
    g = mmm.LDA(10, 0.1, 0.1, 96, X, λ0=rng.integers(1, 101, size=(96, 10)).astype(np.float64))
    mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
    th = np.asarray(g.θ, dtype=np.float64)
    g.close()
    E = np.ascontiguousarray((th / th.sum(axis=0, keepdims=True)).T)      # [560, 10]
    D, P = E.shape
z, _, _ = mmm.classify.standardise(E)
te = rng.exponential(size=D) / np.exp(0.8 * z[:, 0])
tc = rng.exponential(size=D) * 1.9
times, event = np.round(np.minimum(te, tc), 2), (te <= tc).astype(np.uint8)
fold = mmm.cox.make_folds(event, None, F, R, args.seed)


def raw(B=B, outputs=()):
    return mmm.cox._raw(ctx, z, times, event, None, fold, F, PEN, 30, 1e-8, B, 0, args.seed, 0, args.waves, outputs=outputs)


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


run = lambda: mmm.cox_exposures(E, times, event, penalties=PEN, folds=F, repeats=R, permutations=B, seed=args.seed)
clock(run)
ts = []
for _ in range(args.rounds):
    t, res = clock(run)
    ts.append(t)
clock(raw)
tr = []
for _ in range(args.rounds):
    t, _ = clock(raw)
    tr.append(t)
# (c) the host restatement on a few permutations: its outputs must be the device's
hb = args.host_permutations
t0 = time.perf_counter()
ref = K.cox(z, times, event, None, fold, F, PEN, 30, 1e-8, hb, 0, args.seed)
t_c = time.perf_counter() - t0
dev = raw(hb, outputs=mmm.cox.OPTIONAL)
same = all(np.ascontiguousarray(dev[k]).tobytes() == np.ascontiguousarray(getattr(ref, k)).tobytes() and dev[k].dtype == getattr(ref, k).dtype for k in dev)

out = {"device": ctx.device_name(), "D": D, "P": P, "events": int(event.sum()), "censored_fraction": float(1.0 - event.mean()), "distinct_times": int(np.unique(times).size), "penalties": list(PEN), "folds": F, "repeats": R, "permutations": B,
       "fits_per_call": (B + 1) * R * F * len(PEN) + len(PEN), "waves": args.waves, "rounds": args.rounds, "b_end_to_end_s": statistics.median(ts), "b_all_s": ts,
       "raw_call_s": statistics.median(tr), "c_index": [float(v) for v in res.c_index], "best": res.best, "p_best": res.p_best, "fit_events": res.events, "iterations_all_samples": dev["full_iters"][:, 0].tolist(),
       "c_numpy_permutations": hb, "c_numpy_s": t_c, "c_numpy_scaled_s": t_c * (B + 1) / (hb + 1), "numpy_equals_device": bool(same)}
out["c_over_raw_call"] = out["c_numpy_scaled_s"] / out["raw_call_s"]
out["c_over_end_to_end"] = out["c_numpy_scaled_s"] / out["b_end_to_end_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [q for q in csv.DictReader(fh) if "k_cox" in q["Name"]]
    calls = sum(int(q["Calls"]) for q in rows)
    ns = sum(float(q["TotalDurationNs"]) for q in rows)
    out["a_launches"] = calls                                             # two per call: the identity, then the permutations
    out["a_kernel_ms_per_call"] = ns / (calls / 2) / 1e6
    out["a_us_per_permutation"] = out["a_kernel_ms_per_call"] * 1e3 / B   # throughput: many permutations are in flight
    out["a_kernel_rows"] = [dict(calls=int(q["Calls"]), total_ns=float(q["TotalDurationNs"]), min_ns=float(q["MinNs"]), max_ns=float(q["MaxNs"])) for q in rows]
    out["raw_over_a"] = out["raw_call_s"] / (out["a_kernel_ms_per_call"] / 1e3)
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "a") as fh:
        fh.write(line + "\n")
