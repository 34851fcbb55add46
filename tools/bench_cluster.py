#!/usr/bin/env python3
"""Consensus clustering of the BRCA-EU samples by their SNV exposures: θ of an LDA with K = 10 fitted to tests/golden/brca-eu_snv_counts.tsv
(560 samples), ks = 2 .. 9, 1000 replicates, subsample 0.8, Hellinger features.
  (a) the two kernels alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_cluster_samples) in a
      run of its own and hand the summary to the main run with --kernel-stats FILE;
  (b) cluster_samples end to end (host clock around the call, whose library part ends in a device synchronise), warmed up, median of --rounds;
      the library call alone (with the block geometry pinned by --waves / --placement) and the host linkage alone are reported beside it;
  (c) the same definition in numpy on the host (tests/cluster_ref.py): --host-replicates replicates of every k, scaled to the replicates of (b);
      its outputs must be the device's.
Usage: python tools/bench_cluster.py [--replicates 1000] [--waves 0] [--placement 0] [--rounds 5] [--host-replicates 4] [--kernel-stats FILE]
                                     [--out profiles/cluster_brca.json]
       python tools/bench_cluster.py --kernel-only 3
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
import cluster_ref as C  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--replicates", type=int, default=1000)
ap.add_argument("--subsample", type=float, default=0.8)
ap.add_argument("--maxiter", type=int, default=100)
ap.add_argument("--waves", type=int, default=0)
ap.add_argument("--placement", type=int, default=0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-replicates", type=int, default=4)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()

_, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
ctx = mmm.default_context()
rng = np.random.default_rng(args.seed)
g = mmm.LDA(10, 0.1, 0.1, 96, X, λ0=rng.integers(1, 101, size=(96, 10)).astype(np.float64))
mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
th = np.asarray(g.θ, dtype=np.float64)
g.close()
E = np.ascontiguousarray((th / th.sum(axis=0, keepdims=True)).T)          # [560, 10]
x = np.sqrt(E / E.sum(axis=1, keepdims=True))
D, P = x.shape
ks = list(range(2, 10))
B = args.replicates
keep = mmm.cluster._keep(args.subsample)


def raw(B=B, outputs=("together", "same", "ambiguous", "valid")):
    return mmm.cluster._raw(ctx, x, ks, B, 0, keep, args.seed, 0, args.maxiter, 100, 900, args.waves, args.placement, outputs=outputs)


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


run = lambda: mmm.cluster_samples(E, ks=ks, replicates=B, subsample=args.subsample, seed=args.seed, maxiter=args.maxiter)
clock(run)
ts = []
for _ in range(args.rounds):
    t, res = clock(run)
    ts.append(t)
clock(raw)
tr, r = [], None
for _ in range(args.rounds):
    t, r = clock(raw)
    tr.append(t)
cons = C.consensus(r["together"], r["same"])
t0 = time.perf_counter()
for i, k in enumerate(ks):
    mmm.cluster.average_linkage(1.0 - cons[i], k)
t_link = time.perf_counter() - t0
# (c) the host restatement on a few replicates; its outputs must be the device's on the same replicates
hb = args.host_replicates
t0 = time.perf_counter()
ref = C.cluster(x, ks, hb, 0, keep, args.seed, 0, args.maxiter, 100, 900)
t_c = time.perf_counter() - t0
dev = raw(hb)
same = all(np.array_equal(np.ascontiguousarray(dev[k]).view(np.uint8), np.ascontiguousarray(getattr(ref, k)).view(np.uint8))
           for k in ("labels", "iters", "inertia", "together", "same", "ambiguous", "valid"))
iters = r["iters"].astype(np.int64)

out = {"device": ctx.device_name(), "D": D, "P": P, "ks": ks, "replicates": B, "subsample": args.subsample, "maxiter": args.maxiter, "waves": args.waves,
       "placement": args.placement, "rounds": args.rounds, "b_end_to_end_s": statistics.median(ts), "b_all_s": ts, "raw_call_s": statistics.median(tr),
       "host_linkage_all_ks_s": t_link, "pac": [float(v) for v in res.pac], "k": int(res.k), "group_sizes": np.bincount(res.labels).tolist(),
       "iters_mean_per_k": iters.mean(axis=1).tolist(), "iters_max": int(iters.max()), "unsettled": res.unsettled.tolist(), "skipped": res.skipped.tolist(),
       "lloyd_iterations_total": int(iters.sum()), "c_numpy_replicates": hb, "c_numpy_s": t_c, "c_numpy_scaled_s": t_c * B / hb, "numpy_equals_device": bool(same)}
out["c_over_raw_call"] = out["c_numpy_scaled_s"] / out["raw_call_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = list(csv.DictReader(fh))
    for key, pat in (("replicates", "k_cluster_replicates"), ("pairs", "k_consensus_pairs")):
        sel = [q for q in rows if pat in q["Name"]]
        calls = sum(int(q["Calls"]) for q in sel)
        ns = sum(float(q["TotalDurationNs"]) for q in sel)
        out["a_%s_calls" % key] = calls
        out["a_%s_ms" % key] = ns / calls / 1e6
    out["a_replicates_us_per_run"] = out["a_replicates_ms"] * 1e3 / (len(ks) * B)          # throughput: many runs are in flight
    out["raw_over_a"] = out["raw_call_s"] / ((out["a_replicates_ms"] + out["a_pairs_ms"]) / 1e3)
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
