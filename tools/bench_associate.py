#!/usr/bin/env python3
"""Permutation tests of the BRCA-EU exposures against covariates: θ of an LDA with K = 10 fitted to tests/golden/brca-eu_snv_counts.tsv (560
samples); the covariates are the `cluster_samples` labels and two synthetic ones (a numeric score, a binary flag); B = 10^4 permutations.
  (a) the kernel alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_associate_exposures) in a
      run of its own and hand the summary to the main run with --kernel-stats FILE;
  (b) associate_exposures end to end (host clock around the call, whose library part ends in a device synchronise), warmed up, median of
      --rounds; the library call alone (with the block geometry pinned by --waves) is reported beside it;
  (c) the same definition in numpy on the host (tests/associate_ref.py, one integer matrix product per permutation): --host-permutations
      permutations, scaled to the permutations of (b); its outputs must be the device's.
--shape D,P,Q replaces the BRCA inputs by synthetic ones of that size (Q numeric covariates), where the product dominates.
Usage: python tools/bench_associate.py [--permutations 10000] [--waves 0] [--rounds 5] [--host-permutations 300] [--shape 4096,64,64]
                                       [--kernel-stats FILE] [--out profiles/associate_brca.json]
       python tools/bench_associate.py --kernel-only 3
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
import associate_ref as A  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--permutations", type=int, default=10000)
ap.add_argument("--waves", type=int, default=0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-permutations", type=int, default=300)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--shape", default=None)
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()
ctx = mmm.default_context()
rng = np.random.default_rng(args.seed)
B = args.permutations

if args.shape:
    D, P, Q = (int(v) for v in args.shape.split(","))
    E = rng.random((D, P))
    cov = {"c%d" % j: rng.standard_normal(D) for j in range(Q)}
else:
    _, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
    X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
    g = mmm.LDA(10, 0.1, 0.1, 96, X, λ0=rng.integers(1, 101, size=(96, 10)).astype(np.float64))
    mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
    th = np.asarray(g.θ, dtype=np.float64)
    g.close()
    E = np.ascontiguousarray((th / th.sum(axis=0, keepdims=True)).T)      # [560, 10]
    D, P = E.shape
    labels = mmm.cluster_samples(E, ks=range(2, 7), replicates=200, seed=args.seed).labels
    cov = {"cluster": labels, "score": rng.standard_normal(D) + 2.0 * E[:, 0], "flag": rng.integers(0, 2, size=D)}
names, y, levels, _ = mmm.associate._covariates(cov, None, None, D)
Q = int(np.where(levels > 0, levels, 1).sum())


def raw(B=B, outputs=()):
    return mmm.associate._raw(ctx, E, levels, y, None, B, 0, args.seed, 0, args.waves, outputs=outputs)


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


run = lambda: mmm.associate_exposures(E, cov, permutations=B, seed=args.seed)
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
# (c) the host restatement on a few permutations; its outputs must be the device's on the same permutations
hb = args.host_permutations
Rx = np.stack([A.r2(E[:, p]) for p in range(P)], axis=1)
ssx = ((Rx - (D + 1)) ** 2).sum(axis=0)
Y, w, col0 = A.columns(tuple(int(v) for v in levels), y)
t0 = time.perf_counter()
for b in range(hb):
    A.statistic(Rx, Y, A.permutation(D, None, b, args.seed), w, ssx, col0)
t_c = time.perf_counter() - t0
hs = min(hb, 20)
ref = A.associate(E, tuple(int(v) for v in levels), y, None, hs, 0, args.seed)
dev = raw(hs, outputs=("zc_obs", "maxstat"))
same = all(np.array_equal(np.ascontiguousarray(dev[k]).view(np.uint8), np.ascontiguousarray(getattr(ref, k)).view(np.uint8))
           for k in ("obs", "zc_obs", "ge", "ge_max", "maxstat"))

out = {"device": ctx.device_name(), "D": D, "P": P, "C": len(names), "Q": Q, "permutations": B, "waves": args.waves, "rounds": args.rounds,
       "b_end_to_end_s": statistics.median(ts), "b_all_s": ts, "raw_call_s": statistics.median(tr), "significant_p_adj_0.05": len(res.significant(0.05)),
       "c_numpy_permutations": hb, "c_numpy_s": t_c, "c_numpy_scaled_s": t_c * B / hb, "numpy_equals_device": bool(same)}
out["c_over_raw_call"] = out["c_numpy_scaled_s"] / out["raw_call_s"]
out["c_over_end_to_end"] = out["c_numpy_scaled_s"] / out["b_end_to_end_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [q for q in csv.DictReader(fh) if "k_assoc" in q["Name"]]
    calls = sum(int(q["Calls"]) for q in rows)
    ns = sum(float(q["TotalDurationNs"]) for q in rows)
    out["a_launches"] = calls                                             # two per call: the identity, then the permutations
    out["a_kernel_ms_per_call"] = ns / (calls / 2) / 1e6
    out["a_us_per_permutation"] = out["a_kernel_ms_per_call"] * 1e3 / B   # throughput: many permutations are in flight
    out["raw_over_a"] = out["raw_call_s"] / (out["a_kernel_ms_per_call"] / 1e3)
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
