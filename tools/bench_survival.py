#!/usr/bin/env python3
"""Permutation tests of the BRCA-EU exposures against a survival outcome: θ of an LDA with K = 10 fitted to tests/golden/brca-eu_snv_counts.tsv
(560 samples); one group covariate, the `cluster_samples` labels; synthetic times and events (hazard rising with the first signature and in
one cluster, exponential censoring, times rounded to 0.01); B = 10^4 permutations; with the scan over the cutpoints (--cuts 1) or without.
  (a) the kernel alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_survival_association) in
      a run of its own and hand the summary to the main run with --kernel-stats FILE;
  (b) survival_association end to end (host clock around the call, whose library part ends in a device synchronise), warmed up, median of
      --rounds; the library call alone (with the block geometry pinned by --waves) is reported beside it;
  (c) the same definition in numpy on the host (tests/survival_ref.py): --host-permutations permutations, scaled to the permutations of (b);
      the outputs of its first 20 must be the device's in every bit.
--shape D,P replaces the BRCA inputs by synthetic ones of that size (uniform features, three random groups), where the features' work dominates.
Usage: python tools/bench_survival.py [--cuts 1] [--permutations 10000] [--waves 0] [--rounds 5] [--host-permutations 300] [--shape 4096,64]
                                      [--kernel-stats FILE] [--out profiles/survival_brca.json]
       python tools/bench_survival.py --kernel-only 3 [--cuts 0]
Prints one JSON line; --out appends it to the file (one line per configuration)."""
import argparse
import csv
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import mmm_pkg  # noqa: E402
import survival_ref as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cuts", type=int, default=1)
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
    D, P = (int(v) for v in args.shape.split(","))
    E = rng.random((D, P))
    labels = rng.integers(0, 3, size=D)
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
hazard = np.exp(3.0 * E[:, 0] + 0.7 * (labels == labels[0]))
t_event, t_cens = rng.exponential(1.0, size=D) / hazard, rng.exponential(1.5, size=D)
times, events = np.round(np.minimum(t_event, t_cens), 2), (t_event <= t_cens).astype(np.uint8)
names, codes, levels, _ = mmm.survival._groups({"cluster": labels}, D)
m_lo = max(1, int(math.ceil(0.1 * D))) if args.cuts else 0


def raw(B=B, outputs=()):
    return mmm.survival._raw(ctx, E, levels, codes, times, events, None, m_lo, B, 0, args.seed, 0, args.waves, outputs=outputs)


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


run = lambda: mmm.survival_association(E, times, events, groups={"cluster": labels}, cutpoints=bool(args.cuts), permutations=B, seed=args.seed)
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
# (c) the host restatement on a few permutations; the outputs of the first 20 must be the device's
hb = args.host_permutations
lv = tuple(int(v) for v in levels)
t0 = time.perf_counter()
plan = S.Plan(E, lv, codes, times, events, None, m_lo)
t_plan = time.perf_counter() - t0
t0 = time.perf_counter()
for b in range(hb):
    plan.statistics(S.permutation(D, None, b, args.seed))
t_c = time.perf_counter() - t0
hs = min(hb, 20)
ref = S.survival(E, lv, codes, times, events, None, m_lo, hs, 0, args.seed)
dev = raw(hs, outputs=("z_trend", "u_group", "maxstat"))
same = all(np.ascontiguousarray(dev[k]).tobytes() == np.ascontiguousarray(getattr(ref, k)).tobytes() and dev[k].dtype == getattr(ref, k).dtype for k in dev)

out = {"device": ctx.device_name(), "D": D, "P": P, "C": len(names), "Q": int(levels.sum()), "cuts": bool(args.cuts), "m_lo": m_lo, "events": int(events.sum()),
       "permutations": B, "waves": args.waves, "rounds": args.rounds, "b_end_to_end_s": statistics.median(ts), "b_all_s": ts, "raw_call_s": statistics.median(tr),
       "significant_p_adj_0.05": len(res.significant(0.05)), "c_numpy_permutations": hb, "c_numpy_plan_s": t_plan, "c_numpy_s": t_c,
       "c_numpy_scaled_s": t_plan + t_c * B / hb, "numpy_equals_device": bool(same), "numpy_compared_permutations": hs}
out["c_over_raw_call"] = out["c_numpy_scaled_s"] / out["raw_call_s"]
out["c_over_end_to_end"] = out["c_numpy_scaled_s"] / out["b_end_to_end_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [q for q in csv.DictReader(fh) if "k_survival" in q["Name"]]
    calls = sum(int(q["Calls"]) for q in rows)
    ns = sum(float(q["TotalDurationNs"]) for q in rows)
    out["a_launches"] = calls                                             # two per call: the identity, then the permutations
    out["a_kernel_ms_per_call"] = ns / (calls / 2) / 1e6
    out["a_us_per_permutation"] = out["a_kernel_ms_per_call"] * 1e3 / B   # throughput: many permutations are in flight
    out["raw_over_a"] = out["raw_call_s"] / (out["a_kernel_ms_per_call"] / 1e3)
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "a") as fh:
        fh.write(line + "\n")
