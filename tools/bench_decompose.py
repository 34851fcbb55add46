#!/usr/bin/env python3
"""Decomposition of ten de-novo signatures (an LDA with K = 10 fitted to the BRCA-EU SNV table, tests/golden/brca-eu_snv_counts.tsv) into
mixtures of the rows of the 86-row catalogue tools/bench_refit.py builds (ten signatures of ANOTHER fit of the table plus 76 Dirichlet(0.3)
decoys), for max_size S = 3, 4, 5, 6.
  (a) the kernels alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls per S) in a run of its own
      and hand the summary to the main run with --kernel-stats FILE;
  (b) decompose_signatures end to end (host clock around the call, which ends in a device synchronise), warmed up, median of --rounds;
  (c) the same definition in vectorised numpy on the host (tests/decompose_ref.py) at S = 3 and, on --host-sigs signatures scaled to ten, at
      S = 4; its outputs must be the device's;
  (d) where scipy is present: scipy.optimize.nnls on every subset of size <= 3 of ONE signature, scaled to ten.
Usage: python tools/bench_decompose.py [--rounds 5] [--host-sigs 2] [--kernel-stats FILE] [--out profiles/decompose_brca.json]
       python tools/bench_decompose.py --kernel-only 3
Prints one JSON line."""
import argparse
import csv
import itertools
import json
import os
import re
import statistics
import sys
import time
from math import comb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import mmm_pkg  # noqa: E402
import decompose_ref as DR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--C", type=int, default=86)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-sigs", type=int, default=2)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()

_, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
ctx = mmm.default_context()
V = 96
rng = np.random.default_rng(args.seed)


def fitted():
    g = mmm.LDA(10, 0.1, 0.1, V, X, λ0=rng.integers(1, 101, size=(V, 10)).astype(np.float64))
    mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
    out = np.ascontiguousarray(g.β.T)
    g.close()
    return out


cat = np.concatenate([fitted(), rng.dirichlet(np.full(V, 0.3), size=args.C - 10)])      # the catalogue of tools/bench_refit.py
sig = fitted()                                                                           # the signatures: another start of the same fit
SIZES = (3, 4, 5, 6)

if args.kernel_only:
    for S in SIZES:
        for _ in range(args.kernel_only):
            mmm.decompose._raw(ctx, sig, cat, S)
    sys.exit(0)


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, r


out = {"device": ctx.device_name(), "n": int(sig.shape[0]), "V": V, "C": args.C, "rounds": args.rounds}
res = {}
for S in SIZES:
    clock(lambda: mmm.decompose_signatures(sig, cat, max_size=S))
    ts = []
    for _ in range(args.rounds):
        t, res[S] = clock(lambda: mmm.decompose_signatures(sig, cat, max_size=S))
        ts.append(t)
    out["S%d" % S] = {"subsets_per_signature": sum(comb(args.C, s) for s in range(1, S + 1)), "b_end_to_end_s": statistics.median(ts), "b_all_s": ts,
                      "chosen_sizes": res[S].size.tolist(), "chosen_cosine_min": float(res[S].cosine.min()),
                      "path_cosine_mean": res[S].path_cosine.mean(axis=0).tolist()}
out["match_signatures_cosine_min"] = float(mmm.match_signatures(sig, cat).cosine.min())

# (c) the host restatement on the device's own moments
_, (G, b, ss) = mmm.decompose._raw(ctx, sig, cat, 3, moments=True)
t0 = time.perf_counter()
ref = DR.search(G, b, ss, 3)
out["S3"]["c_numpy_s"] = time.perf_counter() - t0
out["S3"]["numpy_equals_device"] = bool(np.array_equal(ref[0], res[3].path_members) and np.array_equal(ref[1], res[3].path_weights) and
                                        np.array_equal(ref[3], res[3].path_cosine))
nh = min(args.host_sigs, sig.shape[0])
t0 = time.perf_counter()
ref = DR.search(G, b[:nh], ss[:nh], 4)
t4 = time.perf_counter() - t0
out["S4"].update(c_numpy_sigs=nh, c_numpy_s=t4, c_numpy_scaled_s=t4 * sig.shape[0] / nh,
                 numpy_equals_device=bool(np.array_equal(ref[0], res[4].path_members[:nh]) and np.array_equal(ref[1], res[4].path_weights[:nh])))
out["S3"]["c_over_b"] = out["S3"]["c_numpy_s"] / out["S3"]["b_end_to_end_s"]
out["S4"]["c_over_b"] = out["S4"]["c_numpy_scaled_s"] / out["S4"]["b_end_to_end_s"]

# (d) per-subset scipy.optimize.nnls, one signature
try:
    from scipy.optimize import nnls
except ImportError:
    nnls = None
if nnls is not None:
    t0 = time.perf_counter()
    best = 0.0
    for s in (1, 2, 3):
        for T in itertools.combinations(range(args.C), s):
            best = max(best, ss[0] - nnls(cat[list(T)].T, sig[0])[1] ** 2)
    t = time.perf_counter() - t0
    out["S3"].update(d_scipy_nnls_one_signature_s=t, d_scipy_scaled_s=t * sig.shape[0], d_over_b=t * sig.shape[0] / out["S3"]["b_end_to_end_s"],
                     d_best_gain_minus_device=float(best - res[3].path_cosine[0].max() ** 2 * ss[0]))

if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh) if "k_decompose" in r["Name"]]
    out["a_kernels"] = {re.search(r"k_decompose_\w+(<[^>]*>)?", r["Name"]).group(0): {"calls": int(r["Calls"]), "mean_us": float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3}
                        for r in rows}
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
