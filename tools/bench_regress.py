#!/usr/bin/env python3
"""Freedman-Lane permutation tests of the BRCA-EU exposures against covariates given adjusters: θ of an LDA with K = 10 fitted to
tests/golden/brca-eu_snv_counts.tsv (560 samples); three tested covariates (the `cluster_samples` labels reduced to two groups, a numeric score,
a binary flag) and two numeric adjusters (a synthetic age and the mutation burden); B = 10^4 permutations.
  (a) the kernel alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_regress_exposures) in a
      run of its own and hand the summary to the main run with --kernel-stats FILE;
  (b) the library call alone (with the block geometry pinned by --waves), warmed up, median of --rounds; --sweep also times it under 1, 2, 4, 8
      and 16 waves per block;
  (c) regress_exposures end to end (host clock around the call, whose library part ends in a device synchronise), warmed up, median of --rounds;
  (d) the baseline, never the code under test: numpy on the host in its natural form, one f64 matrix product [A + Q, D] x [D, P] per permutation
      on rows gathered through a numpy permutation (not the stripe-order restatement): --host-permutations permutations, scaled to those of (b);
  (e) associate_exposures on the same features and tested covariates, the integer yardstick.
The device outputs are compared bit for bit with tests/regress_ref.py on a few permutations.
--shape D,P,Q,A replaces the BRCA inputs by synthetic ones of that size (Q numeric tested covariates, A - 1 numeric adjusters).
Usage: python tools/bench_regress.py [--permutations 10000] [--waves 0] [--rounds 5] [--host-permutations 300] [--shape 4096,64,64,8] [--sweep]
                                     [--kernel-stats FILE] [--out profiles/regress_brca.json]
       python tools/bench_regress.py --kernel-only 3
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
import regress_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--permutations", type=int, default=10000)
ap.add_argument("--waves", type=int, default=0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-permutations", type=int, default=300)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--shape", default=None)
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()
ctx = mmm.default_context()
rng = np.random.default_rng(args.seed)
B = args.permutations

if args.shape:
    D, P, Q, A = (int(v) for v in args.shape.split(","))
    E = rng.random((D, P))
    cov = {"c%d" % j: rng.standard_normal(D) for j in range(Q)}
    adj = {"a%d" % j: rng.standard_normal(D) for j in range(A - 1)}
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
    age = np.round(rng.uniform(30.0, 85.0, size=D))
    cov = {"cluster": (labels == labels[0]).astype(int), "score": rng.standard_normal(D) + 2.0 * E[:, 0] + 0.02 * age, "flag": rng.integers(0, 2, size=D)}
    adj = {"age": age, "burden": snv.sum(axis=0).astype(np.float64)}
names, y, levels, _ = mmm.associate._covariates(cov, None, None, D)
an, ay, al, _ = mmm.associate._covariates(adj, None, None, D) if adj else ([], np.zeros((D, 0)), np.zeros(0, dtype=np.int32), None)
d = mmm.regress._design(E, y, levels, names, ay, al, an, True)
A, Q = d["qz"].shape[1], d["w"].shape[1]


def raw(B=B, outputs=(), waves=args.waves):
    return mmm.regress._raw(ctx, d["e"], d["qz"], d["cols"], d["w"], None, B, 0, args.seed, 0, waves, outputs=outputs)


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


def median_of(fn):
    clock(fn)
    ts = [clock(fn)[0] for _ in range(args.rounds)]
    return statistics.median(ts), ts


run = lambda: mmm.regress_exposures(E, cov, adj or None, permutations=B, seed=args.seed)
t_c, all_c = median_of(run)
res = run()
t_b, all_b = median_of(raw)
sweep = {str(wv): median_of(lambda: raw(waves=wv))[0] for wv in (1, 2, 4, 8, 16)} if args.sweep else None
t_e, _ = median_of(lambda: mmm.associate_exposures(E, cov, permutations=B, seed=args.seed))
t_e_raw, _ = median_of(lambda: mmm.associate._raw(ctx, E, levels, y, None, B, 0, args.seed, 0, 0, outputs=()))
# (d) the natural host form: gather the rows, one f64 product, the two short sums; never the code under test
hb = args.host_permutations
X = np.ascontiguousarray(np.concatenate([d["qz"], d["w"]], axis=1).T)      # [A + Q, D]
ss = (d["e"] * d["e"]).sum(axis=0)
col0 = np.concatenate([[0], np.cumsum(d["cols"])]).astype(int)
prng = np.random.default_rng(1)
t0 = time.perf_counter()
for b in range(hb):
    G = X @ d["e"][prng.permutation(D)]
    rz = ss - (G[:A] * G[:A]).sum(axis=0)
    num = np.add.reduceat(G[A:] * G[A:], col0[:-1], axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(rz > 0, num / rz, 0.0)
    t.max(axis=1)
t_d = time.perf_counter() - t0
# the device's outputs are the restatement's, on a few permutations
hs = 8 if D * P * (A + Q) > 10 ** 6 else 20
ref = R.regress(d["e"], d["qz"], d["cols"], d["w"], None, hs, 0, args.seed)
dev = raw(hs, outputs=("u_obs", "rz_obs", "maxstat"))
same = all(np.array_equal(np.ascontiguousarray(dev[k]).view(np.uint8), np.ascontiguousarray(getattr(ref, k)).view(np.uint8))
           for k in ("obs", "u_obs", "rz_obs", "ge", "ge_max", "maxstat"))

out = {"device": ctx.device_name(), "D": D, "P": P, "C": len(names), "Q": Q, "A": A, "permutations": B, "waves": args.waves, "rounds": args.rounds,
       "b_raw_call_s": t_b, "b_all_s": all_b, "c_end_to_end_s": t_c, "c_all_s": all_c, "significant_p_adj_0.05": len(res.significant(0.05)),
       "d_numpy_permutations": hb, "d_numpy_s": t_d, "d_numpy_scaled_s": t_d * B / hb, "e_associate_end_to_end_s": t_e, "e_associate_raw_call_s": t_e_raw,
       "restatement_equals_device": bool(same), "f64_mac_per_call": float(B) * D * P * (A + Q)}
out["d_over_raw_call"] = out["d_numpy_scaled_s"] / t_b
out["d_over_end_to_end"] = out["d_numpy_scaled_s"] / t_c
out["raw_call_over_associate_raw_call"] = t_b / t_e_raw
if sweep:
    out["b_raw_call_s_by_waves"] = sweep
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [q for q in csv.DictReader(fh) if "k_regress" in q["Name"]]
    calls = sum(int(q["Calls"]) for q in rows)
    ns = sum(float(q["TotalDurationNs"]) for q in rows)
    out["a_launches"] = calls                                             # two per call: the identity, then the permutations
    out["a_kernel_ms_per_call"] = ns / (calls / 2) / 1e6
    out["a_us_per_permutation"] = out["a_kernel_ms_per_call"] * 1e3 / B   # throughput: many permutations are in flight
    out["a_f64_gmac_per_s"] = out["f64_mac_per_call"] / (out["a_kernel_ms_per_call"] / 1e3) / 1e9
    out["raw_over_a"] = t_b / (out["a_kernel_ms_per_call"] / 1e3)
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
