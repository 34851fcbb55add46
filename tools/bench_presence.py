#!/usr/bin/env python3
"""Signature presence test on the BRCA-EU SNV table (560 samples x 96 terms) against the 86-row catalogue of tools/bench_refit.py (ten
signatures fitted on the table plus 76 Dirichlet(0.3) decoys): `allowed` = the sets a BIC refit chose, 3 targets (two fitted signatures and
a decoy), B = 1000 replicates per tested pair.
  (a) the kernels alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_presence_test) in a run
      of its own and hand the summary to the main run with --kernel-stats FILE;
  (b) signature_presence end to end (host clock around the call, which ends in a device synchronise);
  (c) the same test composed from the entries that existed before (the pairs are numbered differently there, so the draws differ): per target a plain refit without and with the target (the observed
      statistic), simulate_counts from the null fits of the pairs that need replicates, and two stacked plain refits of the B x pairs
      replicate samples -- same session, alternating with (b).  The stacked refits go through the raw binding on a dense CSR built with
      numpy, as refit_exposures' own bootstrap does: the list-of-matrices form of the public entry would add minutes of Python;
  (d) the numpy restatement (tests/presence_ref.py) on --host-docs samples, one target and --host-B replicates, scaled by EM iterations.
Reports (c) / (b), the share of replicates whose statistic is exactly 0 (the larger fit skipped by the score rule, or clamped), and checks
that (b) and (c) count the same replicates at or above the observed statistic.
Usage: python tools/bench_presence.py [--B 1000] [--rounds 2] [--kernel-stats FILE] [--out profiles/presence_brca.json]
       python tools/bench_presence.py --kernel-only 2
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
import presence_ref as PR  # noqa: E402
import refit_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--C", type=int, default=86)
ap.add_argument("--B", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--targets", type=int, nargs="+", default=[2, 6, 40])
ap.add_argument("--host-docs", type=int, default=6)
ap.add_argument("--host-B", type=int, default=10)
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
D, V, C, B = len(X), 96, args.C, args.B
rng = np.random.default_rng(args.seed)
g = mmm.LDA(10, 0.1, 0.1, V, X, λ0=rng.integers(1, 101, size=(V, 10)).astype(np.float64))
mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
cat = np.concatenate([np.ascontiguousarray(g.β.T), rng.dirichlet(np.full(V, 0.3), size=C - 10)])
g.close()
P = R.normalise(cat)
N = np.asarray([x[:, 1].sum() for x in X], dtype=np.int64)
chosen = mmm.refit_exposures(X, cat, maxiter=args.maxiter, tol=args.tol)
allowed = np.ascontiguousarray(chosen.active.T, dtype=np.uint8)
targets = np.asarray(args.targets, dtype=np.int32)
T = targets.size


def fused(keep=False):
    return mmm.signature_presence(X, cat, targets, allowed=chosen, B=B, seed=args.seed, maxiter=args.maxiter, tol=args.tol, keep_replicates=keep, ctx=ctx)


if args.kernel_only:
    for _ in range(args.kernel_only):
        fused()
    sys.exit(0)


def plain(D_, dp, tm, cn, al):
    return mmm.refit._raw(ctx, D_, V, dp, tm, cn, cat, al, None, args.maxiter, args.tol)


def composed():
    """-> (count_ge [T, D], status [T, D]) from the entries the parent commit has"""
    ge = np.zeros((T, D), dtype=np.int64); status = np.zeros((T, D), dtype=np.int8)
    for ti, t in enumerate(targets):
        a0 = allowed.copy(); a0[:, t] = 0
        a1 = allowed.copy(); a1[:, t] = 1
        f0, f1 = plain(D, doc_ptr, term, count, a0), plain(D, doc_ptr, term, count, a1)
        lam = np.where(f1["unexplained"] < f0["unexplained"], np.inf, np.maximum(2.0 * (f1["ll_doc"] - f0["ll_doc"]), 0.0))
        # without the score rule a statistic that the larger fit leaves a hair above 0 cannot be told from a real one: what tests/test_presence_cpu.py
        # bounds by 1e-4 is taken as 0 here, in the composed path's favour
        lam[lam < 1e-4] = 0.0
        st = np.where((N == 0) | (a0.sum(axis=1) == 0), 3, np.where(lam == 0, 1, np.where(np.isinf(lam), 2, 0)))
        status[ti] = st
        ge[ti, st == 1] = B
        docs = np.flatnonzero(st == 0)
        if not docs.size:
            continue
        sim = mmm.simulate_counts(f0["w"][docs].T, P.T, N[docs], B=B, seed=args.seed, ctx=ctx)              # [B, docs, V]
        n = B * docs.size
        dp = np.arange(n + 1, dtype=np.int64) * V
        tm = np.tile(np.arange(V, dtype=np.int32), n)
        r0, r1 = plain(n, dp, tm, sim.ravel(), np.tile(a0[docs], (B, 1))), plain(n, dp, tm, sim.ravel(), np.tile(a1[docs], (B, 1)))
        rep = np.maximum(2.0 * (r1["ll_doc"] - r0["ll_doc"]), 0.0).reshape(B, docs.size)
        ge[ti, docs] = (rep >= lam[docs][None, :]).sum(axis=0)
    return ge, status


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, r


clock(lambda: mmm.signature_presence(X, cat, targets, allowed=chosen, B=8, seed=args.seed, maxiter=args.maxiter, tol=args.tol, ctx=ctx))
t_b, t_c = [], []
for _ in range(args.rounds):
    t, res = clock(fused)
    t_b.append(t)
    t, (ge_c, st_c) = clock(composed)
    t_c.append(t)
tested = res.status == 0
# the composed path draws item (ti, d) as document number `position among the tested` of its own call, the fused one as item ti D + d: the
# two see different random words, so their counts agree in distribution, not one by one
p_b, p_c = (1.0 + res.count_ge[tested]) / (B + 1.0), (1.0 + ge_c[tested & (st_c == 0)]) / (B + 1.0)

# (d) the host restatement on a few samples of the first target
nh = min(args.host_docs, D)
sub = PR.PCorpus("host", nh, C, V, doc_ptr[:nh + 1], term, count, cat, allowed[:nh], targets[:1], args.maxiter, args.tol, args.host_B, args.seed, 0)
t0 = time.perf_counter()
ref = PR.presence(sub)
t_d = time.perf_counter() - t0
dev = mmm.presence._raw(ctx, nh, V, doc_ptr[:nh + 1], term, count, cat, targets[:1], allowed[:nh], args.host_B, 0, args.seed, 0, args.maxiter, args.tol)
same = bool(np.array_equal(ref.w_null, dev["w_null"]) and np.array_equal(ref.status, dev["status"]) and np.array_equal(ref.iters, dev["iters"])
            and np.array_equal(ref.count_zero, dev["count_zero"]) and np.array_equal(ref.count_ge, dev["count_ge"]))
share = float(ref.iters.sum()) / float(res.iters.sum())

out = {"device": ctx.device_name(), "D": D, "V": V, "C": C, "targets": [int(t) for t in targets], "B": B, "maxiter": args.maxiter, "tol": args.tol,
       "rounds": args.rounds, "allowed_per_sample_mean": float(allowed.sum(axis=1).mean()), "items": int(T * D),
       "status_counts": {str(k): int((res.status == k).sum()) for k in range(4)}, "replicates_run": int(tested.sum()) * B,
       "share_of_replicates_with_statistic_zero": float(res.count_zero[tested].sum()) / max(1, int(tested.sum()) * B),
       "em_iterations_total": int(res.iters.sum()), "significant_at_0.01": int(res.significant(0.01).sum()),
       "b_signature_presence_s": statistics.median(t_b), "b_all_s": t_b, "c_composed_s": statistics.median(t_c), "c_all_s": t_c,
       "composed_status_equals": bool(np.array_equal(st_c, res.status)), "p_mean_fused": float(p_b.mean()), "p_mean_composed": float(p_c.mean()) if p_c.size else None,
       "d_numpy_docs": nh, "d_numpy_B": args.host_B, "d_numpy_s": t_d, "d_numpy_scaled_s": t_d / share, "d_subset_share_of_iterations": share,
       "numpy_equals_device_on_subset": same}
out["c_over_b"] = out["c_composed_s"] / out["b_signature_presence_s"]
out["d_over_b"] = out["d_numpy_scaled_s"] / out["b_signature_presence_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh) if "k_presence" in r["Name"]]
    for key, name in (("obs", "k_presence_obs"), ("rep", "k_presence_rep")):
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        if calls:
            out["a_%s_calls" % key] = calls
            out["a_%s_ms_per_launch" % key] = sum(float(r["TotalDurationNs"]) for r in sel) / calls / 1e6
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
