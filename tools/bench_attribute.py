#!/usr/bin/env python3
"""Mutation attribution on the BRCA-EU SNV table (560 samples x 96 terms) against the 86-row catalogue of tools/bench_refit.py (ten signatures
fitted on the table plus 76 Dirichlet(0.3) decoys): `allowed` = the sets a BIC refit chose, a query on every non-zero entry, B = 1000.
  (a) the kernels alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls) in a run of its own and hand
      the summary to the main run with --kernel-stats FILE; the replicate launch is also timed by HIP events around it (profile_begin / end);
  (b) attribute_mutations end to end (host clock around the call, which ends in a device synchronise);
  (c) the same numbers composed from the entries that existed before, on the same replicates: mmm_resample_counts (B x nnz counts to the
      host), mmm_refit_exposures on the stacked corpus of B x D samples through the raw binding, B x D x C weights back, the posteriors and
      the fixed-point sums in numpy (per sample, over its allowed signatures only) -- same session, alternating with (b).
Checks that (b) and (c) give the same mean, sd and p_top bit for bit, and reports (c) / (b).
Usage: python tools/bench_attribute.py [--B 1000] [--rounds 2] [--kernel-stats FILE] [--out profiles/attribute_brca.json]
       python tools/bench_attribute.py --kernel-only 1
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
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--maxiter", type=int, default=1000)
ap.add_argument("--tol", type=float, default=1e-9)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()
at = mmm.attribute

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
chosen = mmm.refit_exposures(X, cat, maxiter=args.maxiter, tol=args.tol)
allowed = np.ascontiguousarray(chosen.active.T, dtype=np.uint8)
qs = at._queries(None, doc_ptr, term, count, D, V)
Q = qs.shape[0]
q_ptr = np.concatenate([[0], np.cumsum(np.bincount(qs[:, 0], minlength=D))]).astype(np.int64)


def fused():
    return mmm.attribute_mutations(X, cat, allowed=chosen, B=B, seed=args.seed, maxiter=args.maxiter, tol=args.tol, ctx=ctx)


if args.kernel_only:
    for _ in range(args.kernel_only):
        fused()
    sys.exit(0)


def composed():
    """-> (mean, sd, p_top) [Q, C] from the entries the parent commit has, on the replicates the fused call draws"""
    nnz = int(doc_ptr[-1])
    rc = mmm.bootstrap._resample_csr(ctx, D, doc_ptr, count, B, 0, args.seed, 0)
    dps = np.concatenate([(doc_ptr[:-1][None, :] + nnz * np.arange(B, dtype=np.int64)[:, None]).ravel(), [B * nnz]])
    w = mmm.refit._raw(ctx, B * D, V, dps, np.tile(term, B), rc.ravel(), cat, np.tile(allowed, (B, 1)), None, args.maxiter, args.tol, outputs="w")["w"].reshape(B, D, C)
    s = np.zeros((Q, C), dtype=np.uint64); ss = np.zeros((Q, C), dtype=np.uint64); top = np.zeros((Q, C), dtype=np.int64); void = np.zeros(Q, dtype=np.int64)
    for d in range(D):
        Ad = np.flatnonzero(allowed[d])
        e = np.arange(q_ptr[d], q_ptr[d + 1])
        if not Ad.size or not e.size or not count[doc_ptr[d]:doc_ptr[d + 1]].sum():
            continue
        num = w[:, d, Ad][:, :, None] * P[Ad][:, qs[e, 1]][None, :, :]            # [B, n, nq]: w_c P[c][v]
        qv = np.cumsum(num, axis=1)[:, -1, :]                                      # sequentially over c ascending
        rho = np.zeros_like(num)
        np.divide(num, qv[:, None, :], out=rho, where=qv[:, None, :] > 0)
        x = np.floor(rho * at.FX_ONE).astype(np.uint64)
        s[np.ix_(e, Ad)] = x.sum(axis=0).T
        ss[np.ix_(e, Ad)] = (x * x).sum(axis=0).T
        ok = qv > 0                                                                # [B, nq]
        void[e] = (~ok).sum(axis=0)
        best = Ad[rho.argmax(axis=1)]                                              # [B, nq]: the first largest, ties to the lowest c
        np.add.at(top, (np.broadcast_to(e, ok.shape)[ok], best[ok]), 1)
    mean, sd = at._moments(s, ss, B - void)
    return mean, sd, top / float(B)


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, r


clock(lambda: mmm.attribute_mutations(X, cat, allowed=chosen, B=8, seed=args.seed, maxiter=args.maxiter, tol=args.tol, ctx=ctx))
t_b, t_c = [], []
for _ in range(args.rounds):
    t, res = clock(fused)
    t_b.append(t)
    t, (mean_c, sd_c, ptop_c) = clock(composed)
    t_c.append(t)
same = bool(np.array_equal(res.mean, mean_c, equal_nan=True) and np.array_equal(res.sd, sd_c, equal_nan=True) and np.array_equal(res.p_top, ptop_c))
# the replicate launch by HIP events around it
ctx.profile_begin()
fused()
n_ev, ms_ev = ctx.profile_end()
# where the end-to-end time goes beside the kernels: the raw call alone, and the observed phase alone
raw = lambda b: at._raw(ctx, D, V, doc_ptr, term, count, cat, allowed, q_ptr, qs[:, 1], qs[:, 2], None, 0, b, 0, args.seed, 0, args.maxiter, args.tol)
t_raw, r = clock(lambda: raw(B))
t_obs, _ = clock(lambda: raw(0))

top_post = res.posterior.max(axis=1)
lead = res.posterior.argmax(axis=1)
sd_top = res.sd[np.arange(Q), lead]
out = {"device": ctx.device_name(), "D": D, "V": V, "C": C, "B": B, "Q": int(Q), "maxiter": args.maxiter, "tol": args.tol, "rounds": args.rounds,
       "allowed_per_sample_mean": float(allowed.sum(axis=1).mean()), "status_counts": {str(k): int((res.status == k).sum()) for k in (0, 3, 4)},
       "replicates_run": int((res.status == 0).sum()) * B, "em_iterations_total": int(res.iters.sum()), "void_replicates": int(res.void.sum()),
       "posterior_of_top_median": float(np.median(top_post)), "sd_of_top_median": float(np.nanmedian(sd_top)),
       "share_of_queries_with_top_posterior_below_0.5": float((top_post < 0.5).mean()),
       "b_attribute_mutations_s": statistics.median(t_b), "b_all_s": t_b, "c_composed_s": statistics.median(t_c), "c_all_s": t_c,
       "composed_equals_fused_bit_for_bit": same, "raw_call_s": t_raw, "raw_call_observed_only_s": t_obs, "rep_kernel_event_spans": n_ev, "rep_kernel_event_ms": ms_ev}
out["c_over_b"] = out["c_composed_s"] / out["b_attribute_mutations_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh) if "k_attribute" in r["Name"]]
    for key, name in (("obs", "k_attribute_obs"), ("rep", "k_attribute_rep")):
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        if calls:
            out["a_%s_calls" % key] = calls
            out["a_%s_ms_total" % key] = sum(float(r["TotalDurationNs"]) for r in sel) / 1e6
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
