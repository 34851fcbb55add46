#!/usr/bin/env python3
"""Two-set comparison test on the BRCA-EU SNV table (560 samples x 96 terms) against the 86-row catalogue of tools/bench_refit.py (ten
signatures fitted on the table plus 76 Dirichlet(0.3) decoys).  Every sample's mutations are split into two sets by `split_counts` with two
folds under a fixed seed; in every --plant-every-th sample set b also receives --plant-share x N_b extra mutations drawn from one fitted
signature.  `allowed` = the sets a BIC refit of the POOLED table chose, B = 1000 permutations per sample.
  (a) the kernels alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_compare_exposures and
      N of mmm_deal_counts on the pooled table, the selection and dealing without the fits) in a run of its own and hand the summary to the
      main run with --kernel-stats FILE;
  (b) compare_exposures end to end (host clock around the call, which ends in a device synchronise);
  (c) the same test composed from the entries that existed before: three plain refits for the observed statistic, the dealing on the host in
      numpy (Generator.multivariate_hypergeometric: the same conditional distribution, other draws -- numpy's vectorised form of it, far
      faster than the restatement's lexsort), and two stacked plain refits of the B x D replicate samples through the raw binding on a
      dense CSR, --chunk replicates at a time -- same session, alternating with (b);
  (d) the numpy restatement (tests/compare_ref.py) on --host-docs samples and --host-B replicates, scaled by EM iterations.
Usage: python tools/bench_compare.py [--B 1000] [--rounds 2] [--kernel-stats FILE] [--out profiles/compare_brca.json]
       python tools/bench_compare.py --kernel-only 2
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
import compare_ref as CR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--C", type=int, default=86)
ap.add_argument("--B", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--chunk", type=int, default=250)
ap.add_argument("--plant-every", type=int, default=8)
ap.add_argument("--plant-share", type=float, default=0.3)
ap.add_argument("--plant-signature", type=int, default=2)
ap.add_argument("--host-docs", type=int, default=4)
ap.add_argument("--host-B", type=int, default=6)
ap.add_argument("--maxiter", type=int, default=1000)
ap.add_argument("--tol", type=float, default=1e-9)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--kernel-calls", type=int, default=2, help="the N of the --kernel-only run that --kernel-stats summarises")
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()

_, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
ctx = mmm.default_context()
D, V, C, B = len(X), 96, args.C, args.B
rng = np.random.default_rng(args.seed)
g = mmm.LDA(10, 0.1, 0.1, V, X, λ0=rng.integers(1, 101, size=(V, 10)).astype(np.float64))
mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
cat = np.concatenate([np.ascontiguousarray(g.β.T), rng.dirichlet(np.full(V, 0.3), size=C - 10)])
g.close()

parts = mmm.split_counts(X, 2, args.seed, ctx=ctx)


def dense(part):
    n = np.zeros((D, V), dtype=np.int64)
    for d, x in enumerate(part):
        np.add.at(n[d], x[:, 0] - 1, x[:, 1])
    return n


n_a, n_b = dense(parts[0]), dense(parts[1])
planted = np.arange(D) % args.plant_every == 0
sig = cat[args.plant_signature] / cat[args.plant_signature].sum()
for d in np.flatnonzero(planted):
    n_b[d] += rng.multinomial(int(round(args.plant_share * n_b[d].sum())), sig)
pooled = n_a + n_b
N_a, N_b = n_a.sum(axis=1), n_b.sum(axis=1)
as_X = lambda n: [np.stack([np.flatnonzero(r) + 1, r[np.flatnonzero(r)]], axis=1) for r in n]
Xa, Xb, Xp = as_X(n_a), as_X(n_b), as_X(pooled)
chosen = mmm.refit_exposures(Xp, cat, maxiter=args.maxiter, tol=args.tol)
allowed = np.ascontiguousarray(chosen.active.T, dtype=np.uint8)
pooled_csr = mmm.pack_lda(Xp)


def fused(keep=False):
    return mmm.compare_exposures(Xa, Xb, cat, allowed=chosen, B=B, seed=args.seed, maxiter=args.maxiter, tol=args.tol, keep_replicates=keep, ctx=ctx)


if args.kernel_only:
    for _ in range(args.kernel_only):
        fused()
        mmm.compare._deal_raw(ctx, D, pooled_csr[0], pooled_csr[2], N_a, B, 0, args.seed, 0)
    sys.exit(0)


def plain(D_, cn, al):
    dp = np.arange(D_ + 1, dtype=np.int64) * V
    return mmm.refit._raw(ctx, D_, V, dp, np.tile(np.arange(V, dtype=np.int32), D_), cn, cat, al, None, args.maxiter, args.tol)


def composed(host_rng):
    """-> (count_ge [D], seconds spent dealing on the host) from the entries the parent commit has"""
    fa, fb, fp = plain(D, n_a.ravel(), allowed), plain(D, n_b.ravel(), allowed), plain(D, pooled.ravel(), allowed)
    t_obs = fa["ll_doc"] + fb["ll_doc"]
    ge = np.zeros(D, dtype=np.int64)
    t_deal = 0.0
    for off in range(0, B, args.chunk):
        nb = min(args.chunk, B - off)
        t0 = time.perf_counter()
        dealt = np.stack([host_rng.multivariate_hypergeometric(pooled[d], int(N_a[d]), size=nb, method="marginals") for d in range(D)], axis=1)   # [nb, D, V]
        t_deal += time.perf_counter() - t0
        al = np.tile(allowed, (nb, 1))
        ra, rb = plain(nb * D, dealt.ravel(), al), plain(nb * D, (pooled[None] - dealt).ravel(), al)
        ge += ((ra["ll_doc"] + rb["ll_doc"]).reshape(nb, D) >= t_obs[None, :]).sum(axis=0)
    return ge, t_deal


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, r


clock(lambda: mmm.compare_exposures(Xa, Xb, cat, allowed=chosen, B=8, seed=args.seed, maxiter=args.maxiter, tol=args.tol, ctx=ctx))
t_b, t_c, t_c_deal = [], [], []
host_rng = np.random.default_rng(args.seed + 1)
for _ in range(args.rounds):
    t, res = clock(fused)
    t_b.append(t)
    t, (ge_c, td) = clock(lambda: composed(host_rng))
    t_c.append(t); t_c_deal.append(td)
tested = res.status == 0
p_b, p_c = res.p[tested], (1.0 + ge_c[tested]) / (B + 1.0)

# (d) the host restatement on a few samples
nh = min(args.host_docs, D)
pa, ta, ca = mmm.pack_lda(Xa[:nh])
pb, tb, cb = mmm.pack_lda(Xb[:nh])
sub = CR.CCorpus("host", nh, C, V, pa, ta, ca, pb, tb, cb, cat, allowed[:nh], args.maxiter, args.tol, args.host_B, args.seed, 0)
t0 = time.perf_counter()
ref = CR.compare(sub)
t_d = time.perf_counter() - t0
dev = mmm.compare._raw(ctx, nh, V, (pa, ta, ca), (pb, tb, cb), cat, allowed[:nh], args.host_B, 0, args.seed, 0, args.maxiter, args.tol)
same = bool(all(np.array_equal(getattr(ref, k), dev[k]) for k in ("w_a", "w_b", "w_pool", "status", "iters", "count_sig", "count_max", "count_ge")))
share = float(ref.iters.sum()) / float(res.iters.sum())

out = {"device": ctx.device_name(), "D": D, "V": V, "C": C, "B": B, "maxiter": args.maxiter, "tol": args.tol, "rounds": args.rounds,
       "allowed_per_sample_mean": float(allowed.sum(axis=1).mean()), "N_a_mean": float(N_a.mean()), "N_b_mean": float(N_b.mean()), "N_pooled_max": int((N_a + N_b).max()),
       "planted_samples": int(planted.sum()), "plant_share": args.plant_share, "status_counts": {str(k): int((res.status == k).sum()) for k in (0, 3)},
       "replicates_run": int(tested.sum()) * B, "em_iterations_total": int(res.iters.sum()),
       "planted_found_at_0.01": int((res.p[planted & tested] <= 0.01).sum()), "unplanted_at_0.01": int((res.p[~planted & tested] <= 0.01).sum()),
       "unplanted_tested": int((~planted & tested).sum()), "pairs_changed_at_0.05_adjusted": len(res.changed_signatures(0.05)),
       "b_compare_exposures_s": statistics.median(t_b), "b_all_s": t_b, "c_composed_s": statistics.median(t_c), "c_all_s": t_c,
       "c_host_dealing_s": statistics.median(t_c_deal), "p_mean_fused_unplanted": float(res.p[~planted & tested].mean()),
       "p_mean_composed_unplanted": float(p_c[(~planted)[tested]].mean()), "p_fused_vs_composed_max_abs_diff": float(np.abs(p_b - p_c).max()),
       "d_numpy_docs": nh, "d_numpy_B": args.host_B, "d_numpy_s": t_d, "d_numpy_scaled_s": t_d / share, "d_subset_share_of_iterations": share,
       "numpy_equals_device_on_subset": same}
out["c_over_b"] = out["c_composed_s"] / out["b_compare_exposures_s"]
out["c_without_host_dealing_over_b"] = (out["c_composed_s"] - out["c_host_dealing_s"]) / out["b_compare_exposures_s"]
out["d_over_b"] = out["d_numpy_scaled_s"] / out["b_compare_exposures_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh) if "k_compare" in r["Name"] or "k_deal" in r["Name"]]
    for key, name in (("obs", "k_compare_obs"), ("rep", "k_compare_rep"), ("deal", "k_deal_counts")):
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        if calls:
            out["a_%s_launches" % key] = calls
            out["a_%s_ms_per_call" % key] = sum(float(r["TotalDurationNs"]) for r in sel) / 1e6 / args.kernel_calls       # all launches of one call of the entry
    if "a_rep_ms_per_call" in out and "a_deal_ms_per_call" in out:
        out["a_deal_over_rep"] = out["a_deal_ms_per_call"] / out["a_rep_ms_per_call"]
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
