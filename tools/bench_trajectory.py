#!/usr/bin/env python3
"""Exposure trajectories on the BRCA-EU SNV table (560 samples x 96 terms) against the 86-row catalogue of tools/bench_refit.py (ten signatures
fitted on the table plus 76 Dirichlet(0.3) decoys).  Every sample's mutations are dealt into T = 16 bins by `split_counts` under a fixed
seed; every --plant-every-th sample gets --plant-share extra mutations from one fitted signature in each of its last four bins.
`allowed` = the sets a BIC refit of the POOLED table chose, B = 1000 permutations per sample.
  (a) the kernels alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_exposure_trajectory and N
      of mmm_deal_counts on the pooled table for the middle cut, the selection and dealing without the fits) in a run of its own and hand
      the summary to the main run with --kernel-stats FILE;
  (b) exposure_trajectory end to end (host clock around the call, which ends in a device synchronise);
  (c) the same analysis composed from the entries that existed before: one stacked plain refit for the segment table, and per cut
      `mmm_deal_counts` on the pooled table with n_a = C_t plus two stacked plain refits of the B x D prefixes and suffixes through the raw
      binding, --chunk replicates at a time; the dynamic program and the maximum over the cuts in numpy -- same session, alternating with (b);
  (d) the numpy restatement (tests/trajectory_ref.py) on --host-docs samples and --host-B replicates, scaled by EM iterations.
Usage: python tools/bench_trajectory.py [--B 1000] [--rounds 2] [--kernel-stats FILE] [--out profiles/trajectory_brca.json]
       python tools/bench_trajectory.py --kernel-only 1
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
import trajectory_ref as TR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--C", type=int, default=86)
ap.add_argument("--T", type=int, default=16)
ap.add_argument("--B", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--chunk", type=int, default=250)
ap.add_argument("--min-len", type=int, default=1)
ap.add_argument("--max-changepoints", type=int, default=4)
ap.add_argument("--plant-every", type=int, default=8)
ap.add_argument("--plant-share", type=float, default=0.3)
ap.add_argument("--plant-signature", type=int, default=2)
ap.add_argument("--host-docs", type=int, default=2)
ap.add_argument("--host-B", type=int, default=2)
ap.add_argument("--maxiter", type=int, default=1000)
ap.add_argument("--tol", type=float, default=1e-9)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--kernel-only", type=int, default=0)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--kernel-calls", type=int, default=1, help="the N of the --kernel-only run that --kernel-stats summarises")
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()

_, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
ctx = mmm.default_context()
D, V, C, B, T, L, M = len(X), 96, args.C, args.B, args.T, args.min_len, args.max_changepoints
rng = np.random.default_rng(args.seed)
g = mmm.LDA(10, 0.1, 0.1, V, X, λ0=rng.integers(1, 101, size=(V, 10)).astype(np.float64))
mmm.fit(g, maxiter=200, tol=1e-4, verbose=False)
cat = np.concatenate([np.ascontiguousarray(g.β.T), rng.dirichlet(np.full(V, 0.3), size=C - 10)])
g.close()

parts = mmm.split_counts(X, T, args.seed, ctx=ctx)
dense = np.zeros((D, T, V), dtype=np.int64)
for t, part in enumerate(parts):
    for d, x in enumerate(part):
        np.add.at(dense[d, t], x[:, 0] - 1, x[:, 1])
planted = np.arange(D) % args.plant_every == 0
sig = cat[args.plant_signature] / cat[args.plant_signature].sum()
for d in np.flatnonzero(planted):
    for t in range(T - 4, T):
        dense[d, t] += rng.multinomial(int(round(args.plant_share * dense[d, t].sum())), sig)
pooled = dense.sum(axis=1)
N = pooled.sum(axis=1)
C_t = np.concatenate([np.zeros((D, 1), np.int64), np.cumsum(dense.sum(axis=2), axis=1)], axis=1)          # [D, T + 1]
as_X = lambda n: [np.stack([np.flatnonzero(r) + 1, r[np.flatnonzero(r)]], axis=1) for r in n]
Xp = as_X(pooled)
chosen = mmm.refit_exposures(Xp, cat, maxiter=args.maxiter, tol=args.tol)
allowed = np.ascontiguousarray(chosen.active.T, dtype=np.uint8)
pen = 0.5 * (allowed.sum(axis=1) + 1.0) * np.log(np.maximum(N, 1).astype(np.float64))
p_dp, p_term, p_count = mmm.pack_lda(Xp)                        # term order, no duplicates: the numbering of the dealing
cuts = list(range(L, T - L + 1))


def fused(keep=False):
    return mmm.exposure_trajectory(dense, cat, allowed=chosen, min_len=L, max_changepoints=M, penalty=pen, B=B, seed=args.seed, maxiter=args.maxiter, tol=args.tol,
                                   keep_replicates=keep, changepoint_tests=False, ctx=ctx)


if args.kernel_only:
    for _ in range(args.kernel_only):
        fused()
        mmm.compare._deal_raw(ctx, D, p_dp, p_count, C_t[:, T // 2], B, 0, args.seed, 0)
    sys.exit(0)


def plain_dense(rows, al):
    n = rows.shape[0]
    return mmm.refit._raw(ctx, n, V, np.arange(n + 1, dtype=np.int64) * V, np.tile(np.arange(V, dtype=np.int32), n), rows.ravel(), cat, al, None, args.maxiter, args.tol)


def composed():
    """-> (count_ge [D], n_cp [D]) from the entries the parent commit has"""
    segs = [(i, j) for i in range(T) for j in range(i + 1, T + 1) if j - i >= L]
    cpre = np.concatenate([np.zeros((D, 1, V), np.int64), np.cumsum(dense, axis=1)], axis=1)
    rows = np.concatenate([cpre[:, j] - cpre[:, i] for i, j in segs])
    ll = plain_dense(rows, np.tile(allowed, (len(segs), 1)))["ll_doc"].reshape(len(segs), D)
    tab = np.full((D, T * (T + 1) // 2), np.nan)
    for s, (i, j) in enumerate(segs):
        tab[:, TR.seg_index(T, i, j)] = ll[s]
    n_cp = np.array([TR.partition(tab[d], T, L, M, pen[d])[1] for d in range(D)])
    G = np.stack([tab[:, TR.seg_index(T, 0, t)] + tab[:, TR.seg_index(T, t, T)] for t in cuts])
    g_max = G.max(axis=0)
    ge = np.zeros(D, dtype=np.int64)
    nnz = np.diff(p_dp)
    for off in range(0, B, args.chunk):
        nb = min(args.chunk, B - off)
        dp = np.concatenate([[0], np.cumsum(np.tile(nnz, nb))]).astype(np.int64)
        term = np.tile(p_term, nb)
        al = np.tile(allowed, (nb, 1))
        gm = np.full((nb, D), -np.inf)
        for t in cuts:
            dealt = mmm.compare._deal_raw(ctx, D, p_dp, p_count, C_t[:, t], nb, off, args.seed, 0)          # [nb, nnz]
            fa = mmm.refit._raw(ctx, nb * D, V, dp, term, dealt.ravel(), cat, al, None, args.maxiter, args.tol, outputs="all")
            fz = mmm.refit._raw(ctx, nb * D, V, dp, term, (p_count[None, :] - dealt).ravel(), cat, al, None, args.maxiter, args.tol, outputs="all")
            gm = np.maximum(gm, (fa["ll_doc"] + fz["ll_doc"]).reshape(nb, D))
        ge += (gm >= g_max[None, :]).sum(axis=0)
    return ge, n_cp


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, r


clock(lambda: mmm.exposure_trajectory(dense, cat, allowed=chosen, min_len=L, max_changepoints=M, penalty=pen, B=4, seed=args.seed, maxiter=args.maxiter, tol=args.tol,
                                      changepoint_tests=False, ctx=ctx))
t_b, t_c = [], []
for _ in range(args.rounds):
    t, res = clock(fused)
    t_b.append(t)
    t, (ge_c, ncp_c) = clock(composed)
    t_c.append(t)
tested = res.status == 0

# (d) the host restatement on a few samples
nh = min(args.host_docs, D)
bins = tuple(tuple((np.flatnonzero(dense[d, t]).astype(np.int32), dense[d, t][np.flatnonzero(dense[d, t])].astype(np.int32)) for t in range(T)) for d in range(nh))
sub = TR.TCase("host", C, V, bins, cat, allowed[:nh], L, M, pen[:nh], args.maxiter, args.tol, args.host_B, args.seed, 0)
t0 = time.perf_counter()
ref = TR.trajectory(sub)
t_d = time.perf_counter() - t0
dev = mmm.exposure_trajectory(dense[:nh], cat, allowed=allowed[:nh], min_len=L, max_changepoints=M, penalty=pen[:nh], B=args.host_B, seed=args.seed, maxiter=args.maxiter,
                              tol=args.tol, changepoint_tests=False, ctx=ctx)
same = bool(np.array_equal(ref.iters, dev.iters) and np.array_equal(ref.count_ge, dev.count_ge) and np.array_equal(ref.n_cp, dev.n_changepoints)
            and np.array_equal(ref.cp, dev.changepoints) and all(np.array_equal(ref.w_seg[d, :ref.n_cp[d] + 1], dev.exposures_segment[d]) for d in range(nh)))
share = float(ref.iters.sum()) / float(res.iters.sum())

last4 = np.array([c >= T - 4 for c in res.cut])
out = {"device": ctx.device_name(), "D": D, "V": V, "C": C, "T": T, "B": B, "min_len": L, "max_changepoints": M, "maxiter": args.maxiter, "tol": args.tol,
       "rounds": args.rounds, "allowed_per_sample_mean": float(allowed.sum(axis=1).mean()), "N_mean": float(N.mean()), "N_max": int(N.max()),
       "planted_samples": int(planted.sum()), "plant_share": args.plant_share, "status_counts": {str(k): int((res.status == k).sum()) for k in (0, 1, 3)},
       "segments_in_table": int(tested.sum()) * T * (T + 1) // 2, "replicate_fits": int(tested.sum()) * B * len(cuts) * 2, "em_iterations_total": int(res.iters.sum()),
       "planted_found_at_0.01": int((res.p[planted & tested] <= 0.01).sum()), "unplanted_at_0.01": int((res.p[~planted & tested] <= 0.01).sum()),
       "unplanted_tested": int((~planted & tested).sum()), "expected_unplanted_at_0.01": 0.01 * float((~planted & tested).sum()),
       "planted_with_a_changepoint": int((res.n_changepoints[planted] >= 1).sum()), "unplanted_with_a_changepoint": int((res.n_changepoints[~planted] >= 1).sum()),
       "planted_cut_in_last_four_bins": int(last4[planted].sum()),
       "b_exposure_trajectory_s": statistics.median(t_b), "b_all_s": t_b, "c_composed_s": statistics.median(t_c), "c_all_s": t_c,
       "count_ge_fused_equals_composed": bool(np.array_equal(res.count_ge, ge_c)), "n_cp_fused_equals_composed": bool(np.array_equal(res.n_changepoints, ncp_c)),
       "d_numpy_docs": nh, "d_numpy_B": args.host_B, "d_numpy_s": t_d, "d_numpy_scaled_s": t_d / share, "d_subset_share_of_iterations": share,
       "numpy_equals_device_on_subset": same}
out["c_over_b"] = out["c_composed_s"] / out["b_exposure_trajectory_s"]
out["d_over_b"] = out["d_numpy_scaled_s"] / out["b_exposure_trajectory_s"]
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh) if "k_traj" in r["Name"] or "k_deal" in r["Name"]]
    for key, name in (("fit", "k_traj_fit"), ("rep", "k_traj_rep"), ("prefix", "k_traj_scatter"), ("cumulate", "k_traj_cumulate"), ("deal", "k_deal_counts")):
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        if calls:
            out["a_%s_launches" % key] = calls
            out["a_%s_ms_per_call" % key] = sum(float(r["TotalDurationNs"]) for r in sel) / 1e6 / args.kernel_calls       # all launches of one call of the entry
    if "a_rep_ms_per_call" in out and "a_deal_ms_per_call" in out:
        # one k_deal_counts call deals ONE cut; the replicate launch selects and deals every cut
        out["a_select_share_upper_bound"] = len(cuts) * out["a_deal_ms_per_call"] / out["a_rep_ms_per_call"]
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
