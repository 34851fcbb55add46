#!/usr/bin/env python3
"""Detection power of the presence test on the BRCA-EU SNV table (560 samples x 96 terms) against the 86-row catalogue of
tools/bench_presence.py: `allowed` = the sets a BIC refit chose, 3 targets, B = 1000 replicates per level and pair, four fractions, the
observed totals plus two fixed totals (15 levels).
  (a) the kernels alone: run this script under `rocprofv3 --kernel-trace --stats` with --kernel-only N (N calls of mmm_presence_power and N
      of mmm_presence_test on the same items) in a run of its own and hand the summary to the main run with --kernel-stats FILE;
  (b) presence_power end to end (host clock around the call, which ends in a device synchronise);
  (c) the same levels composed from the entries that existed before: the observed null fits from signature_presence (B = 0), then per level
      simulate_counts of the T D pairs as one corpus (the level as the stream: the L T D-document layout of the definition would make every
      call return L times as many vectors, so the draws differ from (b)'s and the counts agree in distribution only), the replicates fed
      back per target as a dense corpus into mmm_presence_test with B = 0, the critical values and the counts with numpy.
      --composed-levels limits (c) to the first levels and scales by the level count (every level has the same number of replicates).
Reports the mean rejection share per level of (b) and (c) side by side.
Usage: python tools/bench_power.py [--B 1000] [--rounds 2] [--kernel-stats FILE] [--out profiles/power_brca.json]
       python tools/bench_power.py --kernel-only 2
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
ap.add_argument("--targets", type=int, nargs="+", default=[2, 6, 40])
ap.add_argument("--fractions", type=float, nargs="+", default=[0.02, 0.05, 0.1, 0.2])
ap.add_argument("--totals", type=int, nargs="+", default=[150, 9000])
ap.add_argument("--alpha", type=float, default=0.05)
ap.add_argument("--composed-levels", type=int, default=0, help="levels the composed path runs (0: all)")
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
T, G = targets.size, len(args.fractions)
n_level = np.concatenate([np.maximum(N, 1)[None, :], np.repeat(np.asarray(args.totals)[:, None], D, axis=1)]).astype(np.int32)
H = n_level.shape[0]
L, G1, TD = H * (G + 1), G + 1, T * D
m = int(np.floor(args.alpha * (B + 1))) - 1


def fused(B_=B):
    return mmm.presence_power(X, cat, targets, fractions=args.fractions, n_mutations=n_level, alpha=args.alpha, allowed=chosen, B=B_, seed=args.seed,
                              maxiter=args.maxiter, tol=args.tol, ctx=ctx)


def presence(B_=B):
    return mmm.signature_presence(X, cat, targets, allowed=chosen, B=B_, seed=args.seed, maxiter=args.maxiter, tol=args.tol, ctx=ctx)


if args.kernel_only:
    for _ in range(args.kernel_only):
        fused()
        presence()
    sys.exit(0)


def composed(levels):
    """-> (count_reject, count_zero) [levels, TD] of the first `levels` levels from the entries the parent commit has"""
    obs = presence(0)
    w0 = obs.exposures_null.transpose(0, 2, 1).reshape(TD, C)
    live = obs.status.ravel() != 3
    phis = [0.0] + list(args.fractions)
    lam = np.full((levels, B, TD), np.nan)
    dp = np.arange(B * D + 1, dtype=np.int64) * V
    tm = np.tile(np.arange(V, dtype=np.int32), B * D)
    al = np.tile(allowed, (B, 1))
    for lvl in range(levels):
        h, gi = divmod(lvl, G1)
        props = np.zeros((TD, C)); props[:, 0] = 1.0
        n_doc = np.zeros(TD, dtype=np.int64)
        w = w0.copy()
        if gi:
            w = (1.0 - phis[gi]) * w0
            w[np.arange(TD), np.repeat(targets, D)] = phis[gi] * np.cumsum(w0, axis=1)[:, -1]
        props[live] = w[live]
        n_doc[live] = np.tile(n_level[h], T)[live]
        sim = mmm.simulate_counts(props.T, P.T, n_doc, B=B, seed=args.seed, stream=lvl, ctx=ctx)
        for ti in range(T):
            cnt = np.ascontiguousarray(sim[:, ti * D:(ti + 1) * D, :].reshape(B * D, V), dtype=np.int32)
            fed = mmm.presence._raw(ctx, B * D, V, dp, tm, cnt.ravel(), cat, targets[ti:ti + 1], al, 0, 0, 0, 0, args.maxiter, args.tol)
            lam[lvl][:, ti * D:(ti + 1) * D] = fed["stat"].reshape(B, D)
        print("composed: level %d of %d" % (lvl + 1, levels), file=sys.stderr, flush=True)
    lam[:, :, ~live] = np.nan
    rej = np.zeros((levels, TD), dtype=np.int64)
    crit = {}
    for lvl in range(levels):
        h, gi = divmod(lvl, G1)
        if gi == 0:
            crit[h] = -np.sort(-lam[lvl], axis=0)[m] if 0 <= m < B else np.full(TD, np.inf)
        with np.errstate(invalid="ignore"):
            rej[lvl] = (lam[lvl] > crit[h][None, :]).sum(axis=0)
    return rej, (lam == 0).sum(axis=1)


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, r


clock(lambda: fused(8))
t_b, t_p = [], []
for _ in range(args.rounds):
    t, res = clock(fused)
    t_b.append(t)
    t, pres = clock(presence)
    t_p.append(t)
levels = args.composed_levels or L
t_c, (rej_c, zero_c) = clock(lambda: composed(levels))
live = res.status != 3
cr = np.concatenate([np.round(res.size * B)[:, None], res.count_reject], axis=1).reshape(L, TD)
share_b = (np.nan_to_num(cr[:levels])[:, live.ravel()].mean(axis=1) / B).round(4).tolist()
share_c = (rej_c[:, live.ravel()].mean(axis=1) / B).round(4).tolist()
reps_power, reps_presence = int(live.sum()) * L * B, int((pres.status == 0).sum()) * B
out = {"device": ctx.device_name(), "D": D, "V": V, "C": C, "targets": [int(t) for t in targets], "B": B, "alpha": args.alpha, "m": m, "fractions": args.fractions,
       "totals": ["observed"] + args.totals, "levels": L, "maxiter": args.maxiter, "tol": args.tol, "rounds": args.rounds, "items": TD,
       "status_counts": {str(k): int((res.status == k).sum()) for k in range(4)}, "replicates_power": reps_power, "replicates_presence_test": reps_presence,
       "em_iterations_power": int(res.iters.sum()), "em_iterations_presence_test": int(pres.iters.sum()),
       "mean_power": np.nanmean(res.power, axis=(2, 3)).round(4).tolist(), "mean_size": np.nanmean(res.size, axis=(1, 2)).round(4).tolist(),
       "b_presence_power_s": statistics.median(t_b), "b_all_s": t_b, "presence_test_s": statistics.median(t_p), "presence_test_all_s": t_p,
       "c_composed_levels": levels, "c_composed_s": t_c, "c_composed_scaled_s": t_c * L / levels, "reject_share_per_level_fused": share_b,
       "reject_share_per_level_composed": share_c}
out["c_over_b"] = out["c_composed_scaled_s"] / out["b_presence_power_s"]
out["b_us_per_replicate"] = out["b_presence_power_s"] / reps_power * 1e6
out["presence_test_us_per_replicate"] = out["presence_test_s"] / max(1, reps_presence) * 1e6
out["b_ns_per_em_iteration"] = out["b_presence_power_s"] / out["em_iterations_power"] * 1e9
out["presence_test_ns_per_em_iteration"] = out["presence_test_s"] / out["em_iterations_presence_test"] * 1e9
if args.kernel_stats:
    with open(args.kernel_stats) as fh:
        rows = list(csv.DictReader(fh))
    for key, name, reps in (("power_rep", "k_power_rep", reps_power), ("power_select", "k_power_select", 0), ("presence_rep", "k_presence_rep", reps_presence),
                            ("obs", "k_presence_obs", 0)):
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        if calls:
            out["a_%s_launches" % key] = calls
            out["a_%s_ms_total" % key] = sum(float(r["TotalDurationNs"]) for r in sel) / 1e6
    out["a_note"] = "kernel totals are over the --kernel-only N calls of that run; divide by N per call"
line = json.dumps(out)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
