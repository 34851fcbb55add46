#!/usr/bin/env python3
"""Bootstrap of the exposures on the BRCA-EU SNV table (tests/golden/brca-eu_snv_counts.tsv: 560 samples, 96 terms) under an LDA with K = 10
fitted to convergence, B = 1000 replicates:
  (a) mmm_resample_counts alone: wall time of the call (for its kernel time run this tool with --resample-only under a kernel trace);
  (b) bootstrap_exposures end to end, and its split into resample / stacked-handle creation / frozen-topic passes / exposures back / summary
      (the same steps re-enacted one by one from the module's own functions);
  (c) what a user has without it: numpy Generator.multinomial per sample + one transform per replicate -- timed on --baseline-reps
      replicates and scaled to B (the calls are independent and identical in cost).
Usage: python tools/bootstrap_bench.py [--B 1000] [--K 10] [--rounds 3] [--baseline-reps 50] [--resample-only]
(b) and (c) alternate, after a warm-up of each; every timed span is a host clock around work that ends in a device synchronise.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import mmm_pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1000)
ap.add_argument("--K", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--baseline-reps", type=int, default=50)
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--resample-only", action="store_true")
args = ap.parse_args()
mmm = mmm_pkg.load()
from multimodalmusig_jl_amd import bootstrap as bs  # noqa: E402
from multimodalmusig_jl_amd.inference import _lda_infer  # noqa: E402

warnings.simplefilter("ignore")
_, samples, snv = mmm.read_counts_tsv(os.path.join(ROOT, "tests", "golden", "brca-eu_snv_counts.tsv"))
X = mmm.format_counts_lda({s: snv[:, i] for i, s in enumerate(samples)}, samples)
D, V, K, B = len(X), snv.shape[0], args.K, args.B
ctx = mmm.default_context()
doc_ptr, term, count = mmm.pack_lda(X)


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, out


if args.resample_only:
    bs._resample_csr(ctx, D, doc_ptr, count, 8, 0, args.seed, 0)
    ts = [clock(lambda: bs._resample_csr(ctx, D, doc_ptr, count, B, 0, args.seed, 0))[0] for _ in range(args.rounds)]
    print(json.dumps({"resample_only": True, "B": B, "D": D, "nnz": int(doc_ptr[-1]), "draws": int(B * count.sum()), "call_wall_s": ts}))
    sys.exit(0)

model = mmm.LDA(K, 0.1, 0.1, V, X, seed=1)
t_fit, hist = clock(lambda: mmm.fit(model, maxiter=1000, tol=1e-4, verbose=False))


def end_to_end():
    return mmm.bootstrap_exposures(model, X, B, args.seed)


def split():
    """the steps of bootstrap_exposures, one clock each"""
    t = {}
    t["resample_call"], r = clock(lambda: bs._resample_csr(ctx, D, doc_ptr, count, B, 0, args.seed, 0))
    t["resample_and_stack"], Xs = clock(lambda: bs._stack_lda(ctx, D, doc_ptr, term, count, B, 0, args.seed))
    t["handle_creation"], new = clock(lambda: mmm.LDA(model.K, model.α, model.η, model.V, Xs, ctx=ctx))
    new.β = model.β
    t["passes"], h = clock(lambda: _lda_infer(new, True, 1000, 1e-4, False))
    t["exposures_to_host"], th = clock(lambda: new._get("theta"))
    new.close()
    reps = th.reshape(B, D, K).transpose(0, 2, 1).copy()
    t["summary"], _ = clock(lambda: bs.replicate_summary(reps, (0.025, 0.5, 0.975), ctx=ctx))
    t["n_passes"] = len(h)
    return t


def baseline(n):
    """numpy multinomial per sample + one transform per replicate, n replicates"""
    rng = np.random.default_rng(args.seed)
    p = snv / snv.sum(axis=0, keepdims=True)
    N = snv.sum(axis=0)
    out = []
    for _ in range(n):
        Xb = [mmm.make_count_matrix(rng.multinomial(N[d], p[:, d])) for d in range(D)]
        out.append(mmm.transform(model, Xb))
    return out


end_to_end(); baseline(2); split()                      # warm-up
tb, tc, sp = [], [], []
for _ in range(args.rounds):
    tb.append(clock(end_to_end)[0])
    tc.append(clock(lambda: baseline(args.baseline_reps))[0] * B / args.baseline_reps)
    sp.append(split())
res = end_to_end()
med = lambda v: float(np.median(v))  # noqa: E731
print(json.dumps({"B": B, "D": D, "V": V, "K": K, "nnz": int(doc_ptr[-1]), "draws": int(B * count.sum()), "fit_passes": len(hist), "fit_wall_s": t_fit,
                  "bootstrap_wall_s": tb, "baseline_wall_s_scaled_from_%d" % args.baseline_reps: tc, "ratio_b_over_c": med(tb) / med(tc),
                  "split_s": {k: med([s[k] for s in sp]) for k in sp[0]}, "n_iter": res.n_iter, "converged": res.converged,
                  "mean_sd": float(res.sd.mean()), "device": ctx.device_name()}))
