#!/usr/bin/env python3
"""Signature matching across a restart sweep on the BRCA-EU tables (tests/golden/brca-eu_{snv,sv}_counts.tsv), R = 256 restarts:
  (a) match_restarts and restart_consensus on the batch handle (the tables stay on the device);
  (b) the route without them: select(r) + download per restart, then the restatement of the definitions on the host (tests/match_ref.py:
      numpy cosine, pure-Python shortest augmenting paths; scipy's solver too where it is installed), and for the consensus the aligned
      probabilities summarised with numpy;
  (c) the array form, match_signatures of R x 7 x 96 tables against a synthetic catalogue of C = 86 rows.
For the LDA batch (K = 7 over the SNV table) and the MMCTM [7, 7] batch (SNV + SV, modality 0).
Usage: python tools/bench_match.py [--R 256] [--rounds 5] [--kernels-only] [--out profiles/signature_match_brca.json]
Every timed span is a host clock around calls that end in a device synchronise, after one warm-up of each; medians over --rounds.  A device
call of (a) / (c) takes a fraction of a millisecond, so a sample of those is --inner calls back to back, divided by --inner.
--kernels-only runs (a) and (c) once each after the warm-up (for a kernel trace).  Prints one JSON line."""
import argparse
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
import match_ref as mr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--R", type=int, default=256)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--ctm-maxiter", type=int, default=30)
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
mmm = mmm_pkg.load()
try:
    from scipy.optimize import linear_sum_assignment
except ImportError:
    linear_sum_assignment = None

gold = os.path.join(ROOT, "tests", "golden")
_, samples, snv = mmm.read_counts_tsv(os.path.join(gold, "brca-eu_snv_counts.tsv"))
_, _, sv = mmm.read_counts_tsv(os.path.join(gold, "brca-eu_sv_counts.tsv"))
snv_d = {s: snv[:, i] for i, s in enumerate(samples)}; sv_d = {s: sv[:, i] for i, s in enumerate(samples)}
ctx = mmm.default_context()
R, Q = args.R, (0.025, 0.5, 0.975)


def clock(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, out


def median(fn, inner=1):
    fn()
    ts = [clock(lambda: [fn() for _ in range(inner)])[0] / inner for _ in range(args.rounds)]
    return {"median_s": statistics.median(ts), "all_s": ts, "calls_per_sample": inner}


def download(model, field):
    keep = model.selected
    out = []
    for r in range(model.R):
        model.select(r)
        out.append(field(model))
    model.select(keep)
    return np.stack(out)


def host_match(model, field, ref, solver):
    tabs = download(model, field)
    S = mr.cosine(tabs, tabs[ref])
    if solver == "scipy":
        return tabs, np.stack([linear_sum_assignment(S[r], maximize=True)[1] for r in range(len(S))])
    return tabs, np.stack([mr.lsap(S[r]) for r in range(len(S))])


def host_consensus(model, field, ref, solver):
    tabs, assign = host_match(model, field, ref, solver)
    P = mr.align_normalise(tabs, assign)
    return P.mean(axis=0), P.std(axis=0, ddof=1), np.quantile(P, Q, axis=0)


def bench(name, model, modality, field):
    ref = int(np.argmax(model.restart_ll if modality is None else model.restart_ll[:, modality]))
    model.select(ref)
    out = {"R": model.R, "ref": ref}
    if args.kernels_only:
        mmm.match_restarts(model, modality=modality); mmm.restart_consensus(model, modality=modality, q=Q)
        return out
    out["a_match_restarts"] = median(lambda: mmm.match_restarts(model, modality=modality), args.inner)
    out["a_restart_consensus"] = median(lambda: mmm.restart_consensus(model, modality=modality, ref=ref, q=Q), args.inner)
    out["b_download_only"] = median(lambda: download(model, field))
    out["b_host_match_restatement"] = median(lambda: host_match(model, field, ref, "restatement"))
    out["b_host_consensus_restatement"] = median(lambda: host_consensus(model, field, ref, "restatement"))
    if linear_sum_assignment is not None:
        out["b_host_match_scipy"] = median(lambda: host_match(model, field, ref, "scipy"))
        out["b_host_consensus_scipy"] = median(lambda: host_consensus(model, field, ref, "scipy"))
    best_b = min(v["median_s"] for k, v in out.items() if k.startswith("b_host_match"))
    best_bc = min(v["median_s"] for k, v in out.items() if k.startswith("b_host_consensus"))
    out["a_over_b_match"] = out["a_match_restarts"]["median_s"] / best_b
    out["a_over_b_consensus"] = out["a_restart_consensus"]["median_s"] / best_bc
    got = mmm.match_restarts(model, modality=modality)
    _, host = host_match(model, field, ref, "restatement")
    out["restarts_equal_to_host_route"] = int((got.assign == host).all(axis=1).sum())
    out["stability"] = [float(x) for x in mmm.restart_consensus(model, modality=modality, ref=ref, q=Q).stability]
    return out


res = {"device": ctx.device_name(), "rounds": args.rounds, "inner": args.inner, "scipy": linear_sum_assignment is not None}
lda = mmm.LDA(7, 0.1, 0.1, mmm.format_counts_lda(snv_d, samples), restarts=R, seed=1)
t, _ = clock(lambda: mmm.fit_restarts(lda))
res["lda_k7"] = dict(bench("lda", lda, None, lambda m: np.ascontiguousarray(m.λ.T)), fit_restarts_s=t)
lda.close()
mm = mmm.MMCTM([7, 7], [0.1, 0.1], [96, 48], mmm.format_counts_mmctm([snv_d, sv_d], samples), restarts=R, seed=2)
t, _ = clock(lambda: mmm.fit_restarts(mm, maxiter=args.ctm_maxiter, tol=1e-4))
res["mmctm_77_modality0"] = dict(bench("mmctm", mm, 0, lambda m: m._get("gamma")[:7 * 96].reshape(7, 96)), fit_restarts_s=t, maxiter=args.ctm_maxiter)
mm.close()
rng = np.random.default_rng(3)
sig = rng.dirichlet(np.full(96, 0.2), size=(R, 7)) * rng.uniform(1, 1e4, size=(R, 7, 1))
cat = rng.dirichlet(np.full(96, 0.2), size=86)
if args.kernels_only:
    mmm.match_signatures(sig, cat); mmm.match_signatures(sig, cat)
else:
    res["c_array_form_C86"] = dict(median(lambda: mmm.match_signatures(sig, cat), args.inner), R=R, K=7, C=86, V=96)
    res["c_host_restatement_C86"] = median(lambda: mr.match(sig, cat))
line = json.dumps(res)
print(line)
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as fh:
        fh.write(line + "\n")
