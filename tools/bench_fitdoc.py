#!/usr/bin/env python3
"""Per-document stage calls: median wall time per call (1 GPU).
  one_doc_ms: one document through update_ζ!, update_θ!, update_ν!, update_λ!(model, d) -- the four calls the reference's fitdoc!(model, d)
              makes (MMCTM.jl:450-455); these exist at earlier commits too, so `--root OTHER_TREE` times the same thing there (A/B).
  list_ms[n]: fitdoc!(model, S) for lists S of n = 1, 64, 4096 documents (capped at D; where the build has mmm_ctm_update_docs).
Shapes: config 3 (shipped BRCA tables, MMCTM [7, 7], 560 documents), config 4 (MMCTM [10, 10, 8], 50k), config 5 (IMMCTM K = 10, 100k).
--ab OTHER_TREE: both trees, each in a child process, one after the other; the output holds both and the one-document speed-up
(profiles/fitdoc_calls.json is `--ab <parent commit's tree> --out profiles/fitdoc_calls.json`).
Usage: python tools/bench_fitdoc.py [--configs 3,4,5] [--calls 30] [--root TREE | --ab OTHER_TREE] [--out FILE]"""
import argparse, json, os, subprocess, sys, tempfile, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,4,5")
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--root", default=HERE, help="tree whose package is timed (default: this one)")
ap.add_argument("--ab", default="", help="also time OTHER_TREE (child processes) and write both")
ap.add_argument("--ab-label", default="", help="what OTHER_TREE is, for the output (default: its path)")
ap.add_argument("--out", default="")
args = ap.parse_args()
if args.ab:
    runs = {}
    for key, root in (("this_tree", HERE), ("other", os.path.abspath(args.ab))):
        with tempfile.NamedTemporaryFile(suffix=".json", delete=False) as fh:
            tmp = fh.name
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--configs", args.configs, "--calls", str(args.calls), "--root", root,
                               "--out", tmp])
        with open(tmp) as fh:
            runs[key] = json.load(fh)
        os.unlink(tmp)
    a, b = runs["this_tree"], runs["other"]
    res = {"tool": "tools/bench_fitdoc.py --ab", "unit": "ms per call, median wall time", "calls": args.calls, "device": a["device"],
           "other_tree": args.ab_label or os.path.relpath(os.path.abspath(args.ab), HERE), "this_tree": a["configs"], "other": b["configs"],
           "one_doc_speedup": {c: round(b["configs"][c]["one_doc_ms"] / a["configs"][c]["one_doc_ms"], 2) for c in a["configs"]}}
    print(json.dumps(res["one_doc_speedup"]))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    sys.exit(0)
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(HERE, "tests"))
import numpy as np
import mmm_pkg, np_ref

pkg = mmm_pkg.load()
has_list = hasattr(pkg.lib(), "mmm_ctm_update_docs")
SNV3 = [np.array([[t // 16 + 1, (t // 4) % 4 + 1, t % 4 + 1] for t in range(96)])]


def model(cfg):
    if cfg == 3:
        gold = os.path.join(HERE, "tests", "golden")
        _, samples, snv = pkg.read_counts_tsv(os.path.join(gold, "brca-eu_snv_counts.tsv"))
        _, _, sv = pkg.read_counts_tsv(os.path.join(gold, "brca-eu_sv_counts.tsv"))
        X = pkg.format_counts_mmctm([{s: snv[:, i] for i, s in enumerate(samples)}, {s: sv[:, i] for i, s in enumerate(samples)}], samples)
        rng = np.random.default_rng(2)
        return pkg.MMCTM([7, 7], [0.1, 0.1], [96, 48], X, γ0=[rng.integers(1, 101, size=(7, 96)).astype(np.float64),
                                                              rng.integers(1, 101, size=(7, 48)).astype(np.float64)])
    if cfg == 4:
        X, g0 = np_ref.synth_mm(50000, [96, 38, 32], [10, 10, 8], seed=20261003 + 4)
        return pkg.MMCTM([10, 10, 8], [0.1] * 3, [96, 38, 32], X, γ0=g0)
    X, _ = np_ref.synth_mm(100000, [96], [10], seed=20261003 + 5)
    gflat = np.random.default_rng(1).integers(1, 101, size=10 * int(SNV3[0].max(axis=0).sum())).astype(np.float64)
    return pkg.IMMCTM([10], [0.1], SNV3, X, γ0=gflat)


def median_ms(fn, n):
    for _ in range(3):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


res = {"root": "this tree" if ROOT == HERE else ROOT, "calls": args.calls, "device": pkg.default_context().device_name(), "configs": {}}
for cfg in [int(c) for c in args.configs.split(",")]:
    m = model(cfg)
    pkg.fit(m, maxiter=2, tol=0.0, verbose=False)
    D = m.D
    d = D // 2

    def four():
        pkg.update_ζ(m, d); pkg.update_θ(m, d); pkg.update_ν(m, d); pkg.update_λ(m, d)
    r = {"D": D, "one_doc_ms": median_ms(four, args.calls)}
    if has_list:
        rng = np.random.default_rng(cfg)
        r["list_ms"] = {}
        for n in (1, 64, 4096):
            S = [int(x) for x in rng.choice(D, min(n, D), replace=False)]
            r["list_ms"][str(len(S))] = median_ms(lambda: pkg.fitdoc(m, S), args.calls)
    res["configs"][str(cfg)] = r
    print(json.dumps({"config": cfg, **r}), flush=True)
    m.close()
if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
