"""What the creates decide and build, checked without a device: tests/corpus_forms_main.cpp compiles csrc/corpus_forms.h and
csrc/create_plan.h alone (g++ -std=c++17, with -fsanitize=address,undefined where the compiler's runtimes are installed) and prints the
forms of a corpus and the plan of a case.

Forms are held to the numpy restatement below, which imports nothing from the package: the slot rule, every element of the 16- and 32-bit
lane-major rows (the spare tail included), the facts, the (term, count) pairs, the padded rows, the postings by term and stats_waves.

Plans are held to the expectations the GPU tests carry, imported from them (not restated): lda_infer_ref.cases() (the _geo table),
test_ilda_dispatch_gpu (CASES x settings_of, dense_build_exists), ctm_dense_ref (cases(): builds, the seven refusals, the half-density
case, the thirteen GRID_EDGES; dense_build, conditions) and test_ctm_dispatch_gpu (GEO4 and the three threshold walks at geometry_cus = 4,
each from both sides).  The GPU tests remain the authority for what only a device tells, left out here:
  * ILDA's resident_cap settings (the bound comes from hipOccupancyMaxActiveBlocksPerMultiprocessor) and every mmm_lda_last_pass /
    mmm_lda_prologue_moved expectation (decided per pass, not at create);
  * "solve_waves" of test_sum_k_10_two_by_five_refill_and_document_order_under_a_batch is asserted here from the plan's grid_v x waves_s,
    its refill itself is the device's;
  * row_bytes is derived here from the plan (drows, rows16, SLs, padded_rows) by the rule of mmm_lda_row_bytes, which on the device reads
    the buffers that exist."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodalmusig.jl_amd", "csrc")
BUILDS = {"auto": 0, "sparse": 1, "dense": 2, "wide": 3}                       # MMM_BUILD_* (include/mmmusig.h)
OFF = {"lda_count_rows": 1 << 1, "lda_rows16": 1 << 2, "lda_ll_join": 1 << 3, "lda_merged": 1 << 4, "ctm_packed": 1 << 6, "ctm_cpl": 1 << 7,
       "ctm_ll_rows": 1 << 10, "lda_block_stats": 1 << 14}                     # MMM_OFF_* bits the cases use
NOT_PLAN_INPUTS = ("resident_cap",)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no C++ compiler")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("corpus_forms")
    out = str(d / "corpus_forms_main")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "corpus_forms_main.cpp"), "-o", out]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if p.returncode != 0:
        assert "sanitize" in p.stderr or "asan" in p.stderr or "ubsan" in p.stderr, p.stderr      # only a missing runtime excuses the plain build
        print("sanitizer runtimes not installed: building without")
        p = subprocess.run(base, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return out


class Cases:
    """Collects cases, runs the program once over all of them, returns one {key: [integers]} per case."""

    def __init__(self):
        self.text = []

    def _corpus(self, tune, ncu, R, ilda, D, K, V, dp, term, count):
        t = dict(tune)
        for k in NOT_PLAN_INPUTS:
            t.pop(k, None)
        dis = t.pop("disable", ())
        dis = [dis] if isinstance(dis, str) else dis
        head = [BUILDS[t.pop("lda_build", "auto")], BUILDS[t.pop("ctm_build", "auto")], t.pop("geometry_cus", 0), t.pop("grid_blocks", 0),
                t.pop("waves_per_block", 0), t.pop("moment_blocks", 0), sum(OFF[n] for n in dis), t.pop("solve_lanes", 0), t.pop("solve_waves", 0)]
        assert not t, "tuning keys this file does not pass on: %s" % t
        return head + [ncu, R, int(ilda), D, len(K)] + list(K) + list(V) + list(dp) + list(term) + list(count)

    def add(self, mode, *a):
        self.text.append(" ".join(str(int(x)) for x in ([mode] + (list(a) if mode == 4 else self._corpus(*a)))))
        return len(self.text) - 1

    def run(self, exe, tmp_path):
        f = tmp_path / "cases.txt"
        f.write_text("\n".join(self.text + ["0"]) + "\n")
        p = subprocess.run([exe, str(f)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        out = []
        for ln in p.stdout.splitlines():
            key, _, rest = ln.partition(" ")
            if key == "case":
                out.append({})
            elif key == "why":
                out[-1]["why"] = rest
            else:
                out[-1][key] = [int(x) for x in rest.split()]
        assert len(out) == len(self.text)
        return out


def csr(X, M):
    """X[d][m] (or X[d] for M = None): [W, 2] rows [term (1-based), count] -> modality-major doc_ptr [M (D + 1)], term (0-based), count."""
    D = len(X)
    dp, term, count = [], [], []
    for m in range(M or 1):
        dp.append(len(term))
        for d in range(D):
            x = np.asarray(X[d] if M is None else X[d][m], dtype=np.int64).reshape(-1, 2)
            term += (x[:, 0] - 1).tolist(); count += x[:, 1].tolist()
            dp.append(len(term))
    return dp, term, count


def one(v):
    assert len(v) == 1
    return v[0]


# ================================================================================================================ forms
def slots_of(V):
    return 2 if V <= 32 else 3 if V <= 48 else 6 if V <= 96 else 8 if V <= 128 else 0


def rows_of(D, dp, term, count, slots, spare, top):
    r = np.zeros(D * 16 * slots + spare, dtype=np.int64)
    for d in range(D):
        for e in range(dp[d], dp[d + 1]):
            r[d * 16 * slots + (term[e] % 16) * slots + term[e] // 16] = count[e] % top      # lane term % 16, the lane's slot term // 16
    return r.tolist()


def waves_of(nnz, nterms):
    avg, w = nnz // max(1, nterms), 1
    while w < 8 and avg // (2 * w) >= 128:
        w *= 2
    return w


def edge_corpus(V, D, dup, seed):
    """D documents over V terms: document 0 lists a term with count 0 and one with 65,535; 1 is empty; 2 lists its first term twice (dup);
    3 holds a count of 65,536; 4 lists every term but the last, which no document has (V > 1).  Terms in drawn order."""
    rng = np.random.Generator(np.random.PCG64([V, D, seed]))
    last = V - 1 if V > 1 else V
    docs = []
    for d in range(D):
        n = 0 if d == 1 else (last if d == 4 else int(rng.integers(1, last + 1)))
        t = rng.permutation(last)[:n].tolist()
        c = (1 + rng.poisson(20, size=n)).tolist()
        if d == 0 and n:
            c[0] = 0; c[-1] = 65535
        if d == 2 and dup:
            t.append(t[0]); c.append(7)
        if d == 3:
            c[0] = 65536
        docs.append((t, c))
    dp, term, count = [0], [], []
    for t, c in docs:
        term += t; count += c; dp.append(len(term))
    return dp, term, count


def check_forms(o, D, Vs, dp, term, count, tag):
    V = Vs[0]
    seg = slice(dp[0], dp[D])
    sl = slots_of(V)
    assert one(o["slots"]) == sl, tag
    longest = max([dp[d + 1] - dp[d] for d in range(D)] + [0])
    rep = any(len(set(term[dp[d]:dp[d + 1]])) != dp[d + 1] - dp[d] for d in range(D))
    assert o["facts"] == [max(count[seg] + [0]), longest, int(rep)], tag
    assert o["facts_lazy"] == [0], tag
    if sl:
        sls = sl + (sl & 1)
        assert o["rows16"] == rows_of(D, dp, term, count, sls, 8, 65536), tag       # an even number of slots per lane, 16 spare bytes
        assert len(o["rows16"]) == D * 16 * sls + 8 and o["rows16"][-8:] == [0] * 8
        assert o["rows32"] == rows_of(D, dp, term, count, sl, 0, 1 << 32), tag
    else:
        assert "rows16" not in o and "rows32" not in o
    nnz = len(term)
    assert o.get("tc", []) == [x for e in range(nnz) for x in (term[e], count[e])], tag
    if longest <= V:
        ell = np.tile(np.array([-1, 0]), (D, V, 1))
        for d in range(D):
            for j, e in enumerate(range(dp[d], dp[d + 1])):
                ell[d, j] = (term[e], count[e])
        assert o.get("ell", []) == ell.ravel().tolist(), tag
    else:
        assert "ell" not in o
    # postings: M segments, vocabularies stacked; documents ascending within a term
    M = len(Vs)
    voff = np.concatenate([[0], np.cumsum(Vs)])
    gterm = np.array([voff[m] + term[e] for m in range(M) for e in range(dp[m * (D + 1)], dp[m * (D + 1) + D])], dtype=np.int64)
    doc = np.array([d for m in range(M) for d in range(D) for _ in range(dp[m * (D + 1) + d], dp[m * (D + 1) + d + 1])], dtype=np.int64)
    order = np.argsort(gterm, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(gterm, minlength=int(voff[-1])))]).tolist()
    assert one(o["nterms"]) == int(voff[-1]) and o["term_ptr"] == tptr, tag
    post = o.get("post", [])
    assert post == [x for e in order for x in (int(doc[e]), count[e])], tag
    for t in range(int(voff[-1])):
        docs = post[2 * tptr[t]:2 * tptr[t + 1]:2]
        assert docs == sorted(docs), tag
    assert one(o["stats_waves"]) == waves_of(nnz, int(voff[-1])), tag


def test_corpus_forms_against_the_restatement(exe, tmp_path):
    cs, meta = Cases(), []
    for V in (1, 15, 16, 17, 32, 33, 48, 49, 96, 97, 128, 129):
        for D in (0, 1, 5):
            for dup in ((False, True) if D == 5 else (False,)):
                dp, term, count = edge_corpus(V, D, dup, 3)
                meta.append((cs.add(3, {}, 256, 1, 0, D, [1], [V], dp, term, count), D, [V], dp, term, count, "V=%d D=%d dup=%d" % (V, D, dup)))
    # two modalities whose offsets continue (the CTM's corpus): postings over the stacked vocabularies
    a, b = edge_corpus(17, 5, False, 5), edge_corpus(40, 5, False, 6)
    dp = a[0] + [x + a[0][-1] for x in b[0]]
    meta.append((cs.add(3, {}, 256, 1, 0, 5, [1, 1], [17, 40], dp, a[1] + b[1], a[2] + b[2]), 5, [17, 40], dp, a[1] + b[1], a[2] + b[2], "two modalities"))
    waves = [(cs.add(4, avg * 7 + 3, 7), avg) for avg in (127, 128, 255, 256, 511, 512, 1023, 1024, 5000)]
    out = cs.run(exe, tmp_path)
    edges = set()
    for i, D, Vs, dp, term, count, tag in meta:
        check_forms(out[i], D, Vs, dp, term, count, tag)
        if D == 5 and Vs[0] > 1:
            edges |= {"empty"} if dp[1] == dp[2] else set()
            edges |= {"zero"} if 0 in count else set()
            edges |= {"65535", "65536"} & {str(c) for c in count}
            edges |= {"absent"} if Vs[0] - 1 not in term[:dp[5]] else set()
            edges |= {"twice"} if out[i]["facts"][2] else set()
    assert edges == {"empty", "zero", "65535", "65536", "absent", "twice"}
    want = {127: 1, 128: 1, 255: 1, 256: 2, 511: 2, 512: 4, 1023: 4, 1024: 8, 5000: 8}
    for i, avg in waves:
        assert one(out[i]["stats_waves"]) == want[avg] == waves_of(avg * 7 + 3, 7), avg


# ================================================================================================================ LDA plans
def lda_row_bytes(p):
    """mmm_lda_row_bytes from the plan's fields"""
    if one(p["wide"]):
        return 0
    if one(p["drows"]):
        return (2 if one(p["rows16"]) else 4) * 16 * one(p["SLs"])
    return 8 * p["V"] if one(p["padded_rows"]) and not one(p["dense"]) else 0


def lda_geo(p):
    return dict(L=one(p["L"]), KP=one(p["KP"]), single_step=one(p["single_step"]), wide=one(p["wide"]), row_bytes=lda_row_bytes(p), waves_e=one(p["waves_e"]),
                grid_e=one(p["grid_e"]), dense=one(p["dense"]))


def test_lda_plans_give_the_geometry_of_the_inference_walk(exe, tmp_path):
    import lda_infer_ref
    cases = lda_infer_ref.cases()
    cs = Cases()
    idx = [cs.add(1, c["tuning"], 256, 1, 0, c["D"], [c["K"]], [c["V"]], *csr(c["Xn"], None)) for c in cases]
    out = cs.run(exe, tmp_path)
    for c, i in zip(cases, idx):
        p = dict(out[i], V=c["V"])
        assert one(p["refusal"]) == 0, (c["name"], p["why"])
        assert lda_geo(p) == c["geometry"], "%s: the plan gives %s, the device test demands %s" % (c["name"], lda_geo(p), c["geometry"])
    by = {c["name"]: dict(out[i]) for c, i in zip(cases, idx)}
    assert one(by["csr_dup_v24_k6"]["dup_terms"]) == 1 and one(by["csr_dup_v24_k6"]["block_stats"]) == 0
    assert one(by["s16_k10_v96_d70"]["block_stats"]) == 1 and one(by["s16_k10_v96_d70"]["keeps_aexp_next"]) == 1


def test_lda_plans_of_the_ilda_dispatch_space(exe, tmp_path):
    import test_ilda_dispatch_gpu as T
    cs, meta = Cases(), []
    for c in T.CASES:
        X = csr(c["X"], None)
        for env in T.settings_of(c):
            meta.append((c, env, cs.add(1, env, 256, 1, 1, c["D"], [c["K"]], [c["V"]], *X)))
        if c["name"] == "penta":
            penta_lda = cs.add(1, {}, 256, 1, 0, c["D"], [c["K"]], [c["V"]], *X)
    out = cs.run(exe, tmp_path)
    assert len(meta) == T.N_PAIRS
    for c, env, i in meta:
        p = dict(out[i], V=c["V"])
        name = c["name"]
        assert one(p["refusal"]) == 0 and one(p["keeps_aexp_next"]) == 0, (name, env, p["why"])
        if env.get("lda_build") == "wide":
            assert one(p["wide"]) == 1, (name, env)
        if env.get("lda_build") == "dense" and T.dense_build_exists(c):
            assert one(p["dense"]) == 1, (name, env)
        if env.get("grid_blocks") and not one(p["wide"]):
            assert one(p["grid_e"]) == env["grid_blocks"] and one(p["single_step"]) == 0, (name, env)
        if name == "v257" and not env:
            assert one(p["wide"]) == 0
        if name == "penta" and not env:
            assert one(p["wide"]) == 1 and lda_geo(p) == lda_geo(dict(out[penta_lda], V=c["V"]))


def test_lda_batch_refusals(exe, tmp_path):
    """The four reasons a batch of a wide shape is refused with (MMM_ERR_UNSUPPORTED = -4), and K beyond every build."""
    cs = Cases()
    dp, term, count = edge_corpus(96, 5, False, 1)
    i_wide = cs.add(1, {"lda_build": "wide"}, 256, 2, 0, 5, [5], [96], dp, term, count)
    i_k33 = cs.add(1, {"lda_build": "sparse"}, 256, 2, 0, 5, [33], [96], dp, term, count)
    i_k25 = cs.add(1, {}, 256, 2, 0, 5, [25], [96], dp, term, count)
    dpb, tb, cb = edge_corpus(300, 5, False, 1)      # three 24 x 300 tables: 172,800 bytes
    i_lds = cs.add(1, {"lda_build": "sparse"}, 256, 2, 0, 5, [24], [300], dpb, tb, cb)
    i_one = cs.add(1, {"lda_build": "wide"}, 256, 1, 0, 5, [5], [96], dp, term, count)
    i_257 = cs.add(1, {}, 256, 1, 0, 5, [257], [96], dp, term, count)
    out = cs.run(exe, tmp_path)
    for i, why in ((i_wide, "lda_build = MMM_BUILD_WIDE"), (i_k33, "K > 32 topics"), (i_k25, "K >= 25 topics"), (i_lds, "exceed LDS")):
        assert one(out[i]["refusal"]) == -4 and why in out[i]["why"] and "mmm_lda_create_batch" in out[i]["why"], out[i]
    assert one(out[i_one]["refusal"]) == 0 and one(out[i_one]["wide"]) == 1
    assert one(out[i_257]["refusal"]) == -4 and "max 256" in out[i_257]["why"]


# ================================================================================================================ CTM plans
def ctm_geo(p):
    return dict(L=one(p["L"]), grid_e=one(p["grid_e"]), waves_e=one(p["waves_e"]), grid_m=one(p["grid_m"]), wide=one(p["wide"]), tdense=one(p["tdense"]),
                Ls=one(p["Ls"]), cpl=one(p["cpl"]), solve_waves=one(p["grid_v"]) * one(p["waves_s"]) if one(p["persist"]) else 0)


def test_ctm_plans_of_the_rows_of_counts_walk(exe, tmp_path):
    import ctm_dense_ref as R
    cases = R.cases()
    cs = Cases()
    idx = [cs.add(2, dict(c["tune"], ctm_build="dense"), 256, 1, 0, c["D"], c["K"], c["V"], *csr(c["X"], len(c["K"]))) for c in cases]
    out = cs.run(exe, tmp_path)
    groups = {}
    for c, i in zip(cases, idx):
        p, name = out[i], c["name"]
        groups.setdefault(c["group"], []).append(name)
        assert one(p["refusal"]) == 0, (name, p["why"])
        assert one(p["tdense"]) == int(c["dense"]), name
        cond = R.conditions(c["K"], c["V"], c["X"])
        assert all(cond.values()) == c["dense"], (name, cond)
        if c["violates"]:
            assert [k for k, v in cond.items() if not v] == [c["violates"]], (name, cond)
        if c["dense"]:
            builds, _ = R.dense_build(c["K"], c["V"])
            assert p["tSL"] == [b[1] for b in builds] and one(p["waves_e"]) == 8, name
        if c["tune"].get("grid_blocks"):
            assert one(p["grid_e"]) == c["tune"]["grid_blocks"], name
    assert len(groups["refused"]) == 7 and groups["half"] == ["half"] and len(groups["grid"]) == len(R.GRID_EDGES) == 13
    for (D, gb, cus), name in zip(R.GRID_EDGES, groups["grid"]):
        p = out[idx[[c["name"] for c in cases].index(name)]]
        # the arithmetic stated at GRID_EDGES: grid_s = min(ceil(D / 4), 4 CUs - 1) blocks of the ll launch
        assert (one(p["grid_e"]), one(p["grid_s"])) == (gb, min(-(-D // 4), 4 * cus - 1)), name


def test_ctm_plans_of_the_threshold_walks(exe, tmp_path):
    """test_ctm_dispatch_gpu.py at geometry_cus = 4: GEO4 for the singles, what each test there asserts of batch and single handles, and
    the three thresholds (1,171.875, 140.625 and 625 documents) from both sides."""
    import test_ctm_dispatch_gpu as T
    cs = Cases()

    def add(case, R=1, D=None, **tune):
        c = T.walk_case(case, D=D)
        return cs.add(2, dict(tune, geometry_cus=T.CUS), 256, R, 0, c["D"], c["K"], c["V"], *csr(c["X"], len(c["K"])))

    single = {case: add(case) for case in T.GEO4}
    batch = {case: [add(case, R=n) for n in (2, T.R, 16)] for case in ("imm10", "mm55")}
    pinned = {(lanes, R): add("imm10", R=R, D=150, solve_lanes=lanes) for lanes in (2, 8, 16) for R in (1, T.R)}
    refill = [add("imm10", R=R, D=1500, solve_lanes=2) for R in (1, 2)]
    lanes28 = add("cfg4_lanes", R=T.R)
    waves28 = add("cfg4_waves", R=T.R)
    held = {(case, lanes, D): add(case, D=D, solve_lanes=lanes) for case, lanes in (("imm10", 8), ("imm10", 2), ("cfg4_lanes", 0), ("imm10", 0)) for D in (50, 1500)}
    sides = {D: add("imm10", D=D) for D in (1171, 1172)}
    sides28 = {(D, R): add("cfg4_lanes", R=R, D=D) for D, R in ((140, 1), (141, 1), (35, 4), (36, 4), (624, 1), (625, 1), (156, 4), (157, 4))}
    out = cs.run(exe, tmp_path)
    g = lambda i: ctm_geo(out[i])
    lay = lambda i: (g(i)["Ls"], g(i)["cpl"])
    for case, want in T.GEO4.items():
        assert T._bits(g(single[case])) == want, (case, g(single[case]))
    for case, idx in batch.items():                       # the layout follows D alone, for any R
        for i in idx:
            assert T._bits(g(i)) == T.GEO4[case]
    for lanes, expect in ((2, (2, 5)), (8, (8, 2)), (16, (10, 1))):
        assert lay(pinned[(lanes, 1)]) == lay(pinned[(lanes, T.R)]) == expect
    for i in refill:
        geo = g(i)
        assert lay(i) == (2, 5) and geo["solve_waves"] > 0 and 64 // geo["Ls"] < 1500 // geo["solve_waves"] and -(-1500 // geo["solve_waves"]) <= 64, geo
    assert lay(single["cfg4_lanes"]) == (32, 1) and lay(lanes28) == (16, 2)
    assert T._bits(g(lanes28), T.BIT_KEYS[:-2]) == T._bits(g(single["cfg4_lanes"]), T.BIT_KEYS[:-2])
    assert T._bits(g(waves28)) == T.GEO4["cfg4_waves"]
    assert g(single["cfg4_waves"])["solve_waves"] == 4 * min(13, T.CUS * 3) and g(waves28)["solve_waves"] == 4 * min(13, T.CUS * 4)
    for lanes in (8, 2):
        assert lay(held[("imm10", lanes, 50)]) == lay(held[("imm10", lanes, 1500)]) == {8: (8, 2), 2: (2, 5)}[lanes]
    assert lay(held[("cfg4_lanes", 0, 50)]) == (32, 1) and lay(held[("cfg4_lanes", 0, 1500)]) == (16, 2)
    assert lay(held[("imm10", 0, 50)]) == (8, 2) and lay(held[("imm10", 0, 1500)]) == (2, 5)
    # the thresholds themselves: D < 75,000 x 4 / 256 = 1,171.875; D R < 9,000 x 4 / 256 = 140.625; D R >= 40,000 x 4 / 256 = 625
    assert lay(sides[1171]) == (8, 2) and lay(sides[1172]) == (2, 5)
    assert lay(sides28[(140, 1)]) == lay(sides28[(35, 4)]) == (32, 1) and lay(sides28[(141, 1)]) == lay(sides28[(36, 4)]) == (16, 2)
    occ = lambda i: one(out[i]["lam_occ"])
    assert occ(sides28[(624, 1)]) == occ(sides28[(156, 4)]) == 3 and occ(sides28[(625, 1)]) == occ(sides28[(157, 4)]) == 4


def test_ctm_shape_refusals(exe, tmp_path):
    cs = Cases()
    dp, term, count = edge_corpus(24, 5, False, 1)
    bad = [cs.add(2, {}, 256, 1, 0, 5, K, [24], dp, term, count) for K in ([65], [0])]
    dp4 = dp + [dp[-1]] * 6 * 4
    big = cs.add(2, {}, 256, 1, 0, 5, [64] * 5, [24] * 5, dp4, term, count)
    ok = cs.add(2, {}, 256, 1, 0, 5, [64] * 4 , [24] * 4, dp4[:24], term, count)
    out = cs.run(exe, tmp_path)
    for i in bad:
        assert one(out[i]["refusal"]) == -4 and "must be in 1..64" in out[i]["why"]
    assert one(out[big]["refusal"]) == -4 and "<= 256" in out[big]["why"]
    assert one(out[ok]["refusal"]) == 0 and one(out[ok]["big"]) == 1 and one(out[ok]["wide"]) == 1 and (one(out[ok]["Ls"]), one(out[ok]["cpl"])) == (64, 4)
