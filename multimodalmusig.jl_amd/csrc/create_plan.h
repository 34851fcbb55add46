// create_plan.h -- everything mmm_lda_create* / mmm_ctm_create* DECIDE for a shape, as pure host functions (plain C++17, no HIP): which
// build runs each phase, every launch geometry, every LDS size, and the shapes they refuse.  The handles hold the plan they were created
// with (mmm_lda : LdaPlan, mmm_ctm : CtmPlan); mmm_*_geometry report from it; tests/corpus_forms_main.cpp prints it without a device.
//
// The block counts below fix the association of the cross-document sums, and so the bits of a fit: they follow from
// the shard's D and `ncu` (mmm_geo_cus: the device's CU count or mmm_tuning_opts.geometry_cus), never from D x R -- a replica of a batch
// takes what a single handle on the same corpus takes.  R enters only where the comment at the line says that no bit depends on it.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/mmmusig.h"
#include "corpus_forms.h"

constexpr int kPlanWave = 64;                        // lanes of a wave (MMM_WAVE)
constexpr bool plan_off(const mmm_tuning_opts& t, unsigned bit) { return (t.disable & bit) != 0; }

// what comes back beside a plan: create returns `refusal` with `why` as the message when the shape has no build
struct PlanVerdict {
    int refusal = MMM_OK;
    std::string why;
    bool refuse(int code, const char* fmt, ...)
    {
        char buf[512];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        refusal = code; why = buf;
        return true;
    }
};
template <class Plan>
struct Planned : PlanVerdict { Plan plan; };

// ===== LDA / ILDA ====================================================================================================================
constexpr int kWavesPerBlock = 4;                    // stage kernels
constexpr int kMaxWavesE = 12;                       // fused E-step kernel: up to 768 threads
constexpr int kMinWavesSingle = 4;      // single-step build: fewest waves per block the library picks by itself (shard sizes: profiles/r05_lda_small_shards.txt)
constexpr int kLdaTopicSlots = 4;       // topics per lane of the rolled-loop kernels (kLdaSlots, lda_stage.cuh)

inline int pick_kp(int K)
{
    const int opts[] = {2, 4, 6, 8, 10, 12, 16, 20, 24, 32};
    for (int o : opts) if (K <= o) return o;
    if (K <= 64 * kLdaTopicSlots) return (K + 1) & ~1;      // 33..256 topics: the rolled-loop kernels (k_lda_estep_big, k_lda_stats_big), wide path only
    return -1;
}

struct LdaPlan {
    int KP = 0, L = 16;         // topics as the kernels pad them; lanes per document
    int SL = 0, SLs = 0;        // SL: term slots per lane of a 16-lane group (count_row_slots); SLs: as stored (LdaDev::Vp / 16), 0 without rows of counts
    bool dense = false;         // the dense-row E-step build (k_lda_estep_dense)
    bool drows = false;         // rows of counts exist (dense-row E-step build, or rows for the single-step build and the ll blocks)
    bool rows16 = false;        // ... as 16-bit counts (every count < 65536)
    bool padded_rows = false;   // [D][V] (term, count) rows padded with (-1, 0) for the ll blocks
    bool dup_terms = false;     // some document lists a term twice (looked for only where lda_scans_repeats says a build depends on it)
    bool wide = false;          // K*V tables larger than LDS: k_lda_estep_wide + k_lda_stats_terms, tables through L2
    bool single_step = false;   // one step per wave: the grid covers every document
    bool block_stats = false;   // single-step passes without the E-step ll take k_lda_estep_block (statistics as a block product, no slabs)
    bool keeps_aexp_next = false;   // the merged launch's prologue blocks form the next pass's exp(Elntheta) (single-step build, not ILDA)
    int grid_e = 1, waves_e = 8, grid_s = 1;
    size_t lds_e = 0, lds_tab = 0;
    size_t lds_b = 0;           // k_lda_estep_block's dynamic LDS: table | r | a
    size_t lds_d = 0;           // k_lda_estep_dense's
};

// What of the plan needs no look at the corpus.  Rows of counts (drows): a dense corpus over <= 128 terms is also kept as rows of 16 SL
// int32 counts -- 4 bytes per term slot against 8 per nonzero -- which the single-step E-step build (96-term vocabularies) and the ll blocks
// read instead of the padded (term,count) rows: BASELINE config 2 21.2 -> 19.9 us per iteration on the same box.  MMM_OFF_LDA_COUNT_ROWS
// keeps the (term,count) rows (A/B).
struct LdaRowShape : PlanVerdict {      // (with the refusal of K beyond every build)
    int KP, L, SL, dmode;
    bool drows_env, rshape, shape, dense_enough, block_shape;
    // a document that lists a term twice rules out the rows of counts and k_lda_estep_block: the corpus is scanned for one only when
    // one of them could otherwise be taken
    bool scans_repeats() const { return (rshape && ((shape && dmode != 0) || (drows_env && dense_enough))) || block_shape; }
};

inline LdaRowShape lda_row_shape(const mmm_tuning_opts& tune, int D, int V, int K, int64_t nnz)
{
    LdaRowShape s;
    s.KP = pick_kp(K);
    if (s.KP < 0) s.refuse(MMM_ERR_UNSUPPORTED, "mmm_lda_create: K=%d not supported (max 256: an LDS column block of 512 K bytes per wave)", K);
    s.L = (K <= 15) ? 16 : (K <= 31 ? 32 : 64);
    s.SL = count_row_slots(V);
    const int build = tune.lda_build;
    s.dmode = build == MMM_BUILD_DENSE ? 1 : (build == MMM_BUILD_AUTO ? -1 : 0);
    s.drows_env = !plan_off(tune, MMM_OFF_LDA_COUNT_ROWS);
    s.rshape = s.SL > 0 && s.L == 16 && D > 0 && build != MMM_BUILD_WIDE;          // rows of counts make sense
    s.shape = s.rshape && s.KP >= 4 && s.KP * s.SL <= 64;                            // ... and the dense-row E-step build exists
    s.dense_enough = 2 * nnz >= (int64_t)D * V;
    s.block_shape = s.L == 16 && s.KP <= 12 && V <= 96;      // could be single-step: k_lda_estep_block needs every (document, term) listed once
    return s;
}

// rs: lda_row_shape of the same arguments; facts: of the handle's one CSR segment, `repeats` looked for where rs.scans_repeats()
inline Planned<LdaPlan> lda_plan(const mmm_tuning_opts& tune, int ncu, int R, int D, int V, int K, const LdaRowShape& rs, const CorpusFacts& facts, bool ilda)
{
    Planned<LdaPlan> out;
    static_cast<PlanVerdict&>(out) = rs;
    if (out.refusal) return out;
    LdaPlan& p = out.plan;
    const int KP = rs.KP, L = rs.L, SL = rs.SL;
    const int G = kPlanWave / L;
    // waves per block of the fused kernel: as many as fit 160 KiB of LDS next to the two tables, at most 8
    const size_t tabB = (size_t)KP * V * sizeof(double);
    // Small corpora (every document resident at once): 6-wave blocks, two per CU, one step per wave with the <= 168-VGPR
    // single-step build (3 waves per SIMD).  Larger corpora: 8-wave blocks, one per CU, grid-stride steps (2 waves per SIMD).
    // dense-row E-step (k_lda_estep_dense): a dense corpus (at least half of the D x V entries present, no term listed twice in a
    // document) of at least 192 documents per CU, topics and vocabulary within the register budget of a lane (SL KP <= 64
    // doubles).  lda_build = MMM_BUILD_DENSE takes it for any corpus that has the shape (tests), MMM_BUILD_SPARSE never.
    bool dense = false, drows = false;
    {
        const bool dup = rs.scans_repeats() && facts.repeats;
        // measured on MI355X (K = 10, V = 96; E-step launch, dense rows vs the CSR sweep): 10k documents 12.4 vs 10.9 us (the single-step build),
        // 15k 12.8 vs 14.1, 20k 16.7 vs 19.3, 40k 20.2 vs 27.7, 640k 190 vs 380 -- every corpus beyond the single-step build's reach
        // (profiles/experiments/r03_sweeps/dense_crossover.sh; round 2's build only paid from 49k documents: its epilogue cost 19 us)
        const bool big = D > 12 * G * ncu;
        const bool off32 = (int64_t)D * K * 8 < ((int64_t)1 << 32) && (int64_t)D * 16 * (SL + 1) * 4 < ((int64_t)1 << 32);   // the build's 32-bit byte offsets
        dense = rs.shape && !dup && off32 && rs.dmode != 0 && (rs.dmode > 0 || (big && rs.dense_enough));
        drows = rs.drows_env && rs.rshape && !dup && rs.dense_enough;
        p.dup_terms = dup;
    }
    const bool small = !dense && (V <= 96) && KP <= 12 && ((D + 12 * G - 1) / (12 * G) <= ncu) && tune.grid_blocks == 0;
    // single-step build: just enough waves per block to cover the corpus with one block per CU (fewer co-resident waves
    // per SIMD = shorter step); mmm_tuning_opts.waves_per_block pins the count (more blocks than CUs are fine: two blocks share a CU)
    const int swaves = tune.waves_per_block > 0 ? std::min(12, tune.waves_per_block) : std::max(kMinWavesSingle, std::min(12, (D + G * ncu - 1) / (G * ncu)));
    int waves = small ? swaves : 8;
    auto lds_for = [&](int w) { return tabB * (2 + w) + (size_t)2 * w * G * KP * sizeof(double); };
    while (waves > 1 && lds_for(waves) > (small ? 150 : 80) * 1024) --waves;
    // tables + one slab beyond LDS: the wide path (k_lda_estep_wide).  It also takes K > 24: the LDS kernel's 32-topic build
    // spills (10k x 96-term documents, K = 32: 264 us per iteration against 189).  lda_build = MMM_BUILD_WIDE forces it, MMM_BUILD_SPARSE /
    // _DENSE avoid it where the LDS kernels can run (tests, A/B).
    const bool wide = lds_for(waves) > 160 * 1024 || KP > 32 || (tune.lda_build == MMM_BUILD_WIDE) || (tune.lda_build == MMM_BUILD_AUTO && KP >= 32);
    if (R > 1 && wide) {
        const char* why = tune.lda_build == MMM_BUILD_WIDE ? "lda_build = MMM_BUILD_WIDE takes the wide path (tables through L2)"
                        : KP > 32 ? "K > 32 topics take the wide path (no LDS build)"
                        : tune.lda_build == MMM_BUILD_AUTO && KP >= 32 ? "K >= 25 topics take the wide path under MMM_BUILD_AUTO"
                        : "the K x V tables and one slab exceed LDS (wide path)";
        out.refuse(MMM_ERR_UNSUPPORTED, "mmm_lda_create_batch: K=%d V=%d: %s, which has no batched build -- fit such shapes on single handles", K, V, why);
        return out;
    }
    p.KP = KP; p.L = L;
    p.waves_e = waves; p.lds_e = wide ? 0 : lds_for(waves); p.lds_tab = tabB; p.wide = wide;
    p.dense = dense && !wide; p.SL = SL; p.drows = (dense || drows) && !wide;
    if (!wide && tune.waves_per_block > 0) { const int w = tune.waves_per_block; if (w >= 1 && w <= (small ? kMaxWavesE : 8) && lds_for(w) <= 160 * 1024) { p.waves_e = w; p.lds_e = lds_for(w); } }
    const int docs_per_block = p.waves_e * G;
    const int blocks_per_cu = wide ? 8 : std::max(1, std::min<int>((small ? 12 : 8) / p.waves_e, (int)((160 * 1024) / p.lds_e)));
    p.single_step = !wide && small && (int64_t)p.waves_e * G * ncu * blocks_per_cu >= D;      // the grid covers every document at once
    p.grid_e = std::max(1, std::min((D + docs_per_block - 1) / docs_per_block, ncu * blocks_per_cu));
    if (wide) p.grid_e = std::max(1, std::min((D + kWavesPerBlock - 1) / kWavesPerBlock, ncu * blocks_per_cu));     // wave per document
    if (tune.grid_blocks > 0) p.grid_e = tune.grid_blocks;
    if ((int64_t)p.grid_e * docs_per_block < D) p.single_step = false;
    // statistics as a block product (k_lda_estep_block): the single-step geometry above is decided by the slab build's LDS, so that grid,
    // waves and the association of the cross-block sums are the same whichever build runs; the launch itself asks for what it uses
    p.block_stats = p.single_step && L == 16 && KP <= 12 && !p.dup_terms && !plan_off(tune, MMM_OFF_LDA_BLOCK_STATS);
    p.lds_b = sizeof(double) * ((size_t)KP * V + (size_t)p.waves_e * G * (((size_t)V + 15) & ~(size_t)15) + (size_t)p.waves_e * G * KP);
    if (p.dense)      // [16 SL][KP] table | [waves][K][V] slabs | [waves][G][KP] a_k | [waves][64][KP] gamma sums
        p.lds_d = sizeof(double) * ((size_t)16 * SL * KP + (size_t)p.waves_e * 16 * SL * KP + (size_t)p.waves_e * G * KP + (size_t)p.waves_e * kPlanWave * KP);
    if (p.dense && p.lds_d > 160 * 1024) { p.dense = false; p.drows = drows && !wide; }      // no dense-row build: rows only if the corpus is dense enough
    p.grid_s = std::max(1, std::min((D + kWavesPerBlock - 1) / kWavesPerBlock, ncu * 4));
    p.keeps_aexp_next = p.single_step && !ilda;
    // the forms of the corpus beside the CSR arrays
    p.rows16 = p.drows && !plan_off(tune, MMM_OFF_LDA_ROWS16) && facts.max_count < 65536;
    if (p.drows) p.SLs = p.rows16 ? count_row_slots16(SL) : SL;      // lane-major rows (LdaDev::dense): an even number of 16-bit slots per lane
    // padded rows for the ll blocks (V <= 128 slots, no document longer than its row).  (The ll blocks take their lanes per document from KP, the
    // rows of counts serve 16-lane groups only: K = 13..15 needs the padded rows too)
    p.padded_rows = V <= 128 && facts.longest_doc <= V && D > 0 && !wide && (!p.drows || KP > 15);
    return out;
}

// ===== MMCTM / IMMCTM ================================================================================================================
constexpr int kMaxM = 8;
constexpr int kKmax = 64;          // topics per modality (the theta loop is unrolled to 8 / 10 / 16 / 32; 33..64: the 64-topic build of the wide-table path;
                                   // sum K > 64: ctm_big.cuh)
constexpr int kWavesS = 4;         // stage / auxiliary kernels
constexpr int kCtmBigSlots = 4;    // coordinates per lane of ctm_big.cuh (kBigSlots): sum K <= 256

// shard sizes (documents, on a 256-CU device) below which the solve phase takes more lanes per document (measured: profiles/r05_solve_layouts.jsonl)
constexpr int kSolve10Lanes8Below = 75000;      // sum K = 10: 2 lanes x 5 coordinates -> 8 lanes x 2
constexpr int kSolve28Lanes32Below = 9000;        // sum K = 28: 16 lanes x 2 coordinates -> 32 lanes x 1
constexpr int kSolve28Waves4From = 40000;         // sum K = 28 as 16 x 2: three -> four persistent waves per SIMD

struct CtmPlan {
    int L = 64;                    // lanes per document in the theta phase
    bool big = false;              // 64 < sum K <= 256: the generic kernels of ctm_big.cuh (one wave per document, several coordinates per lane)
    bool wide = false;             // wide tables (sum_m K_m V_m beyond LDS): theta phase without table / slabs in LDS + k_ctm_stats_terms over posting lists
    int grid_e = 1, waves_e = 8;
    // dense corpora: the fused pass's theta phase over rows of 16-bit counts, one launch per modality (k_ctm_theta_dense)
    bool tdense = false; int tSL[kMaxM] = {0};
    int grid_s = 1, waves_s = 4;
    int Ls = 64;                   // lanes per document in the solve phase: L, or sum K for the packed builds (6 / 12), or 2 / 4 (cpl > 1)
    int cpl = 1;                   // coordinates per lane in the solve phase (k_ctm_solve_cpl: sum K = 10, 14, 28)
    int lam_occ = 4;               // waves per SIMD of the persistent solve build (3 for sum K = 28)
    bool persist = false;          // solve phase by k_ctm_solve_cpl (persistent waves, document slots refilled): cpl > 1, or cpl = 1 with Ls = L
    int grid_v = 1, grid_m = 1;
};

inline size_t ctm_estep_lds(const CtmPlan& p, int M, const int* K, const int* V, bool slab)     // theta phase
{
    const int G = kPlanWave / p.L;
    if (p.wide) return sizeof(double) * (size_t)p.waves_e * G * 2 * p.L;
    int GT = 0, slabn = 0;      // a wave's slab holds one modality at a time
    for (int i = 0; i < M; ++i) { GT += K[i] * V[i]; slabn = std::max(slabn, K[i] * V[i]); }
    size_t n = (size_t)GT + (size_t)p.waves_e * G * (slab ? 1 : 2) * p.L;      // (the fused pass: one scratch row per group)
    if (slab) n += (size_t)p.waves_e * slabn;
    return n * sizeof(double);
}

inline size_t ctm_theta_dense_lds(const CtmPlan& p, int i, int kmx)
{
    const int NW = p.waves_e;
    return sizeof(double) * ((size_t)16 * p.tSL[i] * kmx + (size_t)NW * 16 * p.tSL[i] * kmx + (size_t)NW * 4 * kmx + (size_t)NW * kPlanWave * kmx);
}

inline int theta_dense_kmx(int Km) { return Km <= 8 ? 8 : (Km <= 10 ? 10 : 16); }

// shapes without a build: refused before the corpus is looked at
inline bool ctm_refuse_shape(PlanVerdict& p, int M, const int* K, const int* V)
{
    int MK = 0;
    for (int i = 0; i < M; ++i) {
        if (K[i] < 1 || K[i] > kKmax || V[i] < 1)
            return p.refuse(MMM_ERR_UNSUPPORTED, "mmm_ctm_create: K[%d]=%d must be in 1..%d and V[%d]=%d >= 1", i, K[i], kKmax, i, V[i]);
        MK += K[i];
    }
    return MK > 64 * kCtmBigSlots && p.refuse(MMM_ERR_UNSUPPORTED, "mmm_ctm_create: sum(K)=%d must be <= %d", MK, 64 * kCtmBigSlots);
}

// The theta phase as far as the dimensions decide it: L, big, wide, waves_e, grid_e and whether rows of counts come into question
// (rows_shape, tSL).  nnz_m: entries per modality.
struct CtmThetaShape : Planned<CtmPlan> {
    bool rows_shape = false;       // shapes, density and size allow rows of counts: the corpus is looked at (repeated terms, counts >= 65536)
};

inline CtmThetaShape ctm_theta_plan(const mmm_tuning_opts& tune, int ncu, int D, int M, const int* K, const int* V, const int64_t* nnz_m)
{
    CtmThetaShape out;
    if (ctm_refuse_shape(out, M, K, V)) return out;
    CtmPlan& p = out.plan;
    int MK = 0;
    for (int i = 0; i < M; ++i) MK += K[i];
    p.L = MK <= 16 ? 16 : (MK <= 32 ? 32 : 64);
    p.big = MK > 64;      // more coordinates than lanes: the generic kernels of ctm_big.cuh (and the wide-table data flow)
    const int G = kPlanWave / p.L;
    p.waves_e = 8;
    while (p.waves_e > 1 && ctm_estep_lds(p, M, K, V, true) > 150 * 1024) p.waves_e >>= 1;
    // table + one slab beyond LDS: the wide path (theta phase through L2, gamma statistics by k_ctm_stats_terms).  ctm_build =
    // MMM_BUILD_WIDE forces it for any shape (tests, A/B)
    int kmax_all = 0;
    for (int i = 0; i < M; ++i) kmax_all = std::max(kmax_all, K[i]);
    if (ctm_estep_lds(p, M, K, V, true) > 160 * 1024 || tune.ctm_build == MMM_BUILD_WIDE || kmax_all > 32 || p.big) { p.wide = true; p.waves_e = 8; }
    const int dpb = p.waves_e * G;
    const int per_cu = p.wide ? 2 : std::max(1, (int)((160 * 1024) / ctm_estep_lds(p, M, K, V, true)));
    p.grid_e = std::max(1, std::min((D + dpb - 1) / dpb, ncu * std::min(per_cu, 2)));
    // Dense corpora: the fused pass's theta phase over rows of 16-bit counts (k_ctm_theta_dense), when every modality has at most 16 topics
    // and 128 terms, no document lists a term twice, every count fits 16 bits and at least half of the D x V_m entries are present.
    // ctm_build = MMM_BUILD_DENSE / _SPARSE forces / forbids it (tests, A/B); by default corpora of at least 32 documents per CU take it (below, a block of
    // the 16-lane layout has less than one wave step and the slab kernel is as fast).
    const int dmode = tune.ctm_build == MMM_BUILD_DENSE ? 1 : (tune.ctm_build == MMM_BUILD_AUTO ? -1 : 0);
    bool ok = !p.wide && !p.big && dmode != 0 && D > 0 && (int64_t)D * MK * 8 < ((int64_t)1 << 32) && D < (1 << 24);      // (32-bit byte offsets into lambda and into the rows)
    int64_t present = 0, cells = 0;
    for (int i = 0; i < M && ok; ++i) {
        const int sl = count_row_slots(V[i]);
        if (sl == 0 || K[i] > 16 || theta_dense_kmx(K[i]) * sl > 64) { ok = false; break; }      // (the statistics must stay in registers)
        p.tSL[i] = sl;
        present += nnz_m[i]; cells += (int64_t)D * V[i];
    }
    if (ok && 2 * present < cells) ok = false;
    if (ok && dmode < 0 && D < 32 * ncu) ok = false;
    out.rows_shape = ok;
    return out;
}

// th: ctm_theta_plan of the same arguments; per_modality: the facts of each modality's segment, `repeats` looked for, read only when th.rows_shape
inline Planned<CtmPlan> ctm_plan(const mmm_tuning_opts& tune, int ncu, int R, int D, int M, const int* K, const CtmThetaShape& th, const CorpusFacts* per_modality)
{
    Planned<CtmPlan> out = th;
    if (out.refusal) return out;
    CtmPlan& p = out.plan;
    int MK = 0;
    for (int i = 0; i < M; ++i) MK += K[i];
    {
        bool ok = th.rows_shape;
        for (int i = 0; i < M && ok; ++i) if (per_modality[i].repeats || per_modality[i].max_count >= 65536) ok = false;
        if (ok) {
            p.waves_e = 8;
            for (int i = 0; i < M; ++i) if (ctm_theta_dense_lds(p, i, theta_dense_kmx(K[i])) > 160 * 1024) ok = false;
        }
        if (ok) {
            p.tdense = true;
            p.grid_e = std::max(1, std::min((D + 31) / 32, ncu));
        }
    }
    if (tune.grid_blocks > 0) p.grid_e = tune.grid_blocks;
    // (one block short of four per CU: the log-likelihood launch carries the Gaussian M-step as one block more, and a 1,025th block waits for a
    // slot -- a second round of one block: + 3.3 us at config 5, + 4.6 us at config 4)
    p.grid_s = std::max(1, std::min((D + kWavesS - 1) / kWavesS, ncu * 4 - 1));
    p.waves_s = 4;
    // solve phase: packed document groups (sum K lanes per document) for the shapes with a build (MMM_OFF_CTM_PACKED: the 16-lane rows)
    p.Ls = p.L;
    {
        if (!plan_off(tune, MMM_OFF_CTM_PACKED) && (MK == 6 || MK == 10 || MK == 12)) p.Ls = MK;
        // several coordinates per lane (k_ctm_solve_cpl): sum K = 10 -> 2 lanes x 5 coordinates (32 document slots per wave; BASELINE config 5:
        // solve phase 334 -> 263 us); sum K = 28 -> 16 lanes, 14 of them x 2 coordinates (round 3; 4 slots per wave, 134 VGPRs at 3 waves per
        // SIMD, no scratch: BASELINE config 4 solve phase 1,096 -> 974 us at pass 20, 794 -> 757 us at pass 60 -- and the sums of a document
        // are associated exactly as the 32-lane butterfly associates them, so not a bit changes).  MMM_OFF_CTM_CPL switches the path off
        // (one coordinate per lane, lock step: k_ctm_estep<L, 1>).
        const int want = tune.solve_lanes;      // 0: by shape and corpus size
        const bool lockstep10 = MK == 10 && want == 16;      // sum K = 10 with solve_lanes = 16: the packed / 16-lane lock-step build (A/B)
        if (!plan_off(tune, MMM_OFF_CTM_CPL) && !lockstep10) {
            // Which layout: the full-size configurations keep the layouts of rounds 2-3 (most documents per wave trip); a SHARD -- D small
            // enough that those layouts leave SIMDs without a wave or slots without a document -- takes more lanes per document
            // (profiles/r05_shard_sizes.jsonl: sum K = 10 at 12,505 documents 2 x 5 -> 8 x 2; sum K = 28 at 6,249 documents 16 x 2 -> 32 x 1).
            if (MK == 10) {
                // The two sum K = 10 layouts associate a document's sums differently, so this choice decides bits: it is made from D alone, and
                // a restart batch takes what a single handle on the same corpus takes (replica r is bitwise the single fit of its gamma0).  The
                // sum K = 28 choices below change no bit (both layouts associate as the 32-lane butterfly does; the wave count only deals the
                // documents out) and count the replicas that fill the chip, D * R.
                const bool wide8 = want == 8 || (want == 0 && D < kSolve10Lanes8Below * (ncu / 256.0));
                if (wide8) { p.Ls = 8; p.cpl = 2; p.lam_occ = 3; } else { p.Ls = 2; p.cpl = 5; p.lam_occ = 2; }
                p.persist = true;
            } else if (MK == 28) {
                const bool wide32 = want == 32 || (want == 0 && (int64_t)D * R < kSolve28Lanes32Below * (ncu / 256.0));
                // (16 x 2 needs 125 VGPRs: four waves per SIMD fit.  With three or more documents per slot the fourth wave pays -- config 4 at
                // 50,000 documents 0.875 -> 0.861 ms per pass; at 25,000 / 12,500 documents it costs 4 % / 8 %: tools/ab_tuning.py, solve_waves)
                const bool four = (int64_t)D * R >= kSolve28Waves4From * (ncu / 256.0);
                if (wide32) { p.Ls = 32; p.cpl = 1; p.lam_occ = 4; } else { p.Ls = 16; p.cpl = 2; p.lam_occ = four ? 4 : 3; }
                p.persist = true;
            }
        }
    }
    if (p.big) { p.Ls = 64; p.cpl = kCtmBigSlots; p.persist = false; }      // ctm_big.cuh: lane l holds coordinates l + 64 q
    const int Gs = kPlanWave / p.Ls;
    p.grid_v = std::max(1, std::min((D + p.waves_s * Gs - 1) / (p.waves_s * Gs), ncu * 8));
    // k_ctm_solve_cpl: persistent waves, each with a contiguous range of documents that its slots work through (a finished slot takes the
    // range's next document): as many as are resident at once (lam_occ per SIMD), fewer when every document has a slot of its own.  (Round 5
    // measured whole numbers of waves per SIMD with more documents than slots each for small shards: slower -- 6,249 documents of config 4:
    // 200 us with one wave per SIMD against 188; the phase is issue-bound per SIMD and a half-filled wave costs a full trip.)
    if (p.persist) {
        const int blocks_full = (D + p.waves_s * Gs - 1) / (p.waves_s * Gs);      // every document a slot of its own
        p.grid_v = std::max(1, std::min(blocks_full, ncu * p.lam_occ));
        if (tune.solve_waves > 0) p.grid_v = std::max(1, std::min(blocks_full, ncu * tune.solve_waves));
    }
    // moment sums: whole 32-document tiles per block (a short last tile is padded to 32 and costs as much as a full one), at most 1024 blocks
    {
        const int tiles_per_block = std::max(1, (D + 32 * 1024 - 1) / (32 * 1024));
        p.grid_m = std::max(1, (D + 32 * tiles_per_block - 1) / (32 * tiles_per_block));
    }
    if (tune.moment_blocks > 0) p.grid_m = tune.moment_blocks;
    return out;
}
