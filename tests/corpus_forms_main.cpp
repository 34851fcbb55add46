// corpus_forms_main.cpp -- prints, without a device, what mmm_lda_create* / mmm_ctm_create* would decide for a case (csrc/create_plan.h)
// and the forms they would build of its corpus (csrc/corpus_forms.h).  tests/test_create_plan_cpu.py compiles and runs it.
//
// Input (a file of whitespace-separated integers, any number of cases):
//   mode  1 = LDA plan, 2 = CTM plan, 3 = corpus forms of one segment, 4 = postings_stats_waves(nnz, nterms), 0 = end
//   modes 1-3: lda_build ctm_build geometry_cus grid_blocks waves_per_block moment_blocks disable solve_lanes solve_waves | ncu R ilda |
//              D M | K[M] | V[M] | doc_ptr[M (D + 1)] | term[nnz] | count[nnz]
//   mode 4:    nnz nterms
// Output: one line "case <n>" per case, then "<key> <integers ...>" lines.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "create_plan.h"

static FILE* in;

static long long next()
{
    long long v;
    if (fscanf(in, "%lld", &v) != 1) { fprintf(stderr, "corpus_forms_main: short input\n"); exit(2); }
    return v;
}

template <class T>
static void line(const char* key, const std::vector<T>& v)
{
    printf("%s", key);
    for (const T& x : v) printf(" %lld", (long long)x);
    printf("\n");
}

static void pairs(const char* key, const std::vector<CountPair>& v)
{
    printf("%s", key);
    for (const CountPair& x : v) printf(" %d %d", x.x, x.y);
    printf("\n");
}

#define SHOW(p, f) printf(#f " %lld\n", (long long)(p).f)

int main(int argc, char** argv)
{
    if (argc != 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: corpus_forms_main CASES\n"); return 2; }
    for (int n = 0;; ++n) {
        const int mode = (int)next();
        if (mode == 0) break;
        printf("case %d\n", n);
        if (mode == 4) {
            const int64_t nnz = next(); const int nterms = (int)next();
            printf("stats_waves %d\n", postings_stats_waves(nnz, nterms));
            continue;
        }
        mmm_tuning_opts t{};
        t.lda_build = (int)next(); t.ctm_build = (int)next(); t.geometry_cus = (int)next(); t.grid_blocks = (int)next(); t.waves_per_block = (int)next();
        t.moment_blocks = (int)next(); t.disable = (unsigned)next(); t.solve_lanes = (int)next(); t.solve_waves = (int)next();
        int ncu = (int)next(); const int R = (int)next(); const bool ilda = next() != 0;
        if (t.geometry_cus > 0) ncu = t.geometry_cus;      // (mmm_geo_cus)
        const int D = (int)next(), M = (int)next();
        std::vector<int> K((size_t)M), V((size_t)M);
        for (int& k : K) k = (int)next();
        for (int& v : V) v = (int)next();
        std::vector<int64_t> dp((size_t)M * (D + 1));
        for (int64_t& x : dp) x = next();
        const int64_t nnz = dp.back();
        std::vector<int32_t> term((size_t)nnz), count((size_t)nnz);
        for (int32_t& x : term) x = (int32_t)next();
        for (int32_t& x : count) x = (int32_t)next();
        std::vector<int64_t> nnz_m((size_t)M);
        for (int i = 0; i < M; ++i) nnz_m[(size_t)i] = dp[(size_t)i * (D + 1) + D] - dp[(size_t)i * (D + 1)];
        if (mode == 1) {
            const LdaRowShape rs = lda_row_shape(t, D, V[0], K[0], nnz);
            const CorpusFacts f = corpus_facts(D, V[0], dp.data(), term.data(), count.data(), rs.scans_repeats());
            const Planned<LdaPlan> out = lda_plan(t, ncu, R, D, V[0], K[0], rs, f, ilda);
            const LdaPlan& p = out.plan;
            SHOW(out, refusal); printf("why %s\n", out.why.c_str());
            SHOW(p, KP); SHOW(p, L); SHOW(p, SL); SHOW(p, SLs); SHOW(p, dense); SHOW(p, drows); SHOW(p, rows16); SHOW(p, padded_rows); SHOW(p, dup_terms);
            SHOW(p, wide); SHOW(p, single_step); SHOW(p, block_stats); SHOW(p, keeps_aexp_next); SHOW(p, grid_e); SHOW(p, waves_e); SHOW(p, grid_s);
            SHOW(p, lds_e); SHOW(p, lds_tab); SHOW(p, lds_b); SHOW(p, lds_d);
        } else if (mode == 2) {
            std::vector<CorpusFacts> f((size_t)M);
            const CtmThetaShape th = ctm_theta_plan(t, ncu, D, M, K.data(), V.data(), nnz_m.data());
            if (th.rows_shape)
                for (int i = 0; i < M; ++i) f[(size_t)i] = corpus_facts(D, V[(size_t)i], dp.data() + (size_t)i * (D + 1), term.data(), count.data(), true);
            const Planned<CtmPlan> out = ctm_plan(t, ncu, R, D, M, K.data(), th, f.data());
            const CtmPlan& p = out.plan;
            SHOW(out, refusal); printf("why %s\n", out.why.c_str());
            SHOW(p, L); SHOW(p, big); SHOW(p, wide); SHOW(p, grid_e); SHOW(p, waves_e); SHOW(th, rows_shape); SHOW(p, tdense);
            line("tSL", std::vector<int>(p.tSL, p.tSL + M));
            SHOW(p, grid_s); SHOW(p, waves_s); SHOW(p, Ls); SHOW(p, cpl); SHOW(p, lam_occ); SHOW(p, persist); SHOW(p, grid_v); SHOW(p, grid_m);
            if (!out.refusal) {
                printf("estep_lds_slab %zu\n", ctm_estep_lds(p, M, K.data(), V.data(), true));
                printf("estep_lds %zu\n", ctm_estep_lds(p, M, K.data(), V.data(), false));
            }
        } else {
            const int v = V[0], sl = count_row_slots(v);
            const CorpusFacts f = corpus_facts(D, v, dp.data(), term.data(), count.data(), true);
            printf("slots %d\n", sl);
            printf("facts %d %lld %d\n", f.max_count, (long long)f.longest_doc, (int)f.repeats);
            printf("facts_lazy %d\n", (int)corpus_facts(D, v, dp.data(), term.data(), count.data(), false).repeats);
            if (sl > 0) {
                line("rows16", pack_count_rows<unsigned short>(D, count_row_slots16(sl), kRows16Spare, dp.data(), term.data(), count.data()));
                line("rows32", pack_count_rows<int>(D, sl, 0, dp.data(), term.data(), count.data()));
            }
            pairs("tc", term_count_pairs(nnz, term.data(), count.data()));
            if (f.longest_doc <= v) pairs("ell", padded_term_rows(D, v, dp.data(), term.data(), count.data()));
            const Postings p = postings_by_term(D, M, V.data(), dp.data(), term.data(), count.data());
            printf("nterms %d\n", p.nterms);
            line("term_ptr", p.term_ptr);
            pairs("post", p.post);
            printf("stats_waves %d\n", p.stats_waves);
        }
    }
    fclose(in);
    return 0;
}
