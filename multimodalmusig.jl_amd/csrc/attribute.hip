// attribute.hip -- mmm_attribute_mutations: which signature caused this mutation?  The posterior of every catalogue signature per queried
// (document, term) pair under the document's fit over its `allowed` row, and its uncertainty by the non-parametric bootstrap of
// mmm_resample_counts, draws, fits, posteriors and accumulation in one launch (no counterpart in the reference; include/mmmusig.h has the
// normative definition, DESIGN.md section 4.26 the reasoning).
//
// Two phases on the context's stream, in the shape of presence.hip.  "Observed": one wave per queried document behind a work counter, as
// k_refit hands out documents; it leaves the weights, the posteriors of the document's queries and the status.  "Replicates": grid
// (status-0 document, replicate chunk); a block stages the rows of the document's signatures in LDS (where they fit), the document's prefix
// sums, the terms of its entries and its query list, and then every wave takes one replicate at a time: Philox draws into its own LDS
// histogram, f = n / N, the fit, the mixture at every term, the posteriors with lanes over (query, active signature) pairs, integer
// atomics.  The replicate's counts never leave LDS.  Lane l owns the terms v = l, l + 64, ...; fit(A) is the one refit.hip runs
// (mixture_fit.cuh), the draw is the resampler's (mmm_philox.h).  No log anywhere; every accumulator is an integer.
#include "mmm_internal.h"
#include "dev_math.h"
#include "mmm_philox.h"
#include "mixture_fit.cuh"

namespace {

constexpr int kAtMaxC = 256;
constexpr int kAtMaxV = 4096;                   // a wave's f, r and count vector stay in LDS
constexpr int kAtMaxRow = 4096;                 // CSR entries of a queried document: its prefix sums and terms are staged in LDS
constexpr int kAtMaxB = 4096;                   // replicates per call: sumsq_fx <= 4096 * 2^48, and mmm_replicate_summary takes the result
constexpr int kAtMaxQLds = 4096;                // query terms a block stages; a longer list is read through L2
constexpr int kAtMaxWaves = 8;                  // 8 waves of up to 256 VGPRs fill a CU: two per SIMD
constexpr size_t kAtLdsBlock = 160 * 1024;      // LDS a block may take (the CU's)
constexpr double kAtScale = 16777216.0;         // 2^24: x = floor(rho 2^24)
constexpr int kAtPairChunk = 1 << 20;           // queries a pair loop takes at once: (query, signature) indices stay 32-bit words

struct AtArgs {
    int D, C, V, Cp, G, maxiter;
    double tol;
    long long Q;
    const int64_t* doc_ptr; const int32_t* term; const int32_t* count;
    const double* P;                 // [C][V], rows normalised
    const uint8_t* allowed;          // [D][C] or NULL
    const int64_t* q_ptr; const int32_t* q_term; const int32_t* q_mult; const int32_t* q_group;      // q_mult / q_group may be NULL
    const int32_t* items;            // the documents this launch takes
    int n_items;
    double* w; double* post; int8_t* status; unsigned long long* iters;
    int* counter;                    // next item of the observed phase
    int wave_doubles;
    // replicate phase
    const uint32_t* cum;             // [nnz] inclusive prefix sums per document
    int B, reps_per_block, P2c, Wl, Ql, fixed_doubles, stage_doubles;      // LDS words of the prefix sums, the entries' terms, the queries
    uint32_t b0, k0, k1, stream;
    unsigned long long* sum_fx; unsigned long long* sumsq_fx; int32_t* top_count; int32_t* void_count; unsigned long long* group_fx;
    double* rep_post;                // [B][Q][C] or NULL
};

// a wave's own LDS: the weights, the list of signatures (in the order of c, padded to a multiple of 64 with a valid row whose results are
// dropped), f_v, r_v (after the fit: the mixture q_v) and the count vector
struct AtWave {
    double* w; int* act; double* fb; double* rb; uint32_t* hist;
};

__host__ __device__ inline int at_wave_doubles(int Cp, int V) { return (Cp + Cp / 2 + 2 * V + (V + 1) / 2 + 1) & ~1; }

__device__ __forceinline__ AtWave at_carve(double* base, int Cp, int V)
{
    AtWave w;
    w.w = base;
    w.act = (int*)(base + Cp);
    w.fb = base + Cp + Cp / 2; w.rb = w.fb + V;
    w.hist = (uint32_t*)(w.rb + V);
    return w;
}

// q[v] = sum_i w[i] P[act[i]][v] in the order of the list, for every term
__device__ __forceinline__ void at_mixture(const double* __restrict__ P, const int* act, const double* w, int n, double* q, int V, int lane)
{
    for (int v = lane; v < V; v += 64) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += w[i] * P[act[i] * V + v];
        q[v] = s;
    }
}

// the posterior of list member i at term v: the product and the division are separate roundings; 0 where the mixture is 0
__device__ __forceinline__ double at_rho(const double* __restrict__ P, const AtWave& w, int i, int v, int V)
{
    const double qv = w.rb[v];
    const double x = w.w[i] * P[w.act[i] * V + v];
    return qv > 0.0 ? x / qv : 0.0;
}

// Observed phase.  Dynamic LDS: per wave at_wave_doubles doubles; the catalogue is read through L2 (one fit per document: a B-th of the
// call's work).  The host has zeroed every output; a document that cannot be fitted (N = 0 or an empty `allowed` row) gets its status and
// nothing else.
__global__ __launch_bounds__(64 * kAtMaxWaves) void k_attribute_obs(const AtArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_at[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, V = a.V;
    const AtWave w = at_carve(s_at + (size_t)wave * a.wave_doubles, a.Cp, V);
    const double* __restrict__ P = a.P;
    const RfCountsU32 counts{w.hist};
    for (;;) {
        const int j = rf_next_item(a.counter, lane);       // its contract shapes this loop: if / else, one closing fence
        if (j >= a.n_items) break;
        const int d = a.items[j];
        // ---- n_v (duplicate terms summed), N, f_v
        for (int v = lane; v < V; v += 64) w.hist[v] = 0u;
        rf_wave_sync();
        double Np = 0.0;
        for (int64_t e = a.doc_ptr[d] + lane; e < a.doc_ptr[d + 1]; e += 64) {
            const int cnt = a.count[e];
            if (cnt > 0) { atomicAdd(&w.hist[a.term[e]], (uint32_t)cnt); Np += (double)cnt; }
        }
        const double N = wave_sum(Np);             // integers below 2^31: exact in any order
        rf_wave_sync();
        for (int v = lane; v < V; v += 64) w.fb[v] = N > 0.0 ? (double)w.hist[v] / N : 0.0;
        int none;
        const int n = rf_active_list(a.allowed ? a.allowed + (size_t)d * C : nullptr, C, -1, w.act, lane, none);
        if (N == 0.0 || n == 0) {
            if (lane == 0) a.status[d] = 3;
        } else {
            rf_pad_list(w.act, n, lane);
            rf_wave_sync();
            const int it = rf_fit(P, w.act, w.w, n, w.fb, counts, w.rb, V, lane, a.maxiter, a.tol);
            at_mixture(P, w.act, w.w, n, w.rb, V, lane);
            rf_wave_sync();
            for (int i = lane; i < n; i += 64) a.w[(size_t)d * C + w.act[i]] = w.w[i];
            const int64_t q0 = a.q_ptr[d];
            const int nq = (int)(a.q_ptr[d + 1] - q0);
            for (int qb = 0; qb < nq; qb += kAtPairChunk) {
                const int m = min(kAtPairChunk, nq - qb);
                for (int idx = lane; idx < m * n; idx += 64) {
                    const int e = idx / n, i = idx - e * n;
                    const int64_t qe = q0 + qb + e;
                    a.post[(size_t)qe * C + w.act[i]] = at_rho(P, w, i, a.q_term[qe], V);
                }
            }
            if (lane == 0) a.iters[d] = (unsigned long long)it;
        }
        rf_wave_sync();
    }
}

// Replicate phase: grid (documents, replicate chunks), blockDim 64 nw.  Dynamic LDS: uint32 cum[P2c] | int eterm[Wl] | int qterm[Ql] |
// int c_of[Cp] (the catalogue rows of the list), together fixed_doubles | P_LDS: the rows of A_d at stride V | per wave at_wave_doubles
// doubles.  After the set-up no wave waits for another.
template <bool P_LDS>
__global__ __launch_bounds__(64 * kAtMaxWaves) void k_attribute_rep(const AtArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_at[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6), nt = (int)blockDim.x;
    const int C = a.C, V = a.V;
    const int d = a.items[blockIdx.x];
    uint32_t* s_cum = (uint32_t*)s_at;
    int* s_et = (int*)(s_cum + a.P2c);
    int* s_q = s_et + a.Wl;
    int* s_c = s_q + a.Ql;
    double* s_rows = s_at + a.fixed_doubles;
    double* wave_base = s_rows + (P_LDS ? a.stage_doubles : 0);
    const AtWave w = at_carve(wave_base + (size_t)wave * a.wave_doubles, a.Cp, V);
    // every wave builds the list for itself (the same bits); wave 0 leaves the catalogue rows it names for the outputs
    int none;
    const int n = rf_active_list(a.allowed ? a.allowed + (size_t)d * C : nullptr, C, -1, w.act, lane, none);      // >= 1: the document has status 0;
    if (wave == 0)                                                                                                // <= stage_doubles / V where staged
        for (int i = lane; i < n; i += 64) s_c[i] = w.act[i];
    if (P_LDS) {
        for (int i = wave; i < n; i += nw) {
            const double* src = a.P + (size_t)w.act[i] * V;
            for (int v = lane; v < V; v += 64) s_rows[(size_t)i * V + v] = src[v];
        }
        rf_wave_sync();
        for (int i = lane; i < ((n + 63) & ~63); i += 64) w.act[i] = i < n ? i : 0;
    } else {
        rf_pad_list(w.act, n, lane);
    }
    const double* __restrict__ P = P_LDS ? s_rows : a.P;
    // ---- the document's prefix sums (padded to a power of two for the search), the terms of its entries, its queries
    const int64_t e0 = a.doc_ptr[d];
    const int W = (int)(a.doc_ptr[d + 1] - e0);                // 1 .. kAtMaxRow: N > 0
    const uint32_t* cg = a.cum + e0;
    const uint32_t N = cg[W - 1];
    int half = 1;
    while (2 * half < W) half <<= 1;
    if (W == 1) half = 0;
    for (int e = tid; e < 2 * half || e < W; e += nt) s_cum[e] = e < W ? cg[e] : 0xffffffffu;
    for (int e = tid; e < W; e += nt) s_et[e] = a.term[e0 + e];
    const int64_t q0 = a.q_ptr[d];
    const int nq = (int)(a.q_ptr[d + 1] - q0);
    const bool q_lds = nq <= a.Ql;
    if (q_lds)
        for (int e = tid; e < nq; e += nt) s_q[e] = a.q_term[q0 + e];
    const int* qt = q_lds ? s_q : a.q_term + q0;
    for (int v = lane; v < V; v += 64) w.hist[v] = 0u;
    __syncthreads();                                           // the staged rows, sums, terms and queries are there
    // ---- the wave's replicates
    const RfCountsU32 counts{w.hist};
    const double Nd = (double)N;
    const int bbeg = (int)blockIdx.y * a.reps_per_block, bend = min(a.B, bbeg + a.reps_per_block);
    const size_t GC = (size_t)a.G * C;
    unsigned long long its = 0ull;
    for (int b = bbeg + wave; b < bend; b += nw) {
        resample_row_terms(lane, half, N, s_cum, s_et, w.hist, (uint32_t)d, a.b0 + (uint32_t)b, a.stream, a.k0, a.k1);
        rf_wave_sync();
        for (int v = lane; v < V; v += 64) w.fb[v] = (double)w.hist[v] / Nd;
        rf_wave_sync();
        its += (unsigned long long)rf_fit(P, w.act, w.w, n, w.fb, counts, w.rb, V, lane, a.maxiter, a.tol);
        at_mixture(P, w.act, w.w, n, w.rb, V, lane);
        rf_wave_sync();
        // ---- lanes over (query, active signature) pairs: rho, x = floor(rho 2^24), the sums
        for (int qb = 0; qb < nq; qb += kAtPairChunk) {
            const int m = min(kAtPairChunk, nq - qb);
            for (int idx = lane; idx < m * n; idx += 64) {
                const int e = idx / n, i = idx - e * n;
                const size_t qe = (size_t)(q0 + qb + e);
                const double rho = at_rho(P, w, i, qt[qb + e], V);
                const unsigned long long x = (unsigned long long)(rho * kAtScale);       // rho <= 1: the product is exact, the conversion floors
                const int c = s_c[i];
                if (x) {
                    atomicAdd(&a.sum_fx[qe * C + c], x);
                    atomicAdd(&a.sumsq_fx[qe * C + c], x * x);
                    const int g = a.q_group ? a.q_group[qe] : -1;
                    if (g >= 0) atomicAdd(&a.group_fx[(size_t)b * GC + (size_t)g * C + c], (unsigned long long)(a.q_mult ? a.q_mult[qe] : 1) * x);
                }
                if (a.rep_post) a.rep_post[((size_t)b * (size_t)a.Q + qe) * C + c] = rho;
            }
        }
        // ---- lanes over queries: the signature with the largest rho (ties: the lowest c, the list is in the order of c), or the void count
        for (int e = lane; e < nq; e += 64) {
            const int v = qt[e];
            if (!(w.rb[v] > 0.0)) {
                atomicAdd(&a.void_count[q0 + e], 1);
            } else {
                double best = -1.0;
                int bi = 0;
                for (int i = 0; i < n; ++i) {
                    const double rho = at_rho(P, w, i, v, V);
                    if (rho > best) { best = rho; bi = i; }
                }
                atomicAdd(&a.top_count[(size_t)(q0 + e) * C + s_c[bi]], 1);
            }
        }
        for (int v = lane; v < V; v += 64) w.hist[v] = 0u;
        rf_wave_sync();
    }
    if (lane == 0 && its) atomicAdd(&a.iters[d], its);
}

// replicates per block: one per wave, more while the launch still covers the device several times over (a block's set-up is shared by
// its replicates); the geometry cannot change a bit of the output
int at_reps_per_block(int nw, int B, size_t n, int cus)
{
    int rpb = nw;
    while (rpb < B && (int64_t)n * ((B + 2 * rpb - 1) / (2 * rpb)) >= 8ll * cus) rpb *= 2;
    while ((B + rpb - 1) / rpb > 65535) rpb *= 2;
    return rpb;
}

int at_pow2(int64_t x)
{
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

} // namespace

extern "C" int mmm_attribute_mutations(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* cat,
                                       const uint8_t* allowed, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_mult, const int32_t* q_group, int G,
                                       int B, int b0, uint64_t seed, uint32_t stream, int maxiter, double tol, double* w, double* post, int8_t* status,
                                       int64_t* iters, uint64_t* sum_fx, uint64_t* sumsq_fx, int32_t* top_count, int32_t* void_count, uint64_t* group_fx,
                                       double* rep_post)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, C >= 1 && V >= 1 && D >= 0 && cat && q_ptr && G >= 0, "mmm_attribute_mutations: NULL argument, D < 0, C < 1, V < 1 or G < 0");
    if (C > kAtMaxC) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_attribute_mutations: C = %d catalogue signatures (limit %d)", C, kAtMaxC);
    if (V > kAtMaxV)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_attribute_mutations: V = %d terms; a wave keeps f, r and its count vector in LDS, which holds at most V = %d", V, kAtMaxV);
    MMM_CHECK(ctx, maxiter >= 1 && tol >= 0.0, "mmm_attribute_mutations: maxiter = %d (>= 1), tol = %g (>= 0)", maxiter, tol);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0, "mmm_attribute_mutations: B < 0 or b0 < 0");
    MMM_CHECK(ctx, (int64_t)b0 + (int64_t)B <= (int64_t)INT32_MAX, "mmm_attribute_mutations: b0 + B exceeds 2^31 - 1");
    if (B > kAtMaxB)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_attribute_mutations: B = %d replicates in one call (limit %d: sumsq_fx stays below 2^64; chunked calls add)", B, kAtMaxB);
    if (int rc = mmm_check_csr(ctx, "mmm_attribute_mutations", D, V, doc_ptr, term, count)) return rc;
    std::vector<int32_t> n_doc((size_t)D);
    if (int rc = mmm_doc_totals(ctx, "mmm_attribute_mutations", D, doc_ptr, count, n_doc.data())) return rc;
    std::vector<double> P;           // the catalogue with rows normalised: mmm_refit_exposures' P
    if (int rc = mmm_normalise_rows(ctx, "mmm_attribute_mutations", C, V, cat, P)) return rc;
    // ---- the queries: a CSR over documents
    MMM_CHECK(ctx, q_ptr[0] == 0, "mmm_attribute_mutations: q_ptr[0] != 0");
    for (int d = 0; d < D; ++d) MMM_CHECK(ctx, q_ptr[d + 1] >= q_ptr[d], "mmm_attribute_mutations: q_ptr decreases at document %d", d);
    const int64_t Q = q_ptr[D];
    MMM_CHECK(ctx, Q == 0 || q_term, "mmm_attribute_mutations: q_term == NULL");
    if (Q >= ((int64_t)1 << 31)) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_attribute_mutations: Q = %lld queries (limit 2^31 - 1)", (long long)Q);
    std::vector<int64_t> gsum((size_t)G, 0);
    for (int64_t e = 0; e < Q; ++e) {
        MMM_CHECK(ctx, q_term[e] >= 0 && q_term[e] < V, "mmm_attribute_mutations: query %lld has term %d (V = %d)", (long long)e, q_term[e], V);
        MMM_CHECK(ctx, !q_mult || q_mult[e] >= 1, "mmm_attribute_mutations: query %lld has mult %d (>= 1)", (long long)e, q_mult ? q_mult[e] : 0);
        MMM_CHECK(ctx, !q_group || (q_group[e] >= -1 && q_group[e] < G), "mmm_attribute_mutations: query %lld has group %d (-1 .. G - 1 = %d)", (long long)e,
                  q_group ? q_group[e] : 0, G - 1);
        if (q_group && q_group[e] >= 0) gsum[(size_t)q_group[e]] += q_mult ? q_mult[e] : 1;
    }
    for (int g = 0; g < G; ++g)
        if (gsum[(size_t)g] >= ((int64_t)1 << 31))
            return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_attribute_mutations: group %d holds mults of %lld in all (limit 2^31 - 1: group_fx stays below 2^64)", g,
                            (long long)gsum[(size_t)g]);
    std::vector<int32_t> queried;
    for (int d = 0; d < D; ++d) {
        if (q_ptr[d + 1] == q_ptr[d]) continue;
        if (doc_ptr[d + 1] - doc_ptr[d] > kAtMaxRow)
            return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_attribute_mutations: queried document %d has %lld CSR entries (limit %d: its prefix sums are staged in LDS)", d,
                            (long long)(doc_ptr[d + 1] - doc_ptr[d]), kAtMaxRow);
        queried.push_back(d);
    }
    if (D == 0 || Q == 0) return MMM_OK;
    const bool groups = G > 0 && q_group;
    MMM_CHECK(ctx, w && post && status && iters, "mmm_attribute_mutations: NULL output");
    MMM_CHECK(ctx, B == 0 || (sum_fx && sumsq_fx && top_count && void_count && (G == 0 || group_fx)), "mmm_attribute_mutations: NULL replicate output");
    const size_t DC = (size_t)D * C, QC = (size_t)Q * C, BGC = (size_t)B * G * C;
    const bool want_rep = rep_post && B > 0;
    const int64_t nnz = doc_ptr[D];
    std::vector<uint32_t> cum((size_t)nnz);      // inclusive prefix sums per document in CSR order: what the resampler's draw searches
    for (int d = 0; d < D; ++d) {
        uint32_t s = 0;
        for (int64_t e = doc_ptr[d]; e < doc_ptr[d + 1]; ++e) { s += (uint32_t)count[e]; cum[(size_t)e] = s; }
    }

    const int Cp = (C + 63) & ~63, cus = std::max(1, mmm_geo_cus(ctx));
    const int wd = at_wave_doubles(Cp, V);
    const size_t pw = sizeof(double) * (size_t)wd;

    DevCsr csr; DevBuf<int64_t> qp; DevBuf<int32_t> qd, itm, cnt; DevBuf<uint32_t> cm; DevBuf<double> Pd, outd, rep; DevBuf<uint8_t> alw; DevBuf<int8_t> st;
    DevBuf<unsigned long long> acc; DevBuf<int> counter;
    const size_t nq3 = (size_t)Q * (1 + (q_mult ? 1 : 0) + (q_group ? 1 : 0));
    MMM_HIP(ctx, qp.alloc((size_t)D + 1)); MMM_HIP(ctx, qd.alloc(nq3)); MMM_HIP(ctx, itm.alloc(queried.size())); MMM_HIP(ctx, cm.alloc((size_t)nnz));
    MMM_HIP(ctx, Pd.alloc(P.size())); MMM_HIP(ctx, outd.alloc(DC + QC)); MMM_HIP(ctx, st.alloc((size_t)D)); MMM_HIP(ctx, counter.alloc(1));
    MMM_HIP(ctx, acc.alloc((size_t)D + (B ? 2 * QC + BGC : 0))); MMM_HIP(ctx, cnt.alloc(B ? QC + (size_t)Q : 0));
    if (allowed) MMM_HIP(ctx, alw.alloc(DC));
    if (int rc = csr.upload(ctx, D, doc_ptr, term, count)) return rc;
    MMM_HIP(ctx, hipMemcpyAsync(qp.p, q_ptr, sizeof(int64_t) * ((size_t)D + 1), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(qd.p, q_term, sizeof(int32_t) * (size_t)Q, hipMemcpyHostToDevice, ctx->stream));
    int32_t* const qm = q_mult ? qd.p + Q : nullptr;
    int32_t* const qg = q_group ? qd.p + (size_t)Q * (q_mult ? 2 : 1) : nullptr;
    if (q_mult) MMM_HIP(ctx, hipMemcpyAsync(qm, q_mult, sizeof(int32_t) * (size_t)Q, hipMemcpyHostToDevice, ctx->stream));
    if (q_group) MMM_HIP(ctx, hipMemcpyAsync(qg, q_group, sizeof(int32_t) * (size_t)Q, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(itm.p, queried.data(), sizeof(int32_t) * queried.size(), hipMemcpyHostToDevice, ctx->stream));
    if (nnz) MMM_HIP(ctx, hipMemcpyAsync(cm.p, cum.data(), sizeof(uint32_t) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(Pd.p, P.data(), sizeof(double) * P.size(), hipMemcpyHostToDevice, ctx->stream));
    if (allowed) MMM_HIP(ctx, hipMemcpyAsync(alw.p, allowed, DC, hipMemcpyHostToDevice, ctx->stream));
    // what a document that is not processed, a signature outside A_d and a query without mass leave behind; a queried document starts with
    // status 0 and the observed phase marks the ones it cannot fit
    std::vector<int8_t> st0((size_t)D, 4);
    for (int32_t d : queried) st0[(size_t)d] = 0;
    MMM_HIP(ctx, hipMemcpyAsync(st.p, st0.data(), (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(outd.p, 0, sizeof(double) * outd.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(acc.p, 0, sizeof(unsigned long long) * acc.n, ctx->stream));
    if (cnt.n) MMM_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * cnt.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));

    AtArgs a{};
    a.D = D; a.C = C; a.V = V; a.Cp = Cp; a.G = G; a.maxiter = maxiter; a.tol = tol; a.Q = (long long)Q;
    a.doc_ptr = csr.ptr; a.term = csr.term; a.count = csr.count; a.P = Pd.p; a.allowed = allowed ? alw.p : nullptr;
    a.q_ptr = qp.p; a.q_term = qd.p; a.q_mult = qm; a.q_group = groups ? qg : nullptr;
    a.items = itm.p; a.n_items = (int)queried.size();
    a.w = outd.p; a.post = outd.p + DC; a.status = st.p; a.iters = acc.p; a.counter = counter.p; a.wave_doubles = wd;
    a.cum = cm.p; a.B = B; a.b0 = (uint32_t)b0; a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.sum_fx = acc.p + D; a.sumsq_fx = a.sum_fx + QC; a.group_fx = a.sumsq_fx + QC; a.top_count = cnt.p; a.void_count = cnt.p + QC;

    // ---- observed phase: as many waves per block as their buffers leave room for; few documents: fewer, so that they spread over the CUs
    {
        int nw = kAtMaxWaves;
        while (nw > 1 && nw * pw > kAtLdsBlock) nw >>= 1;
        while (nw > 1 && ((int64_t)queried.size() + nw - 1) / nw < cus) nw >>= 1;
        const size_t lds = nw * pw;
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(kAtMaxWaves / nw, (int64_t)(kAtLdsBlock / lds)));
        const unsigned grid = (unsigned)std::min<int64_t>(((int64_t)queried.size() + nw - 1) / nw, (int64_t)cus * per_cu);
        if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)k_attribute_obs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_attribute_obs, dim3(grid), dim3(64 * nw), lds, ctx->stream, a);
        MMM_LAUNCH_CHECK(ctx);
    }
    std::vector<int8_t> hst((size_t)D);
    MMM_HIP(ctx, hipMemcpyAsync(hst.data(), st.p, (size_t)D, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));

    // ---- replicate phase: the documents of status 0, those whose rows fit LDS first
    if (B > 0) {
        std::vector<int32_t> docs;
        int max_n = 0;
        int64_t max_w = 1, max_q = 1;
        std::vector<int> nact((size_t)D, 0);
        for (int32_t d : queried) {
            if (hst[(size_t)d] != 0) continue;
            int n = C;
            if (allowed) { n = 0; for (int c = 0; c < C; ++c) n += allowed[(size_t)d * C + c] != 0; }
            nact[(size_t)d] = n; max_n = std::max(max_n, n);
            max_w = std::max(max_w, doc_ptr[d + 1] - doc_ptr[d]);
            max_q = std::max(max_q, q_ptr[d + 1] - q_ptr[d]);
            docs.push_back(d);
        }
        if (!docs.empty()) {
            a.P2c = at_pow2(max_w); a.Wl = (int)max_w; a.Ql = (int)std::min<int64_t>(max_q, kAtMaxQLds);
            const size_t fixed_words = ((size_t)a.P2c + a.Wl + a.Ql + Cp + 3) & ~(size_t)3;
            const size_t fixed = sizeof(uint32_t) * fixed_words;
            a.fixed_doubles = (int)(fixed_words / 2);
            int nw = 1;
            for (int t = kAtMaxWaves; t >= 1; t >>= 1)
                if (fixed + t * pw <= kAtLdsBlock) { nw = t; break; }
            // rows of P a block can stage beside nw waves' buffers (one double may pad the rows to 16 bytes)
            auto cap = [&](int t) { const size_t room = (kAtLdsBlock - fixed - t * pw) / sizeof(double); return room ? (int)((room - 1) / (size_t)V) : 0; };
            int rows_cap = 0;
            if (!mmm_off(ctx->tune, MMM_OFF_REFIT_LDS)) {
                if (nw == kAtMaxWaves && cap(nw) < max_n && cap(nw / 2) >= max_n) nw >>= 1;       // four waves with every document's rows in LDS beat eight through L2
                rows_cap = cap(nw);
            }
            std::vector<int32_t> all, direct;
            int rows = 0;
            for (int32_t d : docs) {
                if (nact[(size_t)d] <= rows_cap) { all.push_back(d); rows = std::max(rows, nact[(size_t)d]); }
                else direct.push_back(d);
            }
            const size_t n_staged = all.size();
            all.insert(all.end(), direct.begin(), direct.end());
            MMM_HIP(ctx, itm.alloc(all.size()));
            MMM_HIP(ctx, hipMemcpyAsync(itm.p, all.data(), sizeof(int32_t) * all.size(), hipMemcpyHostToDevice, ctx->stream));
            if (want_rep) {
                MMM_HIP(ctx, rep.alloc((size_t)B * QC));
                MMM_HIP(ctx, hipMemsetAsync(rep.p, 0, sizeof(double) * (size_t)B * QC, ctx->stream));
            }
            a.rep_post = want_rep ? rep.p : nullptr;
            ProfSpan span(ctx);
            for (int part = 0; part < 2; ++part) {
                const size_t n = part ? all.size() - n_staged : n_staged;
                if (!n) continue;
                const int rpb = at_reps_per_block(nw, B, n, cus);
                a.items = itm.p + (part ? n_staged : 0);
                a.n_items = (int)n;
                a.reps_per_block = rpb;
                a.stage_doubles = part ? 0 : (int)(((size_t)rows * V + 1) & ~(size_t)1);
                const size_t lds = fixed + sizeof(double) * (size_t)a.stage_doubles + nw * pw;
                auto kern = part ? k_attribute_rep<false> : k_attribute_rep<true>;
                if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(kern, dim3((unsigned)n, (unsigned)((B + rpb - 1) / rpb)), dim3(64 * nw), lds, ctx->stream, a);
                MMM_LAUNCH_CHECK(ctx);
            }
        }
    }
    // staged on the host so that a failing copy leaves the caller's arrays as they were
    std::vector<double> ho(DC + QC), hr(want_rep && rep.p ? (size_t)B * QC : 0);
    std::vector<unsigned long long> ha(acc.n);
    std::vector<int32_t> hc(cnt.n);
    MMM_HIP(ctx, hipMemcpyAsync(ho.data(), outd.p, sizeof(double) * ho.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(ha.data(), acc.p, sizeof(unsigned long long) * ha.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (hc.size()) MMM_HIP(ctx, hipMemcpyAsync(hc.data(), cnt.p, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (hr.size()) MMM_HIP(ctx, hipMemcpyAsync(hr.data(), rep.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(w, ho.data(), sizeof(double) * DC);
    memcpy(post, ho.data() + DC, sizeof(double) * QC);
    memcpy(status, hst.data(), (size_t)D);
    for (int d = 0; d < D; ++d) iters[d] = (int64_t)ha[(size_t)d];
    if (B > 0) {
        memcpy(sum_fx, ha.data() + D, sizeof(uint64_t) * QC);
        memcpy(sumsq_fx, ha.data() + D + QC, sizeof(uint64_t) * QC);
        if (BGC) memcpy(group_fx, ha.data() + D + 2 * QC, sizeof(uint64_t) * BGC);
        memcpy(top_count, hc.data(), sizeof(int32_t) * QC);
        memcpy(void_count, hc.data() + QC, sizeof(int32_t) * (size_t)Q);
        if (want_rep) {
            if (hr.size()) memcpy(rep_post, hr.data(), sizeof(double) * hr.size());
            else memset(rep_post, 0, sizeof(double) * (size_t)B * QC);
        }
    }
    return MMM_OK;
}
