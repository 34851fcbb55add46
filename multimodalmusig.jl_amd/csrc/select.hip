// select.hip -- the two pieces of choosing the number of signatures by held-out mutations that have no counterpart in the reference:
//   mmm_split_counts      every document's mutations dealt into F folds (Philox4x32-10 counters, one word per mutation, integer throughout)
//   mmm_mixture_score     per-document log-likelihood and reconstruction cosine of a corpus under given exposures and signatures
// and mmm_score_tables, the same score on R replicas' tables where they lie (the handle entry mmm_lda_score_replicas of lda.hip).  The fits
// between the two are the existing restart batches; the definitions the kernels restate are in include/mmmusig.h and DESIGN.md section
// 4.12.  Integer arithmetic or fixed-order double sums: the same arguments give the same bits on every run and every launch geometry.
#include "mmm_internal.h"
#include "dev_math.h"
#include "mmm_arith.h"
#include "mmm_philox.h"

namespace {

// ---- split -----------------------------------------------------------------------------------------------------------------------------------
constexpr int kSpWaves = 4;                 // waves per block; the block takes one document
constexpr int kSpThreads = 64 * kSpWaves;
constexpr int kSpMaxWords = 10240;          // LDS words a row may take: prefix sums padded to a power of two + F histograms = 40 KiB at most,
                                            // the budget of the resampler (bootstrap.hip)
constexpr int kSpMaxF = 64;

// grid D.  Mutation i of document d (CSR order) lies in the first entry e with cum[e] > i and goes to fold (u_i F) >> 32, u_i = word i % 4 of the
// block (i / 4, d, rep, stream).  out[f * nnz + e].  Rows of at most lds_w entries: prefix sums in LDS, padded with 0xffffffff to lds_p' = a
// power of two >= W so that the search is the same log2 steps for every lane without bound checks (rs_draw_row_lds), one [F][W] integer
// histogram for the block (ds_add_u32: integer adds commute), rows out with plain stores.  Longer rows: bisection over the global prefix sums
// and integer atomics into `out`, which the host has zeroed.
__global__ __launch_bounds__(kSpThreads) void k_split_counts(const int64_t* __restrict__ doc_ptr, const uint32_t* __restrict__ cum, int64_t nnz, int F, uint32_t rep,
                                                             uint32_t stream, uint32_t k0, uint32_t k1, int lds_w, int lds_p, int32_t* __restrict__ out)
{
    extern __shared__ uint32_t s_dyn[];                        // [lds_p] prefix sums, then [F][W] counts
    uint32_t* s_cum = s_dyn;
    int* s_hist = (int*)(s_dyn + lds_p);
    const int tid = threadIdx.x;
    const uint32_t d = blockIdx.x;
    const int64_t e0 = doc_ptr[d];
    const int W = (int)(doc_ptr[d + 1] - e0);
    if (W == 0) return;
    const uint32_t* cg = cum + e0;
    const uint32_t N = cg[W - 1];                              // N < 2^31
    const uint32_t nblk = (N + 3u) >> 2;
    if (W <= lds_w) {
        int half = 1;                                          // 2 * half: the power of two the row is padded to
        while (2 * half < W) half <<= 1;
        if (W == 1) half = 0;
        for (int e = tid; e < 2 * half || e < W; e += kSpThreads) s_cum[e] = e < W ? cg[e] : 0xffffffffu;
        for (int i = tid; i < F * W; i += kSpThreads) s_hist[i] = 0;
        __syncthreads();
        for (uint32_t i4 = (uint32_t)tid; i4 < nblk; i4 += (uint32_t)kSpThreads) {
            uint32_t u[4];
            int pos[4];
            philox4x32_10(i4, d, rep, stream, k0, k1, u);
#pragma unroll
            for (int j = 0; j < 4; ++j) pos[j] = 0;
            for (int step = half; step > 0; step >>= 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (s_cum[pos[j] + step - 1] <= 4u * i4 + (uint32_t)j) pos[j] += step;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4u * i4 + (uint32_t)j < N) atomicAdd(&s_hist[(int)__umulhi(u[j], (uint32_t)F) * W + pos[j]], 1);      // i < N = cum[W-1]: pos <= W - 1
        }
        __syncthreads();
        for (int i = tid; i < F * W; i += kSpThreads) {
            const int f = i / W, e = i - f * W;
            out[(size_t)f * (size_t)nnz + e0 + e] = s_hist[i];
        }
    } else {
        for (uint32_t i4 = (uint32_t)tid; i4 < nblk; i4 += (uint32_t)kSpThreads) {
            uint32_t u[4];
            philox4x32_10(i4, d, rep, stream, k0, k1, u);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t i = 4u * i4 + (uint32_t)j;
                if (i >= N) break;
                int lo = 0, hi = W - 1;                        // first e with cum[e] > i; cum[W-1] = N > i, so it exists
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (cg[mid] > i) hi = mid; else lo = mid + 1;
                }
                atomicAdd(&out[(size_t)__umulhi(u[j], (uint32_t)F) * (size_t)nnz + e0 + lo], 1);
            }
        }
    }
}

// ---- score -----------------------------------------------------------------------------------------------------------------------------------
constexpr int kScWaves = 4;
constexpr size_t kScPhiLds = 64 * 1024;     // a replica's [k V + v] table is staged in LDS up to this size, read through L2 beyond

// grid (ceil(D / 4), R), one wave per (document, replica).  tabs[r]: replica r's K x D table, tabs[R + r]: its [k V + v] table.  FROM_GAMMA: the
// K x D table is gamma and the proportions are gamma / sum gamma by the expressions of k_lda_loglik / k_lda_loglik_big (lane partials over
// k = lane, lane + 64, ..., wave_sum, one division each).  With p_v = sum_k props[k] phi[k V + v] (k ascending, product and sum rounded
// separately):  ll = sum_e n_e log p_ve and N = sum_e n_e exactly as k_free_loglik_docs forms them;  cos = (sum_e n_e p_ve) / (sqrt(sum_e n_e^2)
// sqrt(sum_v p_v^2)), every sum as lane partials over the indices lane, lane + 64, ... ascending, then wave_sum; 0 when a norm is 0.
// Dynamic LDS: [phi_lds ? K V : 0] table, then kScWaves rows of K proportions.  out: ll | N | cos, each [R][D].
template <bool FROM_GAMMA>
__global__ __launch_bounds__(64 * kScWaves) void k_mixture_score(int D, int K, int V, const int64_t* __restrict__ doc_ptr, const int32_t* __restrict__ term,
                                                                 const int32_t* __restrict__ count, const double* const* __restrict__ tabs, int phi_lds,
                                                                 double* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double s_sc[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = gridDim.y, r = blockIdx.y;
    const double* __restrict__ pd = tabs[r];
    const double* __restrict__ phig = tabs[R + r];
    double* s_p = s_sc + (phi_lds ? (size_t)K * V : 0) + (size_t)wave * K;
    const int d = blockIdx.x * kScWaves + wave;
    if (phi_lds)
        for (int i = tid; i < K * V; i += 64 * kScWaves) s_sc[i] = phig[i];
    if (d < D) {
        if (FROM_GAMMA) {
            double gs = 0.0;
            for (int k = lane; k < K; k += 64) gs += pd[(size_t)d * K + k];
            const double S = wave_sum(gs);
            for (int k = lane; k < K; k += 64) s_p[k] = pd[(size_t)d * K + k] / S;
        } else {
            for (int k = lane; k < K; k += 64) s_p[k] = pd[(size_t)d * K + k];
        }
    }
    __syncthreads();
    if (d >= D) return;
    const double* phi = phi_lds ? s_sc : phig;
    double s = 0.0, N = 0.0, num = 0.0, nn = 0.0, pp = 0.0;
    for (int64_t e = doc_ptr[d] + lane; e < doc_ptr[d + 1]; e += 64) {
        const int v = term[e];
        const double n = (double)count[e];
        double pw = 0.0;
        for (int k = 0; k < K; ++k) pw += s_p[k] * phi[(size_t)k * V + v];
        s += n * ar_log(pw);
        N += n;
        num += n * pw;
        nn += n * n;
    }
    for (int v = lane; v < V; v += 64) {
        double pw = 0.0;
        for (int k = 0; k < K; ++k) pw += s_p[k] * phi[(size_t)k * V + v];
        pp += pw * pw;
    }
    s = wave_sum(s); N = wave_sum(N); num = wave_sum(num); nn = wave_sum(nn); pp = wave_sum(pp);
    if (lane == 0) {
        const size_t RD = (size_t)R * D, i = (size_t)r * D + d;
        out[i] = s; out[RD + i] = N;
        out[2 * RD + i] = (nn > 0.0 && pp > 0.0) ? num / (sqrt(nn) * sqrt(pp)) : 0.0;
    }
}

// grid R.  Over the documents with N_d > 0 of replica r: total[0] = sum ll / sum N, [1] = sum ll, [2] = sum N -- the sums and the tree of
// k_free_loglik_total --, [3] = the mean of cos by the same 256 strided partial sums and tree.
__global__ __launch_bounds__(256) void k_score_total(int D, const double* __restrict__ docs, double* __restrict__ total)
{
    __shared__ double sh[4][256];
    const int R = gridDim.x, r = blockIdx.x;
    const size_t RD = (size_t)R * D;
    const double* docsum = docs + (size_t)r * D;
    const double* docN = docsum + RD;
    const double* doccos = docsum + 2 * RD;
    double a = 0.0, b = 0.0, c = 0.0, n = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) if (docN[d] > 0.0) { a += docsum[d]; b += docN[d]; c += doccos[d]; n += 1.0; }
    sh[0][threadIdx.x] = a; sh[1][threadIdx.x] = b; sh[2][threadIdx.x] = c; sh[3][threadIdx.x] = n;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = total + 4 * (size_t)r;
        o[0] = sh[0][0] / sh[1][0]; o[1] = sh[0][0]; o[2] = sh[1][0]; o[3] = sh[2][0] / sh[3][0];
    }
}

} // namespace

int mmm_score_tables(mmm_ctx* ctx, const char* who, int R, int D, int K, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count,
                     const double* const* h_prop, const double* const* h_phi, bool from_gamma, double* total, double* ll_doc, double* n_doc, double* cos_doc)
{
    MMM_CHECK(ctx, R >= 1 && R <= 65535 && K >= 1 && V >= 1 && total, "%s: R = %d replicas (1..65535), K < 1, V < 1 or total == NULL", who, R);
    if (int rc = mmm_check_csr(ctx, who, D, V, doc_ptr, term, count)) return rc;
    const int64_t nnz = doc_ptr[D];
    // one upload: doc_ptr | the 2 R table pointers | term | count
    const size_t n8 = (size_t)D + 1 + 2 * (size_t)R, bytes = 8 * n8 + 8 * (size_t)nnz;
    std::vector<int64_t> h(n8 + (size_t)nnz);
    memcpy(h.data(), doc_ptr, 8 * ((size_t)D + 1));
    for (int r = 0; r < R; ++r) {
        memcpy(&h[(size_t)D + 1 + r], &h_prop[r], 8);
        memcpy(&h[(size_t)D + 1 + R + r], &h_phi[r], 8);
    }
    if (nnz) {
        memcpy((char*)h.data() + 8 * n8, term, 4 * (size_t)nnz);
        memcpy((char*)h.data() + 8 * n8 + 4 * (size_t)nnz, count, 4 * (size_t)nnz);
    }
    DevBuf<int64_t> in; DevBuf<double> out;
    const size_t RD = (size_t)R * D, nout = 4 * (size_t)R + 3 * RD;
    MMM_HIP(ctx, in.alloc(h.size())); MMM_HIP(ctx, out.alloc(nout));
    MMM_HIP(ctx, hipMemcpyAsync(in.p, h.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    const double* const* tabs = (const double* const*)(in.p + D + 1);
    const int32_t* t = (const int32_t*)(in.p + n8);
    const int32_t* c = t + nnz;
    const size_t tab_bytes = sizeof(double) * (size_t)K * V;
    const int phi_lds = tab_bytes <= kScPhiLds ? 1 : 0;
    const size_t lds = (phi_lds ? tab_bytes : 0) + sizeof(double) * kScWaves * (size_t)K;
    if (lds > 96 * 1024) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: K = %d proportions per wave do not fit LDS", who, K);
    double* docs = out.p + 4 * (size_t)R;
    if (D) {
        auto kern = from_gamma ? k_mixture_score<true> : k_mixture_score<false>;
        if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)((D + kScWaves - 1) / kScWaves), (unsigned)R), dim3(64 * kScWaves), lds, ctx->stream, D, K, V, in.p, t, c, tabs,
                           phi_lds, docs);
    }
    hipLaunchKernelGGL(k_score_total, dim3((unsigned)R), dim3(256), 0, ctx->stream, D, docs, out.p);
    MMM_LAUNCH_CHECK(ctx);
    std::vector<double> ho(nout);
    MMM_HIP(ctx, hipMemcpyAsync(ho.data(), out.p, sizeof(double) * nout, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(total, ho.data(), sizeof(double) * 4 * (size_t)R);
    const double* hd = ho.data() + 4 * (size_t)R;
    if (ll_doc && RD) memcpy(ll_doc, hd, sizeof(double) * RD);
    if (n_doc && RD) memcpy(n_doc, hd + RD, sizeof(double) * RD);
    if (cos_doc && RD) memcpy(cos_doc, hd + 2 * RD, sizeof(double) * RD);
    return MMM_OK;
}

extern "C" {

int mmm_split_counts(mmm_ctx* ctx, int D, const int64_t* doc_ptr, const int32_t* count, int F, int rep, uint64_t seed, uint32_t stream, int32_t* out)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, D >= 0 && doc_ptr && rep >= 0, "mmm_split_counts: D < 0, doc_ptr == NULL or rep < 0");
    MMM_CHECK(ctx, F >= 1 && F <= kSpMaxF, "mmm_split_counts: F = %d folds (1..%d)", F, kSpMaxF);
    MMM_CHECK(ctx, stream < 0x80000000u, "mmm_split_counts: stream = %u (below 2^31: the high bit of that counter word marks a split)", stream);
    MMM_CHECK(ctx, doc_ptr[0] == 0, "mmm_split_counts: doc_ptr[0] != 0");
    for (int d = 0; d < D; ++d) MMM_CHECK(ctx, doc_ptr[d + 1] >= doc_ptr[d], "mmm_split_counts: doc_ptr decreases at document %d", d);
    const int64_t nnz = doc_ptr[D];
    MMM_CHECK(ctx, nnz == 0 || count, "mmm_split_counts: count == NULL");
    // inclusive prefix sums per document (what a mutation's index is searched in)
    std::vector<uint32_t> cum((size_t)nnz);
    bool any_long = false;
    int64_t lds_w = 1;                                            // longest row that stays in LDS: p2(W) + F W <= kSpMaxWords, monotone in W
    for (int d = 0; d < D; ++d) {
        const int64_t w = doc_ptr[d + 1] - doc_ptr[d];
        if (w >= ((int64_t)1 << 31)) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_split_counts: document %d has %lld entries (limit 2^31 - 1)", d, (long long)w);
        int64_t p = 1;
        while (p < w) p <<= 1;
        const bool fits = p + (int64_t)F * w <= kSpMaxWords;
        any_long |= !fits;
        if (fits) lds_w = std::max(lds_w, w);
        uint64_t s = 0;
        for (int64_t e = doc_ptr[d]; e < doc_ptr[d + 1]; ++e) {
            MMM_CHECK(ctx, count[e] >= 0, "mmm_split_counts: entry %lld has count %d", (long long)e, count[e]);
            s += (uint64_t)count[e];
            if (s >= ((uint64_t)1 << 31))
                return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_split_counts: document %d holds 2^31 or more counts (a mutation's index is a 32-bit word)", d);
            cum[(size_t)e] = (uint32_t)s;
        }
    }
    if (nnz == 0) return MMM_OK;
    MMM_CHECK(ctx, out, "mmm_split_counts: out == NULL");
    int64_t lds_p = 1;
    while (lds_p < lds_w) lds_p <<= 1;
    DevBuf<int64_t> dp; DevBuf<uint32_t> cm; DevBuf<int32_t> o;
    const size_t bytes = sizeof(int32_t) * (size_t)F * (size_t)nnz;
    MMM_HIP(ctx, dp.alloc((size_t)D + 1)); MMM_HIP(ctx, cm.alloc((size_t)nnz)); MMM_HIP(ctx, o.alloc((size_t)F * (size_t)nnz));
    MMM_HIP(ctx, hipMemcpyAsync(dp.p, doc_ptr, sizeof(int64_t) * ((size_t)D + 1), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(cm.p, cum.data(), sizeof(uint32_t) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
    if (any_long) MMM_HIP(ctx, hipMemsetAsync(o.p, 0, bytes, ctx->stream));
    hipLaunchKernelGGL(k_split_counts, dim3((unsigned)D), dim3(kSpThreads), sizeof(uint32_t) * (size_t)(lds_p + (int64_t)F * lds_w), ctx->stream, dp.p, cm.p, nnz, F,
                       (uint32_t)rep, 0x80000000u | stream, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (int)lds_w, (int)lds_p, o.p);
    MMM_LAUNCH_CHECK(ctx);
    MMM_HIP(ctx, hipMemcpyAsync(out, o.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MMM_OK;
}

int mmm_mixture_score(mmm_ctx* ctx, int D, int K, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* props,
                      const double* phi, double* ll_doc, double* n_doc, double* cos_doc, double* total)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, K >= 1 && V >= 1 && D >= 0 && (D == 0 || props) && phi && total, "mmm_mixture_score: NULL argument, D < 0, K < 1 or V < 1");
    DevBuf<double> p, f;
    MMM_HIP(ctx, p.alloc((size_t)K * D)); MMM_HIP(ctx, f.alloc((size_t)K * V));
    if (D) MMM_HIP(ctx, hipMemcpyAsync(p.p, props, sizeof(double) * K * D, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(f.p, phi, sizeof(double) * K * V, hipMemcpyHostToDevice, ctx->stream));
    const double* hp = p.p; const double* hf = f.p;
    return mmm_score_tables(ctx, "mmm_mixture_score", 1, D, K, V, doc_ptr, term, count, &hp, &hf, false, total, ll_doc, n_doc, cos_doc);
}

} // extern "C"
