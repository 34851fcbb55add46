// trajectory.hip -- mmm_exposure_trajectory: where along a tumour's ordered mutations do the exposures change, how many times, and is that
// more than chance?  A sample is a timeline of T bins.  The segment table holds ll of fit(A) on every run of bins i .. j - 1; optimal
// partitioning over the table picks the change points; the best single cut is tested by the exact permutation of mmm_compare_exposures,
// dealt once per replicate for ALL cuts (no counterpart in the reference; include/mmmusig.h has the normative definition, DESIGN.md
// section 4.24 the reasoning).
//
// Four steps on the context's stream.  "Prefix": the cumulative count vectors c^t, u32 [T + 1][V] per sample, in global memory, built once.
// "Table": the items (sample, i, j) behind a work counter, one wave an item: x = c^j - c^i in the wave's LDS, fit, ll.  The table comes
// back to the host, which runs the dynamic program and the scan (O(M T^2) additions a sample).  "Weights": the same kernel on the few
// chosen segments and on the single bins, weights out (every fit is a cold start, so a refit gives the table's bits).  "Replicates": grid
// (sample, replicate chunk), the block prologue of k_compare_rep; a wave takes one replicate at a time and walks its cuts: select, deal
// the prefix into its LDS histogram, fit, turn the histogram into pooled - prefix in place, fit again, keep the running maximum.  The
// replicate's counts never leave LDS.  fit(A) is mixture_fit.cuh's, the dealing deal_select.cuh's.
#include "mmm_internal.h"
#include "dev_math.h"
#include "mmm_philox.h"
#include "mixture_fit.cuh"
#include "deal_select.cuh"

#include <cmath>
#include <limits>

namespace {

constexpr int kTjMaxC = 256;
constexpr int kTjMaxV = 4096;                   // the pooled vector, its prefix sums and a wave's buffers stay in LDS
constexpr int kTjMaxBins = MMM_TRAJECTORY_MAX_BINS;               // T_d: a block keeps a value per cut in LDS; the table holds T (T + 1) / 2 fits
constexpr int kTjMaxWaves = 8;
constexpr size_t kTjLdsBlock = 160 * 1024;

struct TjArgs {
    int D, C, V, Cp, maxiter, key_bits;
    double tol;
    const uint32_t* pre;             // [rows][V]: the prefix vectors, sample d's row t at row0[d] + t (t = 0 .. T_d)
    const uint32_t* ctot;            // [rows]: their totals C_t
    const int64_t* row0;             // [D]
    const int32_t* nT;               // [D]
    const double* P;                 // [C][V], rows normalised
    const uint8_t* allowed;          // [D][C] or NULL
    // fit launch (table, weights)
    const int32_t* item_dij;         // [n_items][4]: d, i, j, own (1: the fit's iterations and u_0T are the sample's)
    const int64_t* item_out;         // [n_items][2]: the place of ll in seg_ll or -1, the row of wout or -1
    int n_items;
    int* counter;
    double* seg_ll; double* wout;    // wout [.][C], zeroed by the host
    double* unexplained;
    unsigned long long* iters;
    // replicate launch
    const int32_t* items;            // the tested samples this launch takes
    int L, B, reps_per_block, P2, wave_doubles, stage_doubles;
    uint32_t b0, k0, k1, stream;
    const double* g_obs;             // [rows]: G_t at row0[d] + t for the cuts t
    const double* g_max; const double* ll0;     // [D]
    int32_t* count_ge;               // [D]
    int32_t* count_cut;              // [rows], like g_obs
    double* rep;                     // [B][D] or NULL
};

// fit launch, a wave's own LDS: the weights, the list, f_v, r_v and the count vector
__host__ __device__ inline int tj_fit_doubles(int Cp, int V) { return (Cp + Cp / 2 + 2 * V + (V + 1) / 2 + 1) & ~1; }
// replicate launch, a wave's own LDS: the weights, the list, a counter per cut, f_v, r_v, the count vector, the bins
__host__ __device__ inline int tj_rep_doubles(int Cp, int V) { return (Cp + Cp / 2 + kTjMaxBins / 2 + 2 * V + (V + 1) / 2 + kDealBins / 2 + 1) & ~1; }
// replicate launch, the block's LDS before the staged rows: cum [P2] | pooled [V, even] | C_t [kTjMaxBins + 2] | G_t [kTjMaxBins]
__host__ __device__ inline size_t tj_rep_fixed(int P2, int V) { return sizeof(uint32_t) * (size_t)P2 + sizeof(double) * ((size_t)((V + 1) / 2) + (kTjMaxBins + 2) / 2 + kTjMaxBins); }

// ---- prefix vectors ----------------------------------------------------------------------------------------------------------------------------
// one block per bin: its entries added into the row after its own (pre is zeroed; duplicate terms sum)
__global__ __launch_bounds__(64) void k_traj_scatter(const int64_t* __restrict__ ptr, const int32_t* __restrict__ term, const int32_t* __restrict__ count,
                                                     const int64_t* __restrict__ bin_row, int V, uint32_t* __restrict__ pre)
{
    const int64_t bin = blockIdx.x;
    uint32_t* row = pre + (size_t)bin_row[bin] * V;
    for (int64_t e = ptr[bin] + threadIdx.x; e < ptr[bin + 1]; e += 64) {
        const int cnt = count[e];
        if (cnt > 0) atomicAdd(&row[term[e]], (uint32_t)cnt);
    }
}

// grid (D, chunks of 256 terms): row t <- row t + row t - 1, t ascending (integers)
__global__ __launch_bounds__(256) void k_traj_cumulate(const int64_t* __restrict__ row0, const int32_t* __restrict__ nT, int V, uint32_t* __restrict__ pre)
{
    const int d = blockIdx.x, v = (int)(blockIdx.y * 256 + threadIdx.x);
    if (v >= V) return;
    uint32_t* p = pre + (size_t)row0[d] * V + v;
    uint32_t run = 0u;
    for (int t = 1; t <= nT[d]; ++t) {
        run += p[(size_t)t * V];
        p[(size_t)t * V] = run;
    }
}

// ---- table and weights -------------------------------------------------------------------------------------------------------------------------
// One wave an item.  Dynamic LDS: per wave tj_fit_doubles doubles; the catalogue is read through L2 (the table is a B-th of the call's work).
__global__ __launch_bounds__(64 * kTjMaxWaves) void k_traj_fit(const TjArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_tj[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.C, V = a.V, Cp = a.Cp;
    double* base = s_tj + (size_t)wave * a.wave_doubles;
    double* w = base;
    int* act = (int*)(base + Cp);
    double* fb = base + Cp + Cp / 2;
    double* rb = fb + V;
    uint32_t* h = (uint32_t*)(rb + V);
    const double* __restrict__ P = a.P;
    for (;;) {
        const int it = rf_next_item(a.counter, lane);          // its contract shapes this loop: one body, one closing fence
        if (it >= a.n_items) break;
        const int d = a.item_dij[4 * it], i = a.item_dij[4 * it + 1], j = a.item_dij[4 * it + 2], own = a.item_dij[4 * it + 3];
        const int64_t o_ll = a.item_out[2 * it], o_w = a.item_out[2 * it + 1];
        const size_t r0 = (size_t)a.row0[d];
        const uint32_t* ci = a.pre + (r0 + i) * V;
        const uint32_t* cj = a.pre + (r0 + j) * V;
        const uint32_t Nx = a.ctot[r0 + j] - a.ctot[r0 + i];
        for (int v = lane; v < V; v += 64) {
            const uint32_t x = cj[v] - ci[v];
            h[v] = x;
            fb[v] = Nx ? (double)x / (double)Nx : 0.0;
        }
        int pos;
        const int n = rf_active_list(a.allowed ? a.allowed + (size_t)d * C : nullptr, C, -1, act, lane, pos);
        rf_pad_list(act, n, lane);
        rf_wave_sync();
        const RfCountsU32 counts{h};
        double ll = 0.0, u = 0.0;
        int its = 0;
        if (Nx) {                                              // an empty segment: w = 0, ll = 0, no iteration
            its = rf_fit(P, act, w, n, fb, counts, rb, V, lane, a.maxiter, a.tol);
            const RfLoglik R = rf_loglik<false>(P, act, w, n, counts, fb, -1, V, lane);
            ll = R.ll; u = R.u;
            if (o_w >= 0)
                for (int k = lane; k < n; k += 64) a.wout[(size_t)o_w * C + act[k]] = w[k];
        }
        if (lane == 0) {
            if (o_ll >= 0) a.seg_ll[o_ll] = ll;
            if (own) {
                if (its) atomicAdd(&a.iters[d], (unsigned long long)its);
                if (i == 0 && j == a.nT[d]) a.unexplained[d] = u;
            }
        }
        rf_wave_sync();
    }
}

// ---- replicates --------------------------------------------------------------------------------------------------------------------------------
// grid (items, replicate chunks), blockDim 64 nw.  Dynamic LDS: tj_rep_fixed | P_LDS: the rows of A at stride V | per wave tj_rep_doubles.
template <bool P_LDS>
__global__ __launch_bounds__(64 * kTjMaxWaves) void k_traj_rep(const TjArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_tj[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6), nt = (int)blockDim.x;
    const int C = a.C, V = a.V, Cp = a.Cp, P2 = a.P2, Vh = (V + 1) / 2;
    const int d = a.items[blockIdx.x];
    const size_t r0 = (size_t)a.row0[d];
    const int T = a.nT[d], L = a.L;                            // T <= kTjMaxBins, 2 L <= T (the host lists tested samples only)
    uint32_t* s_cum = (uint32_t*)s_tj;
    uint32_t* s_pool = s_cum + P2;                             // P2 >= 2: 8-byte steps
    uint32_t* s_ct = s_pool + 2 * Vh;
    double* s_g = s_tj + P2 / 2 + Vh + (kTjMaxBins + 2) / 2;
    double* s_stage = s_g + kTjMaxBins;
    double* base = s_stage + (P_LDS ? a.stage_doubles : 0) + (size_t)wave * a.wave_doubles;
    double* w = base;
    int* act = (int*)(base + Cp);
    int* ccut = act + Cp;
    double* fb = base + Cp + Cp / 2 + kTjMaxBins / 2;
    double* rb = fb + V;
    uint32_t* hist = (uint32_t*)(rb + V);
    uint32_t* bins = hist + 2 * Vh;
    // every wave builds the list for itself (the same bits): no wave waits for another after the set-up
    int pos;
    const int n = rf_active_list(a.allowed ? a.allowed + (size_t)d * C : nullptr, C, -1, act, lane, pos);
    rf_pad_list(act, n, lane);
    const uint32_t* pooled = a.pre + (r0 + (size_t)T) * V;
    for (int v = tid; v < 2 * Vh; v += nt) s_pool[v] = v < V ? pooled[v] : 0u;
    for (int t = tid; t <= T; t += nt) s_ct[t] = a.ctot[r0 + t];
    for (int t = tid; t < T; t += nt) s_g[t] = a.g_obs[r0 + t];
    if (P_LDS) {
        for (int i = wave; i < n; i += nw) {
            const double* src = a.P + (size_t)act[i] * V;
            for (int v = lane; v < V; v += 64) s_stage[(size_t)i * V + v] = src[v];
        }
    }
    __syncthreads();                                           // the pooled vector, the cuts and the staged rows are there; act has been read
    if (P_LDS)
        for (int i = lane; i < ((n + 63) & ~63); i += 64) act[i] = i < n ? i : 0;
    // inclusive prefix sums of the pooled vector (integers: exact in any order), padded for the branch-free search
    if (wave == 0) {
        const int seg = (V + 63) >> 6, vb = min(V, lane * seg), ve = min(V, vb + seg);
        uint32_t s = 0u;
        for (int v = vb; v < ve; ++v) s += s_pool[v];
        uint32_t inc = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
        uint32_t run = inc - s;
        for (int v = vb; v < ve; ++v) { run += s_pool[v]; s_cum[v] = run; }
    }
    for (int v = V + tid; v < P2; v += nt) s_cum[v] = 0xffffffffu;
    for (int t = lane; t < kTjMaxBins; t += 64) ccut[t] = 0;
    for (int v = lane; v < 2 * Vh; v += 64) hist[v] = 0u;
    __syncthreads();
    const double* __restrict__ P = P_LDS ? s_stage : a.P;
    const uint32_t N = s_ct[T];
    const double g_max = a.g_max[d], ll0 = a.ll0[d];
    const uint32_t item = kDealTag | (uint32_t)d;
    auto slot = [s_cum, P2](uint32_t i) {
        int p = 0;
        for (int step = P2 >> 1; step > 0; step >>= 1)
            if (s_cum[p + step - 1] <= i) p += step;           // the number of terms with cum <= i; cum[V - 1] = N > i: p <= V - 1
        return p;
    };
    const int bbeg = (int)blockIdx.y * a.reps_per_block, bend = min(a.B, bbeg + a.reps_per_block);
    int ge = 0;
    unsigned long long its = 0ull;
    const RfCountsU32 counts{hist};
    for (int b = bbeg + wave; b < bend; b += nw) {
        const uint32_t gb = a.b0 + (uint32_t)b;
        double gm = -std::numeric_limits<double>::infinity();
        for (int t = L; t <= T - L; ++t) {
            const uint32_t Na = s_ct[t], Nb = N - Na;
            if (Na) {                                          // an empty prefix deals nothing
                const DealCut cut = deal_select(lane, N, Na, a.key_bits, bins, item, gb, a.stream, a.k0, a.k1);
                deal_pass(lane, N, cut, a.key_bits, slot, hist, item, gb, a.stream, a.k0, a.k1);
            }
            rf_wave_sync();
            double llx = 0.0, G = 0.0;
            // one call site of the fit and of the sweep for the two sides (mixture_fit.cuh, rf_loglik, has the reason)
            for (int pass = 0; pass < 2; ++pass) {
                if (pass) {
                    for (int v = lane; v < V; v += 64) hist[v] = s_pool[v] - hist[v];  // the suffix = pooled - prefix
                    rf_wave_sync();
                }
                const uint32_t Nx = pass ? Nb : Na;
                double ll = 0.0;
                if (Nx) {                                      // an empty side: ll = 0, no iteration
                    for (int v = lane; v < V; v += 64) fb[v] = (double)hist[v] / (double)Nx;
                    rf_wave_sync();
                    its += (unsigned long long)rf_fit(P, act, w, n, fb, counts, rb, V, lane, a.maxiter, a.tol);
                    ll = rf_loglik<false>(P, act, w, n, counts, fb, -1, V, lane).ll;
                }
                if (pass == 0) llx = ll; else G = llx + ll;
                rf_wave_sync();
            }
            gm = fmax(gm, G);
            for (int v = lane; v < V; v += 64) hist[v] = 0u;
            rf_wave_sync();
        }
        ge += gm >= g_max;
        for (int t = L + lane; t <= T - L; t += 64) ccut[t] += gm >= s_g[t];
        if (a.rep && lane == 0) a.rep[(size_t)b * a.D + d] = 2.0 * (gm - ll0);
    }
    for (int t = L + lane; t <= T - L; t += 64)
        if (ccut[t]) atomicAdd(&a.count_cut[r0 + t], ccut[t]);
    if (lane == 0) {
        if (ge) atomicAdd(&a.count_ge[d], ge);
        if (its) atomicAdd(&a.iters[d], its);
    }
}

// the place of segment (i, j) in a sample's block of the table
inline int64_t tj_seg(int T, int i, int j) { return (int64_t)i * T - (int64_t)i * (i - 1) / 2 + (j - i - 1); }

int tj_launch_fit(mmm_ctx* ctx, TjArgs& a, const std::vector<int32_t>& dij, const std::vector<int64_t>& out, DevBuf<int32_t>& d_dij, DevBuf<int64_t>& d_out,
                  DevBuf<int>& counter)
{
    const size_t n_items = dij.size() / 4;
    if (!n_items) return MMM_OK;
    MMM_HIP(ctx, d_dij.alloc(dij.size())); MMM_HIP(ctx, d_out.alloc(out.size()));
    MMM_HIP(ctx, hipMemcpyAsync(d_dij.p, dij.data(), sizeof(int32_t) * dij.size(), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(d_out.p, out.data(), sizeof(int64_t) * out.size(), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));
    a.item_dij = d_dij.p; a.item_out = d_out.p; a.n_items = (int)n_items; a.counter = counter.p;
    // as many waves per block as their buffers leave room for; few items: fewer, so that they spread over the CUs
    const int cus = std::max(1, mmm_geo_cus(ctx));
    const size_t po = sizeof(double) * (size_t)tj_fit_doubles(a.Cp, a.V);
    int ow = kTjMaxWaves;
    while (ow > 1 && ow * po > kTjLdsBlock) ow >>= 1;
    while (ow > 1 && ((int64_t)n_items + ow - 1) / ow < cus) ow >>= 1;
    const size_t lds = ow * po;
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(kTjMaxWaves / ow, (int64_t)(kTjLdsBlock / lds)));
    const unsigned grid = (unsigned)std::min<int64_t>(((int64_t)n_items + ow - 1) / ow, (int64_t)cus * per_cu);
    a.wave_doubles = tj_fit_doubles(a.Cp, a.V);
    if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)k_traj_fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_traj_fit, dim3(grid), dim3(64 * ow), lds, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    return MMM_OK;
}

} // namespace

extern "C" {

int mmm_exposure_trajectory(mmm_ctx* ctx, int D, int C, int V, int nbins, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const int64_t* bin_ptr,
                            const double* cat, const uint8_t* allowed, int min_len, int max_cp, const double* penalty, int B, int b0, uint64_t seed, uint32_t stream,
                            int key_bits, int maxiter, double tol, double* seg_ll, double* best, int32_t* n_cp, int32_t* cp, double* w_seg, double* w_bin,
                            double* gain_cut, int32_t* cut, double* stat, int32_t* count_ge, int32_t* count_cut, int8_t* status, double* unexplained, int64_t* iters,
                            double* rep_stat)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    const char* who = "mmm_exposure_trajectory";
    MMM_CHECK(ctx, C >= 1 && V >= 1 && D >= 0 && nbins >= 0 && cat && bin_ptr, "%s: NULL argument, D < 0, nbins < 0, C < 1 or V < 1", who);
    if (C > kTjMaxC) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: C = %d catalogue signatures (limit %d)", who, C, kTjMaxC);
    if (V > kTjMaxV)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: V = %d terms; a block keeps the pooled counts and its waves' count vectors in LDS, which holds at most V = %d", who, V, kTjMaxV);
    if (D > kDealMaxD) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: D = %d samples (limit 2^28: the sample shares a counter word with the tag)", who, D);
    MMM_CHECK(ctx, key_bits >= 1 && key_bits <= 32, "%s: key_bits = %d (1..32)", who, key_bits);
    MMM_CHECK(ctx, maxiter >= 1 && tol >= 0.0, "%s: maxiter = %d (>= 1), tol = %g (>= 0)", who, maxiter, tol);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0, "%s: B < 0 or b0 < 0", who);
    MMM_CHECK(ctx, (int64_t)b0 + (int64_t)B <= (int64_t)INT32_MAX, "%s: b0 + B exceeds 2^31 - 1", who);
    MMM_CHECK(ctx, stream < 0x80000000u, "%s: stream = %u (below 2^31)", who, stream);
    MMM_CHECK(ctx, min_len >= 1 && max_cp >= 0, "%s: min_len = %d (>= 1), max_cp = %d (>= 0)", who, min_len, max_cp);
    MMM_CHECK(ctx, bin_ptr[0] == 0, "%s: bin_ptr[0] != 0", who);
    for (int d = 0; d < D; ++d) MMM_CHECK(ctx, bin_ptr[d + 1] >= bin_ptr[d], "%s: bin_ptr decreases at sample %d", who, d);
    MMM_CHECK(ctx, bin_ptr[D] == (int64_t)nbins, "%s: bin_ptr ends at %lld, not at nbins = %d", who, (long long)bin_ptr[D], nbins);
    for (int d = 0; d < D; ++d)
        if (bin_ptr[d + 1] - bin_ptr[d] > kTjMaxBins)
            return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: sample %d has T = %lld bins (limit %d)", who, d, (long long)(bin_ptr[d + 1] - bin_ptr[d]), kTjMaxBins);
    if (int rc = mmm_check_csr(ctx, who, nbins, V, doc_ptr, term, count)) return rc;
    std::vector<int32_t> nbin((size_t)nbins);
    if (int rc = mmm_doc_totals(ctx, who, nbins, doc_ptr, count, nbin.data())) return rc;
    const size_t Ds = (size_t)D, rows = (size_t)nbins + Ds;
    std::vector<uint32_t> ctot(rows, 0u);
    std::vector<int64_t> row0(Ds), seg0(Ds + 1, 0);
    std::vector<int32_t> nT(Ds);
    for (int d = 0; d < D; ++d) {
        const int T = (int)(bin_ptr[d + 1] - bin_ptr[d]);
        row0[(size_t)d] = bin_ptr[d] + d; nT[(size_t)d] = T;
        seg0[(size_t)d + 1] = seg0[(size_t)d] + (int64_t)T * (T + 1) / 2;
        int64_t s = 0;
        for (int t = 0; t < T; ++t) {
            s += nbin[(size_t)(bin_ptr[d] + t)];
            if (s >= ((int64_t)1 << 31))
                return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: sample %d holds 2^31 or more mutations (a mutation's index is a 32-bit word: N_d < 2^31)", who, d);
            ctot[(size_t)row0[(size_t)d] + t + 1] = (uint32_t)s;
        }
    }
    MMM_CHECK(ctx, D == 0 || penalty, "%s: penalty == NULL", who);
    for (int d = 0; d < D; ++d) MMM_CHECK(ctx, std::isfinite(penalty[d]) && penalty[d] >= 0.0, "%s: penalty[%d] = %g is negative or not finite", who, d, penalty[d]);
    std::vector<double> P;           // the catalogue with rows normalised: mmm_refit_exposures' P
    if (int rc = mmm_normalise_rows(ctx, who, C, V, cat, P)) return rc;
    if (D == 0 || nbins == 0) return MMM_OK;
    MMM_CHECK(ctx, seg_ll && best && n_cp && (cp || max_cp == 0) && w_seg && gain_cut && cut && stat && count_ge && count_cut && status && unexplained && iters,
              "%s: NULL output", who);
    const int L = min_len, M = max_cp, M1 = max_cp + 1;
    const size_t nb = (size_t)nbins;
    const int64_t S = seg0[Ds];
    const bool want_rep = rep_stat && B > 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();

    // what is fitted and what is tested is known from the arguments
    std::vector<int8_t> hst(Ds, 0);
    std::vector<int> nA(Ds, 0);
    int max_n = 0;
    size_t n_tested = 0;
    std::vector<int32_t> dij;
    std::vector<int64_t> iout;
    auto defined = [L](int T, int i, int j) { return j - i >= L || (i == 0 && j == T); };    // the whole timeline is a segment whatever L
    for (int d = 0; d < D; ++d) {
        const int T = nT[(size_t)d];
        int n = C;
        if (allowed) {
            n = 0;
            for (int c = 0; c < C; ++c) n += allowed[(size_t)d * C + c] != 0;
        }
        nA[(size_t)d] = n;
        if (T == 0 || ctot[(size_t)row0[(size_t)d] + T] == 0u || n == 0) { hst[(size_t)d] = 3; continue; }
        if (T < 2 * L) hst[(size_t)d] = 1;
        else { max_n = std::max(max_n, n); ++n_tested; }
        for (int i = 0; i < T; ++i)
            for (int j = i + 1; j <= T; ++j)
                if (defined(T, i, j)) {
                    dij.insert(dij.end(), {d, i, j, 1});
                    iout.insert(iout.end(), {seg0[(size_t)d] + tj_seg(T, i, j), (int64_t)-1});
                }
    }
    if (dij.size() / 4 > (size_t)INT32_MAX) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: %zu segments in the table (limit 2^31 - 1)", who, dij.size() / 4);

    const int Cp = (C + 63) & ~63, cus = std::max(1, mmm_geo_cus(ctx));
    DevCsr csr; DevBuf<uint32_t> pre, ct; DevBuf<int64_t> r0d, brow, d_out, d_out2; DevBuf<int32_t> ntd, d_dij, d_dij2, cnt, itm; DevBuf<double> Pd, segd, wout, dd, gobs, rep;
    DevBuf<uint8_t> alw; DevBuf<unsigned long long> its; DevBuf<int> counter;
    if (int rc = csr.upload(ctx, nbins, doc_ptr, term, count)) return rc;
    MMM_HIP(ctx, pre.alloc(rows * (size_t)V)); MMM_HIP(ctx, ct.alloc(rows)); MMM_HIP(ctx, r0d.alloc(Ds)); MMM_HIP(ctx, brow.alloc(nb)); MMM_HIP(ctx, ntd.alloc(Ds));
    MMM_HIP(ctx, Pd.alloc(P.size())); MMM_HIP(ctx, segd.alloc((size_t)std::max<int64_t>(S, 1))); MMM_HIP(ctx, dd.alloc(3 * Ds)); MMM_HIP(ctx, its.alloc(Ds));
    MMM_HIP(ctx, counter.alloc(1)); MMM_HIP(ctx, cnt.alloc(Ds + rows)); MMM_HIP(ctx, gobs.alloc(rows));
    if (allowed) MMM_HIP(ctx, alw.alloc(Ds * C));
    std::vector<int64_t> bin_row(nb);
    for (int d = 0; d < D; ++d)
        for (int64_t t = bin_ptr[d]; t < bin_ptr[d + 1]; ++t) bin_row[(size_t)t] = t + d + 1;
    MMM_HIP(ctx, hipMemcpyAsync(ct.p, ctot.data(), sizeof(uint32_t) * rows, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(r0d.p, row0.data(), sizeof(int64_t) * Ds, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(brow.p, bin_row.data(), sizeof(int64_t) * nb, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(ntd.p, nT.data(), sizeof(int32_t) * Ds, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(Pd.p, P.data(), sizeof(double) * P.size(), hipMemcpyHostToDevice, ctx->stream));
    if (allowed) MMM_HIP(ctx, hipMemcpyAsync(alw.p, allowed, Ds * C, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(pre.p, 0, sizeof(uint32_t) * pre.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(segd.p, 0, sizeof(double) * segd.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(dd.p, 0, sizeof(double) * dd.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(its.p, 0, sizeof(unsigned long long) * Ds, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * cnt.n, ctx->stream));

    // ---- prefix vectors
    hipLaunchKernelGGL(k_traj_scatter, dim3((unsigned)nbins), dim3(64), 0, ctx->stream, csr.ptr, csr.term, csr.count, brow.p, V, pre.p);
    MMM_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_traj_cumulate, dim3((unsigned)D, (unsigned)((V + 255) / 256)), dim3(256), 0, ctx->stream, r0d.p, ntd.p, V, pre.p);
    MMM_LAUNCH_CHECK(ctx);

    TjArgs a{};
    a.D = D; a.C = C; a.V = V; a.Cp = Cp; a.maxiter = maxiter; a.key_bits = key_bits; a.tol = tol;
    a.pre = pre.p; a.ctot = ct.p; a.row0 = r0d.p; a.nT = ntd.p; a.P = Pd.p; a.allowed = allowed ? alw.p : nullptr;
    a.seg_ll = segd.p; a.unexplained = dd.p; a.iters = its.p;

    // ---- the table
    if (int rc = tj_launch_fit(ctx, a, dij, iout, d_dij, d_out, counter)) return rc;
    std::vector<double> hseg((size_t)S, nan), hdev((size_t)S);
    if (S) MMM_HIP(ctx, hipMemcpyAsync(hdev.data(), segd.p, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < iout.size(); k += 2) hseg[(size_t)iout[k]] = hdev[(size_t)iout[k]];

    // ---- optimal partitioning and the scan, on the table
    std::vector<double> hbest(Ds * M1, nan), hgain(nb, nan), hstat(Ds, 0.0), hgobs(rows, nan), hgmax(Ds, 0.0), hll0(Ds, 0.0);
    std::vector<int32_t> hncp(Ds, 0), hcp(Ds * (size_t)M, -1), hcut(Ds, -1);
    std::vector<int32_t> dij2;
    std::vector<int64_t> iout2;
    {
        std::vector<double> F((size_t)M1 * (kTjMaxBins + 1));
        std::vector<int> arg((size_t)M1 * (kTjMaxBins + 1));
        for (int d = 0; d < D; ++d) {
            if (hst[(size_t)d] == 3) continue;
            const int T = nT[(size_t)d];
            const double* tab = hseg.data() + seg0[(size_t)d];
            auto ll = [&](int i, int j) { return tab[tj_seg(T, i, j)]; };
            const int Mx = std::min(M, std::max(T / L - 1, 0));
            const int W = kTjMaxBins + 1;
            for (int j = 1; j <= T; ++j) F[(size_t)j] = defined(T, 0, j) ? ll(0, j) : nan;
            F[0] = nan;
            for (int m = 1; m <= Mx; ++m)
                for (int j = 0; j <= T; ++j) {
                    double bestv = nan; int bi = -1;
                    for (int i = 1; i < j; ++i) {
                        const double f = F[(size_t)(m - 1) * W + i];
                        if (std::isnan(f) || !defined(T, i, j)) continue;
                        const double v = f + ll(i, j);
                        if (bi < 0 || v > bestv) { bestv = v; bi = i; }          // ties: the lowest i
                    }
                    F[(size_t)m * W + j] = bestv; arg[(size_t)m * W + j] = bi;
                }
            int mb = 0;
            double vb = nan;
            for (int m = 0; m <= Mx; ++m) {
                const double f = F[(size_t)m * W + T];
                hbest[(size_t)d * M1 + m] = f;
                if (std::isnan(f)) continue;
                const double v = f - (double)m * penalty[d];
                if (std::isnan(vb) || v > vb) { vb = v; mb = m; }                // ties: the smallest m
            }
            hncp[(size_t)d] = mb;
            int j = T;
            std::vector<int> bounds((size_t)mb + 2);
            bounds[(size_t)mb + 1] = T; bounds[0] = 0;
            for (int m = mb; m >= 1; --m) {
                const int i = arg[(size_t)m * W + j];
                hcp[(size_t)d * M + (m - 1)] = i; bounds[(size_t)m] = i;
                j = i;
            }
            for (int k = 0; k <= mb; ++k) {
                dij2.insert(dij2.end(), {d, bounds[(size_t)k], bounds[(size_t)k + 1], 0});
                iout2.insert(iout2.end(), {(int64_t)-1, (int64_t)d * M1 + k});
            }
            hll0[(size_t)d] = ll(0, T);
            if (hst[(size_t)d] != 0) continue;
            double gmax = nan; int tb = -1;
            for (int t = L; t <= T - L; ++t) {
                const double G = ll(0, t) + ll(t, T);
                hgobs[(size_t)row0[(size_t)d] + t] = G;
                hgain[(size_t)(bin_ptr[d] + t)] = G - ll(0, T);
                if (tb < 0 || G > gmax) { gmax = G; tb = t; }
            }
            hgmax[(size_t)d] = gmax; hcut[(size_t)d] = tb;
            hstat[(size_t)d] = std::fmax(2.0 * (gmax - ll(0, T)), 0.0);
        }
    }

    // ---- the weights of the chosen segments and of the bins: the table's fits again (cold starts: the same bits), not counted in iters
    const size_t wrows = Ds * M1 + (w_bin ? nb : 0);
    if (w_bin)
        for (int d = 0; d < D; ++d) {
            if (hst[(size_t)d] == 3) continue;
            for (int t = 0; t < nT[(size_t)d]; ++t) {
                dij2.insert(dij2.end(), {d, t, t + 1, 0});
                iout2.insert(iout2.end(), {(int64_t)-1, (int64_t)(Ds * M1) + bin_ptr[d] + t});
            }
        }
    MMM_HIP(ctx, wout.alloc(wrows * C));
    MMM_HIP(ctx, hipMemsetAsync(wout.p, 0, sizeof(double) * wout.n, ctx->stream));
    a.wout = wout.p;
    if (int rc = tj_launch_fit(ctx, a, dij2, iout2, d_dij2, d_out2, counter)) return rc;

    // ---- replicates
    if (B > 0 && n_tested) {
        MMM_HIP(ctx, itm.alloc(n_tested));
        MMM_HIP(ctx, hipMemcpyAsync(gobs.p, hgobs.data(), sizeof(double) * rows, hipMemcpyHostToDevice, ctx->stream));
        MMM_HIP(ctx, hipMemcpyAsync(dd.p + Ds, hgmax.data(), sizeof(double) * Ds, hipMemcpyHostToDevice, ctx->stream));
        MMM_HIP(ctx, hipMemcpyAsync(dd.p + 2 * Ds, hll0.data(), sizeof(double) * Ds, hipMemcpyHostToDevice, ctx->stream));
        if (want_rep) {
            MMM_HIP(ctx, rep.alloc((size_t)B * Ds));
            MMM_HIP(ctx, hipMemsetAsync(rep.p, 0, sizeof(double) * (size_t)B * Ds, ctx->stream));
        }
        int P2 = 2;
        while (P2 < V) P2 <<= 1;
        const size_t fixed = tj_rep_fixed(P2, V);
        const size_t pw = sizeof(double) * (size_t)tj_rep_doubles(Cp, V);
        int nw = 1;
        for (int t = kTjMaxWaves; t >= 1; t >>= 1)
            if (fixed + t * pw <= kTjLdsBlock) { nw = t; break; }
        // rows of P a block can stage beside nw waves' buffers (one double may pad the rows to 16 bytes)
        auto cap = [&](int t) { const size_t room = (kTjLdsBlock - fixed - t * pw) / sizeof(double); return room ? (int)((room - 1) / (size_t)V) : 0; };
        int rows_cap = 0;
        if (!mmm_off(ctx->tune, MMM_OFF_REFIT_LDS)) {
            if (nw == kTjMaxWaves && cap(nw) < max_n && cap(nw / 2) >= max_n) nw >>= 1;       // four waves with every sample's rows in LDS beat eight through L2
            rows_cap = cap(nw);
        }
        std::vector<int32_t> staged, direct;
        int srows = 0;
        for (int d = 0; d < D; ++d) {
            if (hst[(size_t)d] != 0) continue;
            if (nA[(size_t)d] <= rows_cap) { staged.push_back(d); srows = std::max(srows, nA[(size_t)d]); }
            else direct.push_back(d);
        }
        std::vector<int32_t> all(staged);
        all.insert(all.end(), direct.begin(), direct.end());
        MMM_HIP(ctx, hipMemcpyAsync(itm.p, all.data(), sizeof(int32_t) * all.size(), hipMemcpyHostToDevice, ctx->stream));
        a.L = L; a.B = B; a.b0 = (uint32_t)b0; a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
        a.g_obs = gobs.p; a.g_max = dd.p + Ds; a.ll0 = dd.p + 2 * Ds; a.count_ge = cnt.p; a.count_cut = cnt.p + Ds;
        a.P2 = P2; a.rep = want_rep ? rep.p : nullptr; a.wave_doubles = tj_rep_doubles(Cp, V);
        for (int part = 0; part < 2; ++part) {
            const size_t n = part ? direct.size() : staged.size();
            if (!n) continue;
            // replicates per block: one per wave, more while the launch still covers the device several times over (a block's set-up is
            // shared by its replicates); the geometry cannot change a bit of the output
            int rpb = nw;
            while (rpb < B && (int64_t)n * ((B + 2 * rpb - 1) / (2 * rpb)) >= 8ll * cus) rpb *= 2;
            while ((B + rpb - 1) / rpb > 65535) rpb *= 2;
            a.items = itm.p + (part ? staged.size() : 0);
            a.reps_per_block = rpb;
            a.stage_doubles = part ? 0 : (int)(((size_t)srows * V + 1) & ~(size_t)1);
            const size_t lds = fixed + sizeof(double) * (size_t)a.stage_doubles + nw * pw;
            auto kern = part ? k_traj_rep<false> : k_traj_rep<true>;
            if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)n, (unsigned)((B + rpb - 1) / rpb)), dim3(64 * nw), lds, ctx->stream, a);
            MMM_LAUNCH_CHECK(ctx);
        }
    }
    // staged on the host so that a failing copy leaves the caller's arrays as they were
    std::vector<double> hw(wout.n), hu(Ds), hr(want_rep && rep.p ? (size_t)B * Ds : 0);
    std::vector<int32_t> hc(cnt.n);
    std::vector<unsigned long long> hi(Ds);
    MMM_HIP(ctx, hipMemcpyAsync(hw.data(), wout.p, sizeof(double) * hw.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hu.data(), dd.p, sizeof(double) * Ds, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hc.data(), cnt.p, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hi.data(), its.p, sizeof(unsigned long long) * Ds, hipMemcpyDeviceToHost, ctx->stream));
    if (hr.size()) MMM_HIP(ctx, hipMemcpyAsync(hr.data(), rep.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (S) memcpy(seg_ll, hseg.data(), sizeof(double) * (size_t)S);
    memcpy(best, hbest.data(), sizeof(double) * hbest.size());
    memcpy(n_cp, hncp.data(), sizeof(int32_t) * Ds);
    if (M) memcpy(cp, hcp.data(), sizeof(int32_t) * hcp.size());
    memcpy(w_seg, hw.data(), sizeof(double) * Ds * M1 * C);
    if (w_bin) memcpy(w_bin, hw.data() + Ds * M1 * C, sizeof(double) * nb * C);
    memcpy(gain_cut, hgain.data(), sizeof(double) * nb);
    memcpy(cut, hcut.data(), sizeof(int32_t) * Ds);
    memcpy(stat, hstat.data(), sizeof(double) * Ds);
    memcpy(count_ge, hc.data(), sizeof(int32_t) * Ds);
    for (int d = 0; d < D; ++d)
        for (int t = 0; t < nT[(size_t)d]; ++t) count_cut[bin_ptr[d] + t] = hc[Ds + (size_t)row0[(size_t)d] + t];
    memcpy(status, hst.data(), Ds);
    memcpy(unexplained, hu.data(), sizeof(double) * Ds);
    for (size_t d = 0; d < Ds; ++d) iters[d] = (int64_t)hi[d];
    if (want_rep)
        for (int b = 0; b < B; ++b)
            for (size_t d = 0; d < Ds; ++d) rep_stat[(size_t)b * Ds + d] = hst[d] == 0 ? hr[(size_t)b * Ds + d] : nan;
    return MMM_OK;
}

} // extern "C"
