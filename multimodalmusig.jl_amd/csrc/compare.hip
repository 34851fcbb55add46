// compare.hip -- mmm_deal_counts and mmm_compare_exposures: did the exposures of a tumour change between its two mutation sets?  An exact
// permutation test per sample: under H0 the partition of the pooled mutations into sets of sizes N_a and N_b is a uniform random subset,
// so a replicate deals N_a of the N pooled mutations to set a, refits both sets and compares (no counterpart in the reference;
// include/mmmusig.h has the normative definition, DESIGN.md section 4.23 the reasoning).
//
// The dealing (deal_select.cuh, shared with trajectory.hip).  Mutation i carries the key k_i = u_i >> (32 - key_bits), u_i its own Philox word; set a is the N_a smallest (k_i, i).  A wave
// never materialises the keys: Philox is counter-based, so it regenerates them.  A radix select over 256 wave-private LDS bins finds the
// N_a-th smallest key digit by digit (8 bits a pass); one more pass, chunks of 256 mutations ascending, deals every key below that
// threshold and, by a ballot prefix in index order, the first r of the keys equal to it.  Integer throughout: the same bits under every
// geometry.
//
// mmm_compare_exposures runs two phases on the context's stream, like presence.hip.  "Observed": one wave per testable sample behind a
// work counter; three fits (set a, set b, pooled).  "Replicates": grid (sample, replicate chunk); a block forms the pooled vector and its
// prefix sums in LDS, stages the rows of the sample's signatures in LDS (where they fit), and every wave takes one replicate at a time:
// select, deal into its own LDS histogram, fit, turn the histogram into pooled - a in place, fit again, compare.  The replicate's counts
// never leave LDS.  fit(A) is the one refit.hip runs (mixture_fit.cuh).
#include "mmm_internal.h"
#include "dev_math.h"
#include "mmm_philox.h"
#include "mixture_fit.cuh"
#include "deal_select.cuh"

#include <limits>

namespace {

constexpr int kCmMaxC = 256;
constexpr int kCmMaxV = 4096;                   // the pooled vector, its prefix sums and a wave's buffers stay in LDS
constexpr int kCmMaxWaves = 8;
constexpr size_t kCmLdsBlock = 160 * 1024;
constexpr int kDealWaves = 4;

// ---- mmm_deal_counts -------------------------------------------------------------------------------------------------------------------------
// grid (D, replicate chunks), kDealWaves waves; a wave takes one replicate at a time.  cum: inclusive prefix sums per document, in global
// memory (a row may be of any length), searched by bisection.  out [nb][nnz], zeroed by the host; static LDS: the waves' bins.
__global__ __launch_bounds__(64 * kDealWaves) void k_deal_counts(const int64_t* __restrict__ doc_ptr, const uint32_t* __restrict__ cum, const int32_t* __restrict__ n_a,
                                                                 int64_t nnz, int nb, int reps_per_block, uint32_t b0, uint32_t stream, uint32_t k0, uint32_t k1,
                                                                 int key_bits, int32_t* __restrict__ out)
{
    __shared__ uint32_t s_bins[kDealWaves][kDealBins];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t d = blockIdx.x;
    const int64_t e0 = doc_ptr[d];
    const int W = (int)(doc_ptr[d + 1] - e0);
    if (W == 0) return;
    const uint32_t* cg = cum + e0;
    const uint32_t N = cg[W - 1], Na = (uint32_t)n_a[d];
    if (N == 0u || Na == 0u) return;
    auto slot = [cg, W](uint32_t i) {
        int lo = 0, hi = W - 1;                                // first e with cum[e] > i; cum[W - 1] = N > i, so it exists
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cg[mid] > i) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    const int bbeg = (int)blockIdx.y * reps_per_block, bend = min(nb, bbeg + reps_per_block);
    for (int b = bbeg + wave; b < bend; b += kDealWaves) {
        const uint32_t gb = b0 + (uint32_t)b;
        const DealCut cut = deal_select(lane, N, Na, key_bits, s_bins[wave], kDealTag | d, gb, stream, k0, k1);
        deal_pass(lane, N, cut, key_bits, slot, out + (size_t)b * (size_t)nnz + e0, kDealTag | d, gb, stream, k0, k1);
    }
}

// ---- mmm_compare_exposures -------------------------------------------------------------------------------------------------------------------
struct CmArgs {
    int D, C, V, Cp, maxiter, key_bits;
    double tol;
    const int64_t* ptr_a; const int32_t* term_a; const int32_t* count_a;
    const int64_t* ptr_b; const int32_t* term_b; const int32_t* count_b;
    const double* P;                 // [C][V], rows normalised
    const uint8_t* allowed;          // [D][C] or NULL
    const int32_t* na; const int32_t* nb;       // [D] totals of the two sets
    const int32_t* items;            // the testable samples this launch takes
    int n_items;
    double* w_a; double* w_b; double* w_pool;   // [D][C]
    double* stat; double* t_obs; double* ll_pool; double* unexplained;      // [D]
    unsigned long long* iters;
    int* counter;                    // next item of the observed phase
    // replicate phase
    int B, reps_per_block, P2, wave_doubles, stage_doubles;     // stage_doubles: the LDS of the staged rows (even), 0 where they are read through L2
    uint32_t b0, k0, k1, stream;
    int32_t* count_ge; int32_t* count_sig; int32_t* count_max;
    double* rep;                     // [B][D] or NULL
};

// observed phase, a wave's own LDS: three weight vectors (a, b, pooled), the list of signatures, f_v, r_v and three count vectors
__host__ __device__ inline int cm_obs_doubles(int Cp, int V) { return (3 * Cp + Cp / 2 + 2 * V + 3 * ((V + 1) / 2) + 1) & ~1; }
// replicate phase, a wave's own LDS: the weights of the two fits, the list, its two counters per signature, f_v, r_v, the count vector, the bins
__host__ __device__ inline int cm_rep_doubles(int Cp, int V) { return (2 * Cp + Cp / 2 + Cp + 2 * V + (V + 1) / 2 + kDealBins / 2 + 1) & ~1; }

// a document's entries added into hist (duplicate terms summed) by the nt threads t = 0 .. nt - 1
__device__ __forceinline__ void cm_add_rows(const int64_t* ptr, const int32_t* term, const int32_t* count, int d, uint32_t* hist, int t, int nt)
{
    for (int64_t e = ptr[d] + t; e < ptr[d + 1]; e += nt) {
        const int cnt = count[e];
        if (cnt > 0) atomicAdd(&hist[term[e]], (uint32_t)cnt);
    }
}

// Observed phase.  Dynamic LDS: per wave cm_obs_doubles doubles; the catalogue is read through L2 (three fits per sample: a B-th of the
// call's work).  The host has zeroed every output and lists the testable samples only.
__global__ __launch_bounds__(64 * kCmMaxWaves) void k_compare_obs(const CmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_cm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.C, V = a.V, Cp = a.Cp, Vh = (V + 1) / 2;
    double* base = s_cm + (size_t)wave * a.wave_doubles;
    double* w3 = base;
    int* act = (int*)(base + 3 * (size_t)Cp);
    double* fb = base + 3 * (size_t)Cp + Cp / 2;
    double* rb = fb + V;
    uint32_t* h3 = (uint32_t*)(rb + V);
    const double* __restrict__ P = a.P;
    for (;;) {
        const int j = rf_next_item(a.counter, lane);           // its contract shapes this loop: one body, one closing fence
        if (j >= a.n_items) break;
        const int d = a.items[j];
        for (int v = lane; v < 3 * 2 * Vh; v += 64) h3[v] = 0u;
        rf_wave_sync();
        cm_add_rows(a.ptr_a, a.term_a, a.count_a, d, h3, lane, 64);
        cm_add_rows(a.ptr_b, a.term_b, a.count_b, d, h3 + 2 * Vh, lane, 64);
        rf_wave_sync();
        for (int v = lane; v < V; v += 64) h3[4 * Vh + v] = h3[v] + h3[2 * Vh + v];
        int pos;
        const int n = rf_active_list(a.allowed ? a.allowed + (size_t)d * C : nullptr, C, -1, act, lane, pos);
        rf_pad_list(act, n, lane);
        rf_wave_sync();
        const double Na = (double)a.na[d], Nb = (double)a.nb[d];
        double llx = 0.0, T = 0.0, ll0 = 0.0, u0 = 0.0;
        int its = 0;
        // a loop with one call site each, so that the kernel holds the fit and the sweep once (mixture_fit.cuh, rf_loglik, has the reason)
        for (int pass = 0; pass < 3; ++pass) {
            const uint32_t* h = h3 + (size_t)pass * 2 * Vh;
            const RfCountsU32 counts{h};
            const double Nx = pass == 0 ? Na : (pass == 1 ? Nb : Na + Nb);
            double* cw = w3 + (size_t)pass * Cp;
            for (int v = lane; v < V; v += 64) fb[v] = (double)h[v] / Nx;
            rf_wave_sync();
            its += rf_fit(P, act, cw, n, fb, counts, rb, V, lane, a.maxiter, a.tol);
            const RfLoglik L = rf_loglik<false>(P, act, cw, n, counts, fb, -1, V, lane);
            if (pass == 0) llx = L.ll;
            else if (pass == 1) T = llx + L.ll;
            else { ll0 = L.ll; u0 = L.u; }
            rf_wave_sync();
        }
        for (int i = lane; i < n; i += 64) {
            const size_t o = (size_t)d * C + act[i];
            a.w_a[o] = w3[i]; a.w_b[o] = w3[Cp + i]; a.w_pool[o] = w3[2 * Cp + i];
        }
        if (lane == 0) {
            a.t_obs[d] = T; a.ll_pool[d] = ll0;
            a.stat[d] = fmax(2.0 * (T - ll0), 0.0);
            a.unexplained[d] = u0;
            a.iters[d] = (unsigned long long)its;
        }
        rf_wave_sync();
    }
}

// Replicate phase: grid (items, replicate chunks), blockDim 64 nw.  Dynamic LDS: uint32 cum[P2] | uint32 pooled[V, even] | double
// delta_obs[Cp] | int rows[Cp] (the catalogue rows of the list) | P_LDS: the rows of A at stride V | per wave cm_rep_doubles doubles.
template <bool P_LDS>
__global__ __launch_bounds__(64 * kCmMaxWaves) void k_compare_rep(const CmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_cm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6), nt = (int)blockDim.x;
    const int C = a.C, V = a.V, Cp = a.Cp, P2 = a.P2, Vh = (V + 1) / 2;
    const int d = a.items[blockIdx.x];
    uint32_t* s_cum = (uint32_t*)s_cm;
    uint32_t* s_pool = s_cum + P2;                             // P2 >= 2: 8-byte steps
    double* s_dobs = s_cm + P2 / 2 + Vh;
    int* s_rows = (int*)(s_dobs + Cp);
    double* s_stage = s_dobs + Cp + Cp / 2;
    double* base = s_stage + (P_LDS ? a.stage_doubles : 0) + (size_t)wave * a.wave_doubles;
    double* wa = base; double* wb = base + Cp;
    int* act = (int*)(base + 2 * (size_t)Cp);
    int* csig = act + Cp; int* cmax = csig + Cp;
    double* fb = base + 3 * (size_t)Cp + Cp / 2;
    double* rb = fb + V;
    uint32_t* hist = (uint32_t*)(rb + V);
    uint32_t* bins = hist + 2 * Vh;
    // every wave builds the list for itself (the same bits): no wave waits for another after the set-up
    int pos;
    const int n = rf_active_list(a.allowed ? a.allowed + (size_t)d * C : nullptr, C, -1, act, lane, pos);
    rf_pad_list(act, n, lane);
    for (int v = tid; v < 2 * Vh; v += nt) s_pool[v] = 0u;
    __syncthreads();
    cm_add_rows(a.ptr_a, a.term_a, a.count_a, d, s_pool, tid, nt);
    cm_add_rows(a.ptr_b, a.term_b, a.count_b, d, s_pool, tid, nt);
    for (int i = tid; i < n; i += nt) {
        const size_t o = (size_t)d * C + act[i];
        s_dobs[i] = fabs(a.w_a[o] - a.w_b[o]);
        s_rows[i] = act[i];
    }
    if (P_LDS) {
        for (int i = wave; i < n; i += nw) {
            const double* src = a.P + (size_t)act[i] * V;
            for (int v = lane; v < V; v += 64) s_stage[(size_t)i * V + v] = src[v];
        }
    }
    __syncthreads();                                           // the pooled vector, delta_obs and the staged rows are there; act has been read
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
    for (int i = lane; i < Cp; i += 64) { csig[i] = 0; cmax[i] = 0; }
    for (int v = lane; v < 2 * Vh; v += 64) hist[v] = 0u;
    __syncthreads();
    const double* __restrict__ P = P_LDS ? s_stage : a.P;
    const uint32_t Na = (uint32_t)a.na[d], Nb = (uint32_t)a.nb[d], N = Na + Nb;
    const double t_obs = a.t_obs[d], ll0 = a.ll_pool[d];
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
    for (int b = bbeg + wave; b < bend; b += nw) {
        const uint32_t gb = a.b0 + (uint32_t)b;
        const DealCut cut = deal_select(lane, N, Na, a.key_bits, bins, item, gb, a.stream, a.k0, a.k1);
        deal_pass(lane, N, cut, a.key_bits, slot, hist, item, gb, a.stream, a.k0, a.k1);
        rf_wave_sync();
        double llx = 0.0, T = 0.0;
        const RfCountsU32 counts{hist};
        // one call site of the fit and of the sweep for the two sets (mixture_fit.cuh, rf_loglik, has the reason)
        for (int pass = 0; pass < 2; ++pass) {
            if (pass) {
                for (int v = lane; v < V; v += 64) hist[v] = s_pool[v] - hist[v];      // set b = pooled - set a
                rf_wave_sync();
            }
            const double Nx = (double)(pass ? Nb : Na);
            double* cw = pass ? wb : wa;
            for (int v = lane; v < V; v += 64) fb[v] = (double)hist[v] / Nx;
            rf_wave_sync();
            its += (unsigned long long)rf_fit(P, act, cw, n, fb, counts, rb, V, lane, a.maxiter, a.tol);
            const RfLoglik L = rf_loglik<false>(P, act, cw, n, counts, fb, -1, V, lane);
            if (pass == 0) llx = L.ll; else T = llx + L.ll;
            rf_wave_sync();
        }
        double dm = 0.0;
        for (int i = lane; i < n; i += 64) dm = fmax(dm, fabs(wa[i] - wb[i]));
        dm = wave_max(dm);
        for (int i = lane; i < n; i += 64) {
            const double dobs = s_dobs[i];
            csig[i] += fabs(wa[i] - wb[i]) >= dobs;
            cmax[i] += dm >= dobs;
        }
        ge += T >= t_obs;
        if (a.rep && lane == 0) a.rep[(size_t)b * a.D + d] = 2.0 * (T - ll0);
        for (int v = lane; v < V; v += 64) hist[v] = 0u;
        rf_wave_sync();
    }
    for (int i = lane; i < n; i += 64) {
        const size_t o = (size_t)d * C + s_rows[i];
        if (csig[i]) atomicAdd(&a.count_sig[o], csig[i]);
        if (cmax[i]) atomicAdd(&a.count_max[o], cmax[i]);
    }
    if (lane == 0) {
        if (ge) atomicAdd(&a.count_ge[d], ge);
        if (its) atomicAdd(&a.iters[d], its);
    }
}

} // namespace

extern "C" {

int mmm_deal_counts(mmm_ctx* ctx, int D, const int64_t* doc_ptr, const int32_t* count, const int32_t* n_a, int B, int b0, uint64_t seed, uint32_t stream,
                    int key_bits, int32_t* out)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, D >= 0 && doc_ptr && (D == 0 || n_a), "mmm_deal_counts: D < 0, doc_ptr == NULL or n_a == NULL");
    MMM_CHECK(ctx, key_bits >= 1 && key_bits <= 32, "mmm_deal_counts: key_bits = %d (1..32)", key_bits);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0, "mmm_deal_counts: B < 0 or b0 < 0");
    MMM_CHECK(ctx, (int64_t)b0 + (int64_t)B <= (int64_t)INT32_MAX, "mmm_deal_counts: b0 + B exceeds 2^31 - 1");
    MMM_CHECK(ctx, stream < 0x80000000u, "mmm_deal_counts: stream = %u (below 2^31)", stream);
    if (D > kDealMaxD) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_deal_counts: D = %d samples (limit 2^28: the sample shares a counter word with the tag)", D);
    MMM_CHECK(ctx, doc_ptr[0] == 0, "mmm_deal_counts: doc_ptr[0] != 0");
    for (int d = 0; d < D; ++d) MMM_CHECK(ctx, doc_ptr[d + 1] >= doc_ptr[d], "mmm_deal_counts: doc_ptr decreases at document %d", d);
    const int64_t nnz = doc_ptr[D];
    MMM_CHECK(ctx, nnz == 0 || count, "mmm_deal_counts: count == NULL");
    std::vector<uint32_t> cum((size_t)nnz);
    for (int d = 0; d < D; ++d) {
        if (doc_ptr[d + 1] - doc_ptr[d] >= ((int64_t)1 << 31))
            return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_deal_counts: document %d has %lld entries (limit 2^31 - 1)", d, (long long)(doc_ptr[d + 1] - doc_ptr[d]));
        uint64_t s = 0;
        for (int64_t e = doc_ptr[d]; e < doc_ptr[d + 1]; ++e) {
            MMM_CHECK(ctx, count[e] >= 0, "mmm_deal_counts: entry %lld has count %d", (long long)e, count[e]);
            s += (uint64_t)count[e];
            if (s >= ((uint64_t)1 << 31))
                return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_deal_counts: document %d holds 2^31 or more counts (a mutation's index is a 32-bit word: N_d < 2^31)", d);
            cum[(size_t)e] = (uint32_t)s;
        }
        MMM_CHECK(ctx, n_a[d] >= 0 && (uint64_t)n_a[d] <= s, "mmm_deal_counts: n_a[%d] = %d is outside [0, N_d = %llu]", d, n_a[d], (unsigned long long)s);
    }
    if (B == 0 || nnz == 0) return MMM_OK;
    MMM_CHECK(ctx, out, "mmm_deal_counts: out == NULL");
    DevBuf<int64_t> dp; DevBuf<uint32_t> cm; DevBuf<int32_t> na, o;
    // replicates go through a device buffer of at most 2^28 counts (1 GiB) at a time
    const int Bc = (int)std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)1 << 28) / nnz));
    MMM_HIP(ctx, dp.alloc((size_t)D + 1)); MMM_HIP(ctx, cm.alloc((size_t)nnz)); MMM_HIP(ctx, na.alloc((size_t)D)); MMM_HIP(ctx, o.alloc((size_t)Bc * (size_t)nnz));
    MMM_HIP(ctx, hipMemcpyAsync(dp.p, doc_ptr, sizeof(int64_t) * ((size_t)D + 1), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(cm.p, cum.data(), sizeof(uint32_t) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(na.p, n_a, sizeof(int32_t) * (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    const int cus = std::max(1, mmm_geo_cus(ctx));
    for (int off = 0; off < B; off += Bc) {
        const int nb = std::min(Bc, B - off);
        int rpb = kDealWaves;
        while (rpb < nb && (int64_t)D * ((nb + 2 * rpb - 1) / (2 * rpb)) >= 8ll * cus) rpb *= 2;
        while ((nb + rpb - 1) / rpb > 65535) rpb *= 2;
        MMM_HIP(ctx, hipMemsetAsync(o.p, 0, sizeof(int32_t) * (size_t)nb * (size_t)nnz, ctx->stream));
        hipLaunchKernelGGL(k_deal_counts, dim3((unsigned)D, (unsigned)((nb + rpb - 1) / rpb)), dim3(64 * kDealWaves), 0, ctx->stream, dp.p, cm.p, na.p, nnz, nb, rpb,
                           (uint32_t)(b0 + off), stream, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), key_bits, o.p);
        MMM_LAUNCH_CHECK(ctx);
        MMM_HIP(ctx, hipMemcpyAsync(out + (size_t)off * (size_t)nnz, o.p, sizeof(int32_t) * (size_t)nb * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
        MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MMM_OK;
}

int mmm_compare_exposures(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr_a, const int32_t* term_a, const int32_t* count_a, const int64_t* doc_ptr_b,
                          const int32_t* term_b, const int32_t* count_b, const double* cat, const uint8_t* allowed, int B, int b0, uint64_t seed, uint32_t stream,
                          int key_bits, int maxiter, double tol, double* w_a, double* w_b, double* w_pool, double* stat, int32_t* count_ge, int32_t* count_sig,
                          int32_t* count_max, int8_t* status, double* unexplained, int64_t* iters, double* rep_stat)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    const char* who = "mmm_compare_exposures";
    MMM_CHECK(ctx, C >= 1 && V >= 1 && D >= 0 && cat, "%s: NULL argument, D < 0, C < 1 or V < 1", who);
    if (C > kCmMaxC) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: C = %d catalogue signatures (limit %d)", who, C, kCmMaxC);
    if (V > kCmMaxV)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: V = %d terms; a block keeps the pooled counts and its waves' count vectors in LDS, which holds at most V = %d", who, V, kCmMaxV);
    if (D > kDealMaxD) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: D = %d samples (limit 2^28: the sample shares a counter word with the tag)", who, D);
    MMM_CHECK(ctx, key_bits >= 1 && key_bits <= 32, "%s: key_bits = %d (1..32)", who, key_bits);
    MMM_CHECK(ctx, maxiter >= 1 && tol >= 0.0, "%s: maxiter = %d (>= 1), tol = %g (>= 0)", who, maxiter, tol);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0, "%s: B < 0 or b0 < 0", who);
    MMM_CHECK(ctx, (int64_t)b0 + (int64_t)B <= (int64_t)INT32_MAX, "%s: b0 + B exceeds 2^31 - 1", who);
    MMM_CHECK(ctx, stream < 0x80000000u, "%s: stream = %u (below 2^31)", who, stream);
    if (int rc = mmm_check_csr(ctx, who, D, V, doc_ptr_a, term_a, count_a)) return rc;
    if (int rc = mmm_check_csr(ctx, who, D, V, doc_ptr_b, term_b, count_b)) return rc;
    std::vector<int32_t> na((size_t)D), nb((size_t)D);
    if (int rc = mmm_doc_totals(ctx, who, D, doc_ptr_a, count_a, na.data())) return rc;
    if (int rc = mmm_doc_totals(ctx, who, D, doc_ptr_b, count_b, nb.data())) return rc;
    for (int d = 0; d < D; ++d)
        if ((int64_t)na[d] + (int64_t)nb[d] >= ((int64_t)1 << 31))
            return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: sample %d pools 2^31 or more mutations (a mutation's index is a 32-bit word: N_d < 2^31)", who, d);
    std::vector<double> P;           // the catalogue with rows normalised: mmm_refit_exposures' P
    if (int rc = mmm_normalise_rows(ctx, who, C, V, cat, P)) return rc;
    if (D == 0) return MMM_OK;
    MMM_CHECK(ctx, w_a && w_b && w_pool && stat && count_ge && count_sig && count_max && status && unexplained && iters, "%s: NULL output", who);
    const size_t DC = (size_t)D * C, Ds = (size_t)D;
    const bool want_rep = rep_stat && B > 0;

    // what is testable is known from the arguments: the host lists those samples, staged-row candidates first
    std::vector<int8_t> hst(Ds, 0);
    std::vector<int> nA(Ds, 0);
    int max_n = 0;
    size_t n_items = 0;
    for (int d = 0; d < D; ++d) {
        int n = C;
        if (allowed) {
            n = 0;
            for (int c = 0; c < C; ++c) n += allowed[(size_t)d * C + c] != 0;
        }
        nA[(size_t)d] = n;
        if (na[(size_t)d] == 0 || nb[(size_t)d] == 0 || n == 0) hst[(size_t)d] = 3;
        else { max_n = std::max(max_n, n); ++n_items; }
    }

    const int Cp = (C + 63) & ~63, cus = std::max(1, mmm_geo_cus(ctx));
    DevCsr ca, cb; DevBuf<int32_t> nd, cnt, itm; DevBuf<double> Pd, outd, rep; DevBuf<uint8_t> alw; DevBuf<unsigned long long> its; DevBuf<int> counter;
    MMM_HIP(ctx, nd.alloc(2 * Ds)); MMM_HIP(ctx, Pd.alloc(P.size())); MMM_HIP(ctx, outd.alloc(3 * DC + 4 * Ds)); MMM_HIP(ctx, its.alloc(Ds));
    MMM_HIP(ctx, cnt.alloc(Ds + 2 * DC)); MMM_HIP(ctx, counter.alloc(1)); MMM_HIP(ctx, itm.alloc(std::max<size_t>(n_items, 1)));
    if (allowed) MMM_HIP(ctx, alw.alloc(DC));
    if (int rc = ca.upload(ctx, D, doc_ptr_a, term_a, count_a)) return rc;
    if (int rc = cb.upload(ctx, D, doc_ptr_b, term_b, count_b)) return rc;
    MMM_HIP(ctx, hipMemcpyAsync(nd.p, na.data(), sizeof(int32_t) * Ds, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(nd.p + Ds, nb.data(), sizeof(int32_t) * Ds, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(Pd.p, P.data(), sizeof(double) * P.size(), hipMemcpyHostToDevice, ctx->stream));
    if (allowed) MMM_HIP(ctx, hipMemcpyAsync(alw.p, allowed, DC, hipMemcpyHostToDevice, ctx->stream));
    // what an untestable sample and a call without replicates leave behind
    MMM_HIP(ctx, hipMemsetAsync(outd.p, 0, sizeof(double) * outd.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(its.p, 0, sizeof(unsigned long long) * Ds, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * cnt.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));

    CmArgs a{};
    a.D = D; a.C = C; a.V = V; a.Cp = Cp; a.maxiter = maxiter; a.key_bits = key_bits; a.tol = tol;
    a.ptr_a = ca.ptr; a.term_a = ca.term; a.count_a = ca.count; a.ptr_b = cb.ptr; a.term_b = cb.term; a.count_b = cb.count;
    a.P = Pd.p; a.allowed = allowed ? alw.p : nullptr; a.na = nd.p; a.nb = nd.p + Ds;
    a.w_a = outd.p; a.w_b = outd.p + DC; a.w_pool = outd.p + 2 * DC; a.stat = outd.p + 3 * DC; a.t_obs = a.stat + Ds; a.ll_pool = a.t_obs + Ds;
    a.unexplained = a.ll_pool + Ds; a.iters = its.p; a.counter = counter.p;
    a.B = B; a.b0 = (uint32_t)b0; a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.count_ge = cnt.p; a.count_sig = cnt.p + Ds; a.count_max = cnt.p + Ds + DC;

    if (n_items) {
        // ---- replicate geometry first: it fixes the order of the item list (samples whose rows are staged come first)
        int P2 = 2;
        while (P2 < V) P2 <<= 1;
        const int Vh = (V + 1) / 2;
        const size_t fixed = sizeof(uint32_t) * (size_t)P2 + sizeof(double) * ((size_t)Vh + Cp + Cp / 2);
        const size_t pw = sizeof(double) * (size_t)cm_rep_doubles(Cp, V);
        int nw = 1;
        for (int t = kCmMaxWaves; t >= 1; t >>= 1)
            if (fixed + t * pw <= kCmLdsBlock) { nw = t; break; }
        // rows of P a block can stage beside nw waves' buffers (one double may pad the rows to 16 bytes)
        auto cap = [&](int t) { const size_t room = (kCmLdsBlock - fixed - t * pw) / sizeof(double); return room ? (int)((room - 1) / (size_t)V) : 0; };
        int rows_cap = 0;
        if (!mmm_off(ctx->tune, MMM_OFF_REFIT_LDS)) {
            if (nw == kCmMaxWaves && cap(nw) < max_n && cap(nw / 2) >= max_n) nw >>= 1;       // four waves with every sample's rows in LDS beat eight through L2
            rows_cap = cap(nw);
        }
        std::vector<int32_t> staged, direct;
        int rows = 0;
        for (int d = 0; d < D; ++d) {
            if (hst[(size_t)d] != 0) continue;
            if (nA[(size_t)d] <= rows_cap) { staged.push_back(d); rows = std::max(rows, nA[(size_t)d]); }
            else direct.push_back(d);
        }
        std::vector<int32_t> all(staged);
        all.insert(all.end(), direct.begin(), direct.end());
        MMM_HIP(ctx, hipMemcpyAsync(itm.p, all.data(), sizeof(int32_t) * all.size(), hipMemcpyHostToDevice, ctx->stream));
        a.items = itm.p; a.n_items = (int)all.size();

        // ---- observed phase: as many waves per block as their buffers leave room for; few samples: fewer, so that they spread over the CUs
        {
            const size_t po = sizeof(double) * (size_t)cm_obs_doubles(Cp, V);
            int ow = kCmMaxWaves;
            while (ow > 1 && ow * po > kCmLdsBlock) ow >>= 1;
            while (ow > 1 && ((int64_t)n_items + ow - 1) / ow < cus) ow >>= 1;
            const size_t lds = ow * po;
            const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(kCmMaxWaves / ow, (int64_t)(kCmLdsBlock / lds)));
            const unsigned grid = (unsigned)std::min<int64_t>(((int64_t)n_items + ow - 1) / ow, (int64_t)cus * per_cu);
            a.wave_doubles = cm_obs_doubles(Cp, V);
            if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)k_compare_obs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_compare_obs, dim3(grid), dim3(64 * ow), lds, ctx->stream, a);
            MMM_LAUNCH_CHECK(ctx);
        }
        // ---- replicate phase
        if (B > 0) {
            if (want_rep) {
                MMM_HIP(ctx, rep.alloc((size_t)B * Ds));
                MMM_HIP(ctx, hipMemsetAsync(rep.p, 0, sizeof(double) * (size_t)B * Ds, ctx->stream));
            }
            a.P2 = P2; a.rep = want_rep ? rep.p : nullptr; a.wave_doubles = cm_rep_doubles(Cp, V);
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
                a.stage_doubles = part ? 0 : (int)(((size_t)rows * V + 1) & ~(size_t)1);
                const size_t lds = fixed + sizeof(double) * (size_t)a.stage_doubles + nw * pw;
                auto kern = part ? k_compare_rep<false> : k_compare_rep<true>;
                if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(kern, dim3((unsigned)n, (unsigned)((B + rpb - 1) / rpb)), dim3(64 * nw), lds, ctx->stream, a);
                MMM_LAUNCH_CHECK(ctx);
            }
        }
    }
    // staged on the host so that a failing copy leaves the caller's arrays as they were
    std::vector<double> ho(outd.n), hr(want_rep && rep.p ? (size_t)B * Ds : 0);
    std::vector<int32_t> hc(cnt.n);
    std::vector<unsigned long long> hi(Ds);
    MMM_HIP(ctx, hipMemcpyAsync(ho.data(), outd.p, sizeof(double) * ho.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hc.data(), cnt.p, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hi.data(), its.p, sizeof(unsigned long long) * Ds, hipMemcpyDeviceToHost, ctx->stream));
    if (hr.size()) MMM_HIP(ctx, hipMemcpyAsync(hr.data(), rep.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(w_a, ho.data(), sizeof(double) * DC); memcpy(w_b, ho.data() + DC, sizeof(double) * DC); memcpy(w_pool, ho.data() + 2 * DC, sizeof(double) * DC);
    memcpy(stat, ho.data() + 3 * DC, sizeof(double) * Ds);
    memcpy(unexplained, ho.data() + 3 * DC + 3 * Ds, sizeof(double) * Ds);
    memcpy(count_ge, hc.data(), sizeof(int32_t) * Ds);
    memcpy(count_sig, hc.data() + Ds, sizeof(int32_t) * DC); memcpy(count_max, hc.data() + Ds + DC, sizeof(int32_t) * DC);
    memcpy(status, hst.data(), Ds);
    for (size_t d = 0; d < Ds; ++d) iters[d] = (int64_t)hi[d];
    if (want_rep) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int b = 0; b < B; ++b)
            for (size_t d = 0; d < Ds; ++d) rep_stat[(size_t)b * Ds + d] = hst[d] == 0 ? hr[(size_t)b * Ds + d] : nan;
    }
    return MMM_OK;
}

} // extern "C"
