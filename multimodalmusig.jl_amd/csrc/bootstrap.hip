// bootstrap.hip -- the two pieces of a non-parametric bootstrap of the exposures that have no counterpart in the reference:
//   mmm_resample_counts      B multinomial resamples of every document of a CSR corpus (Philox4x32-10 counters, integer inverse CDF)
//   mmm_replicate_summary    mean / sd / quantiles over B replicates of n values
// The frozen-topic passes between the two are the existing ones (mmm_lda_infer / mmm_ctm_infer on the stacked corpus); the definitions the
// kernels restate are in include/mmmusig.h and DESIGN.md ("Bootstrap of the exposures").  Everything here is integer arithmetic or a
// fixed-order double sum: the same arguments give the same bits on every run and every launch geometry.
#include "mmm_internal.h"
#include "mmm_philox.h"

namespace {

constexpr int kRsWaves = 4;        // waves per block; each takes one replicate of the block's document at a time
constexpr int kRsMaxW = 2048;      // longest row kept in LDS: 4 B x 2048 x (1 prefix row + kRsWaves histograms) = 40 KiB per block at most;
                                   // a launch asks for the longest row of ITS corpus (96-term rows: 1.9 KiB, occupancy then set by registers)

// One wave draws the N categorical draws of one (document, replicate) pair, 64 Philox blocks (256 draws) per step, and counts them into
// hist[0..W) with integer atomics.  cum[0..W): inclusive prefix sums, cum[W-1] = N; the entry of a draw r is the first e with cum[e] > r
// = the number of e with cum[e] <= r.
// LDS rows: cum is padded with 0xffffffff to a power of two 2 * half >= W, so the search is the same log2 steps for every lane, without
// bound checks, and the four draws of a lane advance side by side (four independent ds_read_b32 in flight per step).
__device__ __forceinline__ void rs_draw_row_lds(int lane, int half, uint32_t N, const uint32_t* cum, int* hist, uint32_t d, uint32_t b, uint32_t stream,
                                                uint32_t k0, uint32_t k1)
{
    const uint32_t nblk = (N + 3u) >> 2;                       // N < 2^31
    for (uint32_t i4 = (uint32_t)lane; i4 < nblk; i4 += 64u) {
        uint32_t u[4], r[4];
        int pos[4];
        philox4x32_10(i4, d, b, stream, k0, k1, u);
#pragma unroll
        for (int j = 0; j < 4; ++j) { r[j] = __umulhi(u[j], N); pos[j] = 0; }      // (u N) >> 32 < N
        for (int step = half; step > 0; step >>= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (cum[pos[j] + step - 1] <= r[j]) pos[j] += step;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4u * i4 + (uint32_t)j < N) atomicAdd(&hist[pos[j]], 1);              // cum[W-1] = N > r: pos <= W - 1
    }
}

// rows beyond the LDS budget: the same draws, bisection over the global prefix sums, counts straight into the pre-zeroed output row
__device__ __forceinline__ void rs_draw_row_global(int lane, int W, uint32_t N, const uint32_t* __restrict__ cum, int32_t* hist, uint32_t d, uint32_t b,
                                                   uint32_t stream, uint32_t k0, uint32_t k1)
{
    const uint32_t nblk = (N + 3u) >> 2;
    for (uint32_t i4 = (uint32_t)lane; i4 < nblk; i4 += 64u) {
        uint32_t u[4];
        philox4x32_10(i4, d, b, stream, k0, k1, u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4u * i4 + (uint32_t)j >= N) break;
            const uint32_t r = __umulhi(u[j], N);
            int lo = 0, hi = W - 1;                            // first e with cum[e] > r; cum[W-1] = N > r, so it exists
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cum[mid] > r) hi = mid; else lo = mid + 1;
            }
            atomicAdd(&hist[lo], 1);
        }
    }
}

// grid (D, replicate chunks); block = kRsWaves waves.  out[b * nnz + e]: replicate b0 + b.  Rows longer than lds_w (<= kRsMaxW) count
// straight into `out`, which the host has zeroed for them.
__global__ __launch_bounds__(64 * kRsWaves) void k_resample_counts(const int64_t* __restrict__ doc_ptr, const uint32_t* __restrict__ cum, int64_t nnz, int B,
                                                                   uint32_t b0, int reps_per_block, uint32_t k0, uint32_t k1, uint32_t stream,
                                                                   int lds_w, int lds_p, int32_t* __restrict__ out)
{
    extern __shared__ uint32_t s_dyn[];                        // [lds_p] prefix sums (lds_p: lds_w rounded up to a power of two), then
    uint32_t* s_cum = s_dyn;                                   // kRsWaves histograms of lds_w counts
    int* s_hist = (int*)(s_dyn + lds_p) + (threadIdx.x >> 6) * lds_w;       // this wave's histogram
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t d = blockIdx.x;
    const int64_t e0 = doc_ptr[d];
    const int W = (int)(doc_ptr[d + 1] - e0);
    if (W == 0) return;
    const uint32_t* cg = cum + e0;
    const uint32_t N = cg[W - 1];
    const int bbeg = (int)blockIdx.y * reps_per_block, bend = min(B, bbeg + reps_per_block);
    if (W <= lds_w) {
        int half = 1;                                           // 2 * half: the power of two the row is padded to
        while (2 * half < W) half <<= 1;
        if (W == 1) half = 0;
        for (int e = tid; e < 2 * half || e < W; e += 64 * kRsWaves) s_cum[e] = e < W ? cg[e] : 0xffffffffu;
        for (int e = lane; e < W; e += 64) s_hist[e] = 0;
        __syncthreads();
        for (int bb = bbeg; bb < bend; bb += kRsWaves) {       // block-uniform trip count: the barriers below are reached by every wave
            const int b = bb + wave;
            if (b < bend && N) rs_draw_row_lds(lane, half, N, s_cum, s_hist, d, b0 + (uint32_t)b, stream, k0, k1);
            __syncthreads();
            if (b < bend) {
                int32_t* row = out + (size_t)b * (size_t)nnz + e0;
                for (int e = lane; e < W; e += 64) { row[e] = s_hist[e]; s_hist[e] = 0; }
            }
            __syncthreads();
        }
    } else if (N) {
        for (int b = bbeg + wave; b < bend; b += kRsWaves)
            rs_draw_row_global(lane, W, N, cg, out + (size_t)b * (size_t)nnz + e0, d, b0 + (uint32_t)b, stream, k0, k1);
    }
}

// ---- summary over replicates ---------------------------------------------------------------------------------------------------------------
constexpr int kSumElems = 4096;    // values a block sorts at once: C = 4096 / P columns of P = max(16, B rounded up to a power of two) slots
constexpr int kSumThreads = 256;

// x[b * n + j].  A block takes C adjacent columns (rows of C doubles are read together), keeps each in LDS with a stride of P + 1 doubles
// (adjacent columns two banks apart), sums it in replicate order (one lane per column), then sorts all of them with one bitonic network
// (slots b >= B hold +inf) and interpolates the quantiles.
__global__ __launch_bounds__(kSumThreads) void k_replicate_summary(int B, size_t n, int P, const double* __restrict__ x, int nq, const double* __restrict__ q,
                                                                   double* __restrict__ mean, double* __restrict__ sd, double* __restrict__ quant)
{
    __shared__ double s[kSumElems + kSumElems / 16];
    __shared__ int s_nan[kSumElems / 16];
    const int tid = threadIdx.x;
    const int C = kSumElems / P, S = P + 1;
    const size_t j0 = (size_t)blockIdx.x * (size_t)C;
    if (tid < C) s_nan[tid] = 0;
    __syncthreads();
    for (int idx = tid; idx < kSumElems; idx += kSumThreads) {
        const int c = idx % C, b = idx / C;
        double v = __longlong_as_double(0x7ff0000000000000ll);
        if (b < B && j0 + c < n) {
            v = x[(size_t)b * n + j0 + c];
            if (v != v) s_nan[c] = 1;
        }
        s[c * S + b] = v;
    }
    __syncthreads();
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    if (tid < C && j0 + tid < n) {
        const double* col = s + tid * S;
        double sum = 0.0;
#pragma unroll 8
        for (int b = 0; b < B; ++b) sum += col[b];
        const double m = sum / (double)B;
        double ss = 0.0;
#pragma unroll 8
        for (int b = 0; b < B; ++b) { const double t = col[b] - m; ss += t * t; }
        const bool bad = s_nan[tid] != 0;
        mean[j0 + tid] = bad ? nanv : m;
        sd[j0 + tid] = bad ? nanv : (B > 1 ? sqrt(ss / (double)(B - 1)) : 0.0);
    }
    if (nq == 0) return;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < kSumElems / 2; t += kSumThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));       // lower element of pair t (bit j clear); its partner is i + j, same column
                const int ii = i & (P - 1);
                const int a = (i / P) * S + ii;
                const double va = s[a], vb = s[a + j];
                const bool up = (ii & k) == 0;
                if (up ? (va > vb) : (va < vb)) { s[a] = vb; s[a + j] = va; }
            }
            __syncthreads();
        }
    }
    for (int idx = tid; idx < nq * C; idx += kSumThreads) {
        const int c = idx % C, i = idx / C;
        if (j0 + c >= n) continue;
        const double h = (double)(B - 1) * q[i];
        int lo = (int)floor(h);
        lo = lo < 0 ? 0 : (lo > B - 1 ? B - 1 : lo);
        const int hi = lo + 1 < B ? lo + 1 : B - 1;
        const double a = s[c * S + lo], b = s[c * S + hi], f = h - (double)lo;
        const double v = (f == 0.0 || a == b) ? a : a + f * (b - a);
        quant[(size_t)i * n + j0 + c] = s_nan[c] ? nanv : v;
    }
}

} // namespace

static_assert(kSumElems == MMM_SUMMARY_MAX_B, "mmm_internal.h states the limit of the summary");

// the summary on device buffers (mmm_internal.h): the launch of mmm_replicate_summary, also used by the consensus of match.hip
int mmm_replicate_summary_dev(mmm_ctx* ctx, int B, size_t n, const double* x, int nq, const double* q, double* out)
{
    int P = 16;
    while (P < B) P <<= 1;
    const size_t C = (size_t)(kSumElems / P), blocks = (n + C - 1) / C;
    if (blocks > 0x7fffffffull) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_replicate_summary: n = %zu columns need more than 2^31 - 1 blocks", n);
    hipLaunchKernelGGL(k_replicate_summary, dim3((unsigned)blocks), dim3(kSumThreads), 0, ctx->stream, B, n, P, x, nq, q, out, out + n, out + 2 * n);
    MMM_LAUNCH_CHECK(ctx);
    return MMM_OK;
}

extern "C" {

int mmm_resample_counts(mmm_ctx* ctx, int D, const int64_t* doc_ptr, const int32_t* count, int B, int b0, uint64_t seed, uint32_t stream, int32_t* out)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, D >= 0 && doc_ptr && B >= 0 && b0 >= 0, "mmm_resample_counts: D < 0, doc_ptr == NULL, B < 0 or b0 < 0");
    MMM_CHECK(ctx, (int64_t)b0 + (int64_t)B <= (int64_t)INT32_MAX, "mmm_resample_counts: b0 + B exceeds 2^31 - 1");
    MMM_CHECK(ctx, doc_ptr[0] == 0, "mmm_resample_counts: doc_ptr[0] != 0");
    for (int d = 0; d < D; ++d) MMM_CHECK(ctx, doc_ptr[d + 1] >= doc_ptr[d], "mmm_resample_counts: doc_ptr decreases at document %d", d);
    const int64_t nnz = doc_ptr[D];
    MMM_CHECK(ctx, nnz == 0 || count, "mmm_resample_counts: count == NULL");
    // inclusive prefix sums per document (what the inverse CDF searches); O(nnz) beside the B * sum N_d draws of the kernel
    std::vector<uint32_t> cum((size_t)nnz);
    bool any_long = false;
    int64_t lds_w = 1;                                            // longest row that stays in LDS
    for (int d = 0; d < D; ++d) {
        const int64_t w = doc_ptr[d + 1] - doc_ptr[d];
        if (w >= ((int64_t)1 << 31)) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_resample_counts: document %d has %lld entries (limit 2^31 - 1)", d, (long long)w);
        any_long |= w > kRsMaxW;
        if (w <= kRsMaxW) lds_w = std::max(lds_w, w);
        uint64_t s = 0;
        for (int64_t e = doc_ptr[d]; e < doc_ptr[d + 1]; ++e) {
            MMM_CHECK(ctx, count[e] >= 0, "mmm_resample_counts: entry %lld has count %d", (long long)e, count[e]);
            s += (uint64_t)count[e];
            if (s >= ((uint64_t)1 << 31))
                return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_resample_counts: document %d holds 2^31 or more counts (the integer draw needs N_d < 2^31)", d);
            cum[(size_t)e] = (uint32_t)s;
        }
    }
    if (B == 0 || nnz == 0) return MMM_OK;
    int64_t lds_p = 1;
    while (lds_p < lds_w) lds_p <<= 1;
    MMM_CHECK(ctx, out, "mmm_resample_counts: out == NULL");
    // replicates go through a device buffer of at most 2^28 counts (1 GiB) at a time
    const int Bc = (int)std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)1 << 28) / nnz));
    DevBuf<int64_t> dp; DevBuf<uint32_t> cm; DevBuf<int32_t> o;
    MMM_HIP(ctx, dp.alloc((size_t)D + 1)); MMM_HIP(ctx, cm.alloc((size_t)nnz)); MMM_HIP(ctx, o.alloc((size_t)Bc * (size_t)nnz));
    MMM_HIP(ctx, hipMemcpyAsync(dp.p, doc_ptr, sizeof(int64_t) * ((size_t)D + 1), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(cm.p, cum.data(), sizeof(uint32_t) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
    for (int off = 0; off < B; off += Bc) {
        const int nb = std::min(Bc, B - off);
        const size_t bytes = sizeof(int32_t) * (size_t)nb * (size_t)nnz;
        if (any_long) MMM_HIP(ctx, hipMemsetAsync(o.p, 0, bytes, ctx->stream));
        int rpb = kRsWaves;                                       // one replicate per wave: the longest document's last block ends soonest
        while ((nb + rpb - 1) / rpb > 65535) rpb *= 2;
        hipLaunchKernelGGL(k_resample_counts, dim3((unsigned)D, (unsigned)((nb + rpb - 1) / rpb)), dim3(64 * kRsWaves), sizeof(uint32_t) * (size_t)(lds_p + lds_w * kRsWaves), ctx->stream, dp.p, cm.p, nnz, nb,
                           (uint32_t)(b0 + off), rpb, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), stream, (int)lds_w, (int)lds_p, o.p);
        MMM_LAUNCH_CHECK(ctx);
        MMM_HIP(ctx, hipMemcpyAsync(out + (size_t)off * (size_t)nnz, o.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MMM_OK;
}

int mmm_replicate_summary(mmm_ctx* ctx, int B, size_t n, const double* x, int nq, const double* q, double* mean, double* sd, double* quant)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, B >= 1 && nq >= 0 && (n == 0 || x) && (nq == 0 || q), "mmm_replicate_summary: B < 1, nq < 0 or NULL x / q");
    for (int i = 0; i < nq; ++i) MMM_CHECK(ctx, q[i] >= 0.0 && q[i] <= 1.0, "mmm_replicate_summary: q[%d] = %g is outside [0, 1]", i, q[i]);
    if (B > kSumElems)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_replicate_summary: B = %d replicates; a column is sorted in LDS, which holds at most %d", B, kSumElems);
    if (!quant) nq = 0;
    if (n == 0 || (!mean && !sd && nq == 0)) return MMM_OK;
    DevBuf<double> xd, qd, od;
    MMM_HIP(ctx, xd.alloc((size_t)B * n)); MMM_HIP(ctx, qd.alloc((size_t)nq)); MMM_HIP(ctx, od.alloc((2 + (size_t)nq) * n));
    MMM_HIP(ctx, hipMemcpyAsync(xd.p, x, sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice, ctx->stream));
    if (nq) MMM_HIP(ctx, hipMemcpyAsync(qd.p, q, sizeof(double) * (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = mmm_replicate_summary_dev(ctx, B, n, xd.p, nq, qd.p, od.p)) return rc;
    if (mean) MMM_HIP(ctx, hipMemcpyAsync(mean, od.p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (sd) MMM_HIP(ctx, hipMemcpyAsync(sd, od.p + n, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (nq) MMM_HIP(ctx, hipMemcpyAsync(quant, od.p + 2 * n, sizeof(double) * (size_t)nq * n, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MMM_OK;
}

} // extern "C"
