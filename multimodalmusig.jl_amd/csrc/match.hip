// match.hip -- matching signatures to a catalogue and across the replicas of a restart batch (no counterpart in the reference, whose README
// leaves the step to the user: "compute the cosine distance between the inferred and COSMIC signatures, then use a linear sum assignment
// solver to find the optimal set of unique matches"):
//   k_signature_cosine    S[r][k][c], the cosine of signature k of replica r and catalogue row c
//   k_signature_assign    per replica, the injective k -> c that maximises the summed cosine (shortest augmenting paths, one wave each)
//   k_align_normalise     every replica's signatures as probabilities, in the labelling of a reference replica (for the consensus)
// The definitions are in include/mmmusig.h and DESIGN.md section 4.11.  Every sum has a fixed order and the assignment uses +, - and
// compares only: the same arguments give the same bits on every run, whatever R and however the replicas are chunked.
#include "mmm_internal.h"
#include "dev_math.h"

namespace {

constexpr int kCosWaves = 4;       // waves per block of k_signature_cosine: one signature each
constexpr int kCosCT = 16;         // catalogue rows per LDS tile
constexpr int kCosVC = 128;        // terms per LDS tile: 16 x 128 doubles = 16 KiB per block
constexpr int kAssignStage = 2048; // k_signature_assign keeps the replica's S in LDS when K * C is at most this (16 KiB)
constexpr size_t kMatchSBudget = (size_t)1 << 22;    // doubles of S held on the device at a time (32 MiB): replicas go through in chunks
constexpr size_t kMatchUpBudget = (size_t)1 << 24;   // doubles of caller signatures uploaded at a time (128 MiB)

static_assert(kCosCT % kCosWaves == 0 && kCosVC % 64 == 0 && kCosCT <= 64, "tile shape");

// (wave_sum_fixed, the one order of every cross-lane sum here, is in dev_math.h: decompose.hip shares it)
// Element (k, v) of replica r is sig[r][k * sk + v * sv]; catalogue row c is cat[c * ck + v * cv].  grid (ceil(K / kCosWaves), R).
// A wave takes one signature and walks the catalogue in tiles of kCosCT rows; the block stages a tile kCosVC terms at a time in LDS.  Lane l
// owns the terms l, l + 64, ... (ascending), so with sv = 1 (both handle layouts and the array form) a wave's loads are contiguous.
// Order of every sum (dot, sum of squares of either side): per lane over its terms ascending, then wave_sum_fixed -- a function of V alone.
__global__ __launch_bounds__(64 * kCosWaves) void k_signature_cosine(int K, int C, int V, const double* const* __restrict__ sig, size_t sk, size_t sv,
                                                                     const double* __restrict__ cat, size_t ck, size_t cv, double* __restrict__ S)
{
    __shared__ double s_cat[kCosCT * kCosVC];
    __shared__ double s_cn[kCosCT];                            // the tile's sums of squares
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r = blockIdx.y;
    const int k = (int)blockIdx.x * kCosWaves + wave;
    const bool active = k < K;                                 // (an idle wave still helps to stage the tiles and reaches every barrier)
    const double* row = sig[r] + (size_t)(active ? k : 0) * sk;
    constexpr int Q = kCosCT / kCosWaves;
    for (int c0 = 0; c0 < C; c0 += kCosCT) {
        double acc[kCosCT], cc[Q], ss = 0.0;
#pragma unroll
        for (int i = 0; i < kCosCT; ++i) acc[i] = 0.0;
#pragma unroll
        for (int i = 0; i < Q; ++i) cc[i] = 0.0;
        for (int v0 = 0; v0 < V; v0 += kCosVC) {
            __syncthreads();                                   // the previous chunk has been consumed
            for (int idx = tid; idx < kCosCT * kCosVC; idx += 64 * kCosWaves) {
                const int ci = idx / kCosVC, vi = idx % kCosVC;
                const int c = c0 + ci, v = v0 + vi;
                s_cat[idx] = (c < C && v < V) ? cat[(size_t)c * ck + (size_t)v * cv] : 0.0;      // (+ 0.0 leaves a non-negative sum as it is)
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kCosVC / 64; ++j) {
                const int v = v0 + 64 * j + lane;
                const double x = v < V ? row[(size_t)v * sv] : 0.0;
                ss += x * x;
#pragma unroll
                for (int ci = 0; ci < kCosCT; ++ci) acc[ci] += x * s_cat[ci * kCosVC + 64 * j + lane];
#pragma unroll
                for (int i = 0; i < Q; ++i) { const double y = s_cat[(wave * Q + i) * kCosVC + 64 * j + lane]; cc[i] += y * y; }
            }
        }
        ss = wave_sum_fixed(ss);
#pragma unroll
        for (int i = 0; i < Q; ++i) { const double t = wave_sum_fixed(cc[i]); if (lane == i) s_cn[wave * Q + i] = t; }
        double mine = 0.0;
#pragma unroll
        for (int ci = 0; ci < kCosCT; ++ci) { const double t = wave_sum_fixed(acc[ci]); if (lane == ci) mine = t; }
        __syncthreads();                                       // s_cn complete (its next writes lie behind the next tile's barriers)
        if (active && lane < kCosCT && c0 + lane < C) {
            const double cn = s_cn[lane];
            S[(r * (size_t)K + (size_t)k) * (size_t)C + (size_t)(c0 + lane)] = (ss == 0.0 || cn == 0.0) ? 0.0 : mine / (sqrt(ss) * sqrt(cn));
        }
    }
}

// orders the LDS traffic of the lanes of ONE wave (the hardware runs a wave's DS instructions in order; this keeps the compiler from moving
// them across the point).  No s_barrier: a block is one wave.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__host__ __device__ inline size_t assign_lds_bytes(int K, int C, bool stage)
{
    return sizeof(double) * ((size_t)2 * C + K + (stage ? (size_t)K * C : 0)) + sizeof(short) * ((size_t)2 * C + 2 * (size_t)K);
}

// One wave (= one block) per replica: rectangular linear sum assignment on W = -S by shortest augmenting paths (Crouse 2016, Algorithm 1),
// with the evaluation order of include/mmmusig.h.  Lane l owns the columns l, l + 64, ...: their spc / v / path entries are written by it
// alone and its part of the scanned set is a bit mask in a register (C <= 1024: 16 columns per lane).  u, col4row, row4col and the list of
// scanned rows are shared through the wave's LDS.  A replica whose S holds a NaN has no smallest column: it gets assign = -1 (the host
// reports it) instead of an index nobody checked.
__global__ __launch_bounds__(64) void k_signature_assign(int K, int C, int stage, const double* __restrict__ S, int32_t* __restrict__ assign, double* __restrict__ matched)
{
    extern __shared__ double s_dyn[];
    const int lane = threadIdx.x;
    const size_t r = blockIdx.x;
    const double* Sr = S + r * (size_t)K * (size_t)C;
    double* spc = s_dyn;                   // [C] shortest path cost to column c in the current search
    double* vd = spc + C;                  // [C] column duals
    double* u = vd + C;                    // [K] row duals
    double* sS = u + K;                    // [K * C] the replica's S (stage != 0)
    short* path = (short*)(sS + (stage ? (size_t)K * C : 0));      // [C] row from which column c was reached
    short* row4col = path + C;             // [C]
    short* col4row = row4col + C;          // [K]
    short* srl = col4row + K;              // [K] rows scanned in the current search, in order (srl[0] = the inserted row)
    const int T = (C + 63) >> 6;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int c = lane; c < C; c += 64) { vd[c] = 0.0; row4col[c] = -1; }
    for (int k = lane; k < K; k += 64) { u[k] = 0.0; col4row[k] = -1; }
    if (stage) for (int i = lane; i < K * C; i += 64) sS[i] = Sr[i];
    wave_sync();
    bool ok = true;
    for (int cur = 0; cur < K && ok; ++cur) {
        unsigned scanned = 0;              // bit t: column lane + 64 t is in the scanned set
        for (int t = 0; t < T; ++t) { const int c = lane + 64 * t; if (c < C) spc[c] = inf; }
        double minval = 0.0;
        int i = cur, nsr = 0, sink = -1;
        while (sink < 0) {
            if (lane == 0) srl[nsr] = (short)i;
            ++nsr;
            const double ui = u[i];
            double bv = inf; int bc = 0x7fffffff;
            for (int t = 0; t < T; ++t) {
                const int c = lane + 64 * t;
                if (c < C && !((scanned >> t) & 1u)) {
                    const double w = -(stage ? sS[i * C + c] : Sr[(size_t)i * C + c]);
                    const double red = ((minval + w) - ui) - vd[c];
                    double s = spc[c];
                    if (red < s) { spc[c] = red; path[c] = (short)i; s = red; }
                    if (s < bv) { bv = s; bc = c; }            // columns ascending: a tie keeps the lower one
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {           // argmin of the pair (spc, c), lexicographic: independent of the lane order
                const double ov = __shfl_xor(bv, off, 64); const int oc = __shfl_xor(bc, off, 64);
                if (ov < bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
            }
            const int j = __builtin_amdgcn_readfirstlane(bc);
            if (j >= C) { ok = false; break; }                 // no comparable cost left: a NaN in S
            minval = bv;
            if (lane == (j & 63)) scanned |= 1u << (j >> 6);
            const int rj = __builtin_amdgcn_readfirstlane((int)row4col[j]);
            if (rj < 0) sink = j; else i = rj;
        }
        if (!ok) break;
        wave_sync();
        for (int n = lane; n < nsr; n += 64) {                 // duals of the scanned rows ...
            const int ii = srl[n];
            if (ii == cur) u[ii] += minval; else u[ii] += minval - spc[col4row[ii]];
        }
        for (int t = 0; t < T; ++t)                            // ... and columns
            if ((scanned >> t) & 1u) { const int c = lane + 64 * t; vd[c] -= minval - spc[c]; }
        wave_sync();
        int j = sink;                                          // augment along the path (every lane does the same writes)
        while (true) {
            const int ii = __builtin_amdgcn_readfirstlane((int)path[j]);
            row4col[j] = (short)ii;
            const int nxt = __builtin_amdgcn_readfirstlane((int)col4row[ii]);
            col4row[ii] = (short)j;
            j = nxt;
            if (ii == cur) break;
        }
        wave_sync();
    }
    for (int k = lane; k < K; k += 64) {
        const int a = ok ? (int)col4row[k] : -1;
        assign[r * (size_t)K + k] = a;
        matched[r * (size_t)K + k] = ok ? Sr[(size_t)k * C + a] : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// grid (K, R), one wave per signature: P[r][assign[r][k]][v] = sig[r][k][v] / sum_v sig[r][k][v].  The sum runs in index order (64 terms are
// loaded together, then added one lane after the other); a zero row stays zero.
__global__ __launch_bounds__(64) void k_align_normalise(int K, int V, const double* const* __restrict__ sig, size_t sk, size_t sv, const int32_t* __restrict__ assign,
                                                        double* __restrict__ P)
{
    const int lane = threadIdx.x, k = blockIdx.x;
    const size_t r = blockIdx.y;
    const double* row = sig[r] + (size_t)k * sk;
    const int a = assign[r * (size_t)K + k];
    if (a < 0 || a >= K) return;                               // (the host has refused such a replica already)
    double s = 0.0;
    for (int v0 = 0; v0 < V; v0 += 64) {
        const double x = v0 + lane < V ? row[(size_t)(v0 + lane) * sv] : 0.0;      // (+ 0.0 leaves a non-negative sum as it is)
#pragma unroll
        for (int j = 0; j < 64; ++j) s += wave_readlane(x, j);
    }
    double* out = P + (r * (size_t)K + (size_t)a) * (size_t)V;
    for (int v = lane; v < V; v += 64) out[v] = s == 0.0 ? 0.0 : row[(size_t)v * sv] / s;
}

// the first entry of x[0..n) that is negative or not finite (n: none)
size_t first_bad(const double* x, size_t n)
{
    for (size_t i = 0; i < n; ++i) if (!(x[i] >= 0.0) || !std::isfinite(x[i])) return i;
    return n;
}

// Cosine (and assignment, when d_assign != NULL) of the R replicas h_tab[0..R) (device pointers) against the device catalogue; S goes
// through a buffer of at most kMatchSBudget doubles.  d_assign / d_matched: device, [R][K]; hS: host [R][K][C] or NULL.  Ends synchronised.
int match_run(mmm_ctx* ctx, int R, int K, int C, int V, const double* const* h_tab, size_t sk, size_t sv, const double* d_cat, size_t ck, size_t cv,
              int32_t* d_assign, double* d_matched, double* hS)
{
    if (R == 0) return MMM_OK;
    const size_t KC = (size_t)K * (size_t)C;
    const int Rc = (int)std::max<size_t>(1, std::min<size_t>({(size_t)R, kMatchSBudget / KC, (size_t)65535}));
    DevBuf<const double*> tab; DevBuf<double> S;
    MMM_HIP(ctx, tab.alloc((size_t)R)); MMM_HIP(ctx, S.alloc((size_t)Rc * KC));
    MMM_HIP(ctx, hipMemcpyAsync(tab.p, h_tab, sizeof(const double*) * (size_t)R, hipMemcpyHostToDevice, ctx->stream));
    const bool stage = KC <= (size_t)kAssignStage;
    const size_t lds = assign_lds_bytes(K, C, stage);
    for (int off = 0; off < R; off += Rc) {
        const int nb = std::min(Rc, R - off);
        hipLaunchKernelGGL(k_signature_cosine, dim3((unsigned)((K + kCosWaves - 1) / kCosWaves), (unsigned)nb), dim3(64 * kCosWaves), 0, ctx->stream, K, C, V,
                           (const double* const*)(tab.p + off), sk, sv, d_cat, ck, cv, S.p);
        MMM_LAUNCH_CHECK(ctx);
        if (d_assign) {
            hipLaunchKernelGGL(k_signature_assign, dim3((unsigned)nb), dim3(64), lds, ctx->stream, K, C, stage ? 1 : 0, (const double*)S.p, d_assign + (size_t)off * K,
                               d_matched + (size_t)off * K);
            MMM_LAUNCH_CHECK(ctx);
        }
        if (hS) MMM_HIP(ctx, hipMemcpyAsync(hS + (size_t)off * KC, S.p, sizeof(double) * (size_t)nb * KC, hipMemcpyDeviceToHost, ctx->stream));
    }
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MMM_OK;
}

int check_shape(mmm_ctx* ctx, const char* who, int R, int K, int C, int V, bool assign)
{
    MMM_CHECK(ctx, R >= 0 && K >= 1 && C >= 1 && V >= 1, "%s: R = %d, K = %d, C = %d, V = %d (R >= 0, the others >= 1)", who, R, K, C, V);
    if (!assign) return MMM_OK;
    MMM_CHECK(ctx, K <= C, "%s: K = %d signatures cannot be matched one to one to C = %d catalogue rows (K <= C)", who, K, C);
    if (C > MMM_MATCH_MAX_C)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: C = %d catalogue rows; the assignment keeps its column arrays in one wave's LDS, which holds at most %d", who, C,
                        MMM_MATCH_MAX_C);
    return MMM_OK;
}

int check_values(mmm_ctx* ctx, const char* who, const char* what, const double* x, size_t n)
{
    const size_t bad = first_bad(x, n);
    MMM_CHECK(ctx, bad == n, "%s: %s[%zu] = %g is negative or not finite", who, what, bad, bad < n ? x[bad] : 0.0);
    return MMM_OK;
}

int check_assigned(mmm_ctx* ctx, const char* who, const int32_t* assign, int R, int K)
{
    for (int r = 0; r < R; ++r)
        MMM_CHECK(ctx, assign[(size_t)r * K] >= 0, "%s: the similarities of replica %d are not all finite (a NaN or Inf in its table): no assignment", who, r);
    return MMM_OK;
}

// the array forms: caller signatures go up kMatchUpBudget doubles at a time
int match_arrays(mmm_ctx* ctx, const char* who, int R, int K, int C, int V, const double* sig, const double* cat, int32_t* assign, double* matched, double* S,
                 bool do_assign)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = check_shape(ctx, who, R, K, C, V, do_assign)) return rc;
    MMM_CHECK(ctx, cat && (R == 0 || sig), "%s: NULL sig or cat", who);
    MMM_CHECK(ctx, R == 0 || (do_assign ? (assign && matched) : S != nullptr), "%s: NULL output", who);
    const size_t KV = (size_t)K * (size_t)V;
    if (int rc = check_values(ctx, who, "cat", cat, (size_t)C * (size_t)V)) return rc;
    if (int rc = check_values(ctx, who, "sig", sig, (size_t)R * KV)) return rc;
    if (R == 0) return MMM_OK;
    const int Ru = (int)std::max<size_t>(1, std::min<size_t>((size_t)R, kMatchUpBudget / KV));
    DevBuf<double> sd, cd, md; DevBuf<int32_t> ad;
    MMM_HIP(ctx, sd.alloc((size_t)Ru * KV)); MMM_HIP(ctx, cd.alloc((size_t)C * (size_t)V));
    if (do_assign) { MMM_HIP(ctx, ad.alloc((size_t)Ru * K)); MMM_HIP(ctx, md.alloc((size_t)Ru * K)); }
    MMM_HIP(ctx, hipMemcpyAsync(cd.p, cat, sizeof(double) * (size_t)C * (size_t)V, hipMemcpyHostToDevice, ctx->stream));
    std::vector<const double*> tab((size_t)Ru);
    for (int i = 0; i < Ru; ++i) tab[(size_t)i] = sd.p + (size_t)i * KV;
    for (int off = 0; off < R; off += Ru) {
        const int nb = std::min(Ru, R - off);
        MMM_HIP(ctx, hipMemcpyAsync(sd.p, sig + (size_t)off * KV, sizeof(double) * (size_t)nb * KV, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = match_run(ctx, nb, K, C, V, tab.data(), (size_t)V, 1, cd.p, (size_t)V, 1, do_assign ? ad.p : nullptr, md.p,
                               S ? S + (size_t)off * K * (size_t)C : nullptr))
            return rc;
        if (do_assign) {
            MMM_HIP(ctx, hipMemcpyAsync(assign + (size_t)off * K, ad.p, sizeof(int32_t) * (size_t)nb * K, hipMemcpyDeviceToHost, ctx->stream));
            MMM_HIP(ctx, hipMemcpyAsync(matched + (size_t)off * K, md.p, sizeof(double) * (size_t)nb * K, hipMemcpyDeviceToHost, ctx->stream));
            MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    return do_assign ? check_assigned(ctx, who, assign, R, K) : MMM_OK;
}

} // namespace

// ---- internals for the handle entries of lda.hip / ctm.hip (mmm_internal.h) ------------------------------------------------------------------
int mmm_match_tables(mmm_ctx* ctx, const char* who, int R, int K, int C, int V, const double* const* h_tab, size_t sk, size_t sv, const double* cat, int self,
                     int32_t* assign, double* matched)
{
    MMM_CHECK(ctx, assign && matched, "%s: NULL assign or matched", who);
    if (!cat) C = K;
    if (int rc = check_shape(ctx, who, R, K, C, V, true)) return rc;
    DevBuf<double> cd, md; DevBuf<int32_t> ad;
    if (cat) {
        if (int rc = check_values(ctx, who, "cat", cat, (size_t)C * (size_t)V)) return rc;
        MMM_HIP(ctx, cd.alloc((size_t)C * (size_t)V));
        MMM_HIP(ctx, hipMemcpyAsync(cd.p, cat, sizeof(double) * (size_t)C * (size_t)V, hipMemcpyHostToDevice, ctx->stream));
    }
    MMM_HIP(ctx, ad.alloc((size_t)R * K)); MMM_HIP(ctx, md.alloc((size_t)R * K));
    if (int rc = match_run(ctx, R, K, C, V, h_tab, sk, sv, cat ? cd.p : h_tab[self], cat ? (size_t)V : sk, cat ? 1 : sv, ad.p, md.p, nullptr)) return rc;
    MMM_HIP(ctx, hipMemcpyAsync(assign, ad.p, sizeof(int32_t) * (size_t)R * K, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(matched, md.p, sizeof(double) * (size_t)R * K, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return check_assigned(ctx, who, assign, R, K);
}

int mmm_consensus_tables(mmm_ctx* ctx, const char* who, int R, int K, int V, const double* const* h_tab, size_t sk, size_t sv, int ref, int nq, const double* q,
                         int32_t* assign, double* matched, double* stability, double* mean, double* sd, double* quant)
{
    if (int rc = check_shape(ctx, who, R, K, K, V, true)) return rc;
    MMM_CHECK(ctx, ref >= 0 && ref < R, "%s: ref = %d is not one of the %d replicas", who, ref, R);
    MMM_CHECK(ctx, nq >= 0 && (nq == 0 || q), "%s: nq < 0 or NULL q", who);
    for (int i = 0; i < nq; ++i) MMM_CHECK(ctx, q[i] >= 0.0 && q[i] <= 1.0, "%s: q[%d] = %g is outside [0, 1]", who, i, q[i]);
    if (R > MMM_SUMMARY_MAX_B)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: R = %d replicas; the summary sorts a column in LDS, which holds at most %d (mmm_replicate_summary)", who, R,
                        MMM_SUMMARY_MAX_B);
    if (!quant) nq = 0;
    const size_t RK = (size_t)R * K, n = (size_t)K * (size_t)V;
    DevBuf<double> md; DevBuf<int32_t> ad;
    MMM_HIP(ctx, ad.alloc(RK)); MMM_HIP(ctx, md.alloc(RK));
    if (int rc = match_run(ctx, R, K, K, V, h_tab, sk, sv, h_tab[ref], sk, sv, ad.p, md.p, nullptr)) return rc;
    std::vector<int32_t> ha(RK); std::vector<double> hm(RK);
    MMM_HIP(ctx, hipMemcpyAsync(ha.data(), ad.p, sizeof(int32_t) * RK, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hm.data(), md.p, sizeof(double) * RK, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = check_assigned(ctx, who, ha.data(), R, K)) return rc;
    if (assign) memcpy(assign, ha.data(), sizeof(int32_t) * RK);
    if (matched) memcpy(matched, hm.data(), sizeof(double) * RK);
    if (stability) {       // per reference signature: the matched cosines of the other replicas, added in replica order
        std::vector<double> acc((size_t)K, 0.0);
        for (int r = 0; r < R; ++r) {
            if (r == ref) continue;
            for (int k = 0; k < K; ++k) acc[(size_t)ha[(size_t)r * K + k]] += hm[(size_t)r * K + k];
        }
        for (int k = 0; k < K; ++k) stability[k] = R > 1 ? acc[(size_t)k] / (double)(R - 1) : 1.0;
    }
    if (!mean && !sd && nq == 0) return MMM_OK;
    DevBuf<const double*> tab; DevBuf<double> P, qd, od;
    MMM_HIP(ctx, tab.alloc((size_t)R)); MMM_HIP(ctx, P.alloc((size_t)R * n)); MMM_HIP(ctx, qd.alloc((size_t)nq)); MMM_HIP(ctx, od.alloc((2 + (size_t)nq) * n));
    MMM_HIP(ctx, hipMemcpyAsync(tab.p, h_tab, sizeof(const double*) * (size_t)R, hipMemcpyHostToDevice, ctx->stream));
    if (nq) MMM_HIP(ctx, hipMemcpyAsync(qd.p, q, sizeof(double) * (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_align_normalise, dim3((unsigned)K, (unsigned)R), dim3(64), 0, ctx->stream, K, V, (const double* const*)tab.p, sk, sv, (const int32_t*)ad.p, P.p);
    MMM_LAUNCH_CHECK(ctx);
    if (int rc = mmm_replicate_summary_dev(ctx, R, n, P.p, nq, qd.p, od.p)) return rc;
    if (mean) MMM_HIP(ctx, hipMemcpyAsync(mean, od.p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (sd) MMM_HIP(ctx, hipMemcpyAsync(sd, od.p + n, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (nq) MMM_HIP(ctx, hipMemcpyAsync(quant, od.p + 2 * n, sizeof(double) * (size_t)nq * n, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MMM_OK;
}

extern "C" {

int mmm_signature_cosine(mmm_ctx* ctx, int R, int K, int C, int V, const double* sig, const double* cat, double* S)
{
    return match_arrays(ctx, "mmm_signature_cosine", R, K, C, V, sig, cat, nullptr, nullptr, S, false);
}

int mmm_signature_match(mmm_ctx* ctx, int R, int K, int C, int V, const double* sig, const double* cat, int32_t* assign, double* matched, double* S)
{
    return match_arrays(ctx, "mmm_signature_match", R, K, C, V, sig, cat, assign, matched, S, true);
}

int mmm_signature_consensus(mmm_ctx* ctx, int R, int K, int V, const double* sig, int ref, int nq, const double* q, int32_t* assign, double* matched,
                            double* stability, double* mean, double* sd, double* quant)
{
    const char* who = "mmm_signature_consensus";
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = check_shape(ctx, who, R, K, K, V, true)) return rc;
    MMM_CHECK(ctx, sig, "%s: NULL sig", who);
    MMM_CHECK(ctx, ref >= 0 && ref < R, "%s: ref = %d is not one of the %d replicas", who, ref, R);
    if (R > MMM_SUMMARY_MAX_B)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: R = %d replicas; the summary sorts a column in LDS, which holds at most %d (mmm_replicate_summary)", who, R,
                        MMM_SUMMARY_MAX_B);
    const size_t KV = (size_t)K * (size_t)V;
    if (int rc = check_values(ctx, who, "sig", sig, (size_t)R * KV)) return rc;
    DevBuf<double> sd_;
    MMM_HIP(ctx, sd_.alloc((size_t)R * KV));
    MMM_HIP(ctx, hipMemcpyAsync(sd_.p, sig, sizeof(double) * (size_t)R * KV, hipMemcpyHostToDevice, ctx->stream));
    std::vector<const double*> tab((size_t)R);
    for (int r = 0; r < R; ++r) tab[(size_t)r] = sd_.p + (size_t)r * KV;
    return mmm_consensus_tables(ctx, who, R, K, V, tab.data(), (size_t)V, 1, ref, nq, q, assign, matched, stability, mean, sd, quant);
}

} // extern "C"
