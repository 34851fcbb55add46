// decompose.hip -- signatures as sparse non-negative mixtures of catalogue rows, by EXHAUSTIVE search over the subsets of every size <= S (no
// counterpart in the reference; the published pipelines search greedily around NNLS because a host cannot afford the exhaustive search):
//   k_decompose_moments     G = cat cat^T, b = sig cat^T, ss = |sig|^2 with the fixed-order sums of match.hip
//   k_decompose_search<s>   per (signature, size s): every subset of size s through a 6 x 6 (at most) LDL^T solve on (G, b), best admissible gain
//   k_decompose_final<s>    the blocks' partial bests reduced, the winner evaluated once more for its weights, gain and cosine
// The definitions are in include/mmmusig.h and DESIGN.md section 4.16.  A subset's numbers are a fixed sequence of correctly rounded
// operations on (G, b) and the winner is the maximum of a total order (gain descending, members ascending), so the outputs depend neither
// on which lane met a subset nor on the order of the reductions: the same arguments give the same bits on every run and on either route
// of G (LDS or L2).
//
// Work distribution.  The unit is a PREFIX (c_1 < ... < c_{s-1}) drawn from the rows 0 .. C - 2, numbered by its rank in the combinatorial
// number system (rank = sum_j binom(c_j, j), 64-bit).  A LANE owns a prefix: it unranks it, factorises its s - 1 rows once and walks the last
// member over c_{s-1} + 1 .. C - 1, which costs one new row, one division and a back substitution per subset.  A wave takes 64 CONSECUTIVE
// ranks.  In this numbering consecutive ranks differ in their low members and share c_{s-1} (it changes once per binom(c, s - 2) ranks), so
// the 64 lanes of a wave have the same number of extensions up to one: the trip counts match without any exchange between lanes.  The
// alternative, a wave sharing one prefix with its lanes spread over c_s, leaves most lanes idle for the prefixes that end high (C - 1 -
// c_{s-1} < 64 extensions for every prefix once C <= 64) and factorises every prefix 64 times over.  The waves of the grid take chunks of 64
// ranks round robin, so that every block sees prefixes that end low (many extensions) and high (few).
#include "mmm_internal.h"
#include "dev_math.h"

namespace {

constexpr int kDcMaxS = 6;                  // largest subset
constexpr int kDcMaxC = 256;                // catalogue rows (a member is 8 bits of the packed key)
constexpr int kDcWaves = 8;                 // waves per block of k_decompose_search
constexpr int kDcMaxBlocks = 512;           // blocks per (signature, size)
constexpr int kDcMomWaves = 4;              // waves per block of k_decompose_moments: one (row, catalogue row) pair each
constexpr int kDcChunk = 1024;              // signatures per launch
constexpr size_t kDcLdsG = 128 * 1024;      // G is staged in LDS up to this size (C <= 128), read through L2 beyond
constexpr unsigned long long kDcNone = ~0ull;

// a candidate: its gain and its members packed 8 bits each, c_1 highest -- among subsets of one size the numeric order of the keys is the
// lexicographic order of the members.  kDcNone: no admissible subset yet (its gain is -1; an admissible gain is >= 0).
struct DcBest { double gain; unsigned long long key; };

__device__ __forceinline__ bool dc_better(double ga, unsigned long long ka, double gb, unsigned long long kb)
{
    return ga > gb || (ga == gb && ka < kb);
}

template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_mov_u64(unsigned long long v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, true);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

template <int CTRL>
__device__ __forceinline__ void dc_stage_dpp(DcBest& v)
{
    const double og = dpp_mov_f64<CTRL>(v.gain);
    const unsigned long long ok = dpp_mov_u64<CTRL>(v.key);
    if (dc_better(og, ok, v.gain, v.key)) { v.gain = og; v.key = ok; }
}

// the row swaps of rows_sum4 on the four words of a candidate: every lane gets its own words and its partner's (in one order or the other);
// it keeps the better of the two
template <bool HALVES>
__device__ __forceinline__ void dc_stage_rows(DcBest& v)
{
    const unsigned long long gb = (unsigned long long)__double_as_longlong(v.gain);
    const unsigned w[4] = {(unsigned)gb, (unsigned)(gb >> 32), (unsigned)v.key, (unsigned)(v.key >> 32)};
    unsigned x[4], y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const mmm_u2 p = HALVES ? __builtin_amdgcn_permlane32_swap(w[i], w[i], false, false) : __builtin_amdgcn_permlane16_swap(w[i], w[i], false, false);
        x[i] = p.x; y[i] = p.y;
    }
    const double gx = __longlong_as_double((long long)(((unsigned long long)x[1] << 32) | x[0])), gy = __longlong_as_double((long long)(((unsigned long long)y[1] << 32) | y[0]));
    const unsigned long long kx = ((unsigned long long)x[3] << 32) | x[2], ky = ((unsigned long long)y[3] << 32) | y[2];
    const bool bx = dc_better(gx, kx, gy, ky);
    v.gain = bx ? gx : gy; v.key = bx ? kx : ky;
}

// lexicographic arg-max (gain descending, key ascending) over the 64 lanes, valid in every lane: the maximum of a total order, so the lane
// order plays no part
__device__ __forceinline__ DcBest wave_best(DcBest v)
{
    dc_stage_dpp<0xB1>(v);
    dc_stage_dpp<0x4E>(v);
    dc_stage_dpp<0x141>(v);
    dc_stage_dpp<0x140>(v);
    dc_stage_rows<true>(v);
    dc_stage_rows<false>(v);
    return v;
}

// ---- the solve of include/mmmusig.h, row by row --------------------------------------------------------------------------------------------
template <int S>
struct DcFact {
    double l[S > 1 ? S * (S - 1) / 2 : 1];      // l_ip at i (i - 1) / 2 + p
    double r[S], y[S], z[S], gs[S];             // gs[i]: the gain through row i
};

// row I from g[j] = G[c_I][c_j] (j <= I) and beta = b[c_I]; false when the pivot fails.  Every index is a compile-time constant after
// unrolling: the state stays in registers.
template <int S, int I>
__device__ __forceinline__ bool dc_row(DcFact<S>& f, const double (&g)[S], double beta)
{
    double u[I + 1];
#pragma unroll
    for (int j = 0; j < I; ++j) {
        double t = g[j];
#pragma unroll
        for (int p = 0; p < j; ++p) t = t - u[p] * f.l[j * (j - 1) / 2 + p];
        u[j] = t;
    }
    double d = g[I];
#pragma unroll
    for (int p = 0; p < I; ++p) {
        const double lip = u[p] * f.r[p];
        f.l[I * (I - 1) / 2 + p] = lip;
        d = d - u[p] * lip;
    }
    if (!(d > 0x1p-26 * g[I])) return false;
    const double r = 1.0 / d;
    double y = beta;
#pragma unroll
    for (int p = 0; p < I; ++p) y = y - f.l[I * (I - 1) / 2 + p] * f.y[p];
    const double z = y * r;
    f.r[I] = r; f.y[I] = y; f.z[I] = z;
    if constexpr (I == 0) f.gs[0] = y * z; else f.gs[I] = f.gs[I - 1] + y * z;
    return true;
}

// rows I .. N - 1 of the subset c; G has the row stride C
template <int S, int I, int N>
__device__ __forceinline__ bool dc_rows(DcFact<S>& f, const int (&c)[S], const double* G, const double* b, int C)
{
    if constexpr (I >= N) return true;
    else {
        double g[S];
        const double* row = G + (size_t)c[I] * C;
#pragma unroll
        for (int j = 0; j <= I; ++j) g[j] = row[c[j]];
        if (!dc_row<S, I>(f, g, b[c[I]])) return false;
        return dc_rows<S, I + 1, N>(f, c, G, b, C);
    }
}

// back substitution; false unless every weight is > 0
template <int S>
__device__ __forceinline__ bool dc_weights(const DcFact<S>& f, double (&w)[S])
{
    bool pos = true;
#pragma unroll
    for (int i = S - 1; i >= 0; --i) {
        double t = f.z[i];
#pragma unroll
        for (int p = i + 1; p < S; ++p) t = t - f.l[p * (p - 1) / 2 + i] * w[p];
        w[i] = t;
        pos = pos && t > 0.0;
    }
    return pos;
}

__host__ __device__ inline size_t dc_lds_bytes(int S, int C, bool lds)
{
    return sizeof(double) * ((size_t)(S - 1) * C + (lds ? (size_t)C * C + C : 0));
}

// grid (blocks, signatures of the chunk).  LDS: binom(c, k) for k = 1 .. S - 1, c < C (64-bit), then with LDSG the whole of G and the
// signature's row of b; without, both are read through L2.  part[i * gridDim.x + block]: the block's best.
template <int S, bool LDSG>
__global__ __launch_bounds__(64 * kDcWaves) void k_decompose_search(int C, const double* __restrict__ G, const double* __restrict__ b, unsigned long long nprefix,
                                                                    DcBest* __restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) double s_dc[];
    __shared__ DcBest s_best[kDcWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t i = blockIdx.y;
    unsigned long long* s_bin = (unsigned long long*)s_dc;
    double* s_G = s_dc + (size_t)(S - 1) * C;
    double* s_b = s_G + (size_t)C * C;
    for (int c = tid; c < C; c += 64 * kDcWaves) {
        unsigned long long v = 1;                                   // binom(c, 0); binom(c, k) = binom(c, k - 1) (c - k + 1) / k, exact
#pragma unroll
        for (int k = 1; k < S; ++k) {
            v = c >= k ? v * (unsigned long long)(c - k + 1) / (unsigned long long)k : 0ull;
            s_bin[(k - 1) * C + c] = v;
        }
    }
    if (LDSG) {
        for (int idx = tid; idx < C * C; idx += 64 * kDcWaves) s_G[idx] = G[idx];
        for (int c = tid; c < C; c += 64 * kDcWaves) s_b[c] = b[i * C + c];
    }
    __syncthreads();
    const double* Gp = LDSG ? s_G : G;
    const double* bp = LDSG ? s_b : b + i * C;
    DcBest best = {-1.0, kDcNone};
    const unsigned long long nchunks = (nprefix + 63) >> 6;
    for (unsigned long long ch = (unsigned long long)blockIdx.x * kDcWaves + wave; ch < nchunks; ch += (unsigned long long)gridDim.x * kDcWaves) {
        unsigned long long rank = (ch << 6) + lane;
        if (rank >= nprefix) continue;
        int c[S];
        int top = C - 1;                                            // the members of a prefix lie below C - 1; each one below its successor
        unsigned long long kpre = 0;
#pragma unroll
        for (int k = S - 1; k >= 1; --k) {                          // member k - 1: the largest m < top with binom(m, k) <= rank
            int lo = k - 1, hi = top;                               // binom(k - 1, k) = 0 <= rank
            const unsigned long long* tab = s_bin + (k - 1) * C;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (tab[mid] <= rank) lo = mid; else hi = mid;
            }
            c[k - 1] = lo; rank -= tab[lo]; top = lo;
        }
#pragma unroll
        for (int j = 0; j + 1 < S; ++j) kpre = (kpre << 8) | (unsigned)c[j];
        DcFact<S> f;
        if (!dc_rows<S, 0, S - 1>(f, c, Gp, bp, C)) continue;       // a prefix that fails a pivot has no admissible extension
        for (int m = S > 1 ? c[S > 1 ? S - 2 : 0] + 1 : 0; m < C; ++m) {
            c[S - 1] = m;
            if (!dc_rows<S, S - 1, S>(f, c, Gp, bp, C)) continue;
            const double gain = f.gs[S - 1];
            const unsigned long long key = (kpre << 8) | (unsigned)m;
            if (!dc_better(gain, key, best.gain, best.key)) continue;      // (it could not win: its weights are not needed)
            double w[S];
            if (!dc_weights<S>(f, w)) continue;
            best.gain = gain; best.key = key;
        }
    }
    best = wave_best(best);
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int wv = 1; wv < kDcWaves; ++wv) {
            const DcBest o = s_best[wv];
            if (dc_better(o.gain, o.key, best.gain, best.key)) best = o;
        }
        part[i * gridDim.x + blockIdx.x] = best;
    }
}

// grid (signatures of the chunk), one wave each: the best of the nb partials of signature i, evaluated again by the same row steps (the same
// operations in the same order: the same bits) for the outputs of size S.  SW: the width of the output rows (the call's maximum size).
template <int S>
__global__ __launch_bounds__(64) void k_decompose_final(int C, int SW, int nb, const double* __restrict__ G, const double* __restrict__ b, const double* __restrict__ ss,
                                                        const DcBest* __restrict__ part, int32_t* __restrict__ subset, double* __restrict__ weight,
                                                        double* __restrict__ gain, double* __restrict__ cosine)
{
    const int lane = threadIdx.x;
    const size_t i = blockIdx.x;
    DcBest best = {-1.0, kDcNone};
    for (int k = lane; k < nb; k += 64) {
        const DcBest o = part[i * nb + k];
        if (dc_better(o.gain, o.key, best.gain, best.key)) best = o;
    }
    best = wave_best(best);
    const double s2 = ss[i];
    bool have = best.key != kDcNone && s2 != 0.0;
    int c[S]; double w[S]; DcFact<S> f;
#pragma unroll
    for (int j = 0; j < S; ++j) { c[j] = (int)((best.key >> (8 * (S - 1 - j))) & 0xffu); w[j] = 0.0; }
    f.gs[S - 1] = 0.0;
    if (have) {
#pragma unroll
        for (int j = 0; j < S; ++j) c[j] = min(c[j], C - 1);       // (a key is a subset: this bounds the reads whatever a partial holds)
        have = dc_rows<S, 0, S>(f, c, G, b + i * C, C) && dc_weights<S>(f, w);
    }
    if (lane != 0) return;
    const size_t o = i * SW + (S - 1);
    int32_t* sub = subset + o * SW; double* wt = weight + o * SW;
#pragma unroll
    for (int j = 0; j < S; ++j) { sub[j] = have ? c[j] : -1; wt[j] = have ? w[j] : 0.0; }
#pragma unroll
    for (int j = S; j < kDcMaxS; ++j) if (j < SW) { sub[j] = -1; wt[j] = 0.0; }
    const double g = have ? f.gs[S - 1] : 0.0;
    gain[o] = g;
    cosine[o] = have ? sqrt(fmin(g / s2, 1.0)) : 0.0;
}

// rows x0 + blockIdx.y of [cat; sig] (x < C: catalogue row x; else signature x - C) against catalogue row c, one wave per pair: lane l adds its
// terms l, l + 64, ... ascending, then wave_sum_fixed -- the order of mmm_signature_cosine's sums.  G: the pairs c >= x are computed and
// written to both places.  ss comes from the wave with c = 0.
__global__ __launch_bounds__(64 * kDcMomWaves) void k_decompose_moments(int x0, int C, int V, const double* __restrict__ sig, const double* __restrict__ cat,
                                                                        double* __restrict__ G, double* __restrict__ b, double* __restrict__ ss)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = (int)blockIdx.x * kDcMomWaves + wave, x = x0 + (int)blockIdx.y;
    const bool is_cat = x < C;
    if (c >= C || (is_cat && c < x)) return;                        // (whole waves leave; there is no barrier)
    const double* xr = is_cat ? cat + (size_t)x * V : sig + (size_t)(x - C) * V;
    const double* cr = cat + (size_t)c * V;
    double dot = 0.0, sq = 0.0;
    for (int v = lane; v < V; v += 64) { const double a = xr[v]; dot += a * cr[v]; sq += a * a; }
    dot = wave_sum_fixed(dot);
    sq = wave_sum_fixed(sq);
    if (lane != 0) return;
    if (is_cat) { G[(size_t)x * C + c] = dot; G[(size_t)c * C + x] = dot; }
    else {
        b[(size_t)(x - C) * C + c] = dot;
        if (c == 0) ss[x - C] = sq;
    }
}

unsigned long long dc_binom(int n, int k)       // exact while the result fits (n <= 256, k <= 6: below 2^39)
{
    if (k < 0 || k > n) return 0;
    unsigned long long v = 1;
    for (int j = 1; j <= k; ++j) v = v * (unsigned long long)(n - j + 1) / (unsigned long long)j;
    return v;
}

int dc_check_shape(mmm_ctx* ctx, const char* who, int n, int C, int S)
{
    MMM_CHECK(ctx, n >= 0 && C >= 1 && S >= 1, "%s: n = %d, C = %d, S = %d (n >= 0, C >= 1, S >= 1)", who, n, C, S);
    if (S > kDcMaxS) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: S = %d members at most (limit %d)", who, S, kDcMaxS);
    if (C > kDcMaxC) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: C = %d catalogue rows (limit %d)", who, C, kDcMaxC);
    const unsigned long long most = dc_binom(C, std::min(S, C));
    if (most >= (1ull << 32))
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: C = %d, S = %d: %llu subsets of the largest size (limit 2^32 - 1)", who, C, S, most);
    return MMM_OK;
}

template <int S>
int dc_launch_size(mmm_ctx* ctx, int nc, int C, int SW, bool lds, const double* dG, const double* db, const double* dss, DcBest* part, int32_t* subset,
                   double* weight, double* gain, double* cosine)
{
    const unsigned long long nprefix = dc_binom(C - 1, S - 1);
    const unsigned long long want = ((nprefix + 63) / 64 + kDcWaves - 1) / kDcWaves;
    const int nb = (int)std::max<unsigned long long>(1, std::min<unsigned long long>(want, (unsigned long long)kDcMaxBlocks));
    const size_t bytes = dc_lds_bytes(S, C, lds);
    auto kern = lds ? k_decompose_search<S, true> : k_decompose_search<S, false>;
    if (bytes > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)nb, (unsigned)nc), dim3(64 * kDcWaves), bytes, ctx->stream, C, dG, db, nprefix, part);
    MMM_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_decompose_final<S>, dim3((unsigned)nc), dim3(64), 0, ctx->stream, C, SW, nb, dG, db, dss, (const DcBest*)part, subset, weight, gain, cosine);
    MMM_LAUNCH_CHECK(ctx);
    return MMM_OK;
}

// Stage 2 on device moments (dG [C][C], db [n][C], dss [n]) into the host outputs; `marked` signatures come out empty.  Ends synchronised.
int dc_search(mmm_ctx* ctx, int n, int C, int S, const double* dG, const double* db, const double* dss, const std::vector<char>& marked, int32_t* subset,
              double* weight, double* gain, double* cosine)
{
    if (n == 0) return MMM_OK;
    const int nc_max = std::min(n, kDcChunk);
    const size_t SS = (size_t)S * S;
    const bool lds = (size_t)C * C * sizeof(double) <= kDcLdsG && !mmm_off(ctx->tune, MMM_OFF_DECOMPOSE_LDS);
    DevBuf<DcBest> part; DevBuf<int32_t> sub; DevBuf<double> wt, gn, cs;
    MMM_HIP(ctx, part.alloc((size_t)nc_max * kDcMaxBlocks)); MMM_HIP(ctx, sub.alloc(nc_max * SS)); MMM_HIP(ctx, wt.alloc(nc_max * SS));
    MMM_HIP(ctx, gn.alloc((size_t)nc_max * S)); MMM_HIP(ctx, cs.alloc((size_t)nc_max * S));
    for (int off = 0; off < n; off += nc_max) {
        const int nc = std::min(nc_max, n - off);
        // the sizes no launch covers (s > C) stay empty: subset -1, the rest 0
        MMM_HIP(ctx, hipMemsetAsync(sub.p, 0xff, sizeof(int32_t) * nc * SS, ctx->stream));
        MMM_HIP(ctx, hipMemsetAsync(wt.p, 0, sizeof(double) * nc * SS, ctx->stream));
        MMM_HIP(ctx, hipMemsetAsync(gn.p, 0, sizeof(double) * (size_t)nc * S, ctx->stream));
        MMM_HIP(ctx, hipMemsetAsync(cs.p, 0, sizeof(double) * (size_t)nc * S, ctx->stream));
        const double* b_ = db + (size_t)off * C; const double* ss_ = dss + off;
        for (int s = 1; s <= std::min(S, C); ++s) {
            int rc = MMM_OK;
            switch (s) {
            case 1: rc = dc_launch_size<1>(ctx, nc, C, S, lds, dG, b_, ss_, part.p, sub.p, wt.p, gn.p, cs.p); break;
            case 2: rc = dc_launch_size<2>(ctx, nc, C, S, lds, dG, b_, ss_, part.p, sub.p, wt.p, gn.p, cs.p); break;
            case 3: rc = dc_launch_size<3>(ctx, nc, C, S, lds, dG, b_, ss_, part.p, sub.p, wt.p, gn.p, cs.p); break;
            case 4: rc = dc_launch_size<4>(ctx, nc, C, S, lds, dG, b_, ss_, part.p, sub.p, wt.p, gn.p, cs.p); break;
            case 5: rc = dc_launch_size<5>(ctx, nc, C, S, lds, dG, b_, ss_, part.p, sub.p, wt.p, gn.p, cs.p); break;
            default: rc = dc_launch_size<6>(ctx, nc, C, S, lds, dG, b_, ss_, part.p, sub.p, wt.p, gn.p, cs.p); break;
            }
            if (rc) return rc;
        }
        MMM_HIP(ctx, hipMemcpyAsync(subset + off * SS, sub.p, sizeof(int32_t) * nc * SS, hipMemcpyDeviceToHost, ctx->stream));
        MMM_HIP(ctx, hipMemcpyAsync(weight + off * SS, wt.p, sizeof(double) * nc * SS, hipMemcpyDeviceToHost, ctx->stream));
        MMM_HIP(ctx, hipMemcpyAsync(gain + (size_t)off * S, gn.p, sizeof(double) * (size_t)nc * S, hipMemcpyDeviceToHost, ctx->stream));
        MMM_HIP(ctx, hipMemcpyAsync(cosine + (size_t)off * S, cs.p, sizeof(double) * (size_t)nc * S, hipMemcpyDeviceToHost, ctx->stream));
        MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int i = 0; i < n; ++i) {
        if (!marked[(size_t)i]) continue;
        for (size_t j = 0; j < SS; ++j) { subset[i * SS + j] = -1; weight[i * SS + j] = 0.0; }
        for (int s = 0; s < S; ++s) { gain[(size_t)i * S + s] = 0.0; cosine[(size_t)i * S + s] = 0.0; }
    }
    return MMM_OK;
}

// The moments as the search takes them: every entry finite, ss >= 0.  A bad entry of G marks every signature, one of b[i] or ss[i] marks
// signature i; `first` names the first of them for the error message (empty: none).
void dc_mark(int n, int C, const double* G, const double* b, const double* ss, std::vector<char>& marked, std::string& first)
{
    char buf[160];
    marked.assign((size_t)n, 0);
    for (size_t k = 0; k < (size_t)C * C; ++k)
        if (!std::isfinite(G[k])) {
            snprintf(buf, sizeof buf, "G[%zu][%zu] = %g is not finite: no signature can be decomposed", k / C, k % C, G[k]);
            first = buf;
            marked.assign((size_t)n, 1);
            return;
        }
    for (int i = 0; i < n; ++i) {
        bool bad = !std::isfinite(ss[i]) || ss[i] < 0.0;
        for (int c = 0; c < C && !bad; ++c) bad = !std::isfinite(b[(size_t)i * C + c]);
        if (!bad) continue;
        marked[(size_t)i] = 1;
        if (first.empty()) {
            snprintf(buf, sizeof buf, "the moments of signature %d (its row of b, or ss) hold a NaN, an Inf or a negative ss: it is left undecomposed", i);
            first = buf;
        }
    }
}

} // namespace

extern "C" {

int mmm_decompose_search(mmm_ctx* ctx, int n, int C, int S, const double* G, const double* b, const double* ss, int32_t* subset, double* weight, double* gain,
                         double* cosine)
{
    const char* who = "mmm_decompose_search";
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dc_check_shape(ctx, who, n, C, S)) return rc;
    MMM_CHECK(ctx, G && (n == 0 || (b && ss && subset && weight && gain && cosine)), "%s: NULL argument", who);
    if (n == 0) return MMM_OK;
    std::vector<char> marked; std::string first;
    dc_mark(n, C, G, b, ss, marked, first);
    DevBuf<double> dG, db, dss;
    MMM_HIP(ctx, dG.alloc((size_t)C * C)); MMM_HIP(ctx, db.alloc((size_t)n * C)); MMM_HIP(ctx, dss.alloc((size_t)n));
    MMM_HIP(ctx, hipMemcpyAsync(dG.p, G, sizeof(double) * (size_t)C * C, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(db.p, b, sizeof(double) * (size_t)n * C, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(dss.p, ss, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = dc_search(ctx, n, C, S, dG.p, db.p, dss.p, marked, subset, weight, gain, cosine)) return rc;
    MMM_CHECK(ctx, first.empty(), "%s: %s", who, first.c_str());
    return MMM_OK;
}

int mmm_signature_decompose(mmm_ctx* ctx, int n, int C, int V, const double* sig, const double* cat, int S, int32_t* subset, double* weight, double* gain,
                            double* cosine, double* G_out, double* b_out, double* ss_out)
{
    const char* who = "mmm_signature_decompose";
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = dc_check_shape(ctx, who, n, C, S)) return rc;
    MMM_CHECK(ctx, V >= 1, "%s: V = %d (V >= 1)", who, V);
    MMM_CHECK(ctx, cat && (n == 0 || (sig && subset && weight && gain && cosine)), "%s: NULL argument", who);
    for (int c = 0; c < C; ++c) {
        bool any = false;
        for (int v = 0; v < V; ++v) {
            const double x = cat[(size_t)c * V + v];
            MMM_CHECK(ctx, std::isfinite(x) && x >= 0.0, "%s: catalogue entry (%d, %d) is negative or not finite", who, c, v);
            any = any || x > 0.0;
        }
        MMM_CHECK(ctx, any, "%s: catalogue row %d is all zero", who, c);
    }
    for (size_t k = 0; k < (size_t)n * V; ++k)
        MMM_CHECK(ctx, std::isfinite(sig[k]) && sig[k] >= 0.0, "%s: signature entry (%zu, %zu) is negative or not finite", who, k / V, k % V);
    DevBuf<double> dsig, dcat, dG, db, dss;
    MMM_HIP(ctx, dsig.alloc((size_t)n * V)); MMM_HIP(ctx, dcat.alloc((size_t)C * V));
    MMM_HIP(ctx, dG.alloc((size_t)C * C)); MMM_HIP(ctx, db.alloc((size_t)n * C)); MMM_HIP(ctx, dss.alloc((size_t)n));
    MMM_HIP(ctx, hipMemcpyAsync(dcat.p, cat, sizeof(double) * (size_t)C * V, hipMemcpyHostToDevice, ctx->stream));
    if (n) MMM_HIP(ctx, hipMemcpyAsync(dsig.p, sig, sizeof(double) * (size_t)n * V, hipMemcpyHostToDevice, ctx->stream));
    const unsigned gx = (unsigned)((C + kDcMomWaves - 1) / kDcMomWaves);
    hipLaunchKernelGGL(k_decompose_moments, dim3(gx, (unsigned)C), dim3(64 * kDcMomWaves), 0, ctx->stream, 0, C, V, (const double*)dsig.p, (const double*)dcat.p, dG.p,
                       db.p, dss.p);
    MMM_LAUNCH_CHECK(ctx);
    for (int off = 0; off < n; off += kDcChunk) {
        hipLaunchKernelGGL(k_decompose_moments, dim3(gx, (unsigned)std::min(kDcChunk, n - off)), dim3(64 * kDcMomWaves), 0, ctx->stream, C + off, C, V,
                           (const double*)dsig.p, (const double*)dcat.p, dG.p, db.p, dss.p);
        MMM_LAUNCH_CHECK(ctx);
    }
    std::vector<double> hG((size_t)C * C), hb((size_t)n * C), hss((size_t)n);
    MMM_HIP(ctx, hipMemcpyAsync(hG.data(), dG.p, sizeof(double) * hG.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (n) {
        MMM_HIP(ctx, hipMemcpyAsync(hb.data(), db.p, sizeof(double) * hb.size(), hipMemcpyDeviceToHost, ctx->stream));
        MMM_HIP(ctx, hipMemcpyAsync(hss.data(), dss.p, sizeof(double) * hss.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (G_out) memcpy(G_out, hG.data(), sizeof(double) * hG.size());
    if (b_out && n) memcpy(b_out, hb.data(), sizeof(double) * hb.size());
    if (ss_out && n) memcpy(ss_out, hss.data(), sizeof(double) * hss.size());
    if (n == 0) return MMM_OK;
    std::vector<char> marked; std::string first;
    dc_mark(n, C, hG.data(), hb.data(), hss.data(), marked, first);        // (finite inputs whose products overflow)
    if (int rc = dc_search(ctx, n, C, S, dG.p, db.p, dss.p, marked, subset, weight, gain, cosine)) return rc;
    MMM_CHECK(ctx, first.empty(), "%s: %s", who, first.c_str());
    return MMM_OK;
}

} // extern "C"
