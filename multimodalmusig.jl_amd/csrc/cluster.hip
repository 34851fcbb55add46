// cluster.hip -- mmm_cluster_samples: consensus k-means of D samples on P features; B subsampled replicates for every candidate number of groups
// in one launch, then the all-pairs co-clustering counts and the PAC inputs (no counterpart in the reference; include/mmmusig.h has the
// normative definition, DESIGN.md section 4.18 the reasoning).
//
// k_cluster_replicates: one workgroup runs one (replicate, k) pair through the subsample, the k-means++ start and all Lloyd iterations; pairs
//   beyond the resident blocks are handed out through a work counter.  The members are compacted in ascending order by ballot and prefix count;
//   a second list groups them by stripe (sample d belongs to stripe d mod 16), in ascending order inside a stripe.
//   assignment: one member per lane, eight centres at a time (eight independent chains over p), the centres broadcast from LDS;
//   centre sums: one (stripe, centre, feature) per thread walking its stripe's members, then one (centre, feature) per thread over the 16 slabs.
//   The members' rows, md, cum, the labels, the two lists and the 16 slabs live in LDS where they fit, in a per-block workspace read through L2
//   otherwise (the rows are then read from x itself); the centres are always in LDS.  Nothing but __syncthreads orders the phases.
// k_consensus_pairs: a wave owns 64 consecutive j and 8 consecutive i and loops over the replicates; every pair is written once.
#include "mmm_internal.h"
#include "mmm_philox.h"

namespace {

constexpr int kClMaxD = 4096, kClMaxP = 256, kClMaxNk = 16, kClMaxK = 32;
constexpr int kClStripes = 16;                  // of the definition
// the library's choice: a run is a latency chain that other blocks on the CU hide, and 8 waves leave room for two blocks (BRCA, 560 samples, ks 2 .. 9,
// 1000 replicates: the call takes 6.6 ms, 9.5 ms with 4 waves, and 8.6 ms with 16, which leave one block per CU)
constexpr int kClAutoWaves = 8;
constexpr size_t kClLdsBlock = 160 * 1024;      // LDS a block may take (the CU's)
constexpr uint32_t kClBits = 0xC0000000u;       // second counter word: bit 31 is extract.hip's, bit 30 is set by no other user
constexpr int kClSmallInts = 18 + 16 + kClStripes * kClMaxK + kClMaxK + 4;      // soff, wcnt, cnt, chosen, ctl
constexpr int kPairTI = 8;                      // rows i of a wave of k_consensus_pairs

struct ClArgs {
    int D, P, nk, B, b0, maxiter, kmax;
    uint32_t keep, k0, k1, stream;
    const double* x;                 // [D][P]
    const int32_t* ks;               // [nk]
    double* wsd; int* wsi;           // per block workspace (memory placement): 2 D + 16 kmax P doubles, 3 D ints
    int8_t* labels; int32_t* iters; double* inertia;
    int* counter;                    // next pair
};

// sum_p (x_p - m_p)^2, p ascending from 0.0
__device__ __forceinline__ double cl_dist(const double* __restrict__ xr, const double* __restrict__ m, int P)
{
    double s = 0.0;
    for (int p = 0; p < P; ++p) {
        const double t = xr[p] - m[p];
        s += t * t;
    }
    return s;
}

template <bool LDS>
__global__ __launch_bounds__(1024) void k_cluster_replicates(const ClArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_cl[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = (int)blockDim.x, nw = nt >> 6;
    const int D = a.D, P = a.P, Ps = LDS ? (P | 1) : P;          // odd row stride in LDS: a lane per member walks its row without bank conflicts
    double* cent = s_cl;                                         // [kmax][P]
    double* red = cent + (size_t)a.kmax * P;                     // 16 stripe sums
    int* soff = (int*)(red + kClStripes);                        // 17 stripe offsets (18: the ints stay even)
    int* wcnt = soff + 18;                                       // per wave / per stripe counts
    int* cnt = wcnt + 16;                                        // [16][32] members of a centre per stripe
    int* chosen = cnt + kClStripes * kClMaxK;                    // the members taken as start centres
    int* ctl = chosen + kClMaxK;
    double* big = LDS ? (double*)(ctl + 4) : a.wsd + (size_t)blockIdx.x * (2 * (size_t)D + (size_t)kClStripes * a.kmax * P);
    double* md = big;                                            // [n] distance to the nearest centre
    double* cum = md + D;                                        // [n] its running sum
    double* slab = cum + D;                                      // [16][k][P]
    double* xs = slab + (size_t)kClStripes * a.kmax * P;         // [n][Ps] (LDS only)
    int* lab = LDS ? (int*)(xs + (size_t)D * Ps) : a.wsi + (size_t)blockIdx.x * 3 * D;
    int* mem = lab + D;                                          // members, ascending
    int* sidx = mem + D;                                         // member positions grouped by stripe
    const double two32 = 4294967296.0;

    for (;;) {
        __syncthreads();
        if (tid == 0) ctl[0] = atomicAdd(a.counter, 1);
        __syncthreads();
        const int w = ctl[0];
        if (w >= a.nk * a.B) break;
        const int b = w / a.nk, ki = w - b * a.nk;               // the pairs of a replicate are neighbours
        const int k = a.ks[ki];
        const uint32_t bg = (uint32_t)(a.b0 + b);
        int8_t* lo = a.labels + ((size_t)ki * a.B + b) * D;
        // ---- the subsample, compacted in ascending order
        int n = 0;
        for (int d0 = 0; d0 < D; d0 += nt) {
            const int d = d0 + tid;
            bool in = false;
            if (d < D) {
                in = true;
                if (a.keep) {
                    uint32_t u[4];
                    philox4x32_10((uint32_t)(d >> 2), kClBits, bg, a.stream, a.k0, a.k1, u);
                    in = u[d & 3] < a.keep;
                }
                lo[d] = -1;
            }
            const unsigned long long m = __ballot(in);
            if (lane == 0) wcnt[wave] = __popcll(m);
            __syncthreads();
            int base = n, tot = 0;
            for (int i = 0; i < nw; ++i) {
                if (i < wave) base += wcnt[i];
                tot += wcnt[i];
            }
            if (in) mem[base + __popcll(m & ((1ull << lane) - 1ull))] = d;
            n += tot;
            __syncthreads();
        }
        if (n < k) {                                             // skipped: labels -1
            if (tid == 0) { a.iters[(size_t)ki * a.B + b] = 0; a.inertia[(size_t)ki * a.B + b] = 0.0; }
            continue;
        }
        if (LDS)
            for (int i = tid; i < n * P; i += nt) {
                const int m_ = i / P, p = i - m_ * P;
                xs[(size_t)m_ * Ps + p] = a.x[(size_t)mem[m_] * P + p];
            }
        auto xrow = [&](int m_) -> const double* { return LDS ? xs + (size_t)m_ * Ps : a.x + (size_t)mem[m_] * P; };
        // ---- the stripes' member lists
        if (tid < kClStripes) {
            int c = 0, m_ = 0;
            for (; m_ + 8 <= n; m_ += 8) {
                int v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = mem[m_ + j];
#pragma unroll
                for (int j = 0; j < 8; ++j) c += (v[j] & (kClStripes - 1)) == tid;
            }
            for (; m_ < n; ++m_) c += (mem[m_] & (kClStripes - 1)) == tid;
            wcnt[tid] = c;
        }
        __syncthreads();
        if (tid == 0) {
            int s = 0;
            for (int st = 0; st < kClStripes; ++st) { soff[st] = s; s += wcnt[st]; }
            soff[kClStripes] = s;
        }
        __syncthreads();
        if (tid < kClStripes) {
            int o = soff[tid], m_ = 0;
            for (; m_ + 8 <= n; m_ += 8) {
                int v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = mem[m_ + j];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if ((v[j] & (kClStripes - 1)) == tid) sidx[o++] = m_ + j;
            }
            for (; m_ < n; ++m_)
                if ((mem[m_] & (kClStripes - 1)) == tid) sidx[o++] = m_;
        }
        // ---- start: k-means++ by integer thresholds
        uint32_t u[4];
        philox4x32_10(0u, kClBits | (uint32_t)k, bg, a.stream, a.k0, a.k1, u);
        const int first = (int)__umulhi(u[0], (uint32_t)n);
        if (tid == 0) chosen[0] = first;
        for (int p = tid; p < P; p += nt) cent[p] = xrow(first)[p];
        __syncthreads();
        for (int m_ = tid; m_ < n; m_ += nt) md[m_] = cl_dist(xrow(m_), cent, P);
        for (int i = 1; i < k; ++i) {
            if ((i & 3) == 0) philox4x32_10((uint32_t)(i >> 2), kClBits | (uint32_t)k, bg, a.stream, a.k0, a.k1, u);
            const uint32_t ui = (i & 3) == 0 ? u[0] : (i & 3) == 1 ? u[1] : (i & 3) == 2 ? u[2] : u[3];
            __syncthreads();
            if (tid == 0) {
                double c = 0.0;
                int m_ = 0;
                for (; m_ + 8 <= n; m_ += 8) {                   // eight loads in flight, then the adds in order: the chain is the adds', not the LDS waits'
                    double v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = md[m_ + j];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { c += v[j]; cum[m_ + j] = c; }
                }
                for (; m_ < n; ++m_) { c += md[m_]; cum[m_] = c; }
                int pick = n;
                if (!(c > 0.0)) {                                // every member coincides with a centre: the lowest one not yet chosen
                    for (pick = 0; pick < n; ++pick) {
                        bool taken = false;
                        for (int j = 0; j < i; ++j) taken |= chosen[j] == pick;
                        if (!taken) break;
                    }
                }
                ctl[1] = pick;
            }
            __syncthreads();
            const double S = cum[n - 1];
            if (S > 0.0) {
                for (int m_ = tid; m_ < n; m_ += nt) {
                    const unsigned long long T = (unsigned long long)((cum[m_] / S) * two32);       // floor: the product is exact and >= 0
                    if (T > (unsigned long long)ui) atomicMin(&ctl[1], m_);
                }
                __syncthreads();
            }
            const int pick = ctl[1];
            if (tid == 0) chosen[i] = pick;
            for (int p = tid; p < P; p += nt) cent[i * P + p] = xrow(pick)[p];
            __syncthreads();
            for (int m_ = tid; m_ < n; m_ += nt) {
                const double dd = cl_dist(xrow(m_), cent + i * P, P);
                if (dd < md[m_]) md[m_] = dd;
            }
        }
        // ---- Lloyd
        for (int m_ = tid; m_ < n; m_ += nt) lab[m_] = -1;
        const int kP = k * P;
        int it = 0;
        while (it < a.maxiter) {
            ++it;
            if (tid == 0) ctl[2] = 0;
            __syncthreads();
            int changed = 0;
            for (int m_ = tid; m_ < n; m_ += nt) {
                const double* xr = xrow(m_);
                int best = 0;
                double bd = 0.0;
                for (int c0 = 0; c0 < k; c0 += 8) {
                    double acc[8];
                    const double* cp[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { acc[j] = 0.0; cp[j] = cent + min(c0 + j, k - 1) * P; }
                    for (int p = 0; p < P; ++p) {
                        const double xv = xr[p];
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const double t = xv - cp[j][p];
                            acc[j] += t * t;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (c0 + j < k && (c0 + j == 0 || acc[j] < bd)) { bd = acc[j]; best = c0 + j; }      // strict: ties to the lowest centre
                }
                changed |= lab[m_] != best;
                lab[m_] = best;
                md[m_] = bd;
            }
            if (changed) ctl[2] = 1;
            __syncthreads();
            if (!ctl[2]) break;
            for (int e = tid; e < kClStripes * kP; e += nt) {
                const int st = e / kP, r = e - st * kP, c = r / P, p = r - c * P;
                double s = 0.0;
                int m = 0;
                for (int q = soff[st]; q < soff[st + 1]; ++q) {
                    const int m_ = sidx[q];
                    if (lab[m_] == c) { s += xrow(m_)[p]; ++m; }
                }
                slab[e] = s;
                if (p == 0) cnt[st * kClMaxK + c] = m;
            }
            __syncthreads();
            for (int e = tid; e < kP; e += nt) {
                const int c = e / P;
                double s = 0.0;
                int m = 0;
                for (int st = 0; st < kClStripes; ++st) { s += slab[(size_t)st * kP + e]; m += cnt[st * kClMaxK + c]; }
                if (m > 0) cent[e] = s / (double)m;              // a centre without members keeps its value
            }
        }
        // ---- finish: inertia in stripe order, the labels at the samples' places
        __syncthreads();
        if (tid < kClStripes) {
            double s = 0.0;
            for (int q = soff[tid]; q < soff[tid + 1]; ++q) s += md[sidx[q]];
            red[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int st = 0; st < kClStripes; ++st) s += red[st];
            a.inertia[(size_t)ki * a.B + b] = s;
            a.iters[(size_t)ki * a.B + b] = it;
        }
        for (int m_ = tid; m_ < n; m_ += nt) lo[mem[m_]] = (int8_t)lab[m_];
    }
}

__device__ __forceinline__ unsigned int cl_wave_sum_u32(unsigned int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// lab [nk][B][D]; together, same [nk][D][D] or NULL; pac [nk][2] = ambiguous, valid over the pairs i < j
__global__ __launch_bounds__(256) void k_consensus_pairs(int D, int B, const int8_t* __restrict__ lab, uint32_t* __restrict__ together, uint32_t* __restrict__ same,
                                                         int pac_lo, int pac_hi, unsigned long long* pac)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ki = blockIdx.z;
    const int j = blockIdx.x * 64 + lane, i0 = (blockIdx.y * 4 + wave) * kPairTI;
    if (i0 >= D) return;
    const int8_t* L = lab + (size_t)ki * B * D;
    const int jj = min(j, D - 1);
    uint32_t tg[kPairTI], sm[kPairTI];
#pragma unroll
    for (int t = 0; t < kPairTI; ++t) tg[t] = sm[t] = 0u;
    for (int b = 0; b < B; ++b) {
        const int8_t* row = L + (size_t)b * D;
        const int lj = row[jj];
#pragma unroll
        for (int t = 0; t < kPairTI; ++t) {
            const int li = row[min(i0 + t, D - 1)];
            tg[t] += (uint32_t)(li >= 0 && lj >= 0);
            sm[t] += (uint32_t)(li >= 0 && li == lj);
        }
    }
    unsigned int valid = 0u, amb = 0u;
#pragma unroll
    for (int t = 0; t < kPairTI; ++t) {
        const int i = i0 + t;
        if (i < D && j < D) {
            const size_t o = ((size_t)ki * D + i) * D + j;
            if (together) together[o] = tg[t];
            if (same) same[o] = sm[t];
            if (i < j && tg[t] > 0u) {
                const unsigned long long s1000 = 1000ull * sm[t];
                ++valid;
                amb += (s1000 > (unsigned long long)pac_lo * tg[t] && s1000 < (unsigned long long)pac_hi * tg[t]) ? 1u : 0u;
            }
        }
    }
    valid = cl_wave_sum_u32(valid); amb = cl_wave_sum_u32(amb);
    if (lane == 0) {
        if (amb) atomicAdd(&pac[2 * ki], (unsigned long long)amb);
        if (valid) atomicAdd(&pac[2 * ki + 1], (unsigned long long)valid);
    }
}

// LDS bytes of a block: the centres and the small arrays; the per-block arrays
size_t cl_lds_base(int kmax, int P) { return sizeof(double) * ((size_t)kmax * P + kClStripes) + sizeof(int) * (size_t)kClSmallInts; }
size_t cl_lds_big(int D, int P, int kmax) { return sizeof(double) * (2 * (size_t)D + (size_t)kClStripes * kmax * P + (size_t)D * (P | 1)) + sizeof(int) * 3 * (size_t)D; }

} // namespace

extern "C" int mmm_cluster_samples(mmm_ctx* ctx, int D, int P, const double* x, int nk, const int32_t* ks, int B, int b0, uint32_t keep, uint64_t seed, uint32_t stream,
                                   int maxiter, int pac_lo, int pac_hi, int waves, int placement, int8_t* labels, int32_t* iters, double* inertia,
                                   uint32_t* together, uint32_t* same, int64_t* ambiguous, int64_t* valid)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, D >= 1 && P >= 1 && nk >= 1, "mmm_cluster_samples: D = %d, P = %d, nk = %d (>= 1 each)", D, P, nk);
    if (D > kClMaxD) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cluster_samples: D = %d samples (limit %d)", D, kClMaxD);
    if (P > kClMaxP) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cluster_samples: P = %d features (limit %d)", P, kClMaxP);
    if (nk > kClMaxNk) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cluster_samples: nk = %d numbers of groups (limit %d)", nk, kClMaxNk);
    MMM_CHECK(ctx, x && ks, "mmm_cluster_samples: NULL argument");
    int kmax = 1;
    for (int i = 0; i < nk; ++i) {
        MMM_CHECK(ctx, ks[i] >= 1, "mmm_cluster_samples: ks[%d] = %d (>= 1)", i, ks[i]);
        if (ks[i] > kClMaxK) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cluster_samples: ks[%d] = %d groups (limit %d)", i, ks[i], kClMaxK);
        kmax = std::max(kmax, (int)ks[i]);
    }
    MMM_CHECK(ctx, B >= 0 && b0 >= 0 && (int64_t)b0 + B <= 0x7fffffffLL, "mmm_cluster_samples: B = %d, b0 = %d (>= 0, b0 + B <= 2^31 - 1)", B, b0);
    MMM_CHECK(ctx, maxiter >= 1, "mmm_cluster_samples: maxiter = %d (>= 1)", maxiter);
    MMM_CHECK(ctx, 0 <= pac_lo && pac_lo < pac_hi && pac_hi <= 1000, "mmm_cluster_samples: pac_lo = %d, pac_hi = %d (0 <= pac_lo < pac_hi <= 1000)", pac_lo, pac_hi);
    MMM_CHECK(ctx, waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8 || waves == 16, "mmm_cluster_samples: waves = %d (0, 1, 2, 4, 8 or 16)", waves);
    MMM_CHECK(ctx, placement >= 0 && placement <= 2, "mmm_cluster_samples: placement = %d (0, 1 or 2)", placement);
    MMM_CHECK(ctx, B == 0 || (labels && iters && inertia), "mmm_cluster_samples: NULL argument");
    // |x| <= 1e150: a difference is at most 2e150, its square 4e300, a distance over P <= 256 features about 1e303 and the sum of D <= 4096 of
    // them 4e306 -- every square and every sum of the definition stays finite
    for (size_t i = 0; i < (size_t)D * P; ++i)
        MMM_CHECK(ctx, std::isfinite(x[i]) && std::fabs(x[i]) <= 1e150, "mmm_cluster_samples: x entry (%zu, %zu) is not finite or beyond 1e150 in magnitude", i / P, i % P);
    const size_t nlab = (size_t)nk * (size_t)B * D;
    if (nlab >= ((size_t)1 << 31)) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cluster_samples: nk B D = %zu labels (limit 2^31 - 1)", nlab);
    if (B == 0) return MMM_OK;

    const int nw = waves ? waves : kClAutoWaves;
    const size_t base = cl_lds_base(kmax, P), bigb = cl_lds_big(D, P, kmax);
    const bool in_lds = placement != 2 && base + bigb <= kClLdsBlock;
    const size_t lds = base + (in_lds ? bigb : 0);
    const int cus = std::max(1, ctx->num_cu);
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(16 / nw, (int64_t)(kClLdsBlock / lds)));
    const int64_t pairs = (int64_t)nk * B;
    const unsigned grid = (unsigned)std::min<int64_t>(pairs, (int64_t)cus * per_cu);
    const size_t wsd_n = 2 * (size_t)D + (size_t)kClStripes * kmax * P, DD = (size_t)nk * D * D;
    const bool pairs_pass = together || same || ambiguous || valid;

    DevBuf<double> xd, wsd, ind; DevBuf<int> wsi, counter; DevBuf<int32_t> ksd, itd; DevBuf<int8_t> labd; DevBuf<uint32_t> tgd, smd; DevBuf<unsigned long long> pacd;
    MMM_HIP(ctx, xd.alloc((size_t)D * P)); MMM_HIP(ctx, ksd.alloc((size_t)nk)); MMM_HIP(ctx, counter.alloc(1));
    MMM_HIP(ctx, labd.alloc(nlab)); MMM_HIP(ctx, itd.alloc((size_t)nk * B)); MMM_HIP(ctx, ind.alloc((size_t)nk * B));
    if (!in_lds) { MMM_HIP(ctx, wsd.alloc((size_t)grid * wsd_n)); MMM_HIP(ctx, wsi.alloc((size_t)grid * 3 * D)); }
    if (together) MMM_HIP(ctx, tgd.alloc(DD));
    if (same) MMM_HIP(ctx, smd.alloc(DD));
    if (pairs_pass) MMM_HIP(ctx, pacd.alloc(2 * (size_t)nk));
    MMM_HIP(ctx, hipMemcpyAsync(xd.p, x, sizeof(double) * (size_t)D * P, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(ksd.p, ks, sizeof(int32_t) * (size_t)nk, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));

    ClArgs a;
    a.D = D; a.P = P; a.nk = nk; a.B = B; a.b0 = b0; a.maxiter = maxiter; a.kmax = kmax;
    a.keep = keep; a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.x = xd.p; a.ks = ksd.p; a.wsd = in_lds ? nullptr : wsd.p; a.wsi = in_lds ? nullptr : wsi.p;
    a.labels = labd.p; a.iters = itd.p; a.inertia = ind.p; a.counter = counter.p;
    auto kern = in_lds ? k_cluster_replicates<true> : k_cluster_replicates<false>;
    if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), lds, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    if (pairs_pass) {
        MMM_HIP(ctx, hipMemsetAsync(pacd.p, 0, sizeof(unsigned long long) * 2 * (size_t)nk, ctx->stream));
        hipLaunchKernelGGL(k_consensus_pairs, dim3((unsigned)((D + 63) / 64), (unsigned)((D + 4 * kPairTI - 1) / (4 * kPairTI)), (unsigned)nk), dim3(256), 0, ctx->stream,
                           D, B, labd.p, together ? tgd.p : nullptr, same ? smd.p : nullptr, pac_lo, pac_hi, pacd.p);
        MMM_LAUNCH_CHECK(ctx);
    }
    std::vector<unsigned long long> pac(2 * (size_t)nk, 0ull);
    MMM_HIP(ctx, hipMemcpyAsync(labels, labd.p, nlab, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(iters, itd.p, sizeof(int32_t) * (size_t)nk * B, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(inertia, ind.p, sizeof(double) * (size_t)nk * B, hipMemcpyDeviceToHost, ctx->stream));
    if (together) MMM_HIP(ctx, hipMemcpyAsync(together, tgd.p, sizeof(uint32_t) * DD, hipMemcpyDeviceToHost, ctx->stream));
    if (same) MMM_HIP(ctx, hipMemcpyAsync(same, smd.p, sizeof(uint32_t) * DD, hipMemcpyDeviceToHost, ctx->stream));
    if (pairs_pass) MMM_HIP(ctx, hipMemcpyAsync(pac.data(), pacd.p, sizeof(unsigned long long) * pac.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < nk; ++i) {
        if (ambiguous) ambiguous[i] = (int64_t)pac[2 * (size_t)i];
        if (valid) valid[i] = (int64_t)pac[2 * (size_t)i + 1];
    }
    return MMM_OK;
}
