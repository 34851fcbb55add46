// assoc.hip -- mmm_associate_exposures: rank statistics of P features against C covariates over D samples, B permutations of the covariate rows
// (within strata) in one launch, with the per-covariate maximum of every permutation for Westfall-Young adjusted p-values (no counterpart in
// the reference; include/mmmusig.h has the normative definition, DESIGN.md section 4.19 the reasoning).
//
// The host turns x and y into doubled midranks (16-bit integers), the weights and the centring terms; everything the device adds is an integer,
// so no order of summation matters until t is formed, and t is formed by one thread per (feature, covariate) in the written order.
// k_assoc: one workgroup runs one permutation; permutations beyond the resident blocks are handed out through a work counter.
//   sort:    a thread computes the Philox words of four samples; the composites (stratum << 44 | key << 12 | d), padded with all-ones to a power
//            of two, go through a bitonic sort in LDS; pi[slot_j] = e_j stays in LDS (the sort buffer is then reused for the tiles of Y).
//   product: features in tiles of PT <= 16 rows against all Q columns; 32 samples at a time, the rows of Y gathered through pi into LDS beside
//            the matching 32 x PT piece of the ranks; a thread owns 4 x 4 cells, sums 32 products in 32 bits (each below 2^26) and carries
//            them into 64 bits; where the cells are fewer than the threads, the 32 samples are split among the spare threads and the partial
//            sums meet in the LDS tile by 64-bit integer atomics.
//   reduce:  t per (p, c), the running maximum per c, the comparisons against obs; counts go to memory with integer atomics (counting per
//            block in LDS first was measured: no gain at 560 x 10 x 3, and its 32 KiB cost a block per CU at 4096 x 64 x 64).
// The identity permutation (obs, zc_obs) is a launch of one block of the same kernel with pi[d] = d.
#include "mmm_internal.h"
#include "mmm_perm.h"

#include <cmath>

namespace {

constexpr int kAsMaxD = 4096, kAsMaxP = 256, kAsMaxQ = 256;
constexpr int kAsIC = 32;                       // samples per staged chunk: 32 products below 2^26 fit 32 bits
constexpr int kAsPT = 16;                       // most feature rows of a tile (4 thread tiles of 4)
constexpr int kAsAutoWaves = 4;
constexpr size_t kAsLdsBlock = 160 * 1024;
constexpr uint32_t kAsBits = 0xE0000000u;       // second counter word: bits 31, 30 and 29 together are set by no other user

struct AsArgs {
    int D, P, C, Q, Qs, B, b0, n2, npt, ident;
    uint32_t k0, k1, stream;
    const uint16_t* rxt;             // [P][D] doubled midranks of the features
    const uint16_t* y;               // [D][Qs] columns of the covariates, rows padded with 0 to Qs = 4 ceil(Q / 4)
    const uint16_t* slot;            // [D] the samples in ascending (stratum, d)
    const uint16_t* strat;           // [D]
    const long long* cen;            // [Q] (D + 1) sum_d Y[d][q]
    const long long* w;              // [Q]
    const long long* ssx;            // [P]
    const int* col0;                 // [C + 1] first column of a covariate
    double* obs; long long* zc;      // [P][C], [P][Q]
    unsigned int* ge; unsigned int* gemax;      // [P][C]
    double* maxstat;                 // [B][C] or NULL
    int* counter;
};

struct AsLds { size_t z, tt, m, rs, pi, ctl, total; };

// the one place that lays a block's LDS out (host and device)
__host__ __device__ inline AsLds as_layout(int D, int C, int Qs, int n2, int npt)
{
    AsLds l;
    const size_t srt = 8 * (size_t)n2, til = 2 * (size_t)kAsIC * Qs, a = srt > til ? srt : til;      // the sort buffer, then the tile of Y
    l.z = (a + 15) & ~(size_t)15;
    l.tt = l.z + 8 * (size_t)(4 * npt) * Qs;
    l.m = l.tt + 8 * (size_t)(4 * npt) * C;
    l.rs = l.m + 8 * (size_t)C;
    l.pi = l.rs + 2 * (size_t)kAsIC * kAsPT;
    l.ctl = (l.pi + 2 * (size_t)D + 7) & ~(size_t)7;
    l.total = l.ctl + 8;
    return l;
}

__global__ __launch_bounds__(1024) void k_assoc(const AsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_as[];
    const int tid = threadIdx.x, nt = (int)blockDim.x;
    const int D = a.D, P = a.P, C = a.C, Q = a.Q, Qs = a.Qs, n2 = a.n2, nq4 = Qs >> 2, PT = 4 * a.npt;
    const AsLds L = as_layout(D, C, Qs, n2, a.npt);
    unsigned long long* keys = (unsigned long long*)s_as;
    uint16_t* Ys = (uint16_t*)s_as;                                      // [32][Qs], after the sort
    unsigned long long* Z = (unsigned long long*)(s_as + L.z);           // [PT][Qs]
    double* tt = (double*)(s_as + L.tt);                                 // [PT][C]
    double* M = (double*)(s_as + L.m);                                   // [C]
    uint16_t* Rs = (uint16_t*)(s_as + L.rs);                             // [32][16]
    uint16_t* pi = (uint16_t*)(s_as + L.pi);                             // [D]
    int* ctl = (int*)(s_as + L.ctl);
    // the thread's 4 x 4 cells and its share of a chunk
    const int groups = a.npt * nq4;                                      // <= nt by the host's choice of npt
    int S = 1;
    while (2 * S <= kAsIC && 2 * S * groups <= nt) S *= 2;
    const int g = tid % groups, sl = tid / groups, pg = g / nq4, qg = g - pg * nq4;
    const bool active = sl < S;
    const int per = kAsIC / S;

    for (;;) {
        int b = 0;
        if (!a.ident) {
            __syncthreads();
            if (tid == 0) ctl[0] = atomicAdd(a.counter, 1);
            __syncthreads();
            b = ctl[0];
            if (b >= a.B) break;
            // ---- sort
            perm_sorted_keys(keys, tid, nt, D, n2, a.strat, kAsBits, (uint32_t)(a.b0 + b), a.stream, a.k0, a.k1);
            for (int j = tid; j < D; j += nt) pi[a.slot[j]] = (uint16_t)(keys[j] & 0xFFFull);
        } else {
            for (int d = tid; d < D; d += nt) pi[d] = (uint16_t)d;
        }
        for (int c = tid; c < C; c += nt) M[c] = 0.0;
        __syncthreads();
        // ---- product and reduce, a tile of features at a time
        for (int p0 = 0; p0 < P; p0 += PT) {
            for (int e = tid; e < PT * Qs; e += nt) Z[e] = 0ull;
            unsigned long long acc64[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc64[j] = 0ull;
            for (int i0 = 0; i0 < D; i0 += kAsIC) {
                __syncthreads();
                for (int e = tid; e < kAsIC * PT; e += nt) {
                    const int pp = e / kAsIC, ii = e - pp * kAsIC, i = i0 + ii, p = p0 + pp;
                    Rs[ii * kAsPT + pp] = (i < D && p < P) ? a.rxt[(size_t)p * D + i] : (uint16_t)0;
                }
                for (int e = tid; e < kAsIC * nq4; e += nt) {
                    const int ii = e / nq4, q4 = e - ii * nq4, i = i0 + ii;
                    uint2 v = make_uint2(0u, 0u);
                    if (i < D) v = *(const uint2*)(a.y + (size_t)pi[i] * Qs + 4 * q4);
                    *(uint2*)(Ys + ii * Qs + 4 * q4) = v;
                }
                __syncthreads();
                if (active) {
                    uint32_t acc[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[j] = 0u;
                    for (int ii = sl * per; ii < (sl + 1) * per; ++ii) {
                        const uint2 r = *(const uint2*)(Rs + ii * kAsPT + 4 * pg), v = *(const uint2*)(Ys + ii * Qs + 4 * qg);
                        const uint32_t rr[4] = {r.x & 0xffffu, r.x >> 16, r.y & 0xffffu, r.y >> 16};
                        const uint32_t vv[4] = {v.x & 0xffffu, v.x >> 16, v.y & 0xffffu, v.y >> 16};
#pragma unroll
                        for (int jp = 0; jp < 4; ++jp)
#pragma unroll
                            for (int jq = 0; jq < 4; ++jq) acc[4 * jp + jq] += rr[jp] * vv[jq];
                    }
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc64[j] += acc[j];
                }
            }
            if (active) {
#pragma unroll
                for (int jp = 0; jp < 4; ++jp)
#pragma unroll
                    for (int jq = 0; jq < 4; ++jq) atomicAdd(&Z[(4 * pg + jp) * Qs + 4 * qg + jq], acc64[4 * jp + jq]);
            }
            __syncthreads();
            for (int e = tid; e < PT * C; e += nt) {
                const int pp = e / C, c = e - pp * C, p = p0 + pp;
                if (p >= P) continue;
                double t = 0.0;
                for (int q = a.col0[c]; q < a.col0[c + 1]; ++q) {
                    const long long wq = a.w[q];
                    if (wq == 0) continue;
                    const double dz = (double)((long long)Z[pp * Qs + q] - a.cen[q]);
                    t += (dz * dz) / (double)wq;
                }
                const long long ss = a.ssx[p];
                t = ss ? t / (double)ss : 0.0;
                tt[e] = t;
                if (a.ident) a.obs[(size_t)p * C + c] = t;
                else if (t >= a.obs[(size_t)p * C + c]) atomicAdd(&a.ge[(size_t)p * C + c], 1u);
            }
            if (a.ident && a.zc)
                for (int e = tid; e < PT * Q; e += nt) {
                    const int pp = e / Q, q = e - pp * Q, p = p0 + pp;
                    if (p < P) a.zc[(size_t)p * Q + q] = (long long)Z[pp * Qs + q] - a.cen[q];
                }
            __syncthreads();
            for (int c = tid; c < C; c += nt) {
                double m = M[c];
                for (int pp = 0; pp < PT && p0 + pp < P; ++pp) m = fmax(m, tt[pp * C + c]);
                M[c] = m;
            }
        }
        if (a.ident) break;
        __syncthreads();
        if (a.maxstat)
            for (int c = tid; c < C; c += nt) a.maxstat[(size_t)b * C + c] = M[c];
        for (int e = tid; e < P * C; e += nt)
            if (M[e % C] >= a.obs[e]) atomicAdd(&a.gemax[e], 1u);
    }
}

} // namespace

extern "C" int mmm_associate_exposures(mmm_ctx* ctx, int D, int P, const double* x, int C, const int32_t* levels, const double* y, const int32_t* strata, int B,
                                       int b0, uint64_t seed, uint32_t stream, int waves, double* obs, int64_t* zc_obs, uint32_t* ge, uint32_t* ge_max, double* maxstat)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, D >= 1 && P >= 1 && C >= 1, "mmm_associate_exposures: D = %d, P = %d, C = %d (>= 1 each)", D, P, C);
    if (D > kAsMaxD) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_associate_exposures: D = %d samples (limit %d)", D, kAsMaxD);
    if (P > kAsMaxP) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_associate_exposures: P = %d features (limit %d)", P, kAsMaxP);
    MMM_CHECK(ctx, x && levels && y && obs, "mmm_associate_exposures: NULL argument");
    int64_t Q64 = 0;
    for (int c = 0; c < C; ++c) {
        MMM_CHECK(ctx, levels[c] >= 0, "mmm_associate_exposures: levels[%d] = %d (>= 0)", c, levels[c]);
        Q64 += levels[c] ? levels[c] : 1;
    }
    if (Q64 > kAsMaxQ) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_associate_exposures: Q = %lld columns (limit %d)", (long long)Q64, kAsMaxQ);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0 && (int64_t)b0 + B <= 0x7fffffffLL, "mmm_associate_exposures: B = %d, b0 = %d (>= 0, b0 + B <= 2^31 - 1)", B, b0);
    MMM_CHECK(ctx, waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8 || waves == 16, "mmm_associate_exposures: waves = %d (0, 1, 2, 4, 8 or 16)", waves);
    MMM_CHECK(ctx, B == 0 || (ge && ge_max), "mmm_associate_exposures: NULL argument");
    for (size_t i = 0; i < (size_t)D * P; ++i)
        MMM_CHECK(ctx, std::isfinite(x[i]), "mmm_associate_exposures: x entry (%zu, %zu) is not finite", i / P, i % P);
    for (int d = 0; d < D; ++d)
        for (int c = 0; c < C; ++c) {
            const double v = y[(size_t)d * C + c];
            MMM_CHECK(ctx, std::isfinite(v), "mmm_associate_exposures: y entry (%d, %d) is not finite", d, c);
            MMM_CHECK(ctx, levels[c] == 0 || (v == std::floor(v) && v >= 0.0 && v < (double)levels[c]),
                      "mmm_associate_exposures: y entry (%d, %d) = %g is not a code in 0 .. %d", d, c, v, levels[c] - 1);
        }
    if (strata)
        for (int d = 0; d < D; ++d) MMM_CHECK(ctx, strata[d] >= 0 && strata[d] < D, "mmm_associate_exposures: strata[%d] = %d (0 .. D - 1)", d, strata[d]);

    // ---- ranks, weights and centring terms on the host: integers all
    const int Q = (int)Q64, Qs = (Q + 3) & ~3;
    std::vector<uint16_t> rxt((size_t)P * D), yq((size_t)D * Qs, 0), slot((size_t)D), strat((size_t)D);
    std::vector<long long> ssx((size_t)P, 0), w((size_t)Q, 0), cen((size_t)Q, 0);
    std::vector<int> col0((size_t)C + 1), idx((size_t)D);
    for (int p = 0; p < P; ++p) {
        perm_ranks(x + p, (size_t)P, D, idx, rxt.data() + (size_t)p * D, 1);
        for (int d = 0; d < D; ++d) {
            const long long dv = (long long)rxt[(size_t)p * D + d] - (D + 1);
            ssx[p] += dv * dv;
        }
    }
    int q0 = 0;
    for (int c = 0; c < C; ++c) {
        col0[c] = q0;
        if (levels[c] == 0) {
            perm_ranks(y + c, (size_t)C, D, idx, yq.data() + q0, (size_t)Qs);
            for (int d = 0; d < D; ++d) {
                const long long dv = (long long)yq[(size_t)d * Qs + q0] - (D + 1);
                w[q0] += dv * dv;
                cen[q0] += yq[(size_t)d * Qs + q0];
            }
            q0 += 1;
        } else {
            for (int d = 0; d < D; ++d) {
                const int gq = q0 + (int)y[(size_t)d * C + c];
                yq[(size_t)d * Qs + gq] = 1;
                w[gq] += 1;
                cen[gq] += 1;
            }
            q0 += levels[c];
        }
    }
    col0[C] = q0;
    for (int q = 0; q < Q; ++q) cen[q] *= (D + 1);
    for (int d = 0; d < D; ++d) { idx[d] = d; strat[d] = (uint16_t)(strata ? strata[d] : 0); }
    std::stable_sort(idx.begin(), idx.end(), [&](int i, int j) { return strat[i] < strat[j]; });
    for (int d = 0; d < D; ++d) slot[d] = (uint16_t)idx[d];

    int n2 = 1;
    while (n2 < D) n2 <<= 1;
    const int nw = waves ? waves : kAsAutoWaves, nt = 64 * nw, nq4 = Qs / 4;
    const int npt = std::max(1, std::min({(P + 3) / 4, kAsPT / 4, nt / nq4}));
    const AsLds L = as_layout(D, C, Qs, n2, npt);
    const size_t PC = (size_t)P * C;

    DevBuf<uint16_t> rxd, yd, slotd, stratd; DevBuf<long long> ssxd, wd, cend, zcd; DevBuf<int> col0d, counter; DevBuf<double> obsd, maxd; DevBuf<unsigned int> ged;
    MMM_HIP(ctx, rxd.alloc(rxt.size())); MMM_HIP(ctx, yd.alloc(yq.size())); MMM_HIP(ctx, slotd.alloc((size_t)D)); MMM_HIP(ctx, stratd.alloc((size_t)D));
    MMM_HIP(ctx, ssxd.alloc((size_t)P)); MMM_HIP(ctx, wd.alloc((size_t)Q)); MMM_HIP(ctx, cend.alloc((size_t)Q)); MMM_HIP(ctx, col0d.alloc((size_t)C + 1));
    MMM_HIP(ctx, counter.alloc(1)); MMM_HIP(ctx, obsd.alloc(PC)); MMM_HIP(ctx, ged.alloc(2 * PC));
    if (zc_obs) MMM_HIP(ctx, zcd.alloc((size_t)P * Q));
    if (maxstat && B > 0) MMM_HIP(ctx, maxd.alloc((size_t)B * C));
    MMM_HIP(ctx, hipMemcpyAsync(rxd.p, rxt.data(), sizeof(uint16_t) * rxt.size(), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(yd.p, yq.data(), sizeof(uint16_t) * yq.size(), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(slotd.p, slot.data(), sizeof(uint16_t) * (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(stratd.p, strat.data(), sizeof(uint16_t) * (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(ssxd.p, ssx.data(), sizeof(long long) * (size_t)P, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(wd.p, w.data(), sizeof(long long) * (size_t)Q, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(cend.p, cen.data(), sizeof(long long) * (size_t)Q, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(col0d.p, col0.data(), sizeof(int) * ((size_t)C + 1), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(ged.p, 0, sizeof(unsigned int) * 2 * PC, ctx->stream));

    AsArgs a;
    a.D = D; a.P = P; a.C = C; a.Q = Q; a.Qs = Qs; a.B = B; a.b0 = b0; a.n2 = n2; a.npt = npt; a.ident = 1;
    a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.rxt = rxd.p; a.y = yd.p; a.slot = slotd.p; a.strat = stratd.p; a.cen = cend.p; a.w = wd.p; a.ssx = ssxd.p; a.col0 = col0d.p;
    a.obs = obsd.p; a.zc = zc_obs ? zcd.p : nullptr; a.ge = ged.p; a.gemax = ged.p + PC; a.maxstat = (maxstat && B > 0) ? maxd.p : nullptr; a.counter = counter.p;
    if (L.total > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)k_assoc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total));
    hipLaunchKernelGGL(k_assoc, dim3(1), dim3(nt), L.total, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    if (B > 0) {
        const int cus = std::max(1, ctx->num_cu);
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(16 / nw, (int64_t)(kAsLdsBlock / L.total)));
        a.ident = 0;
        hipLaunchKernelGGL(k_assoc, dim3((unsigned)std::min<int64_t>(B, (int64_t)cus * per_cu)), dim3(nt), L.total, ctx->stream, a);
        MMM_LAUNCH_CHECK(ctx);
    }
    std::vector<double> obs_h(PC), max_h(a.maxstat ? (size_t)B * C : 0);
    std::vector<long long> zc_h(zc_obs ? (size_t)P * Q : 0);
    std::vector<unsigned int> ge_h(B > 0 ? 2 * PC : 0);
    MMM_HIP(ctx, hipMemcpyAsync(obs_h.data(), obsd.p, sizeof(double) * PC, hipMemcpyDeviceToHost, ctx->stream));
    if (zc_obs) MMM_HIP(ctx, hipMemcpyAsync(zc_h.data(), zcd.p, sizeof(long long) * zc_h.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (B > 0) MMM_HIP(ctx, hipMemcpyAsync(ge_h.data(), ged.p, sizeof(unsigned int) * 2 * PC, hipMemcpyDeviceToHost, ctx->stream));
    if (a.maxstat) MMM_HIP(ctx, hipMemcpyAsync(max_h.data(), maxd.p, sizeof(double) * max_h.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // the caller's arrays are written only now, after everything has succeeded
    std::copy(obs_h.begin(), obs_h.end(), obs);
    if (zc_obs) std::copy(zc_h.begin(), zc_h.end(), zc_obs);
    if (B > 0) { std::copy(ge_h.begin(), ge_h.begin() + PC, ge); std::copy(ge_h.begin() + PC, ge_h.end(), ge_max); }
    if (a.maxstat) std::copy(max_h.begin(), max_h.end(), maxstat);
    return MMM_OK;
}
