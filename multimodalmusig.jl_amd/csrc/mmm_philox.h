// mmm_philox.h -- the counter-based generator of the resampler (bootstrap.hip), the fold split (select.hip) and the starts of extract.hip,
// the categorical sampler built on it that simulate.hip and presence.hip share, and the resampler's draw counted by term (attribute.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) -----------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t u[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    u[0] = c0; u[1] = c1; u[2] = c2; u[3] = c3;
}

// ---- the categorical sampler of mmm_simulate_counts, which mmm_fit_check and mmm_presence_test draw from too (include/mmmusig.h has the
// definition; the draws of a replicate are part of it) -------------------------------------------------------------------------------------
constexpr uint32_t kSimBit = 0x80000000u;    // high bit of the third counter word: free in the resampler and the split (b, rep < 2^31)

// Block-level set-up, called by every thread once the block has written p[0..V) (the barrier after that pass opens this call).  One thread
// runs the sequential inclusive sum cum of p, S = cum[V - 1]; then T_v = floor((cum_v / S) 2^32), z = the number of leading terms with T_v = 0
// (which no word reaches; T is non-decreasing and T_{V-1} = 2^32: the zeros lead, z <= V - 1), thr[v - z] = T_v - 1 for v >= z, padded
// with 0xffffffff to the power of two P2.  cum is scratch and may alias what the caller uses AFTER its next __syncthreads(): that barrier,
// which closes the set-up (the running sums are read, thr is written), is left to the caller, who may have a pass over p to put before it.
// ok == false (S not positive or not finite; the hosts refuse such input): no thresholds, nothing may be drawn -- the whole block returns.
struct DrawSetup {
    double S;
    int z;
    bool ok;
};

__device__ __forceinline__ DrawSetup draw_thresholds(int tid, int nt, int V, int P2, const double* p, double* cum, int* s_z, uint32_t* thr)
{
    __syncthreads();
    if (tid == 0) {
        double c = 0.0;
        for (int v = 0; v < V; ++v) { c += p[v]; cum[v] = c; }
        *s_z = 0;
    }
    __syncthreads();
    DrawSetup r;
    r.S = cum[V - 1]; r.z = 0;
    r.ok = r.S > 0.0 && r.S <= 1.7976931348623157e308;
    if (!r.ok) return r;
    const double two32 = 4294967296.0;
    int nz = 0;
    for (int v = tid; v < V; v += nt) nz += (unsigned long long)((cum[v] / r.S) * two32) == 0ull;
    if (nz) atomicAdd(s_z, nz);
    __syncthreads();
    r.z = *s_z;
    for (int v = tid; v < V; v += nt) {
        const unsigned long long T = (unsigned long long)((cum[v] / r.S) * two32);       // floor: the product is exact and >= 0
        if (v >= r.z) thr[v - r.z] = (uint32_t)(T - 1ull);
    }
    for (int j = V - r.z + tid; j < P2; j += nt) thr[j] = 0xffffffffu;
    return r;
}

// One wave draws the N draws of one (item, replicate) pair, 64 Philox blocks (256 draws) per step, into hist[0..V) with integer atomics
// (Hist: int or uint32_t).  The draw of the word u is z + the number of j with thr[j] < u = the first v with T_v > u.  thr[V - z - 1] =
// 2^32 - 1 is never < u, so the result is <= V - 1.  The same log2(P2) steps for every lane, no bound checks, a lane's four draws side by side.
template <class Hist>
__device__ __forceinline__ void draw_row(int lane, int P2, int z, uint32_t N, const uint32_t* thr, Hist* hist, uint32_t item, uint32_t b, uint32_t stream,
                                         uint32_t k0, uint32_t k1)
{
    const uint32_t nblk = (N + 3u) >> 2;                       // N < 2^31
    for (uint32_t i4 = (uint32_t)lane; i4 < nblk; i4 += 64u) {
        uint32_t u[4];
        int pos[4];
        philox4x32_10(i4, item, kSimBit | b, stream, k0, k1, u);
#pragma unroll
        for (int j = 0; j < 4; ++j) pos[j] = 0;
        for (int step = P2 >> 1; step > 0; step >>= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (thr[pos[j] + step - 1] < u[j]) pos[j] += step;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4u * i4 + (uint32_t)j < N) atomicAdd(&hist[z + pos[j]], (Hist)1);
    }
}

// ---- the draw of mmm_resample_counts (bootstrap.hip, rs_draw_row_lds: the counter (i / 4, d, b, stream), r = (u N) >> 32, the first entry
// e with cum[e] > r), counted by TERM: hist[eterm[e]] takes the draw that lands in entry e, so the wave leaves the replicate's dense count
// vector (duplicate terms summed) where the resampler leaves the counts per entry.  cum[0..W): the document's inclusive prefix sums in CSR
// order, cum[W-1] = N, padded with 0xffffffff to the power of two 2 * half >= W (half = 0 for W = 1); eterm[0..W): the entries' terms.
template <class Hist>
__device__ __forceinline__ void resample_row_terms(int lane, int half, uint32_t N, const uint32_t* cum, const int* eterm, Hist* hist, uint32_t d, uint32_t b,
                                                   uint32_t stream, uint32_t k0, uint32_t k1)
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
            if (4u * i4 + (uint32_t)j < N) atomicAdd(&hist[eterm[pos[j]]], (Hist)1);     // cum[W-1] = N > r: pos <= W - 1
    }
}
