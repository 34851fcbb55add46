// refit_reduce.cuh -- the wave-level pieces of fit(A) (include/mmmusig.h, mmm_refit_exposures) that refit.hip and presence.hip share: the
// wave fence and the TRANSPOSING butterfly that totals the 64 partial sums of up to 32 signatures at once.  Lane l owns the terms
// v = l, l + 64, ...; the order of every addition is the definition's, so both units give the bits of the restatement.
#pragma once
#include "dev_math.h"

__device__ __forceinline__ void rf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// g[j], j < 2^LOG: this lane's partial sums of 2^LOG signatures.  Returns, in lane l, the butterfly total (l ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1) of
// signature j = l >> (6 - LOG): LOG transposing steps, then 6 - LOG plain ones.
template <int LOG, int S>
__device__ __forceinline__ void rf_transpose_steps(double (&g)[1 << LOG], int lane)
{
    if constexpr (S < LOG) {
        constexpr int h = (1 << LOG) >> (S + 1), off = 32 >> S;
        if constexpr (off >= 16) {
#pragma unroll
            for (int i = 0; i < h; ++i) {
                // x = g[i], y = g[i + h]: after the swap the lanes without bit `off` hold (own g[i], partner's g[i]), the lanes with it
                // (partner's g[i + h], own g[i + h])
                const unsigned xl = (unsigned)__double2loint(g[i]), xh = (unsigned)__double2hiint(g[i]);
                const unsigned yl = (unsigned)__double2loint(g[i + h]), yh = (unsigned)__double2hiint(g[i + h]);
                const mmm_u2 a = off == 32 ? __builtin_amdgcn_permlane32_swap(xl, yl, false, false) : __builtin_amdgcn_permlane16_swap(xl, yl, false, false);
                const mmm_u2 b = off == 32 ? __builtin_amdgcn_permlane32_swap(xh, yh, false, false) : __builtin_amdgcn_permlane16_swap(xh, yh, false, false);
                g[i] = __hiloint2double((int)b.x, (int)a.x) + __hiloint2double((int)b.y, (int)a.y);
            }
        } else {
            const bool up = (lane & off) != 0;
#pragma unroll
            for (int i = 0; i < h; ++i) {
                const double send = up ? g[i] : g[i + h];
                const double keep = up ? g[i + h] : g[i];
                g[i] = keep + __shfl_xor(send, off, 64);
            }
        }
        rf_transpose_steps<LOG, S + 1>(g, lane);
    }
}

template <int LOG>
__device__ __forceinline__ double rf_reduce(double (&g)[1 << LOG], int lane)
{
    rf_transpose_steps<LOG, 0>(g, lane);
    double v = g[0];
#pragma unroll
    for (int s = LOG; s < 6; ++s) v += __shfl_xor(v, 32 >> s, 64);
    return v;
}

// the totals g_c of the 2^LOG signatures act[0 .. 2^LOG) (padded with a valid row): per lane the terms v = lane, lane + 64, ... ascending
template <int LOG>
__device__ __forceinline__ double rf_gchunk(const double* __restrict__ P, const int* __restrict__ act, const double* __restrict__ r, int V, int lane)
{
    constexpr int W = 1 << LOG;
    double g[W];
    int row[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { g[j] = 0.0; row[j] = act[j] * V; }
    for (int v = lane; v < V; v += 64) {
        const double rv = r[v];
#pragma unroll
        for (int j = 0; j < W; ++j) g[j] += rv * P[row[j] + v];
    }
    return rf_reduce<LOG>(g, lane);
}
