// mixture_fit.cuh -- fit(A) (include/mmmusig.h, mmm_refit_exposures) for one wave, the one copy that refit.hip and presence.hip run and
// whose weight update extract.hip takes: the wave fence, the TRANSPOSING butterfly that totals the 64 partial sums of up to 32 signatures
// at once, the EM loop with its two sweeps, the normalisation, the ll / u (/ score) sweep, the lists of active signatures and the work
// counter.  Lane l owns the terms v = l, l + 64, ...; the order of every addition is the definition's, so every unit gives the bits of the
// restatement.  All buffers are the wave's own (LDS, or global memory behind the caller's fences).
#pragma once
#include <cstdint>
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

// The count vector of a document as fit(A) reads it: is term v present, and n_v as a double.  refit.hip keeps integer-valued doubles,
// presence.hip the histogram its draws land in (converted where a value is needed, never for the presence test).
struct RfCountsF64 {
    const double* n;
    __device__ __forceinline__ bool present(int v) const { return n[v] > 0.0; }
    __device__ __forceinline__ double value(int v) const { return n[v]; }
};
struct RfCountsU32 {
    const uint32_t* n;
    __device__ __forceinline__ bool present(int v) const { return n[v] != 0u; }
    __device__ __forceinline__ double value(int v) const { return (double)n[v]; }
};

// r_v = f_v / q_v where n_v > 0 and q_v > 0 (else 0), q_v = sum_i w[i] P[act[i]][v] in the order of the list.  Two of the lane's terms
// at a time: their sums are independent chains (each still in the order of c).
template <class Counts>
__device__ __forceinline__ void rf_ratios(const double* __restrict__ P, const int* act, const double* w, int n, const double* f, const Counts counts,
                                          double* r, int V, int lane)
{
    for (int v = lane; v < V; v += 128) {
        const bool two = v + 64 < V;
        const int v1 = two ? v + 64 : v;
        double q = 0.0, q1 = 0.0;
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const double wi = w[i];
            const int row = act[i] * V;
            q += wi * P[row + v];
            q1 += wi * P[row + v1];
        }
        r[v] = (counts.present(v) && q > 0.0) ? f[v] / q : 0.0;
        if (two) r[v1] = (counts.present(v1) && q1 > 0.0) ? f[v1] / q1 : 0.0;
    }
}

// w[i] <- w[i] g_i for the n rows of the list act (padded to a multiple of 64 with a valid row whose results are dropped), g_i = sum_v r_v
// P[act[i]][v]: 32 rows at a time through the narrowest butterfly that holds them.  Returns this lane's max |w' - w|; the caller fences.
__device__ __forceinline__ double rf_update_weights(const double* __restrict__ P, const int* act, double* w, int n, const double* r, int V, int lane)
{
    double md = 0.0;
    for (int b = 0; b < n; b += 32) {
        const int m = min(32, n - b);
        double g; int j;
        if (m <= 4) { g = rf_gchunk<2>(P, act + b, r, V, lane); j = lane >> 4; }
        else if (m <= 8) { g = rf_gchunk<3>(P, act + b, r, V, lane); j = lane >> 3; }
        else if (m <= 16) { g = rf_gchunk<4>(P, act + b, r, V, lane); j = lane >> 2; }
        else { g = rf_gchunk<5>(P, act + b, r, V, lane); j = lane >> 1; }
        if (j < m) {
            const double wo = w[b + j], wn = wo * g;
            md = fmax(md, fabs(wn - wo));
            w[b + j] = wn;           // the lanes that share j write the same bits
        }
    }
    return md;
}

// w <- w / sum_i w[i], the sum sequential in the order of the list; left as it is when the sum is 0
__device__ __forceinline__ void rf_normalise(double* w, int n, int lane)
{
    double S = 0.0;
    for (int i = 0; i < n; ++i) S += w[i];
    rf_wave_sync();
    if (S > 0.0)
        for (int i = lane; i < n; i += 64) w[i] = w[i] / S;
    rf_wave_sync();
}

// fit(A) for the list act: cold start, EM until max |w' - w| < tol or maxiter, normalised weights in w.  r is scratch.  Returns the iterations.
template <class Counts>
__device__ __forceinline__ int rf_fit(const double* __restrict__ P, const int* act, double* w, int n, const double* f, const Counts counts, double* r, int V,
                                      int lane, int maxiter, double tol)
{
    const double w0 = 1.0 / (double)n;
    for (int i = lane; i < n; i += 64) w[i] = w0;
    rf_wave_sync();
    int it = 0;
    while (it < maxiter) {
        ++it;
        rf_ratios(P, act, w, n, f, counts, r, V, lane);
        rf_wave_sync();
        const double md = rf_update_weights(P, act, w, n, r, V, lane);
        rf_wave_sync();
        if (wave_max(md) < tol) break;
    }
    rf_normalise(w, n, lane);
    return it;
}

// ll = sum n_v log q_v over n_v > 0, q_v > 0; u = sum n_v over n_v > 0, q_v = 0; with SCORE and trow >= 0 also s = sum (f_v / q_v)
// P[trow][v] over the terms of ll (SCORE compiles the score in, trow switches it at run time: a caller whose two fits share ONE call
// site keeps one copy of the sweep -- two copies cost presence.hip's kernels the registers that hold the butterflies' lane addresses
// across the EM loop).  The lane is the partial sum, wave_sum the butterfly.
struct RfLoglik {
    double ll, u, s;
};

template <bool SCORE, class Counts>
__device__ __forceinline__ RfLoglik rf_loglik(const double* __restrict__ P, const int* act, const double* w, int n, const Counts counts, const double* f,
                                              int trow, int V, int lane)
{
    double lp = 0.0, up = 0.0, sp = 0.0;
    for (int v = lane; v < V; v += 64) {
        double q = 0.0;
        for (int i = 0; i < n; ++i) q += w[i] * P[act[i] * V + v];
        if (counts.present(v)) {
            const double nv = counts.value(v);
            if (q > 0.0) {
                lp += nv * log(q);
                if (SCORE && trow >= 0) sp += (f[v] / q) * P[trow * V + v];
            } else up += nv;
        }
    }
    RfLoglik r;
    r.ll = wave_sum(lp); r.u = wave_sum(up); r.s = (SCORE && trow >= 0) ? wave_sum(sp) : 0.0;
    return r;
}

// The rows c < C with allowed[c] != 0 (allowed == NULL: all), and the row `extra` whatever allowed says (-1: none), as a list in the
// order of c.  Returns its length; pos: the place of `extra` in it.
__device__ __forceinline__ int rf_active_list(const uint8_t* allowed, int C, int extra, int* act, int lane, int& pos)
{
    int n = 0, p = 0;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const bool on = c < C && (c == extra || (allowed ? allowed[c] != 0 : true));
        const unsigned long long m = __ballot(on);
        if (on) act[n + __popcll(m & ((1ull << lane) - 1ull))] = c;
        if (c0 == (extra & ~63)) p = n + __popcll(m & ((1ull << (extra & 63)) - 1ull));
        n += __popcll(m);
    }
    rf_wave_sync();
    pos = p;
    return n;
}

// pads a list of n >= 1 rows to a multiple of 64 with its first row
__device__ __forceinline__ void rf_pad_list(int* act, int n, int lane)
{
    for (int i = n + lane; i < ((n + 63) & ~63); i += 64) act[i] = act[0];
}

// dst = the n rows of src without the one at pos (n - 1 rows, unpadded)
__device__ __forceinline__ void rf_list_without(const int* src, int* dst, int n, int pos, int lane)
{
    for (int i = lane; i < n - 1; i += 64) dst[i] = src[i < pos ? i : i + 1];
    rf_wave_sync();
}

// The next item of a work counter: lane 0 fetches, the wave takes it from lane 0.  CONTRACT for the caller's loop: every path through its
// body reaches the loop's closing rf_wave_sync() with the whole wave, and no `continue` sits between a lane-0 store and the next fetch.
// A `continue` after a lane-0 store lets the compiler thread lane 0 straight into the lane-0 fetch of the next item, and the other 63
// lanes then take their item from a lane that is not there (seen in k_presence_obs' ISA before it took this shape).
__device__ __forceinline__ int rf_next_item(int* counter, int lane)
{
    int j = 0;
    if (lane == 0) j = atomicAdd(counter, 1);
    return __shfl(j, 0, 64);
}
