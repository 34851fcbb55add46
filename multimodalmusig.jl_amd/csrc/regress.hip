// regress.hip -- mmm_regress_exposures: the Freedman-Lane permutation test of a linear model.  P features' residuals on the adjusters against
// A orthonormal adjuster columns and C tested covariates (Q orthonormal columns) over D samples, B permutations of the residual rows (within
// strata) in one launch, with the per-covariate maximum of every permutation for Westfall-Young adjusted p-values (no counterpart in the
// reference; include/mmmusig.h has the normative definition, DESIGN.md section 4.27 the reasoning).
//
// The host lays the design [qz | w] and the residuals out in padded rows and forms ss_p; everything else is the device's, in f64, every sum in
// the written stripe order, no contraction, no matrix instruction (its internally ordered sums cannot be restated).
// k_regress: one workgroup runs one permutation; permutations beyond the resident blocks are handed out through a work counter.
//   sort:    perm_sorted_keys (mmm_perm.h, shared with k_assoc); pi[slot_j] = e_j stays in LDS as 16-bit indices.
//   product: a group of 16 neighbouring lanes owns a TR x TP tile of cells (design columns x features); lane s of the group walks stripe s
//            (slots s, s + 16, ..) in ascending order, loads the slot's TR design values and TP residuals once and adds the TR TP separately
//            rounded products; the 16 stripe sums of a cell meet by shuffles in ascending stripe order.  Placement: when the block's LDS stays
//            within kRgLdsRows the design (once per block) and the gathered rows e[pi(i)] (once per permutation, over the sort buffer) are
//            held in LDS, else every read goes to memory, the residual row through pi.  The sums do not know where the operands came from.
//   reduce:  a thread per (p, c) forms rz, num and t in the written order (t lies over the sort buffer, which is done with by then); the
//            running maximum per c in LDS; the comparisons against obs; the counts go to memory with 32-bit integer atomics.
// Measured: 4 waves per block, 8 from kRgBigTiles 4 x 4 tiles on; staging the memory placement through LDS in
// chunks of 64 slots was slower at 4 and 8 waves and is not kept.
// The identity permutation (obs, u_obs, rz_obs) is a launch of one block of the same kernel with pi[d] = d.
#include "mmm_internal.h"
#include "mmm_perm.h"

#include <cmath>

namespace {

constexpr int kRgMaxD = 4096, kRgMaxP = 64, kRgMaxA = 32, kRgMaxQ = 64;
constexpr double kRgMaxAbs = 1e70;               // keeps every product, square and sum of the definition finite: no NaN reaches a maximum
constexpr int kRgAutoWaves = 4, kRgAutoWavesBig = 8;                 // the library's waves per block; the second from kRgBigTiles 4 x 4 tiles on
constexpr int kRgBigTiles = 128;
constexpr size_t kRgLdsBlock = 160 * 1024;
constexpr size_t kRgLdsRows = 80 * 1024;        // the design and the gathered rows go to LDS while the whole block stays within this: two blocks share a CU
constexpr uint32_t kRgBits = 0xF0000000u;       // second counter word: bits 31, 30, 29 and 28 together are set by no other user

struct RgArgs {
    int D, P, A, C, Q, B, b0, n2, ident;
    int Re, Pe;                      // doubles per padded row of the design and of the residuals
    int ntr, ntp;                    // tiles along the design columns and along the features
    uint32_t k0, k1, stream;
    const double* x;                 // [D][Re] the design: the A columns of qz, then the Q columns of w, then zeros
    const double* e;                 // [D][Pe] the residuals, then zeros
    const double* ss;                // [P]
    const uint16_t* slot;            // [D] the samples in ascending (stratum, d)
    const uint16_t* strat;           // [D]
    const int* col0;                 // [C + 1] first column of a covariate, among the Q
    double* obs; double* u; double* rz;         // [P][C], [P][Q] or NULL, [P] or NULL
    unsigned int* ge; unsigned int* gemax;      // [P][C]
    double* maxstat;                 // [B][C] or NULL
    int* counter;
};

struct RgLds { size_t er, xr, g, tt, m, pi, ctl, total; };

// a padded row: `n` rounded up to a multiple of the tile's side, then to an odd number of 16-byte units, so that the 16 lanes of a group, which
// read 16 consecutive rows at one column, fall on 16 different groups of four LDS banks
__host__ __device__ inline int rg_row(int n, int side)
{
    const int t = (n + side - 1) / side * side;
    return ((t >> 1) & 1) ? t : t + 2;
}

// the one place that lays a block's LDS out (host and device)
__host__ __device__ inline RgLds rg_layout(int D, int P, int C, int Re, int Pe, int n2, bool rows)
{
    RgLds l;
    // one region in turn: the sort buffer, then the gathered rows, then t of the permutation
    const size_t srt = 8 * (size_t)n2, er = rows ? 8 * (size_t)D * Pe : 0, tt = 8 * (size_t)P * C, a = srt > er ? srt : er;
    l.er = 0;
    l.tt = 0;
    l.xr = ((a > tt ? a : tt) + 15) & ~(size_t)15;
    l.g = l.xr + (rows ? 8 * (size_t)D * Re : 0);
    l.m = l.g + 8 * (size_t)Re * Pe;
    l.pi = l.m + 8 * (size_t)C;
    l.ctl = (l.pi + 2 * (size_t)D + 7) & ~(size_t)7;
    l.total = l.ctl + 8;
    return l;
}

template <int N> struct RgVec { double v[N]; };

template <int N> __device__ __forceinline__ RgVec<N> rg_load(const double* p)
{
    RgVec<N> r;
#pragma unroll
    for (int j = 0; j < N; j += 2) {
        const double2 t = *(const double2*)(p + j);
        r.v[j] = t.x; r.v[j + 1] = t.y;
    }
    return r;
}

template <int TR, int TP, bool kRows>
__global__ __launch_bounds__(1024) void k_regress(const RgArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_rg[];
    const int tid = threadIdx.x, nt = (int)blockDim.x, lane = tid & 63;
    const int D = a.D, P = a.P, A = a.A, C = a.C, Q = a.Q, Re = a.Re, Pe = a.Pe;
    const RgLds L = rg_layout(D, P, C, Re, Pe, a.n2, kRows);
    unsigned long long* keys = (unsigned long long*)s_rg;
    double* Er = (double*)(s_rg + L.er);                                 // [D][Pe], after the sort
    double* Xr = (double*)(s_rg + L.xr);                                 // [D][Re]
    double* G = (double*)(s_rg + L.g);                                   // [Re][Pe]: a_j in the rows j < A, u_q in the rows A + q
    double* tt = (double*)(s_rg + L.tt);                                 // [P][C], after the product
    double* M = (double*)(s_rg + L.m);                                   // [C]
    uint16_t* pi = (uint16_t*)(s_rg + L.pi);                             // [D]
    int* ctl = (int*)(s_rg + L.ctl);
    const int grp = tid >> 4, ngrp = nt >> 4, s = tid & 15, ntile = a.ntr * a.ntp;

    if (kRows)
        for (int i2 = tid; 2 * i2 < D * Re; i2 += nt) *(double2*)(Xr + 2 * i2) = *(const double2*)(a.x + 2 * (size_t)i2);

    for (;;) {
        int b = 0;
        if (!a.ident) {
            __syncthreads();
            if (tid == 0) ctl[0] = atomicAdd(a.counter, 1);
            __syncthreads();
            b = ctl[0];
            if (b >= a.B) break;
            // ---- sort
            perm_sorted_keys(keys, tid, nt, D, a.n2, a.strat, kRgBits, (uint32_t)(a.b0 + b), a.stream, a.k0, a.k1);
            for (int j = tid; j < D; j += nt) pi[a.slot[j]] = (uint16_t)(keys[j] & 0xFFFull);
        } else {
            for (int d = tid; d < D; d += nt) pi[d] = (uint16_t)d;
        }
        __syncthreads();
        if (kRows) {                                                     // slot i receives the residual row of pi(i); the keys are done with
            const int pe2 = Pe >> 1;
            for (int i2 = tid; i2 < D * pe2; i2 += nt) {
                const int i = i2 / pe2, c2 = i2 - i * pe2;
                *(double2*)(Er + (size_t)i * Pe + 2 * c2) = *(const double2*)(a.e + (size_t)pi[i] * Pe + 2 * c2);
            }
            __syncthreads();
        }
        // ---- product: G[r][p] = dot(x[.][r], e[pi(.)][p]) in the stripe order
        for (int t0 = 0; t0 < ntile; t0 += ngrp) {
            const int t = t0 + grp;
            const bool on = t < ntile;
            const int tr = on ? t / a.ntp : 0, tp = on ? t - tr * a.ntp : 0;
            double acc[TR][TP];
#pragma unroll
            for (int jr = 0; jr < TR; ++jr)
#pragma unroll
                for (int jp = 0; jp < TP; ++jp) acc[jr][jp] = 0.0;
            if (on)
                for (int i = s; i < D; i += 16) {
                    const RgVec<TR> xv = rg_load<TR>((kRows ? Xr : a.x) + (size_t)i * Re + TR * tr);
                    const RgVec<TP> ev = rg_load<TP>(kRows ? Er + (size_t)i * Pe + TP * tp : a.e + (size_t)pi[i] * Pe + TP * tp);
#pragma unroll
                    for (int jr = 0; jr < TR; ++jr)
#pragma unroll
                        for (int jp = 0; jp < TP; ++jp) acc[jr][jp] = acc[jr][jp] + xv.v[jr] * ev.v[jp];
                }
#pragma unroll
            for (int jr = 0; jr < TR; ++jr)
#pragma unroll
                for (int jp = 0; jp < TP; ++jp) {
                    double tot = 0.0;
#pragma unroll
                    for (int s2 = 0; s2 < 16; ++s2) tot = tot + __shfl(acc[jr][jp], (lane & ~15) + s2);
                    if (on && s == 0) G[(TR * tr + jr) * Pe + TP * tp + jp] = tot;
                }
        }
        __syncthreads();
        // ---- reduce
        for (int e = tid; e < P * C; e += nt) {
            const int p = e / C, c = e - p * C;
            double fit = 0.0;
            for (int j = 0; j < A; ++j) {
                const double g = G[j * Pe + p];
                fit = fit + g * g;
            }
            const double rz = a.ss[p] - fit;
            double num = 0.0;
            for (int q = a.col0[c]; q < a.col0[c + 1]; ++q) {
                const double u = G[(A + q) * Pe + p];
                num = num + u * u;
            }
            const double t = rz > 0.0 ? num / rz : 0.0;
            tt[e] = t;
            if (a.ident) {
                a.obs[e] = t;
                if (c == 0 && a.rz) a.rz[p] = rz;
            } else if (t >= a.obs[e]) atomicAdd(&a.ge[e], 1u);
        }
        if (a.ident && a.u)
            for (int e = tid; e < P * Q; e += nt) {
                const int p = e / Q, q = e - p * Q;
                a.u[e] = G[(A + q) * Pe + p];
            }
        if (a.ident) break;
        __syncthreads();
        for (int c = tid; c < C; c += nt) {
            double m = 0.0;
            for (int p = 0; p < P; ++p) m = fmax(m, tt[p * C + c]);
            M[c] = m;
        }
        __syncthreads();
        if (a.maxstat)
            for (int c = tid; c < C; c += nt) a.maxstat[(size_t)b * C + c] = M[c];
        for (int e = tid; e < P * C; e += nt)
            if (M[e % C] >= a.obs[e]) atomicAdd(&a.gemax[e], 1u);
    }
}

// dot(f, f) in the stripe order of the definition, on the host (the build has no contraction here either)
double rg_ss(const double* f, size_t stride, int D)
{
    double stripe[16];
    for (int s = 0; s < 16; ++s) {
        double acc = 0.0;
        for (int i = s; i < D; i += 16) {
            const double v = f[(size_t)i * stride], pr = v * v;
            acc = acc + pr;
        }
        stripe[s] = acc;
    }
    double tot = 0.0;
    for (int s = 0; s < 16; ++s) tot = tot + stripe[s];
    return tot;
}

template <int TR, int TP, bool kRows>
int rg_launch(mmm_ctx* ctx, RgArgs& a, const RgLds& L, int nt, int nw)
{
    const void* fn = (const void*)k_regress<TR, TP, kRows>;
    if (L.total > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total));
    a.ident = 1;
    hipLaunchKernelGGL((k_regress<TR, TP, kRows>), dim3(1), dim3(nt), L.total, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    if (a.B > 0) {
        const int cus = std::max(1, ctx->num_cu);
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(16 / nw, (int64_t)(kRgLdsBlock / L.total)));
        a.ident = 0;
        hipLaunchKernelGGL((k_regress<TR, TP, kRows>), dim3((unsigned)std::min<int64_t>(a.B, (int64_t)cus * per_cu)), dim3(nt), L.total, ctx->stream, a);
        MMM_LAUNCH_CHECK(ctx);
    }
    return MMM_OK;
}

} // namespace

extern "C" int mmm_regress_exposures(mmm_ctx* ctx, int D, int P, const double* e, int A, const double* qz, int C, const int32_t* cols, const double* w,
                                     const int32_t* strata, int B, int b0, uint64_t seed, uint32_t stream, int waves, double* obs, double* u_obs, double* rz_obs,
                                     uint32_t* ge, uint32_t* ge_max, double* maxstat)
{
    if (!ctx) return MMM_ERR_ARG;
    // ---- every argument, before a device is asked for
    MMM_CHECK(ctx, D >= 1 && P >= 1 && C >= 1 && A >= 0, "mmm_regress_exposures: D = %d, P = %d, C = %d (>= 1 each), A = %d (>= 0)", D, P, C, A);
    if (D > kRgMaxD) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_regress_exposures: D = %d samples (limit %d)", D, kRgMaxD);
    if (P > kRgMaxP) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_regress_exposures: P = %d features (limit %d)", P, kRgMaxP);
    if (A > kRgMaxA) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_regress_exposures: A = %d adjuster columns (limit %d)", A, kRgMaxA);
    MMM_CHECK(ctx, e && cols && w && obs && (A == 0 || qz), "mmm_regress_exposures: NULL argument");
    int64_t Q64 = 0;
    for (int c = 0; c < C; ++c) {
        MMM_CHECK(ctx, cols[c] >= 1, "mmm_regress_exposures: cols[%d] = %d (>= 1)", c, cols[c]);
        Q64 += cols[c];
        if (Q64 > kRgMaxQ) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_regress_exposures: Q = %lld tested columns up to covariate %d (limit %d)", (long long)Q64, c, kRgMaxQ);
    }
    for (int c = 0; c < C; ++c)
        MMM_CHECK(ctx, D - A - cols[c] >= 1, "mmm_regress_exposures: covariate %d leaves D - A - cols = %d - %d - %d residual degrees of freedom (>= 1)", c, D, A, cols[c]);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0 && (int64_t)b0 + B <= 0x7fffffffLL, "mmm_regress_exposures: B = %d, b0 = %d (>= 0, b0 + B <= 2^31 - 1)", B, b0);
    MMM_CHECK(ctx, waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8 || waves == 16, "mmm_regress_exposures: waves = %d (0, 1, 2, 4, 8 or 16)", waves);
    MMM_CHECK(ctx, B == 0 || (ge && ge_max), "mmm_regress_exposures: NULL argument");
    const int Q = (int)Q64, R = A + Q;
    for (size_t i = 0; i < (size_t)D * P; ++i)
        MMM_CHECK(ctx, std::fabs(e[i]) <= kRgMaxAbs, "mmm_regress_exposures: e entry (%zu, %zu) is not finite or beyond 1e70 in magnitude", i / P, i % P);
    for (size_t i = 0; i < (size_t)D * A; ++i)
        MMM_CHECK(ctx, std::fabs(qz[i]) <= kRgMaxAbs, "mmm_regress_exposures: qz entry (%zu, %zu) is not finite or beyond 1e70 in magnitude", i / A, i % A);
    for (size_t i = 0; i < (size_t)D * Q; ++i)
        MMM_CHECK(ctx, std::fabs(w[i]) <= kRgMaxAbs, "mmm_regress_exposures: w entry (%zu, %zu) is not finite or beyond 1e70 in magnitude", i / Q, i % Q);
    if (strata)
        for (int d = 0; d < D; ++d) MMM_CHECK(ctx, strata[d] >= 0 && strata[d] < D, "mmm_regress_exposures: strata[%d] = %d (0 .. D - 1)", d, strata[d]);
    MMM_HIP(ctx, hipSetDevice(ctx->device));

    // ---- geometry: 4 x 4 tiles where they fill the block, else 2 x 2; padded rows; the placement
    const int tiles44 = ((R + 3) / 4) * ((P + 3) / 4);
    const int nw = waves ? waves : (tiles44 >= kRgBigTiles ? kRgAutoWavesBig : kRgAutoWaves), nt = 64 * nw;
    const bool big = tiles44 * 16 >= nt;
    const int side = big ? 4 : 2, Re = rg_row(R, side), Pe = rg_row(P, side);
    int n2 = 1;
    while (n2 < D) n2 <<= 1;
    const bool rows = rg_layout(D, P, C, Re, Pe, n2, true).total <= kRgLdsRows;
    const RgLds L = rg_layout(D, P, C, Re, Pe, n2, rows);

    // ---- the padded design and residuals, ss_p, the strata order
    std::vector<double> xh((size_t)D * Re, 0.0), eh((size_t)D * Pe, 0.0), ssh((size_t)P);
    for (int d = 0; d < D; ++d) {
        for (int j = 0; j < A; ++j) xh[(size_t)d * Re + j] = qz[(size_t)d * A + j];
        for (int q = 0; q < Q; ++q) xh[(size_t)d * Re + A + q] = w[(size_t)d * Q + q];
        for (int p = 0; p < P; ++p) eh[(size_t)d * Pe + p] = e[(size_t)d * P + p];
    }
    for (int p = 0; p < P; ++p) ssh[p] = rg_ss(e + p, (size_t)P, D);
    std::vector<uint16_t> slot((size_t)D), strat((size_t)D);
    std::vector<int> col0((size_t)C + 1, 0), idx((size_t)D);
    for (int c = 0; c < C; ++c) col0[c + 1] = col0[c] + cols[c];
    for (int d = 0; d < D; ++d) { idx[d] = d; strat[d] = (uint16_t)(strata ? strata[d] : 0); }
    std::stable_sort(idx.begin(), idx.end(), [&](int i, int j) { return strat[i] < strat[j]; });
    for (int d = 0; d < D; ++d) slot[d] = (uint16_t)idx[d];

    const size_t PC = (size_t)P * C, PQ = (size_t)P * Q;
    DevBuf<double> xd, ed, ssd, obsd, ud, rzd, maxd; DevBuf<uint16_t> slotd, stratd; DevBuf<int> col0d, counter; DevBuf<unsigned int> ged;
    MMM_HIP(ctx, xd.alloc(xh.size())); MMM_HIP(ctx, ed.alloc(eh.size())); MMM_HIP(ctx, ssd.alloc((size_t)P)); MMM_HIP(ctx, obsd.alloc(PC));
    MMM_HIP(ctx, slotd.alloc((size_t)D)); MMM_HIP(ctx, stratd.alloc((size_t)D)); MMM_HIP(ctx, col0d.alloc((size_t)C + 1)); MMM_HIP(ctx, counter.alloc(1));
    MMM_HIP(ctx, ged.alloc(2 * PC));
    if (u_obs) MMM_HIP(ctx, ud.alloc(PQ));
    if (rz_obs) MMM_HIP(ctx, rzd.alloc((size_t)P));
    if (maxstat && B > 0) MMM_HIP(ctx, maxd.alloc((size_t)B * C));
    MMM_HIP(ctx, hipMemcpyAsync(xd.p, xh.data(), sizeof(double) * xh.size(), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(ed.p, eh.data(), sizeof(double) * eh.size(), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(ssd.p, ssh.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(slotd.p, slot.data(), sizeof(uint16_t) * (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(stratd.p, strat.data(), sizeof(uint16_t) * (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(col0d.p, col0.data(), sizeof(int) * ((size_t)C + 1), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(ged.p, 0, sizeof(unsigned int) * 2 * PC, ctx->stream));

    RgArgs a;
    a.D = D; a.P = P; a.A = A; a.C = C; a.Q = Q; a.B = B; a.b0 = b0; a.n2 = n2; a.ident = 1; a.Re = Re; a.Pe = Pe;
    a.ntr = (R + side - 1) / side; a.ntp = (P + side - 1) / side;
    a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.x = xd.p; a.e = ed.p; a.ss = ssd.p; a.slot = slotd.p; a.strat = stratd.p; a.col0 = col0d.p;
    a.obs = obsd.p; a.u = u_obs ? ud.p : nullptr; a.rz = rz_obs ? rzd.p : nullptr; a.ge = ged.p; a.gemax = ged.p + PC;
    a.maxstat = (maxstat && B > 0) ? maxd.p : nullptr; a.counter = counter.p;
    const int rc = big ? (rows ? rg_launch<4, 4, true>(ctx, a, L, nt, nw) : rg_launch<4, 4, false>(ctx, a, L, nt, nw))
                       : (rows ? rg_launch<2, 2, true>(ctx, a, L, nt, nw) : rg_launch<2, 2, false>(ctx, a, L, nt, nw));
    if (rc != MMM_OK) return rc;

    std::vector<double> obs_h(PC), u_h(u_obs ? PQ : 0), rz_h(rz_obs ? (size_t)P : 0), max_h(a.maxstat ? (size_t)B * C : 0);
    std::vector<unsigned int> ge_h(B > 0 ? 2 * PC : 0);
    MMM_HIP(ctx, hipMemcpyAsync(obs_h.data(), obsd.p, sizeof(double) * PC, hipMemcpyDeviceToHost, ctx->stream));
    if (u_obs) MMM_HIP(ctx, hipMemcpyAsync(u_h.data(), ud.p, sizeof(double) * PQ, hipMemcpyDeviceToHost, ctx->stream));
    if (rz_obs) MMM_HIP(ctx, hipMemcpyAsync(rz_h.data(), rzd.p, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    if (B > 0) MMM_HIP(ctx, hipMemcpyAsync(ge_h.data(), ged.p, sizeof(unsigned int) * 2 * PC, hipMemcpyDeviceToHost, ctx->stream));
    if (a.maxstat) MMM_HIP(ctx, hipMemcpyAsync(max_h.data(), maxd.p, sizeof(double) * max_h.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // the caller's arrays are written only now, after everything has succeeded
    std::copy(obs_h.begin(), obs_h.end(), obs);
    if (u_obs) std::copy(u_h.begin(), u_h.end(), u_obs);
    if (rz_obs) std::copy(rz_h.begin(), rz_h.end(), rz_obs);
    if (B > 0) { std::copy(ge_h.begin(), ge_h.begin() + PC, ge); std::copy(ge_h.begin() + PC, ge_h.end(), ge_max); }
    if (a.maxstat) std::copy(max_h.begin(), max_h.end(), maxstat);
    return MMM_OK;
}
