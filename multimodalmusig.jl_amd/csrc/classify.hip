// classify.hip -- mmm_classify_exposures: the cross-validated AUC of a ridge-penalised logistic regression of a binary label on P features over
// D samples, for L penalties, with B permutations of the feature rows (within strata) in one launch and the maximum over the penalties of every
// permutation, so that the p-value covers the choice of the penalty (no counterpart in the reference; include/mmmusig.h has the normative
// definition, DESIGN.md section 4.21 the reasoning).
//
// k_classify: one workgroup runs one permutation; permutations beyond the resident blocks are handed out through a work counter.
//   sort:    perm_sorted_keys (mmm_perm.h, shared with k_assoc and k_survival); pi goes to LDS as 16-bit indices, and the permuted rows
//            x[pi(i)] are copied to LDS when the layout leaves room for them (cf_layout), else every read goes through pi to memory.
//   fits:    the R F L fits of the permutation run one after another, the whole block on one fit.  An iteration is three phases:
//            (a) a thread per sample: eta, p, omega, r into LDS;
//            (b) a thread per (entry, stripe): the 16 stripes of a gradient or Hessian entry are 16 neighbouring lanes, each walks its
//                stripe in ascending i, and the 16 sums meet by shuffles in ascending stripe order -- the sum's order is the definition's,
//                whatever the block size;
//            (c) wave 0, lane j owning row j: the Cholesky factor right-looking (after column m every later entry of the row loses
//                C_jm C_km, so an entry's subtractions still run in ascending m), the two substitutions column by column with the solved
//                component passed by a shuffle, the step, the stopping tests.
//   scores:  eta of the held-out samples under the final w, into LDS; after the F folds of (r, l) the pair count U2: a thread per positive
//            sample against every negative one (the negative's score is a broadcast read), 64-bit integer counts.
//   reduce:  S_b[l], their maximum and the comparisons against s_obs by one thread per penalty; 32-bit integer atomics to memory.
// The identity outputs come from a launch of one block of the same kernel with pi = the identity, which also runs the L all-sample fits
// (fold code 255 holds nobody out).  Division and square root are the compiler's IEEE sequences: the quotient's denominator reaches
// 1 + exp(700) and a pivot may be anything, both outside the range dev_div / dev_sqrt are correct on.
#include "mmm_internal.h"
#include "dev_math.h"
#include "mmm_arith.h"
#include "mmm_perm.h"

#include <cmath>

namespace {

constexpr int kCfMaxD = 4096, kCfMaxP = 63, kCfMaxR = 64, kCfMaxL = 32, kCfMaxF = 255;
constexpr int kCfAutoWaves = 4;
constexpr int kCfAll = 255;                     // the fold code no sample has: nobody is held out
constexpr size_t kCfLdsBlock = 160 * 1024;
constexpr size_t kCfLdsRows = 64 * 1024;        // the rows go to LDS while a block stays within this, so that two blocks share a CU
constexpr uint32_t kCfBits = 0x90000000u;       // second counter word: bits 31 and 28 without 30 and 29 are set by no other user

struct CfArgs {
    int D, P, Q, R, F, L, B, b0, n2, ident, maxiter, n1, n0, rows_lds;
    double tol;
    uint32_t k0, k1, stream;
    const double* x;                 // [D][P]
    const uint8_t* y;                // [D]
    const uint8_t* fold;             // [R][D]
    const uint16_t* slot;            // [D] the samples in ascending (stratum, d)
    const uint16_t* strat;           // [D]
    const uint16_t* pos;             // [n1] the samples with y = 1, ascending
    const uint16_t* neg;             // [n0]
    const double* lambda;            // [L]
    double* scores;                  // [R][L][D] or NULL
    long long* u2_obs;               // [R][L]
    long long* s_obs;                // [L]
    double* coef;                    // [L][Q]
    int* full_iters;                 // [L][2]
    unsigned int* ge; unsigned int* gemax;      // [L]
    long long* maxstat;              // [B] or NULL
    unsigned int* events;            // [4]
    int* counter;
};

struct CfLds { size_t pis, fr, om, rs, w, g, h, sl, ctl, z, total; };

// the one place that lays a block's LDS out (host and device); the sort buffer comes first and holds the scores afterwards
__host__ __device__ inline CfLds cf_layout(int D, int P, int n2, int rows_lds)
{
    const int Q = P + 1;
    CfLds l;
    l.pis = 8 * (size_t)n2;
    l.fr = l.pis + 2 * (size_t)D;
    l.om = (l.fr + (size_t)D + 7) & ~(size_t)7;
    l.rs = l.om + 8 * (size_t)D;
    l.w = l.rs + 8 * (size_t)D;
    l.g = l.w + 8 * (size_t)Q;
    l.h = l.g + 8 * (size_t)Q;
    l.sl = l.h + 8 * (size_t)(Q * (Q + 1) / 2);
    l.ctl = l.sl + 8 * (size_t)(kCfMaxL + 1);
    l.z = l.ctl + 16;
    l.total = l.z + (rows_lds ? 8 * (size_t)D * P : 0);
    return l;
}

inline bool cf_rows_in_lds(int D, int P, int n2) { return cf_layout(D, P, n2, 1).total <= kCfLdsRows; }

__device__ __forceinline__ double cf_eta(const double* W, const double* zr, int P)
{
    double e = W[0];
    for (int j = 0; j < P; ++j) e = e + zr[j] * W[j + 1];
    return e;
}

__global__ __launch_bounds__(1024) void k_classify(const CfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_cf[];
    const int tid = threadIdx.x, nt = (int)blockDim.x, lane = tid & 63, wv = tid >> 6;
    const int D = a.D, P = a.P, Q = a.Q, R = a.R, L = a.L, n2 = a.n2;
    const CfLds ly = cf_layout(D, P, n2, a.rows_lds);
    unsigned long long* keys = (unsigned long long*)s_cf;
    double* sc = (double*)s_cf;                                          // [D] the scores of (r, l), once the keys are spent
    uint16_t* pis = (uint16_t*)(s_cf + ly.pis);                          // [D] pi
    uint8_t* fr = s_cf + ly.fr;                                          // [D] the folds of repeat r
    double* om = (double*)(s_cf + ly.om);                                // [D] omega
    double* rs = (double*)(s_cf + ly.rs);                                // [D] r
    double* W = (double*)(s_cf + ly.w);                                  // [Q]
    double* G = (double*)(s_cf + ly.g);                                  // [Q]
    double* Hh = (double*)(s_cf + ly.h);                                 // the lower triangle, row j at j (j + 1) / 2
    unsigned long long* Sl = (unsigned long long*)(s_cf + ly.sl);        // [L] S_b, then the pair count of the (r, l) at hand
    int* ctl = (int*)(s_cf + ly.ctl);                                    // the permutation, the fit's status, the events
    double* Z = (double*)(s_cf + ly.z);                                  // [D][P] the permuted rows
    const int nE = Q * (Q + 1) / 2, ntask = (Q + nE) * 16;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);

    for (;;) {
        int b = 0;
        if (!a.ident) {
            __syncthreads();
            if (tid == 0) ctl[0] = atomicAdd(a.counter, 1);
            __syncthreads();
            b = ctl[0];
            if (b >= a.B) break;
            perm_sorted_keys(keys, tid, nt, D, n2, a.strat, kCfBits, (uint32_t)(a.b0 + b), a.stream, a.k0, a.k1);
            for (int j = tid; j < D; j += nt) pis[a.slot[j]] = (uint16_t)(keys[j] & 0xFFFull);
        } else {
            for (int d = tid; d < D; d += nt) pis[d] = (uint16_t)d;
        }
        for (int l = tid; l <= L; l += nt) Sl[l] = 0ull;
        if (tid < 2) ctl[2 + tid] = 0;
        __syncthreads();
        if (a.rows_lds) {
            for (int e = tid; e < D * P; e += nt) Z[e] = a.x[(size_t)pis[e / P] * P + e % P];
        }
        // repeat R of the identity launch holds the all-sample fits
        for (int r = 0; r < R + a.ident; ++r) {
            const bool cv = r < R;
            __syncthreads();
            for (int i = tid; i < D; i += nt) fr[i] = cv ? a.fold[(size_t)r * D + i] : (uint8_t)0;
            for (int l = 0; l < L; ++l) {
                const double lam = a.lambda[l];
                for (int f = 0; f < (cv ? a.F : 1); ++f) {
                    const int ff = cv ? f : kCfAll;
                    __syncthreads();
                    for (int j = tid; j < Q; j += nt) W[j] = 0.0;
                    int it = 0, status = -1;
                    while (status < 0) {
                        ++it;
                        __syncthreads();
                        // ---- (a) the samples
                        for (int i = tid; i < D; i += nt) {
                            if (fr[i] == ff) continue;
                            const double* zr = a.rows_lds ? Z + (size_t)i * P : a.x + (size_t)pis[i] * P;
                            const double eta = cf_eta(W, zr, P);
                            const double ec = eta < -700.0 ? -700.0 : (eta > 700.0 ? 700.0 : eta);
                            const double p = 1.0 / (1.0 + ar_exp(-ec));
                            om[i] = p * (1.0 - p);
                            rs[i] = p - (double)a.y[i];
                        }
                        __syncthreads();
                        // ---- (b) gradient and Hessian: entry e < Q is g_e, entry Q + j (j + 1) / 2 + k is H_jk
                        for (int t0 = 0; t0 < ntask; t0 += nt) {
                            const int t = t0 + tid, e = t >> 4, s = t & 15;
                            const bool on = t < ntask;
                            int j = e, k = -1;
                            if (on && e >= Q) {
                                const int idx = e - Q;
                                j = (int)((__builtin_sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
                                while (j * (j + 1) / 2 > idx) --j;
                                while ((j + 1) * (j + 2) / 2 <= idx) ++j;
                                k = idx - j * (j + 1) / 2;
                            }
                            double acc = 0.0;
                            if (on)
                                for (int i = s; i < D; i += 16) {
                                    if (fr[i] == ff) continue;
                                    const double* zr = a.rows_lds ? Z + (size_t)i * P : a.x + (size_t)pis[i] * P;
                                    const double zj = j ? zr[j - 1] : 1.0;
                                    if (k < 0) acc = acc + rs[i] * zj;
                                    else { const double zk = k ? zr[k - 1] : 1.0; acc = acc + zj * (om[i] * zk); }
                                }
                            double tot = 0.0;
#pragma unroll
                            for (int s2 = 0; s2 < 16; ++s2) tot = tot + __shfl(acc, (lane & ~15) + s2);
                            if (on && s == 0) {
                                const double pen = j ? lam : 0.0;
                                if (k < 0) G[j] = tot + pen * W[j];
                                else Hh[e - Q] = j == k ? tot + pen : tot;
                            }
                        }
                        __syncthreads();
                        // ---- (c) the Newton step
                        if (wv == 0) {
                            const bool row = lane < Q;
                            double* Hr = Hh + (row ? lane * (lane + 1) / 2 : 0);
                            bool ok = true;
                            for (int m = 0; m < Q; ++m) {
                                const double piv = __shfl(row && lane >= m ? Hr[m] : 0.0, m);
                                if (!(piv > 0.0) || !(piv < inf)) { ok = false; break; }
                                const double ckk = __builtin_sqrt(piv);
                                double cm = 0.0;
                                if (row && lane >= m) { cm = lane == m ? ckk : Hr[m] / ckk; Hr[m] = cm; }
                                for (int k = m + 1; k < Q; ++k) {
                                    const double ckm = __shfl(cm, k);
                                    if (row && lane >= k) Hr[k] = Hr[k] - cm * ckm;
                                }
                            }
                            int st = -1;
                            if (!ok) st = 2;
                            else {
                                __builtin_amdgcn_wave_barrier();
                                double acc = row ? G[lane] : 0.0;
                                for (int k = 0; k < Q; ++k) {                        // C y = g
                                    const double dk = __shfl(lane == k ? acc / Hr[k] : 0.0, k);
                                    if (lane == k) acc = dk;
                                    else if (row && lane > k) acc = acc - Hr[k] * dk;
                                }
                                for (int k = Q - 1; k >= 0; --k) {                   // C' d = y: row k of C is lane k's
                                    const double dk = __shfl(lane == k ? acc / Hr[k] : 0.0, k);
                                    if (lane == k) acc = dk;
                                    else if (lane < k) acc = acc - Hh[k * (k + 1) / 2 + lane] * dk;
                                }
                                const double wn = row ? W[lane] - acc : 0.0;
                                const bool bad = row && !(fabs(wn) < inf);
                                const bool far = row && fabs(acc) > a.tol;
                                if (row) W[lane] = wn;
                                if (__any(bad)) st = 2;
                                else if (!__any(far)) st = 0;
                                else if (it == a.maxiter) st = 1;
                            }
                            if (lane == 0) ctl[1] = st;
                        }
                        __syncthreads();
                        status = ctl[1];
                    }
                    if (tid == 0 && status > 0) ctl[1 + status] += 1;
                    if (cv) {
                        for (int i = tid; i < D; i += nt)
                            if (fr[i] == ff) sc[i] = cf_eta(W, a.rows_lds ? Z + (size_t)i * P : a.x + (size_t)pis[i] * P, P);
                    } else {
                        for (int j = tid; j < Q; j += nt) a.coef[(size_t)l * Q + j] = W[j];
                        if (tid == 0) { a.full_iters[2 * l] = it; a.full_iters[2 * l + 1] = status; }
                    }
                }
                if (!cv) continue;
                __syncthreads();
                // ---- U2 of (r, l): every positive sample against every negative one; a NaN compares false
                long long cnt = 0;
                for (int p1 = tid; p1 < a.n1; p1 += nt) {
                    const double si = sc[a.pos[p1]];
                    for (int q0 = 0; q0 < a.n0; ++q0) {
                        const double sj = sc[a.neg[q0]];
                        cnt += si > sj ? 2 : (si == sj ? 1 : 0);
                    }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
                if (lane == 0 && cnt) atomicAdd(&Sl[L], (unsigned long long)cnt);
                if (a.ident && a.scores)
                    for (int i = tid; i < D; i += nt) a.scores[((size_t)r * L + l) * D + i] = sc[i];
                __syncthreads();
                if (tid == 0) {
                    Sl[l] += Sl[L];
                    if (a.ident) a.u2_obs[(size_t)r * L + l] = (long long)Sl[L];
                    Sl[L] = 0ull;
                }
            }
        }
        __syncthreads();
        if (a.ident) {
            for (int l = tid; l < L; l += nt) a.s_obs[l] = (long long)Sl[l];
            if (tid < 2) a.events[tid] = (unsigned int)ctl[2 + tid];
            break;
        }
        long long M = 0;
        for (int l = 0; l < L; ++l) M = (long long)Sl[l] > M ? (long long)Sl[l] : M;
        for (int l = tid; l < L; l += nt) {
            if ((long long)Sl[l] >= a.s_obs[l]) atomicAdd(&a.ge[l], 1u);
            if (M >= a.s_obs[l]) atomicAdd(&a.gemax[l], 1u);
        }
        if (tid == 0 && a.maxstat) a.maxstat[b] = M;
        if (tid < 2 && ctl[2 + tid]) atomicAdd(&a.events[2 + tid], (unsigned int)ctl[2 + tid]);
    }
}

template <class T> hipError_t cf_upload(mmm_ctx* ctx, DevBuf<T>& d, const T* h, size_t n)
{
    hipError_t e = d.alloc(n);
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpyAsync(d.p, h, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream);
}

} // namespace

extern "C" int mmm_classify_exposures(mmm_ctx* ctx, int D, int P, const double* x, const uint8_t* y, const int32_t* strata, int R, int F, const uint8_t* fold,
                                      int L, const double* lambda, int maxiter, double tol, int B, int b0, uint64_t seed, uint32_t stream, int waves,
                                      double* scores, int64_t* u2_obs, int64_t* s_obs, double* coef, int32_t* full_iters, uint32_t* ge, uint32_t* gemax,
                                      int64_t* maxstat, uint32_t* events)
{
    if (!ctx) return MMM_ERR_ARG;
    // ---- every argument, before a device is asked for
    MMM_CHECK(ctx, D >= 2 && P >= 1 && R >= 1 && F >= 2 && L >= 1, "mmm_classify_exposures: D = %d (>= 2), P = %d, R = %d, L = %d (>= 1 each), F = %d (>= 2)", D, P, R, L, F);
    if (D > kCfMaxD) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_classify_exposures: D = %d samples (limit %d)", D, kCfMaxD);
    if (P > kCfMaxP) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_classify_exposures: P = %d features (limit %d)", P, kCfMaxP);
    if (R > kCfMaxR) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_classify_exposures: R = %d repeats (limit %d)", R, kCfMaxR);
    if (F > kCfMaxF) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_classify_exposures: F = %d folds (limit %d)", F, kCfMaxF);
    if (L > kCfMaxL) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_classify_exposures: L = %d penalties (limit %d)", L, kCfMaxL);
    MMM_CHECK(ctx, x && y && fold && lambda && s_obs && events, "mmm_classify_exposures: NULL argument");
    MMM_CHECK(ctx, B >= 0 && b0 >= 0 && (int64_t)b0 + B <= 0x7fffffffLL, "mmm_classify_exposures: B = %d, b0 = %d (>= 0, b0 + B <= 2^31 - 1)", B, b0);
    MMM_CHECK(ctx, B == 0 || (ge && gemax), "mmm_classify_exposures: NULL argument");
    MMM_CHECK(ctx, waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8 || waves == 16, "mmm_classify_exposures: waves = %d (0, 1, 2, 4, 8 or 16)", waves);
    MMM_CHECK(ctx, maxiter >= 1 && tol >= 0.0, "mmm_classify_exposures: maxiter = %d (>= 1), tol = %g (>= 0)", maxiter, tol);
    for (int l = 0; l < L; ++l) MMM_CHECK(ctx, lambda[l] > 0.0 && std::isfinite(lambda[l]), "mmm_classify_exposures: lambda[%d] = %g is not positive and finite", l, lambda[l]);
    for (size_t i = 0; i < (size_t)D * P; ++i)
        MMM_CHECK(ctx, std::isfinite(x[i]), "mmm_classify_exposures: x entry (%zu, %zu) is not finite", i / P, i % P);
    std::vector<uint16_t> pos, neg, slot((size_t)D), strat((size_t)D);
    for (int d = 0; d < D; ++d) {
        MMM_CHECK(ctx, y[d] <= 1, "mmm_classify_exposures: y[%d] = %d (0 or 1)", d, (int)y[d]);
        (y[d] ? pos : neg).push_back((uint16_t)d);
        if (strata) MMM_CHECK(ctx, strata[d] >= 0 && strata[d] < D, "mmm_classify_exposures: strata[%d] = %d (0 .. D - 1)", d, strata[d]);
        strat[d] = (uint16_t)(strata ? strata[d] : 0);
    }
    const int n1 = (int)pos.size(), n0 = (int)neg.size();
    MMM_CHECK(ctx, n1 >= 1 && n0 >= 1, "mmm_classify_exposures: %d samples with y = 1, %d with y = 0 (both classes are needed)", n1, n0);
    for (int r = 0; r < R; ++r) {
        std::vector<int> held(2 * (size_t)F, 0);
        for (int d = 0; d < D; ++d) {
            const int f = fold[(size_t)r * D + d];
            MMM_CHECK(ctx, f < F, "mmm_classify_exposures: fold entry (%d, %d) = %d (0 .. F - 1 = %d)", r, d, f, F - 1);
            held[2 * (size_t)f + y[d]] += 1;
        }
        for (int f = 0; f < F; ++f)
            MMM_CHECK(ctx, held[2 * (size_t)f] < n0 && held[2 * (size_t)f + 1] < n1, "mmm_classify_exposures: the training set of repeat %d, fold %d lacks a class", r, f);
    }
    MMM_HIP(ctx, hipSetDevice(ctx->device));

    {
        std::vector<int> idx((size_t)D);
        for (int d = 0; d < D; ++d) idx[d] = d;
        std::stable_sort(idx.begin(), idx.end(), [&](int i, int j) { return strat[i] < strat[j]; });
        for (int d = 0; d < D; ++d) slot[d] = (uint16_t)idx[d];
    }
    int n2 = 1;
    while (n2 < D) n2 <<= 1;
    const int Q = P + 1, nw = waves ? waves : kCfAutoWaves, nt = 64 * nw;
    const int rows_lds = cf_rows_in_lds(D, P, n2) ? 1 : 0;
    const CfLds ly = cf_layout(D, P, n2, rows_lds);

    DevBuf<double> xd, lamd, scd, coefd; DevBuf<uint8_t> yd, foldd; DevBuf<uint16_t> slotd, stratd, posd, negd; DevBuf<long long> i64d, maxd;
    DevBuf<unsigned int> u32d; DevBuf<int> itd, counter;
    MMM_HIP(ctx, cf_upload(ctx, xd, x, (size_t)D * P)); MMM_HIP(ctx, cf_upload(ctx, lamd, lambda, (size_t)L)); MMM_HIP(ctx, cf_upload(ctx, yd, y, (size_t)D));
    MMM_HIP(ctx, cf_upload(ctx, foldd, fold, (size_t)R * D)); MMM_HIP(ctx, cf_upload(ctx, slotd, slot.data(), (size_t)D)); MMM_HIP(ctx, cf_upload(ctx, stratd, strat.data(), (size_t)D));
    MMM_HIP(ctx, cf_upload(ctx, posd, pos.data(), (size_t)n1)); MMM_HIP(ctx, cf_upload(ctx, negd, neg.data(), (size_t)n0));
    const size_t nsc = (size_t)R * L * D, n64 = (size_t)R * L + L, nu32 = 2 * (size_t)L + 4;      // u2_obs, s_obs; ge, gemax, events
    if (scores) MMM_HIP(ctx, scd.alloc(nsc));
    MMM_HIP(ctx, coefd.alloc((size_t)L * Q)); MMM_HIP(ctx, itd.alloc(2 * (size_t)L)); MMM_HIP(ctx, i64d.alloc(n64)); MMM_HIP(ctx, u32d.alloc(nu32)); MMM_HIP(ctx, counter.alloc(1));
    if (maxstat && B > 0) MMM_HIP(ctx, maxd.alloc((size_t)B));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(u32d.p, 0, sizeof(unsigned int) * nu32, ctx->stream));

    CfArgs a;
    a.D = D; a.P = P; a.Q = Q; a.R = R; a.F = F; a.L = L; a.B = B; a.b0 = b0; a.n2 = n2; a.ident = 1; a.maxiter = maxiter; a.n1 = n1; a.n0 = n0; a.rows_lds = rows_lds;
    a.tol = tol;
    a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.x = xd.p; a.y = yd.p; a.fold = foldd.p; a.slot = slotd.p; a.strat = stratd.p; a.pos = posd.p; a.neg = negd.p; a.lambda = lamd.p;
    a.scores = scores ? scd.p : nullptr; a.u2_obs = i64d.p; a.s_obs = i64d.p + (size_t)R * L; a.coef = coefd.p; a.full_iters = itd.p;
    a.ge = u32d.p; a.gemax = u32d.p + L; a.events = u32d.p + 2 * (size_t)L;
    a.maxstat = (maxstat && B > 0) ? maxd.p : nullptr; a.counter = counter.p;
    if (ly.total > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)k_classify, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ly.total));
    hipLaunchKernelGGL(k_classify, dim3(1), dim3(nt), ly.total, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    if (B > 0) {
        const int cus = std::max(1, ctx->num_cu);
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(16 / nw, (int64_t)(kCfLdsBlock / ly.total)));
        a.ident = 0;
        hipLaunchKernelGGL(k_classify, dim3((unsigned)std::min<int64_t>(B, (int64_t)cus * per_cu)), dim3(nt), ly.total, ctx->stream, a);
        MMM_LAUNCH_CHECK(ctx);
    }
    std::vector<double> sc_h(scores ? nsc : 0), coef_h((size_t)L * Q);
    std::vector<long long> i64_h(n64), max_h(a.maxstat ? (size_t)B : 0);
    std::vector<int> it_h(2 * (size_t)L);
    std::vector<unsigned int> u32_h(nu32);
    if (scores) MMM_HIP(ctx, hipMemcpyAsync(sc_h.data(), scd.p, sizeof(double) * nsc, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(coef_h.data(), coefd.p, sizeof(double) * coef_h.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(i64_h.data(), i64d.p, sizeof(long long) * n64, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(it_h.data(), itd.p, sizeof(int) * it_h.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(u32_h.data(), u32d.p, sizeof(unsigned int) * nu32, hipMemcpyDeviceToHost, ctx->stream));
    if (a.maxstat) MMM_HIP(ctx, hipMemcpyAsync(max_h.data(), maxd.p, sizeof(long long) * max_h.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // the caller's arrays are written only now, after everything has succeeded
    if (scores) std::copy(sc_h.begin(), sc_h.end(), scores);
    if (u2_obs) std::copy(i64_h.begin(), i64_h.begin() + (size_t)R * L, u2_obs);
    std::copy(i64_h.begin() + (size_t)R * L, i64_h.end(), s_obs);
    if (coef) std::copy(coef_h.begin(), coef_h.end(), coef);
    if (full_iters) std::copy(it_h.begin(), it_h.end(), full_iters);
    if (B > 0) { std::copy(u32_h.begin(), u32_h.begin() + L, ge); std::copy(u32_h.begin() + L, u32_h.begin() + 2 * (size_t)L, gemax); }
    if (a.maxstat) std::copy(max_h.begin(), max_h.end(), maxstat);
    std::copy(u32_h.begin() + 2 * (size_t)L, u32_h.end(), events);
    return MMM_OK;
}
