// cox.hip -- mmm_cox_exposures: the cross-validated concordance index (Harrell's C) of a ridge-penalised, stratified Cox regression (Breslow
// ties, no intercept) of a right-censored outcome on P features over D samples, for L penalties, with B permutations of the feature rows
// (within strata) and the maximum over the penalties of every permutation, so that the p-value covers the choice of the penalty (no
// counterpart in the reference; include/mmmusig.h has the normative definition, DESIGN.md section 4.22 the reasoning).
//
// The outcome is not permuted, so the time order, the tie groups, the chunks of the scans and the comparable pairs are the same for every
// permutation: the host forms them once.  The kernel works in POSITION space: position q holds sample ord[q], its fold, its event
// flag and the feature row x[pi(ord[q])].
//
// k_cox: one workgroup runs one work item behind a work counter.  In the permutation launch an item is a permutation (its R L cells of F fits
// each); in the identity launch an item is one (r, l) cell or one of the L all-sample fits, so the identity's fits spread over the blocks.
//   sort:    perm_sorted_keys (mmm_perm.h); pi goes to LDS as 16-bit indices by position, the permuted rows to LDS when cx_place says so.
//   a fit:   the whole block on one fit.  An iteration is five phases:
//            (a) a thread per position: eta, u;
//            (b) down-scan: a thread per (entry, chunk) sums its 16 positions of u or u z_j and leaves the partial at every group end; one
//                lane per entry turns the chunk totals into their exclusive prefix; a thread per (group, entry) forms r_G and zbar_G;
//            (c) up-scan of r_G over the same chunks from the stratum's end: a thread per chunk, one lane for the totals, then a thread per
//                position: u Hhat and the martingale residual;
//            (d) a thread per (entry, stripe): gradient and lower triangle of the Hessian, a stripe walk over the positions and a second one
//                over the groups for the zbar zbar' term, the 16 stripe sums met by shuffles in ascending stripe order;
//            (e) wave 0, lane j owning row j: Cholesky, both substitutions, the step, the stopping tests (the code shape of k_classify).
//   scores:  eta of the held-out positions under the final w; after the F folds of (r, l) the pair count U2: a thread per event sample against
//            its contiguous partner range, 64-bit integer counts, a wave butterfly, an integer LDS atomic.
//   reduce:  S_b[l], their maximum and the comparisons against s_obs by one thread per penalty; 32-bit integer atomics to memory.
// zbar_G and the chunk totals live in LDS when cx_place finds room for them, else in a workspace per resident block in device memory; the
// permuted rows go to LDS when there is room beside them.
// Division and square root are the compiler's IEEE sequences, for the reasons classify.hip gives.
#include "mmm_internal.h"
#include "dev_math.h"
#include "mmm_arith.h"
#include "mmm_perm.h"

#include <cmath>

namespace {

constexpr int kCxMaxD = 4096, kCxMaxP = 64, kCxMaxR = 64, kCxMaxL = 32, kCxMaxF = 255;
constexpr int kCxAutoWaves = 4;
constexpr int kCxAll = 255;                     // the fold code no sample has: nobody is held out
constexpr size_t kCxLdsBlock = 160 * 1024;
constexpr size_t kCxLdsRows = 64 * 1024;        // rows and zbar go to LDS while a block stays within this, so that two blocks share a CU
constexpr size_t kCxWorkspace = (size_t)256 << 20;      // the grid is capped so that the blocks' workspaces together stay within this
constexpr uint32_t kCxBits = 0xB0000000u;       // second counter word: bits 31, 29 and 28 without 30 are set by no other user

struct CxArgs {
    int D, P, R, F, L, B, b0, n2, ident, maxiter, NG, NC, nev, rows_lds, zb_lds;
    double tol;
    uint32_t k0, k1, stream;
    const double* x;                 // [D][P]
    const uint8_t* evq;              // [D] the event flag of position q
    const uint8_t* foldq;            // [R][D] the fold of position q
    const uint16_t* strat;           // [D] by sample
    const uint16_t* slotpos;         // [D] the position of slot_j
    const uint16_t* ord;             // [D] the sample of position q
    const uint16_t* gq;              // [D] the tie group that ends at position q, 0xFFFF where none does
    const uint16_t* gend;            // [NG] the last position of group g
    const uint16_t* cst;             // [NC + 1] the first position of chunk c
    const uint16_t* chk;             // [D] the chunk of position q
    const uint8_t* cfl;              // [NC] 1: the first chunk of its stratum, 2: the last
    const uint16_t* ord2;            // [D] the positions in the order of the pair count
    const uint16_t* epos;            // [nev] where event sample n stands in ord2
    const uint16_t* plo;             // [nev] its partners are ord2[plo .. phi)
    const uint16_t* phi;
    const double* lambda;            // [L]
    double* ws; size_t ws_block;     // the blocks' workspaces, in doubles per block (zb_lds == 0)
    double* scores;                  // [R][L][D] or NULL
    long long* u2_obs;               // [R][L]
    double* coef;                    // [L][P]
    int* full_iters;                 // [L][2]
    unsigned int* ge; unsigned int* gemax;      // [L]
    long long* maxstat;              // [B] or NULL
    unsigned int* events;            // [4]
    int* counter;
};

struct CxLds { size_t pq, fr, dg, u, rh, w, g, h, sl, so, ctl, z, zb, total; };

// the one place that lays a block's LDS out (host and device); the sort buffer comes first and holds the scores afterwards
__host__ __device__ inline CxLds cx_layout(int D, int P, int n2, int NG, int NC, int rows_lds, int zb_lds)
{
    CxLds l;
    l.pq = 8 * (size_t)n2;
    l.fr = l.pq + 2 * (size_t)D;
    l.dg = (l.fr + (size_t)D + 1) & ~(size_t)1;
    l.u = (l.dg + 2 * (size_t)NG + 7) & ~(size_t)7;
    l.rh = l.u + 8 * (size_t)D;
    l.w = l.rh + 8 * (size_t)D;
    l.g = l.w + 8 * (size_t)P;
    l.h = l.g + 8 * (size_t)P;
    l.sl = l.h + 8 * (size_t)(P * (P + 1) / 2);
    l.so = l.sl + 8 * (size_t)(kCxMaxL + 1);
    l.ctl = l.so + 8 * (size_t)kCxMaxL;
    l.z = l.ctl + 16;
    l.zb = l.z + (rows_lds ? 8 * (size_t)D * P : 0);
    l.total = l.zb + (zb_lds ? 8 * ((size_t)NG * (P + 1) + (size_t)NC * (P + 2)) : 0);
    return l;
}

// zbar and the chunk totals first (the scans read and write them one after another, a round trip to memory each time), then the rows
// beside them
inline void cx_place(int D, int P, int n2, int NG, int NC, int* rows_lds, int* zb_lds)
{
    *zb_lds = cx_layout(D, P, n2, NG, NC, 0, 1).total <= kCxLdsRows ? 1 : 0;
    *rows_lds = cx_layout(D, P, n2, NG, NC, 1, *zb_lds).total <= kCxLdsRows ? 1 : 0;
}

__device__ __forceinline__ double cx_eta(const double* W, const double* zr, int P)
{
    double e = 0.0;
    for (int j = 0; j < P; ++j) e = e + zr[j] * W[j];
    return e;
}

__global__ __launch_bounds__(1024) void k_cox(const CxArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_cx[];
    const int tid = threadIdx.x, nt = (int)blockDim.x, lane = tid & 63, wv = tid >> 6;
    const int D = a.D, P = a.P, R = a.R, L = a.L, n2 = a.n2, NG = a.NG, NC = a.NC, E1 = P + 1;
    const CxLds ly = cx_layout(D, P, n2, NG, NC, a.rows_lds, a.zb_lds);
    unsigned long long* keys = (unsigned long long*)s_cx;
    double* sc = (double*)s_cx;                                          // [D] the scores of (r, l) by position, once the keys are spent
    uint16_t* pq = (uint16_t*)(s_cx + ly.pq);                            // [D] pi(ord[q])
    uint8_t* fr = s_cx + ly.fr;                                          // [D] the folds of repeat r
    uint16_t* DG = (uint16_t*)(s_cx + ly.dg);                            // [NG] the training events of a group
    double* U = (double*)(s_cx + ly.u);                                  // [D] u, then u Hhat; the scores in pair order at the end of a cell
    double* RH = (double*)(s_cx + ly.rh);                                // [D] r_G at group ends, its up-scan, then the residual M
    double* W = (double*)(s_cx + ly.w);                                  // [P]
    double* G = (double*)(s_cx + ly.g);                                  // [P]
    double* Hh = (double*)(s_cx + ly.h);                                 // the lower triangle, row j at j (j + 1) / 2
    unsigned long long* Sl = (unsigned long long*)(s_cx + ly.sl);        // [L] S_b, then the pair count of the (r, l) at hand
    long long* So = (long long*)(s_cx + ly.so);                          // [L] s_obs
    int* ctl = (int*)(s_cx + ly.ctl);                                    // the work item, the fit's status, the events
    double* Z = (double*)(s_cx + ly.z);                                  // [D][P] the permuted rows by position
    double* ZB = a.zb_lds ? (double*)(s_cx + ly.zb) : a.ws + (size_t)blockIdx.x * a.ws_block;       // [NG][E1] S0 partial, zbar
    double* CT = ZB + (size_t)NG * E1;                                   // [E1 + 1][NC] chunk totals; the last row is the up-scan's
    double* UT = CT + (size_t)E1 * NC;
    const int nE = P * (P + 1) / 2, ntask = (P + nE) * 16;
    const int nwork = a.ident ? R * L + L : a.B;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);

    if (!a.ident)
        for (int l = tid; l < L; l += nt) {
            long long s = 0;
            for (int r = 0; r < R; ++r) s += a.u2_obs[(size_t)r * L + l];
            So[l] = s;
        }
    for (;;) {
        __syncthreads();
        if (tid == 0) ctl[0] = atomicAdd(a.counter, 1);
        __syncthreads();
        const int wk = ctl[0];
        if (wk >= nwork) break;
        int rlo = 0, rhi = R, llo = 0, lhi = L;
        if (a.ident) {
            // repeat R of the identity launch holds the all-sample fits
            if (wk < R * L) { rlo = wk / L; llo = wk % L; } else { rlo = R; llo = wk - R * L; }
            rhi = rlo + 1; lhi = llo + 1;
            for (int q = tid; q < D; q += nt) pq[q] = a.ord[q];
        } else {
            perm_sorted_keys(keys, tid, nt, D, n2, a.strat, kCxBits, (uint32_t)(a.b0 + wk), a.stream, a.k0, a.k1);
            for (int j = tid; j < D; j += nt) pq[a.slotpos[j]] = (uint16_t)(keys[j] & 0xFFFull);
        }
        for (int l = tid; l <= L; l += nt) Sl[l] = 0ull;
        if (tid < 2) ctl[2 + tid] = 0;
        __syncthreads();
        if (a.rows_lds) {
            for (int e = tid; e < D * P; e += nt) Z[e] = a.x[(size_t)pq[e / P] * P + e % P];
        }
        for (int r = rlo; r < rhi; ++r) {
            const bool cv = r < R;
            __syncthreads();
            for (int q = tid; q < D; q += nt) fr[q] = cv ? a.foldq[(size_t)r * D + q] : (uint8_t)0;
            for (int l = llo; l < lhi; ++l) {
                const double lam = a.lambda[l];
                for (int f = 0; f < (cv ? a.F : 1); ++f) {
                    const int ff = cv ? f : kCxAll;
                    __syncthreads();
                    for (int j = tid; j < P; j += nt) W[j] = 0.0;
                    for (int g = tid; g < NG; g += nt) {
                        int d = 0;
                        for (int q = g ? a.gend[g - 1] + 1 : 0; q <= (int)a.gend[g]; ++q) d += (a.evq[q] && fr[q] != ff) ? 1 : 0;
                        DG[g] = (uint16_t)d;
                    }
                    int it = 0, status = -1;
                    while (status < 0) {
                        ++it;
                        __syncthreads();
                        // ---- (a) the positions
                        for (int q = tid; q < D; q += nt) {
                            RH[q] = 0.0;
                            if (fr[q] == ff) { U[q] = 0.0; continue; }
                            const double* zr = a.rows_lds ? Z + (size_t)q * P : a.x + (size_t)pq[q] * P;
                            const double eta = cx_eta(W, zr, P);
                            const double ec = eta < -700.0 ? -700.0 : (eta > 700.0 ? 700.0 : eta);
                            U[q] = ar_exp(ec);
                        }
                        __syncthreads();
                        // ---- (b) down-scan: entry 0 is u (S0), entry 1 + j is u z_j (S1_j)
                        for (int t = tid; t < E1 * NC; t += nt) {
                            const int e = t % E1, c = t / E1;
                            double acc = 0.0;
                            for (int q = a.cst[c]; q < (int)a.cst[c + 1]; ++q) {
                                double v = U[q];
                                if (e) v = v * (a.rows_lds ? Z[(size_t)q * P + e - 1] : a.x[(size_t)pq[q] * P + e - 1]);
                                acc = acc + v;
                                const unsigned g = a.gq[q];
                                if (g != 0xFFFFu) ZB[(size_t)g * E1 + e] = acc;
                            }
                            CT[(size_t)e * NC + c] = acc;
                        }
                        __syncthreads();
                        for (int e = tid; e < E1; e += nt) {
                            double run = 0.0;
                            for (int c = 0; c < NC; ++c) {
                                if (a.cfl[c] & 1) run = 0.0;
                                const double t = CT[(size_t)e * NC + c];
                                CT[(size_t)e * NC + c] = run;
                                run = run + t;
                            }
                        }
                        __syncthreads();
                        for (int t = tid; t < NG * E1; t += nt) {
                            const int g = t / E1, e = t % E1, d = DG[g];
                            if (!d) continue;
                            const int qe = a.gend[g], c = a.chk[qe];
                            const double S0 = CT[c] + ZB[(size_t)g * E1];
                            if (e == 0) RH[qe] = (double)d / S0;
                            else {
                                const double S1 = CT[(size_t)e * NC + c] + ZB[(size_t)g * E1 + e];
                                ZB[(size_t)g * E1 + e] = S1 / S0;
                            }
                        }
                        __syncthreads();
                        // ---- (c) up-scan of r_G, then u Hhat and the residual
                        for (int c = tid; c < NC; c += nt) {
                            double acc = 0.0;
                            for (int q = (int)a.cst[c + 1] - 1; q >= (int)a.cst[c]; --q) { acc = acc + RH[q]; RH[q] = acc; }
                            UT[c] = acc;
                        }
                        __syncthreads();
                        if (tid == 0) {
                            double run = 0.0;
                            for (int c = NC - 1; c >= 0; --c) {
                                if (a.cfl[c] & 2) run = 0.0;
                                const double t = UT[c];
                                UT[c] = run;
                                run = run + t;
                            }
                        }
                        __syncthreads();
                        for (int q = tid; q < D; q += nt) {
                            if (fr[q] == ff) { RH[q] = 0.0; continue; }       // with u = +0.0 the position adds +-0.0 to every sum of (d)
                            const double hh = UT[a.chk[q]] + RH[q];
                            const double uh = U[q] * hh;
                            U[q] = uh;
                            RH[q] = (double)a.evq[q] - uh;
                        }
                        __syncthreads();
                        // ---- (d) gradient and Hessian: entry e < P is g_e, entry P + j (j + 1) / 2 + k is H_jk
                        for (int t0 = 0; t0 < ntask; t0 += nt) {
                            const int t = t0 + tid, e = t >> 4, s = t & 15;
                            const bool on = t < ntask;
                            int j = e, k = -1;
                            if (on && e >= P) {
                                const int idx = e - P;
                                j = (int)((__builtin_sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
                                while (j * (j + 1) / 2 > idx) --j;
                                while ((j + 1) * (j + 2) / 2 <= idx) ++j;
                                k = idx - j * (j + 1) / 2;
                            }
                            double acc = 0.0, acg = 0.0;
                            if (on) {
                                // no branch on the training set: outside it M = u Hhat = +0.0, the term is +-0.0 and the sum keeps its bits
                                if (k < 0) {
#pragma unroll 4
                                    for (int q = s; q < D; q += 16) acc = acc + RH[q] * (a.rows_lds ? Z[(size_t)q * P + j] : a.x[(size_t)pq[q] * P + j]);
                                } else {
#pragma unroll 4
                                    for (int q = s; q < D; q += 16) {
                                        const double* zr = a.rows_lds ? Z + (size_t)q * P : a.x + (size_t)pq[q] * P;
                                        acc = acc + zr[j] * (U[q] * zr[k]);
                                    }
#pragma unroll 4
                                    for (int g = s; g < NG; g += 16) {
                                        const int d = DG[g];
                                        const double t = ZB[(size_t)g * E1 + 1 + j] * ((double)d * ZB[(size_t)g * E1 + 1 + k]);
                                        acg = acg + (d ? t : 0.0);          // zbar of a group without a training event is whatever was there
                                    }
                                }
                            }
                            double tot = 0.0, tog = 0.0;
#pragma unroll
                            for (int s2 = 0; s2 < 16; ++s2) { tot = tot + __shfl(acc, (lane & ~15) + s2); tog = tog + __shfl(acg, (lane & ~15) + s2); }
                            if (on && s == 0) {
                                if (k < 0) G[j] = lam * W[j] - tot;
                                else { const double h = tot - tog; Hh[e - P] = j == k ? h + lam : h; }
                            }
                        }
                        __syncthreads();
                        // ---- (e) the Newton step
                        if (wv == 0) {
                            const bool row = lane < P;
                            double* Hr = Hh + (row ? lane * (lane + 1) / 2 : 0);
                            bool ok = true;
                            for (int m = 0; m < P; ++m) {
                                const double piv = __shfl(row && lane >= m ? Hr[m] : 0.0, m);
                                if (!(piv > 0.0) || !(piv < inf)) { ok = false; break; }
                                const double ckk = __builtin_sqrt(piv);
                                double cm = 0.0;
                                if (row && lane >= m) { cm = lane == m ? ckk : Hr[m] / ckk; Hr[m] = cm; }
                                for (int k = m + 1; k < P; ++k) {
                                    const double ckm = __shfl(cm, k);
                                    if (row && lane >= k) Hr[k] = Hr[k] - cm * ckm;
                                }
                            }
                            int st = -1;
                            if (!ok) st = 2;
                            else {
                                __builtin_amdgcn_wave_barrier();
                                double acc = row ? G[lane] : 0.0;
                                for (int k = 0; k < P; ++k) {                        // C y = g
                                    const double dk = __shfl(lane == k ? acc / Hr[k] : 0.0, k);
                                    if (lane == k) acc = dk;
                                    else if (row && lane > k) acc = acc - Hr[k] * dk;
                                }
                                for (int k = P - 1; k >= 0; --k) {                   // C' d = y: row k of C is lane k's
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
                        for (int q = tid; q < D; q += nt)
                            if (fr[q] == ff) sc[q] = cx_eta(W, a.rows_lds ? Z + (size_t)q * P : a.x + (size_t)pq[q] * P, P);
                    } else {
                        for (int j = tid; j < P; j += nt) a.coef[(size_t)l * P + j] = W[j];
                        if (tid == 0) { a.full_iters[2 * l] = it; a.full_iters[2 * l + 1] = status; }
                    }
                }
                if (!cv) continue;
                __syncthreads();
                // ---- U2 of (r, l): every event sample against its partner range, the scores gathered in pair order; a NaN compares false
                for (int k = tid; k < D; k += nt) U[k] = sc[a.ord2[k]];
                if (a.ident && a.scores)
                    for (int q = tid; q < D; q += nt) a.scores[((size_t)r * L + l) * D + a.ord[q]] = sc[q];
                __syncthreads();
                long long cnt = 0;
                for (int n = tid; n < a.nev; n += nt) {
                    const double si = U[a.epos[n]];
                    for (int k = a.plo[n]; k < (int)a.phi[n]; ++k) {
                        const double sj = U[k];
                        cnt += si > sj ? 2 : (si == sj ? 1 : 0);
                    }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
                if (lane == 0 && cnt) atomicAdd(&Sl[L], (unsigned long long)cnt);
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
            if (tid < 2 && ctl[2 + tid]) atomicAdd(&a.events[tid], (unsigned int)ctl[2 + tid]);
            continue;
        }
        long long M = 0;
        for (int l = 0; l < L; ++l) M = (long long)Sl[l] > M ? (long long)Sl[l] : M;
        for (int l = tid; l < L; l += nt) {
            if ((long long)Sl[l] >= So[l]) atomicAdd(&a.ge[l], 1u);
            if (M >= So[l]) atomicAdd(&a.gemax[l], 1u);
        }
        if (tid == 0 && a.maxstat) a.maxstat[wk] = M;
        if (tid < 2 && ctl[2 + tid]) atomicAdd(&a.events[2 + tid], (unsigned int)ctl[2 + tid]);
    }
}

template <class T> hipError_t cx_upload(mmm_ctx* ctx, DevBuf<T>& d, const T* h, size_t n)
{
    hipError_t e = d.alloc(n);
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpyAsync(d.p, h, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream);
}

template <class T> hipError_t cx_upload(mmm_ctx* ctx, DevBuf<T>& d, const std::vector<T>& h) { return cx_upload(ctx, d, h.data(), h.size()); }

} // namespace

extern "C" int mmm_cox_exposures(mmm_ctx* ctx, int D, int P, const double* x, const double* time, const uint8_t* event, const int32_t* strata, int R, int F,
                                 const uint8_t* fold, int L, const double* lambda, int maxiter, double tol, int B, int b0, uint64_t seed, uint32_t stream, int waves,
                                 double* scores, int64_t* u2_obs, int64_t* s_obs, int64_t* n_pairs, double* coef, int32_t* full_iters, uint32_t* ge, uint32_t* gemax,
                                 int64_t* maxstat, uint32_t* events)
{
    if (!ctx) return MMM_ERR_ARG;
    // ---- every argument, before a device is asked for
    MMM_CHECK(ctx, D >= 2 && P >= 1 && R >= 1 && F >= 2 && L >= 1, "mmm_cox_exposures: D = %d (>= 2), P = %d, R = %d, L = %d (>= 1 each), F = %d (>= 2)", D, P, R, L, F);
    if (D > kCxMaxD) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cox_exposures: D = %d samples (limit %d)", D, kCxMaxD);
    if (P > kCxMaxP) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cox_exposures: P = %d features (limit %d)", P, kCxMaxP);
    if (R > kCxMaxR) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cox_exposures: R = %d repeats (limit %d)", R, kCxMaxR);
    if (F > kCxMaxF) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cox_exposures: F = %d folds (limit %d)", F, kCxMaxF);
    if (L > kCxMaxL) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_cox_exposures: L = %d penalties (limit %d)", L, kCxMaxL);
    MMM_CHECK(ctx, x && time && event && fold && lambda && s_obs && n_pairs && events, "mmm_cox_exposures: NULL argument");
    MMM_CHECK(ctx, B >= 0 && b0 >= 0 && (int64_t)b0 + B <= 0x7fffffffLL, "mmm_cox_exposures: B = %d, b0 = %d (>= 0, b0 + B <= 2^31 - 1)", B, b0);
    MMM_CHECK(ctx, B == 0 || (ge && gemax), "mmm_cox_exposures: NULL argument");
    MMM_CHECK(ctx, waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8 || waves == 16, "mmm_cox_exposures: waves = %d (0, 1, 2, 4, 8 or 16)", waves);
    MMM_CHECK(ctx, maxiter >= 1 && tol >= 0.0, "mmm_cox_exposures: maxiter = %d (>= 1), tol = %g (>= 0)", maxiter, tol);
    for (int l = 0; l < L; ++l) MMM_CHECK(ctx, lambda[l] > 0.0 && std::isfinite(lambda[l]), "mmm_cox_exposures: lambda[%d] = %g is not positive and finite", l, lambda[l]);
    for (size_t i = 0; i < (size_t)D * P; ++i)
        MMM_CHECK(ctx, std::isfinite(x[i]), "mmm_cox_exposures: x entry (%zu, %zu) is not finite", i / P, i % P);
    std::vector<uint16_t> strat((size_t)D);
    int nev = 0;
    for (int d = 0; d < D; ++d) {
        MMM_CHECK(ctx, std::isfinite(time[d]) && time[d] >= 0.0, "mmm_cox_exposures: time[%d] = %g is not finite or is negative", d, time[d]);
        MMM_CHECK(ctx, event[d] <= 1, "mmm_cox_exposures: event[%d] = %d (0 or 1)", d, (int)event[d]);
        nev += event[d];
        if (strata) MMM_CHECK(ctx, strata[d] >= 0 && strata[d] < D, "mmm_cox_exposures: strata[%d] = %d (0 .. D - 1)", d, strata[d]);
        strat[d] = (uint16_t)(strata ? strata[d] : 0);
    }
    for (int r = 0; r < R; ++r) {
        std::vector<int> held((size_t)F, 0);
        for (int d = 0; d < D; ++d) {
            const int f = fold[(size_t)r * D + d];
            MMM_CHECK(ctx, f < F, "mmm_cox_exposures: fold entry (%d, %d) = %d (0 .. F - 1 = %d)", r, d, f, F - 1);
            held[(size_t)f] += event[d];
        }
        for (int f = 0; f < F; ++f)
            MMM_CHECK(ctx, held[(size_t)f] < nev, "mmm_cox_exposures: the training set of repeat %d, fold %d holds no event", r, f);
    }
    // ---- what every permutation shares: the time order, the tie groups, the chunks, the pair order
    std::vector<int> idx((size_t)D), posof((size_t)D);
    for (int d = 0; d < D; ++d) idx[d] = d;
    std::stable_sort(idx.begin(), idx.end(), [&](int i, int j) { return strat[i] != strat[j] ? strat[i] < strat[j] : time[i] > time[j]; });
    std::vector<uint16_t> ord((size_t)D), gq((size_t)D, (uint16_t)0xFFFF), gend, cst, chk((size_t)D), slotpos((size_t)D), ord2((size_t)D), epos, plo, phi;
    std::vector<uint8_t> evq((size_t)D), cfl, foldq((size_t)R * D);
    for (int q = 0, s0 = 0; q < D; ++q) {
        const int i = idx[q];
        ord[q] = (uint16_t)i; posof[i] = q; evq[q] = event[i];
        const bool news = q == 0 || strat[i] != strat[idx[q - 1]];
        if (news) s0 = q;
        if (q && (news || time[i] != time[idx[q - 1]])) gend.push_back((uint16_t)(q - 1));
        if (news || (q - s0) % 16 == 0) {
            if (news && !cfl.empty()) cfl.back() |= 2;
            cst.push_back((uint16_t)q); cfl.push_back(news ? 1 : 0);
        }
        chk[q] = (uint16_t)(cst.size() - 1);
    }
    gend.push_back((uint16_t)(D - 1)); cst.push_back((uint16_t)D); cfl.back() |= 2;
    const int NG = (int)gend.size(), NC = (int)cfl.size();
    for (int g = 0; g < NG; ++g) gq[gend[g]] = (uint16_t)g;
    for (int r = 0; r < R; ++r)
        for (int q = 0; q < D; ++q) foldq[(size_t)r * D + q] = fold[(size_t)r * D + ord[q]];
    {
        std::vector<int> sl((size_t)D);
        for (int d = 0; d < D; ++d) sl[d] = d;
        std::stable_sort(sl.begin(), sl.end(), [&](int i, int j) { return strat[i] < strat[j]; });
        for (int j = 0; j < D; ++j) slotpos[j] = (uint16_t)posof[sl[j]];
    }
    // the pair order: (stratum, time ascending, event first, index); an event sample's partners run from the end of its time's events to the
    // end of its stratum
    std::stable_sort(idx.begin(), idx.end(), [&](int i, int j) {
        if (strat[i] != strat[j]) return strat[i] < strat[j];
        if (time[i] != time[j]) return time[i] < time[j];
        return event[i] > event[j];
    });
    long long npairs = 0;
    for (int k = 0; k < D;) {
        int send = k;
        while (send < D && strat[idx[send]] == strat[idx[k]]) ++send;
        for (int t0 = k; t0 < send;) {
            int t1 = t0, e1 = t0;
            while (t1 < send && time[idx[t1]] == time[idx[t0]]) ++t1;
            while (e1 < t1 && event[idx[e1]]) ++e1;
            for (int n = t0; n < e1; ++n) { epos.push_back((uint16_t)n); plo.push_back((uint16_t)e1); phi.push_back((uint16_t)send); npairs += send - e1; }
            t0 = t1;
        }
        k = send;
    }
    for (int k = 0; k < D; ++k) ord2[k] = (uint16_t)posof[idx[k]];
    MMM_CHECK(ctx, npairs > 0, "mmm_cox_exposures: no comparable pair (%d events)", nev);
    MMM_HIP(ctx, hipSetDevice(ctx->device));

    int n2 = 1;
    while (n2 < D) n2 <<= 1;
    const int nw = waves ? waves : kCxAutoWaves, nt = 64 * nw;
    int rows_lds = 0, zb_lds = 0;
    cx_place(D, P, n2, NG, NC, &rows_lds, &zb_lds);
    const CxLds ly = cx_layout(D, P, n2, NG, NC, rows_lds, zb_lds);
    const size_t ws_block = zb_lds ? 0 : (size_t)NG * (P + 1) + (size_t)NC * (P + 2);
    const int cus = std::max(1, ctx->num_cu);
    int64_t resident = (int64_t)cus * std::max<int64_t>(1, std::min<int64_t>(16 / nw, (int64_t)(kCxLdsBlock / ly.total)));
    if (ws_block) resident = std::max<int64_t>(1, std::min<int64_t>(resident, (int64_t)(kCxWorkspace / (8 * ws_block))));
    const int64_t grid_id = std::min<int64_t>((int64_t)R * L + L, resident), grid_pm = std::min<int64_t>(B, resident);

    DevBuf<double> xd, lamd, scd, coefd, wsd; DevBuf<uint8_t> evd, foldd, cfld;
    DevBuf<uint16_t> stratd, slotd, ordd, gqd, gendd, cstd, chkd, ord2d, eposd, plod, phid; DevBuf<long long> i64d, maxd;
    DevBuf<unsigned int> u32d; DevBuf<int> itd, counter;
    MMM_HIP(ctx, cx_upload(ctx, xd, x, (size_t)D * P)); MMM_HIP(ctx, cx_upload(ctx, lamd, lambda, (size_t)L));
    MMM_HIP(ctx, cx_upload(ctx, evd, evq)); MMM_HIP(ctx, cx_upload(ctx, foldd, foldq)); MMM_HIP(ctx, cx_upload(ctx, cfld, cfl));
    MMM_HIP(ctx, cx_upload(ctx, stratd, strat)); MMM_HIP(ctx, cx_upload(ctx, slotd, slotpos)); MMM_HIP(ctx, cx_upload(ctx, ordd, ord));
    MMM_HIP(ctx, cx_upload(ctx, gqd, gq)); MMM_HIP(ctx, cx_upload(ctx, gendd, gend)); MMM_HIP(ctx, cx_upload(ctx, cstd, cst));
    MMM_HIP(ctx, cx_upload(ctx, chkd, chk)); MMM_HIP(ctx, cx_upload(ctx, ord2d, ord2)); MMM_HIP(ctx, cx_upload(ctx, eposd, epos));
    MMM_HIP(ctx, cx_upload(ctx, plod, plo)); MMM_HIP(ctx, cx_upload(ctx, phid, phi));
    const size_t nsc = (size_t)R * L * D, n64 = (size_t)R * L, nu32 = 2 * (size_t)L + 4;              // u2_obs; ge, gemax, events
    if (scores) MMM_HIP(ctx, scd.alloc(nsc));
    if (ws_block) MMM_HIP(ctx, wsd.alloc(ws_block * (size_t)std::max<int64_t>(grid_id, grid_pm)));
    MMM_HIP(ctx, coefd.alloc((size_t)L * P)); MMM_HIP(ctx, itd.alloc(2 * (size_t)L)); MMM_HIP(ctx, i64d.alloc(n64)); MMM_HIP(ctx, u32d.alloc(nu32)); MMM_HIP(ctx, counter.alloc(2));
    if (maxstat && B > 0) MMM_HIP(ctx, maxd.alloc((size_t)B));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, 2 * sizeof(int), ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(u32d.p, 0, sizeof(unsigned int) * nu32, ctx->stream));

    CxArgs a;
    a.D = D; a.P = P; a.R = R; a.F = F; a.L = L; a.B = B; a.b0 = b0; a.n2 = n2; a.ident = 1; a.maxiter = maxiter; a.NG = NG; a.NC = NC; a.nev = (int)epos.size();
    a.rows_lds = rows_lds; a.zb_lds = zb_lds; a.tol = tol;
    a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.x = xd.p; a.evq = evd.p; a.foldq = foldd.p; a.strat = stratd.p; a.slotpos = slotd.p; a.ord = ordd.p; a.gq = gqd.p; a.gend = gendd.p; a.cst = cstd.p; a.chk = chkd.p;
    a.cfl = cfld.p; a.ord2 = ord2d.p; a.epos = eposd.p; a.plo = plod.p; a.phi = phid.p; a.lambda = lamd.p; a.ws = wsd.p; a.ws_block = ws_block;
    a.scores = scores ? scd.p : nullptr; a.u2_obs = i64d.p; a.coef = coefd.p; a.full_iters = itd.p;
    a.ge = u32d.p; a.gemax = u32d.p + L; a.events = u32d.p + 2 * (size_t)L;
    a.maxstat = (maxstat && B > 0) ? maxd.p : nullptr; a.counter = counter.p;
    if (ly.total > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)k_cox, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ly.total));
    hipLaunchKernelGGL(k_cox, dim3((unsigned)grid_id), dim3(nt), ly.total, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    if (B > 0) {
        a.ident = 0; a.counter = counter.p + 1;
        hipLaunchKernelGGL(k_cox, dim3((unsigned)grid_pm), dim3(nt), ly.total, ctx->stream, a);
        MMM_LAUNCH_CHECK(ctx);
    }
    std::vector<double> sc_h(scores ? nsc : 0), coef_h((size_t)L * P);
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
    if (u2_obs) std::copy(i64_h.begin(), i64_h.end(), u2_obs);
    for (int l = 0; l < L; ++l) {
        long long s = 0;
        for (int r = 0; r < R; ++r) s += i64_h[(size_t)r * L + l];
        s_obs[l] = s;
    }
    *n_pairs = npairs;
    if (coef) std::copy(coef_h.begin(), coef_h.end(), coef);
    if (full_iters) std::copy(it_h.begin(), it_h.end(), full_iters);
    if (B > 0) { std::copy(u32_h.begin(), u32_h.begin() + L, ge); std::copy(u32_h.begin() + L, u32_h.begin() + 2 * (size_t)L, gemax); }
    if (a.maxstat) std::copy(max_h.begin(), max_h.end(), maxstat);
    std::copy(u32_h.begin() + 2 * (size_t)L, u32_h.end(), events);
    return MMM_OK;
}
