// refit.hip -- mmm_refit_exposures: exposures of every document to a FIXED catalogue of signatures, with backward elimination per document
// (no counterpart in the reference; include/mmmusig.h has the normative definition, DESIGN.md section 4.13 the reasoning).
//
// One wave per document, documents handed out through a work counter (a document with many active signatures runs up to C - 1 refits, one
// with a one-signature `allowed` row runs one: a static deal would leave the launch waiting for its slowest wave).  All rounds of a document
// run here; the host sees the final state only.  Lane l owns the terms v = l, l + 64, ...: the mixture q_v = sum_c w_c P[c][v] is a loop over
// the active signatures per lane, the 64 partial sums of g_c = sum_v r_v P[c][v] are the lanes' own, and the butterfly that combines them
// (l ^ 32, ^ 16, ..., ^ 1) is taken for up to 32 signatures at once as a TRANSPOSING reduction: at the step `off` a lane keeps half of its
// registers and hands the other half to lane l ^ off, so the same pairs are added in the same order (addition commutes: same bits) with 32
// exchanges for 32 signatures instead of 192, and lane l ends with the total of signature l >> 1.  The two widest steps are gfx950's row
// swaps (v_permlane32_swap / v_permlane16_swap: the exchange and the select in one instruction pair).  64 signatures at once would save one
// exchange in 64 and spill: 128 accumulator registers and 64 row offsets.
#include "mmm_internal.h"
#include "dev_math.h"
#include "mixture_fit.cuh"

namespace {

constexpr int kRfMaxC = 256;
constexpr int kRfMaxWaves = 8;                  // 8 waves of up to 256 VGPRs fill a CU: two per SIMD
constexpr size_t kRfLdsBlock = 160 * 1024;      // LDS a block may take (the CU's)
constexpr size_t kRfLdsP = 96 * 1024;           // the normalised catalogue is staged in LDS up to this size, read through L2 beyond

struct RfArgs {
    int D, C, V, Cp, maxiter;
    double tol;
    const int64_t* doc_ptr; const int32_t* term; const int32_t* count;
    const double* P;                 // [C][V], rows normalised
    const uint8_t* allowed;          // [D][C] or NULL
    const double* penalty;           // [D] or NULL
    double* w; uint8_t* active; int32_t* order; double* cost; double* ll; double* unex; long long* iters;      // order / cost may be NULL
    int* counter;                    // next document
    double* ws;                      // per wave 3 V doubles when they do not fit LDS
};

template <bool P_LDS, bool F_LDS>
__global__ __launch_bounds__(64 * kRfMaxWaves) void k_refit(const RfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_rf[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
    const int C = a.C, V = a.V, Cp = a.Cp;
    if (P_LDS) {
        for (int i = tid; i < C * V; i += (int)blockDim.x) s_rf[i] = a.P[i];
        __syncthreads();
    }
    const double* __restrict__ P = P_LDS ? s_rf : a.P;
    // per wave: two weight vectors and two lists of active signatures (in the order of c, padded to a multiple of 64 with a valid row whose results are dropped),
    // then n_v, f_v, r_v
    double* base = s_rf + (P_LDS ? (size_t)C * V : 0) + (size_t)wave * (3 * (size_t)Cp + (F_LDS ? 3 * (size_t)V : 0));
    double* wA = base;
    double* wB = base + Cp;
    int* actA = (int*)(base + 2 * (size_t)Cp);
    int* actB = actA + Cp;
    double* nb = F_LDS ? base + 3 * (size_t)Cp : a.ws + ((size_t)blockIdx.x * nw + wave) * 3 * (size_t)V;
    double* fb = nb + V;
    double* rb = fb + V;

    const RfCountsF64 counts{nb};
    for (;;) {
        const int d = rf_next_item(a.counter, lane);       // its contract shapes this loop: if / else, one closing fence
        if (d >= a.D) break;
        // ---- n_v (duplicate terms summed: integer-valued doubles, exact in any order), N, f_v
        for (int v = lane; v < V; v += 64) rb[v] = 0.0;
        if (F_LDS) rf_wave_sync(); else __threadfence();
        double Np = 0.0;
        for (int64_t e = a.doc_ptr[d] + lane; e < a.doc_ptr[d + 1]; e += 64) {
            const int cnt = a.count[e];
            if (cnt > 0) { atomicAdd(&rb[a.term[e]], (double)cnt); Np += (double)cnt; }
        }
        const double N = wave_sum(Np);
        if (F_LDS) rf_wave_sync(); else __threadfence();
        for (int v = lane; v < V; v += 64) {
            const double nv = rb[v];
            nb[v] = nv;
            fb[v] = N > 0.0 ? nv / N : 0.0;
        }
        // ---- A0
        int none;
        int n = rf_active_list(a.allowed ? a.allowed + (size_t)d * C : nullptr, C, -1, actA, lane, none);
        if (N == 0.0 || n == 0) {
            if (lane == 0) a.unex[d] = N;       // everything else keeps the zeros (order: -1) the host has put there
        } else {
            rf_pad_list(actA, n, lane);
            const double pen = a.penalty ? a.penalty[d] : 0.0;
            double llA = 0.0, uA = 0.0;
            long long iters = 0;
            int round = 0, drop = 0;
            bool first = true;
            // candidate = the set whose fit runs next: A0 first, then A without its smallest weight
            double* cw = wA; int* cact = actA; int cn = n;
            for (;;) {
                iters += rf_fit(P, cact, cw, cn, fb, counts, rb, V, lane, a.maxiter, a.tol);
                const RfLoglik B = rf_loglik<false>(P, cact, cw, cn, counts, fb, 0, V, lane);
                // ---- decide
                if (first) { first = false; llA = B.ll; uA = B.u; }
                else {
                    const double delta = B.u == uA ? llA - B.ll : __builtin_inf();
                    if (!(delta < pen)) break;
                    if (lane == 0) {
                        if (a.order) a.order[(size_t)d * C + round] = actA[drop];
                        if (a.cost) a.cost[(size_t)d * C + round] = delta;
                    }
                    ++round;
                    double* tw = wA; wA = wB; wB = tw;
                    int* ta = actA; actA = actB; actB = ta;
                    llA = B.ll; n = cn;
                }
                if (!a.penalty || n <= 1) break;
                // ---- the member with the smallest weight, ties to the lowest c (the list is in the order of c)
                double bv = __builtin_inf(); int bi = 0x7fffffff;
                for (int i = lane; i < n; i += 64) { const double x = wA[i]; if (x < bv) { bv = x; bi = i; } }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const double ov = __shfl_xor(bv, off, 64); const int oi = __shfl_xor(bi, off, 64);
                    if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
                }
                drop = bi;
                cn = n - 1;
                rf_list_without(actA, actB, n, drop, lane);
                rf_pad_list(actB, cn, lane);
                cw = wB; cact = actB;
            }
            for (int i = lane; i < n; i += 64) {
                a.w[(size_t)d * C + actA[i]] = wA[i];
                a.active[(size_t)d * C + actA[i]] = 1;
            }
            if (lane == 0) { a.ll[d] = llA; a.unex[d] = uA; a.iters[d] = iters; }
        }
        rf_wave_sync();
    }
}

} // namespace

extern "C" int mmm_refit_exposures(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* cat,
                                   const uint8_t* allowed, const double* penalty, int maxiter, double tol, double* w, uint8_t* active, int32_t* order, double* cost,
                                   double* ll_doc, double* unexplained, int64_t* iters)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, C >= 1 && V >= 1 && D >= 0 && cat && (D == 0 || w), "mmm_refit_exposures: NULL argument, D < 0, C < 1 or V < 1");
    if (C > kRfMaxC) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_refit_exposures: C = %d catalogue signatures (limit %d)", C, kRfMaxC);
    MMM_CHECK(ctx, maxiter >= 1 && tol >= 0.0, "mmm_refit_exposures: maxiter = %d (>= 1), tol = %g (>= 0)", maxiter, tol);
    if ((size_t)C * (size_t)V >= ((size_t)1 << 31)) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_refit_exposures: C V = %zu (limit 2^31 - 1)", (size_t)C * V);
    if (int rc = mmm_check_csr(ctx, "mmm_refit_exposures", D, V, doc_ptr, term, count)) return rc;
    std::vector<double> P;           // the catalogue with rows normalised
    if (int rc = mmm_normalise_rows(ctx, "mmm_refit_exposures", C, V, cat, P)) return rc;
    if (penalty)
        for (int d = 0; d < D; ++d) MMM_CHECK(ctx, std::isfinite(penalty[d]) && penalty[d] >= 0.0, "mmm_refit_exposures: penalty[%d] is negative or not finite", d);
    if (D == 0) return MMM_OK;
    const size_t DC = (size_t)D * C;

    // launch geometry: the catalogue in LDS when it fits, as many waves per block as the per-wave buffers leave room for
    const int Cp = (C + 63) & ~63;
    const size_t p_bytes = sizeof(double) * (size_t)C * V, small = sizeof(double) * 3 * (size_t)Cp, big = small + sizeof(double) * 3 * (size_t)V;
    bool p_lds = p_bytes <= kRfLdsP && !mmm_off(ctx->tune, MMM_OFF_REFIT_LDS), f_lds = true;
    int nw = 0;
    for (int pass = 0; pass < 2 && !nw; ++pass) {
        for (int t = kRfMaxWaves; t >= 1 && !nw; t >>= 1)
            if ((p_lds ? p_bytes : 0) + t * big <= kRfLdsBlock) nw = t;
        if (!nw) { if (p_lds) p_lds = false; else break; }
    }
    if (!nw) { f_lds = false; nw = kRfMaxWaves; }
    // few documents: fewer waves per block, so that they spread over the CUs (a wave alone on its SIMD runs its latency chain fastest)
    const int cus = std::max(1, ctx->num_cu);
    while (nw > 1 && ((int64_t)D + nw - 1) / nw < cus) nw >>= 1;
    const size_t lds = (p_lds ? p_bytes : 0) + nw * (f_lds ? big : small);
    // blocks a CU holds at once: by waves (8 of this kernel's register budget) and by the LDS a block takes
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(kRfMaxWaves / nw, (int64_t)(kRfLdsBlock / lds)));
    const int64_t want = ((int64_t)D + nw - 1) / nw, resident = (int64_t)cus * per_cu;
    const unsigned grid = (unsigned)std::min(want, resident);

    DevCsr csr; DevBuf<int32_t> ord; DevBuf<double> Pd, pend, outd, ws; DevBuf<uint8_t> alw, act; DevBuf<int> counter;
    MMM_HIP(ctx, Pd.alloc(P.size()));
    MMM_HIP(ctx, outd.alloc(DC + (cost ? DC : 0) + 2 * (size_t)D)); MMM_HIP(ctx, act.alloc(DC)); MMM_HIP(ctx, counter.alloc(1));
    if (order) MMM_HIP(ctx, ord.alloc(DC));
    if (allowed) MMM_HIP(ctx, alw.alloc(DC));
    if (penalty) MMM_HIP(ctx, pend.alloc((size_t)D));
    if (!f_lds) MMM_HIP(ctx, ws.alloc((size_t)grid * nw * 3 * (size_t)V));
    if (int rc = csr.upload(ctx, D, doc_ptr, term, count, (size_t)D)) return rc;       // the tail: iters
    int64_t* const itd = csr.dp.p + D + 1;
    MMM_HIP(ctx, hipMemcpyAsync(Pd.p, P.data(), sizeof(double) * P.size(), hipMemcpyHostToDevice, ctx->stream));
    if (allowed) MMM_HIP(ctx, hipMemcpyAsync(alw.p, allowed, DC, hipMemcpyHostToDevice, ctx->stream));
    if (penalty) MMM_HIP(ctx, hipMemcpyAsync(pend.p, penalty, sizeof(double) * (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    // what a document that never runs (N = 0, empty `allowed` row) and a round that never runs leave behind
    MMM_HIP(ctx, hipMemsetAsync(outd.p, 0, sizeof(double) * outd.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(itd, 0, sizeof(int64_t) * (size_t)D, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(act.p, 0, DC, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));
    if (order) MMM_HIP(ctx, hipMemsetAsync(ord.p, 0xff, sizeof(int32_t) * DC, ctx->stream));

    RfArgs a;
    a.D = D; a.C = C; a.V = V; a.Cp = Cp; a.maxiter = maxiter; a.tol = tol;
    a.doc_ptr = csr.ptr; a.term = csr.term; a.count = csr.count; a.P = Pd.p; a.allowed = allowed ? alw.p : nullptr; a.penalty = penalty ? pend.p : nullptr;
    a.w = outd.p; a.cost = cost ? outd.p + DC : nullptr; a.ll = outd.p + DC + (cost ? DC : 0); a.unex = a.ll + D;
    a.active = act.p; a.order = order ? ord.p : nullptr; a.iters = (long long*)itd; a.counter = counter.p; a.ws = f_lds ? nullptr : ws.p;
    auto kern = p_lds ? k_refit<true, true> : (f_lds ? k_refit<false, true> : k_refit<false, false>);
    if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), lds, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    MMM_HIP(ctx, hipMemcpyAsync(w, a.w, sizeof(double) * DC, hipMemcpyDeviceToHost, ctx->stream));
    if (cost) MMM_HIP(ctx, hipMemcpyAsync(cost, a.cost, sizeof(double) * DC, hipMemcpyDeviceToHost, ctx->stream));
    if (ll_doc) MMM_HIP(ctx, hipMemcpyAsync(ll_doc, a.ll, sizeof(double) * (size_t)D, hipMemcpyDeviceToHost, ctx->stream));
    if (unexplained) MMM_HIP(ctx, hipMemcpyAsync(unexplained, a.unex, sizeof(double) * (size_t)D, hipMemcpyDeviceToHost, ctx->stream));
    if (active) MMM_HIP(ctx, hipMemcpyAsync(active, act.p, DC, hipMemcpyDeviceToHost, ctx->stream));
    if (order) MMM_HIP(ctx, hipMemcpyAsync(order, ord.p, sizeof(int32_t) * DC, hipMemcpyDeviceToHost, ctx->stream));
    if (iters) MMM_HIP(ctx, hipMemcpyAsync(iters, a.iters, sizeof(int64_t) * (size_t)D, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MMM_OK;
}
