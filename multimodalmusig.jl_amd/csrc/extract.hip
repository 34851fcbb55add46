// extract.hip -- mmm_extract_signatures: J new signatures learned beside F FIXED catalogue rows, R restarts in one launch (no counterpart in
// the reference; include/mmmusig.h has the normative definition, DESIGN.md section 4.17 the reasoning).
//
// One workgroup per restart runs ALL iterations of that restart; restarts beyond the resident blocks are handed out through a work counter.
// An iteration is a document phase and a row phase with nothing but __syncthreads between them:
//   document phase: a wave takes whole STRIPES (document d belongs to stripe d mod 16) and walks a stripe's documents in ascending order.
//     Per document the q / g loops and the transposing butterfly are those of k_refit (refit.hip), over all K rows: a row the document may
//     not use has w = 0 and adds +0.  Lane l owns the terms l, l + 64, ...: it adds a_dj r_dv into its accumulators of the J free rows --
//     registers while J <= 4 and V <= 128, the stripe's slab itself otherwise -- and the stripe's slab is written once.
//   row phase: every thread totals the 16 slabs of its (j, v) in stripe order and forms t = Q s; one wave per free row takes the 64 partial
//     sums and the butterfly of z and divides.
// The stripe count belongs to the definition, so 1, 2, 4, 8 or 16 waves give the same bits.  P (K V doubles) lives in LDS, the restart's
// w [D][K] too where it fits; n and f are densified once per call into [D][V] arrays that every block reads through L2.
#include "mmm_internal.h"
#include "dev_math.h"
#include "mixture_fit.cuh"
#include "mmm_philox.h"

namespace {

constexpr int kExMaxK = 256, kExMaxJ = 32;
constexpr int kExStripes = 16;                  // of the definition
constexpr int kExMaxWaves = 16;
// the library's choice: 16 waves (4 per SIMD, 128 VGPRs) while K <= 16 -- the document loop is a chain of LDS and L2 waits that more waves hide
// (BRCA, K = 12: 160 ms against 196 ms with 8 and 310 ms with 4) -- and 8 beyond, where the 32-wide chunk of g needs the 256 VGPRs of k_refit
constexpr int kExAutoWavesSmallK = 16, kExAutoWaves = 8, kExSmallK = 16;
constexpr size_t kExLdsBlock = 160 * 1024;      // LDS a block may take (the CU's)
constexpr int kExRegJ = 4, kExRegS = 2;         // accumulators in registers: J <= 4 rows, V <= 128 terms (8 doubles per lane)
constexpr uint32_t kExRowBit = 0x80000000u;     // second counter word of a start: every other user of these words keeps it below 2^31

struct ExArgs {
    int D, F, J, V, K, R, r0, maxiter;
    double tol;
    uint32_t k0, k1, stream;
    const double* Pfix;              // [F][V], rows normalised
    const double* q0;                // [R][J][V], rows normalised, or NULL: drawn here
    const double* f; const double* n;            // [D][V]
    const double* Nd; const double* w0;          // [D]: N_d; 1 / |A_d|, 0 for a document that enters no sum
    const uint8_t* allowed;          // [D][F] or NULL
    double* slab;                    // per block [16][J][V]
    double* wws;                     // per block [D][K] where w does not fit LDS
    double* sig; double* w; double* ll; double* ll_doc; double* unex; int32_t* iters;      // w, ll_doc, unex may be NULL
    int* counter;                    // next restart
};

// n[d][v] += count (duplicate terms summed: integer-valued doubles, exact in any order); n is zero on entry
__global__ void k_extract_count(int D, int V, const int64_t* __restrict__ doc_ptr, const int32_t* __restrict__ term, const int32_t* __restrict__ count, double* n)
{
    const int d = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (d >= D) return;
    for (int64_t e = doc_ptr[d] + lane; e < doc_ptr[d + 1]; e += 64) {
        const int cnt = count[e];
        if (cnt > 0) atomicAdd(&n[(size_t)d * V + term[e]], (double)cnt);
    }
}

__global__ void k_extract_freq(size_t DV, int V, const double* __restrict__ n, const double* __restrict__ Nd, double* __restrict__ f)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= DV) return;
    const double N = Nd[i / V];
    f[i] = N > 0.0 ? n[i] / N : 0.0;
}

// one iteration of one document: r_d. into rb, a_dj r_dv into the accumulators (old w), then w' = w g.  Returns this lane's max |w' - w|.
template <bool ACC_REG>
__device__ __forceinline__ double ex_document(const ExArgs& a, const double* __restrict__ P, const int* __restrict__ ident, double* __restrict__ rb,
                                              double* __restrict__ wd, const double* __restrict__ fd, double Nd, double (&acc)[kExRegJ][kExRegS],
                                              double* __restrict__ sl, int lane)
{
    const int V = a.V, K = a.K, F = a.F, J = a.J;
    // two of the lane's terms at a time: their sums over k are independent chains (each still in the order of k)
    for (int v = lane; v < V; v += 128) {
        const bool two = v + 64 < V;
        const int v1 = two ? v + 64 : v;
        const double f0 = fd[v], f1 = fd[v1];                    // through L2: asked for before the sums that hide the wait
        double q = 0.0, q1 = 0.0;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            const double wk = wd[k];
            q += wk * P[k * V + v];
            q1 += wk * P[k * V + v1];
        }
        rb[v] = (f0 > 0.0 && q > 0.0) ? f0 / q : 0.0;          // f_v > 0 exactly where n_v > 0
        if (two) rb[v1] = (f1 > 0.0 && q1 > 0.0) ? f1 / q1 : 0.0;
    }
    rf_wave_sync();
    if (ACC_REG) {
#pragma unroll
        for (int j = 0; j < kExRegJ; ++j) {
            if (j < J) {
                const double aj = Nd * wd[F + j];
#pragma unroll
                for (int s = 0; s < kExRegS; ++s) {
                    const int v = lane + 64 * s;
                    if (v < V) acc[j][s] += aj * rb[v];
                }
            }
        }
    } else {
        for (int j = 0; j < J; ++j) {
            const double aj = Nd * wd[F + j];
            for (int v = lane; v < V; v += 64) sl[(size_t)j * V + v] += aj * rb[v];
        }
    }
    const double md = rf_update_weights(P, ident, wd, K, rb, V, lane);
    rf_wave_sync();
    return md;
}

template <bool W_LDS, bool ACC_REG, int MAXW>
__global__ __launch_bounds__(64 * MAXW) void k_extract(const ExArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_ex[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = (int)blockDim.x, nw = nt >> 6;
    const int D = a.D, F = a.F, J = a.J, V = a.V, K = a.K, Kp = (K + 31) & ~31;
    const int JV = J * V;
    // P [K][V]; per wave r [V]; 16 wave maxima (row sums of a start) and 16 stripe sums; the identity list of rows, padded with a valid row
    // whose results are dropped; the restart; then w [D][K]
    double* P = s_ex;
    double* rb = P + (size_t)K * V + (size_t)wave * V;
    double* red = P + (size_t)K * V + (size_t)nw * V;
    int* ident = (int*)(red + 2 * kExStripes);
    int* ctl = ident + Kp;
    double* W = W_LDS ? (double*)(ctl + 2) : a.wws + (size_t)blockIdx.x * D * K;
    double* slab = a.slab + (size_t)blockIdx.x * kExStripes * JV;

    for (int i = tid; i < F * V; i += nt) P[i] = a.Pfix[i];
    for (int i = tid; i < Kp; i += nt) ident[i] = min(i, K - 1);
    for (;;) {
        __syncthreads();
        if (tid == 0) ctl[0] = atomicAdd(a.counter, 1);
        __syncthreads();
        const int r = ctl[0];
        if (r >= a.R) break;
        // ---- start: the free rows, w
        if (a.q0) {
            for (int i = tid; i < JV; i += nt) P[F * V + i] = a.q0[(size_t)r * JV + i];
        } else if (J) {
            const int V4 = (V + 3) >> 2;
            for (int i = tid; i < J * V4; i += nt) {
                const int j = i / V4, b = i - j * V4;
                uint32_t u[4];
                philox4x32_10((uint32_t)b, kExRowBit | (uint32_t)j, (uint32_t)(a.r0 + r), a.stream, a.k0, a.k1, u);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (4 * b + c < V) P[(F + j) * V + 4 * b + c] = ((double)u[c] + 1.0) * 0x1p-32;
            }
            __syncthreads();
            if (tid < J) {
                double s = 0.0;
                for (int v = 0; v < V; ++v) s += P[(F + tid) * V + v];
                red[tid] = s;
            }
            __syncthreads();
            for (int i = tid; i < JV; i += nt) P[F * V + i] = P[F * V + i] / red[i / V];
        }
        for (int i = tid; i < D * K; i += nt) {
            const int d = i / K, k = i - d * K;
            W[i] = (k >= F || !a.allowed || a.allowed[(size_t)d * F + k]) ? a.w0[d] : 0.0;
        }
        __syncthreads();

        int it = 0;
        while (it < a.maxiter) {
            ++it;
            double md = 0.0;
            // ---- document phase: whole stripes per wave
            for (int st = wave; st < kExStripes; st += nw) {
                double acc[kExRegJ][kExRegS];
#pragma unroll
                for (int j = 0; j < kExRegJ; ++j)
#pragma unroll
                    for (int s = 0; s < kExRegS; ++s) acc[j][s] = 0.0;
                double* sl = slab + (size_t)st * JV;
                if (!ACC_REG)
                    for (int j = 0; j < J; ++j)
                        for (int v = lane; v < V; v += 64) sl[(size_t)j * V + v] = 0.0;          // the lane that adds into it
                // N_d and 1 / |A_d| of the stripe's next document are asked for while this one runs
                double w0n = st < D ? a.w0[st] : 0.0, Ndn = st < D ? a.Nd[st] : 0.0;
                for (int d = st; d < D; d += kExStripes) {
                    const double w0d = w0n, Ndd = Ndn;
                    if (d + kExStripes < D) { w0n = a.w0[d + kExStripes]; Ndn = a.Nd[d + kExStripes]; }
                    if (w0d == 0.0) continue;
                    md = fmax(md, ex_document<ACC_REG>(a, P, ident, rb, W + (size_t)d * K, a.f + (size_t)d * V, Ndd, acc, sl, lane));
                }
                if (ACC_REG) {
#pragma unroll
                    for (int j = 0; j < kExRegJ; ++j)
#pragma unroll
                        for (int s = 0; s < kExRegS; ++s)
                            if (j < J && lane + 64 * s < V) sl[j * V + lane + 64 * s] = acc[j][s];
                }
            }
            __syncthreads();
            // ---- row phase: s = the 16 stripe sums in stripe order, t = Q s (kept in slab 0), z, Q'
            if (J) {
                for (int e = tid; e < JV; e += nt) {
                    double s = 0.0;
                    for (int st = 0; st < kExStripes; ++st) s += slab[(size_t)st * JV + e];
                    slab[e] = P[F * V + e] * s;
                }
                __syncthreads();
                for (int j = wave; j < J; j += nw) {
                    double p = 0.0;
                    for (int v = lane; v < V; v += 64) p += slab[j * V + v];
                    const double z = wave_sum(p);
                    for (int v = lane; v < V; v += 64) {
                        const double qo = P[(F + j) * V + v], qn = z > 0.0 ? slab[j * V + v] / z : qo;
                        md = fmax(md, fabs(qn - qo));
                        P[(F + j) * V + v] = qn;
                    }
                }
            }
            md = wave_max(md);
            if (lane == 0) red[wave] = md;
            __syncthreads();
            for (int i = 0; i < nw; ++i) md = fmax(md, red[i]);
            __syncthreads();
            if (md < a.tol) break;
        }

        // ---- finish: w / S, q recomputed, ll and u per document, ll of the restart in stripe order
        for (int st = wave; st < kExStripes; st += nw) {
            double lls = 0.0;
            for (int d = st; d < D; d += kExStripes) {
                double* wd = W + (size_t)d * K;
                const size_t od = (size_t)r * D + d;
                double lld = 0.0, ud = a.Nd[d];
                if (a.w0[d] != 0.0) {
                    double S = 0.0;
                    for (int k = 0; k < K; ++k) S += wd[k];
                    rf_wave_sync();
                    if (S > 0.0)
                        for (int k = lane; k < K; k += 64) wd[k] = wd[k] / S;
                    if (!W_LDS) __threadfence();
                    rf_wave_sync();
                    double lp = 0.0, up = 0.0;
                    for (int v = lane; v < V; v += 64) {
                        double q = 0.0;
                        for (int k = 0; k < K; ++k) q += wd[k] * P[k * V + v];
                        const double nv = a.n[(size_t)d * V + v];
                        if (nv > 0.0) { if (q > 0.0) lp += nv * log(q); else up += nv; }
                    }
                    lld = wave_sum(lp); ud = wave_sum(up);
                }
                lls += lld;
                if (a.w)
                    for (int k = lane; k < K; k += 64) a.w[od * K + k] = wd[k];
                if (lane == 0) {
                    if (a.ll_doc) a.ll_doc[od] = lld;
                    if (a.unex) a.unex[od] = ud;
                }
            }
            if (lane == 0) red[kExStripes + st] = lls;
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int st = 0; st < kExStripes; ++st) s += red[kExStripes + st];
            a.ll[r] = s;
            a.iters[r] = it;
        }
        for (int i = tid; i < JV; i += nt) a.sig[(size_t)r * JV + i] = P[F * V + i];
    }
}

// LDS bytes of a block of nw waves without w
size_t ex_lds_base(int K, int V, int nw) { return sizeof(double) * ((size_t)K * V + (size_t)nw * V + 2 * kExStripes + (((K + 31) & ~31) + 2) / 2); }

} // namespace

extern "C" int mmm_extract_signatures(mmm_ctx* ctx, int D, int F, int J, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* cat,
                                      const uint8_t* allowed, int R, int r0, uint64_t seed, uint32_t stream, const double* init, int maxiter, double tol, int waves,
                                      double* sig, double* w, double* ll, double* ll_doc, double* unexplained, int32_t* iters)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, D >= 0 && F >= 0 && J >= 0 && F + (int64_t)J >= 1 && V >= 1, "mmm_extract_signatures: D = %d (>= 0), F = %d, J = %d (>= 0, F + J >= 1), V = %d (>= 1)", D, F, J, V);
    const int64_t K64 = (int64_t)F + J;
    if (K64 > kExMaxK) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_extract_signatures: K = F + J = %lld rows (limit %d)", (long long)K64, kExMaxK);
    if (J > kExMaxJ) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_extract_signatures: J = %d new signatures (limit %d)", J, kExMaxJ);
    const int K = (int)K64;
    MMM_CHECK(ctx, R >= 0 && r0 >= 0 && (int64_t)r0 + R <= 0x7fffffffLL, "mmm_extract_signatures: R = %d, r0 = %d (>= 0, r0 + R <= 2^31 - 1)", R, r0);
    MMM_CHECK(ctx, maxiter >= 1 && tol >= 0.0, "mmm_extract_signatures: maxiter = %d (>= 1), tol = %g (>= 0)", maxiter, tol);
    MMM_CHECK(ctx, waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8 || waves == 16, "mmm_extract_signatures: waves = %d (0, 1, 2, 4, 8 or 16)", waves);
    MMM_CHECK(ctx, (F == 0 || cat) && (D == 0 || R == 0 || ((J == 0 || sig) && ll && iters)), "mmm_extract_signatures: NULL argument");
    if (int rc = mmm_check_csr(ctx, "mmm_extract_signatures", D, V, doc_ptr, term, count)) return rc;
    std::vector<double> P;           // the fixed rows normalised: mmm_refit_exposures' P
    if (int rc = mmm_normalise_rows(ctx, "mmm_extract_signatures", F, V, cat, P)) return rc;
    const size_t JV = (size_t)J * V;
    std::vector<double> Q0;
    if (init && J) {
        Q0.resize((size_t)R * JV);
        for (size_t row = 0; row < (size_t)R * J; ++row) {
            double s = 0.0;
            for (int v = 0; v < V; ++v) {
                const double x = init[row * V + v];
                MMM_CHECK(ctx, std::isfinite(x) && x >= 0.0, "mmm_extract_signatures: init entry (%zu, %zu, %d) is negative or not finite", row / J, row % J, v);
                s += x;
            }
            MMM_CHECK(ctx, s > 0.0 && std::isfinite(s), "mmm_extract_signatures: init row (%zu, %zu) sums to %g", row / J, row % J, s);
            for (int v = 0; v < V; ++v) Q0[row * V + v] = init[row * V + v] / s;
        }
    }
    // launch geometry: P and the per-wave r in LDS; as many waves as that leaves room for; w in LDS where it still fits
    int nw = waves ? waves : (K <= kExSmallK ? kExAutoWavesSmallK : kExAutoWaves);
    while (!waves && nw > 1 && ex_lds_base(K, V, nw) > kExLdsBlock) nw >>= 1;
    if (ex_lds_base(K, V, nw) > kExLdsBlock)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_extract_signatures: K = %d rows of V = %d terms and %d waves take %zu bytes of LDS (limit %zu)", K, V, nw,
                        ex_lds_base(K, V, nw), kExLdsBlock);
    if (D == 0 || R == 0) return MMM_OK;
    const size_t DK = (size_t)D * K, DV = (size_t)D * V;
    if (DK >= ((size_t)1 << 31) || DV >= ((size_t)1 << 31))
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_extract_signatures: D K = %zu, D V = %zu (limit 2^31 - 1 each)", DK, DV);
    const bool w_lds = ex_lds_base(K, V, nw) + sizeof(double) * DK <= kExLdsBlock;
    const size_t lds = ex_lds_base(K, V, nw) + (w_lds ? sizeof(double) * DK : 0);
    const bool acc_reg = J <= kExRegJ && V <= 64 * kExRegS;
    const int cus = std::max(1, ctx->num_cu);
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(kExMaxWaves / nw, (int64_t)(kExLdsBlock / lds)));
    const unsigned grid = (unsigned)std::min<int64_t>(R, (int64_t)cus * per_cu);

    // N_d and 1 / |A_d|
    std::vector<double> dn(2 * (size_t)D);
    for (int d = 0; d < D; ++d) {
        double N = 0.0;
        for (int64_t e = doc_ptr[d]; e < doc_ptr[d + 1]; ++e) N += (double)count[e];
        int na = J;
        for (int c = 0; c < F; ++c) na += allowed ? (allowed[(size_t)d * F + c] != 0) : 1;
        dn[d] = N;
        dn[(size_t)D + d] = (N > 0.0 && na > 0) ? 1.0 / (double)na : 0.0;
    }
    const size_t RD = (size_t)R * D;
    DevCsr csr; DevBuf<int32_t> itd; DevBuf<double> Pd, q0d, nf, dnd, slab, wws, outd; DevBuf<uint8_t> alw; DevBuf<int> counter;
    MMM_HIP(ctx, Pd.alloc(P.size())); MMM_HIP(ctx, nf.alloc(2 * DV));
    MMM_HIP(ctx, dnd.alloc(dn.size())); MMM_HIP(ctx, slab.alloc((size_t)grid * kExStripes * JV)); MMM_HIP(ctx, counter.alloc(1)); MMM_HIP(ctx, itd.alloc((size_t)R));
    MMM_HIP(ctx, outd.alloc((size_t)R * JV + (size_t)R + (w ? RD * K : 0) + (ll_doc ? RD : 0) + (unexplained ? RD : 0)));
    if (!Q0.empty()) MMM_HIP(ctx, q0d.alloc(Q0.size()));
    if (allowed && F) MMM_HIP(ctx, alw.alloc((size_t)D * F));
    if (!w_lds) MMM_HIP(ctx, wws.alloc((size_t)grid * DK));
    if (int rc = csr.upload(ctx, D, doc_ptr, term, count)) return rc;
    if (F) MMM_HIP(ctx, hipMemcpyAsync(Pd.p, P.data(), sizeof(double) * P.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!Q0.empty()) MMM_HIP(ctx, hipMemcpyAsync(q0d.p, Q0.data(), sizeof(double) * Q0.size(), hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(dnd.p, dn.data(), sizeof(double) * dn.size(), hipMemcpyHostToDevice, ctx->stream));
    if (allowed && F) MMM_HIP(ctx, hipMemcpyAsync(alw.p, allowed, (size_t)D * F, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(nf.p, 0, sizeof(double) * DV, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_extract_count, dim3((unsigned)((D + 3) / 4)), dim3(256), 0, ctx->stream, D, V, csr.ptr, csr.term, csr.count, nf.p);
    MMM_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_extract_freq, dim3((unsigned)((DV + 255) / 256)), dim3(256), 0, ctx->stream, DV, V, nf.p, dnd.p, nf.p + DV);
    MMM_LAUNCH_CHECK(ctx);

    ExArgs a;
    a.D = D; a.F = F; a.J = J; a.V = V; a.K = K; a.R = R; a.r0 = r0; a.maxiter = maxiter; a.tol = tol;
    a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.Pfix = Pd.p; a.q0 = Q0.empty() ? nullptr : q0d.p; a.n = nf.p; a.f = nf.p + DV; a.Nd = dnd.p; a.w0 = dnd.p + D;
    a.allowed = (allowed && F) ? alw.p : nullptr; a.slab = slab.p; a.wws = w_lds ? nullptr : wws.p;
    double* o = outd.p;
    a.sig = o; o += (size_t)R * JV;
    a.ll = o; o += R;
    a.w = w ? o : nullptr; o += w ? RD * K : 0;
    a.ll_doc = ll_doc ? o : nullptr; o += ll_doc ? RD : 0;
    a.unex = unexplained ? o : nullptr;
    a.iters = itd.p; a.counter = counter.p;
    // up to 8 waves: the register budget of k_refit (256 VGPRs); 16 waves run in 128
    auto kern = nw > 8 ? (w_lds ? (acc_reg ? k_extract<true, true, 16> : k_extract<true, false, 16>) : (acc_reg ? k_extract<false, true, 16> : k_extract<false, false, 16>))
                       : (w_lds ? (acc_reg ? k_extract<true, true, 8> : k_extract<true, false, 8>) : (acc_reg ? k_extract<false, true, 8> : k_extract<false, false, 8>));
    if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), lds, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    if (J) MMM_HIP(ctx, hipMemcpyAsync(sig, a.sig, sizeof(double) * (size_t)R * JV, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(ll, a.ll, sizeof(double) * (size_t)R, hipMemcpyDeviceToHost, ctx->stream));
    if (w) MMM_HIP(ctx, hipMemcpyAsync(w, a.w, sizeof(double) * RD * K, hipMemcpyDeviceToHost, ctx->stream));
    if (ll_doc) MMM_HIP(ctx, hipMemcpyAsync(ll_doc, a.ll_doc, sizeof(double) * RD, hipMemcpyDeviceToHost, ctx->stream));
    if (unexplained) MMM_HIP(ctx, hipMemcpyAsync(unexplained, a.unex, sizeof(double) * RD, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(iters, itd.p, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MMM_OK;
}
