// simulate.hip -- model simulation and the parametric-bootstrap goodness of fit (no counterpart in the reference):
//   mmm_simulate_counts   B count vectors per document drawn from its own mixture props x phi (Philox4x32-10 counters, integer thresholds)
//   mmm_fit_check         cosine and chi-square of every document against its mixture, and where they fall among B such replicates
// The definitions the kernel restates are in include/mmmusig.h and DESIGN.md section 4.14.  Integer arithmetic or fixed-order double sums of
// separately rounded +, -, x, /, sqrt: the same arguments give the same bits on every run and every launch geometry.
#include "mmm_internal.h"
#include "dev_math.h"
#include "mmm_philox.h"

namespace {

constexpr int kSimWaves = 4;                 // waves per block; each takes one replicate of the block's document at a time
constexpr int kSimThreads = 64 * kSimWaves;
constexpr int kSimMaxV = 4096;               // LDS per block: pi 8 V + thresholds 4 p2(V) + kSimWaves histograms 16 V = 112 KiB at V = 4096 of 160 KiB;
                                             // a launch asks for ITS V (96 terms: 2.8 KiB)

// grid ceil(D / 4), one wave per document: S[d] = the sequential sum over v of p_v -- the S of the definition, for the host's check.  Lanes
// form p of 64 terms at a time (phi coalesced), then every lane adds the 64 values in index order.
__global__ __launch_bounds__(kSimThreads) void k_sim_total(int D, int K, int V, const double* __restrict__ props, const double* __restrict__ phi,
                                                           double* __restrict__ S)
{
    const int lane = threadIdx.x & 63, d = blockIdx.x * kSimWaves + (threadIdx.x >> 6);
    if (d >= D) return;
    const double* pr = props + (size_t)d * K;
    double cum = 0.0;
    for (int base = 0; base < V; base += 64) {
        const int v = base + lane;
        double p = 0.0;
        if (v < V)
            for (int k = 0; k < K; ++k) p += pr[k] * phi[(size_t)k * V + v];
        const int n = min(64, V - base);
        for (int j = 0; j < n; ++j) cum += __shfl(p, j, 64);
    }
    if (lane == 0) S[d] = cum;
}

// the statistics of the count vector in hist (cleared on the way) against pi: the lane is the partial sum, wave_sum the butterfly
__device__ __forceinline__ void sim_stats(int lane, int V, int* hist, const double* pi, double Nd, double pp, double& cosv, double& chiv)
{
    double num = 0.0, nn = 0.0, chi = 0.0;
    for (int v = lane; v < V; v += 64) {
        const int ni = hist[v];
        hist[v] = 0;
        const double n = (double)ni, q = pi[v];
        num += n * q;
        nn += n * n;
        double t;
        if (q > 0.0) {
            const double e = Nd * q, dd = n - e;
            t = (dd * dd) / e;
        } else {
            t = ni > 0 ? __longlong_as_double(0x7ff0000000000000ll) : 0.0;
        }
        chi += t;
    }
    num = wave_sum(num); nn = wave_sum(nn); chi = wave_sum(chi);
    cosv = (nn > 0.0 && pp > 0.0) ? num / (sqrt(nn) * sqrt(pp)) : 0.0;      // f64 sqrt: the compiler's IEEE sequence
    chiv = chi;
}

// grid (D, replicate chunks); block = kSimWaves waves.  Once per block: p (lanes over v, K multiply-adds each, phi read through L2), the
// sequential cum (one thread), pi = p / S and the threshold row in LDS.  Then one replicate per wave at a time.
// FIT = false (mmm_simulate_counts): out[(b D + d) V + v] = the draws per term of replicate b0 + b.
// FIT = true (mmm_fit_check): the observed vector is built in wave 0's histogram and goes through sim_stats like a replicate; obs[d],
// obs[D + d]: its cosine and chi-square (written by the blocks of chunk 0); cnt[d] += #{cos_rep <= cos_obs}, cnt[D + d] += #{chi_rep >=
// chi_obs} over this block's replicates (integer atomics: order-free); rep (or NULL): [2][B][D] the replicates' statistics.  The host has
// zeroed obs, cnt and rep.
// Dynamic LDS: double pi[V] | uint32 thr[P] | int hist[kSimWaves][V]; the running sums of the set-up lie where the histograms follow.
template <bool FIT>
__global__ __launch_bounds__(kSimThreads) void k_simulate(int D, int K, int V, int P, const double* __restrict__ props, const double* __restrict__ phi,
                                                          const int32_t* __restrict__ n_doc, const int64_t* __restrict__ doc_ptr,
                                                          const int32_t* __restrict__ term, const int32_t* __restrict__ count, int B, uint32_t b0,
                                                          int reps_per_block, uint32_t k0, uint32_t k1, uint32_t stream, int32_t* __restrict__ out,
                                                          double* __restrict__ obs, int32_t* __restrict__ cnt, double* __restrict__ rep)
{
    extern __shared__ __attribute__((aligned(16))) double s_sim[];
    __shared__ int s_z;
    __shared__ double s_obs[2];
    double* s_pi = s_sim;
    uint32_t* s_thr = (uint32_t*)(s_pi + V);                   // P >= 2: the histograms stay 8-byte aligned
    int* s_hist0 = (int*)(s_thr + P);
    double* s_cum = (double*)s_hist0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* s_hist = s_hist0 + (size_t)wave * V;
    const uint32_t d = blockIdx.x;
    const uint32_t N = (uint32_t)n_doc[d];
    const int bbeg = (int)blockIdx.y * reps_per_block, bend = min(B, bbeg + reps_per_block);
    if (N == 0) {                                              // nothing is drawn: all-zero rows; both statistics 0, every replicate counts
        if (FIT) {
            if (tid == 0 && bend > bbeg) { atomicAdd(&cnt[d], bend - bbeg); atomicAdd(&cnt[D + d], bend - bbeg); }
        } else {
            for (int b = bbeg; b < bend; ++b) {
                int32_t* row = out + ((size_t)b * D + d) * (size_t)V;
                for (int v = tid; v < V; v += kSimThreads) row[v] = 0;
            }
        }
        return;
    }
    const double* pr = props + (size_t)d * K;
    for (int v = tid; v < V; v += kSimThreads) {
        double p = 0.0;
        for (int k = 0; k < K; ++k) p += pr[k] * phi[(size_t)k * V + v];
        s_pi[v] = p;
    }
    const DrawSetup su = draw_thresholds(tid, kSimThreads, V, P, s_pi, s_cum, &s_z, s_thr);
    if (!su.ok) return;                                        // refused by the host
    const int z = su.z;
    for (int v = tid; v < V; v += kSimThreads) s_pi[v] = s_pi[v] / su.S;
    __syncthreads();                                           // the running sums are read; the histograms take their place
    for (int v = lane; v < V; v += 64) s_hist[v] = 0;
    double pp = 0.0, cos_obs = 0.0, chi_obs = 0.0;
    const double Nd = (double)N;
    if (FIT) {
        for (int v = lane; v < V; v += 64) pp += s_pi[v] * s_pi[v];
        pp = wave_sum(pp);
        if (wave == 0)
            for (int64_t e = doc_ptr[d] + lane; e < doc_ptr[d + 1]; e += 64) atomicAdd(&s_hist[term[e]], count[e]);
        __syncthreads();
        if (wave == 0) {
            sim_stats(lane, V, s_hist, s_pi, Nd, pp, cos_obs, chi_obs);
            if (lane == 0) {
                s_obs[0] = cos_obs; s_obs[1] = chi_obs;
                if (blockIdx.y == 0) { obs[d] = cos_obs; obs[D + d] = chi_obs; }
            }
        }
        __syncthreads();
        cos_obs = s_obs[0]; chi_obs = s_obs[1];
    }
    int le = 0, ge = 0;
    for (int bb = bbeg; bb < bend; bb += kSimWaves) {          // block-uniform trip count: the barriers below are reached by every wave
        const int b = bb + wave;
        if (b < bend) draw_row(lane, P, z, N, s_thr, s_hist, d, b0 + (uint32_t)b, stream, k0, k1);
        __syncthreads();
        if (b < bend) {
            if (FIT) {
                double c, x;
                sim_stats(lane, V, s_hist, s_pi, Nd, pp, c, x);
                le += c <= cos_obs; ge += x >= chi_obs;
                if (rep && lane == 0) { rep[(size_t)b * D + d] = c; rep[((size_t)B + b) * D + d] = x; }
            } else {
                int32_t* row = out + ((size_t)b * D + d) * (size_t)V;
                for (int v = lane; v < V; v += 64) { row[v] = s_hist[v]; s_hist[v] = 0; }
            }
        }
        __syncthreads();
    }
    if (FIT && lane == 0) {
        if (le) atomicAdd(&cnt[d], le);
        if (ge) atomicAdd(&cnt[D + d], ge);
    }
}

struct SimTables {
    DevBuf<double> props, phi;
    DevBuf<int32_t> n_doc;
    int P = 2;
    size_t lds = 0;
};

// the checks and uploads both entries share: every argument is refused before anything is written.  n_doc: [D] totals, >= 0.
int sim_prepare(mmm_ctx* ctx, const char* who, int D, int K, int V, const double* props, const double* phi, const int32_t* n_doc, int B, int b0, SimTables& t)
{
    MMM_CHECK(ctx, D >= 0 && K >= 1 && V >= 1 && phi && (D == 0 || (props && n_doc)), "%s: NULL argument, D < 0, K < 1 or V < 1", who);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0, "%s: B < 0 or b0 < 0", who);
    MMM_CHECK(ctx, (int64_t)b0 + (int64_t)B <= (int64_t)INT32_MAX, "%s: b0 + B exceeds 2^31 - 1", who);
    for (int d = 0; d < D; ++d) MMM_CHECK(ctx, n_doc[d] >= 0, "%s: document %d has the total %d", who, d, n_doc[d]);
    const size_t np = (size_t)K * (size_t)D, nf = (size_t)K * (size_t)V;
    for (size_t i = 0; i < np; ++i) MMM_CHECK(ctx, props[i] >= 0.0 && std::isfinite(props[i]), "%s: props[%zu] = %g is negative or not finite", who, i, props[i]);
    for (size_t i = 0; i < nf; ++i) MMM_CHECK(ctx, phi[i] >= 0.0 && std::isfinite(phi[i]), "%s: phi[%zu] = %g is negative or not finite", who, i, phi[i]);
    if (V > kSimMaxV) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "%s: V = %d terms; a block keeps pi, the thresholds and its histograms in LDS, which holds at most V = %d", who, V, kSimMaxV);
    if (D == 0) return MMM_OK;
    while (t.P < V) t.P <<= 1;
    t.lds = sizeof(double) * (size_t)V + sizeof(uint32_t) * (size_t)t.P + sizeof(int) * (size_t)kSimWaves * (size_t)V;
    DevBuf<double> S;
    MMM_HIP(ctx, t.props.alloc(np)); MMM_HIP(ctx, t.phi.alloc(nf)); MMM_HIP(ctx, t.n_doc.alloc((size_t)D)); MMM_HIP(ctx, S.alloc((size_t)D));
    MMM_HIP(ctx, hipMemcpyAsync(t.props.p, props, sizeof(double) * np, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(t.phi.p, phi, sizeof(double) * nf, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(t.n_doc.p, n_doc, sizeof(int32_t) * (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_sim_total, dim3((unsigned)((D + kSimWaves - 1) / kSimWaves)), dim3(kSimThreads), 0, ctx->stream, D, K, V, t.props.p, t.phi.p, S.p);
    MMM_LAUNCH_CHECK(ctx);
    std::vector<double> hS((size_t)D);
    MMM_HIP(ctx, hipMemcpyAsync(hS.data(), S.p, sizeof(double) * (size_t)D, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int d = 0; d < D; ++d)
        MMM_CHECK(ctx, n_doc[d] == 0 || (hS[d] > 0.0 && std::isfinite(hS[d])), "%s: document %d has %d mutations and a mixture that sums to %g", who, d, n_doc[d], hS[d]);
    return MMM_OK;
}

// replicates per block: one per wave, more while the launch still covers the device several times over (a block's set-up is shared by its
// replicates); the geometry cannot change a bit of the output
int sim_reps_per_block(const mmm_ctx* ctx, int D, int nb)
{
    int rpb = kSimWaves;
    while (rpb < 4 * kSimWaves && (int64_t)D * ((nb + 2 * rpb - 1) / (2 * rpb)) >= 8ll * ctx->num_cu) rpb *= 2;
    while ((nb + rpb - 1) / rpb > 65535) rpb *= 2;
    return rpb;
}

template <bool FIT>
int sim_set_lds(mmm_ctx* ctx, size_t lds)
{
    if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)k_simulate<FIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MMM_OK;
}

} // namespace

extern "C" {

int mmm_simulate_counts(mmm_ctx* ctx, int D, int K, int V, const double* props, const double* phi, const int32_t* n_doc, int B, int b0, uint64_t seed,
                        uint32_t stream, int32_t* out)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    SimTables t;
    if (int rc = sim_prepare(ctx, "mmm_simulate_counts", D, K, V, props, phi, n_doc, B, b0, t)) return rc;
    if (B == 0 || D == 0) return MMM_OK;
    MMM_CHECK(ctx, out, "mmm_simulate_counts: out == NULL");
    if (int rc = sim_set_lds<false>(ctx, t.lds)) return rc;
    // replicates go through a device buffer of at most 2^28 counts (1 GiB) at a time
    const size_t DV = (size_t)D * (size_t)V;
    const int Bc = (int)std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)1 << 28) / (int64_t)DV));
    DevBuf<int32_t> o;
    MMM_HIP(ctx, o.alloc((size_t)Bc * DV));
    for (int off = 0; off < B; off += Bc) {
        const int nb = std::min(Bc, B - off);
        const int rpb = sim_reps_per_block(ctx, D, nb);
        hipLaunchKernelGGL(k_simulate<false>, dim3((unsigned)D, (unsigned)((nb + rpb - 1) / rpb)), dim3(kSimThreads), t.lds, ctx->stream, D, K, V, t.P, t.props.p,
                           t.phi.p, t.n_doc.p, (const int64_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr, nb, (uint32_t)(b0 + off), rpb,
                           (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), stream, o.p, (double*)nullptr, (int32_t*)nullptr, (double*)nullptr);
        MMM_LAUNCH_CHECK(ctx);
        MMM_HIP(ctx, hipMemcpyAsync(out + (size_t)off * DV, o.p, sizeof(int32_t) * (size_t)nb * DV, hipMemcpyDeviceToHost, ctx->stream));
        MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MMM_OK;
}

int mmm_fit_check(mmm_ctx* ctx, int D, int K, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* props,
                  const double* phi, int B, int b0, uint64_t seed, uint32_t stream, double* cos_obs, double* chi_obs, int32_t* cos_le, int32_t* chi_ge,
                  double* cos_rep, double* chi_rep)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, V >= 1, "mmm_fit_check: V < 1");
    if (int rc = mmm_check_csr(ctx, "mmm_fit_check", D, V, doc_ptr, term, count)) return rc;
    MMM_CHECK(ctx, D == 0 || (cos_obs && chi_obs && cos_le && chi_ge), "mmm_fit_check: NULL output");
    std::vector<int32_t> n_doc((size_t)D);
    if (int rc = mmm_doc_totals(ctx, "mmm_fit_check", D, doc_ptr, count, n_doc.data())) return rc;
    SimTables t;
    if (int rc = sim_prepare(ctx, "mmm_fit_check", D, K, V, props, phi, n_doc.data(), B, b0, t)) return rc;
    if (D == 0) return MMM_OK;
    if (int rc = sim_set_lds<true>(ctx, t.lds)) return rc;
    const size_t BD = (size_t)B * (size_t)D;
    const bool want_rep = (cos_rep || chi_rep) && BD;
    DevCsr csr; DevBuf<int32_t> cnt; DevBuf<double> obs, rep;
    MMM_HIP(ctx, cnt.alloc(2 * (size_t)D)); MMM_HIP(ctx, obs.alloc(2 * (size_t)D));
    if (want_rep) MMM_HIP(ctx, rep.alloc(2 * BD));
    if (int rc = csr.upload(ctx, D, doc_ptr, term, count)) return rc;
    MMM_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * 2 * (size_t)D, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(obs.p, 0, sizeof(double) * 2 * (size_t)D, ctx->stream));
    if (want_rep) MMM_HIP(ctx, hipMemsetAsync(rep.p, 0, sizeof(double) * 2 * BD, ctx->stream));
    const int rpb = sim_reps_per_block(ctx, D, B);
    hipLaunchKernelGGL(k_simulate<true>, dim3((unsigned)D, (unsigned)std::max(1, (B + rpb - 1) / rpb)), dim3(kSimThreads), t.lds, ctx->stream, D, K, V, t.P, t.props.p,
                       t.phi.p, t.n_doc.p, csr.ptr, csr.term, csr.count, B, (uint32_t)b0, rpb, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), stream,
                       (int32_t*)nullptr, obs.p, cnt.p, want_rep ? rep.p : (double*)nullptr);
    MMM_LAUNCH_CHECK(ctx);
    // staged on the host so that a failing copy leaves the caller's arrays as they were
    std::vector<double> ho(2 * (size_t)D), hr(want_rep ? 2 * BD : 0);
    std::vector<int32_t> hc(2 * (size_t)D);
    MMM_HIP(ctx, hipMemcpyAsync(ho.data(), obs.p, sizeof(double) * 2 * (size_t)D, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hc.data(), cnt.p, sizeof(int32_t) * 2 * (size_t)D, hipMemcpyDeviceToHost, ctx->stream));
    if (want_rep) MMM_HIP(ctx, hipMemcpyAsync(hr.data(), rep.p, sizeof(double) * 2 * BD, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(cos_obs, ho.data(), sizeof(double) * (size_t)D); memcpy(chi_obs, ho.data() + D, sizeof(double) * (size_t)D);
    memcpy(cos_le, hc.data(), sizeof(int32_t) * (size_t)D); memcpy(chi_ge, hc.data() + D, sizeof(int32_t) * (size_t)D);
    if (want_rep && cos_rep) memcpy(cos_rep, hr.data(), sizeof(double) * BD);
    if (want_rep && chi_rep) memcpy(chi_rep, hr.data() + BD, sizeof(double) * BD);
    return MMM_OK;
}

} // extern "C"
