// survival.hip -- mmm_survival_association: permutation tests of P features and C group covariates against a censored survival outcome over D
// samples; B permutations of the outcome rows (within strata) in one launch, with the maximum over the features of every permutation for
// adjusted p-values, and the scan over every cutpoint of a feature as one statistic (no counterpart in the reference; include/mmmusig.h has
// the normative definition, DESIGN.md section 4.20 the reasoning).
//
// The host forms the integer log-rank scores A, the doubled midranks Rx, the orders o_p, and the permutation mean E and variance V of every
// test column (P trends, Q group indicators, P (D - 1) cuts; V = 0 marks a cut that is not allowed).  Everything the device adds is an integer,
// so no order of summation matters; a statistic is formed from its integer by one lane in the written order.
// k_survival: one workgroup runs one permutation; permutations beyond the resident blocks are handed out through a work counter.
//   sort:    perm_sorted_keys (mmm_perm.h, shared with k_assoc); the scores go through the permutation straight into LDS, Api[slot_j] = A[e_j]:
//            features and groups stay with their sample, so the permutation itself is never stored.
//   group:   the score sums of the Q levels by 64-bit integer atomics in LDS; a thread per covariate adds its levels' statistics in order.
//   feature: a wave per feature.  Trend: the row of ranks (coalesced) against Api, summed in 64 bits over the lanes, reduced by shuffles.
//            Cut: Api gathered through o_p, 256 cuts at a time, four consecutive ones per lane; the lane's running sums, a wave scan of the
//            lanes' totals and the carry of the tiles before give T of every cut; the lane standardises its cuts against E and V streamed from
//            memory and keeps a running maximum (a later cut replaces it only when greater, so the lowest j stays); the lanes' maxima meet
//            by shuffles, the lower j winning on equal values.
//   reduce:  the maxima over the features by one wave, the comparisons against obs; counts go to memory with 32-bit integer atomics.
// The identity permutation (every obs, z_trend, u_group, cut_at) is a launch of one block of the same kernel with Api = A.
#include "mmm_internal.h"
#include "mmm_perm.h"

#include <cmath>

namespace {

constexpr int kSvMaxD = 4096, kSvMaxP = 256, kSvMaxQ = 256, kSvMaxStrata = 64;
constexpr int kSvAutoWaves = 4;
constexpr int kSvSeg = 4;                       // consecutive cuts of a lane in the scan
constexpr size_t kSvLdsBlock = 160 * 1024;
constexpr uint32_t kSvBits = 0xA0000000u;       // second counter word: bits 31 and 29 without bits 30 and 28 are set by no other user
constexpr double kSvScale = 16777216.0;         // 2^24

struct SvArgs {
    int D, P, C, Q, B, b0, n2, ident, cuts;
    uint32_t k0, k1, stream;
    const int* A;                    // [D] the scores
    const uint16_t* rxt;             // [P][D] doubled midranks of the features
    const uint16_t* ord;             // [P][D] o_p
    const uint16_t* col;             // [C][D] the column (first column of the covariate + code) of a sample
    const uint16_t* slot;            // [D] the samples in ascending (stratum, d)
    const uint16_t* strat;           // [D]
    const int* col0;                 // [C + 1] first column of a covariate
    const double* ev_trend;          // [2][P] E, then V
    const double* ev_group;          // [2][Q]
    const double* e_cut; const double* v_cut;    // [P][D - 1], cut j at j - 1
    double* obs_trend; double* obs_group; double* obs_cut;      // [P], [C], [P]
    long long* z_trend; long long* u_group; int* cut_at;        // [P], [Q], [P]
    unsigned int* ge_trend; unsigned int* gemax_trend; unsigned int* ge_cut; unsigned int* gemax_cut; unsigned int* ge_group;
    double* maxstat;                 // [B][2] or NULL
    int* counter;
};

struct SvLds { size_t api, gs, tt, tc, mx, ctl, total; };

// the one place that lays a block's LDS out (host and device)
__host__ __device__ inline SvLds sv_layout(int D, int P, int Q, int n2)
{
    SvLds l;
    l.api = 8 * (size_t)n2;                                  // the sort buffer comes first
    l.gs = (l.api + 4 * (size_t)D + 7) & ~(size_t)7;
    l.tt = l.gs + 8 * (size_t)Q;
    l.tc = l.tt + 8 * (size_t)P;
    l.mx = l.tc + 8 * (size_t)P;
    l.ctl = l.mx + 16;
    l.total = l.ctl + 8;
    return l;
}

__device__ __forceinline__ double sv_stat(long long T, double E, double V)
{
    if (!(V > 0.0)) return 0.0;
    const double dz = (double)T - E;
    return (dz * dz) / V;
}

__global__ __launch_bounds__(1024) void k_survival(const SvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_sv[];
    const int tid = threadIdx.x, nt = (int)blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
    const int D = a.D, P = a.P, C = a.C, Q = a.Q, n2 = a.n2;
    const SvLds L = sv_layout(D, P, Q, n2);
    unsigned long long* keys = (unsigned long long*)s_sv;
    int* Api = (int*)(s_sv + L.api);                                     // [D]
    unsigned long long* gs = (unsigned long long*)(s_sv + L.gs);         // [Q]
    double* tt = (double*)(s_sv + L.tt);                                 // [P]
    double* tc = (double*)(s_sv + L.tc);                                 // [P]
    double* mx = (double*)(s_sv + L.mx);                                 // [2]
    int* ctl = (int*)(s_sv + L.ctl);

    for (;;) {
        int b = 0;
        if (!a.ident) {
            __syncthreads();
            if (tid == 0) ctl[0] = atomicAdd(a.counter, 1);
            __syncthreads();
            b = ctl[0];
            if (b >= a.B) break;
            perm_sorted_keys(keys, tid, nt, D, n2, a.strat, kSvBits, (uint32_t)(a.b0 + b), a.stream, a.k0, a.k1);
            for (int j = tid; j < D; j += nt) Api[a.slot[j]] = a.A[(int)(keys[j] & 0xFFFull)];
        } else {
            for (int d = tid; d < D; d += nt) Api[d] = a.A[d];
        }
        for (int q = tid; q < Q; q += nt) gs[q] = 0ull;
        __syncthreads();
        // ---- group sums
        for (int e = tid; e < C * D; e += nt) atomicAdd(&gs[a.col[e]], (unsigned long long)(long long)Api[e % D]);
        // ---- a wave per feature: the trend product, then the scan over the cuts
        for (int p = wv; p < P; p += nw) {
            const uint16_t* r = a.rxt + (size_t)p * D;
            long long s = 0;
            for (int i = lane; i < D; i += 64) s += (long long)r[i] * (long long)Api[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) {
                const double t = sv_stat(s, a.ev_trend[p], a.ev_trend[P + p]);
                tt[p] = t;
                if (a.ident) { a.obs_trend[p] = t; if (a.z_trend) a.z_trend[p] = s; }
                else if (t >= a.obs_trend[p]) atomicAdd(&a.ge_trend[p], 1u);
            }
            if (!a.cuts) continue;
            const uint16_t* o = a.ord + (size_t)p * D;
            const double* Ec = a.e_cut + (size_t)p * (D - 1);
            const double* Vc = a.v_cut + (size_t)p * (D - 1);
            long long carry = 0;
            double m = -1.0;                                             // below every statistic
            int at = 0;
            for (int k0 = 0; k0 < D - 1; k0 += 64 * kSvSeg) {
                const int kb = k0 + kSvSeg * lane;                       // cut j = k + 1 takes the samples o_p(0) .. o_p(k)
                long long c[kSvSeg], run = 0;
#pragma unroll
                for (int s = 0; s < kSvSeg; ++s) {
                    if (kb + s < D - 1) run += (long long)Api[o[kb + s]];
                    c[s] = run;
                }
                long long inc = run;                                     // the lanes' segment sums, scanned over the wave
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const long long up = __shfl_up(inc, off);
                    if (lane >= off) inc += up;
                }
                const long long before = carry + inc - run;
                carry += __shfl(inc, 63);
#pragma unroll
                for (int s = 0; s < kSvSeg; ++s) {
                    const int k = kb + s;
                    if (k >= D - 1) break;
                    const double V = Vc[k];
                    if (V > 0.0) {
                        const double t = sv_stat(before + c[s], Ec[k], V);
                        if (t > m) { m = t; at = k + 1; }
                    }
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double m2 = __shfl_xor(m, off);
                const int at2 = __shfl_xor(at, off);
                if (m2 > m || (m2 == m && at2 < at)) { m = m2; at = at2; }
            }
            if (lane == 0) {
                const double t = m < 0.0 ? 0.0 : m;
                tc[p] = t;
                if (a.ident) { a.obs_cut[p] = t; a.cut_at[p] = at; }
                else if (t >= a.obs_cut[p]) atomicAdd(&a.ge_cut[p], 1u);
            }
        }
        __syncthreads();
        // ---- the statistic of a covariate: its levels in ascending order
        for (int c = tid; c < C; c += nt) {
            double t = 0.0;
            for (int q = a.col0[c]; q < a.col0[c + 1]; ++q) {
                const double V = a.ev_group[Q + q];
                if (V > 0.0) t += sv_stat((long long)gs[q], a.ev_group[q], V);
            }
            if (a.ident) a.obs_group[c] = t;
            else if (t >= a.obs_group[c]) atomicAdd(&a.ge_group[c], 1u);
        }
        if (a.ident) {
            if (a.u_group)
                for (int q = tid; q < Q; q += nt) a.u_group[q] = (long long)gs[q];
            break;
        }
        // ---- the maxima over the features
        if (wv == 0) {
            double mt = 0.0, mc = 0.0;
            for (int p = lane; p < P; p += 64) { mt = fmax(mt, tt[p]); if (a.cuts) mc = fmax(mc, tc[p]); }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { mt = fmax(mt, __shfl_xor(mt, off)); mc = fmax(mc, __shfl_xor(mc, off)); }
            if (lane == 0) {
                mx[0] = mt; mx[1] = mc;
                if (a.maxstat) { a.maxstat[2 * (size_t)b] = mt; a.maxstat[2 * (size_t)b + 1] = mc; }
            }
        }
        __syncthreads();
        for (int p = tid; p < P; p += nt) {
            if (mx[0] >= a.obs_trend[p]) atomicAdd(&a.gemax_trend[p], 1u);
            if (a.cuts && mx[1] >= a.obs_cut[p]) atomicAdd(&a.gemax_cut[p], 1u);
        }
    }
}

// what the permutation moments need of the strata: sizes, score sums, and NA_s = n_s sum A^2 - SA_s^2 as a double
struct SvStrata {
    int S = 0;
    std::vector<int> of;             // [D] the dense index of a sample's stratum, ascending in the code
    std::vector<long long> n, SA;
    std::vector<double> NA, den;     // den = (n n) (n - 1)

    // E and V of a column with the per-stratum sums F and sums of squares F2
    void moments(const long long* F, const long long* F2, double& E, double& V) const
    {
        E = 0.0; V = 0.0;
        for (int s = 0; s < S; ++s) {
            E += ((double)F[s] * (double)SA[s]) / (double)n[s];
            if (n[s] >= 2) V += ((double)(n[s] * F2[s] - F[s] * F[s]) * NA[s]) / den[s];
        }
    }
};

template <class T> hipError_t sv_upload(mmm_ctx* ctx, DevBuf<T>& d, const std::vector<T>& h)
{
    hipError_t e = d.alloc(h.size());
    if (e != hipSuccess || h.empty()) return e;
    return hipMemcpyAsync(d.p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, ctx->stream);
}

} // namespace

extern "C" int mmm_survival_association(mmm_ctx* ctx, int D, int P, const double* x, int C, const int32_t* levels, const int32_t* groups, const double* time,
                                        const uint8_t* event, const int32_t* strata, int m_lo, int B, int b0, uint64_t seed, uint32_t stream, int waves,
                                        double* obs_trend, int64_t* z_trend, double* obs_group, int64_t* u_group, double* obs_cut, int32_t* cut_at,
                                        uint32_t* ge_trend, uint32_t* gemax_trend, uint32_t* ge_cut, uint32_t* gemax_cut, uint32_t* ge_group, double* maxstat)
{
    if (!ctx) return MMM_ERR_ARG;
    // ---- every argument, before a device is asked for
    MMM_CHECK(ctx, D >= 1 && P >= 1 && C >= 0, "mmm_survival_association: D = %d, P = %d (>= 1 each), C = %d (>= 0)", D, P, C);
    if (D > kSvMaxD) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_survival_association: D = %d samples (limit %d)", D, kSvMaxD);
    if (P > kSvMaxP) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_survival_association: P = %d features (limit %d)", P, kSvMaxP);
    MMM_CHECK(ctx, x && time && event && obs_trend && (C == 0 || (levels && groups && obs_group)), "mmm_survival_association: NULL argument");
    int64_t Q64 = 0;
    for (int c = 0; c < C; ++c) {
        MMM_CHECK(ctx, levels[c] >= 1, "mmm_survival_association: levels[%d] = %d (>= 1)", c, levels[c]);
        Q64 += levels[c];
    }
    if (Q64 > kSvMaxQ) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_survival_association: Q = %lld levels (limit %d)", (long long)Q64, kSvMaxQ);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0 && (int64_t)b0 + B <= 0x7fffffffLL, "mmm_survival_association: B = %d, b0 = %d (>= 0, b0 + B <= 2^31 - 1)", B, b0);
    MMM_CHECK(ctx, waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8 || waves == 16, "mmm_survival_association: waves = %d (0, 1, 2, 4, 8 or 16)", waves);
    MMM_CHECK(ctx, m_lo >= 0 && m_lo <= std::max(1, D / 2), "mmm_survival_association: m_lo = %d (0 .. max(1, D / 2) = %d)", m_lo, std::max(1, D / 2));
    const bool cuts = m_lo >= 1;
    MMM_CHECK(ctx, !cuts || (obs_cut && cut_at), "mmm_survival_association: NULL argument");
    MMM_CHECK(ctx, B == 0 || (ge_trend && gemax_trend && (!cuts || (ge_cut && gemax_cut)) && (C == 0 || ge_group)), "mmm_survival_association: NULL argument");
    for (size_t i = 0; i < (size_t)D * P; ++i)
        MMM_CHECK(ctx, std::isfinite(x[i]), "mmm_survival_association: x entry (%zu, %zu) is not finite", i / P, i % P);
    for (int d = 0; d < D; ++d) {
        MMM_CHECK(ctx, std::isfinite(time[d]) && time[d] >= 0.0, "mmm_survival_association: time[%d] = %g is not finite or negative", d, time[d]);
        MMM_CHECK(ctx, event[d] <= 1, "mmm_survival_association: event[%d] = %d (0 or 1)", d, (int)event[d]);
        for (int c = 0; c < C; ++c) {
            const int32_t g = groups[(size_t)d * C + c];
            MMM_CHECK(ctx, g >= 0 && g < levels[c], "mmm_survival_association: groups entry (%d, %d) = %d is not a code in 0 .. %d", d, c, g, levels[c] - 1);
        }
        if (strata) MMM_CHECK(ctx, strata[d] >= 0 && strata[d] < D, "mmm_survival_association: strata[%d] = %d (0 .. D - 1)", d, strata[d]);
    }
    SvStrata st;
    st.of.assign((size_t)D, 0);
    {
        std::vector<int> dense((size_t)D, 0);                 // code -> 1 if present, then its index
        for (int d = 0; d < D; ++d) dense[strata ? strata[d] : 0] = 1;
        for (int s = 0; s < D; ++s)
            if (dense[s]) dense[s] = ++st.S;
        if (st.S > kSvMaxStrata) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_survival_association: %d distinct strata (limit %d)", st.S, kSvMaxStrata);
        for (int d = 0; d < D; ++d) st.of[d] = dense[strata ? strata[d] : 0] - 1;
    }
    MMM_HIP(ctx, hipSetDevice(ctx->device));

    // ---- the scores: per stratum, the Nelson-Aalen sum at every distinct time, ascending
    const int Q = (int)Q64, S = st.S, D1 = D - 1;
    std::vector<int> A((size_t)D), idx((size_t)D);
    std::vector<uint16_t> slot((size_t)D), strat((size_t)D);
    for (int d = 0; d < D; ++d) { idx[d] = d; strat[d] = (uint16_t)(strata ? strata[d] : 0); }
    std::stable_sort(idx.begin(), idx.end(), [&](int i, int j) { return strat[i] < strat[j]; });
    for (int d = 0; d < D; ++d) slot[d] = (uint16_t)idx[d];
    st.n.assign((size_t)S, 0); st.SA.assign((size_t)S, 0); st.NA.assign((size_t)S, 0.0); st.den.assign((size_t)S, 0.0);
    for (int lo = 0; lo < D;) {                               // idx holds the strata one after another
        const int s = st.of[idx[lo]];
        int hi = lo + 1;
        while (hi < D && st.of[idx[hi]] == s) ++hi;
        std::vector<int> mem(idx.begin() + lo, idx.begin() + hi);
        std::stable_sort(mem.begin(), mem.end(), [&](int i, int j) { return time[i] < time[j]; });
        const int ns = hi - lo;
        double H = 0.0;
        __int128 sa2 = 0;
        long long sa = 0;
        for (int u = 0; u < ns;) {
            int v = u + 1, dj = event[mem[u]];
            while (v < ns && time[mem[v]] == time[mem[u]]) dj += event[mem[v++]];
            if (dj > 0) H += (double)dj / (double)(ns - u);
            for (int k = u; k < v; ++k) {
                const double ai = (double)event[mem[k]] - H;
                const int Ai = (int)std::nearbyint(ai * kSvScale);        // ties to even
                A[mem[k]] = Ai;
                sa += Ai;
                sa2 += (__int128)Ai * Ai;
            }
            u = v;
        }
        st.n[s] = ns; st.SA[s] = sa;
        st.NA[s] = (double)((__int128)ns * sa2 - (__int128)sa * sa);     // round to nearest even
        st.den[s] = ((double)ns * (double)ns) * (double)(ns - 1);
        lo = hi;
    }

    // ---- ranks, orders, columns and the moments of every test column
    std::vector<uint16_t> rxt((size_t)P * D), ord((size_t)P * D), col((size_t)C * D);
    std::vector<int> col0((size_t)C + 1, 0);
    std::vector<double> ev_trend(2 * (size_t)P), ev_group(2 * (size_t)Q), e_cut(cuts ? (size_t)P * D1 : 0), v_cut(cuts ? (size_t)P * D1 : 0, 0.0);
    std::vector<long long> F((size_t)S), F2((size_t)S);
    for (int p = 0; p < P; ++p) {
        uint16_t* r = rxt.data() + (size_t)p * D;
        perm_ranks(x + p, (size_t)P, D, idx, r, 1);
        std::fill(F.begin(), F.end(), 0); std::fill(F2.begin(), F2.end(), 0);
        for (int d = 0; d < D; ++d) { F[st.of[d]] += r[d]; F2[st.of[d]] += (long long)r[d] * r[d]; }
        st.moments(F.data(), F2.data(), ev_trend[p], ev_trend[(size_t)P + p]);
        for (int d = 0; d < D; ++d) ord[(size_t)p * D + d] = (uint16_t)idx[d];           // perm_ranks left o_p in idx
        if (!cuts) continue;
        std::fill(F.begin(), F.end(), 0);
        for (int j = 1; j <= D1; ++j) {                       // an indicator: the sum of squares is the sum
            F[st.of[idx[j - 1]]] += 1;
            const bool allowed = x[(size_t)idx[j - 1] * P + p] < x[(size_t)idx[j] * P + p] && m_lo <= j && j <= D - m_lo;
            if (allowed) st.moments(F.data(), F.data(), e_cut[(size_t)p * D1 + j - 1], v_cut[(size_t)p * D1 + j - 1]);
        }
    }
    for (int c = 0, q0 = 0; c < C; ++c) {
        col0[c] = q0;
        for (int d = 0; d < D; ++d) col[(size_t)c * D + d] = (uint16_t)(q0 + groups[(size_t)d * C + c]);
        for (int g = 0; g < levels[c]; ++g) {
            std::fill(F.begin(), F.end(), 0);
            for (int d = 0; d < D; ++d) F[st.of[d]] += groups[(size_t)d * C + c] == g;
            st.moments(F.data(), F.data(), ev_group[(size_t)q0 + g], ev_group[(size_t)Q + q0 + g]);
        }
        q0 += levels[c];
        col0[c + 1] = q0;
    }

    int n2 = 1;
    while (n2 < D) n2 <<= 1;
    const int nw = waves ? waves : kSvAutoWaves, nt = 64 * nw;
    const SvLds L = sv_layout(D, P, Q, n2);

    DevBuf<int> Ad, col0d, counter, cutd; DevBuf<uint16_t> rxd, ordd, cold, slotd, stratd; DevBuf<double> evtd, evgd, ecd, vcd, obsd, maxd;
    DevBuf<long long> zd; DevBuf<unsigned int> ged;
    MMM_HIP(ctx, sv_upload(ctx, Ad, A)); MMM_HIP(ctx, sv_upload(ctx, col0d, col0)); MMM_HIP(ctx, sv_upload(ctx, rxd, rxt)); MMM_HIP(ctx, sv_upload(ctx, ordd, ord));
    MMM_HIP(ctx, sv_upload(ctx, cold, col)); MMM_HIP(ctx, sv_upload(ctx, slotd, slot)); MMM_HIP(ctx, sv_upload(ctx, stratd, strat));
    MMM_HIP(ctx, sv_upload(ctx, evtd, ev_trend)); MMM_HIP(ctx, sv_upload(ctx, evgd, ev_group)); MMM_HIP(ctx, sv_upload(ctx, ecd, e_cut)); MMM_HIP(ctx, sv_upload(ctx, vcd, v_cut));
    const size_t nobs = 2 * (size_t)P + C, nge = 4 * (size_t)P + C, nz = (size_t)P + Q;      // trend, cut, group
    MMM_HIP(ctx, obsd.alloc(nobs)); MMM_HIP(ctx, zd.alloc(nz)); MMM_HIP(ctx, cutd.alloc((size_t)P)); MMM_HIP(ctx, ged.alloc(nge)); MMM_HIP(ctx, counter.alloc(1));
    if (maxstat && B > 0) MMM_HIP(ctx, maxd.alloc(2 * (size_t)B));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(ged.p, 0, sizeof(unsigned int) * nge, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(obsd.p, 0, sizeof(double) * nobs, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(cutd.p, 0, sizeof(int) * (size_t)P, ctx->stream));

    SvArgs a;
    a.D = D; a.P = P; a.C = C; a.Q = Q; a.B = B; a.b0 = b0; a.n2 = n2; a.ident = 1; a.cuts = cuts ? 1 : 0;
    a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.A = Ad.p; a.rxt = rxd.p; a.ord = ordd.p; a.col = cold.p; a.slot = slotd.p; a.strat = stratd.p; a.col0 = col0d.p;
    a.ev_trend = evtd.p; a.ev_group = evgd.p; a.e_cut = ecd.p; a.v_cut = vcd.p;
    a.obs_trend = obsd.p; a.obs_cut = obsd.p + P; a.obs_group = obsd.p + 2 * (size_t)P;
    a.z_trend = zd.p; a.u_group = zd.p + P; a.cut_at = cutd.p;
    a.ge_trend = ged.p; a.gemax_trend = ged.p + P; a.ge_cut = ged.p + 2 * (size_t)P; a.gemax_cut = ged.p + 3 * (size_t)P; a.ge_group = ged.p + 4 * (size_t)P;
    a.maxstat = (maxstat && B > 0) ? maxd.p : nullptr; a.counter = counter.p;
    if (L.total > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)k_survival, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total));
    hipLaunchKernelGGL(k_survival, dim3(1), dim3(nt), L.total, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    if (B > 0) {
        const int cus = std::max(1, ctx->num_cu);
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(16 / nw, (int64_t)(kSvLdsBlock / L.total)));
        a.ident = 0;
        hipLaunchKernelGGL(k_survival, dim3((unsigned)std::min<int64_t>(B, (int64_t)cus * per_cu)), dim3(nt), L.total, ctx->stream, a);
        MMM_LAUNCH_CHECK(ctx);
    }
    std::vector<double> obs_h(nobs), max_h(a.maxstat ? 2 * (size_t)B : 0);
    std::vector<long long> z_h(nz);
    std::vector<int> cut_h((size_t)P);
    std::vector<unsigned int> ge_h(B > 0 ? nge : 0);
    MMM_HIP(ctx, hipMemcpyAsync(obs_h.data(), obsd.p, sizeof(double) * nobs, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(z_h.data(), zd.p, sizeof(long long) * nz, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(cut_h.data(), cutd.p, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    if (B > 0) MMM_HIP(ctx, hipMemcpyAsync(ge_h.data(), ged.p, sizeof(unsigned int) * nge, hipMemcpyDeviceToHost, ctx->stream));
    if (a.maxstat) MMM_HIP(ctx, hipMemcpyAsync(max_h.data(), maxd.p, sizeof(double) * max_h.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // the caller's arrays are written only now, after everything has succeeded
    std::copy(obs_h.begin(), obs_h.begin() + P, obs_trend);
    if (z_trend) std::copy(z_h.begin(), z_h.begin() + P, z_trend);
    if (C > 0) std::copy(obs_h.begin() + 2 * (size_t)P, obs_h.end(), obs_group);
    if (u_group) std::copy(z_h.begin() + P, z_h.end(), u_group);
    if (cuts) { std::copy(obs_h.begin() + P, obs_h.begin() + 2 * (size_t)P, obs_cut); std::copy(cut_h.begin(), cut_h.end(), cut_at); }
    if (B > 0) {
        const unsigned int* g = ge_h.data();
        std::copy(g, g + P, ge_trend); std::copy(g + P, g + 2 * (size_t)P, gemax_trend);
        if (cuts) { std::copy(g + 2 * (size_t)P, g + 3 * (size_t)P, ge_cut); std::copy(g + 3 * (size_t)P, g + 4 * (size_t)P, gemax_cut); }
        if (C > 0) std::copy(g + 4 * (size_t)P, g + nge, ge_group);
    }
    if (a.maxstat) std::copy(max_h.begin(), max_h.end(), maxstat);
    return MMM_OK;
}
