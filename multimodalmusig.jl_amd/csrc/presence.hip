// presence.hip -- mmm_presence_test: is signature t present in document d?  A likelihood-ratio statistic per (target, document) item and its
// null distribution by a parametric bootstrap, draws, both fits and the comparison in one launch (no counterpart in the reference;
// include/mmmusig.h has the normative definition, DESIGN.md section 4.15 the reasoning).
//
// Two phases on the context's stream.  "Observed": one wave per item behind a work counter, as k_refit hands out documents; it leaves the
// null weights, the score, the statistic and the status of every item.  "Replicates": grid (status-0 item, replicate chunk); a block stages
// the rows of the item's signatures in LDS (where they fit), forms the mixture of the null weights and its integer thresholds exactly as
// k_simulate does, and then every wave takes one replicate at a time: Philox draws into its own LDS histogram, f = n / N, the null fit,
// the score, the alternative fit only where the score exceeds 1, one comparison.  The replicate's counts never leave LDS.
// Lane l owns the terms v = l, l + 64, ...; fit(A) is the one refit.hip runs (mixture_fit.cuh), the thresholds and the draw are the ones
// simulate.hip runs (mmm_philox.h).
//
// mmm_presence_power asks what that test could have seen: the same observed phase, then the same replicate at every
// level of a grid of totals and spiked-in fractions.  k_power_rep stages an item's rows once and walks its levels; the null levels leave
// their statistics in a bounded buffer, k_power_select takes the critical value from them, and the other levels are compared with it
// where they are computed.
#include "mmm_internal.h"
#include "dev_math.h"
#include "mmm_philox.h"
#include "mixture_fit.cuh"

namespace {

constexpr int kPrMaxC = 256;
constexpr int kPrMaxV = 4096;                   // k_simulate's limit: the threshold row and a wave's buffers stay in LDS
constexpr int kPrMaxWaves = 8;                  // 8 waves of up to 256 VGPRs fill a CU: two per SIMD
constexpr size_t kPrLdsBlock = 160 * 1024;      // LDS a block may take (the CU's)
constexpr int kPwMaxLevels = 64;                // mmm_presence_power: fractions, and totals, of one call
constexpr size_t kPwNullBytes = 64u << 20;      // mmm_presence_power: the null statistics of one chunk of items

struct PrArgs {
    int D, C, V, Cp, T, maxiter;
    double tol;
    const int64_t* doc_ptr; const int32_t* term; const int32_t* count;      // observed phase
    const double* P;                 // [C][V], rows normalised
    const uint8_t* allowed;          // [D][C] or NULL
    const int32_t* targets;          // [T]
    double* w_null; double* stat; double* score; double* w_alt; int8_t* status; unsigned long long* iters;     // [T D] (w_null [T D][C])
    int* counter;                    // next item of the observed phase
    // replicate phase
    const int32_t* items;            // the status-0 items this launch takes
    const int32_t* n_doc;            // [D] totals
    int B, reps_per_block, P2, wave_doubles, stage_doubles;     // stage_doubles: the LDS of the staged rows (even), 0 in the observed phase
    uint32_t b0, k0, k1, stream;
    int32_t* count_ge; int32_t* count_zero;
    double* rep;                     // [B][T D] or NULL
};

// a wave's own LDS: the weights of the null and the alternative fit, the two lists of signatures (in the order of c, padded to a multiple
// of 64 with a valid row whose results are dropped), f_v, r_v and the count vector
struct PrWave {
    double* w0; double* w1; int* act1; int* act0; double* fb; double* rb; uint32_t* hist;
};

__host__ __device__ inline int pr_wave_doubles(int Cp, int V) { return (3 * Cp + 2 * V + (V + 1) / 2 + 1) & ~1; }

__device__ __forceinline__ PrWave pr_carve(double* base, int Cp, int V)
{
    PrWave w;
    w.w0 = base; w.w1 = base + Cp;
    w.act1 = (int*)(base + 2 * (size_t)Cp); w.act0 = w.act1 + Cp;
    w.fb = base + 3 * (size_t)Cp; w.rb = w.fb + V;
    w.hist = (uint32_t*)(w.rb + V);
    return w;
}

// A1 = allowed_d + {t} as the list act1 (catalogue rows in the order of c) and A0 = A1 - {t} as act0, both padded.  Returns |A1|; tpos: the
// place of t in act1.
__device__ __forceinline__ int pr_lists(const PrArgs& a, int d, int t, const PrWave& w, int lane, int& tpos)
{
    const int n1 = rf_active_list(a.allowed ? a.allowed + (size_t)d * a.C : nullptr, a.C, t, w.act1, lane, tpos);
    rf_list_without(w.act1, w.act0, n1, tpos, lane);
    rf_pad_list(w.act1, n1, lane);
    if (n1 > 1) rf_pad_list(w.act0, n1 - 1, lane);
    rf_wave_sync();
    return n1;
}

// The statistic of the count vector in w.hist (total N, f_v in w.fb) for the lists w.act0 (n0 >= 1 rows) and w.act1 (n0 + 1 rows, the
// target at tpos); trow: the target's row of P.  The null fit ends with the score s = sum_v r_v P[t][v] under the normalised null weights,
// taken in the sweep that takes ll; the alternative fit runs only where the definition asks for it.  Leaves the null weights in w.w0 and
// the alternative ones in w.w1.
struct PrStat {
    double lam, s;
    bool alt;
    int iters;
};

__device__ __forceinline__ PrStat pr_statistic(const double* __restrict__ P, const PrWave& w, int n0, int trow, int V, int lane, int maxiter, double tol)
{
    const RfCountsU32 counts{w.hist};
    RfLoglik f0{}, f1{};
    PrStat r;
    r.iters = 0; r.alt = false;
    // a loop with one call site each, so that a kernel holds the fit and the sweep once (mixture_fit.cuh, rf_loglik, has the reason)
    for (int pass = 0; pass < 2; ++pass) {
        const int* act = pass ? w.act1 : w.act0;
        double* cw = pass ? w.w1 : w.w0;
        r.iters += rf_fit(P, act, cw, n0 + pass, w.fb, counts, w.rb, V, lane, maxiter, tol);
        const RfLoglik L = rf_loglik<true>(P, act, cw, n0 + pass, counts, w.fb, pass ? -1 : trow, V, lane);
        if (pass == 0) {
            f0 = L;
            if (f0.u == 0.0 && !(f0.s > 1.0)) break;        // the null optimum is the optimum over A1 (KKT): the statistic is 0 exactly
        } else {
            f1 = L; r.alt = true;
        }
    }
    r.s = f0.s;
    r.lam = !r.alt ? 0.0 : ((f0.u > 0.0 && f1.u < f0.u) ? __builtin_inf() : fmax(2.0 * (f1.ll - f0.ll), 0.0));
    return r;
}

// Observed phase.  Dynamic LDS: per wave pr_wave_doubles doubles; the catalogue is read through L2 (one fit or two per item: a B-th of the
// call's work).  The host has zeroed every output; an untestable item (N = 0 or A0 empty) gets its status and nothing else.
__global__ __launch_bounds__(64 * kPrMaxWaves) void k_presence_obs(const PrArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_pr[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, V = a.V;
    const PrWave w = pr_carve(s_pr + (size_t)wave * a.wave_doubles, a.Cp, V);
    const double* __restrict__ P = a.P;
    const int TD = a.T * a.D;
    for (;;) {
        const int j = rf_next_item(a.counter, lane);       // its contract shapes this loop: if / else, one closing fence
        if (j >= TD) break;
        const int d = j % a.D, t = a.targets[j / a.D];
        // ---- n_v (duplicate terms summed), N, f_v
        for (int v = lane; v < V; v += 64) w.hist[v] = 0u;
        rf_wave_sync();
        double Np = 0.0;
        for (int64_t e = a.doc_ptr[d] + lane; e < a.doc_ptr[d + 1]; e += 64) {
            const int cnt = a.count[e];
            if (cnt > 0) { atomicAdd(&w.hist[a.term[e]], (uint32_t)cnt); Np += (double)cnt; }
        }
        const double N = wave_sum(Np);             // integers below 2^31: exact in any order
        rf_wave_sync();
        for (int v = lane; v < V; v += 64) w.fb[v] = N > 0.0 ? (double)w.hist[v] / N : 0.0;
        int tpos;
        const int n0 = pr_lists(a, d, t, w, lane, tpos) - 1;
        if (N == 0.0 || n0 == 0) {
            if (lane == 0) a.status[j] = 3;
        } else {
            const PrStat r = pr_statistic(P, w, n0, t, V, lane, a.maxiter, a.tol);
            for (int i = lane; i < n0; i += 64) a.w_null[(size_t)j * C + w.act0[i]] = w.w0[i];
            if (lane == 0) {
                a.stat[j] = r.lam; a.score[j] = r.s;
                a.w_alt[j] = r.alt ? w.w1[tpos] : 0.0;
                a.status[j] = r.lam == 0.0 ? 1 : (r.lam == __builtin_inf() ? 2 : 0);
                a.iters[j] = (unsigned long long)r.iters;
            }
        }
        rf_wave_sync();
    }
}

// Replicate phase: grid (items, replicate chunks), blockDim 64 nw.  Dynamic LDS: int z (16 bytes) | uint32 thr[P2] | P_LDS: the rows of A1 at
// stride V | per wave pr_wave_doubles doubles.  The mixture p and its running sums are formed where wave 0's f and r follow.
template <bool P_LDS>
__global__ __launch_bounds__(64 * kPrMaxWaves) void k_presence_rep(const PrArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_pr[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6), nt = (int)blockDim.x;
    const int C = a.C, V = a.V, P2 = a.P2;
    const int j = a.items[blockIdx.x], d = j % a.D, t = a.targets[j / a.D], TD = a.T * a.D;
    int* s_z = (int*)s_pr;
    uint32_t* s_thr = (uint32_t*)(s_pr + 2);
    double* s_rows = s_pr + 2 + P2 / 2;                        // P2 >= 4: 16-byte steps
    double* wave_base = s_rows + (P_LDS ? a.stage_doubles : 0);
    // every wave builds the lists for itself (the same bits): no wave waits for another after the set-up
    const PrWave w = pr_carve(wave_base + (size_t)wave * a.wave_doubles, a.Cp, V);
    int tpos;
    const int n1 = pr_lists(a, d, t, w, lane, tpos);           // <= stage_doubles / V where the rows are staged: the host sorts the items
    const int n0 = n1 - 1;
    // the observed null weights, in the order of the list
    for (int i = lane; i < n0; i += 64) w.w0[i] = a.w_null[(size_t)j * C + w.act0[i]];
    int trow = t;
    if (P_LDS) {
        for (int i = wave; i < n1; i += nw) {
            const double* src = a.P + (size_t)w.act1[i] * V;
            for (int v = lane; v < V; v += 64) s_rows[(size_t)i * V + v] = src[v];
        }
        rf_wave_sync();
        for (int i = lane; i < ((n1 + 63) & ~63); i += 64) w.act1[i] = i < n1 ? i : 0;
        for (int i = lane; i < ((n0 + 63) & ~63); i += 64) w.act0[i] = i < n0 ? (i < tpos ? i : i + 1) : (tpos == 0 ? 1 : 0);
        trow = tpos;
    }
    const double* __restrict__ P = P_LDS ? s_rows : a.P;
    __syncthreads();                                           // the staged rows are there
    // ---- p_v = sum_c w0_c P[c][v] (the zero weights outside A0 add nothing: same bits as k_simulate's sum over all C), then its thresholds
    double* s_p = pr_carve(wave_base, a.Cp, V).fb;
    for (int v = tid; v < V; v += nt) {
        double p = 0.0;
        for (int i = 0; i < n0; ++i) p += w.w0[i] * P[w.act0[i] * V + v];
        s_p[v] = p;
    }
    const DrawSetup su = draw_thresholds(tid, nt, V, P2, s_p, s_p + V, s_z, s_thr);
    if (!su.ok) return;                                        // no status-0 item has such a null fit
    const int z = su.z;
    __syncthreads();                                           // the running sums are read; wave 0's f and r take their place
    // ---- the wave's replicates
    const uint32_t N = (uint32_t)a.n_doc[d];
    const double Nd = (double)N, lam_obs = a.stat[j];
    const int bbeg = (int)blockIdx.y * a.reps_per_block, bend = min(a.B, bbeg + a.reps_per_block);
    for (int v = lane; v < V; v += 64) w.hist[v] = 0u;
    rf_wave_sync();
    int ge = 0, zero = 0;
    unsigned long long its = 0ull;
    for (int b = bbeg + wave; b < bend; b += nw) {
        draw_row(lane, P2, z, N, s_thr, w.hist, (uint32_t)j, a.b0 + (uint32_t)b, a.stream, a.k0, a.k1);
        rf_wave_sync();
        for (int v = lane; v < V; v += 64) w.fb[v] = (double)w.hist[v] / Nd;
        rf_wave_sync();
        const PrStat r = pr_statistic(P, w, n0, trow, V, lane, a.maxiter, a.tol);
        ge += r.lam >= lam_obs; zero += r.lam == 0.0; its += (unsigned long long)r.iters;
        if (a.rep && lane == 0) a.rep[(size_t)b * TD + j] = r.lam;
        for (int v = lane; v < V; v += 64) w.hist[v] = 0u;
        rf_wave_sync();
    }
    if (lane == 0) {
        if (ge) atomicAdd(&a.count_ge[j], ge);
        if (zero) atomicAdd(&a.count_zero[j], zero);
        if (its) atomicAdd(&a.iters[j], its);
    }
}

// ---- mmm_presence_power: the same replicate, drawn at every level of a grid of totals and spiked-in fractions --------------------------------
struct PwArgs {
    PrArgs pr;                       // as the presence test's replicate launch takes it; pr.rep is [L][B][T D] here
    int H, G1, g_lo, g_hi;           // G1 = 1 + G fractions; this launch walks g in [g_lo, g_hi) of every h
    const double* frac;              // [G1], frac[0] = 0
    const int32_t* n_level;          // [H][D] totals, or NULL: the observed ones (H = 1)
    const double* crit;              // [H][T D]: read where null_buf == NULL
    double* null_buf;                // [items of this launch][H][B]: the statistics of the null levels, or NULL
    int32_t* count_reject; int32_t* count_zero;     // [L][T D]
};

// Grid (items, replicate chunks), blockDim 64 nw.  Dynamic LDS: int z (16 bytes) | uint32 thr[P2] | the observed null weights in the order
// of the list [Cp] | P_LDS: the rows of A1 at stride V | per wave pr_wave_doubles doubles.  The lists and the staged rows are built once;
// then the block walks the item's levels.  Per level the mixture p and its running sums are formed where wave 0's f and r follow, as in
// k_presence_rep, so a block-wide barrier separates the levels.  A null level (g = 0) leaves its statistics in null_buf for
// k_power_select; every other level is compared with crit[h][j] where it is computed.
template <bool P_LDS>
__global__ __launch_bounds__(64 * kPrMaxWaves) void k_power_rep(const PwArgs q)
{
    extern __shared__ __attribute__((aligned(16))) double s_pr[];
    const PrArgs& a = q.pr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6), nt = (int)blockDim.x;
    const int C = a.C, V = a.V, P2 = a.P2;
    const int j = a.items[blockIdx.x], d = j % a.D, t = a.targets[j / a.D], TD = a.T * a.D;
    int* s_z = (int*)s_pr;
    uint32_t* s_thr = (uint32_t*)(s_pr + 2);
    double* s_w0 = s_pr + 2 + P2 / 2;                          // P2 >= 4, Cp a multiple of 64: 16-byte steps
    double* s_rows = s_w0 + a.Cp;
    double* wave_base = s_rows + (P_LDS ? a.stage_doubles : 0);
    const PrWave w = pr_carve(wave_base + (size_t)wave * a.wave_doubles, a.Cp, V);
    int tpos;
    const int n1 = pr_lists(a, d, t, w, lane, tpos);
    const int n0 = n1 - 1;
    // the observed null weights, in the order of the list: kept for all levels (every fit overwrites the wave's own w0)
    if (wave == 0)
        for (int i = lane; i < n0; i += 64) s_w0[i] = a.w_null[(size_t)j * C + w.act0[i]];
    int trow = t;
    if (P_LDS) {
        for (int i = wave; i < n1; i += nw) {
            const double* src = a.P + (size_t)w.act1[i] * V;
            for (int v = lane; v < V; v += 64) s_rows[(size_t)i * V + v] = src[v];
        }
        rf_wave_sync();
        for (int i = lane; i < ((n1 + 63) & ~63); i += 64) w.act1[i] = i < n1 ? i : 0;
        for (int i = lane; i < ((n0 + 63) & ~63); i += 64) w.act0[i] = i < n0 ? (i < tpos ? i : i + 1) : (tpos == 0 ? 1 : 0);
        trow = tpos;
    }
    const double* __restrict__ P = P_LDS ? s_rows : a.P;
    for (int v = lane; v < V; v += 64) w.hist[v] = 0u;
    __syncthreads();                                           // the staged rows and the weights are there
    double W0 = 0.0;                                           // the sequential sum over ascending c (the zeros outside A0 add nothing)
    for (int i = 0; i < n0; ++i) W0 += s_w0[i];
    double* s_p = pr_carve(wave_base, a.Cp, V).fb;
    const int bbeg = (int)blockIdx.y * a.reps_per_block, bend = min(a.B, bbeg + a.reps_per_block);
    for (int h = 0; h < q.H; ++h) {
        const uint32_t N = (uint32_t)(q.n_level ? q.n_level[(size_t)h * a.D + d] : a.n_doc[d]);
        const double Nd = (double)N;
        for (int g = q.g_lo; g < q.g_hi; ++g) {
            const int lvl = h * q.G1 + g;
            __syncthreads();                                   // the level before is done with wave 0's f and r
            // ---- the generating weights in the order of act1 (g = 0: w0 itself over act0), the mixture in ascending c, its thresholds
            const int ng = g ? n1 : n0;
            const int* actg = g ? w.act1 : w.act0;
            if (g) {
                const double phi = q.frac[g], keep = 1.0 - phi, wt = phi * W0;
                for (int i = lane; i < n1; i += 64) w.w1[i] = i == tpos ? wt : keep * s_w0[i < tpos ? i : i - 1];
                rf_wave_sync();
            }
            const double* wg = g ? w.w1 : s_w0;
            for (int v = tid; v < V; v += nt) {
                double p = 0.0;
                for (int i = 0; i < ng; ++i) p += wg[i] * P[actg[i] * V + v];
                s_p[v] = p;
            }
            const DrawSetup su = draw_thresholds(tid, nt, V, P2, s_p, s_p + V, s_z, s_thr);
            if (!su.ok) return;                                // the whole block: no testable item has such a null fit
            const int z = su.z;
            __syncthreads();                                   // the running sums are read; wave 0's f and r take their place
            const double crit = q.null_buf ? 0.0 : q.crit[(size_t)h * TD + j];
            int rej = 0, zero = 0;
            unsigned long long its = 0ull;
            for (int b = bbeg + wave; b < bend; b += nw) {
                draw_row(lane, P2, z, N, s_thr, w.hist, (uint32_t)(lvl * TD + j), a.b0 + (uint32_t)b, a.stream, a.k0, a.k1);
                rf_wave_sync();
                for (int v = lane; v < V; v += 64) w.fb[v] = (double)w.hist[v] / Nd;
                rf_wave_sync();
                const PrStat r = pr_statistic(P, w, n0, trow, V, lane, a.maxiter, a.tol);
                rej += r.lam > crit; zero += r.lam == 0.0; its += (unsigned long long)r.iters;
                if (lane == 0) {
                    if (q.null_buf) q.null_buf[((size_t)blockIdx.x * q.H + h) * a.B + b] = r.lam;
                    if (a.rep) a.rep[((size_t)lvl * a.B + b) * TD + j] = r.lam;
                }
                for (int v = lane; v < V; v += 64) w.hist[v] = 0u;
                rf_wave_sync();
            }
            if (lane == 0) {
                if (rej && !q.null_buf) atomicAdd(&q.count_reject[(size_t)lvl * TD + j], rej);
                if (zero) atomicAdd(&q.count_zero[(size_t)lvl * TD + j], zero);
                if (its) atomicAdd(&a.iters[j], its);
            }
        }
    }
}

// One wave per (item of the chunk, h): crit[h][j] = s_{m+1}, the (m + 1)-th largest of the B null statistics, by m + 1 extractions of the
// largest remaining pair (value descending, equal values by ascending index; nothing is moved), +inf where m < 0 or m + 1 > B; then
// count_reject of the null level, #{b : s_b > crit}.  The value is an element of the set: no arithmetic touches it.
__global__ __launch_bounds__(256) void k_power_select(const double* __restrict__ null_buf, const int32_t* __restrict__ items, int n_items, int H, int B, int m,
                                                      int TD, int G1, double* crit, int32_t* count_reject)
{
    const int lane = threadIdx.x & 63, wv = (int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (wv >= n_items * H) return;
    const int h = wv % H, j = items[wv / H];
    const double* s = null_buf + (size_t)wv * B;
    double c = __builtin_inf();
    if (m >= 0 && m < B) {
        double pv = __builtin_inf();
        int pi = -1;
        for (int k = 0; k <= m; ++k) {
            double bv = -1.0;                                  // a statistic is >= 0
            int bi = 0x7fffffff;
            for (int i = lane; i < B; i += 64) {
                const double x = s[i];
                if ((x < pv || (x == pv && i > pi)) && x > bv) { bv = x; bi = i; }
            }
            double mv = bv;
            for (int off = 32; off > 0; off >>= 1) mv = fmax(mv, __shfl_xor(mv, off, 64));
            int mi = bv == mv ? bi : 0x7fffffff;
            for (int off = 32; off > 0; off >>= 1) mi = min(mi, __shfl_xor(mi, off, 64));
            pv = mv; pi = mi;
        }
        c = pv;
    }
    int n = 0;
    for (int i = lane; i < B; i += 64) n += s[i] > c;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) {
        crit[(size_t)h * TD + j] = c;
        count_reject[(size_t)h * G1 * TD + j] = n;
    }
}

// ---- what the two entries' hosts share ---------------------------------------------------------------------------------------------------------
// observed phase: as many waves per block as their buffers leave room for; few items: fewer, so that they spread over the CUs
int pr_launch_obs(mmm_ctx* ctx, const PrArgs& a, size_t TD, size_t pw, int cus)
{
    int nw = kPrMaxWaves;
    while (nw > 1 && nw * pw > kPrLdsBlock) nw >>= 1;
    while (nw > 1 && ((int64_t)TD + nw - 1) / nw < cus) nw >>= 1;
    const size_t lds = nw * pw;
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(kPrMaxWaves / nw, (int64_t)(kPrLdsBlock / lds)));
    const unsigned grid = (unsigned)std::min<int64_t>(((int64_t)TD + nw - 1) / nw, (int64_t)cus * per_cu);
    if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)k_presence_obs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_presence_obs, dim3(grid), dim3(64 * nw), lds, ctx->stream, a);
    MMM_LAUNCH_CHECK(ctx);
    return MMM_OK;
}

// |A1| of item j
int pr_n1(const uint8_t* allowed, int C, int d, int t)
{
    if (!allowed) return C;
    int n = 0;
    for (int c = 0; c < C; ++c) n += allowed[(size_t)d * C + c] != 0 || c == t;
    return n;
}

// replicate phase: the waves of a block and the rows of P it can stage beside their buffers, `fixed` bytes going to the block's own arrays
struct PrPlan {
    int nw, rows_cap;
};

PrPlan pr_plan(const mmm_ctx* ctx, size_t fixed, size_t pw, int V, int max_n1)
{
    int nw = 1;
    for (int t = kPrMaxWaves; t >= 1; t >>= 1)
        if (fixed + t * pw <= kPrLdsBlock) { nw = t; break; }
    // rows of P a block can stage beside nw waves' buffers (one double may pad the rows to 16 bytes)
    auto cap = [&](int t) { const size_t room = (kPrLdsBlock - fixed - t * pw) / sizeof(double); return room ? (int)((room - 1) / (size_t)V) : 0; };
    int rows_cap = 0;
    if (!mmm_off(ctx->tune, MMM_OFF_REFIT_LDS)) {
        if (nw == kPrMaxWaves && cap(nw) < max_n1 && cap(nw / 2) >= max_n1) nw >>= 1;       // four waves with every item's rows in LDS beat eight through L2
        rows_cap = cap(nw);
    }
    return PrPlan{nw, rows_cap};
}

// replicates per block: one per wave, more while the launch still covers the device several times over (a block's set-up is shared by
// its replicates); the geometry cannot change a bit of the output
int pr_reps_per_block(int nw, int B, size_t n, int cus)
{
    int rpb = nw;
    while (rpb < B && (int64_t)n * ((B + 2 * rpb - 1) / (2 * rpb)) >= 8ll * cus) rpb *= 2;
    while ((B + rpb - 1) / rpb > 65535) rpb *= 2;
    return rpb;
}

} // namespace

extern "C" int mmm_presence_test(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* cat,
                                 const uint8_t* allowed, int T, const int32_t* targets, int B, int b0, uint64_t seed, uint32_t stream, int maxiter, double tol,
                                 double* w_null, double* stat, double* score, double* w_alt, int32_t* count_ge, int32_t* count_zero, int8_t* status,
                                 int64_t* iters, double* rep_stat)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, C >= 1 && V >= 1 && D >= 0 && T >= 1 && cat && targets, "mmm_presence_test: NULL argument, D < 0, C < 1, V < 1 or T < 1");
    if (C > kPrMaxC) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_presence_test: C = %d catalogue signatures (limit %d)", C, kPrMaxC);
    if (V > kPrMaxV)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_presence_test: V = %d terms; a block keeps the thresholds and its waves' count vectors in LDS, which holds at most V = %d", V, kPrMaxV);
    MMM_CHECK(ctx, maxiter >= 1 && tol >= 0.0, "mmm_presence_test: maxiter = %d (>= 1), tol = %g (>= 0)", maxiter, tol);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0, "mmm_presence_test: B < 0 or b0 < 0");
    MMM_CHECK(ctx, (int64_t)b0 + (int64_t)B <= (int64_t)INT32_MAX, "mmm_presence_test: b0 + B exceeds 2^31 - 1");
    if ((int64_t)T * (int64_t)D >= ((int64_t)1 << 31))
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_presence_test: T D = %lld items (limit 2^31 - 1: the item is a 32-bit counter word)", (long long)T * D);
    for (int i = 0; i < T; ++i) MMM_CHECK(ctx, targets[i] >= 0 && targets[i] < C, "mmm_presence_test: targets[%d] = %d is no row of the catalogue (C = %d)", i, targets[i], C);
    if (int rc = mmm_check_csr(ctx, "mmm_presence_test", D, V, doc_ptr, term, count)) return rc;
    std::vector<int32_t> n_doc((size_t)D);
    if (int rc = mmm_doc_totals(ctx, "mmm_presence_test", D, doc_ptr, count, n_doc.data())) return rc;
    std::vector<double> P;           // the catalogue with rows normalised: mmm_refit_exposures' P
    if (int rc = mmm_normalise_rows(ctx, "mmm_presence_test", C, V, cat, P)) return rc;
    if (D == 0) return MMM_OK;
    MMM_CHECK(ctx, w_null && stat && score && w_alt && count_ge && count_zero && status && iters, "mmm_presence_test: NULL output");
    const size_t TD = (size_t)T * (size_t)D, TDC = TD * (size_t)C, DC = (size_t)D * C;
    const bool want_rep = rep_stat && B > 0;

    const int Cp = (C + 63) & ~63, cus = std::max(1, ctx->num_cu);
    const int wd = pr_wave_doubles(Cp, V);
    const size_t pw = sizeof(double) * (size_t)wd;

    DevCsr csr; DevBuf<int32_t> tg, nd, cnt, itm; DevBuf<double> Pd, outd, rep; DevBuf<uint8_t> alw; DevBuf<int8_t> st; DevBuf<unsigned long long> its;
    DevBuf<int> counter;
    MMM_HIP(ctx, tg.alloc((size_t)T)); MMM_HIP(ctx, nd.alloc((size_t)D));
    MMM_HIP(ctx, Pd.alloc(P.size())); MMM_HIP(ctx, outd.alloc(TDC + 3 * TD)); MMM_HIP(ctx, st.alloc(TD)); MMM_HIP(ctx, its.alloc(TD));
    MMM_HIP(ctx, cnt.alloc(2 * TD)); MMM_HIP(ctx, counter.alloc(1));
    if (allowed) MMM_HIP(ctx, alw.alloc(DC));
    if (int rc = csr.upload(ctx, D, doc_ptr, term, count)) return rc;
    MMM_HIP(ctx, hipMemcpyAsync(tg.p, targets, sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(nd.p, n_doc.data(), sizeof(int32_t) * (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(Pd.p, P.data(), sizeof(double) * P.size(), hipMemcpyHostToDevice, ctx->stream));
    if (allowed) MMM_HIP(ctx, hipMemcpyAsync(alw.p, allowed, DC, hipMemcpyHostToDevice, ctx->stream));
    // what an untestable item and an item without replicates leave behind
    MMM_HIP(ctx, hipMemsetAsync(outd.p, 0, sizeof(double) * outd.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(st.p, 0, TD, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(its.p, 0, sizeof(unsigned long long) * TD, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * 2 * TD, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));

    PrArgs a{};
    a.D = D; a.C = C; a.V = V; a.Cp = Cp; a.T = T; a.maxiter = maxiter; a.tol = tol;
    a.doc_ptr = csr.ptr; a.term = csr.term; a.count = csr.count; a.P = Pd.p; a.allowed = allowed ? alw.p : nullptr; a.targets = tg.p;
    a.w_null = outd.p; a.stat = outd.p + TDC; a.score = a.stat + TD; a.w_alt = a.score + TD; a.status = st.p; a.iters = its.p; a.counter = counter.p;
    a.n_doc = nd.p; a.B = B; a.b0 = (uint32_t)b0; a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.count_ge = cnt.p; a.count_zero = cnt.p + TD; a.wave_doubles = wd;

    // ---- observed phase
    if (int rc = pr_launch_obs(ctx, a, TD, pw, cus)) return rc;
    // the statuses come back: the host lists the items that take replicates (a T D-byte copy; the list could be compacted on the device, but
    // the host needs the statuses anyway to fill the counts of the items that take none)
    std::vector<int8_t> hst(TD);
    MMM_HIP(ctx, hipMemcpyAsync(hst.data(), st.p, TD, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));

    // ---- replicate phase
    std::vector<int32_t> staged, direct;
    if (B > 0) {
        int P2 = 4;
        while (P2 < V) P2 <<= 1;
        const size_t fixed = 16 + sizeof(uint32_t) * (size_t)P2;
        std::vector<int> n1((size_t)TD, 0);
        int max_n1 = 0;
        size_t n_items = 0;
        for (size_t j = 0; j < TD; ++j) {
            if (hst[j] != 0) continue;
            const int n = pr_n1(allowed, C, (int)(j % (size_t)D), targets[j / (size_t)D]);
            n1[j] = n; max_n1 = std::max(max_n1, n); ++n_items;
        }
        if (n_items) {
            const PrPlan plan = pr_plan(ctx, fixed, pw, V, max_n1);
            const int nw = plan.nw, rows_cap = plan.rows_cap;
            int rows = 0;
            for (size_t j = 0; j < TD; ++j) {
                if (hst[j] != 0) continue;
                if (n1[j] <= rows_cap) { staged.push_back((int32_t)j); rows = std::max(rows, n1[j]); }
                else direct.push_back((int32_t)j);
            }
            std::vector<int32_t> all(staged);
            all.insert(all.end(), direct.begin(), direct.end());
            MMM_HIP(ctx, itm.alloc(all.size()));
            MMM_HIP(ctx, hipMemcpyAsync(itm.p, all.data(), sizeof(int32_t) * all.size(), hipMemcpyHostToDevice, ctx->stream));
            if (want_rep) {
                MMM_HIP(ctx, rep.alloc((size_t)B * TD));
                MMM_HIP(ctx, hipMemsetAsync(rep.p, 0, sizeof(double) * (size_t)B * TD, ctx->stream));
            }
            a.P2 = P2; a.rep = want_rep ? rep.p : nullptr;
            for (int part = 0; part < 2; ++part) {
                const size_t n = part ? direct.size() : staged.size();
                if (!n) continue;
                const int rpb = pr_reps_per_block(nw, B, n, cus);
                a.items = itm.p + (part ? staged.size() : 0);
                a.reps_per_block = rpb;
                a.stage_doubles = part ? 0 : (int)(((size_t)rows * V + 1) & ~(size_t)1);
                const size_t lds = fixed + sizeof(double) * (size_t)a.stage_doubles + nw * pw;
                auto kern = part ? k_presence_rep<false> : k_presence_rep<true>;
                if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(kern, dim3((unsigned)n, (unsigned)((B + rpb - 1) / rpb)), dim3(64 * nw), lds, ctx->stream, a);
                MMM_LAUNCH_CHECK(ctx);
            }
        }
    }
    // staged on the host so that a failing copy leaves the caller's arrays as they were
    std::vector<double> ho(TDC + 3 * TD), hr(want_rep && rep.p ? (size_t)B * TD : 0);
    std::vector<int32_t> hc(2 * TD);
    std::vector<unsigned long long> hi(TD);
    MMM_HIP(ctx, hipMemcpyAsync(ho.data(), outd.p, sizeof(double) * ho.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hc.data(), cnt.p, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hi.data(), its.p, sizeof(unsigned long long) * TD, hipMemcpyDeviceToHost, ctx->stream));
    if (hr.size()) MMM_HIP(ctx, hipMemcpyAsync(hr.data(), rep.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(w_null, ho.data(), sizeof(double) * TDC);
    memcpy(stat, ho.data() + TDC, sizeof(double) * TD); memcpy(score, ho.data() + TDC + TD, sizeof(double) * TD);
    memcpy(w_alt, ho.data() + TDC + 2 * TD, sizeof(double) * TD);
    memcpy(status, hst.data(), TD);
    for (size_t j = 0; j < TD; ++j) {
        count_ge[j] = hst[j] == 1 ? B : hc[j];            // statistic 0: every replicate is at least as large, and none is run
        count_zero[j] = hc[TD + j];
        iters[j] = (int64_t)hi[j];
    }
    if (want_rep) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int b = 0; b < B; ++b)
            for (size_t j = 0; j < TD; ++j) rep_stat[(size_t)b * TD + j] = hst[j] == 0 ? hr[(size_t)b * TD + j] : nan;
    }
    return MMM_OK;
}

extern "C" int mmm_presence_power(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* cat,
                                  const uint8_t* allowed, int T, const int32_t* targets, int G, const double* fractions, int H, const int32_t* n_level,
                                  double alpha, int B, int b0, uint64_t seed, uint32_t stream, int maxiter, double tol, const double* crit_in, double* w_null,
                                  double* stat, double* score, double* w_alt, int8_t* status, int64_t* iters, double* crit, int32_t* count_reject,
                                  int32_t* count_zero, double* rep_stat)
{
    if (!ctx) return MMM_ERR_ARG;
    MMM_HIP(ctx, hipSetDevice(ctx->device));
    MMM_CHECK(ctx, C >= 1 && V >= 1 && D >= 0 && T >= 1 && cat && targets, "mmm_presence_power: NULL argument, D < 0, C < 1, V < 1 or T < 1");
    if (C > kPrMaxC) return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_presence_power: C = %d catalogue signatures (limit %d)", C, kPrMaxC);
    if (V > kPrMaxV)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_presence_power: V = %d terms; a block keeps the thresholds and its waves' count vectors in LDS, which holds at most V = %d", V, kPrMaxV);
    MMM_CHECK(ctx, maxiter >= 1 && tol >= 0.0, "mmm_presence_power: maxiter = %d (>= 1), tol = %g (>= 0)", maxiter, tol);
    MMM_CHECK(ctx, G >= 1 && H >= 1 && fractions, "mmm_presence_power: G < 1, H < 1 or fractions == NULL");
    if (G > kPwMaxLevels || H > kPwMaxLevels)
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_presence_power: G = %d fractions, H = %d totals (limit %d each)", G, H, kPwMaxLevels);
    MMM_CHECK(ctx, n_level || H == 1, "mmm_presence_power: n_level == NULL means the observed totals alone, H = 1 (got H = %d)", H);
    MMM_CHECK(ctx, alpha > 0.0 && alpha < 1.0, "mmm_presence_power: alpha = %g is not in (0, 1)", alpha);
    for (int g = 0; g < G; ++g)
        MMM_CHECK(ctx, fractions[g] > (g ? fractions[g - 1] : 0.0) && fractions[g] <= 1.0,
                  "mmm_presence_power: fractions[%d] = %g: the fractions must increase strictly within (0, 1]", g, fractions[g]);
    MMM_CHECK(ctx, B >= 0 && b0 >= 0, "mmm_presence_power: B < 0 or b0 < 0");
    MMM_CHECK(ctx, B >= 1 || crit_in, "mmm_presence_power: B = 0 replicates leave no critical value; give crit_in");
    MMM_CHECK(ctx, (int64_t)b0 + (int64_t)B <= (int64_t)INT32_MAX, "mmm_presence_power: b0 + B exceeds 2^31 - 1");
    const int G1 = 1 + G, L = H * G1;
    if ((int64_t)L * (int64_t)T * (int64_t)D >= ((int64_t)1 << 31))
        return mmm_fail(ctx, MMM_ERR_UNSUPPORTED, "mmm_presence_power: L T D = %lld level items (limit 2^31 - 1: the level item is a 32-bit counter word)",
                        (long long)L * T * D);
    for (int i = 0; i < T; ++i) MMM_CHECK(ctx, targets[i] >= 0 && targets[i] < C, "mmm_presence_power: targets[%d] = %d is no row of the catalogue (C = %d)", i, targets[i], C);
    if (n_level)
        for (size_t i = 0; i < (size_t)H * (size_t)D; ++i)
            MMM_CHECK(ctx, n_level[i] >= 1, "mmm_presence_power: n_level[%d][%d] = %d (>= 1)", (int)(i / (size_t)D), (int)(i % (size_t)D), n_level[i]);
    if (int rc = mmm_check_csr(ctx, "mmm_presence_power", D, V, doc_ptr, term, count)) return rc;
    std::vector<int32_t> n_doc((size_t)D);
    if (int rc = mmm_doc_totals(ctx, "mmm_presence_power", D, doc_ptr, count, n_doc.data())) return rc;
    std::vector<double> P;
    if (int rc = mmm_normalise_rows(ctx, "mmm_presence_power", C, V, cat, P)) return rc;
    if (D == 0) return MMM_OK;
    MMM_CHECK(ctx, w_null && stat && score && w_alt && status && iters && crit && count_reject && count_zero, "mmm_presence_power: NULL output");
    const size_t TD = (size_t)T * (size_t)D, TDC = TD * (size_t)C, DC = (size_t)D * C, HTD = (size_t)H * TD, LTD = (size_t)L * TD;
    const bool want_rep = rep_stat && B > 0;
    const int m = (int)std::floor(alpha * (double)((int64_t)B + 1)) - 1;

    const int Cp = (C + 63) & ~63, cus = std::max(1, mmm_geo_cus(ctx));
    const int wd = pr_wave_doubles(Cp, V);
    const size_t pw = sizeof(double) * (size_t)wd;

    DevCsr csr; DevBuf<int32_t> tg, nd, nl, cnt, itm; DevBuf<double> Pd, outd, fr, cr, nb, rep; DevBuf<uint8_t> alw; DevBuf<int8_t> st; DevBuf<unsigned long long> its;
    DevBuf<int> counter;
    MMM_HIP(ctx, tg.alloc((size_t)T)); MMM_HIP(ctx, nd.alloc((size_t)D)); MMM_HIP(ctx, fr.alloc((size_t)G1)); MMM_HIP(ctx, cr.alloc(HTD));
    MMM_HIP(ctx, Pd.alloc(P.size())); MMM_HIP(ctx, outd.alloc(TDC + 3 * TD)); MMM_HIP(ctx, st.alloc(TD)); MMM_HIP(ctx, its.alloc(TD));
    MMM_HIP(ctx, cnt.alloc(2 * LTD)); MMM_HIP(ctx, counter.alloc(1));
    if (allowed) MMM_HIP(ctx, alw.alloc(DC));
    if (n_level) MMM_HIP(ctx, nl.alloc((size_t)H * D));
    if (int rc = csr.upload(ctx, D, doc_ptr, term, count)) return rc;
    std::vector<double> hfr((size_t)G1, 0.0);
    std::copy(fractions, fractions + G, hfr.begin() + 1);
    MMM_HIP(ctx, hipMemcpyAsync(tg.p, targets, sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(nd.p, n_doc.data(), sizeof(int32_t) * (size_t)D, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(fr.p, hfr.data(), sizeof(double) * (size_t)G1, hipMemcpyHostToDevice, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(Pd.p, P.data(), sizeof(double) * P.size(), hipMemcpyHostToDevice, ctx->stream));
    if (allowed) MMM_HIP(ctx, hipMemcpyAsync(alw.p, allowed, DC, hipMemcpyHostToDevice, ctx->stream));
    if (n_level) MMM_HIP(ctx, hipMemcpyAsync(nl.p, n_level, sizeof(int32_t) * (size_t)H * D, hipMemcpyHostToDevice, ctx->stream));
    // what an untestable item leaves behind
    MMM_HIP(ctx, hipMemsetAsync(outd.p, 0, sizeof(double) * outd.n, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(st.p, 0, TD, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(its.p, 0, sizeof(unsigned long long) * TD, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * 2 * LTD, ctx->stream));
    MMM_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int), ctx->stream));
    if (crit_in) MMM_HIP(ctx, hipMemcpyAsync(cr.p, crit_in, sizeof(double) * HTD, hipMemcpyHostToDevice, ctx->stream));
    else MMM_HIP(ctx, hipMemsetAsync(cr.p, 0, sizeof(double) * HTD, ctx->stream));

    PwArgs q{};
    PrArgs& a = q.pr;
    a.D = D; a.C = C; a.V = V; a.Cp = Cp; a.T = T; a.maxiter = maxiter; a.tol = tol;
    a.doc_ptr = csr.ptr; a.term = csr.term; a.count = csr.count; a.P = Pd.p; a.allowed = allowed ? alw.p : nullptr; a.targets = tg.p;
    a.w_null = outd.p; a.stat = outd.p + TDC; a.score = a.stat + TD; a.w_alt = a.score + TD; a.status = st.p; a.iters = its.p; a.counter = counter.p;
    a.n_doc = nd.p; a.B = B; a.b0 = (uint32_t)b0; a.k0 = (uint32_t)(seed & 0xffffffffull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream;
    a.wave_doubles = wd;
    q.H = H; q.G1 = G1; q.frac = fr.p; q.n_level = n_level ? nl.p : nullptr; q.crit = cr.p; q.count_reject = cnt.p; q.count_zero = cnt.p + LTD;

    // ---- observed phase: the presence test's
    if (int rc = pr_launch_obs(ctx, a, TD, pw, cus)) return rc;
    std::vector<int8_t> hst(TD);
    MMM_HIP(ctx, hipMemcpyAsync(hst.data(), st.p, TD, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));

    // ---- levels: every testable item (status 0, 1 and 2), staged items first
    if (B > 0) {
        int P2 = 4;
        while (P2 < V) P2 <<= 1;
        const size_t fixed = 16 + sizeof(uint32_t) * (size_t)P2 + sizeof(double) * (size_t)Cp;
        std::vector<int> n1((size_t)TD, 0);
        int max_n1 = 0;
        for (size_t j = 0; j < TD; ++j) {
            if (hst[j] == 3) continue;
            n1[j] = pr_n1(allowed, C, (int)(j % (size_t)D), targets[j / (size_t)D]);
            max_n1 = std::max(max_n1, n1[j]);
        }
        if (max_n1) {
            const PrPlan plan = pr_plan(ctx, fixed, pw, V, max_n1);
            const int nw = plan.nw;
            std::vector<int32_t> all, direct;
            int rows = 0;
            for (size_t j = 0; j < TD; ++j) {
                if (hst[j] == 3) continue;
                if (n1[j] <= plan.rows_cap) { all.push_back((int32_t)j); rows = std::max(rows, n1[j]); }
                else direct.push_back((int32_t)j);
            }
            const size_t n_staged = all.size();
            all.insert(all.end(), direct.begin(), direct.end());
            MMM_HIP(ctx, itm.alloc(all.size()));
            MMM_HIP(ctx, hipMemcpyAsync(itm.p, all.data(), sizeof(int32_t) * all.size(), hipMemcpyHostToDevice, ctx->stream));
            if (want_rep) {
                MMM_HIP(ctx, rep.alloc((size_t)B * LTD));
                MMM_HIP(ctx, hipMemsetAsync(rep.p, 0, sizeof(double) * (size_t)B * LTD, ctx->stream));
            }
            a.P2 = P2; a.rep = want_rep ? rep.p : nullptr;
            const int stage_doubles = (int)(((size_t)rows * V + 1) & ~(size_t)1);
            // items [first, first + n) of the list: the staged ones and the direct ones in a launch each
            auto launch = [&](size_t first, size_t n, double* null_buf) -> int {
                for (int part = 0; part < 2; ++part) {
                    const size_t lo = part ? std::max(first, n_staged) : first, hi = part ? first + n : std::min(first + n, n_staged);
                    if (lo >= hi) continue;
                    a.items = itm.p + lo;
                    a.reps_per_block = pr_reps_per_block(nw, B, hi - lo, cus);
                    a.stage_doubles = part ? 0 : stage_doubles;
                    q.null_buf = null_buf ? null_buf + (lo - first) * (size_t)H * (size_t)B : nullptr;
                    const size_t lds = fixed + sizeof(double) * (size_t)a.stage_doubles + nw * pw;
                    auto kern = part ? k_power_rep<false> : k_power_rep<true>;
                    if (lds > 48 * 1024) MMM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                    hipLaunchKernelGGL(kern, dim3((unsigned)(hi - lo), (unsigned)((B + a.reps_per_block - 1) / a.reps_per_block)), dim3(64 * nw), lds, ctx->stream, q);
                    MMM_LAUNCH_CHECK(ctx);
                }
                return MMM_OK;
            };
            if (!crit_in) {
                // the null levels, items in chunks so that their statistics stay within kPwNullBytes (one item's H B at the least)
                const size_t per_item = (size_t)H * (size_t)B;
                const size_t chunk = std::max<size_t>(1, std::min(all.size(), kPwNullBytes / (sizeof(double) * per_item)));
                MMM_HIP(ctx, nb.alloc(chunk * per_item));
                q.g_lo = 0; q.g_hi = 1;
                for (size_t first = 0; first < all.size(); first += chunk) {
                    const size_t n = std::min(chunk, all.size() - first);
                    if (int rc = launch(first, n, nb.p)) return rc;
                    const int64_t waves = (int64_t)n * H;
                    hipLaunchKernelGGL(k_power_select, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream, nb.p, itm.p + first, (int)n, H, B, m, (int)TD, G1,
                                       cr.p, cnt.p);
                    MMM_LAUNCH_CHECK(ctx);
                }
            }
            q.g_lo = 1; q.g_hi = G1;
            if (int rc = launch(0, all.size(), nullptr)) return rc;
        }
    }
    // staged on the host so that a failing copy leaves the caller's arrays as they were
    std::vector<double> ho(TDC + 3 * TD), hcr(HTD), hr(want_rep && rep.p ? (size_t)B * LTD : 0);
    std::vector<int32_t> hc(2 * LTD);
    std::vector<unsigned long long> hi(TD);
    MMM_HIP(ctx, hipMemcpyAsync(ho.data(), outd.p, sizeof(double) * ho.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hcr.data(), cr.p, sizeof(double) * HTD, hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hc.data(), cnt.p, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipMemcpyAsync(hi.data(), its.p, sizeof(unsigned long long) * TD, hipMemcpyDeviceToHost, ctx->stream));
    if (hr.size()) MMM_HIP(ctx, hipMemcpyAsync(hr.data(), rep.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, ctx->stream));
    MMM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(w_null, ho.data(), sizeof(double) * TDC);
    memcpy(stat, ho.data() + TDC, sizeof(double) * TD); memcpy(score, ho.data() + TDC + TD, sizeof(double) * TD);
    memcpy(w_alt, ho.data() + TDC + 2 * TD, sizeof(double) * TD);
    memcpy(status, hst.data(), TD);
    memcpy(crit, hcr.data(), sizeof(double) * HTD);
    memcpy(count_reject, hc.data(), sizeof(int32_t) * LTD); memcpy(count_zero, hc.data() + LTD, sizeof(int32_t) * LTD);
    for (size_t j = 0; j < TD; ++j) iters[j] = (int64_t)hi[j];
    if (want_rep) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int l = 0; l < L; ++l) {
            const bool ran = !(crit_in && l % G1 == 0);
            for (int b = 0; b < B; ++b)
                for (size_t j = 0; j < TD; ++j) {
                    const size_t i = ((size_t)l * B + b) * TD + j;
                    rep_stat[i] = ran && hst[j] != 3 && hr.size() ? hr[i] : nan;
                }
        }
    }
    return MMM_OK;
}
