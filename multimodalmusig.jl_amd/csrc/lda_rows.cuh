// lda_rows.cuh -- how the document kernels of lda.hip (included there, inside its anonymous namespace, ahead of them) fetch a document's
// terms from the four forms a corpus has on the device (LdaDev), the Elntheta prologue and the ll term they share.  The row format is
// known HERE: k_lda_estep_dense and the `fast` branch of lda_ll_block keep loads of their own, pinned where they stand, over the same
// lane-major 16-bit rows.

// position of term slot w (lane w % 16, the lane's slot w / 16) in a lane-major row of 16 x slp slots
__device__ __forceinline__ int row_slot(int w, int slp) { return (w & 15) * slp + (w >> 4); }
// 16-bit lane-major rows: slot c (0..7) of a lane's part, held as four 32-bit words (ONE 16-byte load; the rows are allocated with 16 bytes to spare)
__device__ __forceinline__ int row16_count(unsigned w0, unsigned w1, unsigned w2, unsigned w3, int c)
{
    const unsigned word = c < 4 ? (c < 2 ? w0 : w1) : (c < 6 ? w2 : w3);
    return (int)((c & 1) ? word >> 16 : word & 0xffffu);
}

// 16-bit lane-major rows: the four words of lane l's part of document dl's row (dl < D: a clamped index, the caller masks), ONE 16-byte load
__device__ __forceinline__ void lda_row16_load(const LdaDev& c, const int dl, const int l, unsigned (&w)[4])
{
    const unsigned* __restrict__ r32 = (const unsigned*)(c.dense16 + (size_t)dl * c.Vp + (size_t)l * (c.Vp >> 4));
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = r32[q];
}
// ... and the put calls of lda_row_read over them
template <int L, int PRE, bool ROT, bool ZERO_OFF, class Put>
__device__ __forceinline__ void lda_row16_put(const unsigned (&w4)[4], const bool valid, const int l, const int V, const int nch, const int rot, Put&& put)
{
#pragma unroll
    for (int j = 0; j < PRE; ++j) {
        int q = j; if (ROT) { q += rot; if (q >= nch) q -= nch; }
        const int w = q * L + l;
        const bool in = valid && (!ROT || j < nch) && w < V;
        const int n = in ? row16_count(w4[0], w4[1], w4[2], w4[3], q) : 0;
        put(j, (ZERO_OFF ? n > 0 : in) ? w : -1, n);
    }
}

// The first PRE chunks of document d for lane l of its L-lane group: put(j, term slot, count) for j = 0 .. PRE - 1 (static indices), slot -1 where
// the lane has no term in chunk j.  counts: rows of counts (16-bit lane-major rows when the corpus has them, 32-bit rows otherwise; term = slot);
// pairs (and not counts): padded (term,count) rows; neither: CSR, the document's W pairs from `start`.  V: terms of a row.
// ROT: chunk j of the lane is chunk (j + rot) mod nch of the document (nch: the document's chunks; k_lda_estep keeps the groups of a wave
// instruction on different term ranges this way); without it nch and rot are not read.
// ZERO_OFF: a zero in a row of counts is an inactive slot (the E-step kernels); otherwise the slot stays active with count 0 (the ll blocks:
// 0 log p, NaN where p underflows to 0) -- the two rules are the consumers' and are not to be unified.
// WIDE16 (L == 16): over 16-bit rows the lane's slots arrive with ONE 16-byte load (the E-step kernels; the ll blocks have their `fast` branch for
// that and keep 2-byte loads here: three registers less, which is a wave per SIMD at KP = 4).  Every load is issued where the call stands,
// ahead of the first put.
template <int L, int PRE, bool ROT, bool ZERO_OFF, bool WIDE16, bool GROUP, class Put>
__device__ __forceinline__ void lda_row_read(const LdaDev& c, const bool counts, const bool pairs, const int d, const bool valid, const int l, const int V,
                                             const int nch, const int rot, const int64_t start, const int W, Put&& put)
{
    // GROUP (the E-step kernels), every form: the PRE loads leave first, unconditional, at clamped indices; the masks are applied by the put calls
    // that follow them.  (A load inside a lane-conditional block is followed by a wait of its own: six chunks were six round trips, one after the
    // other.)  Without it (the ll blocks, PRE = 8) each load stands in its lane-conditional block: eight clamped addresses alive at once are 16
    // registers more, which the merged launch does not have -- 120 -> 128 VGPRs and 20 bytes of scratch at KP = 10, a wave per SIMD less in
    // k_lda_reduce_ll at KP <= 4; the ll blocks over 16-bit rows have their `fast` branch and do not come here.
    auto chunk = [&](int j) { int q = j; if (ROT) { q += rot; if (q >= nch) q -= nch; } return q; };
    if (counts) {
        const int* __restrict__ row = c.dense + (size_t)(valid ? d : 0) * c.Vp;
        const unsigned short* __restrict__ row16 = c.dense16 + (size_t)(valid ? d : 0) * c.Vp;
        const bool h16 = c.dense16 != nullptr;
        const int slp = c.Vp >> 4;
        if (WIDE16 && L == 16 && h16) {      // one 16-byte load instead of one 2-byte load per chunk
            unsigned w[4];
            lda_row16_load(c, valid ? d : 0, l, w);
            lda_row16_put<L, PRE, ROT, ZERO_OFF>(w, valid, l, V, nch, rot, put);
        } else if constexpr (!GROUP) {
#pragma unroll
            for (int j = 0; j < PRE; ++j) {
                const int q = chunk(j), w = q * L + l;
                const bool in = valid && (!ROT || j < nch) && w < V;
                const int n = in ? (h16 ? (int)row16[row_slot(w, slp)] : row[row_slot(w, slp)]) : 0;
                put(j, (ZERO_OFF ? n > 0 : in) ? w : -1, n);
            }
        } else {
            int n[PRE];
            if (h16) {
#pragma unroll
                for (int j = 0; j < PRE; ++j) { const int w = chunk(j) * L + l; n[j] = (int)row16[row_slot(w < V ? w : 0, slp)]; }
            } else {
#pragma unroll
                for (int j = 0; j < PRE; ++j) { const int w = chunk(j) * L + l; n[j] = row[row_slot(w < V ? w : 0, slp)]; }
            }
            __builtin_amdgcn_sched_barrier(0);      // (the puts' selects stay behind the last load: scheduled between the loads each waits for its own)
#pragma unroll
            for (int j = 0; j < PRE; ++j) {
                const int w = chunk(j) * L + l;
                const bool in = valid && (!ROT || j < nch) && w < V;
                const int nn = in ? n[j] : 0;
                put(j, (ZERO_OFF ? nn > 0 : in) ? w : -1, nn);
            }
        }
    } else {
        // GROUP: a lane without a pair in chunk j reads the first 8 bytes of doc_ptr and drops them (LdaDev::doc_ptr: there for every corpus form)
        const int2* __restrict__ src = pairs ? c.ell + (size_t)(valid ? d : 0) * V : c.tc + start;
        const int lim = pairs ? (valid ? V : 0) : W;
        if constexpr (!GROUP) {
#pragma unroll
            for (int j = 0; j < PRE; ++j) {
                const int w = chunk(j) * L + l;
                const int2 p = ((!ROT || j < nch) && w < lim) ? src[w] : make_int2(-1, 0);
                put(j, p.x, p.y);
            }
        } else {
            int2 p[PRE];
#pragma unroll
            for (int j = 0; j < PRE; ++j) {
                const int w = chunk(j) * L + l;
                const int2* __restrict__ at = ((!ROT || j < nch) && w < lim) ? src + w : (const int2*)c.doc_ptr;
                p[j] = *at;
            }
            __builtin_amdgcn_sched_barrier(0);      // (as above)
#pragma unroll
            for (int j = 0; j < PRE; ++j) {
                const int w = chunk(j) * L + l;
                const bool in = (!ROT || j < nch) && w < lim;
                put(j, in ? p[j].x : -1, in ? p[j].y : 0);
            }
        }
    }
}

// Elntheta_l = psi(gamma_l) - psi(sum_k gamma_k) (LDA.jl:78-80) of lane l < K of L-lane document group g, from the lane's gamma (0 on the lanes
// >= K).  One function for the E-step kernels and for the merged launch's early prologue: the same operations on the same lanes, so the
// same bits wherever a pass's prologue runs.
template <int L>
__device__ __forceinline__ double lda_elntheta(const double gk, const int g, const int l, const int K)
{
    const double S = group_sum<L>(gk);
    const double ps = dev_digamma_pos(l < K ? gk : S);        // lane K of the group holds psi(S)
    return ps - __shfl(ps, g * L + K, MMM_WAVE);
}

// one term of the ll numerator (LDA.jl:174-188): acc + count log(sum_k theta_k beta_kv), bc the term's KP table entries; an inactive slot adds count log 1
template <int KP>
__device__ __forceinline__ double lda_ll_term(const double (&tv)[KP], const double* bc, const bool act, const double count, const double* sLog, const double acc)
{
    double p0 = 0.0, p1 = 0.0;
#pragma unroll
    for (int k = 0; k + 1 < KP; k += 2) { p0 = fma(tv[k], bc[k], p0); p1 = fma(tv[k + 1], bc[k + 1], p1); }
    if (KP & 1) p0 = fma(tv[KP - 1], bc[KP - 1], p0);
    const double p = act ? p0 + p1 : 1.0;
    return fma(count, dev_log_tab(p, sLog), acc);
}
