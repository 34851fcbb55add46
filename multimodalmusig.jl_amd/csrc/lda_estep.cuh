// lda_estep.cuh -- the E-step kernels of lda.hip (included there, inside its anonymous namespace): k_lda_estep (any corpus form, LDS slabs;
// grid-stride or single-step), k_lda_estep_block (single-step, statistics as a block product, no slabs) and k_lda_estep_dense (rows of
// counts, statistics in registers).  The first two read documents through lda_row_read (lda_rows.cuh).  LDA.jl:69-108.
__device__ __forceinline__ void lds_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// What k_lda_estep and k_lda_estep_block resolve first: the arrays of pass t (EstepArgs::now: the host has resolved the ring slots; replica
// blockIdx.y's copies in a batch build, rep()) and the block's partial statistics.  (k_lda_estep_dense and the wide kernels of lda_stage.cuh
// spell their four slots out: through this struct the scalar instructions at their heads come out in another order, and those kernels
// are kept instruction for instruction.)
template <bool RB = false>
struct EstepPass {
    const double* __restrict__ gam; const double* __restrict__ gprev; double* __restrict__ gnext; double* __restrict__ Eln;
    const double* __restrict__ eB; const double* __restrict__ bprev;
    __device__ __forceinline__ explicit EstepPass(const EstepArgs& a)
        : gam(a.now.gam), gprev(a.now.gprev), gnext(a.now.gnext), Eln(a.now.Eln), eB(a.now.eB), bprev(a.now.bprev)
    {
        if constexpr (RB) {
            const size_t KD = (size_t)a.c.K * a.c.D, VK = (size_t)a.c.V * a.c.K;
            gam = rep<RB>(gam, KD); gprev = rep<RB>(gprev, KD); gnext = rep<RB>(gnext, KD); Eln = rep<RB>(Eln, KD);
            eB = rep<RB>(eB, VK); bprev = rep<RB>(bprev, VK);
        }
    }
    // ctl->stop was written by the previous launch's tail wave: a trip to memory.  As a VECTOR load (a relaxed atomic load is not made a scalar
    // one) issued ahead of the kernel's other loads it returns in order with them and no other load's issue waits for it -- scalar loads
    // return out of order, so the wait for any kernel argument fetched after it was a wait for this flag.  stop_now() where it is consumed.
    static __device__ __forceinline__ int stop_request(const EstepArgs& a) { return lda_stop_request(rep<RB>(a.ctl, 1)); }
    static __device__ __forceinline__ double* partial(const EstepArgs& a, const int K)
    {
        double* out = a.partial + (size_t)blockIdx.x * K * a.pstride;
        if constexpr (RB) out += (size_t)blockIdx.y * gridDim.x * K * a.pstride;
        return out;
    }
};

// one chunk of L terms of a document group: phi_kw n_w into the accumulators and the wave's slab, and (LL) the
// log-likelihood numerator of the previous iteration.  __restrict__ tells the compiler that the slab atomics do not
// alias the table reads, so the reads of the following chunk can be issued ahead of them.
template <int KP, bool LL>
__device__ __forceinline__ void lda_chunk(const int2 tcv, const bool act, const int V, const double (&av)[KP], double (&acc)[KP],
                                          const double* __restrict__ sB, const double* __restrict__ sBeta,
                                          const double* __restrict__ myT, double* __restrict__ slab, double& ll_acc)
{
    const double n = (double)tcv.y;
    if (LL) {
        const double* bc = sBeta + tcv.x;
        double p0 = 0.0, p1 = 0.0;
#pragma unroll
        for (int k = 0; k + 1 < KP; k += 2) { p0 = fma(myT[k], bc[k * V], p0); p1 = fma(myT[k + 1], bc[(k + 1) * V], p1); }
        if (KP & 1) p0 = fma(myT[KP - 1], bc[(KP - 1) * V], p0);
        ll_acc = fma(n, dev_log_pos(p0 + p1), ll_acc);                    // inactive lanes: n = 0
        __builtin_amdgcn_sched_barrier(0);                                  // keep the two halves' live ranges apart
    }
    const double* bcol = sB + tcv.x;
    if (KP >= 20) {
        // many topics: the products are formed twice (a second LDS read of the column) instead of being kept -- 64 registers
        // less, which is the difference between this build fitting its 256 and spilling
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int k = 0; k + 1 < KP; k += 2) { s0 = fma(av[k], bcol[k * V], s0); s1 = fma(av[k + 1], bcol[(k + 1) * V], s1); }
        const double r = act ? n * dev_rcp(s0 + s1) : 0.0;
        __builtin_amdgcn_sched_barrier(0);
        double* scol = slab + tcv.x;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const double x = av[k] * bcol[k * V] * r;
            acc[k] += x;
            if (act) unsafeAtomicAdd(&scol[k * V], x);
        }
        return;
    }
    double b[KP], s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) b[k] = av[k] * bcol[k * V];
#pragma unroll
    for (int k = 0; k + 1 < KP; k += 2) { s0 += b[k]; s1 += b[k + 1]; }
    if (KP & 1) s0 += b[KP - 1];
    const double r = act ? n * dev_rcp(s0 + s1) : 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) { b[k] *= r; acc[k] += b[k]; }        // phi_kw * n_w (padded topics: exact zeros)
    if (act) {
        double* scol = slab + tcv.x;
#pragma unroll
        for (int k = 0; k < KP; ++k) unsafeAtomicAdd(&scol[k * V], b[k]);
    }
}

// SINGLE: the grid covers every document with one step per wave (no step loop: 46 VGPRs less -> 3 waves per SIMD)
// RB: batch build, replica blockIdx.y (rep())
template <int KP, int L, bool LL, int VT, bool SINGLE, bool RB = false>
__global__ __launch_bounds__(SINGLE ? kMaxWavesE * MMM_WAVE : 512, SINGLE ? 3 : 2) void k_lda_estep(EstepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int G = MMM_WAVE / L;                   // documents per wave step
    constexpr int PRE = (96 + L - 1) / L;             // chunks prefetched into registers (covers a 96-term document)
    MMM_STAMP(0);
    const int stop = EstepPass<RB>::stop_request(a);  // consumed after the first prologue; a vector load ahead of every other (lda_stop_request)
    const EstepPass<RB> io(a);
    const int K = a.c.K, D = a.c.D;
    const int V = VT ? VT : a.c.V;                    // VT != 0: row stride known at compile time (immediate LDS offsets)
    const int NW = blockDim.x >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane / L, l = lane % L;
    double* sB = smem;                                   // [KP][V] exp(Elnbeta_{t-1})
    double* sBeta = sB + (size_t)KP * V;                 // [KP][V] beta_{t-1}
    double* sSlab = sBeta + (size_t)KP * V;              // [NW][KP][V]
    double* sA = sSlab + (size_t)NW * KP * V;            // [NW][G][KP]
    double* sT = sA + (size_t)NW * G * KP;               // [NW][G][KP]
    double* slab = sSlab + (size_t)wid * KP * V;
    double* myA = sA + ((size_t)wid * G + g) * KP;
    double* myT = sT + ((size_t)wid * G + g) * KP;
    const int stride = gridDim.x * NW * G;
    int base = (blockIdx.x * NW + wid) * G;
    double ll_acc = 0.0;

    // ---- document loads of the first step are issued before the tables are staged (latency overlap) -------------
    int d = base + g;
    bool valid = d < D;
    // ext: this pass's prologue (digamma, exp: 2 us of this kernel's 10 at BASELINE config 2, all of it on every wave's dependent chain)
    // has run beside the previous pass's reduction, off the critical path; the same functions on the same lanes, hence the same bits
    const bool ext = SINGLE && !LL && !RB && a.aexp != nullptr;      // (batches have no merged launch, so no prologue formed ahead)
    double gk = ext ? ((valid && l < K) ? a.aexp[(size_t)d * K + l] : 0.0) : ((valid && l < K) ? io.gam[(size_t)d * K + l] : (l < K ? 1.0 : 0.0));
    double gp = (LL && valid && l < K) ? io.gprev[(size_t)d * K + l] : (l < K ? 1.0 : 0.0);
    // Single-step build over padded rows (c.ell: [D][V] (term,count), (-1,0) past the document's end): the document's pairs are
    // addressed by d alone, so their loads leave with the gamma row instead of a memory round trip later (doc_ptr -> tc), every
    // document has the same V / L chunks (static register indices, no per-step shuffles)
    const bool drows = V <= PRE * L && (a.c.dense != nullptr || a.c.dense16 != nullptr);      // rows of counts: term = slot, 4 or 2 bytes per slot
    const bool rows = drows || (V <= PRE * L && a.c.ell != nullptr);      // (the grid-stride build requests the next step's row a step ahead)
    int64_t start = (valid && !rows) ? a.c.doc_ptr[d] : 0;
    int W = (valid && !rows) ? (int)(a.c.doc_ptr[d + 1] - start) : 0;
    // SINGLE: the table stays in registers (<= 5 entries per thread: KP*V <= 12 * 96, >= 4 waves) until just before the barrier, so
    // that the prologue arithmetic below runs while these loads are in flight instead of after them
    constexpr int TB = KP <= 10 ? 4 : 5;
    double tb[TB];
    if (SINGLE) {
#pragma unroll
        for (int q = 0; q < TB; ++q) { const int i = tid + q * (int)blockDim.x; tb[q] = (i < K * V) ? io.eB[i] : 0.0; }
    }
    for (int i = tid; i < NW * KP * V; i += blockDim.x) sSlab[i] = 0.0;
    for (int i = tid; i < KP * V; i += blockDim.x) {
        if (!SINGLE) sB[i] = (i < K * V) ? io.eB[i] : 0.0;
        if (LL) sBeta[i] = (i < K * V) ? io.bprev[i] : 0.0;
    }
    MMM_STAMP(1);

    // Grid-stride build: a two-deep software pipeline over the wave's steps.  The CSR offsets of step i+2 and the (term,count)
    // pairs + gamma row of step i+1 are requested while step i computes, so that no step starts with the two dependent memory
    // round trips doc_ptr -> tc (at 160k-640k documents they were ~70 % of a step: the SIMDs ran at 30 % VALU utilisation).
    int d1 = 0; bool valid1 = false; int64_t start1 = 0; int W1 = 0;
    if (!SINGLE) {
        d1 = base + stride + g; valid1 = (base + stride < D) && d1 < D;
        start1 = (valid1 && !rows) ? a.c.doc_ptr[d1] : 0;
        W1 = (valid1 && !rows) ? (int)(a.c.doc_ptr[d1 + 1] - start1) : 0;
    }
    int2 tcp[PRE];                           // (term,count) of the first PRE chunks of the current step
    bool first = true;
    for (;;) {
        // ---- groups start at rotated chunks so that the G documents of a wave instruction touch different term ranges of the slab
        const int NCHR = VT ? (VT + L - 1) / L : (V + L - 1) / L;      // chunks of a padded row (<= PRE)
        const int nch = rows ? NCHR : (W + L - 1) / L;
        const int rot = nch > 0 ? g % nch : 0;
        const int2* __restrict__ tcd = a.c.tc + start;
        int nchmax = nch;
        if (!rows) {
            if (G >= 2) nchmax = max(nchmax, __shfl_xor(nchmax, 32, MMM_WAVE));
            if (G >= 4) nchmax = max(nchmax, __shfl_xor(nchmax, 16, MMM_WAVE));
            nchmax = __builtin_amdgcn_readfirstlane(nchmax);
        }
        // first step: loads issued before the prologue math (later steps: requested a step ahead)
        if (SINGLE || first) lda_row_read<L, PRE, true, true, true, true>(a.c, drows, rows, d, valid, l, V, nch, rot, start, W, [&](int j, int w, int n) { tcp[j] = make_int2(w, n); });
        // ---- Elntheta (LDA.jl:78-80), a_k = exp(Elntheta_k), theta_{t-1} (LDA.jl:92-94) ------------------------------
        double el = 0.0;
        if (ext) { if (l < KP) myA[l] = gk; }
        else {
            el = lda_elntheta<L>(gk, g, l, K);
            if (l < KP) myA[l] = (l < K) ? ar_exp(el) : 0.0;
        }
        if (LL) {
            const double Sp = group_sum<L>(gp);
            if (l < KP) myT[l] = (l < K) ? gp / Sp : 0.0;
        }
        if (first) {
            if (lda_stop_now(stop)) return;            // a previous pass met the stopping rule: this launch must not touch the state
            if (SINGLE) {
#pragma unroll
                for (int q = 0; q < TB; ++q) { const int i = tid + q * (int)blockDim.x; if (i < KP * V) sB[i] = tb[q]; }
                // (waves_per_block pinned below 4: the registers do not cover the table)
                for (int i = tid + TB * (int)blockDim.x; i < KP * V; i += blockDim.x) sB[i] = (i < K * V) ? io.eB[i] : 0.0;
            }
            __syncthreads();
            first = false;
            MMM_STAMP(2);
        } else lds_wave_sync();
        if (!ext && valid && l < K) io.Eln[(size_t)d * K + l] = el;
        MMM_STAMP(3);
        // ---- requests of the next two steps (grid-stride build) ---------------------------------------------------------
        int2 tcn[PRE];
        double gkn = 0.0, gpn = 0.0;
        int d2 = 0; bool valid2 = false; int64_t start2 = 0; int W2 = 0;
        const bool more = !SINGLE && base + stride < D;
        if (more) {
            const int nch1 = rows ? NCHR : (W1 + L - 1) / L;
            const int rot1 = nch1 > 0 ? g % nch1 : 0;
            lda_row_read<L, PRE, true, true, true, true>(a.c, drows, rows, d1, valid1, l, V, nch1, rot1, start1, W1, [&](int j, int w, int n) { tcn[j] = make_int2(w, n); });
            gkn = (valid1 && l < K) ? io.gam[(size_t)d1 * K + l] : (l < K ? 1.0 : 0.0);
            gpn = (LL && valid1 && l < K) ? io.gprev[(size_t)d1 * K + l] : (l < K ? 1.0 : 0.0);
            d2 = base + 2 * stride + g; valid2 = (base + 2 * stride < D) && d2 < D;
            start2 = (valid2 && !rows) ? a.c.doc_ptr[d2] : 0;
            W2 = (valid2 && !rows) ? (int)(a.c.doc_ptr[d2 + 1] - start2) : 0;
        }
        {
            double av[KP], acc[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) { av[k] = myA[k]; acc[k] = 0.0; }
            if (rows) {
#pragma unroll
                for (int j = 0; j < PRE; ++j) {
                    if (j < NCHR) {
                        int2 tcv = tcp[j];
                        const bool act = tcv.x >= 0;
                        tcv.x = act ? tcv.x : 0;
                        lda_chunk<KP, LL>(tcv, act, V, av, acc, sB, sBeta, myT, slab, ll_acc);
                    }
                }
            } else
#pragma unroll 2
            for (int j = 0; j < nchmax; ++j) {
                int2 tcv = tcp[0];
#pragma unroll
                for (int q = 1; q < PRE; ++q) tcv = (j == q) ? tcp[q] : tcv;     // register select (static indices only)
                if (j >= PRE) {
                    int c = j + rot; if (c >= nch) c -= nch;
                    const int w = c * L + l;
                    tcv = ((j < nch) && (w < W)) ? tcd[w] : make_int2(-1, 0);
                }
                const bool act = tcv.x >= 0;
                tcv.x = act ? tcv.x : 0;
                lda_chunk<KP, LL>(tcv, act, V, av, acc, sB, sBeta, myT, slab, ll_acc);
            }
            MMM_STAMP(4);
            // ---- gamma_{t+1} = alpha + sum_w phi_kw n_w (LDA.jl:83-87 of the next pass) ---------------------------
            double mine = 0.0;
#pragma unroll
            for (int k = 0; k < KP; ++k) { const double tot = group_sum<L>(acc[k]); if (l == k) mine = tot; }
            if (valid && l < K) io.gnext[(size_t)d * K + l] = a.c.alpha + mine;
        }
        MMM_STAMP(5);
        if (SINGLE) break;
        base += stride;
        if (base >= D) break;
        // ---- the next step's operands were requested above ------------------------------------------------------------
        d = d1; valid = valid1; gk = gkn; gp = gpn; start = start1; W = W1;
#pragma unroll
        for (int j = 0; j < PRE; ++j) tcp[j] = tcn[j];
        d1 = d2; valid1 = valid2; start1 = start2; W1 = W2;
        lds_wave_sync();
    }
    MMM_STAMP(6);
    // ---- block epilogue: slabs -> one partial; ll partial ------------------------------------------------------
    if (LL) ll_acc = wave_sum(ll_acc);
    __syncthreads();
    if (LL && lane == 0) sA[wid] = ll_acc;      // sA is free now
    double* out = EstepPass<RB>::partial(a, K);
    for (int i = tid; i < K * V; i += blockDim.x) {
        double v8[kMaxWavesE];
#pragma unroll
        for (int w = 0; w < kMaxWavesE; ++w) v8[w] = (w < NW) ? sSlab[(size_t)w * KP * V + i] : 0.0;
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kMaxWavesE; ++w) s += v8[w];
        out[a.pstride == V ? i : (i / V) * a.pstride + i % V] = s;
    }
    if (LL) {
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int w = 0; w < NW; ++w) s += sA[w];
            if constexpr (RB) a.llpart[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
            else a.llpart[blockIdx.x] = s;
        }
    }
    MMM_STAMP(7);
}


// ---- single-step E-step, statistics as a block product ------------------------------------------------------------------------------
// The single-step build of k_lda_estep without its slabs.  phi itself is never needed (k_lda_estep_dense): with s_dv = sum_k a_dk B_kv and
// r_dv = n_dv / s_dv,   gamma_dk = alpha + a_dk sum_v B_kv r_dv   and the block's statistics are   S_kv = B_kv sum_{d in block} a_dk r_dv,
// a (K x docs)(docs x V) product over the block's <= 48 documents.  So a term slot costs 2 KP fused multiply-adds and ONE plain 8-byte LDS
// store of r (no ds_add_f64, no per-wave slab, no slab zeroing, no ten-way slab sum), and after one block barrier thread (v, topic pair)
// sums a_dk r_dv over the block's documents in increasing d -- an order fixed by (waves per block, V, KP) alone -- and writes B_kv times
// it where the slab sums went.  The document groups start at chunk 0 (the rotation kept them off each other's slab entries): the four
// documents of a wave instruction read the same table addresses, which broadcast.
// A document that lists a term twice would write one sR cell twice: such corpora keep k_lda_estep (mmm_lda::block_stats, set at create).
// LDS: [KP / 2][V][2] table | [2 NW][16 ceil(V / 16)][2] r | [4 NW][KP] a.
// The table and r are held as PAIRS -- topics 2p, 2p + 1 of a term, documents 2p, 2p + 1 of a term slot, side by side in 16 bytes -- so that
// every read of either is one ds_read_b128 (a wave's costs 4 LDS-array cycles; the ds_read2_b64 the compiler formed of two rows a stride
// apart costs 8): a lane's term is KP / 2 reads whose 16 lanes cover 256 contiguous bytes, and the product takes two documents' r per read.
constexpr int lda_pair_cell(int i, int v, int stride) { return ((i >> 1) * stride + v) * 2 + (i & 1); }
constexpr int lda_tab_cell(int k, int v, int V) { return lda_pair_cell(k, v, V); }         // B_kv in sB
constexpr int lda_r_cell(int d, int v, int Vs) { return lda_pair_cell(d, v, Vs); }         // r_dv in sR (d: the document's number in the block)
// n rows (even) of `stride` cells: every (i, v) has a cell of its own inside the n * stride, and a pair starts on a 16-byte boundary
constexpr bool pair_cells_fill(int n, int stride)
{
    bool seen[48 * 96] = {};
    if (n % 2 || n * stride > 48 * 96) return false;
    for (int i = 0; i < n; ++i)
        for (int v = 0; v < stride; ++v) {
            const int c = lda_pair_cell(i, v, stride);
            if (c < 0 || c >= n * stride || seen[c]) return false;
            if (c != lda_pair_cell(i & ~1, v, stride) + (i & 1) || lda_pair_cell(i & ~1, v, stride) % 2) return false;
            seen[c] = true;
        }
    return true;
}
constexpr bool tab_cells_fill(int V) { for (int KP = 2; KP <= 12; KP += 2) if (!pair_cells_fill(KP, V)) return false; return true; }
constexpr bool r_cells_fill(int V) { for (int NW : {1, 2, 3, 4, 12}) if (!pair_cells_fill(4 * NW, (V + 15) & ~15)) return false; return true; }      // waves per block
static_assert(tab_cells_fill(5) && tab_cells_fill(50) && tab_cells_fill(96), "k_lda_estep_block's table: KP = 2 ... 12 topics as pairs");
static_assert(r_cells_fill(5), "k_lda_estep_block's r: 4, 8, 12, 16 and 48 documents as pairs");
static_assert(r_cells_fill(50), "k_lda_estep_block's r: 4, 8, 12, 16 and 48 documents as pairs");
static_assert(r_cells_fill(96), "k_lda_estep_block's r: 4, 8, 12, 16 and 48 documents as pairs");

template <int KP>
__device__ __forceinline__ double lda_chunk_r(const int v, const double n, const bool act, const int V, const double (&av)[KP], double (&acc)[KP],
                                              const double* __restrict__ sB)
{
    const double2* __restrict__ bcol = (const double2*)sB + v;      // lda_tab_cell(2 p, v, V) / 2 = p V + v
    double b[KP], s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k < KP; k += 2) { const double2 p = bcol[(k / 2) * V]; b[k] = p.x; b[k + 1] = p.y; }
#pragma unroll
    for (int k = 0; k + 1 < KP; k += 2) { s0 = fma(av[k], b[k], s0); s1 = fma(av[k + 1], b[k + 1], s1); }
    if (KP & 1) s0 = fma(av[KP - 1], b[KP - 1], s0);
    const double r = act ? n * dev_rcp(s0 + s1) : 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = fma(b[k], r, acc[k]);          // padded topics: B = 0
    return r;
}

// R16: the corpus is rows of 16-bit counts (the default form of a single fit).  A build of its own, so that the other forms' branches -- never
// taken over such a corpus -- do not share registers with its loads: the compiler priced the reuse of the row's address registers by the CSR
// branch's doc_ptr load as vmcnt(0) at the join, and the row was requested only after the table and a had arrived.
template <int KP, int VT, bool RB = false, bool R16 = false>
__global__ __launch_bounds__(kMaxWavesE * MMM_WAVE, 3) void k_lda_estep_block(EstepArgs a)
{
    static_assert(KP <= 12 && KP % 2 == 0, "topic pairs, table of <= 5 registers per thread");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int L = 16, G = MMM_WAVE / L, PRE = 96 / L;
    MMM_STAMP(0);
    // one round of scalar loads for every kernel argument the block uses (left alone the compiler fetches some of them where they are first used,
    // each a round of its own in front of the loads that follow it)
    asm volatile("" :: "s"(a.ctl), "s"(a.aexp), "s"(a.now.gam), "s"(a.now.gnext), "s"(a.now.Eln), "s"(a.now.eB), "s"(a.c.dense16), "s"(a.c.dense), "s"(a.c.ell),
                 "s"(a.c.doc_ptr), "s"(a.c.tc), "s"(a.c.Vp), "s"(a.c.D), "s"(a.c.K), "s"(a.c.V), "s"(a.c.alpha), "s"(a.partial), "s"(a.pstride), "s"((int)blockDim.x));
    const int stop = EstepPass<RB>::stop_request(a);  // consumed after the prologue; a vector load ahead of every other (lda_stop_request)
    const EstepPass<RB> io(a);
    const int K = a.c.K, D = a.c.D;
    const int V = VT ? VT : a.c.V;                    // VT != 0: row stride known at compile time (immediate LDS offsets)
    const int NCHR = VT ? (VT + L - 1) / L : (V + L - 1) / L;      // chunks of a row (<= PRE: the host takes this build for V <= 96 only)
    const int Vs = NCHR * L;                          // row stride of sR
    const int NW = blockDim.x >> 6, ND = NW * G;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane / L, l = lane % L;
    double* sB = smem;                                   // [KP / 2][V][2] exp(Elnbeta_{t-1}), lda_tab_cell
    double* sR = sB + (size_t)KP * V;                    // [ND / 2][Vs][2] r_dv = n_dv / sum_k a_dk B_kv (0: term absent, document past D), lda_r_cell
    double* sA = sR + (size_t)ND * Vs;                   // [ND][KP] a_dk
    double* myR = sR + lda_r_cell(wid * G + g, l, Vs);   // the document's r_v at myR[2 (v - l)]: the lane's own slots are immediates away
    double* myA = sA + (size_t)(wid * G + g) * KP;

    // ---- every start-up load leaves here, in one group behind the stop flag's: a (or gamma), the table, the document's row.  Unconditional,
    //      at clamped indices (document 0 for a lane past D, topic K - 1, entry K V - 1); the masks are applied where the values are used.  One
    //      trip to memory before the first barrier (k_lda_estep_dense: "what the dense-row kernels were actually waiting for", EXPERIMENTS.md)
    const int d = (blockIdx.x * NW + wid) * G + g;
    const bool valid = d < D;
    const int dl = valid ? d : 0;
    const bool ext = !RB && a.aexp != nullptr;      // the previous pass's merged launch has formed a = exp(Elntheta) (EstepArgs::aexp)
    const double* __restrict__ gsrc = ext ? a.aexp : io.gam;
    const double graw = gsrc[(size_t)dl * K + (l < K ? l : K - 1)];
    const bool drows = R16 || a.c.dense != nullptr || a.c.dense16 != nullptr;      // rows of counts: term = slot
    const bool rows = drows || a.c.ell != nullptr;
    constexpr int TB = KP <= 10 ? 4 : 5;            // the table stays in registers until just before the barrier (KP V <= 12 * 96, >= 4 waves; fewer waves: the loop below)
    double tb[TB];
#pragma unroll
    for (int q = 0; q < TB; ++q) { const int i = tid + q * (int)blockDim.x; tb[q] = io.eB[i < K * V ? i : K * V - 1]; }
    // (CSR's doc_ptr step after the table's loads: its lane-conditional loads end in a wait of their own, which the table's would stand behind)
    int64_t start = 0; int W = 0;
    if constexpr (!R16) {
        start = (valid && !rows) ? a.c.doc_ptr[d] : 0;
        W = (valid && !rows) ? (int)(a.c.doc_ptr[d + 1] - start) : 0;
    }
    unsigned w16[4] = {0u, 0u, 0u, 0u};
    if constexpr (R16) lda_row16_load(a.c, dl, l, w16);
    // (term,count) rows and CSR visit the listed terms only: every other r is the zero written here, before the barrier the stores come after
    if (!drows) for (int i = tid; i < ND * Vs; i += blockDim.x) sR[i] = 0.0;
    MMM_STAMP(1);

    int tv[PRE]; double tn[PRE];      // term slot (-1: none) and count of the lane's chunks
    const int nch = rows ? NCHR : (W + L - 1) / L;
    auto put = [&](int j, int w, int n) { tv[j] = w; tn[j] = (double)n; };
    if constexpr (R16) lda_row16_put<L, PRE, false, true>(w16, valid, l, V, nch, 0, put);
    else lda_row_read<L, PRE, false, true, true, true>(a.c, drows, rows, d, valid, l, V, nch, 0, start, W, put);
    const double gk = (valid && l < K) ? graw : ((ext || l >= K) ? 0.0 : 1.0);
    // ---- Elntheta (LDA.jl:78-80), a_k = exp(Elntheta_k) ------------------------------------------------------------------------------
    double el = 0.0, al = gk;        // al: the lane's own a_l
    if (!ext) {
        el = lda_elntheta<L>(gk, g, l, K);
        al = (l < K) ? ar_exp(el) : 0.0;
    }
    if (l < KP) myA[l] = al;
    if (lda_stop_now(stop)) return;            // a previous pass met the stopping rule: this launch must not touch the state
#pragma unroll
    for (int q = 0; q < TB; ++q) {
        const int i = tid + q * (int)blockDim.x, k = VT ? i / VT : i / V;      // entry i = k V + v of the topic-major table in memory
        if (i < KP * V) sB[lda_tab_cell(k, i - k * V, V)] = (i < K * V) ? tb[q] : 0.0;
    }
    for (int i = tid + TB * (int)blockDim.x; i < KP * V; i += blockDim.x) {      // (waves_per_block pinned below 4)
        const int k = VT ? i / VT : i / V;
        sB[lda_tab_cell(k, i - k * V, V)] = (i < K * V) ? io.eB[i] : 0.0;
    }
    __syncthreads();
    MMM_STAMP(2);
    if (!ext && valid && l < K) io.Eln[(size_t)d * K + l] = el;
    MMM_STAMP(3);
    // ---- chunk phase: r into sR, the gamma sums without their factor a_k ----------------------------------------------------------------
    double av[KP], acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) { av[k] = myA[k]; acc[k] = 0.0; }
    int nchmax = nch;
    if (!rows) {
        nchmax = max(nchmax, __shfl_xor(nchmax, 32, MMM_WAVE));
        nchmax = max(nchmax, __shfl_xor(nchmax, 16, MMM_WAVE));
        nchmax = __builtin_amdgcn_readfirstlane(nchmax);
    }
#pragma unroll
    for (int j = 0; j < PRE; ++j) {
        if (j < nchmax) {
            const bool act = tv[j] >= 0;
            const double r = lda_chunk_r<KP>(act ? tv[j] : 0, tn[j], act, V, av, acc, sB);
            if (drows) myR[2 * (j * L)] = r;           // every slot of the row, zeros included (slots past V are never read)
            else if (act) myR[2 * (tv[j] - l)] = r;
        }
    }
    MMM_STAMP(4);
    // ---- gamma_{t+1} = alpha + a_k sum_v B_kv r_v (LDA.jl:83-87 of the next pass) -----------------------------------------------------
    double mine = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) { const double tot = group_sum<L>(acc[k]); if (l == k) mine = tot; }
    if (valid && l < K) io.gnext[(size_t)d * K + l] = fma(al, mine, a.c.alpha);
    MMM_STAMP(5);
    // ---- block product: T_kv = sum_d a_dk r_dv in increasing d, S_kv = B_kv T_kv -> the block's partial ---------------------------------
    __syncthreads();
    MMM_STAMP(6);
    double* out = EstepPass<RB>::partial(a, K);
    for (int i = tid; i < (KP / 2) * V; i += blockDim.x) {
        const int kp = VT ? i / VT : i / V, v = i - kp * V, k = 2 * kp;
        const double2* __restrict__ rc = (const double2*)sR + v;      // lda_r_cell(2 p, v, Vs) / 2 = p Vs + v: documents 2 p, 2 p + 1
        const double* ac = sA + k;
        const double2 bb = ((const double2*)sB)[kp * V + v];          // lda_tab_cell(k, v, V) / 2: B_kv, B_(k+1)v
        double t0 = 0.0, t1 = 0.0;
#pragma unroll 2
        for (int dd = 0; dd < ND; dd += G) {
            double rr[G], a0[G], a1[G];
#pragma unroll
            for (int q = 0; q < G; q += 2) { const double2 p = rc[(size_t)((dd + q) >> 1) * Vs]; rr[q] = p.x; rr[q + 1] = p.y; }
#pragma unroll
            for (int q = 0; q < G; ++q) { a0[q] = ac[(dd + q) * KP]; a1[q] = ac[(dd + q) * KP + 1]; }
#pragma unroll
            for (int q = 0; q < G; ++q) { t0 = fma(a0[q], rr[q], t0); t1 = fma(a1[q], rr[q], t1); }
        }
        if (k < K) out[k * a.pstride + v] = bb.x * t0;
        if (k + 1 < K) out[(k + 1) * a.pstride + v] = bb.y * t1;
    }
    MMM_STAMP(7);
}


// ---- dense-row E-step (large corpora over a small vocabulary) ---------------------------------------------------------------------
// The corpora this model is used on are dense: mutation catalogues over the 96 SNV channels list nearly every channel in every sample
// (data/brca-eu_snv_counts.tsv: 53,559 of 53,760 entries).  For such a corpus the CSR sweep of k_lda_estep spends its time in LDS: per
// nonzero an 80-byte table column read and an 80-byte read-modify-write of the wave's slab (PMC: LDS pipe, not VALU, bounds the chunk
// loop).  Here a document is a row of Vp = 16 SL counts (zeros where a term is absent); lane l of a 16-lane document group owns the terms
// l, 16 + l, ..., the same ones in every document it meets, so the statistics sum_d phi_kv n_dv of its terms stay in REGISTERS for the
// whole launch (SL * KP doubles per lane) and reach the slab once, at the end.  Per term slot: a conflict-free 16-byte-per-lane read
// of the term-major table and 2 KP + 16 f64 instructions; no atomics in the loop.  HBM per document: 4 Vp bytes of counts instead of
// 8 bytes per nonzero.  Same formulas as k_lda_estep (LDA.jl:69-108); the sums are associated per lane, then lanes, waves, blocks.
template <class T> __device__ __forceinline__ T* at_byte(T* base, unsigned off) { return (T*)((char*)base + off); }   // uniform base + 32-bit lane offset: one VGPR per address
typedef unsigned short mmm_us2 __attribute__((ext_vector_type(2)));

template <int KP, int SL, bool C16, bool RB = false>
__global__ __launch_bounds__(512, 2) void k_lda_estep_dense(EstepArgs a, const int* __restrict__ cnt, const unsigned short* __restrict__ cnt16)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int L = 16, G = MMM_WAVE / L, Vp = L * SL;
    MMM_STAMP(0);
    const int t = a.t;
    const int stop = rep<RB>(a.ctl, 1)->stop;
    const double* __restrict__ gam = a.gamma.s[t % 3];
    double* __restrict__ gnext = a.gamma.s[(t + 1) % 3];
    double* __restrict__ Eln = a.Elntheta.s[t % 3];
    const double* __restrict__ eB = a.expElnbeta.s[(t + 2) % 3];
    if constexpr (RB) {
        const size_t KD = (size_t)a.c.K * a.c.D, VK = (size_t)a.c.V * a.c.K;
        gam = rep<RB>(gam, KD); gnext = rep<RB>(gnext, KD); Eln = rep<RB>(Eln, KD); eB = rep<RB>(eB, VK);
    }
    const int K = a.c.K, D = a.c.D, V = a.c.V;
    const int NW = blockDim.x >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane / L, l = lane % L;
    double* sT = smem;                                   // [Vp][KP] exp(Elnbeta_{t-1}), term-major; rows v >= V hold 1 (their counts are 0)
    double* sSlab = sT + (size_t)Vp * KP;                // [NW][Vp][KP], term-major like the table (written once, in the epilogue)
    double* sA = sSlab + (size_t)NW * Vp * KP;           // [NW][G][KP]
    double* sR = sA + (size_t)NW * G * KP;               // [NW][64][KP] gamma sums, lane-major
    double* slab = sSlab + (size_t)wid * Vp * KP;
    double* myA = sA + ((size_t)wid * G + g) * KP;
    double* myR = sR + (size_t)wid * MMM_WAVE * KP;
    const int stride = gridDim.x * NW * G;
    int base = (blockIdx.x * NW + wid) * G;
    // exp / log tables of the prologue (mmm_arith.h: ar_exp_tab, ar_digamma_pos_tab -- a third of this kernel's vector work is the K + 1
    // digammas and K exps per document; no division in exp, 20 instructions fewer in the log)
    __shared__ __attribute__((aligned(16))) double sTabs[MMM_EXPTAB_N + MMM_LOGTAB_N];
    for (int i = tid; i < MMM_EXPTAB_N + MMM_LOGTAB_N; i += blockDim.x) sTabs[i] = i < MMM_EXPTAB_N ? g_mmm_exptab[i] : g_mmm_logtab[i - MMM_EXPTAB_N];

    // The next step's gamma row and counts are requested a step ahead and must stay in flight across the step: nothing between a request and
    // its use may wait for memory (vmcnt counts in order, so ONE scratch reload in the loop waits for every load before it -- the build
    // that spilled 12 registers exposed the HBM round trip in every step: 640k documents 280 us at 53 % of its own issue time).  So: loads
    // are unconditional (a clamped document index; masks are applied when the values are used), 16-bit counts land in register halves
    // (SL / 2 registers), addresses are a uniform base + one 32-bit offset per lane (D K 8 and D Vp 4 bytes < 4 GB, checked at create).
    constexpr int NC = C16 ? (SL + 1) / 2 : SL;
    int d = base + g;
    bool valid = d < D;
    const int lk = l < K ? l : K - 1;
    unsigned dl = valid ? (unsigned)d : 0u;
    double gk = *at_byte(gam, (dl * (unsigned)K + lk) * 8u);
    gk = (valid && l < K) ? gk : (l < K ? 1.0 : 0.0);
    constexpr int SLs = C16 ? 2 * NC : SL;                  // slots a lane owns in a stored row
    unsigned c[NC], cn[NC];
    auto request = [&](unsigned* o, unsigned dd) {          // the lane's part of the row: NC consecutive 32-bit words, one load
        const unsigned* row = C16 ? at_byte((const unsigned*)cnt16, (dd * (unsigned)(16 * SLs) + l * SLs) * 2u)
                                  : at_byte((const unsigned*)cnt, (dd * (unsigned)(16 * SLs) + l * SLs) * 4u);
#pragma unroll
        for (int j = 0; j < NC; ++j) o[j] = row[j];
    };
    auto take = [&](const unsigned* raw, bool ok) {
#pragma unroll
        for (int j = 0; j < NC; ++j) c[j] = ok ? raw[j] : 0u;
    };
    request(cn, dl);
    take(cn, valid);
    for (int i = tid; i < Vp * KP; i += blockDim.x) {
        const int v = i / KP, k = i % KP;
        sT[i] = (k < K) ? (v < V ? eB[(size_t)k * V + v] : 1.0) : 0.0;
    }
    __syncthreads();          // the function tables are read by the first step's prologue
    double st[SL][KP];
#pragma unroll
    for (int q = 0; q < SL; ++q)
#pragma unroll
        for (int k = 0; k < KP; ++k) st[q][k] = 0.0;
    bool first = true;
    for (;;) {
        // ---- the next step's gamma row and counts are requested before this step's term phase
        const int dn = d + stride;
        const bool more = base + stride < D, validn = more && dn < D;
        const unsigned dnl = validn ? (unsigned)dn : dl;
        // ---- Elntheta (LDA.jl:78-80), a_k = exp(Elntheta_k)
        const double S = group_sum<L>(gk);
        const double ps = ar_digamma_pos_tab(l < K ? gk : S, sTabs + MMM_EXPTAB_N);        // lane K of the group holds psi(S)
        const double psS = __shfl(ps, g * L + K, MMM_WAVE);
        const double el = ps - psS;
        const double ak = (l < K) ? ar_exp_tab(el, sTabs) : 0.0;
        if (l < KP) myA[l] = ak;
        // (requested here, after the prologue: its polynomial constants overflow the scalar registers and one is reloaded from scratch in there)
        const double gkn = *at_byte(gam, (dnl * (unsigned)K + lk) * 8u);
        request(cn, dnl);
        if (first) {
            if (stop) return;            // a previous pass met the stopping rule: this launch must not touch the state
            __syncthreads();
            first = false;
            MMM_STAMP(1);
        } else lds_wave_sync();
        if (valid && l < K) *at_byte(Eln, (dl * (unsigned)K + l) * 8u) = el;
        double acc[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[k] = 0.0;
        // ---- phi_kv n_v (LDA.jl:92-106) for the lane's SL terms.  (Tried at K = 10, V = 96, 640k documents: a_k re-read from LDS in every slot,
        // no spilled register instead of 12: 330 vs 307 us; the next slot's table row requested a slot ahead, 62 spilled: 509 us.)
        double av[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) av[k] = myA[k];
#pragma unroll
        for (int q = 0; q < SL; ++q) {
            const double* tb = sT + (size_t)(q * L + l) * KP;
            // three fused multiply-adds per (term slot, topic): the normaliser s = sum_k a_k B_kv, the lane's gamma sums WITHOUT their factor
            // a_k (it is the document's, applied once after the lanes' sums have met) and the statistics WITHOUT their factor B_kv (it is
            // the term's, the same for every document, applied once when the registers reach the slab)
            double b[KP], s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int k = 0; k < KP; ++k) b[k] = tb[k];
#pragma unroll
            for (int k = 0; k + 1 < KP; k += 2) { s0 = fma(av[k], b[k], s0); s1 = fma(av[k + 1], b[k + 1], s1); }
            if (KP & 1) s0 = fma(av[KP - 1], b[KP - 1], s0);
            // a slot without mass must not see 0 x rcp(0) = NaN: with tiny priors the normaliser of a never-observed term underflows to 0.
            // (v_max with the smallest normal: the bits of every other quotient are unchanged; a select on the count costs 150 spilled registers here)
            const unsigned cq = C16 ? ((q & 1) ? c[q / 2] >> 16 : c[q / 2] & 0xffffu) : c[q];
            const double r = (double)cq * dev_rcp(dev_max_raw(s0 + s1, 2.2250738585072014e-308));
#pragma unroll
            for (int k = 0; k < KP; ++k) { acc[k] = fma(b[k], r, acc[k]); st[q][k] = fma(av[k], r, st[q][k]); }
            // one slot at a time, its statistics updated here (left alone the compiler sinks the SL KP updates to the end of the step and keeps
            // every slot's products alive until then: 190 spilled registers)
#pragma unroll
            for (int k = 0; k < KP; ++k) asm volatile("" : "+v"(st[q][k]));
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
        MMM_STAMP(2);
        // ---- the requested values are taken over HERE, before the step's last store: the compiler prices a wait for loads as if the
        // (lane-conditional) stores after them had not been issued, i.e. as vmcnt(0) -- placed after the gamma store below it waited for
        // that store's round trip in every step
        const bool valid_now = valid;
        const unsigned dl_now = dl;
        // (the empty statements are the first use of the loaded registers and cannot move above the term phase's own)
        double gk_next = gkn;
        asm volatile("" : "+v"(gk_next) :: "memory");
#pragma unroll
        for (int j = 0; j < NC; ++j) asm volatile("" : "+v"(cn[j]) :: "memory");
        gk_next = (validn && l < K) ? gk_next : (l < K ? 1.0 : 0.0);
        take(cn, validn);
#pragma unroll
        for (int j = 0; j < NC; ++j) asm volatile("" : "+v"(c[j]));
        __builtin_amdgcn_sched_barrier(0);
        // ---- gamma_{t+1} = alpha + sum_v phi_kv n_v: the lanes' sums meet in LDS, lane k of the group adds its column
#pragma unroll
        for (int k = 0; k < KP; ++k) myR[(size_t)lane * KP + k] = acc[k];
        lds_wave_sync();
        if (l < K) {
            const double* col = myR + (size_t)(g * L) * KP + l;
            double r0 = col[0], r1 = col[KP], r2 = col[2 * KP], r3 = col[3 * KP];
#pragma unroll
            for (int j = 4; j < L; j += 4) { r0 += col[j * KP]; r1 += col[(j + 1) * KP]; r2 += col[(j + 2) * KP]; r3 += col[(j + 3) * KP]; }
            if (valid_now) *at_byte(gnext, (dl_now * (unsigned)K + l) * 8u) = fma(ak, (r0 + r1) + (r2 + r3), a.c.alpha);
        }
        base += stride;
        if (base >= D) break;
        d = dn; valid = validn; dl = dnl; gk = gk_next;
        lds_wave_sync();
    }
    MMM_STAMP(3);
    // ---- the wave's statistics: the four document groups' registers are added across the rows of the wave (rows_sum4: (g0 + g2) + (g1 + g3),
    // no LDS), multiplied by the term's table entry once, and the first group's lanes store them -- the slab is term-major with padded
    // bounds like the table, written once (no zero fill, no read-modify-write; 16-byte pairs at compile-time offsets).  (One group at a
    // time through LDS with run-time bounds, every entry its own round trip: 19 of the 27 us of a 15k-document launch,
    // tools/diag_dense_stamps.py; batched per term slot: 6.4.)
#pragma unroll
    for (int q = 0; q < SL; ++q) {
        double* sl = slab + (size_t)(q * L + l) * KP;
        const double* tb = sT + (size_t)(q * L + l) * KP;
        double t[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) t[k] = rows_sum4(st[q][k]) * tb[k];
        if (g == 0) {
#pragma unroll
            for (int k = 0; k < KP; ++k) sl[k] = t[k];
        }
    }
    MMM_STAMP(4);
    __syncthreads();
    MMM_STAMP(5);
    double* out = a.partial + (size_t)blockIdx.x * K * a.pstride;
    if constexpr (RB) out += (size_t)blockIdx.y * gridDim.x * K * a.pstride;
    for (int i = tid; i < K * V; i += blockDim.x) {
        const int kk = i / V, v = i - kk * V;
        double s = 0.0;
        for (int w = 0; w < NW; ++w) s += sSlab[((size_t)w * Vp + v) * KP + kk];
        out[a.pstride == V ? i : kk * a.pstride + v] = s;
    }
    MMM_STAMP(6);
    MMM_STAMP(7);
}
