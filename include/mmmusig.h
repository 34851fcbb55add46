/*
 * mmmusig.h -- C ABI of libmmmusig_hip.so: the MI355X (gfx950) variational-EM backend that sits under the
 * MultiModalMuSig.jl API (LDA / ILDA / MMCTM / IMMCTM: fit!, the update_*! functions, transform, fit_heldout,
 * predict_modality_η, and the restart sweep of scripts/run_mmctm.jl as batched fits).
 *
 * The reference has no FFI: its hot path is reached by ordinary Julia dispatch.  Each entry point below
 * therefore names the Julia function (file:line under the reference's src/) whose work it replaces; the Julia
 * shim that `ccall`s them is multimodalmusig.jl_amd/julia/MultiModalMuSigHIP.jl.
 *
 * Conventions
 *   - plain C types only; every function returns an int status (0 = MMM_OK, negative = error);
 *     nothing throws across the ABI; mmm_last_error() returns the message of the last failure.
 *   - all reals are double; term ids are 0-based int32, counts int32, CSR offsets int64 (the shim converts
 *     the reference's 1-based Int64 `X[d][:,1]`).
 *   - host pointers in/out unless a name ends in `_dev`; the library copies inside the call and keeps no
 *     host pointer after return.  Model state lives in HBM between calls, owned by the handle.
 *   - one mmm_ctx per host thread / process = one GPU + one HIP stream (+ one RCCL rank when
 *     mmm_comm_init_rank has been called).  Calls on a ctx are serialised by the caller.
 *   - array layouts are exactly the reference's Julia (column-major) layouts flattened:
 *       LDA    lambda/Elnbeta/beta  V x K   [v + V*k]        (LDA.jl:8-10)
 *              gamma/Elntheta/theta K x D   [k + K*d]        (LDA.jl:13-15)
 *              phi   per doc K x W_d, docs concatenated      [K*doc_ptr[d] + k + K*w]   (LDA.jl:16)
 *       MMCTM  doc_ptr M*(D+1) absolute offsets into the modality-major concatenated term/count arrays
 *              lambda/nu/props MK x D [i + MK*d]; zeta M x D [m + M*d]
 *              gamma/Elnphi/phi [goff[m] + k*V[m] + v]
 *              theta [toff[m] + (e - doc_ptr[m*(D+1)])*K[m] + k]   (e = absolute entry index)
 *              mu MK; Sigma/invSigma MK x MK column-major
 *       IMMCTM features [foff[m] + i*V[m] + v] 0-based; gamma/Elnphi [goff[m] + k*SJ[m] + joff[m][i] + j]
 */
#ifndef MMMUSIG_H
#define MMMUSIG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMM_VERSION 123

enum {
    MMM_OK = 0,
    MMM_DEFERRED = 1,         /* mmm_ctx_destroy with live models: communicator and mailboxes released now, the rest with the last model */
    MMM_ERR_ARG = -1,         /* bad argument / inconsistent sizes                         */
    MMM_ERR_HIP = -2,         /* a HIP runtime call failed (message has hipGetErrorString) */
    MMM_ERR_RCCL = -3,        /* an RCCL call failed                                       */
    MMM_ERR_UNSUPPORTED = -4, /* shape outside what the kernels are built for              */
    MMM_ERR_NUMERIC = -5,     /* singular Sigma in the M-step                              */
    MMM_ERR_NO_DEVICE = -6    /* no gfx950 device visible                                  */
};

typedef struct mmm_ctx mmm_ctx;
typedef struct mmm_lda mmm_lda;
typedef struct mmm_ctm mmm_ctm;

/* ---- context ------------------------------------------------------------------------------------------ */
int mmm_version(void);
/* Create a context on HIP device `device_id` with its own non-blocking stream. */
int mmm_ctx_create(int device_id, mmm_ctx** out);
/* With models still alive on it (a garbage-collected host destroys in no particular order) the context gives up its communicator and
 * mailboxes at once and returns MMM_DEFERRED; stream and memory go with the last mmm_*_destroy.  Such models may be destroyed; if the
 * context had a communicator (nranks > 1) every other call on them returns MMM_ERR_ARG -- their sums would silently be rank-local. */
int mmm_ctx_destroy(mmm_ctx* ctx);
/* Message of the last error on this ctx (ctx == NULL: last error of a failed mmm_ctx_create). */
const char* mmm_last_error(const mmm_ctx* ctx);
int mmm_ctx_synchronize(mmm_ctx* ctx);
/* The hipStream_t every kernel of this ctx is launched on (for event timing by the caller). */
void* mmm_ctx_stream(mmm_ctx* ctx);
int mmm_ctx_device_name(mmm_ctx* ctx, char* buf, size_t n);

/* ---- run-time choices of the caller (SURVEY section 5 "Config / flags": a plain C struct across the ABI) -------------------------------
 * What a caller may legitimately choose -- which E-step build a handle takes, a PINNED launch geometry, the side stream -- travels here,
 * not in environment variables: mmm_ctx_set_tuning stores the options on the context and every handle CREATED afterwards keeps its own
 * copy (two handles of one process may differ).  0 in a field = the library decides.  The all-reduce transport is chosen separately
 * (mmm_p2p_enable).  The only environment variables the library still reads concern the transport set-up: MMM_P2P, MMM_P2P_TIMEOUT_S,
 * MMM_P2P_ONE_RANK, MMM_FORCE_RCCL. */
enum { MMM_BUILD_AUTO = 0,
       MMM_BUILD_SPARSE = 1,   /* sweep the CSR arrays / padded rows through the LDS tables (any corpus)                              */
       MMM_BUILD_DENSE = 2,    /* rows of counts, statistics in registers (dense corpora; falls back when the shape has no such build) */
       MMM_BUILD_WIDE = 3 };   /* topic tables through L2 instead of LDS, term-major statistics sweep (large vocabularies)             */
enum { /* mmm_tuning_opts.disable: optimisations a test or an A/B run may switch off, one bit each (results are unchanged unless noted) */
    MMM_OFF_LDA_PADDED_ROWS = 1 << 0,   /* single-step E-step build: fetch (term, count) through doc_ptr instead of padded rows                  */
    MMM_OFF_LDA_COUNT_ROWS = 1 << 1,    /* dense corpora: keep (term, count) rows instead of rows of counts                                        */
    MMM_OFF_LDA_ROWS16 = 1 << 2,        /* rows of int32 instead of 16-bit counts                                                                  */
    MMM_OFF_LDA_LL_JOIN = 1 << 3,       /* reduce blocks do not join the log-likelihood sweep of the merged launch                                 */
    MMM_OFF_LDA_MERGED = 1 << 4,        /* reduce, ll and M-step as separate launches instead of k_lda_reduce_ll_mstep                             */
    MMM_OFF_P2P_FOLDED = 1 << 5,        /* several GPUs: the mailbox exchange as its own launch instead of folded into the reduce / M-step blocks */
    MMM_OFF_CTM_PACKED = 1 << 6,        /* solve phase: no packed document groups (sum K = 6 / 10 / 12 lanes per document)                         */
    MMM_OFF_CTM_CPL = 1 << 7,           /* solve phase: one coordinate per lane everywhere (no several-coordinates-per-lane builds)                */
    MMM_OFF_CTM_KFIT = 1 << 8,          /* theta phase: 16-wide topic loops for every shape                                                        */
    MMM_OFF_CTM_FUSED_GAUSS = 1 << 9,   /* Gaussian M-step as its own launch instead of block 0 of the log-likelihood launch                       */
    MMM_OFF_CTM_LL_ROWS = 1 << 10,      /* handles with rows of counts: props / log-likelihood sweep over the CSR arrays                           */
    MMM_OFF_LDA_EARLY_PROLOGUE = 1 << 11, /* single-step E-step build: every pass forms its own Elntheta / exp(Elntheta) instead of the previous pass's merged launch */
    MMM_OFF_CTM_PIPE_GAUSS = 1 << 12,    /* Gaussian M-step: the three-barrier-per-column inversion instead of the pipelined one (sum K <= 32); same bits         */
    MMM_OFF_CTM_SOLVE_ORDER = 1 << 13,   /* solve phase: a wave's slots take its documents in index order instead of longest-lambda-solve-of-the-previous-pass first; same bits */
    MMM_OFF_LDA_BLOCK_STATS = 1 << 14,   /* single-step E-step build: per-wave LDS slabs filled by ds_add_f64 (k_lda_estep) instead of the block product of k_lda_estep_block */
    MMM_OFF_REFIT_LDS = 1 << 15,         /* mmm_refit_exposures, mmm_presence_test / _power, mmm_attribute_mutations: read the catalogue through L2 even where it (an item's rows) fits LDS; same bits       */
    MMM_OFF_DECOMPOSE_LDS = 1 << 16,     /* mmm_decompose_search, mmm_signature_decompose: read G and b through L2 even where they fit LDS; same bits                        */
    MMM_OFF_ALL = (1 << 17) - 1          /* every bit this build knows; mmm_ctx_set_tuning rejects others (and non-zero reserved fields) with MMM_ERR_ARG */
};
typedef struct {
    int lda_build;        /* MMM_BUILD_*: E-step build of LDA / ILDA handles                                                              */
    int ctm_build;        /* MMM_BUILD_*: theta phase of the fused pass of MMCTM / IMMCTM handles                                         */
    int geometry_cus;     /* > 0: size every launch whose block count fixes the association of a cross-document sum (and so the bits of  */
                          /* a fit) as if the device had this many CUs -- the same value gives the same bits on any gfx950 device or     */
                          /* partition mode (256 = an MI355X in SPX mode).  0: the device's own CU count.                                */
    int grid_blocks;      /* > 0: that many blocks for the E-step kernel (LDA: forces the grid-stride build) / the theta phase (CTM)      */
    int waves_per_block;  /* > 0: waves per block of the LDA E-step kernel                                                                */
    int moment_blocks;    /* > 0: blocks of the CTM moment sums                                                                           */
    int side_stream;      /* CTM fit passes on one GPU: -1 never, 0 library's choice (IMMCTM only), 1 whenever possible                   */
    int resident_cap;     /* > 0: lowers the residency bound of the merged LDA launch (tests of the fallback)                             */
    unsigned disable;     /* MMM_OFF_* bits                                                                                               */
    int solve_lanes;      /* CTM solve phase: lanes per document, 0 = the library's choice by shape and corpus size (mmm_ctm_geometry out[5]); */
                          /* sum K = 10: 2 (x 5 coordinates) or 8 (x 2); sum K = 28: 16 (x 2) or 32 (x 1).  The layouts associate a document's  */
                          /* sums differently (sum K = 10) -- the value pins the bits across corpus sizes                                   */
    int solve_waves;      /* > 0: persistent solve kernels run with this many waves per SIMD (1..8) instead of the library's choice           */
    int reserved[5];      /* 0                                                                                                            */
} mmm_tuning_opts;
void mmm_tuning_opts_default(mmm_tuning_opts* o);
/* opts == NULL: back to the defaults.  Applies to handles created on ctx from now on. */
int mmm_ctx_set_tuning(mmm_ctx* ctx, const mmm_tuning_opts* opts);
int mmm_ctx_get_tuning(const mmm_ctx* ctx, mmm_tuning_opts* out);
/* HIP-event timing of the dominant kernel of the hot path (the fused E-step kernel) on the ctx stream: between
 * begin and end every launch of it is bracketed by an event pair; end synchronises and returns the number of
 * launches and the sum of their durations in milliseconds. */
int mmm_ctx_profile_begin(mmm_ctx* ctx);
/* repeat = 2: every profiled span holds the (idempotent) LDA E-step kernel twice; the difference of the spans measured with
 * repeat 2 and repeat 1 is the kernel's duration without the ~4 us that an event pair adds around a single launch. */
int mmm_ctx_profile_repeat(mmm_ctx* ctx, int repeat);
/* which launches the spans bracket: 0 (default) the dominant kernel; LDA 1 = everything of a pass after the E-step kernel
 * (reduction, ll sweep, M-step); CTM 1 = theta phase, 2 = moments + reduction + M-step, 3 = props / log-likelihood launches;
 * Lets bench.py account for the whole iteration kernel by kernel (its `iteration` block). */
int mmm_ctx_profile_select(mmm_ctx* ctx, int phase);
/* phase 8 brackets every phase at once; mmm_ctx_profile_end_phases then returns span counts and summed durations per phase (0..7).  For
 * passes of milliseconds (CTM), where the few microseconds an event pair adds do not matter. */
int mmm_ctx_profile_end_phases(mmm_ctx* ctx, int n_spans[8], double total_ms[8]);
int mmm_ctx_profile_end(mmm_ctx* ctx, int* n_launches, double* total_ms);

/* ---- multi-GPU: documents are sharded across ranks, sufficient statistics are all-reduced (RCCL) ---------
 * (no counterpart in the reference, which is single-threaded; replaces the doc loops' cross-document sums
 *  LDA.jl:103-105, MMCTM.jl:201,205-210,230-240 and the log-likelihood sums).
 * With a communicator on ctx, every model call that produces or consumes a cross-document sum is COLLECTIVE: all ranks make
 * the same calls on their handles in the same order -- *_create, *_iterate, *_fit, *_infer, the update_* stages, *_loglik,
 * *_elbo, and *_ll_history / *_set (they complete the last pass's pending log-likelihood first).  *_get and *_destroy are
 * local. */
#define MMM_UNIQUE_ID_BYTES 128
int mmm_comm_unique_id(char out[MMM_UNIQUE_ID_BYTES]);                 /* rank 0: ncclGetUniqueId   */
int mmm_comm_init_rank(mmm_ctx* ctx, int nranks, int rank, const char id[MMM_UNIQUE_ID_BYTES]);
int mmm_comm_nranks(const mmm_ctx* ctx);
/* The all-reduce transport.  The payload is 1-20 KB once per iteration, so latency decides: after mmm_comm_init_rank the
 * library all-reduces through per-rank MAILBOXES in fine-grained device memory that the peers write directly over xGMI
 * (one kernel per call, sums in rank order: same bits on every rank), provided the IPC mappings could be made and a
 * known-answer rehearsal passed on every rank; otherwise, and for payloads above the mailbox capacity, ncclAllReduce.
 * MMM_P2P=0 in the environment keeps RCCL.  mmm_comm_transport: "p2p", "rccl" or "none".
 * The mailbox path can also be set up without RCCL: every rank calls mmm_p2p_local_handle, the host exchanges the
 * handles (nranks x MMM_P2P_HANDLE_BYTES, rank-major), every rank calls mmm_p2p_attach and mmm_p2p_selftest, and all
 * ranks call mmm_p2p_enable(ctx, 0) unless every rank's rehearsal passed. */
#define MMM_P2P_HANDLE_BYTES 64
const char* mmm_comm_transport(const mmm_ctx* ctx);
int mmm_p2p_local_handle(mmm_ctx* ctx, int nranks, char out[MMM_P2P_HANDLE_BYTES]);
int mmm_p2p_attach(mmm_ctx* ctx, int nranks, int rank, const char* handles);
int mmm_p2p_selftest(mmm_ctx* ctx, int* ok);
int mmm_p2p_enable(mmm_ctx* ctx, int on);

/* ---- LDA (src/LDA.jl) ----------------------------------------------------------------------------------- */
enum { /* field ids for mmm_lda_get / mmm_lda_set; sizes in doubles */
    MMM_LDA_LAMBDA = 0,   /* V*K  */
    MMM_LDA_ELNBETA = 1,  /* V*K  */
    MMM_LDA_BETA = 2,     /* V*K  */
    MMM_LDA_GAMMA = 3,    /* K*D  */
    MMM_LDA_ELNTHETA = 4, /* K*D  */
    MMM_LDA_THETA = 5,    /* K*D  */
    MMM_LDA_PHI = 6,      /* K*nnz */
    /* ILDA handles (mmm_ilda_create): the factor arrays of ILDA.jl:6-9, lambda[i] J_i x K column-major at K*sum_{q<i} J_q;
     * for such handles ELNBETA / BETA above are the effective V x K tables sum_i Elnβ[i][f_vi,k] / prod_i β[i][f_vi,k] */
    MMM_ILDA_LAMBDA = 7, MMM_ILDA_ELNBETA = 8, MMM_ILDA_BETA = 9      /* sum(J)*K */
};
/* Constructor LDA(k, alpha, eta, V, X) -- LDA.jl:24-54.  lambda0 (V*K) is the random init the shim draws with
 * rand(1:100, V, K) (LDA.jl:36); the ctor state gamma=1, phi=1/K, Elnbeta, Elntheta is built on the GPU.
 * With an RCCL communicator on ctx, (D, doc_ptr, term, count) is THIS RANK'S shard of the documents.
 * Shapes: any V; K <= 256 (tuned builds to 32 topics, rolled-loop kernels beyond); MMM_ERR_UNSUPPORTED otherwise -- the reference has no limit. */
int mmm_lda_create(mmm_ctx* ctx, int D, int V, int K, double alpha, double eta, const int64_t* doc_ptr,
                   const int32_t* term, const int32_t* count, const double* lambda0, mmm_lda** out);
/* Constructor ILDA(k, alpha, eta::Vector, features, X) -- ILDA.jl:25-56: the topic-term distribution factorises over the I
 * features of a term (features: [i*V + v], 0-based values < J[i]).  lambda0: rand(1:100, J_i, K) per feature (ILDA.jl:36).
 * The handle is an mmm_lda: every mmm_lda_* entry point works on it (update_ϕ!/γ!/λ!/β! ILDA.jl:65-130, ll :203-239,
 * ELBO :132-201 -- including the reference's ElnQβ, which keeps only the last feature's term, :175-182 --, fit! :246-272,
 * and the frozen-topic passes of fit_heldout :320-353). */
int mmm_ilda_create(mmm_ctx* ctx, int D, int V, int K, double alpha, int I, const int* J, const double* eta,
                    const int32_t* features, const int64_t* doc_ptr, const int32_t* term, const int32_t* count,
                    const double* lambda0, mmm_lda** out);
int mmm_lda_destroy(mmm_lda* m);
int mmm_lda_get(mmm_lda* m, int field, double* host, size_t n);
int mmm_lda_set(mmm_lda* m, int field, const double* host, size_t n);
/* The hyper-parameters are plain mutable fields upstream (`model.α = 0.5; fit!(model)`, LDA.jl:2-12 / ILDA.jl:2-12): alpha, and eta as
 * n_eta = 1 value (LDA) or one per feature (ILDA).  Takes effect from the next update_γ! / update_λ! on. */
int mmm_lda_set_hyper(mmm_lda* m, double alpha, const double* eta, int n_eta);
/* One-to-one GPU counterparts of the reference's update functions (stage API; used by the parity tests) */
int mmm_lda_update_gamma(mmm_lda* m);   /* update_γ!  LDA.jl:82-90  (+ update_Elnθ! :78-80)  */
int mmm_lda_update_phi(mmm_lda* m);     /* update_ϕ!  LDA.jl:69-76                           */
int mmm_lda_update_lambda(mmm_lda* m);  /* update_λ!  LDA.jl:100-108 (+ update_Elnβ! :96-98) */
int mmm_lda_update_beta(mmm_lda* m);    /* update_β!  LDA.jl:110-112                         */
int mmm_lda_update_Elntheta(mmm_lda* m);/* update_Elnθ! alone  LDA.jl:78-80   (the reference calls it at the end of update_γ!) */
int mmm_lda_update_Elnbeta(mmm_lda* m); /* update_Elnβ! alone  LDA.jl:96-98 / ILDA.jl:96-101 (... at the end of update_λ!)    */
int mmm_lda_update_theta(mmm_lda* m);   /* update_θ!  LDA.jl:92-94                           */
int mmm_lda_loglik(mmm_lda* m, double* ll);                    /* calculate_loglikelihood LDA.jl:174-196 */
int mmm_lda_elbo(mmm_lda* m, double* elbo, double terms[7]);   /* calculate_elbo LDA.jl:114-172          */
/* Fused hot path: n_iter passes of { update_γ!; update_ϕ!; update_λ!; update_β!; update_θ!; ll } (the body of
 * fit!, LDA.jl:201-209) enqueued on the ctx stream without host synchronisation.  ll of pass i is written
 * to an internal device history; read it with mmm_lda_ll_history. */
int mmm_lda_iterate(mmm_lda* m, int n_iter);
int mmm_lda_ll_history(mmm_lda* m, double* ll, int max_n, int* n);
/* Which E-step build the handle uses and its launch geometry (diagnostics, tests): out[0] = lanes per document, [1] = blocks,
 * [2] = waves per block, [3] = 1 for the single-step build (small corpora: the grid covers every document at once), [4] = 1 for
 * the wide-table path (tables beyond LDS), [5] = 1 for the dense-row build (dense corpus over <= 128 terms: rows of counts,
 * statistics accumulated in registers; 2: its 32-lane variant), [6] = its term slots per lane, [7] = topics padded to. */
int mmm_lda_geometry(const mmm_lda* m, int out[8]);
/* Bytes of corpus the E-step build reads per document when the handle keeps rows (rows of 16- or 32-bit counts: 2 or 4 bytes x 16 x
 * slots per lane; padded (term,count) rows: 8 x V); 0 when it sweeps the CSR arrays (8 bytes per nonzero + offsets).  bench.py's
 * "algorithmic bytes as implemented". */
int mmm_lda_row_bytes(const mmm_lda* m);
/* 1 once fused passes of this handle have formed the NEXT pass's Elntheta / exp(Elntheta) inside their merged launch (single-step build: the
 * E-step kernel of every pass but the first of a call then reads exp(Elntheta) and writes gamma only -- bench.py counts its bytes
 * accordingly), else 0. */
int mmm_lda_prologue_moved(const mmm_lda* m);
/* How the single-step E-step build forms a block's lambda statistics: 1 = as a block product B_kv sum_d a_dk r_dv (k_lda_estep_block), 0 = per-wave
 * LDS slabs (k_lda_estep: MMM_OFF_LDA_BLOCK_STATS, a corpus in which a document lists a term twice, or not the single-step build at all). */
int mmm_lda_stats_build(const mmm_lda* m);
/* Which launches the last training pass enqueued on this handle took (mmm_lda_iterate / mmm_lda_fit; 0 before the first), as MMM_PASS_* bits:
 * MERGED = reduction, ll sweep and M-step in one launch, SPLIT = the reduce launch and k_lda_mstep, WIDE = the term sweep and
 * k_lda_mstep_wide (BIG: its build for more than 32 topics); P2P = the ranks' exchange rode inside those launches (mailboxes), otherwise a
 * communicating context all-reduced between them; LL_JOIN = the reduce blocks joined the ll sweep; PACKED = two logical reduce blocks per
 * block; LL_CELLS = the ll blocks handed their sums to the reduce blocks through cells (exchange not folded). */
enum { MMM_PASS_MERGED = 1, MMM_PASS_SPLIT = 2, MMM_PASS_WIDE = 4, MMM_PASS_P2P = 8, MMM_PASS_LL_JOIN = 16, MMM_PASS_PACKED = 32,
       MMM_PASS_LL_CELLS = 64, MMM_PASS_BIG = 128 };
int mmm_lda_last_pass(const mmm_lda* m);
/* Blocks of that pass's launch that wait for each other -- the merged launch's reduce and ll blocks, or (LL_CELLS) the reduce launch's -- and so
 * must be resident together; with the exchange folded in they also wait for the peers' blocks.  0 when no block of the pass waits for another. */
int mmm_lda_last_pass_blocks(const mmm_lda* m);
/* fit!(model; maxiter, tol) -- LDA.jl:198-224: iterate until |dll|/|ll| < tol after > 10 passes, then ELBO. */
int mmm_lda_fit(mmm_lda* m, int maxiter, double tol, double* ll_hist, int* n_iter, int* converged,
                double* elbo);
/* Frozen-topic inference on a model whose topics were uploaded with mmm_lda_set: the loop of
 * transform(model, X) LDA.jl:233-263 (unsmoothed = 1: unsmoothed_update_ϕ!, phi ∝ exp(Elnθ)·β, needs BETA) or of
 * fit_heldout(Xheldout, model) LDA.jl:265-295 (unsmoothed = 0: update_ϕ! with Elnβ, needs ELNBETA and BETA):
 * { update_γ!; (unsmoothed_)update_ϕ!; update_θ!; ll } until the stopping rule fires after > 10 passes.  Topics are
 * not touched; γ, Elnθ, θ, ϕ of the handle's documents are the result. */
int mmm_lda_infer(mmm_lda* m, int unsmoothed, int maxiter, double tol, double* ll_hist, int* n_iter,
                  int* converged);

/* LDA restart batching -- LDA's constructor draws its topics at random (rand(1:100, V, K), LDA.jl:36), so users run several restarts
 * and keep the best.  A batch handle holds R >= 1 LDA models ("replicas") over ONE resident corpus; replica r is created from
 * lambda0[r] (R contiguous V*K blocks, each as in mmm_lda_create).  The batched fit advances all replicas with one launch per kernel
 * (replica on grid.y) of the split pipeline: the E-step build of the shape, the reduction with its ll blocks, the M-step with its pass
 * tail.  Contract:
 *   - replica r computes, bit for bit, what a single handle created from lambda0[r] computes under the same mmm_tuning_opts plus
 *     MMM_OFF_LDA_MERGED over a whole fit!: ll history, pass count, converged, ELBO and every field;
 *   - its bits do not depend on R or on the other replicas: the launch geometry that fixes the order of the sums comes from D (and
 *     geometry_cus) alone;
 *   - each replica stops by its own rule (LDA.jl:215 + common.jl:53-56, evaluated on the device as in the single fit); later passes
 *     are no-ops for it.  The batch ends when every replica has stopped or after maxiter passes.
 * R = 1 is exactly mmm_lda_create (merged launch included).  MMM_ERR_UNSUPPORTED, with the limit in the message, for R > 1 on shapes
 * whose single handle takes the wide path (lda_build = MMM_BUILD_WIDE, K >= 25 under MMM_BUILD_AUTO, tables beyond LDS) and on a
 * context with a communicator (deal restarts over ranks on the host); MMM_ERR_ARG for R < 1.  ILDA has no batches
 * (mmm_lda_fit_batch on an ILDA handle: MMM_ERR_UNSUPPORTED).
 * On a handle with R > 1: mmm_lda_get (every field), mmm_lda_ll_history, mmm_lda_elbo and mmm_lda_events act on the selected replica
 * (0 after create; theta and phi are one buffer, formed for it on demand); mmm_lda_geometry and mmm_lda_destroy work as on any
 * handle; set, set_hyper, the update_* stages, loglik, iterate, fit and infer return MMM_ERR_UNSUPPORTED and leave the handle as it was. */
int mmm_lda_create_batch(mmm_ctx* ctx, int R, int D, int V, int K, double alpha, double eta, const int64_t* doc_ptr,
                         const int32_t* term, const int32_t* count, const double* lambda0, mmm_lda** out);
int mmm_lda_replicas(const mmm_lda* m);
int mmm_lda_select(mmm_lda* m, int r);
/* fit! of every replica.  ll_hist: [R][maxiter] (replica-major, n_iter[r] values each) or NULL; n_iter, converged: [R]; elbo: [R] or
 * NULL.  Replicas that reach maxiter get mmm_lda_fit's final convergence test.  All replicas must stand at the same pass (a fresh
 * batch, or one whose earlier fit ran every replica to maxiter). */
int mmm_lda_fit_batch(mmm_lda* m, int maxiter, double tol, double* ll_hist, int* n_iter, int* converged, double* elbo);

/* ---- MMCTM (src/MMCTM.jl) and IMMCTM (src/IMMCTM.jl) -------------------------------------------------------- */
typedef struct {
    double xtol_rel;     /* 1e-4   MMCTM.jl:129,158 */
    double xtol_abs;     /* 1e-4   MMCTM.jl:130,159 */
    double nu_lower;     /* 1e-7   MMCTM.jl:157     */
    int xtol_rule;       /* 0: NLopt >= 2.7 stopping rule, 1: NLopt <= 2.6 (Project.toml:15 allows both) */
    int max_eval;        /* safety cap on objective evaluations per MMA solve (NLopt: unlimited); 0 -> 2000 */
} mmm_solver_opts;
void mmm_solver_opts_default(mmm_solver_opts* o);

enum { /* field ids for mmm_ctm_get / mmm_ctm_set */
    MMM_CTM_MU = 0, MMM_CTM_SIGMA = 1, MMM_CTM_INVSIGMA = 2, MMM_CTM_GAMMA = 3, MMM_CTM_ELNPHI = 4,
    MMM_CTM_PHI = 5, MMM_CTM_LAMBDA = 6, MMM_CTM_NU = 7, MMM_CTM_ZETA = 8, MMM_CTM_PROPS = 9,
    MMM_CTM_THETA = 10, MMM_CTM_ALPHA = 11
};
/* Constructor MMCTM(k, alpha, V, X) -- MMCTM.jl:29-91 (init = :random; gamma0 is the rand(1:100, V[m]) draw per
 * topic, MMCTM.jl:60-63).  n_feat/J/features == NULL: MMCTM.  Otherwise IMMCTM(k, alpha, features, X) --
 * IMMCTM.jl:29-78 with alpha of length sum_m I[m] and gamma0 in the IMMCTM layout.
 * Shapes: any V[m]; M <= 8; K[m] <= 64; sum K <= 256 (tuned kernels to sum K = 64 with K[m] <= 32, generic ones beyond);
 * MMM_ERR_UNSUPPORTED otherwise -- the reference has no limit. */
int mmm_ctm_create(mmm_ctx* ctx, int D, int M, const int* K, const int* V, const double* alpha,
                   const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const int* n_feat,
                   const int* J, const int32_t* features, const double* gamma0, const mmm_solver_opts* opts,
                   mmm_ctm** out);
int mmm_ctm_destroy(mmm_ctm* m);
int mmm_ctm_get(mmm_ctm* m, int field, double* host, size_t n);
int mmm_ctm_set(mmm_ctm* m, int field, const double* host, size_t n);
/* stage API (GPU counterparts of the reference's per-document and M-step functions) */
int mmm_ctm_update_zeta(mmm_ctm* m);    /* update_ζ! for every doc      MMCTM.jl:172-181              */
int mmm_ctm_update_theta(mmm_ctm* m);   /* update_θ! for every doc      MMCTM.jl:183-198 / IMMCTM.jl:152-172 */
int mmm_ctm_update_nu(mmm_ctm* m);      /* update_ν! for every doc      MMCTM.jl:156-170 (LD_MMA)     */
int mmm_ctm_update_lambda(mmm_ctm* m);  /* update_λ! for every doc      MMCTM.jl:127-143 (LD_MMA)     */
int mmm_ctm_update_mu(mmm_ctm* m);      /* update_μ!                    MMCTM.jl:200-202              */
int mmm_ctm_update_Sigma(mmm_ctm* m);   /* update_Σ!                    MMCTM.jl:204-212              */
int mmm_ctm_update_gamma(mmm_ctm* m);   /* update_γ! (+ update_Elnϕ!)   MMCTM.jl:224-242,214-222      */
int mmm_ctm_update_Elnphi(mmm_ctm* m);  /* update_Elnϕ!                 MMCTM.jl:214-222 / IMMCTM.jl:188-197 */
int mmm_ctm_update_alpha(mmm_ctm* m);   /* update_α! (1-D LD_MMA per α) MMCTM.jl:252-269, IMMCTM.jl:225-244 */
int mmm_ctm_update_props(mmm_ctm* m);   /* update_props!                MMCTM.jl:145-154              */
int mmm_ctm_update_phi(mmm_ctm* m);     /* update_ϕ!                    MMCTM.jl:244-250              */
/* The reference's per-document functions take the document: update_ζ!(model, d), update_θ!(model, d), update_ν!(model, d),
 * update_λ!(model, d), fitdoc!(model, d) (MMCTM.jl:127-198, 450-455; test/mmctm.jl:92-199 call them that way).
 * mmm_ctm_update_docs runs a stage on the n documents docs[0..n) (0-based ids of this rank's shard, distinct, any order) of the selected
 * replica.  MMM_STAGE_FITDOC = ζ, θ, ν, λ in that order, one wait.  Every listed document gets, bit for bit, what the whole-corpus stage
 * call(s) write for it on this handle (λ, ν, ζ, θ, sumθ, its evaluation counters); every other document keeps its values and counters.
 * Device work is the listed documents' (plus an O(n) upload of the list; theta of the replica is formed first if it is held implicitly).
 * MMM_ERR_ARG, before anything runs and with nothing changed: unknown stage, n < 0, docs == NULL with n > 0, an id outside [0, D), an id
 * listed twice.  n == 0: nothing.  Not collective.  mmm_ctm_update_doc(m, stage, d) = mmm_ctm_update_docs(m, stage, &d, 1). */
enum { MMM_STAGE_ZETA = 0, MMM_STAGE_THETA = 1, MMM_STAGE_NU = 2, MMM_STAGE_LAMBDA = 3, MMM_STAGE_FITDOC = 4 };
int mmm_ctm_update_docs(mmm_ctm* m, int stage, const int32_t* docs, int n);
int mmm_ctm_update_doc(mmm_ctm* m, int stage, int d);
/* Document d's part of a per-document field of the selected replica, without a whole-field transfer: MMM_CTM_LAMBDA, _NU, _PROPS (sum K
 * values), _ZETA (M), _THETA (the K_m x W_dm block of every modality, modality-major, each in the flat field's layout: sum_m K_m W_dm
 * values).  n must be that count; other fields: MMM_ERR_ARG.  set_doc of THETA changes no other document's theta (the replica's theta is
 * formed first if it is held implicitly, and is explicit afterwards, as after mmm_ctm_set). */
int mmm_ctm_get_doc(mmm_ctm* m, int field, int d, double* host, size_t n);
int mmm_ctm_set_doc(mmm_ctm* m, int field, int d, const double* host, size_t n);
/* calculate_sumθ(model, d) and calculate_Ndivζ(model, d) -- MMCTM.jl:110-125 / IMMCTM.jl:90-105: sum K doubles each (either may be NULL),
 * from the stored θ and ζ of document d (0-based) */
int mmm_ctm_doc_sums(mmm_ctm* m, int d, double* sumtheta, double* Ndivzeta);
int mmm_ctm_loglik(mmm_ctm* m, double* ll /* M */);                /* calculate_loglikelihoods MMCTM.jl:384-448 */
int mmm_ctm_elbo(mmm_ctm* m, double* elbo, double terms[7]);       /* calculate_elbo MMCTM.jl:271-382           */
/* objective/gradient of one document evaluated by the device code the MMA solves use (common.jl:11-36) */
int mmm_ctm_objectives(mmm_ctm* m, int d, double* lambda_val, double* lambda_grad, double* nu_val,
                       double* nu_grad);
/* solver statistics of the last E-step: total objective evaluations of the nu and lambda solves, number of
 * solves that hit max_eval, and (optional, D ints each) per-document evaluation counts */
int mmm_ctm_solver_stats(mmm_ctm* m, int64_t* n_eval_nu, int64_t* n_eval_lambda, int64_t* n_capped,
                         int* per_doc_nu, int* per_doc_lambda);
/* Non-fatal events, COUNTED instead of raised (SURVEY section 8b "error convention": the reference ignores NLopt's return code, MMCTM.jl:141,
 * 168, never checks for NaN, and carries on -- so does the library): out[0] = LD_MMA solves of the last E-step that hit max_eval (= n_capped
 * above), out[1] = LD_MMA solves of the last E-step in which an objective value was not finite (a NaN / Inf in a document's λ, ν, ζ or in
 * μ / invΣ: such a solve cannot satisfy NLopt's tests and runs into the cap), out[2] = values of the handle's log-likelihood history that
 * are not finite (a fit whose ll is NaN never meets the stopping rule of common.jl:48-56 and runs to maxiter), out[3] = 0.  LDA / ILDA
 * handles have no solves: out[0] = out[1] = 0. */
int mmm_ctm_events(mmm_ctm* m, int64_t out[4]);
int mmm_lda_events(mmm_lda* m, int64_t out[4]);
/* Launch geometry that fixes the ORDER of the sums across documents (and so their bits): out[0] = lanes per document L,
 * [1] = theta-phase blocks, [2] = waves per theta-phase block, [3] = blocks of the moment sums, [4] = 1 when the handle
 * takes the wide-table path (term-major posting sweep instead of LDS slabs), 2 when the fused pass's theta phase runs over rows of counts
 * (dense corpora: 16 lanes per document, statistics in registers), [5] = lanes per document in the solve phase (L, sum K for the packed
 * builds, or 2 / 4), [6] = coordinates per lane in the solve phase, [7] = waves of the persistent solve launch (each takes a contiguous
 * range of D / [7] documents; 0: one document group per wave step -- no bits depend on it).  The parity tests hand it to the
 * order-matched CPU restatement (oracle/mmm_twin.c), which then reproduces a whole fit bit for bit. */
int mmm_ctm_geometry(const mmm_ctm* m, int out[8]);
/* Parity probe: out[i] = op(a[i], b[i]) evaluated by the device functions the kernels use (csrc/mmm_arith.h, dev_math.h).
 * op 0 exp, 1 log, 2 digamma (x > 0), 3 a / b, 4 sqrt, 5 / 6 / 7 sum over consecutive groups of 16 / 32 / 64 values in the
 * lane-butterfly order of the document groups (out[i] = total of i's group; n a multiple of 64), 8 the full-wave butterfly,
 * 9 / 10 the table-driven exp / log of the LD_MMA objectives (ar_exp_tab, ar_log_tab).  The device-only functions of dev_math.h:
 * 11 dev_digamma (any x), 12 dev_rcp, 13 dev_sqrt_pos, 14 dev_log_pos, 15 dev_log_tab (the log of the log-likelihood sweeps),
 * 16 ar_digamma_pos_tab, 17 dev_xlogx; and its collectives over each 64 consecutive values (n a multiple of 64): 18 wave_max,
 * 19 wave_max_dpp, 20 rows_sum4 (out[i] = (a[j] + a[j + 32]) + (a[j + 16] + a[j + 48]), j = i % 16, within i's 64), 21 wave_bcast
 * (out[i] = a[64 (i / 64) + (int)b[i]]), 22 the sum of the 64 values in index order through wave_readlane. */
int mmm_debug_math(mmm_ctx* ctx, int op, size_t n, const double* a, const double* b, double* out);
/* Fused hot path: n_iter passes of the body of fit! (MMCTM.jl:462-479 / IMMCTM.jl:440-451) */
/* fit_flags: keyword arguments of fit! (MMCTM.jl:457-458): MMM_FIT_UPDATE_SIGMA = updateΣ (IMMCTM always updates Σ,
 * IMMCTM.jl:445), MMM_FIT_AUTO_ALPHA = autoα (update_α! after update_γ!, MMCTM.jl:472-474) */
enum { MMM_FIT_UPDATE_SIGMA = 1, MMM_FIT_AUTO_ALPHA = 2 };
int mmm_ctm_iterate(mmm_ctm* m, int n_iter, int fit_flags);
int mmm_ctm_ll_history(mmm_ctm* m, double* ll /* M*max_n */, int max_n, int* n);
int mmm_ctm_fit(mmm_ctm* m, int maxiter, double tol, int fit_flags, double* ll_hist /* M*maxiter */,
                int* n_iter, int* converged, double* elbo);

/* Frozen-topic inference on a model whose globals were uploaded with mmm_ctm_set.  Every pass runs the document loop
 * { update_ζ!; update_θ!; update_ν!; update_λ! }, update_props! and the log-likelihoods; the stopping rule applies after
 * > 10 passes.  flags = 0: fit_heldout / predict_modality_η (MMCTM.jl:554-634, IMMCTM.jl:468-545; needs MU, SIGMA,
 * INVSIGMA, GAMMA, ELNPHI, PHI).  MMM_INFER_UNSMOOTHED: unsmoothed_update_θ! instead of update_θ! (θ ∝ exp(λ)·ϕ,
 * MMCTM.jl:496-509; needs PHI) -- with it, transform (MMCTM.jl:511-552).  MMM_INFER_FIT_GAUSSIAN: also update_μ! and
 * update_Σ! every pass (transform's fit_gaussian).  Topics are not touched. */
enum { MMM_INFER_UNSMOOTHED = 1, MMM_INFER_FIT_GAUSSIAN = 2 };
int mmm_ctm_infer(mmm_ctm* m, int flags, int maxiter, double tol, double* ll_hist /* M*maxiter */, int* n_iter,
                  int* converged);

/* Restart batching -- scripts/run_mmctm.jl:77-134 fits the same corpus from several random initialisations and
 * keeps the best.  A batch handle holds R independent models ("replicas") over ONE resident corpus; the batched
 * fit advances all of them with one launch per kernel (replica on grid.y), so the many small-corpus fits of a
 * restart sweep fill the GPU together.  Replica r computes exactly what a model created from gamma0[r] alone
 * computes.  gamma0: R contiguous blocks in the layout of mmm_ctm_create.
 * The per-model API above (get/set/update_* /loglik/elbo/iterate/fit) acts on the selected replica (0 after
 * create).  theta is kept for one replica at a time and rebuilt when the selection changes. */
int mmm_ctm_create_batch(mmm_ctx* ctx, int R, int D, int M, const int* K, const int* V, const double* alpha,
                         const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const int* n_feat,
                         const int* J, const int32_t* features, const double* gamma0,
                         const mmm_solver_opts* opts, mmm_ctm** out);
int mmm_ctm_replicas(const mmm_ctm* m);
int mmm_ctm_select(mmm_ctm* m, int r);
/* fit! of every replica, in lock step; a replica stops when its own stopping rule fires (common.jl:48-51).
 * ll_hist: [R][maxiter][M]; n_iter, converged: [R]; elbo: [R] or NULL.  All replicas must have the same number
 * of earlier passes. */
int mmm_ctm_fit_batch(mmm_ctm* m, int maxiter, double tol, int fit_flags, double* ll_hist, int* n_iter,
                      int* converged, double* elbo);

/* ---- free functions of the reference (arguments are caller arrays, no model) --------------------------------------
 * The reference's tests call these directly (test/common.jl:79-97; test/mmctm.jl:135-148,268-293,349-388; test/immctm.jl:122-160,
 * 273-294,350-386).  Values and gradients in the reference's MAXIMISATION form; grad may be NULL (the reference's `length(∇) > 0`). */
/* λ_objective(λ, ∇λ, ν, Ndivζ, sumθ, μ, invΣ) -- common.jl:11-23; invSigma n x n column-major */
int mmm_lambda_objective(mmm_ctx* ctx, int n, const double* lambda, const double* nu, const double* Ndivzeta, const double* sumtheta,
                         const double* mu, const double* invSigma, double* val, double* grad);
/* ν_objective(ν, ∇ν, λ, Ndivζ, μ, invΣ) -- common.jl:25-36 (μ is unused there too and may be NULL) */
int mmm_nu_objective(mmm_ctx* ctx, int n, const double* nu, const double* lambda, const double* Ndivzeta, const double* mu,
                     const double* invSigma, double* val, double* grad);
/* α_objective(α, ∇α, sum_Elnϕ, K, V) -- common.jl:38-46 */
int mmm_alpha_objective(mmm_ctx* ctx, double alpha, double sum_Elnphi, int K, int V, double* val, double* grad);
/* Σ_d Σ_w n_w log(Σ_k props[k + K d] · phi[k V + v_w]) / Σ_d N_d over the documents with N_d > 0, CSR as in mmm_lda_create:
 * calculate_loglikelihood(X, θ, β) LDA.jl:174-188 (props = θ K x D, phi = β V x K column-major -- the same [k V + v]),
 * calculate_modality_loglikelihood(X, props, ϕ) MMCTM.jl:402-418, calculate_docmodality_loglikelihood (D = 1) MMCTM.jl:384-400. */
int mmm_mixture_loglik(mmm_ctx* ctx, int D, int K, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count,
                       const double* props, const double* phi, double* ll);
/* The same with a topic-term probability that factorises over the I features of a term: Π_i phi[k ΣJ + Σ_{q<i} J_q + features[i V + v]]
 * (features 0-based, [i V + v]; phi in the IMMCTM gamma layout of one modality).  softmax = 1: calculate_modality_loglikelihood(X, η, ϕ,
 * features) -- IMMCTM.jl:362-407, props = softmax(eta[:, d]) (eta K x D); softmax = 0: eta holds the proportions themselves --
 * calculate_loglikelihood(X, features, θ, β) of ILDA.jl:203-231 (phi[k][i][j] = β[i][j, k]). */
int mmm_mixture_loglik_features(mmm_ctx* ctx, int D, int K, int V, int I, const int* J, const int32_t* features, const int64_t* doc_ptr,
                                const int32_t* term, const int32_t* count, const double* eta, int softmax, const double* phi, double* ll);

/* ---- bootstrap of the exposures under trained topics (no counterpart in the reference; DESIGN.md "Bootstrap of the exposures") -------------
 * Resample every sample's counts multinomially B times, infer the exposures of every replicate under the frozen topics (the stacked
 * corpus of B x D replicate documents goes through the existing frozen-topic passes: mmm_lda_infer / mmm_ctm_infer), summarise.  The two
 * entry points below are the pieces around those passes; they take caller arrays, need no model and no communicator (on a multi-rank
 * context they act on the arrays they are given: no collective). */
/* B multinomial resamples of every document of a CSR corpus, drawn on the GPU.
 * out[b * nnz + e], b = 0..B-1: the resampled count of entry e in replicate b0 + b.
 * The sparsity pattern is kept: an entry may come out 0; a document keeps its total N_d.
 * Random numbers: Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85), key =
 * (seed low 32 bits, seed high 32 bits), counter = (i / 4, d, b, stream) with d the document index in the arrays given, b the GLOBAL
 * replicate index (b0 + ..., so chunked calls are slices of one big call) and i the draw index within the (document, replicate) pair; draw
 * i is output word i % 4 of its block.  Draw: for the 32-bit word u and the document total N_d, r = (uint64(u) * N_d) >> 32 (all integer;
 * bias <= N_d / 2^32, not corrected); with cum the inclusive prefix sums of the document's counts in CSR order the draw lands in the
 * entry e with cum[e-1] <= r < cum[e].  A zero count never receives a draw; N_d = 0 gives an all-zero row.  Output = draws per entry.
 * The same arguments give the same bits on every run.
 * MMM_ERR_ARG: NULL pointer, negative count, doc_ptr[0] != 0 or decreasing doc_ptr, B < 0, b0 < 0, b0 + B > 2^31 - 1;
 * MMM_ERR_UNSUPPORTED: some N_d >= 2^31.  B = 0 or nnz = 0: MMM_OK, nothing written. */
int mmm_resample_counts(mmm_ctx* ctx, int D, const int64_t* doc_ptr, const int32_t* count, int B, int b0, uint64_t seed, uint32_t stream,
                        int32_t* out);
/* x[b * n + j], b < B: B replicates of n values.  Per column j, with x_(0) <= ... <= x_(B-1) its sorted values:
 *   mean[j] = (sum_b x_b) / B, summed in replicate order;
 *   sd[j] = sqrt(sum_b (x_b - mean)^2 / (B - 1)) (two passes, Julia's std; 0 when B = 1);
 *   quant[i * n + j] = the q[i]-quantile (0 <= q[i] <= 1, i < nq): h = (B - 1) q, lo = floor(h),
 *                      x_(lo) + (h - lo) (x_(min(lo + 1, B - 1)) - x_(lo)) -- Julia's default quantile, numpy's "linear";
 *                      q = 0 and q = 1 are the minimum and the maximum exactly.
 * Any of mean / sd / quant may be NULL.  A column that contains a NaN gives NaN in all its outputs.  1 <= B <= 4096 (a column is sorted
 * in LDS); MMM_ERR_UNSUPPORTED above that; MMM_ERR_ARG for B < 1, a q outside [0, 1], NULL x or q. */
int mmm_replicate_summary(mmm_ctx* ctx, int B, size_t n, const double* x, int nq, const double* q, double* mean, double* sd, double* quant);

/* ---- matching signatures to a catalogue and across the replicas of a restart batch (no counterpart in the reference, whose README leaves
 * the step to the user: cosine to the catalogue, then a linear sum assignment) -------------------------------------
 * Inputs: sig[r][k][v] (R sets of K signatures over V terms, row-major) and cat[c][v] (C catalogue signatures), all finite and >= 0; rows
 * need NOT be normalised (the cosine is scale-free).
 * 1. Cosine.  S[r][k][c] = (sum_v sig cat) / (sqrt(sum_v sig^2) sqrt(sum_v cat^2)); a row whose sum of squares is 0 gives S = 0 against
 *    everything (never NaN).  Each of the three sums is taken in the same order, fixed by V alone: 64 partial sums, partial l over the terms
 *    l, l + 64, l + 128, ... ascending, combined as a tree -- l with l ^ 1, then with l ^ 2, then the two quads of a group of 8, the two
 *    halves of a group of 16, and the four groups of 16 as (0 + 2) + (1 + 3); products and sums are separate roundings (no fused
 *    multiply-add).  Neither R, the chunking of the replicas nor the device enters.
 * 2. Assignment.  For every r the injective a_r : k -> c that maximises sum_k S[r][k][a_r(k)], by the shortest-augmenting-path algorithm
 *    of Crouse (IEEE TAES 52(4), 2016, Algorithm 1) on W = -S: rows are inserted in the order k = 0..K-1; the duals u, v start at 0; in a
 *    search from row i (minval = 0 at first) the reduced cost of an unscanned column c is ((minval + W[i][c]) - u[i]) - v[c] and replaces
 *    spc[c] (and path[c] = i) only when strictly smaller; the next column is the unscanned c with the smallest spc[c], ties to the lowest
 *    c; minval = its spc; it is scanned; if it is assigned the search goes on from its row, else it is the sink.  Dual update:
 *    u[cur] += minval; u[i] += minval - spc[col4row[i]] for the other scanned rows; v[c] -= minval - spc[c] for the scanned columns; then
 *    the assignment is flipped along `path` from the sink.  Only +, - and compares: given S, the same result on any machine.
 * 3. Outputs per replica: assign[r][k] (0-based), matched[r][k] = S[r][k][assign[r][k]], optionally S.
 * 4. Consensus of R replicas against replica `ref`: the catalogue is replica ref's own K signatures (C = K);
 *    P[r][assign[r][k]][v] = sig[r][k][v] / sum_v sig[r][k][v] (sum in index order; a zero row stays zero) is every replica in the
 *    labelling of `ref`; mean / sd / quant of P[.][k][v] over the R replicas by the definitions of mmm_replicate_summary ([K][V],
 *    [K][V], [nq][K][V]); stability[k] = the mean over r != ref, added in replica order, of the matched cosine of the signature of
 *    replica r that is assigned to k (R = 1: 1.0).
 * Limits: 1 <= K <= C <= 1024, V >= 1, any R >= 0 (replicas go through the device in chunks, which cannot change a replica's bits; R = 0
 * writes nothing); the consensus 1 <= R <= 4096.  mmm_signature_cosine alone takes any K, C >= 1.
 * MMM_ERR_ARG: NULL pointers, K > C, K < 1, a negative or non-finite entry in a caller array, `ref` outside [0, R), q outside [0, 1], a
 * replica table (handle forms) with a non-finite entry.  MMM_ERR_UNSUPPORTED, with the limit in the message: C > 1024, R > 4096 replicas
 * in a consensus, ILDA / IMMCTM handles (feature-factorised tables). */
int mmm_signature_cosine(mmm_ctx* ctx, int R, int K, int C, int V, const double* sig, const double* cat, double* S /* [R][K][C] */);
int mmm_signature_match(mmm_ctx* ctx, int R, int K, int C, int V, const double* sig, const double* cat, int32_t* assign /* [R][K] */,
                        double* matched /* [R][K] */, double* S /* [R][K][C] or NULL */);
/* each of assign, matched [R][K], stability [K], mean, sd [K][V], quant [nq][K][V] may be NULL */
int mmm_signature_consensus(mmm_ctx* ctx, int R, int K, int V, const double* sig, int ref, int nq, const double* q, int32_t* assign,
                            double* matched, double* stability, double* mean, double* sd, double* quant);
/* The same on the replicas of a handle (R = mmm_lda_replicas / mmm_ctm_replicas; an ordinary handle is one replica), read where they lie:
 * LDA: the lambda of every replica (topic k = column k of the V x K table); MMCTM: the gamma of modality `modality`.  cat == NULL: the
 * catalogue is the selected replica's own topics (C is ignored, C = K).  Only cat goes up and only the outputs come down. */
int mmm_lda_match_replicas(mmm_lda* m, int C, const double* cat, int32_t* assign, double* matched);
int mmm_ctm_match_replicas(mmm_ctm* m, int modality, int C, const double* cat, int32_t* assign, double* matched);
int mmm_lda_replica_consensus(mmm_lda* m, int ref, int nq, const double* q, int32_t* assign, double* matched, double* stability, double* mean,
                              double* sd, double* quant);
int mmm_ctm_replica_consensus(mmm_ctm* m, int modality, int ref, int nq, const double* q, int32_t* assign, double* matched, double* stability,
                              double* mean, double* sd, double* quant);

/* ---- choosing the number of signatures by held-out mutations (no counterpart in the reference, which takes K as given; DESIGN.md section
 * 4.12).  A document's mutations are dealt into F folds, models are fitted on F - 1 of them (the existing restart batches) and scored on
 * the fold they did not see.  The two array entries need no model and no communicator; the handle entry scores every restart of a batch
 * where its tables lie. */
/* Partition every document's mutations into F folds.  out[f * nnz + e], f < F: the number of mutations of entry e that fall in fold f.
 * The N_d mutations of document d are numbered i = 0 .. N_d - 1 in CSR order: with cum the inclusive prefix sums of the document's counts,
 * mutation i lies in the entry e with cum[e-1] <= i < cum[e].  Its fold is (uint64(u_i) * F) >> 32, where u_i is output word i % 4 of the
 * Philox4x32-10 block (constants as for mmm_resample_counts) with key = (seed low 32 bits, seed high 32 bits) and counter =
 * (i / 4, d, rep, 0x80000000 | stream): the high bit of the fourth counter word keeps a split from sharing its random words with a
 * resample of the same seed, hence stream < 2^31.  `rep` numbers repeated splits of one seed.
 * It follows that sum_f out[f][e] = count[e] exactly; the sparsity pattern is kept (an entry may come out 0 in a fold, as with the
 * resampler); the same arguments give the same bits on every run and under every launch geometry (integer arithmetic only).
 * MMM_ERR_ARG: NULL pointer, negative count, doc_ptr[0] != 0 or decreasing doc_ptr, F outside 1..64, rep < 0, stream >= 2^31;
 * MMM_ERR_UNSUPPORTED: some N_d >= 2^31.  nnz = 0: MMM_OK, nothing written. */
int mmm_split_counts(mmm_ctx* ctx, int D, const int64_t* doc_ptr, const int32_t* count, int F, int rep, uint64_t seed, uint32_t stream,
                     int32_t* out);
/* Per-document log-likelihood and reconstruction cosine of a CSR corpus under proportions props [k + K d] and a table phi [k V + v], as
 * mmm_mixture_loglik takes them.  With p_v = sum_k props[k + K d] * phi[k V + v], k ascending, product and sum rounded separately:
 *   ll_doc[d] = sum_e n_e log p_{v_e},  n_doc[d] = N_d  -- the per-document sums of mmm_mixture_loglik, same expressions, same order;
 *   total[0] = sum_d ll_doc / sum_d n_doc, total[1] = sum_d ll_doc, total[2] = sum_d n_doc over the documents with N_d > 0: total[0] is
 *              the value of mmm_mixture_loglik on the same arguments, bit for bit;
 *   cos_doc[d] = (sum_e n_e p_{v_e}) / (sqrt(sum_e n_e^2) * sqrt(sum_{v < V} p_v^2)): the cosine between the document's counts and its
 *              reconstruction N_d p.  Each of the three sums is 64 partial sums, partial l over the indices l, l + 64, ... ascending (entries
 *              in CSR order, terms v in index order), combined as a butterfly: l with l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  0 where a norm
 *              is 0 (an empty or all-zero document).  The entries of a document are taken as given: duplicate terms are NOT merged (each
 *              entry is a coordinate of its own in the numerator and in sum n_e^2);
 *   total[3] = the mean of cos_doc over the documents with N_d > 0, by the 256 strided partial sums and the tree of total[0].
 * No document with N_d > 0: total[0] and total[3] are NaN (0 / 0), as with mmm_mixture_loglik.  ll_doc, n_doc, cos_doc ([D] each) may be
 * NULL.  MMM_ERR_ARG as mmm_mixture_loglik. */
int mmm_mixture_score(mmm_ctx* ctx, int D, int K, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count,
                      const double* props, const double* phi, double* ll_doc, double* n_doc, double* cos_doc, double* total /* [4] */);
/* The same for every replica of a handle (R = mmm_lda_replicas; an ordinary handle is one replica) on a corpus of the caller's with the
 * handle's D documents and terms < V (doc_ptr holds D + 1 offsets), read where the tables lie: replica r's outputs equal those of
 * mmm_mixture_score on the theta and beta that mmm_lda_get returns after mmm_lda_select(r), bit for bit (theta = gamma / sum gamma is formed
 * in the kernel from the gamma of the replica's own pass).  total [R][4]; ll_doc, cos_doc [R][D], may be NULL.  One upload (the corpus), two
 * launches, one download, whatever R.  The handle is left as it was, its selected replica included.
 * MMM_ERR_UNSUPPORTED: ILDA handles; MMM_ERR_ARG: a replica on which no pass has run, a corpus that is no CSR of terms < V. */
int mmm_lda_score_replicas(mmm_lda* m, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, double* total, double* ll_doc,
                           double* cos_doc);

/* ---- exposures to a FIXED catalogue of signatures, with sparse selection (signature assignment / refitting; no counterpart in the reference,
 * DESIGN.md section 4.13).  CSR corpus as mmm_mixture_score takes it; cat [C][V], >= 0, finite, every row sum > 0 (rows need not be
 * normalised); allowed [D][C] (non-zero: the signature may be used) or NULL = all; penalty [D] or NULL = no elimination.
 * Per document d.  n_v: the dense count vector (duplicate terms summed), N = sum_v n_v, f_v = n_v / N; P[c][v] = cat[c][v] / sum_v cat[c][v]
 * (the sum in index order).
 * fit(A), A a set of signatures: w_c = 1 / |A| on A, 0 elsewhere (every fit is a cold start: fit(A) depends on A alone, not on the path to
 *   A); iterations t = 1 .. maxiter:  q_v = sum_c w_c P[c][v];  r_v = f_v / q_v where n_v > 0 and q_v > 0, else 0;  g_c = sum_v r_v P[c][v];
 *   w'_c = w_c g_c;  stop after an iteration with max_c |w'_c - w_c| < tol (strict: tol = 0 runs maxiter iterations).  Then, with
 *   S = sum_c w_c:  w <- w / S if S > 0 (S = 0: A produces none of the document's mutations and w stays 0);  q recomputed;
 *   ll(A) = sum over n_v > 0, q_v > 0 of n_v log q_v;  u(A) = sum over n_v > 0, q_v = 0 of n_v -- the mutations no signature of A can produce.
 * Order of the sums: q_v and S sequentially over c ascending; g_c and ll as 64 partial sums, partial l over the indices l, l + 64, ...
 *   ascending, combined by the butterfly of mmm_mixture_score's cosine sums (l with l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1).  Products, sums
 *   and the (IEEE, correctly rounded) divisions are separate roundings.  All terms are >= 0, so a zero weight or a zero r_v may be added or
 *   left out without changing a bit.  log is the device library's (< 1 ulp); it enters ll and cost only.
 * Elimination: A = {c : allowed[d][c]}; fit(A).  With a penalty, while |A| > 1: c* = the member of A with the smallest w_c (ties: the lowest
 *   c); B = A \ {c*}; fit(B); delta = ll(A) - ll(B) if u(B) == u(A), else +inf; if delta < penalty[d]: order[d][j] = c*, cost[d][j] = delta
 *   for round j = 0, 1, ..., and A <- B with B's w and ll; otherwise stop.  (Smallest contribution first: one refit per round, and the choice
 *   is made on values that only +, x, / and comparisons decide.)
 * Outputs: w[d][.] the final weights (exactly 0 outside A), active[d][c] = 1 on A, order / cost (rounds that did not run: -1 / 0),
 *   ll_doc = ll(A), unexplained = u(A), iters = the EM iterations of all fits of the document.  N = 0 or an empty `allowed` row: all outputs 0,
 *   order -1, unexplained = N.  Every output except w may be NULL.  The same arguments give the same bits on every run, whatever D and
 *   wherever the catalogue is held (LDS, or read through L2 when C V doubles exceed 96 KiB).
 * Limits: 1 <= C <= 256, V >= 1 (C V < 2^31), D >= 0 (D = 0 writes nothing).  MMM_ERR_ARG: NULL pointers, a catalogue entry that is negative or
 *   not finite, a catalogue row whose sum is 0, a penalty that is negative or not finite, maxiter < 1, tol < 0, a corpus that is no CSR of
 *   terms < V.  MMM_ERR_UNSUPPORTED, with the limit in the message: C > 256.  No collective: on a multi-rank context it acts on its arrays. */
int mmm_refit_exposures(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* cat,
                        const uint8_t* allowed, const double* penalty, int maxiter, double tol, double* w, uint8_t* active, int32_t* order, double* cost,
                        double* ll_doc, double* unexplained, int64_t* iters);

/* ---- model simulation and per-sample goodness of fit by a parametric bootstrap (no counterpart in the reference).
 * props [k + K d] and phi [k V + v] as mmm_mixture_score takes them, every entry >= 0 and finite; rows need not be normalised.
 * Per document d:
 * Mixture.  p_v = sum_k props[k + K d] * phi[k V + v], k ascending, product and sum rounded separately (mmm_mixture_score's p);
 *   cum_v = the inclusive sum of p over v ascending, strictly sequential; S = cum_{V-1}; pi_v = p_v / S (an IEEE division).
 * Thresholds.  T_v = floor((cum_v / S) * 2^32), an integer in [0, 2^32]: non-decreasing, T_{V-1} = 2^32 exactly, and a term with p_v = 0
 *   has T_v = T_{v-1}.
 * Draws.  Draw i < N_d of replicate b (the GLOBAL index b0 + ..., so chunked calls are slices of one big call) uses output word i % 4 of
 *   the Philox4x32-10 block with the constants and the key of mmm_resample_counts and the counter (i / 4, d, 0x80000000 | b, stream), d
 *   being the document's index in the arrays given.  The high bit of the third counter word is free in mmm_resample_counts and in
 *   mmm_split_counts (both keep b, rep < 2^31), so a simulation shares no random word with either, whatever the stream.  With u that
 *   word, the draw lands on the first v with T_v > u.  Integer throughout; a term with p_v = 0 never receives a draw; the resolution is
 *   2^-32 per term and is not corrected, as with the resampler.  A replicate is the vector of draws per term: it sums to N_d.
 * Statistics of a count vector n with total N over the V terms (for the observed document: the dense vector, duplicate terms summed):
 *   cosine = (sum_v n_v pi_v) / (sqrt(sum_v n_v^2) * sqrt(sum_v pi_v^2)), 0 where a norm is 0;
 *   chi2 = sum_v t_v, with t_v = ((n_v - e_v) * (n_v - e_v)) / e_v and e_v = N * pi_v where pi_v > 0; where pi_v = 0, t_v = +inf if
 *   n_v > 0, else 0.
 *   Each of the four sums is 64 partial sums, partial l over v = l, l + 64, ... ascending from 0.0, combined by the butterfly of
 *   mmm_mixture_score's cosine sums (l with l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1).  Every product, sum, difference, division and square
 *   root is a separate, correctly rounded operation; there is no log.  So every output is decided by exactly rounded operations in a
 *   fixed order: the same arguments give the same bits on every run and under every launch geometry; a document gives the same bits
 *   whatever its neighbours as long as its index d is the same; a call with (b0, B) is a slice of the call with (0, b0 + B).
 * N_d = 0: nothing is drawn; the replicates are all-zero rows, both statistics and every replicate value are 0, both counts are B.
 * MMM_ERR_ARG, nothing written: NULL pointers, K < 1, V < 1, D < 0, B < 0, b0 < 0, b0 + B > 2^31 - 1, a negative n_doc or count, a corpus
 *   that is no CSR of terms < V, a props or phi entry that is negative or not finite, a document with N_d > 0 whose S is 0 or not finite
 *   (the message names it).  MMM_ERR_UNSUPPORTED, with the limit in the message: N_d >= 2^31; V > 4096 (a block keeps pi, the thresholds
 *   and its histograms in LDS).  Any K >= 1.  No collective: on a multi-rank context both act on the arrays they are given. */
/* out[(b D + d) V + v], b < B: the draws on term v of replicate b0 + b of document d, n_doc[d] of them.  Replicates go through a bounded
 * device buffer in chunks.  B = 0 or D = 0: MMM_OK, nothing written. */
int mmm_simulate_counts(mmm_ctx* ctx, int D, int K, int V, const double* props, const double* phi, const int32_t* n_doc /* [D] */, int B, int b0,
                        uint64_t seed, uint32_t stream, int32_t* out /* [B][D][V] */);
/* CSR corpus as mmm_mixture_score takes it; N_d is the sum of the document's counts.  cos_obs, chi_obs [D]: the statistics of the observed
 * vector.  Replicate (d, b) is exactly the vector mmm_simulate_counts gives for the same arguments with n_doc[d] = N_d; it never leaves
 * the device.  cos_le[d] = the number of b with cos_rep <= cos_obs, chi_ge[d] = the number of b with chi_rep >= chi_obs, over the B
 * replicates of THIS call (the counts of chunked calls add).  cos_rep, chi_rep: [b D + d] the replicates' statistics, or NULL.
 * B = 0: the observed statistics and zero counts.  D = 0: nothing written. */
int mmm_fit_check(mmm_ctx* ctx, int D, int K, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* props,
                  const double* phi, int B, int b0, uint64_t seed, uint32_t stream, double* cos_obs, double* chi_obs /* [D] */, int32_t* cos_le,
                  int32_t* chi_ge /* [D] */, double* cos_rep, double* chi_rep /* [B][D] or NULL */);

/* ---- is signature t present in document d?  A likelihood-ratio statistic per (target, document) and its null distribution by a parametric
 * bootstrap, in one call (no counterpart in the reference).  CSR corpus, cat and allowed as mmm_refit_exposures
 * takes them; P, n_v, N, f_v, fit(A) with the order of its sums, ll(A) and u(A) are those of mmm_refit_exposures.
 * Items.  Item j = t_idx D + d for t_idx in [0, T) and document d; t = targets[t_idx].  A1 = allowed_d + {t}, A0 = allowed_d - {t}
 *   (allowed == NULL: the whole catalogue), so t is always in A1 and never in A0.
 * Statistic of a count vector n of total N.  Null fit: (w0, ll0, u0) = fit(A0).  Score: s = sum_v r_v P[t][v] with r_v = f_v / q0_v where
 *   n_v > 0 and q0_v > 0, else 0, q0 the mixture of the NORMALISED w0; the sum as 64 partial sums (v = l, l + 64, ... ascending) and the
 *   butterfly of fit(A); no log enters s.
 *   u0 = 0 and not (s > 1):  Lambda = 0 exactly and fit(A1) is NOT run -- the mixture likelihood is concave in w and s <= 1 is the
 *     Karush-Kuhn-Tucker condition for the null optimum to be the optimum over A1.
 *   u0 = 0 and s > 1:  (w1, ll1, u1) = fit(A1), Lambda = max(2 (ll1 - ll0), 0).
 *   u0 > 0 (the null cannot produce some mutation):  fit(A1) runs; Lambda = +inf if u1 < u0, else max(2 (ll1 - ll0), 0).
 * Observed.  status[j] = 3: N_d = 0 or A0 empty, untestable -- every other output of the item is 0 (the caller's p is NaN); 1: Lambda_obs = 0,
 *   count_ge = B and no replicate is run; 2: Lambda_obs = +inf, count_ge = 0 and no replicate is run; 0: tested by the replicates below.
 *   w_null[j][.] = w0 (exactly 0 outside A0), score[j] = s, stat[j] = Lambda_obs, w_alt[j] = w1_t (0 where fit(A1) did not run).
 * Replicates (status 0).  Replicate b in [b0, b0 + B) of item j is the draw of mmm_simulate_counts for document j of a T D-document corpus
 *   with the props row w_null[j][.], phi = P and the total N_d: the sequential cum, T_v = floor((cum_v / S) 2^32), the counter
 *   (i / 4, j, 0x80000000 | b, stream) under the key (seed low, seed high) -- deliberately the words mmm_simulate_counts(w_null, P, N) uses
 *   under the same (seed, stream), so that the replicates can be reproduced through it (and a goodness of fit under the same seed and
 *   stream is correlated with this test).  Lambda_b is the statistic of the replicate.  count_ge[j] = #{b : Lambda_b >= Lambda_obs},
 *   count_zero[j] = #{b : Lambda_b = 0} over the B replicates of THIS call (the counts of chunked calls add); p = (1 + count_ge) / (B + 1) is
 *   the caller's.  rep_stat (or NULL): [b T D + j] = Lambda_b, NaN for the items without replicates.
 * iters[j]: the EM iterations of all the item's fits, the replicates' of this call included.
 * w_null, score, the branch taken (observed and in every replicate), the draws, status, count_zero and iters are decided by +, x, / and
 *   comparisons in a fixed order: the same bits on every run, under every launch geometry and wherever the catalogue is read from.  Lambda and
 *   count_ge pass through the device log (< 1 ulp per term), as ll of mmm_refit_exposures does.
 * Limits: 1 <= C <= 256, 1 <= V <= 4096, T >= 1, T D < 2^31, N_d < 2^31, b0 + B <= 2^31 - 1; B = 0 runs the observed phase only; D = 0 writes
 *   nothing.  MMM_ERR_ARG, nothing written: NULL pointers, a target outside [0, C), B < 0, b0 < 0, b0 + B > 2^31 - 1, maxiter < 1, tol < 0 and
 *   the catalogue and corpus errors of mmm_refit_exposures.  MMM_ERR_UNSUPPORTED, with the limit in the message: C > 256, V > 4096,
 *   T D >= 2^31, N_d >= 2^31.  No collective: on a multi-rank context it acts on its arrays. */
int mmm_presence_test(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* cat,
                      const uint8_t* allowed /* [D][C] or NULL */, int T, const int32_t* targets /* [T] */, int B, int b0, uint64_t seed, uint32_t stream,
                      int maxiter, double tol, double* w_null /* [T D][C] */, double* stat, double* score, double* w_alt /* [T D] */, int32_t* count_ge,
                      int32_t* count_zero, int8_t* status, int64_t* iters, double* rep_stat /* [B][T D] or NULL */);

/* ---- what is a negative of the presence test worth?  Its detection power per (target, document) over a grid of spiked-in fractions and
 * totals, in one call (no counterpart in the reference).  Items, A0, A1, fit(A), the statistic Lambda, the score, the
 * rule that skips fit(A1) and the statuses are those of mmm_presence_test, unchanged.
 * Observed.  As mmm_presence_test: w0 = w_null[j][.], stat, score, w_alt, status per item j = t_idx D + d.  Items of status 3 (untestable)
 *   take no part: every other output of theirs is 0 (rep_stat NaN; the caller's power is NaN).  Items of status 0, 1 AND 2 all take part --
 *   an item with Lambda_obs = 0 is the main customer.
 * Levels.  H totals x (1 + G) fractions: phi_0 = 0 (the null level), phi_g = fractions[g - 1] for g >= 1, strictly increasing in (0, 1];
 *   level l = h (1 + G) + g, L = H (1 + G) of them.  The total of (h, d) is N^h_d = n_level[h D + d] (>= 1); n_level == NULL: H = 1 and the
 *   observed N_d.
 * Generating weights of (l, j).  W0 = the sequential sum of w0_c over c ascending.  For g >= 1: w^l_c = (1 - phi_g) * w0_c for c in A0,
 *   w^l_t = phi_g * W0, 0 elsewhere ((1 - phi_g) one subtraction, each weight one product).  For g = 0: w^l = w0 itself, by definition and
 *   not by a product with 1.
 * Replicates.  Replicate b in [b0, b0 + B) of (l, j) is the vector mmm_simulate_counts gives for document l T D + j of an L T D-document
 *   corpus whose props rows are the w^l_j, phi = P and n_doc = N^h_d, under the same (seed, stream): the mixture summed over all C in
 *   ascending c, the sequential cum, T_v = floor((cum_v / S) 2^32), the counter (i / 4, l T D + j, 0x80000000 | b, stream).  So every
 *   replicate can be reproduced through a shipped entry, and level 0 at the observed totals is word for word the replicate sequence of
 *   mmm_presence_test.  Lambda^l_b is the statistic of that replicate over the same A0 and A1.
 * Critical value.  m = floor(alpha * (B + 1)) - 1, the product one multiplication in double.  With s_1 >= s_2 >= ... the B null statistics
 *   (g = 0) of (h, j): crit[h T D + j] = s_{m+1}; +inf where m < 0 (the test cannot reject at this B) and where m + 1 > B.  Rejection is
 *   Lambda > crit, which is exactly "p = (1 + #{Lambda_null >= Lambda}) / (B + 1) <= alpha" of the presence test.  crit is an element of the
 *   set: how it is selected cannot change its bits.
 * Outputs.  crit [H][T D]; count_reject[l T D + j] = #{b : Lambda^l_b > crit[h][j]}; count_zero[l T D + j] = #{b : Lambda^l_b = 0};
 *   iters[j]: the EM iterations of all the item's fits, every level's replicates of this call included; rep_stat (or NULL):
 *   [(l B + b) T D + j] = Lambda^l_b, NaN for the levels and items without replicates.  At g = 0 count_reject <= max(m, 0) by construction:
 *   the attained size of the test.
 * crit_in (or NULL): [H][T D].  Given, the null levels (g = 0) are NOT run: crit = crit_in, the counts of the null levels are 0 and their
 *   rep_stat is NaN; the other outputs are then a pure function of the replicates, and the counts of calls over (b0, B) chunks add.  Without
 *   crit_in a call takes its critical values from the B null replicates of THIS call only, so its counts do not add over chunks.
 * The draws, the branch taken in every replicate, count_zero and iters are decided as in mmm_presence_test: the same bits on every run, under
 *   every launch geometry and wherever the catalogue is read from.  Lambda passes through the device log; crit is one of those values and
 *   count_reject compares with it.  All counts are integers added by integer atomics.
 * Limits: 1 <= C <= 256, 1 <= V <= 4096, T >= 1, 1 <= G <= 64, 1 <= H <= 64, L T D < 2^31, N_d < 2^31, b0 + B <= 2^31 - 1; D = 0 writes
 *   nothing.  MMM_ERR_ARG, nothing written: NULL pointers, G < 1, H < 1, n_level == NULL with H != 1, an n_level entry < 1, alpha outside
 *   (0, 1), fractions not strictly increasing or outside (0, 1], B < 0, B = 0 without crit_in, b0 < 0, b0 + B > 2^31 - 1 and every error of
 *   mmm_presence_test.  MMM_ERR_UNSUPPORTED, with the limit in the message: C > 256, V > 4096, G > 64, H > 64, L T D >= 2^31, N_d >= 2^31.
 *   No collective: on a multi-rank context it acts on its arrays. */
int mmm_presence_power(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* cat,
                       const uint8_t* allowed /* [D][C] or NULL */, int T, const int32_t* targets /* [T] */, int G, const double* fractions /* [G] */, int H,
                       const int32_t* n_level /* [H][D] or NULL */, double alpha, int B, int b0, uint64_t seed, uint32_t stream, int maxiter, double tol,
                       const double* crit_in /* [H][T D] or NULL */, double* w_null /* [T D][C] */, double* stat, double* score, double* w_alt /* [T D] */,
                       int8_t* status, int64_t* iters, double* crit /* [H][T D] */, int32_t* count_reject, int32_t* count_zero /* [L][T D] */,
                       double* rep_stat /* [L][B][T D] or NULL */);

/* ---- which signature caused this mutation?  The posterior of every signature per queried (document, term) pair and its uncertainty by the
 * non-parametric bootstrap, in one call (no counterpart in the reference).  CSR corpus, cat and allowed as
 * mmm_refit_exposures takes them; P, n_v, N, f_v and fit(A) with the order of every sum are those of mmm_refit_exposures, unchanged.  No
 * elimination runs here: A_d is the `allowed` row (NULL: the whole catalogue), normally the chosen set of an earlier refit.
 * Queries.  A CSR over documents: q_ptr [D + 1] (from 0, not decreasing), Q = q_ptr[D]; q_term [Q], terms < V -- a queried term need not
 *   occur in the document, and a (document, term) pair may be queried more than once; q_mult [Q] >= 1 or NULL = 1; q_group [Q] in [-1, G)
 *   or NULL, -1 = no group.  A document without queries is not processed: status 4, its w row 0, no replicates.
 * Observed.  w = fit(A_d).  q_v = sum_c w_c P[c][v], sequentially over c ascending.  For query e = (d, v): post[e][c] = (w_c * P[c][v]) / q_v
 *   where q_v > 0, the product and the (IEEE, correctly rounded) division separate roundings; exactly 0 outside A_d; the whole row 0 where
 *   q_v = 0.  w[d][.] is output too.  status[d]: 0 processed; 3: N_d = 0 or an empty `allowed` row -- every other output of the document
 *   and of its queries is 0 and no replicates run; 4: no queries.
 * Replicates (status 0).  Replicate b in [b0, b0 + B) of document d is EXACTLY the count vector mmm_resample_counts gives for (d, b, seed,
 *   stream): the counter (i / 4, d, b, stream), r = (u N_d) >> 32, the inclusive prefix sums of the document's entries in CSR order, the
 *   draws counted by term.  Deliberately so: the replicate can be reproduced through the shipped entry, and an attribution under the same
 *   (seed, stream) uses the replicates of a bootstrap of the exposures (refit_exposures(bootstrap = B) in the Python layer), so the two
 *   sets of intervals describe the same resamples.  Per replicate w_b = fit(A_d) on the replicate's counts (f_v = n_v / N_d) and
 *   rho_b[e][c] is formed as post is.  With x = floor(rho_b * 2^24), an exact integer <= 2^24 (rho <= 1: q_v is a sum of non-negative
 *   terms that holds the numerator):
 *     sum_fx[e][c] += x;  sumsq_fx[e][c] += x * x;
 *     top_count[e][c] += 1 for the c with the largest rho_b (ties: the lowest c), skipped where the replicate's q_v = 0;
 *     void_count[e] += 1 where the replicate's q_v = 0;
 *     group_fx[b - b0][g][c] += q_mult[e] * x for g = q_group[e] >= 0;
 *     rep_post[b - b0][e][c] = rho_b (or NULL).
 *   iters[d]: the EM iterations of all the document's fits in this call.
 * No log is used anywhere: every output is decided by +, x, / and comparisons in a fixed order, and every accumulator is an integer added
 *   by integer atomics, so the same arguments give the same bits on every run, under every launch geometry and wherever the catalogue is
 *   read from (LDS, or L2 where an A_d's rows do not fit or under MMM_OFF_REFIT_LDS).  The counts and sums of calls with (b0, B) chunks
 *   add; a call with (b0, B) is a slice of the call with (0, b0 + B).
 * Limits: 1 <= C <= 256, 1 <= V <= 4096, N_d < 2^31, b0 + B <= 2^31 - 1, B <= 4096 per call (sumsq_fx cannot overflow and
 *   mmm_replicate_summary takes rep_post; B = 0 runs the observed phase only), a QUERIED document has at most 4096 CSR entries (its
 *   prefix sums are staged in LDS), the q_mult of a group sum to less than 2^31, Q < 2^31.  D = 0 or Q = 0: MMM_OK, nothing written.
 *   MMM_ERR_ARG, nothing written: NULL pointers (group_fx may be NULL when G = 0, the replicate outputs when B = 0), a q_ptr that is no
 *   CSR, a query term >= V, a mult < 1, a group outside [-1, G), G < 0, B < 0, b0 < 0, b0 + B > 2^31 - 1, maxiter < 1, tol < 0 and the
 *   catalogue and corpus errors of mmm_refit_exposures.  MMM_ERR_UNSUPPORTED, with the limit in the message: C > 256, V > 4096,
 *   N_d >= 2^31, B > 4096, a queried document with more than 4096 entries, a group whose mults reach 2^31, Q >= 2^31.  No collective: on a
 *   multi-rank context it acts on its arrays. */
int mmm_attribute_mutations(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, const double* cat,
                            const uint8_t* allowed /* [D][C] or NULL */, const int64_t* q_ptr /* [D + 1] */, const int32_t* q_term,
                            const int32_t* q_mult, const int32_t* q_group /* [Q]; mult / group or NULL */, int G, int B, int b0, uint64_t seed,
                            uint32_t stream, int maxiter, double tol, double* w /* [D][C] */, double* post /* [Q][C] */, int8_t* status,
                            int64_t* iters /* [D] */, uint64_t* sum_fx, uint64_t* sumsq_fx /* [Q][C] */, int32_t* top_count /* [Q][C] */,
                            int32_t* void_count /* [Q] */, uint64_t* group_fx /* [B][G][C] */, double* rep_post /* [B][Q][C] or NULL */);

/* ---- did the exposures change between a tumour's two mutation sets (clonal / subclonal, early / late, primary / relapse)?  An exact
 * permutation test per sample, in one call (no counterpart in the reference).  Two CSR corpora over the same D
 * samples and V terms, cat and allowed as mmm_refit_exposures takes them; P, f, fit(A) with the order of its sums, ll(A) and u(A) are those
 * of mmm_refit_exposures, unchanged.
 * Per sample d.  n^a, n^b: the dense count vectors of the two corpora (duplicate terms summed); n = n^a + n^b the pooled vector; N_a, N_b,
 *   N = N_a + N_b their totals; A = {c : allowed[d][c]} (allowed == NULL: the whole catalogue).
 * Dealing.  Under H0 the two sets are draws from one mixture, so given the pooled counts the partition into sets of sizes N_a and N_b is a
 *   uniform random subset -- whatever was fitted: no null model is needed.  The N pooled mutations are numbered i = 0 .. N - 1 in term order
 *   of the DENSE pooled vector: with cum the inclusive prefix sums of n over v ascending, mutation i lies in the term v with
 *   cum[v-1] <= i < cum[v].  The key of mutation i in replicate b (the GLOBAL index b0 + ..., so chunked calls are slices of one big call) is
 *   k_i = u_i >> (32 - key_bits), u_i being output word i % 4 of the Philox4x32-10 block with the constants and the key (seed low, seed
 *   high) of mmm_resample_counts and the counter (i / 4, 0xD0000000 | d, b, stream).  High nibble 0xD of the second counter word is set by
 *   no other user of these words (mmm_extract_signatures 0x8, mmm_classify_exposures 0x9, mmm_survival_association 0xA, mmm_cox_exposures
 *   0xB, mmm_cluster_samples 0xC | k, mmm_associate_exposures 0xE; the resampler, the split and the simulator keep that word below 2^31),
 *   hence D <= 2^28, b < 2^31, stream < 2^31.  Set a of the replicate is the N_a mutations with the smallest (k_i, i) in lexicographic
 *   order; n^{a,b}_v = the number of those in term v, n^{b,b} = n - n^{a,b}.  So sum_v n^{a,b}_v = N_a exactly, 0 <= n^{a,b}_v <= n_v, and
 *   the arithmetic is integer throughout: the same arguments give the same bits on every run and under every launch geometry.
 *   key_bits in 1 .. 32.  With 32 the tie-break by index acts with probability about N / 2^32 per replicate and is not corrected, like the
 *   2^-32 resolution of the resampler.  SMALL VALUES ARE A TEST HOOK: they make ties at the threshold the rule, so that the tie path is
 *   run thousands of times per call, and they are BIASED towards low indices (with key_bits = 2 a quarter of the mutations share each key
 *   and the lowest indices of the threshold's group always win).  Callers pass 32.
 * Statistic of a pair (x, y) of count vectors (observed: (n^a, n^b); replicate: (n^{a,b}, n^{b,b})).  (w^x, ll_x, u_x) = fit(A) on x with
 *   f = x / N_a;  (w^y, ll_y, u_y) = fit(A) on y with f = y / N_b;  T = ll_x + ll_y (one rounding);  delta_c = |w^x_c - w^y_c| for c in A
 *   (0 outside), delta_max = max_c delta_c.  Once per sample (w^0, ll_0, u_0) = fit(A) on n with f = n / N.  stat[d] = max(2 (T_obs - ll_0), 0).
 *   Mutations on terms that no signature of A can produce drop out of all three log-likelihoods alike; unexplained[d] = u_0 reports them.
 *   With ONE signature in A every fit is w = 1 and T is the same for every partition up to rounding: count_ge of such a sample says nothing.
 * Counts over the B replicates of THIS call (the counts of chunked calls add):  count_ge[d] = #{b : T_b >= T_obs};  count_sig[d][c] =
 *   #{b : delta_{c,b} >= delta_{c,obs}};  count_max[d][c] = #{b : delta_{max,b} >= delta_{c,obs}} (single-step Westfall-Young max-T over the
 *   signatures of the sample; both 0 outside A).  p = (1 + count) / (B + 1) is the caller's.
 * status[d] = 3: untestable (N_a = 0, N_b = 0 or A empty) -- every other output of the sample is 0, no replicate is run (the caller's p is
 *   NaN); 0: tested.  w_a, w_b, w_pool [D][C]: w^x, w^y of the observed pair and w^0 (exactly 0 outside A).  iters[d]: the EM iterations of
 *   all the sample's fits, the replicates' of this call included.  rep_stat (or NULL): [b D + d] = 2 (T_b - ll_0), NaN for status 3.
 * The dealt counts, every weight, delta, count_sig, count_max, status and iters are decided by +, x, / and comparisons in a fixed order:
 *   the same bits on every run, under every launch geometry and wherever the catalogue is read from (LDS, or L2 where a sample's rows do
 *   not fit or under MMM_OFF_REFIT_LDS).  T, stat, count_ge and rep_stat pass through the device log (< 1 ulp per term), as ll of
 *   mmm_refit_exposures does.
 * Limits: 1 <= C <= 256, 1 <= V <= 4096, D <= 2^28, N_d < 2^31, b0 + B <= 2^31 - 1; B = 0 runs the observed phase only; D = 0 writes
 *   nothing.  MMM_ERR_ARG, nothing written: NULL pointers, key_bits outside 1 .. 32, B < 0, b0 < 0, b0 + B > 2^31 - 1, stream >= 2^31,
 *   maxiter < 1, tol < 0, either corpus not a CSR of terms < V, a negative count and the catalogue errors of mmm_refit_exposures.
 *   MMM_ERR_UNSUPPORTED, with the limit in the message: C > 256, V > 4096, D > 2^28, N_d >= 2^31.  No collective: on a multi-rank context
 *   both act on their arrays. */
/* The dealing alone, on ONE CSR corpus: mutations are numbered in CSR order of the entries, as mmm_split_counts numbers them, the counter
 * is the one above, and out[b nnz + e] (b < B, nnz = doc_ptr[D]) is the part of entry e that goes to set a of replicate b0 + b, n_a[d] of
 * the document's mutations in all.  For a corpus whose entries are in term order without duplicates this is the dealing above.
 * Replicates go through a bounded device buffer in chunks.  B = 0 or nnz = 0: MMM_OK, nothing written.  MMM_ERR_ARG also for an n_a[d]
 * outside [0, N_d]; no term array and no V limit here. */
int mmm_deal_counts(mmm_ctx* ctx, int D, const int64_t* doc_ptr, const int32_t* count, const int32_t* n_a /* [D] */, int B, int b0, uint64_t seed,
                    uint32_t stream, int key_bits, int32_t* out /* [B][nnz] */);
int mmm_compare_exposures(mmm_ctx* ctx, int D, int C, int V, const int64_t* doc_ptr_a, const int32_t* term_a, const int32_t* count_a,
                          const int64_t* doc_ptr_b, const int32_t* term_b, const int32_t* count_b, const double* cat,
                          const uint8_t* allowed /* [D][C] or NULL */, int B, int b0, uint64_t seed, uint32_t stream, int key_bits, int maxiter, double tol,
                          double* w_a, double* w_b, double* w_pool /* [D][C] */, double* stat /* [D] */, int32_t* count_ge /* [D] */,
                          int32_t* count_sig, int32_t* count_max /* [D][C] */, int8_t* status, double* unexplained, int64_t* iters /* [D] */,
                          double* rep_stat /* [B][D] or NULL */);

/* ---- exposure trajectories: where along a tumour's ORDERED mutations (by cancer cell fraction, by inferred timing) do the exposures
 * change, how many times, and is that more than chance?  Change points by optimal partitioning over a table of segment fits, and an exact
 * permutation test of the best single cut, in one call (no counterpart in the reference).
 * A CSR corpus of nbins BINS over V terms (doc_ptr [nbins + 1], term, count, as mmm_refit_exposures takes a corpus); bin_ptr [D + 1]: sample d
 * owns the bins bin_ptr[d] .. bin_ptr[d+1] - 1 in timeline order, T = T_d their number.  cat and allowed as mmm_refit_exposures takes them;
 * P, f, fit(A) with the order of its sums, ll(A) and u(A) are those of mmm_refit_exposures, unchanged.  L = min_len >= 1 (bins), M = max_cp >= 0.
 * Per sample d, A = {c : allowed[d][c]} (allowed == NULL: the whole catalogue).
 * Vectors.  n^t: the dense count vector of bin t (duplicate terms summed), N_t its total; c^t = sum_{s<t} n^s, c^0 = 0, c^T = n (the pooled
 *   vector, total N); C_t the total of c^t.
 * Segment table.  A segment (i, j), 0 <= i < j <= T, is the bins i .. j - 1; it is DEFINED when j - i >= L, and (0, T) is defined whatever L (a
 *   timeline shorter than L is one segment).  For a defined segment, x = c^j - c^i, N_ij its total: (w^{ij}, ll_ij, u_ij) = fit(A) on x with
 *   f = x / N_ij; N_ij = 0: w = 0, ll = 0, and no iteration is run.  Every defined segment is fitted exactly once.  seg_ll holds ll_ij at
 *   index i T - i (i - 1) / 2 + (j - i - 1) of the sample's block, which starts at sum_{d'<d} T_d' (T_d' + 1) / 2; NaN where the segment is
 *   not defined.
 * Optimal partitioning (on the host, on the table: O(M T^2) additions a sample).  F_0(j) = ll_0j;  F_m(j) = max_i F_{m-1}(i) + ll_ij (one
 *   rounding) over the i for which both are defined, i ascending, ties to the lowest i;  m <= min(M, max(floor(T / L) - 1, 0)).
 *   best[d][m] = F_m(T), NaN where it is not defined (and for every larger m <= M).  n_cp[d] = the m that maximises
 *   F_m(T) - (double)m * penalty[d] (one product, one subtraction) over the defined m, ties to the smallest m.  cp[d][k], k < n_cp, by
 *   backtracking: the first bin of segment k + 1; -1 beyond.  w_seg[d][k][.], k <= n_cp: the weights w^{ij} of the chosen segments (exactly
 *   0 outside A and in the rows beyond n_cp).  w_bin[bin][.] (or NULL): fit(A) on every bin alone.  Both are, bit for bit, what
 *   mmm_refit_exposures with penalty == NULL gives on the same count vector (every fit is a cold start).
 * Scan (T >= 2 L).  For the cuts t in [L, T - L]: G_t = ll_0t + ll_tT (one rounding, the values of the table); gain_cut[bin_ptr[d] + t] =
 *   G_t - ll_0T, NaN for every other t; G_max = max_t G_t; cut[d] = the lowest t that attains it; stat[d] = max(2 (G_max - ll_0T), 0).
 * Replicates.  Under H0 the exposures are constant along the timeline, so given the pooled counts the assignment of the N mutations to
 *   bins of sizes N_0 .. N_{T-1} is uniform.  The keys are exactly those of mmm_compare_exposures' dealing for sample d: mutations numbered
 *   in term order of the dense pooled vector, k_i from word i % 4 of the block with the counter (i / 4, 0xD0000000 | d, b, stream), b the
 *   GLOBAL index b0 + ..., key_bits as there (callers pass 32).  With the mutations ordered by (k_i, i), the replicate's prefix vector
 *   c^{t,b} counts, per term, the C_t smallest: it is what mmm_deal_counts gives for the pooled row with n_a = C_t under the same seed and
 *   stream, and the prefixes of one replicate are nested because they share the keys.  (The tag is shared with the two-set test on
 *   purpose, as mmm_presence_test shares the simulator's words: replicates can be reproduced through a shipped entry; a two-set test of
 *   the same sample index under the same seed and stream is correlated with this one.)
 *   G_{t,b} = ll(fit(A) on c^{t,b}) + ll(fit(A) on n - c^{t,b}) (a side without mutations: ll = 0, no iteration); G_{max,b} the maximum over
 *   the same cuts.  count_ge[d] = #{b : G_{max,b} >= G_max};  count_cut[bin_ptr[d] + t] = #{b : G_{max,b} >= G_t}, the single-step max-T
 *   adjusted count of cut t, 0 for every other t.  Both over the B replicates of THIS call (the counts of chunked calls add).
 *   rep_stat (or NULL): [b D + d] = 2 (G_{max,b} - ll_0T), NaN for the samples that are not tested.
 * status[d] = 3: N = 0 or A empty -- seg_ll, best and gain_cut of the sample are NaN, cp and cut -1, everything else 0;  1: T < 2 L -- table,
 *   partitioning (n_cp = 0 necessarily) and weights are computed, there is no scan and there are no replicates (cut -1, stat 0, gain_cut
 *   NaN, counts 0);  0: tested.  unexplained[d] = u_0T.  iters[d] = the EM iterations of the table's fits plus those of this call's
 *   replicate fits; the fits that produce w_bin and w_seg are not counted.
 * The dealt vectors, every weight, status, unexplained and iters are decided by +, x, / and comparisons in a fixed order: the same bits on
 *   every run, under every launch geometry and wherever the catalogue is read from (LDS, or L2 where a sample's rows do not fit or under
 *   MMM_OFF_REFIT_LDS).  seg_ll, best, gain_cut, stat, cut, n_cp, cp, the counts and rep_stat pass through the device log (< 1 ulp per
 *   term), as ll of mmm_refit_exposures does; given seg_ll, the partitioning and the scan are exact double arithmetic in the order above.
 *   With ONE signature in A every fit is w = 1 and every G is the same up to rounding: cut, the counts and the change points of such a
 *   sample say nothing.
 * Limits: 1 <= C <= 256, 1 <= V <= 4096, D <= 2^28, N_d < 2^31, b0 + B <= 2^31 - 1, T_d <= 128 (MMM_TRAJECTORY_MAX_BINS); B = 0 runs the
 *   observed part only; D = 0 or nbins = 0 writes nothing.  MMM_ERR_ARG, nothing written: NULL pointers (cp may be NULL when max_cp = 0), a
 *   bin_ptr that does not start at 0, decreases or does not end at nbins, min_len < 1, max_cp < 0, a penalty that is negative or not finite
 *   and the argument errors of mmm_compare_exposures.  MMM_ERR_UNSUPPORTED, with the limit in the message: C > 256, V > 4096, D > 2^28,
 *   T_d > 128, N_d >= 2^31.  No collective: on a multi-rank context it acts on its arrays. */
#define MMM_TRAJECTORY_MAX_BINS 128
int mmm_exposure_trajectory(mmm_ctx* ctx, int D, int C, int V, int nbins, const int64_t* doc_ptr, const int32_t* term, const int32_t* count,
                            const int64_t* bin_ptr /* [D + 1] */, const double* cat, const uint8_t* allowed /* [D][C] or NULL */, int min_len, int max_cp,
                            const double* penalty /* [D] */, int B, int b0, uint64_t seed, uint32_t stream, int key_bits, int maxiter, double tol,
                            double* seg_ll /* [sum_d T_d (T_d + 1) / 2] */, double* best /* [D][max_cp + 1] */, int32_t* n_cp /* [D] */,
                            int32_t* cp /* [D][max_cp] */, double* w_seg /* [D][max_cp + 1][C] */, double* w_bin /* [nbins][C] or NULL */,
                            double* gain_cut /* [nbins] */, int32_t* cut /* [D] */, double* stat /* [D] */, int32_t* count_ge /* [D] */,
                            int32_t* count_cut /* [nbins] */, int8_t* status, double* unexplained, int64_t* iters /* [D] */,
                            double* rep_stat /* [B][D] or NULL */);

/* ---- signatures as sparse non-negative mixtures of catalogue rows: for every size s <= S the best subset of exactly s rows, by exhaustive
 * search (the step between extraction and assignment; no counterpart in the reference).
 * n signatures sig [n][V] and a catalogue cat [C][V], every entry finite and >= 0; rows need not be normalised.
 * Stage 1, moments.  G[c][c'] = sum_v cat[c][v] cat[c'][v];  b[i][c] = sum_v sig[i][v] cat[c][v];  ss[i] = sum_v sig[i][v]^2.  Each sum in
 *   the order of mmm_signature_cosine's sums: 64 partial sums, partial l over v = l, l + 64, ... ascending from 0.0, combined inside the 16-lane
 *   rows as l with l ^ 1, ^ 2, the other quad pair, the other half, then the rows as (row 0 + row 2) + (row 1 + row 3).  Products and sums are
 *   separate roundings.  G is symmetric by construction: the entries c <= c' are computed and written to both places.
 * Stage 2, search, on (G, b, ss) alone.  For a subset c_1 < ... < c_s with g_ij = G[c_i][c_j] and beta_i = b[c_i], row by row for i = 0 .. s-1
 *   (every product, difference and reciprocal one IEEE rounding):
 *     u_ij = g_ij - sum_{p<j} u_ip l_jp for j < i, sequentially with p ascending: ((g - t_0) - t_1) - ...;   l_ij = u_ij r_j;
 *     d_i = g_ii - sum_{p<i} u_ip l_ip;   r_i = 1 / d_i (one correctly rounded division per pivot, the only division);
 *     y_i = beta_i - sum_{p<i} l_ip y_p;   z_i = y_i r_i;
 *   gain = sum_i y_i z_i, i ascending, starting from y_0 z_0;  then for i = s-1 .. 0:  w_i = z_i - sum_{p>i} l_pi w_p, p ascending.
 *   Row i uses the rows before it only, so two subsets with a common prefix share its numbers bit for bit.
 *   The subset is ADMISSIBLE when every d_i > 2^-26 g_ii (otherwise row c_i lies in the span of the earlier ones: a duplicated or scaled
 *   catalogue row, an exact blend) and every w_i > 0.  best[s] = the admissible subset of size EXACTLY s with the largest gain, ties to the
 *   lexicographically smallest (c_1, ..., c_s): the maximum of a total order, independent of the order in which subsets are visited or reduced.
 *   A weight of an NNLS solution that is 0 makes it the solution on a smaller subset, which is enumerated too: the best non-negative
 *   reconstruction with AT MOST s rows is the running maximum of gain over the sizes <= s, its squared residual ss - gain and its cosine to
 *   the signature sqrt(gain / ss).
 * Outputs per (i, s), s = 1 .. S:  subset[(i S + s-1) S + j] (j < S; -1 beyond the s members), weight likewise (0 beyond), gain[i S + s-1],
 *   cosine[i S + s-1] = sqrt(min(gain / ss, 1)).  No admissible subset of size s, ss = 0 or s > C: subset -1, weight 0, gain 0, cosine 0.
 *   The same arguments give the same bits on every run, whatever n and wherever G and b are held (LDS, or read through L2 when C > 128).
 * Limits: 1 <= S <= 6, 1 <= C <= 256, binom(C, min(S, C)) < 2^32, V >= 1, n >= 0 (n = 0 computes the moments asked for and nothing else).
 *   MMM_ERR_UNSUPPORTED, with the limit in the message: S > 6, C > 256, binom(C, min(S, C)) >= 2^32.  MMM_ERR_ARG: NULL pointers, S < 1, C < 1,
 *   n < 0, V < 1, a negative or non-finite entry of sig or cat, a catalogue row that is all zero.  Moments that are not finite (caller-supplied,
 *   or finite inputs whose products overflow) or ss < 0: an entry of G marks every signature, one of b[i] or ss[i] marks signature i; a marked
 *   signature comes out empty (subset -1), the others are computed, and the call returns MMM_ERR_ARG naming the first.
 *   No collective: on a multi-rank context both act on the arrays they are given. */
int mmm_decompose_search(mmm_ctx* ctx, int n, int C, int S, const double* G /* [C][C] */, const double* b /* [n][C] */, const double* ss /* [n] */,
                         int32_t* subset /* [n][S][S] */, double* weight /* [n][S][S] */, double* gain /* [n][S] */, double* cosine /* [n][S] */);
/* Stage 1 on the device, then stage 2 on its moments.  G_out [C][C], b_out [n][C], ss_out [n]: the moments, each may be NULL. */
int mmm_signature_decompose(mmm_ctx* ctx, int n, int C, int V, const double* sig, const double* cat, int S, int32_t* subset, double* weight, double* gain,
                            double* cosine, double* G_out, double* b_out, double* ss_out);

/* ---- new signatures beside a FIXED catalogue: the F catalogue rows are held, J free rows are learned, R restarts in one call ("fit and
 * extract"; F = 0 is plain KL-NMF / pLSA extraction, J = 0 the plain refit; no counterpart in the reference).
 * CSR corpus of D documents over V terms and cat [F][V] as mmm_refit_exposures takes them, with its checks and its index-order normalisation to
 * P (F = 0: cat may be NULL); allowed [D][F] or NULL = all (the free rows are always allowed); K = F + J rows in all, the fixed ones first.
 * n_dv, N_d, f_dv = n_dv / N_d, the 64 `partials` (partial l over the indices l, l + 64, ... ascending from 0.0), the `butterfly` that combines
 * them (l with l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1) and the mixture, sequential over the rows ascending, are those of mmm_refit_exposures.
 * Start of restart r (GLOBAL index r0 + r).  Rows 0 .. F-1 of P are the normalised catalogue, row F + j is the free row Q_j:
 *   from init [R][J][V]: entries finite and >= 0, every row sum > 0, each row divided by its sum in index order;
 *   init == NULL: Q0_jv = (u + 1) 2^-32 (exact in a double), u being output word v % 4 of the Philox4x32-10 block with the constants and the key
 *   (seed low 32 bits, seed high 32 bits) of mmm_resample_counts and the counter (v / 4, 0x80000000 | j, r0 + r, stream); Q0_j is then divided by
 *   its sequential sum over v.  mmm_resample_counts, mmm_split_counts, mmm_simulate_counts and mmm_presence_test all put a document or item
 *   index in the second counter word, an int >= 0 and so below 2^31: a start shares no random word with any of them, whatever the stream.
 *   A_d = the allowed fixed rows and all free rows; w_dk = 1 / |A_d| on A_d, 0 elsewhere.  A document with N_d = 0 or an empty A_d keeps w = 0
 *   and enters no sum.
 * Iteration t = 1 .. maxiter, all documents jointly:
 *   q_dv = sum_k w_dk P_kv, k ascending;  r_dv = f_dv / q_dv where n_dv > 0 and q_dv > 0, else 0;  g_dk = butterfly(partials(r_d. o P_k.));
 *   w'_dk = w_dk g_dk.
 *   Free rows, with a_dj = N_d w_d,F+j (the OLD w):  s_jv = sum_d a_dj r_dv, every product rounded, then added, in this order: document d
 *   belongs to stripe d mod 16; a stripe's sum runs over its documents in ascending d from 0.0; the 16 stripe sums are then added in ascending
 *   stripe order from 0.0.  t_jv = Q_jv s_jv;  z_j = butterfly(partials(t_j.));  Q'_jv = t_jv / z_j if z_j > 0, else Q_jv.
 *   Stop after an iteration with max(max_dk |w' - w|, max_jv |Q' - Q|) < tol (strict: tol = 0 runs maxiter iterations).
 * Finish, per document as fit(A) of mmm_refit_exposures: w_d <- w_d / S_d if S_d > 0, S_d the sequential sum over k; q recomputed;
 *   ll_doc = sum over n_dv > 0, q_dv > 0 of n_dv log q_dv (partials and butterfly); unexplained = sum over n_dv > 0, q_dv = 0 of n_dv (N_d
 *   for a document that entered no sum, whose other outputs are 0); ll[r] = sum_d ll_doc in stripe order (as s_jv).
 * Products, sums and the (IEEE, correctly rounded) divisions are separate roundings.  All terms are >= 0, so padding, a zero weight and an
 *   absent document change no bit.  The stripe count 16 belongs to the definition, not to the launch: every launch geometry (`waves`, the
 *   number of restarts in flight, w held in LDS or in memory) gives the same bits, and so does every run.  Only +, x, / and comparisons decide
 *   sig, w, iters and unexplained; log (the device library's, < 1 ulp) enters ll and ll_doc only.
 * Consequences.  (a) J = 0, tol = 0: w, ll_doc and unexplained of every document are those of mmm_refit_exposures with penalty = NULL and the
 *   same maxiter (with tol > 0 the refit stops per document, this per restart).  (b) A call with (r0, R) is a slice of the call with
 *   (0, r0 + R) (with init: of its rows).  (c) F = 0: multiplicative KL-NMF / pLSA with normalised rows.
 * Outputs: sig [R][J][V] the free rows; w [R][D][K] the normalised weights (or NULL); ll [R]; ll_doc, unexplained [R][D] (or NULL);
 *   iters [R] the iterations run.  waves: the waves of a block, a pinned geometry for tests (0 = the library's choice, else 1, 2, 4, 8 or 16).
 * Limits: 1 <= K <= 256, J <= 32, V >= 1, D K < 2^31, D V < 2^31, r0 + R <= 2^31 - 1; P and one r vector per wave are held in LDS:
 *   8 (K V + waves V) + 4 K + 392 bytes may not exceed 160 KiB (the library's choice, 16 waves for K <= 16 and 8 beyond, halves the waves until they fit).  One block
 *   runs a restart: a call with few restarts and very many documents uses few CUs.
 * MMM_ERR_ARG, nothing written: NULL pointers (ctx, cat with F > 0, sig with J > 0, ll, iters, the CSR arrays), D < 0, F < 0, J < 0, K < 1,
 *   V < 1, R < 0, r0 < 0, r0 + R > 2^31 - 1, maxiter < 1, tol < 0 or NaN, waves not one of 0, 1, 2, 4, 8, 16, an init entry that is negative
 *   or not finite, an init row whose sum is 0, and the catalogue and corpus errors of mmm_refit_exposures.  MMM_ERR_UNSUPPORTED, with the limit
 *   in the message: K > 256, J > 32, D K or D V >= 2^31, more LDS than a block may take.  D = 0 or R = 0: MMM_OK, nothing written.  No
 *   collective: on a multi-rank context it acts on its arrays. */
int mmm_extract_signatures(mmm_ctx* ctx, int D, int F, int J, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count,
                           const double* cat /* [F][V] or NULL if F = 0 */, const uint8_t* allowed /* [D][F] or NULL */, int R, int r0, uint64_t seed,
                           uint32_t stream, const double* init /* [R][J][V] or NULL */, int maxiter, double tol, int waves, double* sig /* [R][J][V] */,
                           double* w /* [R][D][K] or NULL */, double* ll /* [R] */, double* ll_doc, double* unexplained /* [R][D] or NULL */,
                           int32_t* iters /* [R] */);

/* ---- groups of samples: consensus k-means (Monti et al. 2003) of D samples on P features, B subsampled replicates for each of nk candidate
 * numbers of groups in one call, then the pair counts and the inputs of PAC, the proportion of ambiguously clustered pairs (no counterpart in
 * the reference).  x [D][P]: a sample's features, already transformed by the caller.  ks [nk]: the numbers of groups.
 * Subsample of replicate b (GLOBAL index b0 + b).  keep == 0: every sample is a member.  Otherwise sample d is a member iff w < keep, w being
 *   output word d % 4 of the Philox4x32-10 block with the constants and the key (seed low 32 bits, seed high 32 bits) of mmm_resample_counts
 *   and the counter (d / 4, 0xC0000000, b0 + b, stream).  The members in ascending d are a = 0 .. n-1; the same subsample serves every k of the
 *   replicate.  Bit 30 of the second counter word is set by no other user of these words: mmm_extract_signatures uses 0x80000000 | j with
 *   j < 32, all others an index below 2^31 -- a subsample or a start shares no random word with any of them, whatever the stream.
 * Distance.  dist(x, m) = sum_p (x_p - m_p)^2, p ascending from 0.0; each difference, product and sum is rounded separately.
 * Start of the pair (b, k): k-means++ by integer thresholds.  u_i, i < k, is output word i % 4 of the block with the counter
 *   (i / 4, 0xC0000000 | k, b0 + b, stream).  Centre 0 is member floor(u_0 n / 2^32); md_a = dist(x_a, centre 0).  For i = 1 .. k-1: cum_a = the
 *   inclusive sum of md over a ascending, strictly sequential from 0.0; S = cum_{n-1}.  S > 0: T_a = floor((cum_a / S) * 2^32) (an IEEE division;
 *   the product is exact), and centre i is the first member a with T_a > u_i -- it exists because T_{n-1} = 2^32, and it is never a member with
 *   md_a = 0, whose T_a = T_{a-1}.  S = 0 (every member coincides with a centre): centre i is the lowest a that is not yet the member of a
 *   centre.  Then md_a = min(md_a, dist(x_a, centre i)).  A centre is a copy of its member's row.
 *   n < k: the pair is SKIPPED -- its labels are all -1, iters 0, inertia 0.
 * Iteration t = 1 .. maxiter.  Every member's label becomes the centre with the smallest dist, ties to the lowest centre.  If no label changed,
 *   stop (in iteration 1 every label counts as changed).  Otherwise centre c becomes (the sum of its members' rows) / count_c, an IEEE division
 *   per feature, the sum in the order of mmm_extract_signatures: sample d (its index in x, not a) belongs to stripe d mod 16; a stripe's sum runs
 *   over its members of the centre in ascending d from 0.0; the 16 stripe sums are then added in ascending stripe order from 0.0.  A centre
 *   without members keeps its value.  iters = the iterations run (the stopping one included); iters == maxiter: the pair did not settle.
 *   inertia = the sum over the members of their smallest dist at the LAST assignment, in the same stripe order.
 * Pair counts over the B replicates of THIS call (the counts of chunked calls add), integers: together[k][i][j] = the number of replicates b
 *   in which i and j are both members and the pair (b, k) was not skipped (the diagonal: how often i was drawn in such a replicate);
 *   same[k][i][j] = the number of those in which their labels are equal.  together is kept per k because the skipped pairs differ per k: so
 *   0 <= same <= together holds entry by entry, same is symmetric, same[k][i][i] = together[k][i][i].
 * PAC inputs, in 64-bit integers, over the pairs i < j: valid[k] = #{together > 0}; ambiguous[k] = #{1000 same > pac_lo together and
 *   1000 same < pac_hi together} (per mille bounds of the consensus same / together).  The quotient ambiguous / valid is the caller's.
 * Only +, -, x, /, comparisons and integers decide every output: the same arguments give the same bits on every run and under every launch
 *   geometry (`waves`, `placement`, the number of pairs in flight).  Consequences.  (a) labels, iters and inertia of a call with (b0, B) are a
 *   slice of the call with (0, b0 + B).  (b) together and same are additive: counts(0, B1 + B2) = counts(0, B1) + counts(B1, B2); valid and
 *   ambiguous of the whole follow from the summed counts by the rule above.
 * Outputs: labels [nk][B][D] int8, -1 = not a member or skipped; iters, inertia [nk][B]; together, same [nk][D][D] uint32, ambiguous, valid [nk]
 *   int64, each of the four may be NULL (all four NULL: the pair pass does not run).
 * waves: the waves of a block, a pinned geometry for tests (0 = the library's choice, 8; else 1, 2, 4, 8 or 16).  placement: 0 = the library's
 *   choice -- the members' rows, md, cum, the labels, the member lists and the 16 stripe slabs of the centre sums are held in LDS when
 *   8 (kmax P + 16) + 2328 + 8 (2 D + 16 kmax P + D (P | 1)) + 12 D bytes do not exceed 160 KiB (kmax = the largest k), and in a per-block
 *   workspace in memory otherwise; 1 = in LDS where they fit (the same as 0); 2 = in memory.
 * Limits: 1 <= D <= 4096, 1 <= P <= 256, 1 <= nk <= 16, 1 <= k <= 32, nk B D < 2^31, b0 + B <= 2^31 - 1.  Every entry of x is finite with
 *   |x| <= 1e150, which keeps every square and every sum of the definition finite.
 * MMM_ERR_ARG, nothing written: NULL pointers (ctx, x, ks; labels, iters, inertia with B > 0), D < 1, P < 1, nk < 1, a k < 1, B < 0, b0 < 0,
 *   b0 + B > 2^31 - 1, maxiter < 1, not 0 <= pac_lo < pac_hi <= 1000, waves not one of 0, 1, 2, 4, 8, 16, placement not 0, 1 or 2, an entry of x
 *   that is not finite or beyond 1e150.  MMM_ERR_UNSUPPORTED, with the limit in the message: D > 4096, P > 256, nk > 16, a k > 32,
 *   nk B D >= 2^31.  B = 0: MMM_OK, nothing written.  No collective: on a multi-rank context it acts on its arrays. */
int mmm_cluster_samples(mmm_ctx* ctx, int D, int P, const double* x /* [D][P] */, int nk, const int32_t* ks /* [nk] */, int B, int b0, uint32_t keep,
                        uint64_t seed, uint32_t stream, int maxiter, int pac_lo, int pac_hi, int waves, int placement, int8_t* labels /* [nk][B][D] */,
                        int32_t* iters, double* inertia /* [nk][B] */, uint32_t* together, uint32_t* same /* [nk][D][D] or NULL */,
                        int64_t* ambiguous, int64_t* valid /* [nk] or NULL */);

/* ---- exposures against sample covariates: rank statistics of P features against C covariates over D samples, with B permutations of the
 * covariate rows (within strata) for exact p-values under ties and Westfall-Young max-T adjustment (no counterpart in the reference;
 * DESIGN.md section 4.19).  x [D][P]: a sample's features.  y [D][C]: its covariates.  levels [C]: 0 = covariate c is numeric and owns one
 * column; G >= 1 = categorical, y[d][c] is an integral code in 0 .. G-1 and the covariate owns G indicator columns.  Q = the sum of the
 * column counts; the columns stand in covariate order.
 * Doubled midranks.  For n values v: r2_d = 2 #{e : v_e < v_d} + #{e : v_e = v_d} + 1, the comparisons IEEE (-0.0 equals 0.0): integers in
 *   2 .. 2n whose sum is n (n + 1), whose mean is exactly n + 1.  Rx[d][p] = r2 of feature p over all D samples.  Y[d][q] = r2 of the covariate
 *   for a numeric column; for the indicator column of level g, 1 if the code is g, else 0.  Both fit 16 bits; the library forms them on the host.
 * Weights, integers all.  SSx_p = sum_d (Rx[d][p] - (D + 1))^2.  w_q = sum_d (Y[d][q] - (D + 1))^2 for a numeric column, n_g (the number of
 *   samples with code g) for an indicator column.
 * Permutation of replicate b (GLOBAL index b0 + b).  key_d = output word d % 4 of the Philox4x32-10 block with the constants and the key
 *   (seed low 32 bits, seed high 32 bits) of mmm_resample_counts and the counter (d / 4, 0xE0000000, b0 + b, stream).  Bits 31, 30 and 29 of
 *   the second counter word together are set by no other user of these words: mmm_extract_signatures uses 0x80000000 | j with j < 32,
 *   mmm_cluster_samples 0xC0000000 | k with k <= 32, mmm_survival_association 0xA0000000 (bit 30 clear), mmm_classify_exposures 0x90000000
 *   (bits 30 and 29 clear, bit 28 set), mmm_cox_exposures 0xB0000000 (bit 30 clear), all others (the resampler, the
 *   split, the simulator) an index below 2^31 -- a permutation shares no random word with any of them, whatever the stream.  s_d = strata[d], or 0 without strata.  slot_0 .. slot_{D-1}
 *   are the samples in ascending (s_d, d); e_0 .. e_{D-1} the samples in ascending (s_d, key_d, d); pi(slot_j) = e_j.  Both lists carry the
 *   same sequence of strata, so pi maps every stratum onto itself.  Equal keys are ordered by d: the orders of a stratum are not exactly
 *   equally likely, the bias is below D^2 / 2^33 (the chance that two of D keys coincide) and is accepted.
 * Statistic.  Z_b[p][q] = sum_i Rx[i][p] Y[pi(i)][q]: sample i keeps its features and receives the covariate row of pi(i); an integer.
 *   Zc = Z_b[p][q] - (D + 1) sum_d Y[d][q]; |Zc| <= 2^38 at D = 4096.  t_b[p][c] = (the sum over the columns q of c, ascending, from 0.0,
 *   skipping w_q = 0, of ((double)Zc (double)Zc) / (double)w_q) / (double)SSx_p; the product, every division and every sum is rounded
 *   separately; t = 0 when SSx_p = 0 (a constant feature).  (D - 1) t is the tie-corrected Kruskal-Wallis H of a categorical covariate (with
 *   two levels the squared Wilcoxon rank-sum z) and (D - 1) rho^2, rho Spearman's coefficient, of a numeric one; the scaling is the caller's.
 * Outputs.  obs [P][C] and zc_obs [P][Q] (or NULL): t and Zc under the identity permutation, formed by the same device code.
 *   ge[p][c] = #{b in this call : t_b[p][c] >= obs[p][c]}.  M_b[c] = max_p t_b[p][c], within a covariate only: statistics of covariates with
 *   different numbers of levels are not on one scale.  ge_max[p][c] = #{b : M_b[c] >= obs[p][c]}.  maxstat [B][C] (or NULL) = M_b[c].
 * Everything the device sums is an integer; t is formed by one thread in the written order, maxima and comparisons are exact.
 *   Consequences.  (a) Every output is the same bits on every run and under every `waves`.  (b) maxstat of a call with (b0, B) is a slice of
 *   the call with (0, b0 + B).  (c) ge and ge_max of chunked calls add.  (d) obs and zc_obs do not depend on B, b0, seed or stream.
 *   (e) If every stratum has one member, every pi is the identity, t_b = obs and ge = ge_max = B everywhere (a maximum is no smaller than any obs).
 * waves: the waves of a block, a pinned geometry for tests (0 = the library's choice, 4; else 1, 2, 4, 8 or 16).
 * Limits: 1 <= D <= 4096, 1 <= P <= 256, 1 <= C, Q <= 256, b0 + B <= 2^31 - 1, 0 <= strata[d] < D.
 * MMM_ERR_ARG, nothing written: NULL pointers (ctx, x, levels, y, obs; ge and ge_max with B > 0), D < 1, P < 1, C < 1, a negative level,
 *   B < 0, b0 < 0, b0 + B > 2^31 - 1, an x or y that is not finite, a categorical y that is not an integer in 0 .. G-1, a stratum out of range,
 *   waves not one of 0, 1, 2, 4, 8, 16.  MMM_ERR_UNSUPPORTED, with the limit in the message: D > 4096, P > 256, Q > 256.  B = 0: obs and
 *   zc_obs are written, the counts are untouched, MMM_OK.  No collective: on a multi-rank context it acts on its arrays. */
int mmm_associate_exposures(mmm_ctx* ctx, int D, int P, const double* x /* [D][P] */, int C, const int32_t* levels /* [C] */,
                            const double* y /* [D][C] */, const int32_t* strata /* [D] or NULL */, int B, int b0, uint64_t seed, uint32_t stream,
                            int waves, double* obs /* [P][C] */, int64_t* zc_obs /* [P][Q] or NULL */, uint32_t* ge, uint32_t* ge_max /* [P][C] */,
                            double* maxstat /* [B][C] or NULL */);

/* ---- exposures against survival: permutation tests of P features and C group covariates against a right-censored time-to-event outcome
 * over D samples, B permutations of the outcome rows (within strata): the log-rank test of every group covariate, the Cox score (trend) test
 * of every ranked feature with max-T adjustment over the features, and the maximally selected log-rank statistic over every cutpoint of a
 * feature, its p-value corrected for the scan by permuting the whole scan (no counterpart in the reference).
 * x [D][P]: a sample's features.  groups [D][C]: its codes, groups[d][c] in 0 .. levels[c]-1 (NULL iff C == 0); Q = the sum of the levels.
 * time [D] >= 0, event [D] in {0, 1} (1 = the event was seen at time, 0 = censored there).  strata [D] or NULL.
 * Strata.  s_d = strata[d], or 0 without strata.  A stratum is a code with at least one member; n_s its size.
 * Scores, per stratum s.  u_1 < u_2 < .. are the distinct times of the stratum's events (IEEE comparisons), d_j = #{i in s : event_i = 1,
 *   time_i = u_j}, n_j = #{i in s : time_i >= u_j}.  H_i = the sum over the j with u_j <= time_i, ascending, from 0.0, of (double)d_j /
 *   (double)n_j, every quotient and every sum rounded separately (the Nelson-Aalen estimate at time_i).  a_i = (double)event_i - H_i, the
 *   log-rank (Savage) score.  A_i = rint(a_i 2^24), ties to even, an int32: H < 1 + ln 4096 < 9.4, so |A_i| < 2^27.3.  Any fixed score
 *   vector gives a valid permutation test, so the quantisation costs nothing statistically, and every sum below is an exact integer.
 * Features.  Rx[d][p] = the doubled midranks of mmm_associate_exposures (2 #{less} + #{equal} + 1 over all D samples; 16 bits).  o_p = the
 *   samples in ascending (x[.][p], d), the comparisons IEEE (-0.0 equals 0.0).
 * Permutation of replicate b (GLOBAL index b0 + b): pi exactly as in mmm_associate_exposures (slot, key and e lists, ties by d), with the
 *   second Philox counter word 0xA0000000: bits 31 and 29 without bits 30 and 28 are set by no other user of these words (mmm_extract_signatures
 *   uses 0x80000000 | j with j < 32, mmm_cluster_samples 0xC0000000 | k with k <= 32, mmm_associate_exposures 0xE0000000,
 *   mmm_classify_exposures 0x90000000, mmm_cox_exposures 0xB0000000 (bit 28 set as well), all others an index
 *   below 2^31).  Sample i keeps its features and groups and receives the score of pi(i): Api_i = A[pi(i)].
 * One rule for every test column, an integer column f over the samples.  T_b(f) = sum_i f_i Api_i, an integer.  With F_s = the sum of f over
 *   stratum s and SA_s = the sum of A over it: E(f) = the sum over the strata, in ascending code, from 0.0, of ((double)F_s (double)SA_s) /
 *   (double)n_s.  With NF_s = n_s sum f^2 - F_s^2 and NA_s = n_s sum A^2 - SA_s^2, formed exactly as integers (NA_s needs 128 bits) and
 *   converted to double by round-to-nearest-even: V(f) = the sum over the strata with n_s >= 2, in ascending code, from 0.0, of
 *   ((double)NF_s (double)NA_s) / (((double)n_s (double)n_s) (double)(n_s - 1)).  Every product, division and sum is rounded separately.
 *   t_b(f): dz = (double)T_b - E, t = (dz dz) / V; where V is not > 0, t is 0 and the column is skipped in sums and maxima.  |T| < 2^53 in
 *   every family (Rx <= 2^13, D <= 2^12, |A| < 2^27.3): the conversion is exact.  E and V are the exact mean and variance of T under the
 *   within-stratum permutation; the host forms them once per call.
 * Trend.  f = Rx[.][p]: the Cox score test on the ranked feature in its permutation form.  z_trend[p] = T under the identity.
 * Group.  t_b[c] = the sum over the levels g of covariate c, ascending, from 0.0, of t_b(the indicator of code g).  u_group[q] = T of the
 *   indicator under the identity = 2^24 (O_g - E_g), observed minus expected events of the level.  With two levels and no strata t / 2 is
 *   the log-rank chi-square with the permutation variance; with more levels t is the sum of the one-against-rest statistics.
 * Cut.  On iff m_lo >= 1.  For j = 1 .. D-1, f_j = the indicator of {o_p(0) .. o_p(j-1)}.  Cut j is allowed iff x[o_p(j-1)][p] <
 *   x[o_p(j)][p] and m_lo <= j <= D - m_lo.  t_b^cut[p] = the maximum over the allowed j with V(f_j) > 0 of t_b(f_j), 0 if there is none.
 *   cut_at[p] = the lowest such j that attains the maximum under the identity, 0 if there is none: x > x[o_p(cut_at - 1)][p] is "high".
 * Outputs.  obs_trend [P], obs_group [C], obs_cut [P]: the statistics under the identity, formed by the same device code (a launch of one
 *   block with pi = the identity), as are z_trend [P] (or NULL), u_group [Q] (or NULL) and cut_at [P].  Every ge.. = #{b in this call : t_b >=
 *   obs}: ge_trend [P], ge_cut [P], ge_group [C].  M_b^trend = max_p t_b^trend[p], M_b^cut = max_p t_b^cut[p] (0 with the cuts off);
 *   gemax_trend[p] = #{b : M_b^trend >= obs_trend[p]}, gemax_cut likewise.  maxstat [B][2] (or NULL) = (M_b^trend, M_b^cut).  A group
 *   covariate has one statistic and gets ge only.  With m_lo = 0 obs_cut, cut_at, ge_cut and gemax_cut may be NULL and are not written.
 * Consequences.  (a) Every output is the same bits on every run and under every `waves`.  (b) maxstat of a call with (b0, B) is a slice of
 *   the call with (0, b0 + B).  (c) The counts of chunked calls add.  (d) Every obs.., z_trend, u_group and cut_at is independent of B, b0,
 *   seed and stream.  (e) If every stratum has one member, every V is 0, every statistic is 0 and every count equals B.  (f) Without events
 *   every A_i is 0, every V is 0, and (e) holds as well.
 * waves: the waves of a block, a pinned geometry for tests (0 = the library's choice, 4; else 1, 2, 4, 8 or 16).
 * Limits: 1 <= D <= 4096, 1 <= P <= 256, 0 <= C, levels >= 1, Q <= 256, at most 64 distinct strata (the host's per-cut constants cost
 *   O(P D 64)), 0 <= strata[d] < D, b0 + B <= 2^31 - 1, 0 <= m_lo <= max(1, D / 2) (m_lo = 1 is accepted at every D; D = 1 has no cut).
 * MMM_ERR_ARG, nothing written: NULL pointers (ctx, x, time, event, obs_trend; levels, groups, obs_group with C > 0; obs_cut, cut_at with
 *   m_lo >= 1; the counts of the families that are on with B > 0), D < 1, P < 1, C < 0, a level < 1, B < 0, b0 < 0, b0 + B > 2^31 - 1, m_lo
 *   out of range, an x that is not finite, a time that is not finite or is negative, an event other than 0 or 1, a code outside 0 .. G-1, a
 *   stratum outside 0 .. D-1, waves not one of 0, 1, 2, 4, 8, 16.  MMM_ERR_UNSUPPORTED, with the limit in the message: D > 4096, P > 256,
 *   Q > 256, more than 64 distinct strata.  B = 0: the obs.. outputs are written, the counts and maxstat are untouched, MMM_OK.  Every
 *   argument is checked before a device is asked for.  No collective: on a multi-rank context it acts on its arrays. */
int mmm_survival_association(mmm_ctx* ctx, int D, int P, const double* x /* [D][P] */, int C, const int32_t* levels /* [C] */,
                             const int32_t* groups /* [D][C] or NULL */, const double* time /* [D] */, const uint8_t* event /* [D] */,
                             const int32_t* strata /* [D] or NULL */, int m_lo, int B, int b0, uint64_t seed, uint32_t stream, int waves,
                             double* obs_trend /* [P] */, int64_t* z_trend /* [P] or NULL */, double* obs_group /* [C] */,
                             int64_t* u_group /* [Q] or NULL */, double* obs_cut /* [P] */, int32_t* cut_at /* [P] */, uint32_t* ge_trend,
                             uint32_t* gemax_trend, uint32_t* ge_cut, uint32_t* gemax_cut /* [P] each */, uint32_t* ge_group /* [C] */,
                             double* maxstat /* [B][2] or NULL */);

/* ---- a binary label against the exposures together: the cross-validated AUC of a ridge-penalised logistic regression of y on P features
 * over D samples, for L penalties, with B permutations of the feature rows (within strata); the maximum over the penalties is permuted with
 * the rest, so the p-value of the best penalty covers its choice (no counterpart in the reference).
 * x [D][P]: a sample's features, as given (the Python layer standardises them).  y [D] in {0, 1}.  strata [D] or NULL.  fold [R][D]: the fold
 * (< F) of sample i in repeat r, formed by the caller.  lambda [L], each > 0 and finite.  Q = P + 1 coefficients, the intercept first.
 * n_1 = #{y = 1}, n_0 = #{y = 0}.
 * Permutation of replicate b (GLOBAL index b0 + b): pi exactly as in mmm_associate_exposures (slot, key and e lists, ties by d), with the
 *   second Philox counter word 0x90000000: bits 31 and 28 without bits 30 and 29 are set by no other user of these words
 *   (mmm_extract_signatures uses 0x80000000 | j with j < 32, mmm_cluster_samples 0xC0000000 | k with k <= 32, mmm_survival_association
 *   0xA0000000, mmm_cox_exposures 0xB0000000 (bit 29 set as well), mmm_associate_exposures 0xE0000000, all others an index below 2^31).  Sample i keeps its label, its folds and its stratum
 *   and receives the feature row x[pi(i)].  The identity replicate uses pi = id.
 * One fit (T, lam), T a set of samples.  z_i = (1, x[pi(i)][0 .. P-1]), pen = (0, lam, .., lam).  From w = 0, for it = 1, 2, ..:
 *   eta_i = w_0 + sum_{j = 1 .. P} z_ij w_j, in ascending j, starting from w_0.  ec_i = -700 if eta_i < -700, 700 if eta_i > 700, else eta_i
 *   (a NaN stays).  p_i = 1 / (1 + ar_exp(-ec_i)), ar_exp of csrc/mmm_arith.h: the clamp keeps every operand of the quotient normal and
 *   finite.  om_i = p_i (1 - p_i), r_i = p_i - (double)y_i.
 *   g_j = (sum_{i in T} r_i z_ij) + pen_j w_j.  H_jk = (sum_{i in T} z_ij (om_i z_ik)) + [j = k] pen_j, for j >= k (nothing is added off the
 *   diagonal).  Both sums over i run in the stripe order of mmm_extract_signatures: sample i belongs to stripe i mod 16; a stripe's sum runs
 *   over its members of T in ascending i from 0.0; the 16 stripe sums are then added in ascending stripe order from 0.0.  Every product and
 *   every sum is rounded separately (no contraction).
 *   H = C C' by Cholesky in column order: C_kk = sqrt(H_kk - sum_{m < k} C_km C_km), C_jk = (H_jk - sum_{m < k} C_jm C_km) / C_kk, the
 *   subtractions one by one in ascending m.  If a radicand is not > 0 or not finite, the fit ends with status 2 and w is what it was before
 *   this iteration.  Otherwise C u = g forward (u_k = (g_k - sum_{m < k} C_km u_m) / C_kk, ascending m), C' d = u backward (d_k = (u_k -
 *   sum_{m > k} C_mk d_m) / C_kk, descending m), w <- w - d.  If a w_j is not finite the fit ends with status 2 (with that w); else if
 *   max_j |d_j| <= tol, with status 0; else if it = maxiter, with status 1.  Division and square root are the IEEE correctly rounded ones.
 * Scores and statistic.  For (b, r, l) and every fold f: fit (T = {i : fold[r][i] != f}, lambda[l]); s_i = eta_i (unclamped) under the final
 *   w for every i with fold[r][i] = f.  U2(b, r, l) = sum_{i : y = 1} sum_{j : y = 0} (2 [s_i > s_j] + [s_i = s_j]), a NaN comparing false.
 *   S_b[l] = sum_r U2(b, r, l): the cross-validated AUC is S / (2 R n_1 n_0).  M_b = max_l S_b[l].  Integers all: every comparison between
 *   replicates is exact once the scores are.
 * Outputs.  Under the identity, by a launch of one block of the same device code: scores [R][L][D] (or NULL), u2_obs [R][L] (or NULL),
 *   s_obs [L], and coef [L][Q] with full_iters [L][2] = (iterations, status) (or NULL each) of the fit on T = all samples per penalty.
 *   ge[l] = #{b in this call : S_b[l] >= s_obs[l]}, gemax[l] = #{b : M_b >= s_obs[l]}, maxstat [B] (or NULL) = M_b.  events [4] = the fits
 *   that ended with status 1 and with status 2 under the identity (the all-sample fits included), then among the permutations of this call:
 *   counted, not raised -- any deterministic procedure gives a valid permutation test, a fit that stops at maxiter costs only power.
 * Consequences.  (a) Every output is the same bits on every run and under every `waves`.  (b) maxstat of a call with (b0, B) is a slice of
 *   the call with (0, b0 + B).  (c) ge, gemax and events[2], events[3] of chunked calls add.  (d) scores, u2_obs, s_obs, coef, full_iters,
 *   events[0] and events[1] are independent of B, b0, seed and stream.
 * waves: the waves of a block, a pinned geometry for tests (0 = the library's choice, 4; else 1, 2, 4, 8 or 16).  The permuted rows are
 *   held in LDS when the block then stays within 64 KiB, and read through pi from memory otherwise; no bit depends on it.
 * Limits: 2 <= D <= 4096, 1 <= P <= 63, 2 <= F <= 255, 1 <= R <= 64, 1 <= L <= 32, 0 <= strata[d] < D, b0 + B <= 2^31 - 1.
 * MMM_ERR_ARG, nothing written and before any launch: NULL pointers (ctx, x, y, fold, lambda, s_obs, events; ge and gemax with B > 0), D < 2,
 *   P < 1, R < 1, F < 2, L < 1, B < 0, b0 < 0, b0 + B > 2^31 - 1, maxiter < 1, not tol >= 0, a lambda that is not > 0 and finite, an x that
 *   is not finite, a y other than 0 or 1, a fold >= F, a stratum outside 0 .. D-1, waves not one of 0, 1, 2, 4, 8, 16, a class without
 *   members, a training set (r, f) that lacks a class.  MMM_ERR_UNSUPPORTED, with the limit in the message: D > 4096, P > 63, R > 64,
 *   F > 255, L > 32.  B = 0: the identity outputs and events are written, ge, gemax and maxstat are untouched, MMM_OK.  No collective: on a
 *   multi-rank context it acts on its arrays. */
int mmm_classify_exposures(mmm_ctx* ctx, int D, int P, const double* x /* [D][P] */, const uint8_t* y /* [D] */,
                           const int32_t* strata /* [D] or NULL */, int R, int F, const uint8_t* fold /* [R][D] */, int L,
                           const double* lambda /* [L] */, int maxiter, double tol, int B, int b0, uint64_t seed, uint32_t stream, int waves,
                           double* scores /* [R][L][D] or NULL */, int64_t* u2_obs /* [R][L] or NULL */, int64_t* s_obs /* [L] */,
                           double* coef /* [L][Q] or NULL */, int32_t* full_iters /* [L][2] or NULL */, uint32_t* ge, uint32_t* gemax /* [L] each */,
                           int64_t* maxstat /* [B] or NULL */, uint32_t* events /* [4] */);

/* ---- a censored outcome against the exposures together: the cross-validated concordance index (Harrell's C) of a ridge-penalised,
 * stratified Cox regression (Breslow ties, no intercept) on P features over D samples, for L penalties, with B permutations of the feature
 * rows (within strata); the maximum over the penalties is permuted with the rest, so the p-value of the best penalty covers its choice (no
 * counterpart in the reference).
 * x [D][P]: a sample's features, as given (the Python layer standardises them).  time [D], finite and >= 0; event [D] in {0, 1} (1 = the
 * event was seen at time, 0 = censored there).  strata [D] or NULL; s_i = strata[i], or 0.  fold [R][D]: the fold (< F) of sample i in
 * repeat r, formed by the caller.  lambda [L], each > 0 and finite.  Q = P coefficients, no intercept.
 * Permutation of replicate b (GLOBAL index b0 + b): pi exactly as in mmm_associate_exposures (slot, key and e lists, ties by d), with the
 *   second Philox counter word 0xB0000000: bits 31, 29 and 28 without bit 30 are set by no other user of these words
 *   (mmm_extract_signatures uses 0x80000000 | j with j < 32, mmm_classify_exposures 0x90000000, mmm_survival_association 0xA0000000,
 *   mmm_cluster_samples 0xC0000000 | k with k <= 32, mmm_associate_exposures 0xE0000000, all others an index below 2^31).  Sample i keeps
 *   its time, event, folds and stratum and receives the feature row x[pi(i)].  The outcome is not permuted: everything in the next three
 *   paragraphs is the same for every replicate, and the host forms it once.  The identity replicate uses pi = id.
 * Time order.  Positions q = 0 .. D-1 hold the samples in ascending (s_i, -time_i, i): within a stratum by descending time, ties by
 *   ascending index (IEEE comparisons: -0.0 equals 0.0).  A tie group is a maximal run of positions with one stratum and one time; the
 *   groups are numbered g = 0 .. NG-1 in position order, whether they hold an event or not.  The risk set of a group is every position of
 *   its stratum from the stratum's first through the group's last.  Chunks: a stratum's positions are cut into chunks of 16 consecutive
 *   positions counted from the stratum's first position (its last chunk may be shorter); NC chunks in all.
 * One fit (T, lam), T a set of samples.  z_q = x[pi(i)] for the sample i at position q.  From w = 0, for it = 1, 2, ..:
 *   eta_q = sum_{j = 0 .. P-1} z_qj w_j in ascending j from 0.0.  ec = -700 if eta < -700, 700 if eta > 700, else eta (a NaN stays).
 *   u_q = ar_exp(ec_q) (csrc/mmm_arith.h) for a sample of T, +0.0 for any other.
 *   Down-scan, for the 1 + P entries v = u and v = u z_j (one product): in a chunk the partial at position q is the sequential sum from 0.0
 *   of v over the chunk's positions up to q; a chunk's total is its last partial; the offset of a chunk is the sequential sum from 0.0 of
 *   the totals of the earlier chunks of its stratum; S(q) = offset + partial (one addition).  S0 and S1_j are S of the two kinds of entry.
 *   Group terms.  d_G = the events of T in group G.  For d_G > 0, at the group's last position e: r_G = (double)d_G / S0(e), zbar_Gj =
 *   S1_j(e) / S0(e).  A group with d_G = 0 contributes nothing anywhere, no quotient is formed for it.
 *   Up-scan.  rho_q = r_G at the last position of a group with d_G > 0, +0.0 at every other position.  Over the SAME chunks, backwards: the
 *   partial at q is the sequential sum from 0.0 of rho over the chunk's positions from its last down to q; the offset of a chunk is the
 *   sequential sum from 0.0 of the totals of the LATER chunks of its stratum, taken from the stratum's last chunk downwards; Hhat_q = offset
 *   + partial: the Breslow cumulative hazard at the sample's time (the sum of r_G over the groups of the stratum with time <= its own).
 *   Residuals.  For a sample of T: uh_q = u_q Hhat_q, M_q = (double)event_q - uh_q (at w = 0 the log-rank score of
 *   mmm_survival_association, up to the order of the hazard sum).
 *   g_j = lam w_j - sum_{q in T} M_q z_qj.  H_jk = (sum_{q in T} z_qj (uh_q z_qk)) - (sum_{G : d_G > 0} zbar_Gj ((double)d_G zbar_Gk)),
 *   then + lam where j = k: the subtraction first, then the penalty; for j >= k.  The sums over q run in the stripe order of
 *   mmm_classify_exposures taken over POSITIONS: position q belongs to stripe q mod 16, a stripe's sum runs over its members of T in
 *   ascending q from 0.0, the 16 stripe sums are added in ascending stripe order from 0.0.  The sum over G runs in the same stripe order
 *   over the group index g.  Every product, quotient and sum is rounded separately (no contraction).
 *   Cholesky, both substitutions, w <- w - d and the stopping rule exactly as in mmm_classify_exposures with Q = P: status 2 if a radicand
 *   is not > 0 or not finite (w is what it was before this iteration) or if a w_j is not finite (with that w); else status 0 if max_j |d_j|
 *   <= tol; else status 1 if it = maxiter.  Division and square root are the IEEE correctly rounded ones.
 * Scores and statistic.  For (b, r, l) and every fold f: fit (T = {i : fold[r][i] != f}, lambda[l]); s_i = eta (unclamped) under the final
 *   w for every i with fold[r][i] = f.  An event sample i is comparable with j iff s_i = s_j as strata and (time_j > time_i, or time_j =
 *   time_i and event_j = 0).  U2(b, r, l) = sum_{i : event_i = 1} sum_{j comparable with i} (2 [s_i > s_j] + [s_i = s_j]), a NaN comparing
 *   false.  n_pairs = the number of comparable pairs.  S_b[l] = sum_r U2(b, r, l): the cross-validated C-index is S / (2 R n_pairs).
 *   M_b = max_l S_b[l].  Integers all.  (In the order (stratum, time ascending, events first, index) the partners of an event sample are
 *   one contiguous range that ends with its stratum; the host forms the ranges.)
 * Outputs.  Under the identity, by the same device code (a launch whose blocks share the R L cells and the L all-sample fits): scores
 *   [R][L][D] (or NULL), u2_obs [R][L] (or NULL), s_obs [L], n_pairs [1], and coef [L][P] with full_iters [L][2] = (iterations, status) (or
 *   NULL each) of the fit on T = all samples per penalty.  ge[l] = #{b in this call : S_b[l] >= s_obs[l]}, gemax[l] = #{b : M_b >=
 *   s_obs[l]}, maxstat [B] (or NULL) = M_b.  events [4] = the fits that ended with status 1 and with status 2 under the identity (the
 *   all-sample fits included), then among the permutations of this call: counted, not raised.
 * Consequences.  (a) Every output is the same bits on every run and under every `waves`.  (b) maxstat of a call with (b0, B) is a slice of
 *   the call with (0, b0 + B); ge, gemax and events[2], events[3] of chunked calls add.  (c) B = 0: the identity outputs, n_pairs and events
 *   are written, ge, gemax and maxstat are untouched, MMM_OK.  (d) scores, u2_obs, s_obs, n_pairs, coef, full_iters, events[0] and
 *   events[1] are independent of B, b0, seed and stream.
 * waves: the waves of a block, a pinned geometry for tests (0 = the library's choice, 4; else 1, 2, 4, 8 or 16).  Placement, no bit depends
 *   on it: zbar and the chunk totals (8 (NG (P + 1) + NC (P + 2)) bytes) are held in LDS when the block then stays within 64 KiB, else in a
 *   workspace per resident block in device memory, the grid capped so that the workspaces together stay within 256 MiB; the permuted rows
 *   are held in LDS when the block, with zbar if it is there, still stays within 64 KiB, else every read goes through pi to memory.
 * Limits: 2 <= D <= 4096, 1 <= P <= 64, 2 <= F <= 255, 1 <= R <= 64, 1 <= L <= 32, 0 <= strata[d] < D, b0 + B <= 2^31 - 1.
 * MMM_ERR_ARG, nothing written and before a device is asked for: NULL pointers (ctx, x, time, event, fold, lambda, s_obs, n_pairs, events;
 *   ge and gemax with B > 0), D < 2, P < 1, R < 1, F < 2, L < 1, B < 0, b0 < 0, b0 + B > 2^31 - 1, maxiter < 1, not tol >= 0, a lambda
 *   that is not > 0 and finite, an x that is not finite, a time that is not finite or is negative, an event other than 0 or 1, a fold >= F,
 *   a stratum outside 0 .. D-1, waves not one of 0, 1, 2, 4, 8, 16, a training set (r, f) without an event, n_pairs = 0.
 *   MMM_ERR_UNSUPPORTED, with the figure and the limit in the message: D > 4096, P > 64, R > 64, F > 255, L > 32.  Not handled: Efron
 *   ties, time-varying covariates, left truncation, L1 penalties.  No collective: on a multi-rank context it acts on its arrays. */
int mmm_cox_exposures(mmm_ctx* ctx, int D, int P, const double* x /* [D][P] */, const double* time /* [D] */, const uint8_t* event /* [D] */,
                      const int32_t* strata /* [D] or NULL */, int R, int F, const uint8_t* fold /* [R][D] */, int L,
                      const double* lambda /* [L] */, int maxiter, double tol, int B, int b0, uint64_t seed, uint32_t stream, int waves,
                      double* scores /* [R][L][D] or NULL */, int64_t* u2_obs /* [R][L] or NULL */, int64_t* s_obs /* [L] */,
                      int64_t* n_pairs /* [1] */, double* coef /* [L][P] or NULL */, int32_t* full_iters /* [L][2] or NULL */, uint32_t* ge,
                      uint32_t* gemax /* [L] each */, int64_t* maxstat /* [B] or NULL */, uint32_t* events /* [4] */);

/* ---- exposures against covariates with continuous adjusters: the Freedman-Lane permutation test of a linear model (Freedman & Lane 1983;
 * Winkler et al. 2014), P features against C tested covariates given A adjuster columns over D samples, B permutations of the reduced model's
 * residual rows (within strata), with the per-covariate maximum for Westfall-Young max-T adjustment (no counterpart in the reference;
 * DESIGN.md section 4.27).  The caller forms the linear algebra once: qz [D][A], an orthonormal basis of the adjustment space, intercept
 * included (NULL iff A == 0); e [D][P], the features' residuals on that basis; w [D][Q], per tested covariate c its cols[c] >= 1 orthonormal
 * columns spanning the covariate residualised on qz (one column for a numeric or binary covariate, G - 1 for G levels), in covariate order,
 * Q = the sum of cols.  The library checks shapes and finiteness, not orthogonality: the outputs are what the formulas below give.
 * Permutation of replicate b (GLOBAL index b0 + b): pi exactly as in mmm_associate_exposures (slot, key and e lists, ties by d), with the
 *   second Philox counter word 0xF0000000: bits 31, 30, 29 and 28 together are set by no other user of these words (mmm_extract_signatures
 *   uses 0x80000000 | j with j < 32, mmm_classify_exposures 0x90000000, mmm_survival_association 0xA0000000, mmm_cox_exposures 0xB0000000,
 *   mmm_cluster_samples 0xC0000000 | k with k <= 32, mmm_deal_counts 0xD0000000 | d, mmm_associate_exposures 0xE0000000, all others an
 *   index below 2^31).  Slot i keeps its design rows qz[i], w[i] and its stratum and receives the residual row e[pi(i)].  The identity
 *   replicate uses pi = id.
 * Dot products.  dot(f, g) over the slots i = 0 .. D-1 runs in the stripe order of mmm_extract_signatures and mmm_classify_exposures: slot
 *   i belongs to stripe i mod 16; a stripe's sum runs over its slots in ascending i, from 0.0, over the separately rounded products
 *   f_i g_i; the 16 stripe sums are added in ascending stripe order, from 0.0.  Nothing is contracted.
 * Per feature p.  ss_p = dot(e[.][p], e[.][p]) in the identity order, formed once per call and used by every replicate.
 *   a_j = dot(qz[.][j], e[pi(.)][p]).  rz = ss_p - (the sum over j = 0 .. A-1, ascending, from 0.0, of a_j a_j).
 * Per covariate c.  u_q = dot(w[.][q], e[pi(.)][p]).  num = the sum over the columns q of c, ascending, from 0.0, of u_q u_q.
 *   t[p][c] = num / rz if rz > 0, else +0.0 (a constant or fully explained feature gets p = 1).  Every product, sum and quotient is rounded
 *   separately.  t is the partial R^2 of c given the adjusters; the partial F, (t / cols_c) / ((1 - t) / (D - A - cols_c)), is monotone in t
 *   at fixed degrees of freedom, so the permutation p-values are those of F, and t of different features is on one scale for max-T within
 *   a covariate.
 * Outputs.  obs [P][C], u_obs [P][Q] (or NULL) and rz_obs [P] (or NULL): t, u and rz of the identity replicate, by a launch of the same
 *   kernel.  ge[p][c] = #{b in this call : t_b[p][c] >= obs[p][c]}, IEEE comparisons.  M_b[c] = max_p t_b[p][c], within a covariate only.
 *   ge_max[p][c] = #{b : M_b[c] >= obs[p][c]}.  maxstat [B][C] (or NULL) = M_b[c].
 *   Consequences.  (a) Every output is the same bits on every run and under every `waves`, wherever the kernel holds its operands.
 *   (b) maxstat of a call with (b0, B) is a slice of the call with (0, b0 + B).  (c) ge and ge_max of chunked calls add.  (d) obs, u_obs and
 *   rz_obs do not depend on B, b0, seed or stream.  (e) If every stratum has one member, every pi is the identity and ge = ge_max = B.
 * waves: the waves of a block, a pinned geometry for tests (0 = the library's choice; else 1, 2, 4, 8 or 16).
 * Limits: 1 <= D <= 4096, 1 <= P <= 64, 0 <= A <= 32, 1 <= C, Q <= 64, D - A - cols[c] >= 1 for every c, b0 + B <= 2^31 - 1,
 *   0 <= strata[d] < D.  Every entry of e, qz and w is finite with |v| <= 1e70, which keeps every product, square and sum of the
 *   definition finite (4096 products below 1e140, u below 1e144, u u below 1e288), so no NaN arises and the maxima are plain.
 * MMM_ERR_ARG, nothing written and before a device is asked for: NULL pointers (ctx, e, cols, w, obs; qz with A > 0; ge and ge_max with
 *   B > 0), D < 1, P < 1, C < 1, A < 0, a cols[c] < 1, D - A - cols[c] < 1, B < 0, b0 < 0, b0 + B > 2^31 - 1, an entry of e, qz or w that is
 *   not finite or beyond 1e70 in magnitude (its row and column are in the message), a stratum out of range, waves not one of 0, 1, 2, 4, 8, 16.  MMM_ERR_UNSUPPORTED,
 *   with the figure and the limit in the message: D > 4096, P > 64, A > 32, Q > 64.  B = 0: obs, u_obs and rz_obs are written, the counts
 *   are untouched, MMM_OK.  No collective: on a multi-rank context it acts on its arrays. */
int mmm_regress_exposures(mmm_ctx* ctx, int D, int P, const double* e /* [D][P] */, int A, const double* qz /* [D][A] or NULL when A = 0 */,
                          int C, const int32_t* cols /* [C], each >= 1 */, const double* w /* [D][Q], Q = sum cols */,
                          const int32_t* strata /* [D] or NULL */, int B, int b0, uint64_t seed, uint32_t stream, int waves,
                          double* obs /* [P][C] */, double* u_obs /* [P][Q] or NULL */, double* rz_obs /* [P] or NULL */, uint32_t* ge,
                          uint32_t* ge_max /* [P][C] each */, double* maxstat /* [B][C] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MMMUSIG_H */
