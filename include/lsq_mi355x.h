/*
 * lsq_mi355x.h -- C-ABI of liblsq_mi355x.so: the MI355X (gfx950) LSQ encoding engine.
 *
 * Drop-in boundary for the ILS/ICM encoding hot path of
 * una-dinosauria/local-search-quantization.  Every entry point cites the reference
 * interface it replaces (paths relative to the reference repository root).
 *
 * Conventions (the reference's own, src/linscan/Linscan.jl:63-69 style):
 *   - extern "C", plain pointers + integer sizes, no torch/STL types;
 *   - HOST buffers are the Julia column-major arrays read in place:
 *       RX/X  d x n  Float32          -> x_i[t]        at  X[i*d + t]
 *       K     d x (m*h) Float32 = hcat(C...) (encode_icm_cuda.jl:80, Linscan.jl:68)
 *                                      -> c_{j,a}[t]    at  K[(j*h + a)*d + t]
 *       B     m x n  Int16, 1-BASED   -> code (i,j)    at  B[i*m + j]
 *   - DEVICE buffers (the *_dev entry points) use the same X / K layouts and
 *     uint8 0-BASED codes [n][m] (the layout the reference hands to search,
 *     demos/demo_lsq_gpu.jl:67);
 *   - the caller allocates every output (encode_icm_cuda.jl:40-41,275-279) and lends
 *     pointers for the duration of the call; nothing is retained;
 *   - every function returns 0 on success, a negative LSQ_E* code otherwise;
 *     lsq_last_error() returns a thread-local message (the reference has no error
 *     convention at all: encode_icm_cuda.jl:264 "TODO check that splits >= 1");
 *   - calls are blocking unless stated; one host thread per lsq_ctx.
 *
 * Supported shapes: h == 256 (the reference GPU path hard-codes it:
 * src/encodings/cuda/cudautils.cu:38,58,155,245), 1 <= m <= 16 (cudautils.cu:38),
 * any d >= 1, any n >= 0.
 *
 * RNG (build-defined; the reference seeds curand with clock(), cudautils.cu:21):
 * Philox4x32-10 keyed by `seed`, counter = (global vector index, ILS iteration,
 * domain|block).  `global_offset` is the global index of the first vector of the
 * buffer, so results do not depend on nsplits / #GPUs / chunking.
 */
#ifndef LSQ_MI355X_H
#define LSQ_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_VERSION 2600

#if defined(__GNUC__)
#define LSQ_API __attribute__((visibility("default")))
#else
#define LSQ_API
#endif

enum {
    LSQ_OK = 0,
    LSQ_EINVAL = -1,    /* bad argument (shape, range, null pointer)      */
    LSQ_EHIP = -2,      /* a HIP runtime call failed (message has details) */
    LSQ_ENOMEM = -3,    /* device or host allocation failed                */
    LSQ_ECODE = -4,     /* an input code is outside 1..h                   */
    LSQ_ENODEV = -5     /* no usable gfx950 device                         */
};

typedef struct lsq_ctx lsq_ctx;

/* Accumulated device time per kernel class since the last lsq_reset_timings (hipEvent pairs on
 * the context's stream), only collected while option "profile" is 1. */
typedef struct lsq_timings {
    double tables_ms;        /* sqnorms + pairwise tables (get_binaries)            */
    double unaries_ms;       /* unary build (get_unaries)                            */
    double perturb_ms;       /* perturbation kernels                                 */
    double icm_ms;           /* ICM node-update kernels (the dominant kernel)        */
    double cost_ms;          /* cost + accept (+ objective) kernels                  */
    double other_ms;         /* layout conversion, snapshots                         */
    int64_t icm_launches;    /* number of ICM kernel launches inside icm_ms           */
    int64_t icm_node_updates;/* vector x node updates executed inside icm_ms          */
    /* which path the ICM blocks took (counted per block and node update, on the device; since v200): */
    int64_t staged_blocks;   /* table slices staged through LDS, the block walked all of them (team size 1)  */
    int64_t light_blocks;    /* few active vectors: table columns gathered from L2, one wave per vector       */
    int64_t filtered_blocks; /* 16-bit filtered walk (exact refinement of ambiguous vectors), LDS-staged slices       */
    int64_t filter_refined;  /* node updates the 16-bit filter could not decide: every candidate within the window evaluated exactly */
    int64_t filter_exact;    /* ... number of exact f32 candidate evaluations that took                               */
    int64_t filter_f32;      /* node updates sent to the f32 path because a unary fell outside the sampled level range  */
    int64_t filter_fallback_chunks; /* resident chunks the filter handed to the f32 walk: non-finite / degenerate value ranges, more than 1/64 of the
                                * (vector, node) pairs outside the sampled level range, or a first ILS iteration in which the filter decided too
                                * little (since v300)                                                                   */
    int64_t xs_launches;     /* reserved, always 0 (counted launches of round 4's schedule 7, which left the tree in v600; kept for the layout) */
    int64_t xs_fallback_launches; /* reserved, always 0 (as above)                                                      */
    int64_t table_reuses;    /* host-buffer calls that found their codebooks unchanged since the previous one: no upload of K, no table rebuild (since v500) */
} lsq_timings;      /* fields are only ever APPENDED: a caller built against an older header passes its own sizeof to lsq_get_timings_sized */

LSQ_API const char *lsq_last_error(void);
LSQ_API int lsq_version(void);
LSQ_API int lsq_device_count(int *count);

/* Context = device + stream + workspace.  Replaces the per-call CuContext / module load /
 * destroy! of encode_icm_cuda.jl:59-64,226-228. */
LSQ_API int lsq_create(lsq_ctx **ctx, int device);
LSQ_API int lsq_destroy(lsq_ctx *ctx);
/* Launch on the caller's hipStream_t (e.g. torch's current stream).  NULL = HIP's default (null)
 * stream; option "own_stream" switches back to the context's private non-blocking stream.
 * Nothing orders work on the new stream behind un-awaited work this context enqueued on the old one: the caller
 * must have awaited the old stream (lsq_synchronize, or its own stream / device synchronisation) before every switch. */
LSQ_API int lsq_set_stream(lsq_ctx *ctx, void *hip_stream);
/* Options: "chunk" (vectors per resident chunk, default 1015808 = 256 blocks x 3968 vectors: one pass of the walk kernel per block), "profile" (0/1), "own_stream",
 *   "schedule" -- how the ICM node updates run; all give bit-identical codes:
 *        6 (default) 16-bit FILTERED walk, one launch per ILS iteration: every term of a conditioned sum is also held as a 16-bit level
 *                    on a common step (u16 unary planes written by the unary GEMM's epilogue, u16 pair-table slices staged in LDS); a
 *                    1024-thread block owns <= 4096 vectors, sums the levels with packed 16-bit adds, tracks the two smallest keys and
 *                    decides a node update on the levels alone when the runner-up lies outside a rigorous error window; otherwise every
 *                    candidate inside the window is evaluated exactly in f32.  Half the HBM / LDS bytes of schedule 4.  Chunks below
 *                    "q16_min" vectors, and chunks whose data are not finite (decided on the device), run as schedule 4.
 *        4           f32 walk, one launch per ILS iteration: the block runs the icmiter x m node updates back to back, walking all LDS-staged
 *                    f32 table slices for each; f32 unaries streamed slice-major from HBM;
 *        3           the f32 walk, one launch per node update;
 *   "q16_min" (default 65536): schedule 6 applies to chunks with at least this many vectors (below, every block is "light": nothing to filter);
 *   "per_node" (0/1, default 0): schedule 6 with one launch per node update (profiling: per-sweep timings and counters);
 *   "light" (default 160 in the filtered walk, 256 in the f32 walk: the measured crossovers): a block with at most this many active vectors
 *        gathers f32 table columns straight from L2 (one wave per vector, two vectors in flight) instead of staging slices through LDS;
 *        0 = always stage.  Same codes.
 *   "wave_max" (default 64): a chunk with at most this many vectors per block of the walk kernel (n <= 256 x 64) -- all of them light -- runs
 *        icm_wave_kernel instead: a wave owns its two vectors through every node update of the launch (records and validity words in registers,
 *        no compaction, no barriers); 0 = never.  Same codes.
 *   "fallback" (0/1, default 1): a candidate whose codes become equal to the vector's current codes inherits the current state's validity
 *        bits (validity depends on the code tuple only): exact, ~12 % fewer node updates.
 *   "skip" (0/1, default 1): a node whose conditioning codes did not change since it was last minimised is not recomputed (exact memoisation --
 *        same codes, fewer bytes).
 *   "filter_fallback_div" (default 64): schedule 6 hands a resident chunk to the f32 walk when more than 1 / div of its (vector, node) pairs
 *        have a unary outside the sampled 16-bit level range (each such pair takes the one-wave-per-vector f32 routine, ~5x the cost of a filtered update);
 *        0 = never.  Same codes.
 *   "filter_probe_div" (default 8): after the FIRST ILS iteration of a resident chunk schedule 6 reads that iteration's counters and runs the
 *        remaining iterations as schedule 4 when more than 1 / div of the recomputed node updates needed the exact refinement or the f32 routine
 *        (a level step blown up by a few extreme values: scale-mixture / heavy-tailed data); 0 = never.  Same codes.  A call of ONE ILS iteration
 *        (lsq_encoding_icm chained by a trainer) splits its launch after the first SWEEP and probes that; nothing is remembered between calls.
 *   "async" (0/1, default 0): lsq_encode_icm_dev without any host synchronisation (see there).  Which entry points block: every entry point that
 *        takes or returns HOST buffers waits for its results; lsq_encode_icm_dev waits (per chunk: verdict, probe; at the end: sums) unless "async" = 1;
 *        lsq_linscan_dev, lsq_quantize_norms_dev, lsq_update_codebooks_dev and lsq_update_codebooks_struct_dev read small control words back (threshold
 *        lists, convergence counter, the cover map) and wait.
 *   "ils_counter": the next iteration index used by lsq_encoding_icm / lsq_encode_icm_fully when called with it = LSQ_IT_AUTO
 *        (starts at 0, advances by one per such call).
 *   "rerank_batch" (default 0): queries per batch of the re-rank stage of every lsq_index created on this context; 0 = automatic (batches of at most
 *        2^28 (query, candidate) records, like the scans).  A test hook: small shapes cross batch boundaries.  Same results.
 *   "knn_u8_int" (0/1, default 1): 0 = lsq_index_knn widens 8-bit rows and queries even where its integer road applies.  A test hook: same results.
 *   "range_batch" (default 0): records per fill batch of lsq_index_range_search on every lsq_index created on this context; 0 = automatic (2^28).  A
 *        test hook: small shapes cross batch boundaries, and a query larger than the budget is a batch of its own.  Same results.
 *   (liblsq_mi355x_tuning.so only) "ablation": timing-only kernel variants whose results are garbage. */
LSQ_API int lsq_set_option(lsq_ctx *ctx, const char *key, int64_t value);
LSQ_API int lsq_get_timings(lsq_ctx *ctx, lsq_timings *out);      /* writes the v400 layout only (everything before table_reuses: a caller built against any header since v400 is never overrun); the fields appended since come through: */
/* ... the size-checked form: at most `bytes` bytes of the structure are written (the fields a caller compiled against an older header knows about);
 * compare lsq_version() with LSQ_VERSION at load time to learn which fields the library fills. */
LSQ_API int lsq_get_timings_sized(lsq_ctx *ctx, void *out, size_t bytes);
/* Node updates actually recomputed (not memoised) per POSITION in an ILS iteration's node sequence, position = sweep * m + rank in
 * the visiting order (mod 64), summed over ILS iterations, chunks and calls since the last lsq_reset_timings: the device-side
 * counterpart of the reference's per-iteration "% equal / % better" prints, for the sweeps.  out[count], count <= 64. */
LSQ_API int lsq_get_walk_trace(lsq_ctx *ctx, int64_t *out, int count);
/* Read-only snapshot of what the LAST resident chunk of the last encode call left in the context for the 16-bit filtered walk (schedule 6; since v1200):
 * the inputs of the inequality the filter's window rests on (csrc/lsq_icmq.hip, BOUND), for a checker outside the library.  Computes nothing and changes
 * no result: one hipMemcpyAsync of default kind on the context's stream, so `dst` may be host or device memory (wait for the stream before reading it).
 * With cn = the chunk's rows, SLQ = 32 (m <= 8) or 16 candidates per 16-bit slice, SLF = SLQ / 2 per f32 slice, h = 256:
 *   LSQ_SNAP_PARAMS  lsq_q16_snapshot_params below (the library's level parameters as the walk reads them)
 *   LSQ_SNAP_UQ      u16 [m][h / SLQ][cn][SLQ]                   unary levels:  candidate a of (node j, row i) at ((j * (h / SLQ) + a / SLQ) * cn + i) * SLQ + a % SLQ
 *   LSQ_SNAP_TQ      u16 [m][h / SLQ][(m - 1) * h][SLQ]          table levels of node j, conditioning table kk (codebook k = kk + (kk >= j)) and code b: row
 *                                                                R(kk, b) of slice a / SLQ, where with S = 4 (SLQ = 32) or 8 (SLQ = 16) slots per line and
 *                                                                n0 = min(m - 1, S):  R = b * n0 + kk  (kk < S),  R = n0 * h + b * (m - 1 - n0) + (kk - S)  (kk >= S)
 *   LSQ_SNAP_QFLAG   u16 [cn]                                    bit j: the pair (row, node j) lies outside the sampled level range and takes the f32 routine
 *   LSQ_SNAP_U       f32 [m][h / SLF][cn][SLF]                   the f32 unaries, slice-major like the levels
 *   LSQ_SNAP_T       f32 [m][m][h][h]                            the f32 pair tables: T[j][k][b][a] (the diagonal blocks j == k are never read)
 * info (optional) receives 6 values: cn, the chunk's first row within the call, m, SLQ, SLF, and 1 when the chunk stayed on the filtered walk to its end
 * (0: the probe after its first ILS iteration handed the rest to the f32 walk; the levels are resident either way).
 * LSQ_EINVAL: no filtered chunk is resident (no encode yet, a chunk below "q16_min", a verdict for the f32 walk, option "async" -- its verdict stays on the
 * device --, or a later call that rebuilt the unaries or the tables), `bytes` smaller than the item, or an unknown `what`. */
enum { LSQ_SNAP_PARAMS = 0, LSQ_SNAP_UQ = 1, LSQ_SNAP_TQ = 2, LSQ_SNAP_QFLAG = 3, LSQ_SNAP_U = 4, LSQ_SNAP_T = 5 };
typedef struct lsq_q16_snapshot_node {
    float loU, invD, D;      /* unary levels start at loU; the common step of node j and its f32 reciprocal */
    float hiq;               /* largest unary level inside the sampled range: a pair with a level outside [0, hiq] is flagged */
    int32_t window;          /* levels: the exact argmin lies within `window` of the smallest level sum (65535: everything is refined) */
    int32_t pad_;
    double slack;            /* bound of |C_i + D Q[a] - s_f32[a]|; window = floor(2 slack / D) + 1 */
} lsq_q16_snapshot_node;
typedef struct lsq_q16_snapshot_params {
    int32_t ok;              /* 1: usable bounds */
    int32_t oor;             /* values outside the sampled level range so far in the call */
    int32_t nflag;           /* flagged (row, node) pairs of the chunk */
    int32_t pad_;
    lsq_q16_snapshot_node node[16];
} lsq_q16_snapshot_params;
LSQ_API int lsq_get_q16_snapshot(lsq_ctx *ctx, int what, void *dst, size_t bytes, int64_t *info);
LSQ_API int lsq_reset_timings(lsq_ctx *ctx);
LSQ_API int lsq_synchronize(lsq_ctx *ctx);

/* ---- single-process multi-GPU (the `ngpus` of SURVEY 8(b); what a Julia master process calls on a multi-GPU node) --------
 * One context and one host thread per listed device; the n vectors are split with `splitarray` (src/utils.jl:152-177,
 * the reference's own sharding of encode_icm.jl:165-173) and every shard is encoded with its global offset, so the result
 * is bit-identical to the one-device call for any device list (RNG keyed by the global vector index).  No data-path
 * collective: K is uploaded to every device, objective sums and counters are added on the host.  `devices` may repeat an
 * ordinal (two shards time-share one GPU).  Options apply to every context.  One process per GPU with torch.distributed /
 * RCCL (local-search-quantization_amd/distributed.py) is the other, multi-process way to use several GPUs. */
typedef struct lsq_multi lsq_multi;
LSQ_API int lsq_multi_create(lsq_multi **out, const int *devices, int ndev);
LSQ_API int lsq_multi_destroy(lsq_multi *mg);
LSQ_API int lsq_multi_set_option(lsq_multi *mg, const char *key, int64_t value);
/* Same arguments, layouts and outputs as lsq_encode_icm (below), minus nsplits. */
LSQ_API int lsq_multi_encode_icm(lsq_multi *mg, const float *RX, const int16_t *B, const float *K, int d, int64_t n, int m, int h,
                                 const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, uint64_t seed,
                                 uint64_t global_offset, int verbose, int16_t *Bs, float *objs);

/* ---- (1) the whole call ------------------------------------------------------------------
 * Replaces encode_icm_cuda(RX, B, C, ilsiters, icmiter, npert, randord, nsplits, V)
 *   -> (Bs, objs)      src/encodings/encode_icm_cuda.jl:253-296 (and _single, :22-234);
 * call site demos/demo_lsq_gpu.jl:50.  Runs max(ilsiters) ILS iterations; snapshot k holds the
 * codes and the objective (qerror, src/utils.jl:257-285) after ilsiters[k] iterations.
 * Semantics of each ILS iteration follow the reference CPU path (src/encodings/encode_icm.jl:
 * 131-189): perturb, icmiter sweeps, accept iff strictly better.
 *   Bs   : nr x (m x n Int16, 1-based), caller-allocated;   objs : nr Float32.
 * nsplits is accepted for signature compatibility (the reference needs it for 12 GB GPUs,
 * demos/demo_lsq_gpu.jl:49); results do not depend on it. */
LSQ_API int lsq_encode_icm(lsq_ctx *ctx, const float *RX, const int16_t *B, const float *K,
                   int d, int64_t n, int m, int h,
                   const int64_t *ilsiters, int nr, int icmiter, int npert, int randord,
                   int nsplits, uint64_t seed, uint64_t global_offset, int verbose,
                   int16_t *Bs, float *objs);

/* Same call on DEVICE-resident buffers: launches go to the context's stream.  BLOCKING by default: the host waits once per resident chunk for the
 * chunk's three-word verdict after the unary GEMM, once more for the probe after the first ILS iteration, and at the end for the read-back of the
 * objective sums and counters.  Option "async" = 1 removes every one of those waits: the verdict and the probe are taken by one-thread kernels, BOTH walk
 * kernels are enqueued each ILS iteration (the one the device word does not name returns at once: ~3 us per launch), and obj_sums / stats are written in
 * stream order -- they must then be DEVICE pointers or PINNED host memory, and are valid once the stream has been synchronised by the caller.  With "async"
 * the call contains no host synchronisation and no allocation once the context's work buffers have the size of the shape (i.e. from the second call of
 * that shape on): it can be captured into a hipGraph.  Walk statistics of async calls are folded into lsq_get_timings at its next call (which waits).
 * dB0 / dBs: uint8 0-based [n][m] (dBs: nr of them).
 * obj_sums (host, nr doubles) receives SUM_i cost_i (not the mean) so that a multi-GPU caller
 * can add shards; objs = obj_sums / n_total.  stats (host, optional, 2*max(ilsiters) int64):
 * per ILS iteration the number of vectors whose new cost was == / < the previous one
 * (the two counters the reference prints, encode_icm.jl:180-184). */
LSQ_API int lsq_encode_icm_dev(lsq_ctx *ctx, const float *dX, const uint8_t *dB0, const float *dK,
                       int d, int64_t n, int m, int h,
                       const int64_t *ilsiters, int nr, int icmiter, int npert, int randord,
                       uint64_t seed, uint64_t global_offset,
                       uint8_t *dBs, double *obj_sums, int64_t *stats);

/* ---- (1b) the whole call on 8-bit data (since v1300) ----------------------------------------
 * Base sets stored as unsigned bytes -- the TEXMEX .bvecs files of SIFT1B-style sets, read by the reference's bvecs_read (src/read/read_datasets.jl)
 * into a UInt8 matrix -- are encoded WITHOUT being widened to float by the caller: d bytes per vector in host memory, over the bus and in the
 * context's resident chunk buffers; the kernels that read X widen four components per dword load in registers.  uint8 -> float32 is exact, so every
 * call returns, bit for bit, what its f32 counterpart returns on Float32.(X): the same codes, objective sums and counters, under every option
 * (schedules 6 / 4 / 3, "chunk", "per_node", "light", "async", the probe and fall-back roads).  8-bit and f32 calls may be mixed on one context in
 * any order.  RX8 / dX8: d x n UInt8 column-major ([n][d] bytes); any byte alignment (a 4-byte-aligned base with d % 4 == 0 takes the dword loads,
 * anything else byte loads).  Everything else -- B, K, Bs, objs, errors, the h = 256 rule -- as in the call each one stands in for:
 *   lsq_encode_icm_u8        stands in for lsq_encode_icm        (encode_icm_cuda on Float32.(RX), encode_icm_cuda.jl:253-296)
 *   lsq_encode_icm_u8_dev    stands in for lsq_encode_icm_dev    (device-resident; "async" and graph capture under the same conditions)
 *   lsq_multi_encode_icm_u8  stands in for lsq_multi_encode_icm  (one shard per device)
 * The other entry points (k-NN, trainers, codebook updates, scan queries) take float32 as before.
 * (The context argument is spelled with its struct tag here: the catalogue of tests/ctx_ops.py collects the context entry points it walks by the
 * typedef spelling and is closed; these two are walked, pair by pair with their f32 counterparts, by tests/ctx_ops_u8.py.) */
LSQ_API int lsq_encode_icm_u8(struct lsq_ctx *ctx, const uint8_t *RX8, const int16_t *B, const float *K,
                   int d, int64_t n, int m, int h,
                   const int64_t *ilsiters, int nr, int icmiter, int npert, int randord,
                   int nsplits, uint64_t seed, uint64_t global_offset, int verbose,
                   int16_t *Bs, float *objs);
LSQ_API int lsq_encode_icm_u8_dev(struct lsq_ctx *ctx, const uint8_t *dX8, const uint8_t *dB0, const float *dK,
                       int d, int64_t n, int m, int h,
                       const int64_t *ilsiters, int nr, int icmiter, int npert, int randord,
                       uint64_t seed, uint64_t global_offset,
                       uint8_t *dBs, double *obj_sums, int64_t *stats);
LSQ_API int lsq_multi_encode_icm_u8(lsq_multi *mg, const uint8_t *RX8, const int16_t *B, const float *K, int d, int64_t n, int m, int h,
                                    const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, uint64_t seed,
                                    uint64_t global_offset, int verbose, int16_t *Bs, float *objs);

/* ---- (2) the CPU-path shaped entry points -------------------------------------------------
 * encoding_icm(X, oldB, C, niter, randord, npert, V) -> B     src/encodings/encode_icm.jl:131-189
 * ONE ILS iteration with the accept rule.  `it` = the iteration's 0-based index: it keys the perturbation and the node
 * order (the reference draws them from Julia's global RNG, so every call differs).  The reference's callers keep no
 * such count (demos/demo_lsq.jl:48-51: `for i = 1:ilsiter; B = encoding_icm(...); end`), so an unchanged caller passes
 * it = LSQ_IT_AUTO: the CONTEXT then counts -- the k-th such call on a context uses it = k-1 (option "ils_counter" sets
 * the next value; lsq_encode_icm_fully shares the counter) -- and `ilsiter` chained calls give exactly the codes of
 * lsq_encode_icm(ilsiters = [ilsiter]) on a fresh context.  A fixed `it` on every call would re-draw the SAME
 * perturbation each time and the ILS would silently stop exploring. */
#define LSQ_IT_AUTO 0xFFFFFFFFu
LSQ_API int lsq_encoding_icm(lsq_ctx *ctx, const float *X, const int16_t *oldB, const float *K,
                     int d, int64_t n, int m, int h, int niter, int randord, int npert,
                     uint64_t seed, uint32_t it, uint64_t global_offset, int16_t *outB);

/* encode_icm_fully!(B, X, C, binaries, cbi, niter, randord, npert, IDX, V)
 *   src/encodings/encode_icm.jl:4-127 -- the worker: perturb + niter sweeps, in place, NO accept
 * test.  This is the hook the authors left commented at encode_icm.jl:163 (`encode_icm_cpp!`).
 * `binaries`/`cbi` are rebuilt on the device from K (cheaper than shipping them);
 * idx_first = first(IDX), 1-based global column of X[:,1] (keys the RNG). */
LSQ_API int lsq_encode_icm_fully(lsq_ctx *ctx, int16_t *B, const float *X, const float *K,
                         int d, int64_t n, int m, int h, int niter, int randord, int npert,
                         int64_t idx_first, uint64_t seed, uint32_t it);

/* ---- (3) the numeric helpers the path is made of (host buffers) ---------------------------
 * get_unaries(X, C)   src/utils.jl:94-122  -> U [m][n][h]  (unaries[j] is h x n column-major) */
LSQ_API int lsq_get_unaries(lsq_ctx *ctx, const float *X, const float *K, int d, int64_t n, int m, int h, float *U);
/* get_binaries(C)     src/utils.jl:125-144 (+ the transposes of encode_icm.jl:25-28)
 *   -> T [m][m][h][h], T[j][k][b][a] = 2<c_{j,a}, c_{k,b}>; binaries[idx(i<j)][a + b*h] = T[i][j][b][a] */
LSQ_API int lsq_get_binaries(lsq_ctx *ctx, const float *K, int d, int m, int h, float *T);
/* veccost(X, B, C)    src/utils.jl:225-254  -> cost [n] */
LSQ_API int lsq_veccost(lsq_ctx *ctx, const float *X, const int16_t *B, const float *K,
                int d, int64_t n, int m, int h, float *cost);
/* qerror(X, B, C)     src/utils.jl:257-285  -> mean squared error (f64 accumulation) */
LSQ_API int lsq_qerror(lsq_ctx *ctx, const float *X, const int16_t *B, const float *K,
               int d, int64_t n, int m, int h, double *out);
/* perturb kernel      src/encodings/cuda/cudautils.cu:27-80 (host buffers, in place) */
LSQ_API int lsq_perturb(lsq_ctx *ctx, int16_t *B, int64_t n, int m, int h, int npert,
                uint64_t seed, uint32_t it, uint64_t global_offset);
/* randinit(n, m, h)   src/initializations.jl:2-8   (host function, Philox-keyed) */
LSQ_API int lsq_randinit(uint64_t seed, uint64_t global_offset, int64_t n, int m, int h, int16_t *B);
/* node visiting order of ILS iteration `it` (randperm of encode_icm.jl:46-49), 0-based */
LSQ_API int lsq_node_order(uint64_t seed, uint32_t it, int m, int randord, int32_t *order);
/* splitarray(1:n, nparts)  src/utils.jl:152-177 -> part's [start, start+len) , 0-based */
LSQ_API int lsq_splitarray(int64_t n, int nparts, int part, int64_t *start, int64_t *len);

/* ---- (3b) search side of the path (host code) --------------------------------
 * linscan_aqd_query_extra_byte(dists, idx, codes, queries, codebooks, dbnorms, nqueries, ncodes, m, h, d, nn)
 *   src/linscan/cpp/linscan_aqd_pairwise_byte.cpp:97-104, ccall at src/linscan/Linscan.jl:63-69.
 * Same argument list plus `nthreads` (0 = all cores).  codes: m x n uint8 0-based; queries: d x nq;
 * codebooks = hcat(C...); dbnorms: n.  Outputs (caller-allocated): dists nn x nq f32 ascending,
 * idx nn x nq int32, 1-BASED.  Distances are bit-identical to the reference build (same f32
 * operation order); ties are ordered by id, as the reference's pair sort does.  Requires nn <= n. */
LSQ_API int lsq_linscan_aqd_query_extra_byte(float *dists, int *idx, const unsigned char *codes, const float *queries,
                                     const float *codebooks, const float *dbnorms, int nqueries, int ncodes,
                                     int m, int h, int d, int nn, int nthreads);

/* The same scan ON THE DEVICE (SURVEY 8(f)-1 "HIP scan later"; csrc/lsq_adc.hip).  Same argument list behind a context; same results bit for
 * bit -- distances, 1-based ids, order including ties -- as the host function above and as the reference build.  Requires h == 256,
 * 1 <= m <= 16, 1 <= nn <= ncodes.  NaN distances (undefined order in the reference's partial_sort) sort last.
 *   lsq_linscan      host buffers (uploaded, searched, downloaded);
 *   lsq_linscan_dev  device buffers: codes [ncodes][m] uint8 0-based, queries [nq][d], codebooks [m*h][d], dbnorms [ncodes]; outputs [nq][nn]. */
LSQ_API int lsq_linscan(lsq_ctx *ctx, float *dists, int *idx, const unsigned char *codes, const float *queries, const float *codebooks,
                        const float *dbnorms, int nqueries, int ncodes, int m, int h, int d, int nn);
LSQ_API int lsq_linscan_dev(lsq_ctx *ctx, float *d_dists, int *d_idx, const uint8_t *d_codes, const float *d_queries, const float *d_codebooks,
                            const float *d_dbnorms, int nqueries, int ncodes, int m, int h, int d, int nn);
/* The same over a database sharded across the devices of an lsq_multi (splitarray shards, one host thread per device, host merge of the per-device
 * lists by (distance, id)): the result of ONE scan of the whole database, ties across shards included. */
LSQ_API int lsq_multi_linscan(lsq_multi *mg, float *dists, int *idx, const unsigned char *codes, const float *queries, const float *codebooks,
                              const float *dbnorms, int nqueries, int ncodes, int m, int h, int d, int nn);
/* ---- (3c) the reference's other scan: PQ / OPQ codes (since v700) -------------------------------------------------------------------------
 * linscan_aqd_query(dists, res, codes, centers, queries, N, NQ, B, K, dim1codes, dim1queries, subdim)
 *   src/linscan/cpp/linscan_aqd.cpp:37-114, bound by linscan_pq / linscan_opq at src/linscan/Linscan.jl:5-43 (linscan_opq = linscan_pq of R'X).
 * The reference's argument list and types, host code (std::thread workers).  m = B/8 sub-spaces of h = 256 centres each.
 *   codes    [N][dim1codes] uint8 0-based (Julia B, m x n: dim1codes = m); only the first m bytes of a row are read.
 *   centers  [m][256][subdim] = cat(3, C...) (C[k] subdim x 256)  -> c_{k,r}[s] at centers[(k*256 + r)*subdim + s].
 *   queries  [NQ][dim1queries] (Julia X, d x nq: dim1queries = d); sub-space k reads q[k*subdim .. k*subdim + subdim).
 *   table[k*256 + r] = ((0 + e_0*e_0) + e_1*e_1) + ..., e_s = c_{k,r}[s] - q[k*subdim + s]        (f32, s ascending, no FMA)
 *   dist(i)          = ((0 + table[0*256 + b_i0]) + table[1*256 + b_i1]) + ...                    (k ascending, no norm term)
 * Outputs (caller-allocated): dists [NQ][K] f32 ascending; res [NQ][K] uint32, 0-BASED ids (linscan_pq adds 1 on the Julia side).  The K smallest
 * (dist, id) pairs in lexicographic order (ties: smaller id first), bit-identical to the reference build; NaN distances sort last.
 * Requires B % 8 == 0, 1 <= B/8 <= dim1codes, subdim >= 1, (B/8)*subdim <= dim1queries, 1 <= K <= N, non-null pointers (NQ > 0). */
LSQ_API int lsq_linscan_aqd_query(float *dists, uint32_t *res, const uint8_t *codes, const float *centers, const float *queries, int N,
                                  uint32_t NQ, int B, int K, int dim1codes, int dim1queries, int subdim);
/* The same scan ON THE DEVICE (csrc/lsq_adc.hip: the LSQ scan's kernels with the sub-space squared-distance tables and no norm term).  Same
 * argument list behind a context, same results bit for bit as lsq_linscan_aqd_query, 0-based uint32 ids included.  Device limits of lsq_linscan:
 * B/8 <= 16 (LSQ_EINVAL beyond), NQ <= 2^31 - 1.  Options "linscan_exhaustive" / "linscan_rank" and lsq_get_linscan_stats cover it.
 *   lsq_linscan_pq      host buffers (uploaded, searched, downloaded);
 *   lsq_linscan_pq_dev  device buffers, the layouts above. */
LSQ_API int lsq_linscan_pq(lsq_ctx *ctx, float *dists, uint32_t *res, const uint8_t *codes, const float *centers, const float *queries, int N,
                           uint32_t NQ, int B, int K, int dim1codes, int dim1queries, int subdim);
LSQ_API int lsq_linscan_pq_dev(lsq_ctx *ctx, float *d_dists, uint32_t *d_res, const uint8_t *d_codes, const float *d_centers, const float *d_queries,
                               int N, uint32_t NQ, int B, int K, int dim1codes, int dim1queries, int subdim);
/* ---- (3d) exact k-NN: the ground truth of a recall figure (since v900) ---------------------------------------------------------------------------
 * The reference reads ground truth from sift_groundtruth.ivecs (full SIFT1M base only); these compute it for any float base.
 *   base     [n][ldb] f32, queries [nq][ldq] f32; only the first d floats of each row are read.
 *   dist(q, i) = ((0 + e_0*e_0) + e_1*e_1) + ... + e_{d-1}*e_{d-1},   e_s = x_i[s] - q[s]       (f32, s ascending, every op rounded, no FMA)
 *   -- the PQ table rule above with one sub-space of width d.
 * Outputs (caller-allocated): dists [nq][nn] f32 ascending; ids [nq][nn] uint32, 0-BASED (the .ivecs convention).  The nn smallest (dist, id) pairs
 * in lexicographic order (ties: smaller id first); NaN distances sort last.  All three functions return the same bits.
 * LSQ_EINVAL: d < 1, ldb < d, ldq < d, nq < 1, nn < 1, nn > n, a null pointer or context.
 *   lsq_knn_exact_cpu  host cores, std::thread workers (nthreads 0 = all): the checker and the engine-less road;
 *   lsq_knn_exact      device, host buffers (uploaded, searched, downloaded);
 *   lsq_knn_exact_dev  device, device buffers.  The device forms run the selection of the scans above: options "linscan_exhaustive" /
 *                      "linscan_rank" and lsq_get_linscan_stats cover them (lut_ms stays 0). */
LSQ_API int lsq_knn_exact_cpu(float *dists, uint32_t *ids, const float *base, const float *queries, int n, int nq, int d, int ldb, int ldq, int nn,
                              int nthreads);
LSQ_API int lsq_knn_exact(lsq_ctx *ctx, float *dists, uint32_t *ids, const float *base, const float *queries, int n, int nq, int d, int ldb, int ldq,
                          int nn);
LSQ_API int lsq_knn_exact_dev(lsq_ctx *ctx, float *d_dists, uint32_t *d_ids, const float *d_base, const float *d_queries, int n, int nq, int d,
                              int ldb, int ldq, int nn);
/* What the device scans (LSQ, PQ and exact k-NN) did since the last lsq_reset_timings (times only with option "profile" = 1). */
typedef struct lsq_linscan_stats {
    int64_t queries, codes;          /* queries searched (accumulated); database size of the last call */
    int64_t candidates;              /* (dist, id) pairs written to memory: the lists the selection sorted */
    int64_t fallback_queries;        /* queries redone by the exhaustive road (candidate list short or overflowing) */
    int64_t batches;
    int64_t exhaustive;              /* last call: 1 = every distance written and sorted (small database / large nn / option) */
    int64_t threshold_rank, list_capacity;      /* last call: sample rank of the threshold, entries per candidate list */
    double lut_ms, sample_ms, scan_ms, select_ms;
} lsq_linscan_stats;
LSQ_API int lsq_get_linscan_stats(lsq_ctx *ctx, lsq_linscan_stats *out);

/* ---- (3e) two-stage search: exact re-rank of ADC shortlists, on a resident index (since v1400) ---------------------------------------------------
 * Stage one is the scan of linscan_lsq, src/linscan/Linscan.jl:46-73 (lsq_linscan_dev above).  Stage two HAS NO COUNTERPART IN THE REFERENCE, whose
 * recall figures are those of the ADC distances alone: every query's shortlist is re-ordered by the true distance to the stored vectors,
 *   dist = ((0 + e_0*e_0) + e_1*e_1) + ... + e_{d-1}*e_{d-1},   e_s = x[s] - q[s]       (f32, s ascending, every op rounded, no FMA)
 * -- lsq_knn_exact's rule: a re-ranked distance has the bits lsq_knn_exact gives for the same (query, row).  A uint8 base (base_u8 = 1: the un-widened rows
 * of a .bvecs set) is widened in registers (exact): the bits of the f32 call on the widened matrix.  Any byte alignment and any ldb >= d; the loads are
 * 16 bytes, 4 bytes or single bytes wide by what the base pointer and the row pitch in bytes are both multiples of.
 *   cand [nq][L] int32 ids in the caller's id_base (0 or 1); dists / ids [nq][nn], ids int32 in the same id_base.
 *   Result per query: the nn smallest (dist, id) pairs among its L candidates in lexicographic order; ties go to the smaller id; NaN distances sort
 *   after every number.  An id that occurs twice is returned twice.  An id outside [id_base, id_base + n) is never dereferenced: it sorts after everything,
 *   NaN included, and is reported as (+inf, id_base - 1).
 * base_u8 = LSQ_BASE_F16 / LSQ_BASE_BF16 (since v2500, (3o)): rows of 2-byte elements, 2-byte aligned, widened likewise -- the bits of the f32 call on
 * the widened matrix; 16-byte, 4-byte or 2-byte loads by the same rule (the last, partial dword of an odd-d row travels as one 2-byte load).
 * LSQ_EINVAL: nn < 1, nn > L, d < 1, ldb < d, ldq < d, n < 1, an id_base other than 0 / 1, a null pointer.
 *   lsq_rerank_cpu  host cores, std::thread workers (nthreads 0 = all), no context: the checker and the engine-less road. */
LSQ_API int lsq_rerank_cpu(float *dists, int *ids, const void *base, int base_u8, const float *queries, const int *cand, int n, int nq, int d, int ldb,
                           int ldq, int L, int nn, int id_base, int nthreads);
/* The index: a handle that keeps the database RESIDENT on a context's device -- codes, norms and codebooks for stage one, the base rows for stage two -- so
 * that a C or Julia caller uploads it once instead of once per lsq_linscan call.
 *   on_device = 0: host buffers, copied once at creation and owned by the index;  on_device = 1: device pointers, borrowed -- the caller keeps them alive.
 *   codes == NULL: a base-only index (re-rank only; codebooks / dbnorms / m / h are ignored);  base == NULL: a scan-only index.  One of them must be set.
 * The index runs on the context's device and on the stream the context is bound to at each call; the context must outlive it, and -- like the context --
 * it serves one host thread at a time.  It owns its own scratch (scan state, record buffers): calls on the index and calls on the context do not disturb
 * each other, and neither do two indexes of one context.  Limits of lsq_linscan: h == 256, 1 <= m <= 16; n <= 2^31 - 2. */
typedef struct lsq_index lsq_index;
typedef struct lsq_index_desc {
    int64_t n;
    int d, m, h;
    const uint8_t *codes;        /* [n][m] uint8 0-based, or NULL */
    const float *codebooks;      /* [m*h][d] */
    const float *dbnorms;        /* [n] */
    const void *base;            /* [n][ldb] float32, uint8, binary16 or bfloat16 (base_u8 says which), or NULL */
    int base_u8, ldb;            /* base_u8 is the FORMAT of the base rows (since v2500, (3o)): 0 f32, 1 uint8, LSQ_BASE_F16, LSQ_BASE_BF16; any other non-zero value
                                    means uint8, as it did while the field was a flag.  ldb in elements */
    int on_device;
} lsq_index_desc;
typedef struct lsq_index_stats {
    int64_t queries;             /* queries answered (search + rerank), accumulated since creation */
    int64_t rows;                /* candidate rows gathered by stage two */
    int64_t invalid;             /* candidate ids outside the base: skipped, never dereferenced */
    int64_t batches;             /* batches of stage two */
    double scan_ms, gather_ms, select_ms;      /* with the context's option "profile" = 1: stage one; stage two's distances; stage two's sort + hand-out */
} lsq_index_stats;
LSQ_API int lsq_index_create(lsq_index **out, lsq_ctx *ctx, const lsq_index_desc *desc);
LSQ_API int lsq_index_destroy(lsq_index *ix);
/* shortlist == 0: the ADC scan alone -- the results of lsq_linscan_dev bit for bit (ADC distances, 1-BASED int32 ids).
 * shortlist = L >= nn: the scan for L, then the re-rank of every query's L ids to nn -- exact distances, 1-based ids.  L <= n and L <= 2^28.
 * q_scan [nq][ldq] is what the scan reads (the ROTATED queries of linscan_lsq, R'X), q_exact [nq][ldq] what the re-rank reads (the queries in the base
 * set's own frame; may equal q_scan, ignored when shortlist == 0).  The rotation stays with the caller, as in linscan_lsq: a device GEMM would not give
 * numpy's bits.  on_device: 0 = q_scan, q_exact, dists, ids are host buffers, 1 = device buffers.  dists / ids [nq][nn]. */
LSQ_API int lsq_index_search(lsq_index *ix, float *dists, int *ids, const float *q_scan, const float *q_exact, int nq, int ldq, int shortlist, int nn,
                             int on_device);
/* Stage two alone, on the caller's candidates (see lsq_rerank_cpu; the same bits): how the 0-based shortlists of lsq_linscan_pq(_dev) are re-ranked.
 * L <= 2^28 (candidates may repeat, so L may exceed n): one query's records are one batch. */
LSQ_API int lsq_index_rerank(lsq_index *ix, float *dists, int *ids, const float *queries, const int *cand, int nq, int ldq, int L, int nn, int id_base,
                             int on_device);
LSQ_API int lsq_index_get_stats(lsq_index *ix, lsq_index_stats *out);
/* LSQ_EINVAL for all of them: a null pointer, nn > L, shortlist > n, a re-rank on an index without base rows, a search on an index without codes;
 * nothing is launched then. */

/* ---- (3f) exact k-NN on the index's resident base rows, f32 or un-widened uint8 (since v1500) -----------------------------------------------------
 * The ground truth of a recall figure (what the reference reads from sift_groundtruth.ivecs and feeds to eval_recall, src/linscan/Linscan.jl:76-117)
 * from the base the index already holds: a .bvecs set is never widened to f32, on the host or in HBM.  ONE contract for every road: per query the nn
 * smallest (dist, id) pairs over the base rows, dist with the bits lsq_knn_exact gives for the same (query, row) on the widened matrices, ties to the
 * smaller id, NaN last; ids int32 in the caller's id_base (0 or 1) as in lsq_index_rerank.
 *   f32 base:                      lsq_knn_exact_dev on the resident rows, ids shifted by id_base.
 *   uint8 base, f32 queries or d > 258:  the same kernel, bytes widened in registers (exact).
 *   uint8 base, uint8 queries, d <= 258: D = |x|^2 + |q|^2 - 2<x, q> in 32-bit integers (v_dot4_u32_u8), dist = (float)D.  The same bits: every term of the
 *        f32 chain is an integer <= 255^2 and its partial sums only grow, so while the final D <= 2^24 no step rounds; d*255^2 <= 2^24 up to d = 258.
 * queries [nq][ldq] f32 (queries_u8 = 0, 4-byte aligned) or uint8 (queries_u8 = 1, any byte alignment), ldq in ELEMENTS; dists / ids [nq][nn];
 * on_device: 0 = queries, dists, ids are host buffers, 1 = device buffers.  The call uses the index's own scan state; options "linscan_exhaustive",
 * "linscan_rank" and "profile" act as on lsq_knn_exact_dev, "knn_u8_int" = 0 takes the integer road out.
 * LSQ_EINVAL, nothing launched: an index without base rows, nn < 1, nn > n, nq < 1, ldq < d, an id_base other than 0 / 1, f32 queries not 4-byte
 * aligned, a null pointer. */
LSQ_API int lsq_index_knn(lsq_index *ix, float *dists, int *ids, const void *queries, int queries_u8, int nq, int ldq, int nn, int id_base, int on_device);
/* what the LAST lsq_index_knn call did (a struct of its own: lsq_index_stats is ABI and keeps its size) */
typedef struct lsq_index_knn_info {
    int64_t queries, rows, batches;      /* queries answered, base rows scanned, batches of the selection */
    int64_t fallback_queries;            /* queries redone by the exhaustive road */
    int64_t exhaustive;                  /* 1 = every distance written and sorted */
    int64_t int_road;                    /* 1 = the integer road ran */
    double norms_ms, scan_ms, select_ms; /* with option "profile" = 1: the integer road's norms; sample + scan; sort + hand-out */
} lsq_index_knn_info;
LSQ_API int lsq_index_get_knn_info(lsq_index *ix, lsq_index_knn_info *out);
/* The host drop-in and checker (no context): lsq_knn_exact_cpu for base rows and queries that are f32 or uint8 (base_u8 / queries_u8) at ANY byte
 * alignment, ldb / ldq in elements; uint8 elements are widened (exact) and the f32 chain runs: the bits of lsq_knn_exact_cpu on the widened matrices.
 * ids uint32 0-based.  LSQ_EINVAL as lsq_knn_exact_cpu.  base_u8 = LSQ_BASE_F16 / LSQ_BASE_BF16 (since v2500, (3o)): half rows, widened likewise. */
LSQ_API int lsq_knn_exact_u8_cpu(float *dists, uint32_t *ids, const void *base, int base_u8, const void *queries, int queries_u8, int n, int nq, int d,
                                 int ldb, int ldq, int nn, int nthreads);

/* ---- (3g) inverted lists (IVF) on the resident index: a search that reads only the probed lists (since v1700) ------------------------------------
 * THE REFERENCE HAS NO COUNTERPART: linscan_lsq (src/linscan/Linscan.jl:46-73) reads every code for every query.  Here a coarse partition -- nlist
 * centroids and the list of every row, both the caller's (the library neither trains nor assigns them) -- is laid over an index that holds codes, and
 * a query reads the rows of its nprobe nearest lists alone.
 *   probed lists   the nprobe smallest (dist, list id) pairs, dist = lsq_knn_exact's distance of the query's q_coarse row to the centroid (f32 direct
 *                  form, dimensions ascending, every op rounded, no FMA), ties to the smaller id, NaN last: the exact search with the centroids as base.
 *   distance       of a row i of a probed list l: lsq_linscan's bits, (((0 + table[0 h + b_i0]) + table[1 h + b_i1]) + ...) + dbnorms[i], the tables built
 *                  from the query's q_scan row; with LSQ_IVF_ADD_COARSE one more rounded add, (... + dbnorms[i]) + dist(q, l) -- what residual codes need
 *                  (encode x - c_l, store |r^|^2 + 2<c_l, r^> as dbnorms: the sum is |q - c_l - r^|^2).
 *   result         per query the nn smallest (dist, id) pairs over all rows of its probed lists, lexicographic; ids are the ORIGINAL row ids, 1-BASED int32
 *                  as in lsq_index_search; ties to the smaller original id; NaN after every number; where the probed lists hold fewer than nn rows the
 *                  remaining entries are (+inf, 0), after everything, NaN included (lsq_index_rerank's id outside the base).  Empty lists are legal.
 *   shortlist      0: the result above.  L >= nn: the result above for L, then lsq_index_rerank's stage two on those ids with q_exact: exact distances;
 *                  the (+inf, 0) entries are never dereferenced and stay last.  L <= 2^28.
 * With nprobe = nlist and no flag the result is lsq_index_search(shortlist = 0)'s bit for bit.  lsq_index_search, _rerank and _knn are unchanged by lists.
 * lsq_index_set_lists builds the inverted layout on the device -- rows grouped by list and, within a list, ascending by original id: one radix sort of
 * (list, row) keys, no atomic decides a position, the same bits on every call -- as OWNED copies (m + 8 bytes per row: codes, norm, original id; whether
 * the index borrows its codes or not), plus the centroids and nlist + 1 offsets.  It may be called again to replace the lists; a call that fails its
 * range check (made on the device before anything is laid out) leaves the former lists in place.  centroids / list_of_row: host (on_device = 0) or device.
 * lsq_index_search_ivf: q_scan, q_coarse (NULL = q_scan), q_exact (read when shortlist > 0) [nq][ldq] f32; dists / ids [nq][nn]; on_device as in
 * lsq_index_search.  Two roads, the same results: every record of every probed row written and sorted (LSQ_IVF_EVERY_RECORD forces it; it is also the
 * fallback), or the HEAD -- the first probed lists, in rank order, that hold nn rows together -- written in full, its nn-th record an exact upper bound
 * tau of the answer's nn-th, and the other lists appending only records with !(dist > tau) to 8 nn + 256 further slots; a query that overflows them is
 * redone on the first road.  LSQ_IVF_TEST_BATCH is a test hook: batches of at most 8 queries (lsq_ivf_info.batch_queries says what a call used).
 * Runs on the context's stream with the index's own scratch; options "linscan_exhaustive" / "linscan_rank" act on the coarse search, "profile" fills
 * the four times.
 * LSQ_EINVAL, nothing launched: a null handle or pointer, an index without codes, a search before set_lists, nprobe outside 1 .. nlist, nlist outside
 * 1 .. 2^24, nn < 1, shortlist neither 0 nor >= nn, shortlist > 0 without base rows, a flag outside the three.  A list_of_row entry outside [0, nlist)
 * is LSQ_EINVAL too, found by the one kernel that reads the entries, before any of them is used as an offset. */
typedef struct lsq_ivf_desc {
    int nlist;
    const float *centroids;        /* [nlist][d] */
    const int32_t *list_of_row;    /* [n], 0-based list of every row */
    int on_device;
} lsq_ivf_desc;
enum { LSQ_IVF_ADD_COARSE = 1, LSQ_IVF_EVERY_RECORD = 2, LSQ_IVF_TEST_BATCH = 4 };
typedef struct lsq_ivf_info {            /* the last lsq_index_search_ivf call */
    int64_t queries, probed_rows;        /* queries answered; rows of their probed lists, summed */
    int64_t records;                     /* records written to the sort's input, padding included, both roads */
    int64_t threshold_queries;           /* queries answered by the thresholded road */
    int64_t fallback_queries;            /* queries whose tail overflowed: redone with every record */
    int64_t batches;
    int64_t batch_queries, tail_capacity;        /* the plan: queries per batch (the larger of the two roads'), tail slots per query */
    double coarse_ms, lut_ms, scan_ms, select_ms;        /* with option "profile" = 1 */
} lsq_ivf_info;
LSQ_API int lsq_index_set_lists(lsq_index *ix, const lsq_ivf_desc *desc);
LSQ_API int lsq_index_search_ivf(lsq_index *ix, float *dists, int *ids, const float *q_scan, const float *q_coarse, const float *q_exact, int nq, int ldq,
                                 int nprobe, int shortlist, int nn, int flags, int on_device);
LSQ_API int lsq_index_get_ivf_info(lsq_index *ix, lsq_ivf_info *out);
/* The host checker and engine-less road (no context, std::thread workers, nthreads 0 = all): the index's ingredients as plain arrays -- codes [n][m],
 * codebooks [m*h][d], dbnorms [n], centroids [nlist][d], list_of_row [n] -- and the contract's result for shortlist = 0.  Tables and distances by
 * lsq_linscan_aqd_query_extra_byte's arithmetic, coarse distances by lsq_knn_exact_cpu's.  It walks the rows in their original order and knows nothing of
 * the inverted layout.  q_coarse NULL = q_scan.  LSQ_EINVAL as above, and for h outside 1 .. 256, m < 1, d < 1, n < 1, nq < 0, ldq < d. */
LSQ_API int lsq_ivf_search_cpu(float *dists, int *ids, const uint8_t *codes, const float *codebooks, const float *dbnorms, const float *centroids,
                               const int32_t *list_of_row, const float *q_scan, const float *q_coarse, int n, int m, int h, int d, int nlist, int nq,
                               int ldq, int nprobe, int nn, int flags, int nthreads);

/* ---- (3h) the packed index: rows of m code bytes and ONE norm byte, searched as stored (since v1800) ---------------------------------------------------
 * What the reference computes for a base set is m code bytes and one norm byte per vector -- quantize_norms' index into the <= 256 scalar centroids
 * cbnorms that train_lsq learns (src/utils.jl:6-31): the "64-bit code" at m = 7 -- and what it searches is the widened array cbnorms[index]
 * (demos/demo_lsq_gpu.jl:57-60).  A packed index keeps the byte: row i is its m code bytes followed by its norm byte c_i, m + 1 bytes in an allocation
 * the index OWNS, and cbnorms is held once per index.  THE CONTRACT IS AN IDENTITY: every call on a packed index returns bit for bit what the same call
 * returns on an lsq_index_create index with dbnorms[i] = cbnorms[c_i] -- distances, ids, tie order, NaN order, padding records.  The arithmetic is
 * lsq_linscan's, dist = ((((0 + t_0) + t_1) + ...) + t_{m-1}) + cbnorms[c_i], the last operand read from a 256-entry table beside the query tables
 * instead of from a float per row.  lsq_index_search, _set_lists, _search_ivf, _rerank, _knn and their getters take a packed index unchanged; the
 * inverted layout of a packed index holds m + 5 bytes per row (the packed row and the original id).  The scans read rows as dwords when m + 1 is a
 * multiple of 4 (m = 3, 7, 11, 15), as bytes otherwise.
 *   codes [n][m] uint8 0-based; norm_codes [n] uint8 0-based (lsq_quantize_norms_dev's d_idx_out as it is); cbnorms [ncb] f32, 1 <= ncb <= 256.  The three
 *   are read ONCE, in stream order, before the call returns -- on_device = 1 included: the caller may free or overwrite them afterwards.  codebooks and base
 *   are copied (on_device = 0) or borrowed (on_device = 1) exactly as in lsq_index_create.
 * LSQ_EINVAL: the limits of lsq_index_create; codes == NULL (a base-only index is lsq_index_create's); a null norm_codes, cbnorms or codebooks; ncb outside
 * 1 .. 256; a norm byte >= ncb -- found on the device by the one kernel that reads the bytes, which counts them, before the index exists: *out stays
 * NULL and nothing is kept. */
typedef struct lsq_index_packed_desc {
    int64_t n;
    int d, m, h;
    const uint8_t *codes;        /* [n][m] uint8 0-based */
    const uint8_t *norm_codes;   /* [n] uint8 0-based */
    const float *cbnorms;        /* [ncb] */
    int ncb;
    const float *codebooks;      /* [m*h][d] */
    const void *base;            /* [n][ldb] float32 or uint8, or NULL */
    int base_u8, ldb;
    int on_device;
} lsq_index_packed_desc;
typedef struct lsq_index_packed_info {   /* all zero on an index that is not packed */
    int64_t row_bytes;                   /* m + 1 */
    int64_t ivf_row_bytes;               /* m + 5 once lists are set, else 0 */
    int64_t ncb;
    int64_t dword_rows;                  /* 1 = the scans read rows as dwords */
    int64_t resident_bytes;              /* the packed rows and the norm table: n (m + 1) + 4 ncb */
} lsq_index_packed_info;
LSQ_API int lsq_index_create_packed(lsq_index **out, lsq_ctx *ctx, const lsq_index_packed_desc *desc);
LSQ_API int lsq_index_get_packed_info(lsq_index *ix, lsq_index_packed_info *out);
/* The selection statistics of the LAST lsq_index_search call's scan (any index; lsq_get_linscan_stats' struct, this call's figures alone): exhaustive,
 * threshold_rank, list_capacity, candidates, fallback_queries, batches -- what tells a scan that sampled other rows from one that did not when the
 * fallback road has repaired the results. */
LSQ_API int lsq_index_get_scan_stats(lsq_index *ix, lsq_linscan_stats *out);

/* ---- (3i) the coarse partition: building a residual inverted-list index resident on the device (csrc/lsq_partition.hip; since v1900) ---------------------
 * THE REFERENCE HAS NO COUNTERPART.  (3g) searches residual codes (LSQ_IVF_ADD_COARSE); these eleven symbols BUILD them: every step between "a base set
 * in HBM" and "a residual index with lists set" that is not already the resident trainer's or encoder's -- nearest centroid, cluster means, residuals,
 * the scalar a residual row stores -- on f32 rows or the un-widened uint8 rows of a .bvecs set, each with a host checker that fixes its bits.
 * The handle: lsq_partition_create COPIES nlist x d f32 centroids (host memory, or device memory with on_device = 1) -- lsq_partition_update replaces
 * them, so they are never borrowed --, owns its scratch and runs on the context's device and on the stream the context is bound to at each call; the
 * context must outlive it; like the context it serves one host thread at a time.  Nothing of the context is written: calls on the partition and calls
 * on the context, or on an index or encoder of the same context, do not disturb each other.
 * X [n][ldx] f32 (x_u8 = 0, 4-byte aligned) or uint8 (x_u8 = 1, any byte alignment); ldx, ldr in ELEMENTS; only the first d elements of a row are read
 * or written.  on_device: 0 = every array of the call is a host buffer (uploaded, computed, downloaded), 1 = device buffers.  Every call waits for the
 * device (a control word comes back); n = 0 is LSQ_OK and touches nothing.
 *
 * assign      list_of_row[i] = the first of the (dist, list id) pairs of lsq_index_knn / lsq_knn_exact with the centroids as base and nn = 1: f32
 *             direct form, dimensions ascending, every op rounded, no FMA; ties to the smaller list, NaN last -- the rule lsq_index_search_ivf probes by
 *             and the ids lsq_knn_exact_u8_cpu returns for (base = centroids, queries = X).  uint8 rows are widened in registers (exact).  dist
 *             (optional, [n]) receives the distance.  The search is the exact search of (3f) on a base-only index inside the handle.
 * update      one Lloyd half-step.  For every list l with at least one row and every dimension t: the values (double)x_it of its rows in ASCENDING ROW
 *             ID, added one after another from +0.0 in float64, divided by (double)count and rounded to f32 (numpy: np.add.at on float64 sums, then
 *             sums / counts and .astype(float32)).  A list without rows keeps its centroid's bits.  counts (optional, [nlist] int32) receives the list
 *             sizes.  No atomics: rows are grouped by the radix sort of lsq_index_set_lists, two calls give the same bits.
 * residuals   R[i][t] = x_it - c_{l_i, t}: one rounded f32 subtraction (uint8 widened first, exact); NaN, +-inf and -0.0 as IEEE gives them.  By what
 *             the base pointer and the pitch in bytes are both multiples of, four components of an f32 row travel as one 16-byte load or four
 *             dwords, four of a uint8 row as one dword or four bytes (lsq_partition_info.loader_bytes: 16, 4 or 1).
 * code_norms  the scalar a residual index stores.  With r^_t the reconstruction of a row's codes in lsq_quantize_norms' order (codebooks ascending from
 *             the first codeword) and c the centroid of the row's list:  a = chain over t ascending of a + r^_t r^_t from 0 (the bits of
 *             lsq_quantize_norms_dev's norms);  b = chain of b + c_t r^_t from 0;  s = a + (b + b); every product and add rounded, no FMA.  norms
 *             (optional with cbnorms) receives s.  With cbnorms (1 <= ncb <= 256): norm_codes (optional) the 0-based first minimum of
 *             (s - cbnorms[j])^2 in f32 (lsq_quantize_norms' rule), dbnorms (optional) cbnorms[code] -- what lsq_index_create and
 *             lsq_index_create_packed take.  With cbnorms NULL, norms must be given and the other two outputs are ignored.  codes [n][m] uint8
 *             0-based, codebooks [m*h][d], h = 256, 1 <= m <= 16.
 * LSQ_EINVAL, nothing launched: a null handle or pointer, nlist outside 1 .. 2^24, d < 1, n < 0 or n > 2^31 - 2, ldx < d, ldr < d, f32 rows not 4-byte
 * aligned, h != 256, m outside 1 .. 16, ncb outside 1 .. 256.  A list_of_row entry outside [0, nlist) is LSQ_EINVAL too: it is found on the device and never
 * used as an offset; update then leaves the centroids as they were, residuals and code_norms leave their outputs unspecified. */
typedef struct lsq_partition lsq_partition;
typedef struct lsq_partition_desc {
    int nlist, d;
    const float *centroids;      /* [nlist][d] */
    int on_device;
} lsq_partition_desc;
enum { LSQ_PARTITION_ASSIGN = 1, LSQ_PARTITION_UPDATE = 2, LSQ_PARTITION_RESIDUALS = 3, LSQ_PARTITION_CODE_NORMS = 4 };
typedef struct lsq_partition_info {      /* the last call on the handle */
    int64_t call;                        /* LSQ_PARTITION_*: which one (0: none yet) */
    int64_t rows;                        /* n */
    int64_t lists_touched, empty_lists;  /* update: lists with rows (their centroids were replaced) and without; other calls: 0 */
    int64_t loader_bytes;                /* residuals: 16, 4 or 1 -- how wide the loads of X were; update: the element size; other calls: 0 */
    int64_t max_list_rows;               /* update: the longest list (the longest chain of dependent float64 adds) */
    double group_ms, kernel_ms;          /* with the context's option "profile" = 1: update's keys + sort + offsets; the call's own kernel (assign: the search) */
} lsq_partition_info;
LSQ_API int lsq_partition_create(lsq_partition **out, lsq_ctx *ctx, const lsq_partition_desc *desc);
LSQ_API int lsq_partition_destroy(lsq_partition *p);
LSQ_API int lsq_partition_get_centroids(lsq_partition *p, float *out, int on_device);
LSQ_API int lsq_partition_get_info(lsq_partition *p, lsq_partition_info *out);
LSQ_API int lsq_partition_assign(lsq_partition *p, const void *X, int x_u8, int64_t n, int ldx, int32_t *list_of_row, float *dist, int on_device);
LSQ_API int lsq_partition_update(lsq_partition *p, const void *X, int x_u8, int64_t n, int ldx, const int32_t *list_of_row, int32_t *counts,
                                 int on_device);
LSQ_API int lsq_partition_residuals(lsq_partition *p, const void *X, int x_u8, int64_t n, int ldx, const int32_t *list_of_row, float *R, int ldr,
                                    int on_device);
LSQ_API int lsq_partition_code_norms(lsq_partition *p, const uint8_t *codes, const float *codebooks, int64_t n, int m, int h,
                                     const int32_t *list_of_row, const float *cbnorms, int ncb, float *norms, uint8_t *norm_codes, float *dbnorms,
                                     int on_device);
/* The host checkers and engine-less roads (no context, std::thread workers, nthreads 0 = all): the three contracts above on plain arrays, bit for bit.
 * centroids [nlist][d]: read (residuals, code_norms) or updated in place (update).  assign's checker is lsq_knn_exact_u8_cpu with nn = 1 and the
 * centroids as base.  LSQ_EINVAL as above; a list_of_row entry outside [0, nlist) is found before anything is written. */
LSQ_API int lsq_partition_update_cpu(float *centroids, int32_t *counts, const void *X, int x_u8, int64_t n, int d, int ldx, const int32_t *list_of_row,
                                     int nlist, int nthreads);
LSQ_API int lsq_partition_residuals_cpu(float *R, int ldr, const void *X, int x_u8, int64_t n, int d, int ldx, const float *centroids,
                                        const int32_t *list_of_row, int nlist, int nthreads);
LSQ_API int lsq_partition_code_norms_cpu(float *norms, uint8_t *norm_codes, float *dbnorms, const uint8_t *codes, const float *codebooks,
                                         const float *centroids, const int32_t *list_of_row, int64_t n, int m, int h, int d, int nlist,
                                         const float *cbnorms, int ncb, int nthreads);

/* ---- (3j) row filters on the resident index: search only the allowed rows (csrc/lsq_filter.hip; since v2000) -------------------------------------------
 * THE REFERENCE HAS NO COUNTERPART: its scan answers over every code.  A filter is a set A of allowed rows, 0 <= row < n, OWNED by the index: deletions
 * (a tombstone list with LSQ_FILTER_DENY), predicates (a boolean mask the caller computed), and the ground truth of a filtered recall figure
 * (lsq_index_knn under the same filter).  An index without a filter behaves exactly as before v2000.
 *   contract     while a filter is set, lsq_index_search, lsq_index_search_ivf and lsq_index_knn return, per query, THE RESULT THE SAME CALL WOULD RETURN
 *                FOR nn = (all candidate rows), WITH EVERY ROW OUTSIDE A REMOVED, TRUNCATED TO nn.  The distance bits of every returned row and their
 *                order -- (dist, id) lexicographic, ties to the smaller original id, NaN after every number -- are unchanged; ids are the original ones
 *                in the id base the call already uses.  Where fewer than nn allowed rows exist (or are probed) the remaining entries are
 *                (+inf, id_base - 1), after everything, NaN included: (+inf, 0) for the 1-based searches, what lsq_index_search_ivf already returns past
 *                its probed rows.  nn <= n stays the argument rule; nn > |A| is legal.
 *   shortlist    shortlist = L: stage one under the filter for L, then stage two as it is; padding entries are never dereferenced and stay last.
 *   re-rank      lsq_index_rerank IGNORES the filter: the candidates are the caller's choice.
 *   identities   a filter that allows every row, and a cleared filter, give the unfiltered call's result bit for bit.
 *   lists        the filter and the inverted lists are independent: lsq_index_set_lists and lsq_index_set_filter may be called in either order and
 *                either may be replaced later.  lsq_ivf_info.probed_rows counts the filtered rows of the probed lists too (they are read); the head of
 *                the thresholded road is chosen on ALLOWED counts, so its nn-th record is a finite, exact bound whenever the probed lists hold nn
 *                allowed rows.
 *   inputs       LSQ_FILTER_BITS: uint32 [ceil(n/32)], bit (i & 31) of word i >> 5 = row i; bits at or past n are ignored.  LSQ_FILTER_BYTES: uint8
 *                [n], non-zero = set (a numpy / torch bool array as it is).  LSQ_FILTER_IDS: int32 [count] row ids in id_base (0 or 1), duplicates
 *                legal.  LSQ_FILTER_DENY: the set rows are the EXCLUDED ones.  on_device: 0 = a host array, 1 = a device array.  The filter is always a
 *                copy (n/8 bytes, 4 bytes per 32 rows of prefix and 4 bytes per allowed row; with inverted lists the same bitmap and prefix once more in
 *                layout order): the caller's array may be freed or changed when the call returns.  desc == NULL clears the filter.
 *   roads        dense: the scans read every row and the bit beside it; a filtered row leaves as the record of an id outside the base.  compact: the
 *                scans walk the ascending list of allowed rows.  The same distances, bit for bit.  Compact is taken when allowed <=
 *                lsq_filter_info.crossover_rows (n / 2, measured) -- except, on an index of more than 65 536 rows, for 65 536 allowed rows or fewer
 *                with allowed * c > n (c = 64 for lsq_index_search, 8 for lsq_index_knn): so few rows take the selection that writes and sorts every
 *                distance, which costs c dense steps per row.  LSQ_FILTER_FORCE_DENSE / _COMPACT are test hooks that override the rule.
 *                lsq_index_search_ivf reads the inverted layout with the filter's bits in layout order (there is no compact form of the layout).
 * LSQ_EINVAL with nothing changed and the former filter left in place: a null handle, null data, an unknown form or flag, both FORCE flags, count < 0, an
 * id_base other than 0 / 1, an IDS entry outside [id_base, id_base + n) -- found by the one kernel that reads the entries, which counts them, before any
 * of them is used as an address. */
enum { LSQ_FILTER_BITS = 0, LSQ_FILTER_BYTES = 1, LSQ_FILTER_IDS = 2 };                    /* form */
enum { LSQ_FILTER_DENY = 1, LSQ_FILTER_FORCE_DENSE = 2, LSQ_FILTER_FORCE_COMPACT = 4 };    /* flags; the two FORCE flags are test hooks */
typedef struct lsq_filter_desc {
    int form;
    const void *data;     /* BITS: uint32 [ceil(n/32)]; BYTES: uint8 [n]; IDS: int32 [count] */
    int64_t count;        /* IDS only */
    int id_base;          /* IDS only: 0 or 1 */
    int flags;            /* LSQ_FILTER_DENY | one FORCE flag */
    int on_device;
} lsq_filter_desc;
typedef struct lsq_filter_info {
    int64_t active, n, allowed;
    int64_t lists, lists_without_allowed;   /* 0 / 0 without inverted lists (or without a filter) */
    int64_t road;                           /* last search / knn call: 0 unfiltered, 1 dense, 2 compact */
    int64_t crossover_rows;                 /* compact road taken by default when allowed <= this (and outside the band described above) */
} lsq_filter_info;
LSQ_API int lsq_index_set_filter(lsq_index *ix, const lsq_filter_desc *desc);   /* desc == NULL clears */
LSQ_API int lsq_index_get_filter_info(lsq_index *ix, lsq_filter_info *out);

/* ---- (3k) appending rows to the resident index: lsq_index_add, with the inverted lists merged on the device (csrc/lsq_grow.hip; since v2100) ---------------
 * THE REFERENCE HAS NO COUNTERPART.  An index of n rows takes `count` more: they become rows n .. n + count - 1 (0-based).
 *   contract     (Identity G) after a successful lsq_index_add EVERY CALL ON THE INDEX RETURNS, BIT FOR BIT, WHAT IT RETURNS ON AN INDEX FRESHLY BUILT over
 *                the concatenated arrays, given lsq_index_set_lists with the same centroids and the concatenated list_of_row, and a filter that is the old
 *                allowed set plus every new row: distances, ids, tie order, NaN order, padding records, and the deterministic statistics (the layout is
 *                the same array for array).  Codebooks, centroids and cbnorms are the index's own and do not change.
 *   filter       new rows are ALLOWED.  A caller with a predicate sets its filter again; lsq_index_set_filter afterwards sees the new n.
 *   ownership    an index created with on_device = 1 BORROWS codes, norms and base.  The first add with count > 0 (or the first reserve) ADOPTS them: one
 *                device-to-device copy into owned storage with capacity; when that call has returned the caller's arrays are never read again.
 *                Codebooks stay borrowed.  The arrays of lsq_index_add_desc are read once, in stream order, before the call returns (on_device = 1
 *                too).  The owned base keeps the index's pitch; added rows of another pitch are re-pitched on the way in.
 *   capacity     growth is geometric, FACTOR 3/2: an add that does not fit re-allocates to max(n + count, capacity + capacity / 2) rows.  Re-allocation
 *                keeps the contents (allocate, copy, swap, free): THE TRANSIENT PEAK IS OLD PLUS NEW.  lsq_index_reserve(rows) makes the adds up to `rows`
 *                rows free of RE-ALLOCATION OF THE INDEX'S OWNED STORAGE -- the flat arrays and both halves of the layout: what `reallocations` counts.  Scratch
 *                is not covered: the keys and workspace of the sort, the filter's spare buffers and a packed index's staging are sized at the first add
 *                that needs them (a few MB at 10^6 rows) and kept.  The inverted layout is kept in two capacity-sized halves (the merge is written out of place into the spare
 *                one): with lists, the layout's bytes are resident twice from the first add on.
 *   atomicity    validate first, commit last.  A REFUSED call (LSQ_EINVAL) leaves the index exactly as it was: every answer, every info struct, n, lists and
 *                filter.  The list ids and the norm bytes of the new rows are range-checked on the device, by the one kernel that reads them, before any
 *                is used as an offset and before anything of the index is written.  A call that fails later (LSQ_ENOMEM, LSQ_EHIP) leaves every answer,
 *                n, the lists and the filter as they were -- nothing is committed before the last step --, but the storage may already have moved:
 *                lsq_index_growth_info.capacity_rows and .adopted may have grown (adopted storage holds the same rows; `reallocations` is not advanced).
 * LSQ_EINVAL (nothing launched unless noted): a null handle or desc; count < 0; n + count > 2^31 - 2; a required array missing; dbnorms given to a packed
 * index or norm_codes to a plain one; list_of_row given when no lists are set; ldb < d; an f32 base that is not 4-byte aligned; a list_of_row entry outside
 * [0, nlist) (device); a norm byte >= ncb (device); reserve(rows < n).  count == 0 is a legal no-op and adopts nothing. */
typedef struct lsq_index_add_desc {
    int64_t count;               /* rows appended: they become rows n .. n + count - 1 (0-based) */
    const uint8_t *codes;        /* [count][m] uint8 0-based        -- required iff the index holds codes */
    const float   *dbnorms;      /* [count]                         -- required iff plain index with codes */
    const uint8_t *norm_codes;   /* [count] uint8 0-based           -- required iff packed index */
    const void    *base;         /* [count][ldb] f32 or uint8, the index's own type -- required iff the index holds base rows */
    int ldb;                     /* pitch of `base` in elements, >= d; need not equal the index's pitch */
    const int32_t *list_of_row;  /* [count] 0-based list ids        -- required iff lists are set */
    int on_device;               /* 0 host arrays, 1 device arrays -- independent of how the index was created */
} lsq_index_add_desc;
typedef struct lsq_index_growth_info {
    int64_t n, capacity_rows;    /* rows held; rows the owned storage holds without another allocation (n while the arrays are borrowed) */
    int64_t adds, rows_added;    /* successful lsq_index_add calls with count > 0 since creation; their rows */
    int64_t reallocations;       /* times owned storage was re-allocated by add / reserve (one per call that re-allocated) */
    int64_t adopted;             /* 1 once borrowed arrays have been copied into owned storage */
    int64_t merged_rows;         /* last add: positions of the inverted layout written (0 without lists) */
    double append_ms, merge_ms, filter_ms;   /* last add, with option "profile" = 1 */
} lsq_index_growth_info;
LSQ_API int lsq_index_add(lsq_index *ix, const lsq_index_add_desc *desc);
LSQ_API int lsq_index_reserve(lsq_index *ix, int64_t rows);       /* capacity for at least `rows` rows in total */
LSQ_API int lsq_index_get_growth_info(lsq_index *ix, lsq_index_growth_info *out);

/* ---- (3l) removing rows from the resident index: lsq_index_remove (tombstones) and lsq_index_compact (the rows leave; csrc/lsq_compact.hip; since v2200) ----
 * THE REFERENCE HAS NO COUNTERPART.
 *   remove       (Identity R) after a successful lsq_index_remove the index is, for every call and every field of lsq_filter_info but `road`, the index
 *                after lsq_index_set_filter(BITS = (the allowed set in force, or every row if none) minus the given rows).  A FORCE flag of the filter in
 *                force stays.  Duplicates and rows already removed are legal; count == 0 is a no-op and creates no filter.  The ids are range-checked on
 *                the device by the one kernel that reads them, before any is used as an address and before anything is written: a refused call leaves
 *                the filter and every answer as they were.  lsq_index_rerank ignores the filter, as ever.
 *   compact      A = the allowed set in force, n' = |A| >= 1.  The rows outside A LEAVE: the surviving rows keep their order and become rows 0 .. n' - 1
 *                (old_of_new = the filter's ascending row list).  (Identity C) afterwards EVERY CALL ON THE INDEX RETURNS, BIT FOR BIT, WHAT IT RETURNS ON
 *                AN INDEX FRESHLY BUILT over the surviving rows in that order, given lsq_index_set_lists with the same centroids and the survivors' lists
 *                (same nlist: lists may become empty) and NO filter: distances, ids, tie order, NaN order, padding records, every deterministic statistic
 *                (the layout is the same array for array).  (Identity M) for nn <= n' the filtered answer before the call and the answer after it have the
 *                same distance bits, and id_after = new_of_old[id_before].  Codebooks, centroids and cbnorms do not change.  The filter is cleared.
 *                Without an active filter nothing is dropped (LSQ_OK, identity maps; LSQ_COMPACT_SHRINK still acts).
 *   ownership    a borrowing index (on_device = 1, never added to) is ADOPTED BY THE GATHER: the survivors are written straight from the caller's arrays
 *                into owned storage; the caller's arrays are never written, and never read once the call has returned.  (Without an active filter and
 *                without LSQ_COMPACT_SHRINK nothing moves and a borrowing index keeps borrowing.)
 *   capacity     capacity_rows is kept: adds into the freed rows re-allocate nothing.  LSQ_COMPACT_SHRINK sizes the owned arrays and both halves of the
 *                layout to n' rows.
 *   atomicity    validate, allocate, write beside, one wait, commit.  A refused call changes nothing; a call that fails later (LSQ_ENOMEM, LSQ_EHIP) leaves
 *                every answer, n, the lists and the filter as they were.  THE PRICE: until the commit the old and the new arrays coexist -- the transient
 *                peak is old plus new of everything the index owns.
 * LSQ_EINVAL: a null handle; remove: count < 0 or > 2^31 - 1, null ids with count > 0, id_base not 0 or 1, an id outside [id_base, id_base + n) (device);
 * compact: unknown flags, id_base not 0 or 1, no allowed row. */
enum { LSQ_COMPACT_SHRINK = 1 };
typedef struct lsq_index_compact_desc {
    int32_t *old_of_new;         /* optional out [allowed]: the former row of every new row, ascending, in id_base */
    int32_t *new_of_old;         /* optional out [n]: the new row of every former row in id_base, -1 for a removed row */
    int id_base;                 /* 0 or 1, for both maps */
    int flags;                   /* LSQ_COMPACT_SHRINK */
    int on_device;               /* 0 host arrays, 1 device arrays (the maps) */
} lsq_index_compact_desc;
typedef struct lsq_index_compact_info {
    int64_t n_before, n_after;   /* last compact */
    int64_t removes, rows_tombstoned;    /* successful lsq_index_remove calls with count > 0 since creation; the bits they newly cleared */
    int64_t compactions, rows_dropped;   /* successful lsq_index_compact calls since creation; the rows that left */
    int64_t moved_bytes;         /* last compact: destination bytes written, flat arrays plus layout */
    int64_t shrunk;              /* last compact: 1 when LSQ_COMPACT_SHRINK re-sized the storage */
    double tombstone_ms, gather_ms, layout_ms;   /* last remove; last compact's flat gather and layout phases -- with option "profile" = 1 */
} lsq_index_compact_info;
LSQ_API int lsq_index_remove (lsq_index *ix, const int32_t *ids, int64_t count, int id_base, int on_device);
LSQ_API int lsq_index_compact(lsq_index *ix, const lsq_index_compact_desc *desc);   /* desc == NULL: no map wanted, no flags */
LSQ_API int lsq_index_get_compact_info(lsq_index *ix, lsq_index_compact_info *out);

/* ---- (3m) range search on the resident index: every row within a radius (csrc/lsq_range.hip; since v2300) ----------------------------------------------
 * THE REFERENCE HAS NO COUNTERPART.  For every query q with radius r_q the result is every (dist(q, i), id_i) over the CANDIDATE ROWS i with
 * dist(q, i) <= r_q, in (dist, id) lexicographic order -- no padding, no truncation, a result of variable length.
 *   candidates   nprobe == 0: every row of the index.  nprobe >= 1: the rows of the query's nprobe nearest lists, chosen as lsq_index_search_ivf chooses
 *                them.  Under a row filter (3j): the allowed rows among those.
 *   dist         bit for bit the value lsq_index_search (nprobe == 0) or lsq_index_search_ivf (nprobe >= 1, with or without LSQ_IVF_ADD_COARSE) gives
 *                the same (query, row): the same tables, the same add order, the norm last, then the coarse add.
 *   comparison   IEEE <=: a NaN distance or a NaN radius returns nothing; r = +inf returns every candidate with a non-NaN distance, r = -inf nothing.
 *                Ties go to the smaller id.  Ids are original rows, 1-based, as the two search calls return them.
 *   identity     THE RESULT OF q IS THE LONGEST PREFIX WITH dist <= r_q OF THE FULL RANKING THE EXISTING CALL RETURNS FOR nn = (all candidate rows), with
 *                that ranking's own (+inf, 0) padding dropped.  So a packed index answers as the plain index with dbnorms[i] = cbnorms[c_i]; nprobe ==
 *                nlist without a flag answers as nprobe == 0; after add / remove / compact the result is that of the index identities G / R / C name.
 *   two passes   a COUNT pass and a FILL pass walk the same rows: the counts size every query's segment exactly, nothing overflows and nothing is redone.
 *                The fill runs in batches of at most 2^28 records (option "range_batch": a test hook; the results are the same for every value); a
 *                query larger than the budget is a batch of its own.
 * lsq_index_range_search writes lims [nq + 1] as a CSR -- query q's results are entries lims[q] .. lims[q + 1] - 1, lims[0] = 0 -- and HOLDS the result in
 * device buffers owned by the index (8 bytes per result).  It waits for the device (the counts come back to plan the batches).  nq == 0: LSQ_OK,
 * lims[0] = 0, an empty held result.  lsq_index_range_fetch copies the held result of the last successful range search: exactly lims[nq] entries of
 * each array; capacity < lims[nq], or no held result: LSQ_EINVAL and nothing written.  It may be called more than once.  The held result is dropped, and
 * its memory released, by the next range search on the index and by every call that changes what a search would see: lsq_index_add / _remove with
 * count > 0, lsq_index_compact, lsq_index_set_lists, lsq_index_set_filter.  Search calls do not drop it.
 * lsq_range_search_cpu is the host drop-in and the engine-less road: plain arrays, no context, std::thread workers, the arithmetic of
 * lsq_linscan_aqd_query_extra_byte and lsq_ivf_search_cpu.  centroids == NULL or nprobe == 0: every row; else list_of_row [n], nlist, nprobe, flags as
 * lsq_ivf_search_cpu takes them.  allowed (optional): [n] bytes, non-zero = the row is a candidate.  Two-call protocol: lims is always written; dists / ids
 * are written only if lims[nq] <= capacity (and both are non-null), and are otherwise untouched.
 * LSQ_EINVAL, nothing launched: a null handle or pointer (q_coarse may be null: q_scan), an index without codes, nq < 0, ldq < d, nprobe < 0, nprobe >= 1
 * before lsq_index_set_lists, nprobe > nlist, a flag other than LSQ_IVF_ADD_COARSE, LSQ_IVF_ADD_COARSE with nprobe == 0.  A refused call leaves a held
 * result as it was. */
typedef struct lsq_range_info {          /* the last lsq_index_range_search call; fields are only ever appended */
    int64_t queries;
    int64_t rows_walked;         /* rows one pass read, summed over the queries (every row / the allowed rows / the probed lists' rows) */
    int64_t results;             /* = lims[nq] */
    int64_t max_per_query;
    int64_t batches;             /* fill batches launched (a batch without records launches nothing and is not counted) */
    int64_t road;                /* 0 unfiltered, 1 dense (the bitmap beside every row), 2 compact (the allowed rows alone); 0 or 1 with nprobe >= 1 */
    int64_t held_bytes;          /* device bytes of the held result */
    double coarse_ms, lut_ms, count_ms, fill_ms, sort_ms;      /* with option "profile" = 1; sort_ms includes the hand-out */
} lsq_range_info;
/* nprobe == 0: every row (no lists needed; q_coarse ignored).  nprobe >= 1: the probed lists, rule and flags of lsq_index_search_ivf
 * (LSQ_IVF_ADD_COARSE; q_coarse NULL = q_scan).  radius [nq] f32, q_scan / q_coarse [nq][ldq]; lims [nq + 1] int64 out.
 * on_device: 0 = q_scan, q_coarse, radius, lims are host arrays, 1 = device arrays. */
LSQ_API int lsq_index_range_search(lsq_index *ix, int64_t *lims, const float *q_scan, const float *q_coarse, const float *radius,
                                   int nq, int ldq, int nprobe, int flags, int on_device);
/* dists / ids [capacity]: host (on_device = 0) or device arrays, whatever the form of the search that made the result */
LSQ_API int lsq_index_range_fetch(lsq_index *ix, float *dists, int *ids, int64_t capacity, int on_device);
LSQ_API int lsq_index_get_range_info(lsq_index *ix, lsq_range_info *out);
LSQ_API int lsq_range_search_cpu(int64_t *lims, float *dists, int *ids, int64_t capacity, const uint8_t *codes, const float *codebooks,
                                 const float *dbnorms, const float *centroids, const int32_t *list_of_row, int nlist, int nprobe, int flags,
                                 const uint8_t *allowed, const float *q_scan, const float *q_coarse, const float *radius, int n, int m, int h, int d,
                                 int nq, int ldq, int nthreads);

/* ---- (3n) decode: the vectors the codes stand for, and search by stored row (csrc/lsq_recon.hip; since v2400) -------------------------------------------
 * reconstruct(B, C)     src/utils.jl:203-223.  For a code row b (m bytes, 0-based) and codebooks K [m h][d]
 *     x^[t] = (((+0.0f + K[(0 h + b_0) d + t]) + K[(1 h + b_1) d + t]) + ...) + K[((m - 1) h + b_(m-1)) d + t]
 * in f32, every add rounded, codebooks ascending, the sum STARTING FROM +0.0 as the reference's zeros / += does: a component whose m codewords are all -0.0
 * is +0.0 (lsq_quantize_norms starts from the first codeword: fine for a norm, not for these bits).  With the coarse flag one more rounded add follows:
 * x^[t] + centroid[l][t], l the list the row belongs to (a residual index, (3i): the stored codes are of x - c_l).  Every form below returns these bits;
 * where the contract's value is a NaN the result is a NaN of any payload.
 *   lsq_reconstruct_cpu    the host checker and the engine-less road: plain arrays, no context, std::thread workers.  ids == NULL: rows 0 .. count - 1; else
 *                          ids [count] int32 in id_base.  centroids [..][d] and list_of_row [n] are read only with LSQ_RECON_ADD_COARSE.  It takes any
 *                          1 <= h <= 256 (codebook j starts at row j h of K; a code >= h: LSQ_EINVAL); an index holds h = 256 (lsq_index_create), and the
 *                          device kernel is built for that stride alone.
 *   lsq_index_reconstruct  from the index's own resident codes and codebooks.  ids == NULL: rows [start, start + count) (start 0-based); else ids [count] int32
 *                          in id_base 0 or 1, in any order, repeats allowed (start is ignored).  out [count][ldo]; ids and out are host arrays (on_device =
 *                          0) or device arrays (1).  LSQ_RECON_ADD_COARSE adds the centroid of the row's list and needs lsq_index_set_lists; the row ->
 *                          list map is derived on the device from the inverted layout and kept until lsq_index_set_lists / _add / _compact change the
 *                          layout, then rebuilt on demand.  LSQ_RECON_PAD_NAN: an id outside [id_base, id_base + n) gives a row of 0x7FC00000; it is never
 *                          dereferenced and is counted (lsq_index_recon_info.invalid) -- this is how search results decode: the (+inf, 0) padding of
 *                          lsq_index_search_ivf and the id_base - 1 of a filtered search are such ids.  Without that flag a bad id is LSQ_EINVAL, found
 *                          BEFORE anything is written to out.  Plain and packed indexes, borrowed and owned arrays, after add / remove / compact alike.
 *                          NOT AFFECTED BY A ROW FILTER (3j): a filtered-out or tombstoned row stays addressable until lsq_index_compact removes it.  The call
 *                          changes nothing a search would see: a held range result (3m) stays fetchable.  It waits for the device.  A host call (on_device =
 *                          0) is decoded and fetched in chunks of rows (64 MiB of output at a time; option "recon_chunk" = rows per chunk: a test hook,
 *                          the same bits).
 *                          LSQ_EINVAL, nothing launched: a null handle or pointer (count > 0), an index without codes, count < 0, ldo < d, a range past n, an
 *                          id_base other than 0 / 1, a flag outside the two, the coarse flag without lists.  count == 0: LSQ_OK.
 *   lsq_index_search_rows  searches whose queries are STORED ROWS: rows [nq] int32 in id_base (host or device, on_device).  The rows are decoded into staging
 *                          the index owns -- with the coarse add exactly when flags carries LSQ_IVF_ADD_COARSE -- and then nprobe == 0 is
 *                          lsq_index_search(shortlist = 0) on those queries, nprobe >= 1 is lsq_index_search_ivf(shortlist = 0, q_coarse = q_scan, flags).
 *                          THE RESULT IS BIT FOR BIT WHAT THOSE CALLS RETURN FOR q = lsq_index_reconstruct(rows, ...), the filter and the statistics
 *                          included (ids 1-based as theirs).  A composition: it adds no scan kernel.  NO SELF-EXCLUSION: with quantised norms a row need
 *                          not be its own nearest neighbour, and it is returned like any other row.  flags: those of lsq_index_search_ivf (none but 0 with
 *                          nprobe == 0).  A row outside the index: LSQ_EINVAL, dists / ids untouched. */
#define LSQ_RECON_ADD_COARSE 1
#define LSQ_RECON_PAD_NAN 2
#define LSQ_RECON_ROAD_DWORD 1       /* lsq_index_recon_info.road: dword loads and stores (odd d, odd pitch, unaligned out) */
#define LSQ_RECON_ROAD_VEC16 2       /* 16-byte loads and stores */
#define LSQ_RECON_ROAD_CODE_DWORDS 4 /* or-ed in: the code rows went by dword loads (a pitch of whole dwords), else by bytes */
typedef struct lsq_index_recon_info {    /* the last lsq_index_reconstruct / lsq_index_search_rows call; fields are only ever appended */
    int64_t rows;                /* rows decoded (valid ids) */
    int64_t invalid;             /* ids outside the index: padded with LSQ_RECON_PAD_NAN, or the reason of a refusal */
    int64_t map_rebuilt;         /* 1: this call built the row -> list map */
    int64_t map_rebuilds;        /* since the index was made */
    int64_t road;                /* LSQ_RECON_ROAD_* of the decode kernel */
    int64_t calls;               /* since the index was made */
    double map_ms, decode_ms;    /* with option "profile" = 1 */
} lsq_index_recon_info;
LSQ_API int lsq_reconstruct_cpu(float *out, int64_t ldo, const uint8_t *codes, int64_t ldc, const float *K, const int32_t *ids, int64_t count,
                                int id_base, int64_t n, int m, int h, int d, const float *centroids, const int32_t *list_of_row, int flags, int nthreads);
LSQ_API int lsq_index_reconstruct(lsq_index *ix, float *out, int64_t ldo, const int32_t *ids, int64_t start, int64_t count, int id_base, int flags,
                                  int on_device);
LSQ_API int lsq_index_search_rows(lsq_index *ix, float *dists, int *ids_out, const int32_t *rows, int nq, int id_base, int nn, int nprobe, int flags,
                                  int on_device);
LSQ_API int lsq_index_get_recon_info(lsq_index *ix, lsq_index_recon_info *out);

/* ---- (3o) half-precision base rows: binary16 and bfloat16 (csrc/lsq_half.hip; since v2500) ---------------------------------------------------------------
 * THE REFERENCE HAS NO COUNTERPART: it keeps no base rows at all (its recall figures are those of the ADC distances, src/linscan/Linscan.jl:76-117).  The
 * index's second copy of the base set -- what the exact re-rank (3e) and exact k-NN (3f) read -- may hold 2-byte elements: 2 d bytes per row beside the
 * m or m + 1 bytes of codes, instead of 4 d.
 *   LSQ_BASE_F16   IEEE binary16.          LSQ_BASE_BF16   the upper 16 bits of a binary32.
 * Both go in the base_u8 field of lsq_index_desc / lsq_index_packed_desc and in the base_u8 argument of lsq_rerank_cpu / lsq_knn_exact_u8_cpu; the field
 * keeps its place and size.  A half base must be 2-byte aligned (LSQ_EINVAL otherwise; the f32 rule asks for 4); ldb is in elements, >= d, and may be odd.
 * lsq_index_add takes appended base rows in the index's own format.
 *   IDENTITY W.  Widening a half to f32 is exact (subnormals are kept, never flushed; +-inf and NaN stay what they are), and every kernel widens in registers
 *   right before the arithmetic, as the 8-bit rows do ((3e), (3f)).  So an index whose base rows are the halves H returns, for EVERY call that reads base rows --
 *   lsq_index_rerank, lsq_index_search / _search_ivf with a shortlist, lsq_index_knn on its unfiltered, dense-filter and compact-filter roads -- and after
 *   lsq_index_add / _remove / _compact / _reserve, what the same index over the f32 matrix widen(H) returns: distances and ids bit for bit, NaN where that
 *   call has NaN, every statistic that does not count bytes or name the format.  Queries stay f32 (or uint8 for lsq_index_knn); the integer road of (3f)
 *   does not apply.
 *   IDENTITY N.  Narrowing is round-to-nearest-even.  binary16: overflow (from 65520 on) to +-inf, subnormals kept, NaN to a NaN -- the bits of numpy's
 *   astype(float16).  bfloat16: for a non-NaN x with bits u, (u + 0x7fff + ((u >> 16) & 1)) >> 16 (the carry may reach the exponent, and f32 max becomes inf);
 *   NaN to a NaN, payload not pinned.  Device and host give the same bits for every non-NaN input.
 *   lsq_narrow_rows_cpu     beside lsq_rerank_cpu: the host narrowing, no context, std::thread workers (nthreads 0 = all).  dst row i (ldd halves apart, 2-byte
 *                           aligned) = narrow(src row i, lds floats apart), d components each; nothing else of dst is written.  The checker of the device
 *                           narrowing and the road the host binding uses.  LSQ_EINVAL, nothing written: a format other than the two, n < 0, d < 1, lds < d,
 *                           ldd < d, a null or misaligned pointer.
 *   lsq_index_narrow_base   beside lsq_index_compact: the index's resident F32 base rows are converted ON THE DEVICE into rows of `format` that the index owns,
 *                           dense (ldb becomes d).  Afterwards the index is, for every call, the index created over narrow(base).  A borrowed f32 base is left
 *                           untouched and dropped from the index (the caller may free it); an owned one is freed after the convert.  THE TRANSIENT PEAK IS OLD
 *                           PLUS NEW: 6 d bytes per row until the call returns.  The capacity of an owned base (lsq_index_reserve) is kept.  Like
 *                           lsq_index_add and lsq_index_compact it drops a held range result (3m).  It waits for the device.  LSQ_EINVAL, NOTHING CHANGED: an
 *                           index without base rows, a base that is not f32 (a second call included), a format other than the two.
 *   lsq_index_get_base      beside lsq_index_reconstruct, which returns what the CODES stand for: this returns the STORED base rows [start, start + count),
 *                           widened to f32 whatever the format (an f32 base: a copy; a uint8 base: widened).  out [count][ldo] host (on_device = 0: widened
 *                           into staging in chunks of rows and fetched, 64 MiB at a time; option "recon_chunk" as for lsq_index_reconstruct) or device (1).
 *                           NOT AFFECTED BY A ROW FILTER.  It changes nothing.  LSQ_EINVAL BEFORE ANYTHING IS WRITTEN: a range that leaves [0, n], ldo < d, an
 *                           index without base rows, a null (count > 0) or misaligned out.  count == 0: LSQ_OK.
 *   lsq_index_get_base_info beside lsq_index_get_packed_info: what the base rows are now, and what the last lsq_index_narrow_base did. */
#define LSQ_BASE_F16 2
#define LSQ_BASE_BF16 3
typedef struct lsq_index_base_info {     /* fields are only ever appended */
    int64_t format;              /* 0 f32, 1 uint8, LSQ_BASE_F16, LSQ_BASE_BF16; all zero on an index without base rows */
    int64_t elem_bytes;          /* 4, 1, 2 */
    int64_t ldb;                 /* elements between rows */
    int64_t owned;               /* 1: the index owns the rows; 0: it borrows the caller's */
    int64_t resident_bytes;      /* ((n - 1) ldb + d) elem_bytes: the rows up to the d-th element of the last one */
    int64_t to_inf;              /* the last lsq_index_narrow_base: finite values that became +-inf */
    int64_t to_zero;             /*   non-zero values that became +-0 */
    int64_t nans;                /*   NaNs */
    double narrow_ms;            /*   its kernel, with option "profile" = 1 */
} lsq_index_base_info;
LSQ_API int lsq_narrow_rows_cpu(void *dst, const float *src, int64_t n, int d, int64_t lds, int64_t ldd, int format, int nthreads);
LSQ_API int lsq_index_narrow_base(lsq_index *ix, int format);
LSQ_API int lsq_index_get_base(lsq_index *ix, float *out, int64_t start, int64_t count, int64_t ldo, int on_device);
LSQ_API int lsq_index_get_base_info(lsq_index *ix, lsq_index_base_info *out);

/* ---- (3p) snapshots: an index saved to a file, loaded from it, exported as arrays, digested (csrc/lsq_snapshot.hip, csrc/lsq_snapshot_check.h; since v2600) ----
 * THE REFERENCE HAS NO COUNTERPART for any of the nine symbols below: it keeps no resident index, and its demos write codes with HDF5 by hand.
 * THE LOGICAL STATE of an index is the set of arrays a caller would pass to build it fresh -- never capacity, scratch, statistics, a held range result or
 * ownership.  Its canonical form, section by section, in this order (kind = LSQ_SNAP_*):
 *   CODEBOOKS    f32 [m 256][d]                       with codes          CODES      u8 [n][m]                         with codes
 *   DBNORMS      f32 [n]                              plain index         NORM_CODES u8 [n]   and  CBNORMS f32 [ncb]   packed index
 *   BASE         [n][d] in the stored format, dense   with base rows      CENTROIDS  f32 [nlist][d]  and  LIST_OF_ROW i32 [n]   with lists
 *   FILTER_BITS  u32 [ceil(n/32)], bits at or past n zero                 with an active filter
 * and the scalars n, d, m, h, packed, ncb, base format, nlist, filter active, the filter's FORCE flag (a forced road survives lsq_index_remove: it is
 * state) and the allowed count.  Bytes are kept verbatim: NaN payloads survive.
 * THE FILE (format version 1, everything little-endian) is a function of the logical state alone -- no time, host name or pointer:
 *   header, 128 bytes:  0 magic "LSQSNAP\0" | 8 u32 version = 1 | 12 u32 endianness marker 0x01020304 | 16 u32 header bytes = 128 | 20 u32 sections |
 *                       24 i64 n | 32 i32 d | 36 i32 m | 40 i32 h | 44 i32 packed | 48 i32 ncb | 52 i32 base format | 56 i32 nlist |
 *                       60 i32 flags (1 codes, 2 base rows, 4 filter active) | 64 i32 FORCE flag (0, LSQ_FILTER_FORCE_DENSE, _COMPACT) | 68 i32 zero |
 *                       72 i64 allowed | 80 i64 file bytes | 88 .. 127 zero
 *   table:              per section { u32 kind, u32 element bytes, u64 offset, u64 bytes, u64 digest }, then the u64 digest of every byte before it
 *   sections:           in the order above, the first at the next multiple of 64 after the table, each at the next multiple of 64 after the one before;
 *                       the padding is zero and is checked; the file ends with the last section's last byte.
 * THE DIGEST of a byte range that starts at word `first_word` of its section (a word = 4 bytes, little-endian, the last one zero-padded):
 *     SUM over the range's words w_i, i = first_word, first_word + 1, ...  of  (uint64) fmix32(w_i ^ (uint32)(i * 0x9E3779B1)) * (uint64)(uint32)(2 i + 1)
 *     + bytes * 0x9E3779B97F4A7C15                                                     all mod 2^64
 *     fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16        (murmur3's finaliser, a bijection)
 * A section's digest is that of all its bytes from word 0.  The digests of ranges that partition a section at multiples of 4 bytes ADD UP to it: blocks,
 * waves and staging chunks combine by addition, with no atomics and no ordering.  lsq_snapshot_digest_cpu, the kernel snap_digest_kernel and the numpy
 * statement in tests/snapshot_check.py agree on it bit for bit.
 *   IDENTITY S.  lsq_index_load(lsq_index_save(ix)) answers every call bit for bit like ix -- searches on every road, re-rank, k-NN, range search, decode,
 *   base rows, filter info except `road`, and every later lsq_index_add / _remove / _compact / _set_lists -- and like an index built from lsq_index_export.
 *   IDENTITY F.  The bytes lsq_index_save writes are those lsq_snapshot_write_cpu writes over lsq_index_export's arrays: two indexes that Identities G / R /
 *   C declare equal save byte-identical files, and lsq_index_digest equals the file's table.
 *   lsq_index_save          the file at `path` (flags: 0).  Sections move through two pinned staging chunks (option "snapshot_chunk": their bytes, rounded
 *                           down to a multiple of 64; 0 = the default 8 MiB): the copy of chunk k + 1 runs under the write of chunk k, the host never holds
 *                           more.  What is canonical in HBM is read where it lies; packed rows, a pitched base, list_of_row are derived on the device first.
 *                           Digests come from the device.  A borrowing index is saved from the caller's arrays; nothing is adopted, nothing changes.  The
 *                           bytes go to a temporary file beside `path` that is renamed on success: a failed save leaves a file at `path` as it was.
 *   lsq_index_load          header and table are validated on the host before anything is allocated; the sections stream into device arrays the new index
 *                           OWNS; it is built by lsq_index_create / _create_packed / _set_lists / _set_filter on those arrays (their device-side range checks
 *                           apply: LSQ_EINVAL), and what arrived in HBM is digested there and compared with the table (LSQ_EFORMAT).  On any error *out is
 *                           NULL and nothing is leaked.
 *   lsq_index_export        fills the arrays of `out` whose pointers are not NULL (host memory, or device memory with on_device = 1) and every scalar.  An
 *                           array the index does not have, requested anyway: LSQ_EINVAL before anything is written.
 *   lsq_index_digest        scalars, section table (with the offsets a file would have) and digests of the logical state; no file involved.
 *   lsq_index_get_snapshot_info   the last save of / the load that made this index.
 *   lsq_snapshot_write_cpu / _read_cpu / _inspect_cpu / _digest_cpu   host only, no context: the engine-less road.  write: has codes <=> codes != NULL, has
 *                           base rows <=> base != NULL, lists <=> nlist > 0, filter <=> filter_active (bits past n are written as zero, `allowed` is
 *                           recounted).  read: fills the non-NULL arrays (sized from inspect) after verifying every digest.  inspect: header and table, and
 *                           with verify != 0 every digest and the padding.
 * LSQ_EIO: open, read, write or rename failed, or a write was short.  LSQ_EFORMAT: not a snapshot, truncated, inconsistent, a digest mismatch, or a newer
 * format version.  lsq_last_error names the section and what was wrong. */
enum { LSQ_EIO = -6, LSQ_EFORMAT = -7 };
enum { LSQ_SNAP_CODEBOOKS = 1, LSQ_SNAP_CODES = 2, LSQ_SNAP_DBNORMS = 3, LSQ_SNAP_NORM_CODES = 4, LSQ_SNAP_CBNORMS = 5, LSQ_SNAP_BASE = 6,
       LSQ_SNAP_CENTROIDS = 7, LSQ_SNAP_LIST_OF_ROW = 8, LSQ_SNAP_FILTER_BITS = 9, LSQ_SNAP_MAX_SECTIONS = 9 };
#define LSQ_SNAPSHOT_FORMAT 1
typedef struct lsq_snapshot_arrays {     /* the logical state as plain arrays; a NULL pointer: not wanted / not there */
    int64_t n;
    int d, m, h, packed, ncb, base_format, nlist, filter_active, filter_force, reserved;
    int64_t allowed;
    void *codebooks, *codes, *dbnorms, *norm_codes, *cbnorms, *base, *centroids, *list_of_row, *filter_bits;
} lsq_snapshot_arrays;
typedef struct lsq_snapshot_section {
    int64_t kind, elem_bytes, offset, bytes;
    uint64_t digest;
} lsq_snapshot_section;
typedef struct lsq_snapshot_info {
    int64_t format, n, d, m, h, packed, ncb, base_format, nlist, has_codes, has_base, filter_active, filter_force, allowed;
    int64_t file_bytes, nsections;
    uint64_t header_digest;
    lsq_snapshot_section sections[9];    /* LSQ_SNAP_MAX_SECTIONS of them; the first nsections are filled */
} lsq_snapshot_info;
typedef struct lsq_snapshot_io_info {    /* fields are only ever appended */
    int64_t op;                  /* 0 none, 1 the last lsq_index_save, 2 the lsq_index_load that made the index */
    int64_t bytes, chunks, chunk_bytes, sections;
    int64_t host_staging_bytes;  /* pinned host memory the call held: two chunks */
    double derive_ms, digest_ms, copy_ms;        /* with option "profile" = 1: device time deriving sections, digesting, copying between HBM and the chunks */
    double file_ms, total_ms;    /* host clock: fwrite / fread; the whole call */
} lsq_snapshot_io_info;
LSQ_API int lsq_index_save(lsq_index *ix, const char *path, int flags);
LSQ_API int lsq_index_load(lsq_index **out, lsq_ctx *ctx, const char *path, int flags);
LSQ_API int lsq_index_export(lsq_index *ix, lsq_snapshot_arrays *out, int on_device);
LSQ_API int lsq_index_digest(lsq_index *ix, lsq_snapshot_info *out);
LSQ_API int lsq_index_get_snapshot_info(lsq_index *ix, lsq_snapshot_io_info *out);
LSQ_API int lsq_snapshot_write_cpu(const char *path, const lsq_snapshot_arrays *arrays);
LSQ_API int lsq_snapshot_read_cpu(const char *path, lsq_snapshot_arrays *out);
LSQ_API int lsq_snapshot_inspect_cpu(const char *path, lsq_snapshot_info *out, int verify);
LSQ_API int lsq_snapshot_digest_cpu(const void *data, int64_t bytes, int64_t first_word, uint64_t *out);

/* quantize_norms(B, C, cbnorms) -> dbnormsB     src/utils.jl:6-31: per database vector the squared norm of its reconstruction
 * (f32; codebooks, then dimensions, ascending) and the 1-based index of the nearest of the `ncb` (<= 256) scalar centroids, first minimum of
 * (norm - cbnorms[j])^2 like findmin.  `dbnorms` (optional) receives cbnorms[index] -- what the scan consumes (demos/demo_lsq_gpu.jl:57-60);
 * `norms` (optional) the unquantised norms (the input of the reference's norm k-means, src/lsq/LSQ.jl:80-84).  PARITY UNPINNED: the reference's
 * norm loop is `@simd`; this is the sequential order.  The _dev variant takes device pointers and uint8 0-BASED codes [n][m], index output 0-based. */
LSQ_API int lsq_quantize_norms(lsq_ctx *ctx, const int16_t *B, const float *K, const float *cbnorms, int ncb, int d, int64_t n, int m, int h,
                               int16_t *idx_out, float *dbnorms, float *norms);
LSQ_API int lsq_quantize_norms_dev(lsq_ctx *ctx, const uint8_t *d_codes, const float *d_K, const float *d_cbnorms, int ncb, int d, int64_t n,
                                   int m, int h, uint8_t *d_idx_out, float *d_dbnorms, float *d_norms);

/* update_codebooks(X, B, h) -> C      src/codebook_update.jl:52-86 (host code; north_star keeps it on the host).
 * K[t, :] = lsqr(sparsify_codes(B, h), X[t, :]) for every dimension t (LSQR of Paige & Saunders, Float32,
 * x0 = 0, atol = btol = sqrt(eps(Float32)), conlim = 1e8 -- IterativeSolvers' defaults; PARITY UNPINNED, the
 * reference neither vendors nor pins IterativeSolvers).  X d x n, B m x n Int16 1-based; K_out d x (m*h)
 * = hcat(C...) caller-allocated.  nthreads 0 = all cores (dimensions are independent). */
LSQ_API int lsq_update_codebooks(const float *X, const int16_t *B, int d, int64_t n, int m, int h, int nthreads, float *K_out);
/* The reference's other solver, codebook_upd_method = "lsmr" (src/codebook_update.jl:18-21 -> IterativeSolvers.lsmr): LSMR of Fong & Saunders with the same
 * operator, tolerances and threading as lsq_update_codebooks (host code; since v500). */
LSQ_API int lsq_update_codebooks_lsmr(const float *X, const int16_t *B, int d, int64_t n, int m, int h, int nthreads, float *K_out);

/* The same update ON THE DEVICE (csrc/lsq_lsqr.hip): all d systems advanced together, the same LSQR restatement (Float32 recurrences, the long sums
 * in double, IterativeSolvers' default stopping rules), the rows sorted by code once per call so that S'u is added in the host's order without atomics.
 * The same bits on every call; the same bits as lsq_update_codebooks on every tested problem (its norms are added in another order: agreement is
 * required to 1e-5 only).  _gpu: host buffers, Julia layout as above (X d x n, B m x n Int16 1-based, K_out d x (m*h));  _dev: device buffers,
 * codes [n][m] uint8 0-BASED.  h must be 256.  iterations (optional): LSQR iterations LAUNCHED = the slowest dimension's count rounded up to the host's
 * next look at the convergence counter (every 4 iterations for the first 8, every 2 after: up to 3 more than needed; a converged system is frozen, so the
 * extra launches change nothing but this number); `maxiter` bounds launched iterations likewise. */
LSQ_API int lsq_update_codebooks_gpu(lsq_ctx *ctx, const float *X, const int16_t *B, int d, int64_t n, int m, int h, float *K_out, int *iterations);
LSQ_API int lsq_update_codebooks_dev(lsq_ctx *ctx, const float *d_X, const uint8_t *d_codes, int d, int64_t n, int m, int h, float *d_K_out,
                                     int *iterations);

/* ---- the structured codebook update (since v1000) -------------------------------------------------------------------------------------------
 * update_codebooks_generic(X, B, h, odimsfunc) -> C and update_codebooks_chain(X, B, h) -> C      src/codebook_update.jl:104-158
 * dim2C is the reference's map of dimensions to codebooks (:134-136): a d x m Bool matrix in Julia's (column-major) order, one byte per entry, 1 where
 * codebook j covers dimension t, every entry 0 or 1 (anything else: LSQ_EINVAL).  For every dimension t, over cbs(t) = the codebooks that cover it, ascending:
 *     K[t, columns of cbs(t)] = lsqr(S[:, columns of cbs(t)], X[t, :])        K[t, every other column] = 0 (exactly)
 * with the restatement, tolerances and accumulation rules of lsq_update_codebooks and maxiter = max(n, |cbs(t)| h), the size of the sub-matrix.  A
 * dimension that no codebook covers gets a zero row.  dim2C = NULL: every codebook covers every dimension -- the call IS the unstructured one below it
 * (same path, same bits).  The chain's map is get_cbdims_chain(d, m) (:88-102; m >= 2, d >= m - 1).  Layouts, limits and `iterations` as for the
 * unstructured functions: host code, any h;  _gpu: host buffers on the device solver, h = 256, n m < 2^31;  _dev: device buffers (d_dim2C too: its d m
 * bytes are read back once per call), uint8 0-BASED codes [n][m], on the context's stream.  K_out may hold anything on entry.  The host solver groups
 * the dimensions by equal cover set and returns the bits of lsq_update_codebooks called on each group's sub-problem; the device solver has returned the
 * host solver's bits on every tested problem (required: 1e-5 on the reconstruction). */
LSQ_API int lsq_update_codebooks_struct(const float *X, const int16_t *B, const uint8_t *dim2C, int d, int64_t n, int m, int h, int nthreads, float *K_out);
LSQ_API int lsq_update_codebooks_struct_gpu(lsq_ctx *ctx, const float *X, const int16_t *B, const uint8_t *dim2C, int d, int64_t n, int m, int h,
                                            float *K_out, int *iterations);
LSQ_API int lsq_update_codebooks_struct_dev(lsq_ctx *ctx, const float *d_X, const uint8_t *d_codes, const uint8_t *d_dim2C, int d, int64_t n, int m,
                                            int h, float *d_K_out, int *iterations);

/* ---- sparse codebooks: the SPGL1 (LASSO) codebook update ON THE DEVICE (csrc/lsq_spgl1.hip; since v800) -------------------------------------
 * update_codebooks_spgl1(X, B, h, tau, prevC) and update_codebooks_spgl1_threshold(..., S)      src/codebook_update_sparse.jl (the reference calls
 * MATLAB's SPGL1 on the operator of matlab/sparse_lsq_fun.m): one joint problem over all d dimensions,
 *     minimise 1/2 ||A k - b||^2  subject to  ||k||_1 <= tau,      A = I_d (x) sparsify_codes(B, h),  b = vec(X'),
 * solved in float64 by SPGL1's single-tau spectral projected gradient (van den Berg & Friedlander 2008; spgSetParms defaults: optTol 1e-4,
 * 3 previous objectives, steps in [1e-16, 1e5], at most 10 n d iterations), warm-started from the projection of K_init (NULL: from 0).
 * "Solved" means rGap = |r'(r - b) + tau ||A'r||_inf| / max(1, ||r||^2 / 2) <= opt_tol, or ||r|| < opt_tol ||b||.
 * K_out (d x (m*h) = [m*h][d], f32) receives the best accepted iterate; then, for 0 <= S < d m h, only its S entries largest in |K| are kept
 * (ties: the lower flat index first -- Julia's sortperm(abs(K[:]), rev=true)) and the others become +0.0.  tau = 0 gives K = 0; S >= d m h keeps all.
 * The same bits on every call.  Host form: X d x n, B m x n Int16 1-based; _dev: device pointers, codes [n][m] uint8 0-based.  h must be 256.
 * LSQ_OK is returned whatever info->status says (the trainer goes on with the best iterate); bad tau (< 0 or NaN), S or shapes: LSQ_EINVAL. */
typedef struct lsq_spgl1_params {
    double opt_tol;          /* <= 0: 1e-4 */
    int64_t max_iter;        /* <= 0: 10 n d */
} lsq_spgl1_params;          /* NULL -> SPGL1's defaults */
enum { LSQ_SPGL1_OPTIMAL = 0, LSQ_SPGL1_ITERATIONS = 1, LSQ_SPGL1_LINE_ERROR = 2 };
typedef struct lsq_spgl1_info {
    int status;                          /* LSQ_SPGL1_*: the gap test passed / the iteration cap / the line search failed 10 times */
    int64_t iterations, line_search_trials;
    double f, rel_gap, l1, tau;          /* of the returned iterate before thresholding: 1/2 ||r||^2, rGap, ||K_out||_1 (of the f32 values) */
    int64_t nnz_before_threshold, nnz;
} lsq_spgl1_info;
LSQ_API int lsq_update_codebooks_spgl1(lsq_ctx *ctx, const float *X, const int16_t *B, int d, int64_t n, int m, int h, double tau,
                                       const float *K_init, int64_t S, const lsq_spgl1_params *params, float *K_out, lsq_spgl1_info *info);
LSQ_API int lsq_update_codebooks_spgl1_dev(lsq_ctx *ctx, const float *d_X, const uint8_t *d_codes, int d, int64_t n, int m, int h, double tau,
                                           const float *d_K_init, int64_t S, const lsq_spgl1_params *params, float *d_K_out, lsq_spgl1_info *info);

/* ---- the initialisers' two data-parallel steps ON THE DEVICE (csrc/lsq_init.hip; since v600) -----------------------------------
 * encoding_viterbi(X, C) -> B      src/encodings/encode_chain.jl:92-123 (worker encode_viterbi! :2-89): the exact MAP codes of a CHAIN -- unaries
 * (get_unaries, utils.jl:94-122) plus the binaries 2 C_i' C_{i+1} of consecutive codebooks only (:103-106) -- by dynamic programming: m - 1 min-plus
 * steps over a 256 x 256 table per vector, first minimum on ties (the reference's strict-'<' scans, :58-66,74), then the trace (:77-83).  K = hcat(C...)
 * as everywhere (chain codebooks are zero outside the dimensions they cover: codebook_update.jl:88-102); 2 <= m <= 16, h must be 256.
 * Host form: X d x n, B m x n Int16 1-BASED (the reference's return value).  _dev: device pointers, codes [n][m] uint8 0-BASED. */
LSQ_API int lsq_encode_viterbi(lsq_ctx *ctx, const float *X, const float *K, int d, int64_t n, int m, int h, int16_t *B);
LSQ_API int lsq_encode_viterbi_dev(lsq_ctx *ctx, const float *d_X, const float *d_K, int d, int64_t n, int m, int h, uint8_t *d_B);
/* quantize_pq(X, C) / the assignment step of the k-means behind train_pq and train_opq      src/pq/PQ.jl:12-41, src/opq/kmeans.jl:6-75 (update_assignments!),
 * src/opq/OPQ.jl:60-66,88-91: per codebook j INDEPENDENTLY the first argmin_a of ||c_ja||^2 - 2 <x, c_ja> (= the sub-space distance minus ||x_sub||^2 when
 * codebook j is zero outside its sub-space -- PQ / OPQ codebooks padded to d rows -- and the plain nearest codeword of full-dimensional codebooks otherwise).
 * minval (optional, [n][m] floats, vector-major): the minimum itself; add ||x_sub||^2 for the squared distance the reference's `costs` hold.
 * PARITY UNPINNED as every initialiser: the reference takes pairwise(SqEuclidean()) from Distances.jl and argmin from its own scan; near-ties may differ.
 * Host form: B m x n Int16 1-based; _dev: codes [n][m] uint8 0-based.  h must be 256. */
LSQ_API int lsq_assign_codewords(lsq_ctx *ctx, const float *X, const float *K, int d, int64_t n, int m, int h, int16_t *B, float *minval);
LSQ_API int lsq_assign_codewords_dev(lsq_ctx *ctx, const float *d_X, const float *d_K, int d, int64_t n, int m, int h, uint8_t *d_B, float *d_minval);

/* ---- the beam-search encoder on resident codebooks (csrc/lsq_beam.hip; since v1600) -----------------------------------------------------------
 * THE REFERENCE HAS NO COUNTERPART.  It stands beside the random start of every encode there -- randinit, src/encodings/encode_icm.jl:55-70 and
 * demos/demo_lsq_gpu.jl:46, which its codes can replace as the B0 of lsq_encode_icm(_dev) -- and beside the chain's exact DP, src/encodings/
 * encode_chain.jl:2-89 (lsq_encode_viterbi), which it generalises from the m - 1 adjacent pair tables to all of them: the classical encoder of additive
 * quantisation and of residual quantisers, beam search over the full pair tables.  Deterministic, no RNG.  Per vector i, with U = what lsq_get_unaries
 * returns, T = what lsq_get_binaries returns, the visiting order o_0 .. o_{m-1} (a permutation of 0 .. m-1; NULL = ascending) and beam width L:
 *   stage 0       candidates v(0, a) = U[o_0][i][a];
 *   stage t >= 1  for every live beam p in rank order, score S_p and codes b^p:  s = U[o_t][i][.];  then for r = 0 .. t-1 in stage order
 *                 s[a] = s[a] + T[o_t][o_r][b^p_{o_r}][a]  (plain f32 adds, never fused);  then v(p, a) = S_p + s[a], one rounded add;
 *   selection     the min(L, L_t * 256) smallest triples (v, p, a) in lexicographic order become the next beams, ranked in that order (ties: the smaller
 *                 parent rank, then the smaller code); a child's score is v, its codes are the parent's plus b_{o_t} = a;
 *   output        the codes of the rank-0 beam after stage m - 1 and, optionally, its score S_0 (f32): ||x||^2 + S_0 is the vector's veccost up to rounding.
 * Inputs are finite; nothing is promised about NaN except that every code written lies in 0 .. 255.  tests/beam_check.py restates this in numpy; the
 * kernel returns its codes and score bits.
 * The handle: lsq_encoder_create COPIES the codebooks ([m*h][d]; host memory, or device memory with on_device = 1) and builds ||c||^2 and the m x m pair
 * tables ONCE; it owns all its scratch (tables, one chunk's unaries, staging), so calls on it and calls on the context do not disturb each other -- the
 * context's table cache and chunk state are untouched -- and neither do two encoders of one context.  It runs on the context's device and on the stream the
 * context is bound to at each call; the context must outlive it; like the context it serves one host thread at a time.  chunk: vectors per pass (0 = the
 * default 65 536: 512 MB of unaries at m = 8).
 * lsq_encoder_beam: X [n][d] float32 (x_u8 = 0) or uint8 (x_u8 = 1: the un-widened rows of a .bvecs set; the bits of the f32 call on the widened rows).
 *   on_device = 0: X, codes, score are HOST buffers, codes int16 1-BASED [n][m] (the boundary's type, as in lsq_encode_viterbi);
 *   on_device = 1: device buffers, codes uint8 0-based [n][m] -- exactly the dB0 of lsq_encode_icm_dev.
 *   order: m int32 in HOST memory in both forms (or NULL), checked before any launch.  score: [n] float32 or NULL.
 * LSQ_EINVAL with nothing launched: a null handle, description or pointer (X / codes with n > 0), h != 256, m outside 1 .. 16, d < 1, chunk < 0, beam
 * outside 1 .. 32, n < 0, an order that is not a permutation.  n = 0 is LSQ_OK. */
typedef struct lsq_encoder lsq_encoder;
typedef struct lsq_encoder_desc {
    int d, m, h;
    const float *codebooks;      /* [m*h][d] */
    int on_device;
    int64_t chunk;               /* vectors per pass, 0 = default */
} lsq_encoder_desc;
typedef struct lsq_encoder_info {        /* the last lsq_encoder_beam call */
    int64_t vectors, chunks;
    int64_t beam;
    double unaries_ms, beam_ms;  /* with the context's option "profile" = 1: the unary GEMMs; the beam kernel */
} lsq_encoder_info;
LSQ_API int lsq_encoder_create(lsq_encoder **out, lsq_ctx *ctx, const lsq_encoder_desc *desc);
LSQ_API int lsq_encoder_destroy(lsq_encoder *en);
LSQ_API int lsq_encoder_beam(lsq_encoder *en, const void *X, int x_u8, int64_t n, int beam, const int32_t *order, void *codes, float *score, int on_device);
LSQ_API int lsq_encoder_get_info(lsq_encoder *en, lsq_encoder_info *out);

/* ---- PQ / OPQ training resident on the device: cluster means and k-means++ seeding (csrc/lsq_kmeans.hip; since v1100) -------------------------
 * Both steps run for all m sub-spaces of a vector set in one call.  The sub-space structure is the cover map dim2C of the structured update above (d x m
 * in Julia's order, one byte per entry, 0 or 1), here HOST memory in BOTH forms: it is checked before anything is launched, every codebook must cover
 * at least one dimension (else LSQ_EINVAL), and a _dev call enqueues its work on the context's stream without waiting for the device.  PQ / OPQ: codebook j
 * covers splitarray(1:d, m)[j]; plain k-means is m = 1 with every dimension covered.  K is d x (m*h) = hcat of the codebooks padded to d rows -- what
 * lsq_assign_codewords takes -- and exactly +0.0 outside the cover.  h must be 256, m <= 16.  Host forms: X d x n, B m x n Int16 1-based; _dev: device
 * pointers, codes [n][m] uint8 0-BASED.  No atomics anywhere: the same bits on every call.
 *
 * update_centers!(X, assignments, centers, counts)      src/opq/kmeans.jl:77-123
 * For codebook j, code c and covered dimension t: the values X[t, i] of the vectors i holding code c, added in ascending i with plain Float32 adds from
 * +0.0, divided by their count in double and rounded to Float32 (numpy's np.add.at followed by `f32 /= int64`: the bits of this package's host trainers).
 * counts (optional, m*h Int32) receives the cluster sizes.  An empty cluster takes its column of K_prev (OPQ keeps the old codeword) or, with K_prev = NULL,
 * zero, as the reference leaves it (:86,112); its count is 0 either way.  K_prev may be K_out.  n = 0: every cluster is empty.  n m < 2^31. */
LSQ_API int lsq_update_centers(lsq_ctx *ctx, const float *X, const int16_t *B, const uint8_t *dim2C, const float *K_prev, int d, int64_t n, int m, int h,
                               float *K_out, int *counts);
LSQ_API int lsq_update_centers_dev(lsq_ctx *ctx, const float *d_X, const uint8_t *d_codes, const uint8_t *dim2C, const float *d_K_prev, int d, int64_t n,
                                   int m, int h, float *d_K_out, int *d_counts);
/* k-means++ seeding: Clustering.kmeans(X, h, init=:kmpp)      src/pq/PQ.jl:60 (Clustering.jl is neither vendored nor pinned: PARITY UNPINNED)
 * D^2 sampling with the caller's random numbers: u is HOST memory, m x h doubles in [0, 1) (row j for sub-space j; anything else: LSQ_EINVAL); the library
 * holds no generator and the result is a function of (X, u).  Per sub-space j:
 *     step 0       row min(n - 1, floor(u[j][0] n));
 *     step k >= 1  d2[i] = min(d2[i], SUM_t (x_it - c_t)^2) -- Float32, direct form over the covered dimensions ascending, no FMA -- with c the row chosen
 *                  at step k - 1; tot = SUM_i d2[i] in double; tot > 0: the first row whose double prefix sum exceeds u[j][k] tot (a row at distance 0 is
 *                  never chosen); tot = 0 (fewer distinct rows than steps): row min(n - 1, floor(u[j][k] n)).
 * The double sums run in a fixed order that depends on n alone (block partial sums of fixed row sets combined in a fixed order: csrc/lsq_kmeans.hip), so
 * two calls choose the same rows; another summation order can choose a neighbouring row where u tot falls within rounding (2 n 2^-53 tot) of a boundary.
 * K_out: the chosen rows restricted to the cover.  idx_out (optional, m x h Int64, row-major [m][h]): their 0-based indices.  d2_out (optional, [n][m]
 * Float32, vector-major): the squared distance of every vector to the nearest of ALL h chosen rows.  n = 0: K_out = 0, indices -1, d2 untouched. */
LSQ_API int lsq_kmeanspp_seed(lsq_ctx *ctx, const float *X, const uint8_t *dim2C, const double *u, int d, int64_t n, int m, int h, float *K_out,
                              int64_t *idx_out, float *d2_out);
LSQ_API int lsq_kmeanspp_seed_dev(lsq_ctx *ctx, const float *d_X, const uint8_t *dim2C, const double *u, int d, int64_t n, int m, int h, float *d_K_out,
                                  int64_t *d_idx_out, float *d_d2_out);

/* ---- (4) device-side generators used by the benchmark harness -----------------------------
 * X[i][t] = float(uniform integer 0..255) (SIFT-like);  codes uniform 0..h-1 (randinit);
 * codebooks: K[j][a][:] = scale * x_{pick(j,a)} for a Philox-picked synthetic vector. */
LSQ_API int lsq_synth_data_u8_dev(lsq_ctx *ctx, uint64_t seed, uint64_t global_offset, int64_t n, int d, float *dX);
LSQ_API int lsq_randinit_dev(lsq_ctx *ctx, uint64_t seed, uint64_t global_offset, int64_t n, int m, int h, uint8_t *dB);
LSQ_API int lsq_synth_codebooks_dev(lsq_ctx *ctx, uint64_t seed, int m, int h, int d, float *dK);

#ifdef __cplusplus
}
#endif
#endif /* LSQ_MI355X_H */
