// lsq_api.hip -- the C-ABI of liblsq_mi355x.so (see include/lsq_mi355x.h for the contract and the
// reference interfaces each entry point replaces).  Host orchestration only: every numeric step is
// a HIP kernel in lsq_gemm.hip / lsq_icm.hip.  There is NO CPU fallback: without a gfx950 device
// every compute entry point fails with LSQ_ENODEV / LSQ_EHIP.
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "lsq_internal.h"

// ---- errors -------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void lsq_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *lsq_last_error(void) { return g_err; }
extern "C" int lsq_version(void) { return LSQ_VERSION; }

extern "C" int lsq_device_count(int *count) {
    if (!count) { lsq_set_error("lsq_device_count: null pointer"); return LSQ_EINVAL; }
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; lsq_set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return LSQ_ENODEV; }
    *count = c;
    return LSQ_OK;
}

// ---- context ------------------------------------------------------------------------------------

enum { CAT_TABLES = 0, CAT_UNARIES, CAT_PERTURB, CAT_ICM, CAT_COST, CAT_OTHER, CAT_COUNT };

// layout of the context's block of small per-call words (bytes; [0, SMALL_READ_END) is what a call zeroes and reads back)
enum : size_t { SMALL_COUNTERS = 0, SMALL_OBJ = 8192, SMALL_BAD = 8704, SMALL_QP = 8832, SMALL_ACTIVE = 10240, SMALL_ROAD = 11008,
                SMALL_READ_END = 11072, SMALL_PROBE = 11264, SMALL_BYTES = 12288 };
static_assert(sizeof(lsq_q16_params) <= SMALL_ACTIVE - SMALL_QP && sizeof(unsigned long long) * LSQ_WALK_COUNTERS <= SMALL_ROAD - SMALL_ACTIVE &&
              sizeof(unsigned long long) * LSQ_WALK_COUNTERS <= SMALL_BYTES - SMALL_PROBE, "the per-call block's windows");

// The road of the resident chunk -- which kernel runs its node updates, and who decided -- and what lsq_get_q16_snapshot needs to know of it after the
// call.  Forgotten where a chunk's unaries start to be built (start_chunk), written by the verdict (q16_verdict) and the probe (encode_chunk), read by run_sweeps.
struct ChunkRoad {
    bool filtered = false;      // the chunk runs the 16-bit filtered walk
    bool on_device = false;     // option "async": the road lives in road[0] (2 = filtered, 0 = f32), BOTH walks are enqueued and the word picks
    bool resident = false;      // the chunk's levels are resident: the host verdict named the filtered walk (a later probe may still leave it) ...
    int64_t cn = 0, row0 = 0;   // ... its rows and its first row within the call
    int m = 0;
};

struct lsq_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int64_t chunk = 256 * 3968;      // vectors per resident chunk: one pass of the filtered walk per block (256 blocks x 3968 vectors: lsq_q16.h, WalkqRot::pp())
    int profile = 0;
    int schedule = 6;        // 3: LDS-walk (f32), one launch per node; 4: the same, one launch per ILS iteration; 6 (default): 16-bit filtered walk
                             // with exact refinement, one launch per ILS iteration (chunks below q16_min vectors / non-finite data: schedule 4);
    int64_t q16_min = 65536; // schedule 6: smaller chunks take schedule 4 (every block is light there: nothing to filter)
    int tables_changed = 1;  // schedule 6: the pair tables were rebuilt since the last lsq_launch_q16_prepare
    // Host-buffer entry points called again with the SAME codebooks (the trainer's chained encoding_icm, demos/demo_lsq.jl:48-51 / LSQ.jl:54-57 -- the
    // reference rebuilds its binaries in every call, encode_icm.jl:145, with identical results): the uploaded K, ||c||^2, the pair tables and what the
    // filtered walk derives from them are still in this context -- one memcmp of the caller's K against a host copy decides
    std::vector<float> hostK;
    int hostK_d = 0, hostK_m = 0;
    bool tables_valid = false;
    int64_t table_reuses = 0;
    int per_node = 0;        // schedule 6: one launch per node update instead of 64 per launch (profiling: per-sweep timings / counters)
    int ablation = 0;        // timing-only kernel ablations (results are garbage when != 0)
    int light = -1;          // schedules 3/4: light-block threshold (-1 = default)
    int wave_max = 64;       // chunks with at most this many vectors per block of the walk kernel (and all-light blocks) run icm_wave_kernel
    int fallback = 1;        // schedules 3/4: a candidate equal to its current record inherits that record's validity bits (exact)
    int skip = 1;            // schedule 3: skip node updates whose inputs did not change (exact memoisation)
    uint32_t auto_it = 0;    // ILS-iteration counter of the CPU-shaped entry points called with it = LSQ_IT_AUTO: advances by one per call
    // workspace
    DevBuf sci, T, Ts, U, vCur, vNew, active, recCur, recNew, prev, counters, obj, bad;
    DevBuf probe;                                      // walk counters of a chunk's FIRST ILS iteration on the filtered path (read back: is the filter paying off?)
    int64_t probe_div = 8;                             // option "filter_probe_div": after the first iteration the chunk goes to the f32 walk when
                                                       // (refined + f32-routed) * div > recomputed node updates (0 = never)
    DevBuf small;                                              // one block for the small per-call words below (counters, obj, bad, qp, active, road, probe are windows into it)
    char *small_host = nullptr;                                // its pinned mirror
    bool small_packed = false;                                 // this call: every window still in place (an outgrown one gets an allocation of its own)
    DevBuf Uq, Tq, qp, qscratch, qflag, qsigma;                // 16-bit filtered walk: u16 unary planes, u16 slice tables, lsq_q16_params, bound scratch, per-vector out-of-range flags
    lsq_q16_work qw;                                   // ... their pointers, mapped once per chunk (q16_map)
    ChunkRoad chunk_road;
    int64_t call_row0 = 0;                             // first row of the chunk being encoded within its call
    // option "async" (lsq_encode_icm_dev only): no host round trip inside the call and none at its end -- the chunk's road (verdict after the unary
    // GEMM, probe after the first ILS iteration) is decided by one-thread kernels into `road`, BOTH walks are enqueued every ILS iteration and the one
    // the word does not name returns at once; objective sums and counters are copied to the caller's (device or pinned) buffers on the stream
    int async_mode = 0;
    bool pending_fold = false;                         // async calls left walk statistics in `active` / road[1]: folded at the next synchronising entry point
    DevBuf road;
    int64_t fallback_div = 64;                         // option "filter_fallback_div": the chunk goes to the f32 walk when flagged pairs * div > all pairs (0 = never)
    int64_t filter_fallback_chunks = 0;                // chunks the filter handed to the f32 walk (unusable bounds or too many out-of-range vectors)
    lsq_lsqr_state *lsqr = nullptr;                    // device LSQR (lsq_lsqr.hip): work buffers, created on first use
    lsq_kmeans_state *kmeans = nullptr;                // cluster means and k-means++ seeding (lsq_kmeans.hip): work buffers, created on first use
    lsq_spgl1_state *spgl1 = nullptr;                  // device SPGL1 (lsq_spgl1.hip): work buffers, created on first use
    lsq_adc_state *adc = nullptr;                      // device ADC scan (lsq_adc.hip): buffers, created on first use
    lsq_linscan_stats adc_stats{};
    lsq_search_opts search;                            // options "linscan_exhaustive", "linscan_rank": test hooks of the scan's selection (search_opts fills in the rest per call)
    int knn_u8_int = 1;                                // option "knn_u8_int": 0 = lsq_index_knn widens 8-bit rows and queries even where the integer road applies; a test hook
    int64_t rerank_batch = 0;                          // option "rerank_batch": queries per re-rank batch of this context's indexes (0 = automatic); a test hook
    int64_t range_batch = 0;                           // option "range_batch": records per fill batch of lsq_index_range_search (0 = automatic); a test hook
    int64_t recon_chunk = 0;                           // option "recon_chunk": rows per staging chunk of a host-buffer lsq_index_reconstruct (0 = automatic); a test hook
    int64_t snapshot_chunk = 0;                        // option "snapshot_chunk": bytes per staging chunk of lsq_index_save / _load (0 = LSQ_SNAP_CHUNK_DEFAULT); a test hook
    // Staging for the host-buffer entry points.  Who writes what (a later call may assume NOTHING of their contents, except sK under tables_valid):
    //   sX, sX2  X: one chunk at a time, double-buffered, by the pipelined encode; the whole X by stage_X
    //   sK       the call's codebooks: uploaded (host_codebooks; claim_sK: K, K_prev) or computed into it (claim_sK: LSQR, SPGL1, the seeding).
    //            tables_valid says that sK, sci, T and what the filtered walk derives from them still belong to hostK
    //   sB16     int16 1-based codes on their way up (stage_codes, the pipelined encode) or down (fetch_codes, the pipelined encode's snapshots)
    //   sTight   tight [n][m] codes: stage_codes' for the solvers, the initialisers' result
    //   sOut16   quantize_norms' indices;  sF32: small arrays, the slices a call carves (carve_f32) and names in that line
    DevBuf sX, sX2, sK, sB16, sOut16, sTight, sF32;
    DevBuf sSample, sSigmaS;                           // host-buffer pipeline: the level sample (compacted rows of X) and its sigma
    std::vector<float> sample_host;                    // ... packed on the host before its upload
    std::vector<hipEvent_t> panel_ev;                  // ... one event per uploaded panel
    int64_t panel_bytes = 48ll << 20;                  // option "upload_panel_bytes": size of one uploaded panel (rounded down to whole 128-row tiles)
    int64_t pipeline_min_bytes = 64ll << 20;           // option "upload_pipeline_min_bytes": first chunks of at least this many bytes of X are uploaded panel by panel under their unary GEMM (0 = never)
    hipStream_t copy_stream = nullptr;               // H2D of X runs here, under the compute of the previous panel / chunk
    hipEvent_t copy_done = nullptr;
    // timings
    double cat_ms[CAT_COUNT] = {0, 0, 0, 0, 0, 0};
    int64_t icm_launches = 0, icm_node_updates = 0, staged_blocks = 0, light_blocks = 0, filtered_blocks = 0, filter_refined = 0, filter_exact = 0, filter_f32 = 0;
    int64_t trace[LSQ_WALK_TRACE] = {0};
    struct Pending { hipEvent_t a, b; int cat; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
};

static int fold_pending(lsq_ctx *c);
struct AsyncOff {        // option "async" applies to the device-resident encodes alone: the other entry points that reach its readers (q16_verdict, begin_call,
                         // finish_call) return results through host memory they must wait for
    lsq_ctx *c; int saved;
    explicit AsyncOff(lsq_ctx *ctx) : c(ctx), saved(ctx ? ctx->async_mode : 0) { if (c) c->async_mode = 0; }
    ~AsyncOff() { if (c) c->async_mode = saved; }
};

static int use_device(lsq_ctx *ctx) {
    if (!ctx) { lsq_set_error("null lsq_ctx"); return LSQ_EINVAL; }
    LSQ_HIP(hipSetDevice(ctx->device));
    return LSQ_OK;
}

int lsq_ctx_bind(lsq_ctx *c, hipStream_t *stream, int *profile) {
    LSQ_TRY(use_device(c));
    *stream = c->stream;
    *profile = c->profile;
    return LSQ_OK;
}

struct Timer {        // brackets a group of launches with an event pair when profiling is on
    lsq_ctx *c; int cat; hipEvent_t a = nullptr, b = nullptr; bool on;
    Timer(lsq_ctx *ctx, int category) : c(ctx), cat(category), on(ctx->profile != 0) {
        if (!on) return;
        a = grab(); b = grab();
        if (!a || !b) { on = false; return; }
        (void)hipEventRecord(a, c->stream);
    }
    hipEvent_t grab() {
        if (!c->pool.empty()) { hipEvent_t e = c->pool.back(); c->pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
    ~Timer() {
        if (!on) return;
        (void)hipEventRecord(b, c->stream);
        c->pending.push_back({a, b, cat});
    }
};

static int resolve_timings(lsq_ctx *ctx) {
    for (auto &p : ctx->pending) {
        LSQ_HIP(hipEventSynchronize(p.b));
        float ms = 0.f;
        LSQ_HIP(hipEventElapsedTime(&ms, p.a, p.b));
        ctx->cat_ms[p.cat] += (double)ms;
        ctx->pool.push_back(p.a);
        ctx->pool.push_back(p.b);
    }
    ctx->pending.clear();
    return LSQ_OK;
}

extern "C" int lsq_create(lsq_ctx **out, int device) {
    if (!out) { lsq_set_error("lsq_create: null out pointer"); return LSQ_EINVAL; }
    *out = nullptr;
    int count = 0;
    LSQ_TRY(lsq_device_count(&count));
    if (count <= 0) { lsq_set_error("no HIP device visible (this library has no CPU fallback)"); return LSQ_ENODEV; }
    if (device < 0 || device >= count) { lsq_set_error("device %d out of range (0..%d)", device, count - 1); return LSQ_EINVAL; }
    LSQ_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    LSQ_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        lsq_set_error("device %d is %s; this library carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
        return LSQ_ENODEV;
    }
    lsq_ctx *c = new lsq_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; lsq_set_error("hipStreamCreate: %s", hipGetErrorString(e)); return LSQ_EHIP; }
    c->stream = c->own_stream;
    // the small per-call words (counters, sums, flags, level parameters) share ONE block: a call zeroes it with one fill and reads it back with one copy into
    // pinned memory (they were seven fills and four pageable copies of a few bytes each, 5 - 20 us apiece: a quarter of a 10 000-vector call)
    if (hipMalloc(&c->small.p, SMALL_BYTES) != hipSuccess || hipHostMalloc(reinterpret_cast<void **>(&c->small_host), SMALL_BYTES, hipHostMallocDefault) != hipSuccess) {
        if (c->small.p) (void)hipFree(c->small.p);
        (void)hipStreamDestroy(c->own_stream);
        delete c;
        lsq_set_error("lsq_create: no memory for the per-call block");
        return LSQ_ENOMEM;
    }
    c->small.cap = SMALL_BYTES;
    // What the first call of a process would otherwise pay inside its timed region (the reference creates its context and loads its module per CALL,
    // encode_icm_cuda.jl:59-64): the code objects of the encode path's three translation units, the copy stream and its event, and the runtime's pinned
    // staging for pageable copies (one small round trip through this context's stream).
    {
        hipFuncAttributes fa;
        (void)hipFuncGetAttributes(&fa, lsq_probe_kernel_gemm());
        (void)hipFuncGetAttributes(&fa, lsq_probe_kernel_icm());
        (void)hipFuncGetAttributes(&fa, lsq_probe_kernel_icmq());
        (void)hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
        (void)hipEventCreateWithFlags(&c->copy_done, hipEventDisableTiming);
        char warm[256] = {0};
        (void)hipMemcpyAsync(c->small.p, warm, sizeof(warm), hipMemcpyHostToDevice, c->own_stream);
        (void)hipMemcpyAsync(warm, c->small.p, sizeof(warm), hipMemcpyDeviceToHost, c->own_stream);
        (void)hipStreamSynchronize(c->own_stream);
        (void)hipGetLastError();
    }
    c->counters.window(c->small.p, SMALL_COUNTERS, SMALL_OBJ - SMALL_COUNTERS);
    c->obj.window(c->small.p, SMALL_OBJ, SMALL_BAD - SMALL_OBJ);
    c->bad.window(c->small.p, SMALL_BAD, 64);
    c->qp.window(c->small.p, SMALL_QP, SMALL_ACTIVE - SMALL_QP);
    c->active.window(c->small.p, SMALL_ACTIVE, SMALL_ROAD - SMALL_ACTIVE);
    c->road.window(c->small.p, SMALL_ROAD, SMALL_READ_END - SMALL_ROAD);
    c->probe.window(c->small.p, SMALL_PROBE, SMALL_BYTES - SMALL_PROBE);
    *out = c;
    return LSQ_OK;
}

extern "C" int lsq_destroy(lsq_ctx *c) {
    if (!c) return LSQ_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto &p : c->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : c->pool) (void)hipEventDestroy(e);
    DevBuf *bufs[] = {&c->road, &c->probe, &c->Uq, &c->Tq, &c->qp, &c->qscratch, &c->qflag, &c->qsigma, &c->sci, &c->T, &c->Ts, &c->U, &c->vCur, &c->vNew, &c->active, &c->recCur, &c->recNew, &c->prev, &c->counters, &c->obj, &c->bad,
                      &c->sX, &c->sX2, &c->sK, &c->sB16, &c->sOut16, &c->sTight, &c->sF32, &c->sSample, &c->sSigmaS};
    for (DevBuf *b : bufs) b->release();
    c->small.release();
    if (c->small_host) (void)hipHostFree(c->small_host);
    for (auto e : c->panel_ev) (void)hipEventDestroy(e);
    lsq_adc_free(c->adc);
    lsq_lsqr_free(c->lsqr);
    lsq_spgl1_free(c->spgl1);
    lsq_kmeans_free(c->kmeans);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->copy_done) (void)hipEventDestroy(c->copy_done);
    delete c;
    return LSQ_OK;
}

extern "C" int lsq_set_stream(lsq_ctx *c, void *hip_stream) {
    LSQ_TRY(use_device(c));
    if (c->stream != reinterpret_cast<hipStream_t>(hip_stream)) c->tables_valid = false;      // cached tables were built on the old stream: nothing orders them before work on the new one
    c->stream = reinterpret_cast<hipStream_t>(hip_stream);      // NULL = HIP's default (null) stream, e.g. torch's default
    return LSQ_OK;
}

extern "C" int lsq_set_option(lsq_ctx *c, const char *key, int64_t value) {
    if (!c || !key) { lsq_set_error("lsq_set_option: null argument"); return LSQ_EINVAL; }
    if (!strcmp(key, "chunk")) {
        if (value < 1) { lsq_set_error("chunk must be >= 1"); return LSQ_EINVAL; }
        c->chunk = value;
    } else if (!strcmp(key, "profile")) c->profile = value != 0;
    else if (!strcmp(key, "own_stream")) { if (c->stream != c->own_stream) c->tables_valid = false; c->stream = c->own_stream; }
    else if (!strcmp(key, "skip")) c->skip = value != 0;
#ifdef LSQ_TUNING
    else if (!strcmp(key, "ablation")) c->ablation = (int)value;      // timing-only kernel variants: tuning build only
#endif
    else if (!strcmp(key, "light")) c->light = (int)value;
    else if (!strcmp(key, "wave_max")) c->wave_max = (int)value;
    else if (!strcmp(key, "fallback")) c->fallback = (int)value;
    else if (!strcmp(key, "q16_min")) c->q16_min = value;
    else if (!strcmp(key, "async")) c->async_mode = value != 0;
    else if (!strcmp(key, "per_node")) c->per_node = value != 0;
    else if (!strcmp(key, "upload_panel_bytes")) {
        if (value < 1) { lsq_set_error("upload_panel_bytes must be >= 1"); return LSQ_EINVAL; }
        c->panel_bytes = value;
    }
    else if (!strcmp(key, "upload_pipeline_min_bytes")) {
        if (value < 0) { lsq_set_error("upload_pipeline_min_bytes must be >= 0"); return LSQ_EINVAL; }
        c->pipeline_min_bytes = value;
    }
    else if (!strcmp(key, "filter_probe_div")) {
        if (value < 0) { lsq_set_error("filter_probe_div must be >= 0"); return LSQ_EINVAL; }
        c->probe_div = value;
    }
    else if (!strcmp(key, "filter_fallback_div")) {
        if (value < 0) { lsq_set_error("filter_fallback_div must be >= 0"); return LSQ_EINVAL; }
        c->fallback_div = value;
    }
    else if (!strcmp(key, "linscan_exhaustive")) c->search.force_exhaustive = value != 0;
    else if (!strcmp(key, "linscan_rank")) {
        if (value < 0) { lsq_set_error("linscan_rank must be >= 0"); return LSQ_EINVAL; }
        c->search.rank_override = (int)value;
    }
    else if (!strcmp(key, "knn_u8_int")) c->knn_u8_int = value != 0;
    else if (!strcmp(key, "rerank_batch")) {
        if (value < 0) { lsq_set_error("rerank_batch must be >= 0"); return LSQ_EINVAL; }
        c->rerank_batch = value;
    }
    else if (!strcmp(key, "range_batch")) {
        if (value < 0 || value > LSQ_RANGE_BATCH_RECORDS) { lsq_set_error("range_batch must lie in 0..2^28"); return LSQ_EINVAL; }
        c->range_batch = value;
    }
    else if (!strcmp(key, "recon_chunk")) {
        if (value < 0) { lsq_set_error("recon_chunk must be >= 0"); return LSQ_EINVAL; }
        c->recon_chunk = value;
    }
    else if (!strcmp(key, "snapshot_chunk")) {
        if (value < 0 || value > (1ll << 30)) { lsq_set_error("snapshot_chunk must lie in 0..2^30"); return LSQ_EINVAL; }
        c->snapshot_chunk = value;
    }
    else if (!strcmp(key, "ils_counter")) {
        if (value < 0 || value >= (int64_t)LSQ_IT_AUTO) { lsq_set_error("ils_counter must lie in 0..2^32-2"); return LSQ_EINVAL; }
        c->auto_it = (uint32_t)value;
    }
    else if (!strcmp(key, "schedule")) {
        if (value != 3 && value != 4 && value != 6) { lsq_set_error("schedule must be 3, 4 or 6"); return LSQ_EINVAL; }
        c->schedule = (int)value;
    } else { lsq_set_error("unknown option '%s'", key); return LSQ_EINVAL; }
    return LSQ_OK;
}

static int fill_timings(lsq_ctx *c, lsq_timings *out);

extern "C" int lsq_get_timings(lsq_ctx *c, lsq_timings *out) {
    if (!out) { lsq_set_error("lsq_get_timings: null out"); return LSQ_EINVAL; }
    // This symbol writes the v400 layout only -- a caller compiled against the v400 header and loading a newer library must not have its struct overrun
    // (ADVICE r5); the fields appended since (table_reuses, ...) are reached through lsq_get_timings_sized, which is told the caller's sizeof.
    lsq_timings t;
    LSQ_TRY(fill_timings(c, &t));
    memcpy(out, &t, offsetof(lsq_timings, table_reuses));
    return LSQ_OK;
}

extern "C" int lsq_get_timings_sized(lsq_ctx *c, void *out, size_t bytes) {
    if (!out) { lsq_set_error("lsq_get_timings_sized: null out"); return LSQ_EINVAL; }
    lsq_timings t;
    LSQ_TRY(fill_timings(c, &t));
    memcpy(out, &t, bytes < sizeof(t) ? bytes : sizeof(t));      // fields are only ever appended: an older caller gets the prefix it knows
    return LSQ_OK;
}

static int fill_timings(lsq_ctx *c, lsq_timings *out) {
    LSQ_TRY(use_device(c));
    LSQ_TRY(fold_pending(c));
    LSQ_TRY(resolve_timings(c));
    out->tables_ms = c->cat_ms[CAT_TABLES];
    out->unaries_ms = c->cat_ms[CAT_UNARIES];
    out->perturb_ms = c->cat_ms[CAT_PERTURB];
    out->icm_ms = c->cat_ms[CAT_ICM];
    out->cost_ms = c->cat_ms[CAT_COST];
    out->other_ms = c->cat_ms[CAT_OTHER];
    out->icm_launches = c->icm_launches;
    out->icm_node_updates = c->icm_node_updates;
    out->staged_blocks = c->staged_blocks;
    out->light_blocks = c->light_blocks;
    out->filtered_blocks = c->filtered_blocks;
    out->filter_refined = c->filter_refined;
    out->filter_exact = c->filter_exact;
    out->filter_f32 = c->filter_f32;
    out->filter_fallback_chunks = c->filter_fallback_chunks;
    out->xs_launches = 0;               // (schedule 7 left the tree in v600: the fields stay for the ABI)
    out->xs_fallback_launches = 0;
    out->table_reuses = c->table_reuses;
    return LSQ_OK;
}

extern "C" int lsq_get_walk_trace(lsq_ctx *c, int64_t *out, int count) {
    if (!c || !out || count < 0) { lsq_set_error("lsq_get_walk_trace: bad arguments"); return LSQ_EINVAL; }
    for (int q = 0; q < count; ++q) out[q] = q < LSQ_WALK_TRACE ? c->trace[q] : 0;
    return LSQ_OK;
}

// The level parameters, the levels and the f32 terms they were taken of, as the last filtered chunk left them: a copy in stream order, nothing else
static_assert(sizeof(lsq_q16_snapshot_params) == sizeof(lsq_q16_params) && sizeof(lsq_q16_snapshot_node) == sizeof(lsq_q16_node) &&
              offsetof(lsq_q16_snapshot_params, node) == offsetof(lsq_q16_params, node) && offsetof(lsq_q16_snapshot_node, window) == offsetof(lsq_q16_node, window) &&
              offsetof(lsq_q16_snapshot_node, slack) == offsetof(lsq_q16_node, slack) && offsetof(lsq_q16_snapshot_node, hiq) == offsetof(lsq_q16_node, hiq),
              "the public snapshot structure restates lsq_q16_params");
extern "C" int lsq_get_q16_snapshot(lsq_ctx *c, int what, void *dst, size_t bytes, int64_t *info) {
    LSQ_TRY(use_device(c));
    if (!c->chunk_road.resident) {
        lsq_set_error("lsq_get_q16_snapshot: no filtered chunk is resident (the last chunk whose unaries were built did not take the 16-bit filtered walk)");
        return LSQ_EINVAL;
    }
    const size_t cn = (size_t)c->chunk_road.cn, m = (size_t)c->chunk_road.m;
    const DevBuf *src = nullptr;
    size_t need = 0;
    switch (what) {
    case LSQ_SNAP_PARAMS: src = &c->qp; need = sizeof(lsq_q16_params); break;
    case LSQ_SNAP_UQ: src = &c->Uq; need = sizeof(uint16_t) * m * cn * LSQ_H; break;
    case LSQ_SNAP_TQ: src = &c->Tq; need = sizeof(uint16_t) * m * (m - 1) * LSQ_H * LSQ_H; break;
    case LSQ_SNAP_QFLAG: src = &c->qflag; need = sizeof(unsigned short) * cn; break;
    case LSQ_SNAP_U: src = &c->U; need = sizeof(float) * m * cn * LSQ_H; break;
    case LSQ_SNAP_T: src = &c->T; need = sizeof(float) * m * m * LSQ_H * LSQ_H; break;
    default: lsq_set_error("lsq_get_q16_snapshot: unknown item %d", what); return LSQ_EINVAL;
    }
    if (need > 0 && (!dst || bytes < need || src->cap < need)) {
        lsq_set_error("lsq_get_q16_snapshot: item %d takes %zu bytes, the buffer has %zu", what, need, dst ? bytes : (size_t)0);
        return LSQ_EINVAL;
    }
    if (info) {
        info[0] = c->chunk_road.cn; info[1] = c->chunk_road.row0; info[2] = c->chunk_road.m;
        info[3] = lsq_q16_slice_width(c->chunk_road.m); info[4] = lsq_walk_slice_width(c->chunk_road.m); info[5] = c->chunk_road.filtered ? 1 : 0;
    }
    if (need > 0) LSQ_HIP(hipMemcpyAsync(dst, src->p, need, hipMemcpyDefault, c->stream));
    return LSQ_OK;
}

extern "C" int lsq_reset_timings(lsq_ctx *c) {
    LSQ_TRY(use_device(c));
    LSQ_TRY(fold_pending(c));
    LSQ_TRY(resolve_timings(c));
    for (double &v : c->cat_ms) v = 0.0;
    c->icm_launches = c->icm_node_updates = c->staged_blocks = c->light_blocks = c->filtered_blocks = c->filter_refined = c->filter_exact = c->filter_f32 = 0;
    c->filter_fallback_chunks = 0;
    c->table_reuses = 0;
    for (int64_t &v : c->trace) v = 0;
    c->adc_stats = lsq_linscan_stats{};
    return LSQ_OK;
}

// ---- device ADC scan (lsq_adc.hip) -------------------------------------------------------------------------------------------------------
static int linscan_check(const char *fn, const void *a, const void *b, const void *c0, const void *d0, const void *e, const void *f, int nq, int n,
                         int m, int h, int d, int nn) {
    if (nq < 0 || n < 0 || d < 1 || nn < 1) { lsq_set_error("%s: bad shape nq=%d n=%d d=%d nn=%d", fn, nq, n, d, nn); return LSQ_EINVAL; }
    if (h != LSQ_H || m < 1 || m > LSQ_MAX_M) { lsq_set_error("%s: needs h == 256 and 1 <= m <= 16 (got h=%d m=%d)", fn, h, m); return LSQ_EINVAL; }
    if (nn > n) { lsq_set_error("%s: nn=%d exceeds the database size %d", fn, nn, n); return LSQ_EINVAL; }
    if (nq > 0 && (!a || !b || !c0 || !d0 || !e || !f)) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    return LSQ_OK;
}

// the context's hooks, with where this call's statistics go and whether its phases are timed
static lsq_search_opts search_opts(const lsq_ctx *c, lsq_linscan_stats *stats) {
    lsq_search_opts o = c->search;
    o.stats = stats;
    o.timed = c->profile;
    return o;
}

// the three kinds of search (lsq_search_input); the pointers are all device pointers or all host pointers
static lsq_search_input lsq_input(const uint8_t *codes, const float *Q, const float *K, const float *dbnorms, int n, int m, int d) {
    lsq_search_input in{};
    in.kind = LSQ_SEARCH_LSQ; in.codes = codes; in.cstride = m; in.Q = Q; in.qstride = d; in.K = K; in.dbnorms = dbnorms; in.n = n; in.m = m; in.d = d;
    return in;
}
static lsq_search_input pq_input(const uint8_t *codes, int cstride, const float *centers, const float *Q, int qstride, int n, int m, int subdim) {
    lsq_search_input in{};
    in.kind = LSQ_SEARCH_PQ; in.codes = codes; in.cstride = cstride; in.Q = Q; in.qstride = qstride; in.K = centers; in.n = n; in.m = m; in.d = subdim;
    return in;
}
static lsq_search_input exact_input(const void *base, int base_u8, int ldb, const void *Q, int q_u8, int ldq, int n, int d) {
    lsq_search_input in{};
    in.kind = LSQ_SEARCH_EXACT; in.Q = Q; in.qstride = ldq; in.n = n; in.d = d; in.base = base; in.bstride = ldb; in.base_u8 = base_u8; in.q_u8 = q_u8;
    return in;
}

extern "C" int lsq_linscan_dev(lsq_ctx *c, float *d_dists, int *d_idx, const uint8_t *d_codes, const float *d_queries, const float *d_codebooks,
                               const float *d_dbnorms, int nqueries, int ncodes, int m, int h, int d, int nn) {
    if (!c) { lsq_set_error("lsq_linscan_dev: null context"); return LSQ_EINVAL; }
    LSQ_TRY(linscan_check("lsq_linscan_dev", d_dists, d_idx, d_codes, d_queries, d_codebooks, d_dbnorms, nqueries, ncodes, m, h, d, nn));
    if (nqueries == 0) return LSQ_OK;
    LSQ_TRY(use_device(c));
    return lsq_adc_search(c->stream, &c->adc, d_dists, d_idx, lsq_input(d_codes, d_queries, d_codebooks, d_dbnorms, ncodes, m, d), nqueries, nn,
                          search_opts(c, &c->adc_stats));
}

extern "C" int lsq_linscan(lsq_ctx *c, float *dists, int *idx, const unsigned char *codes, const float *queries, const float *codebooks,
                           const float *dbnorms, int nqueries, int ncodes, int m, int h, int d, int nn) {
    if (!c) { lsq_set_error("lsq_linscan: null context"); return LSQ_EINVAL; }
    LSQ_TRY(linscan_check("lsq_linscan", dists, idx, codes, queries, codebooks, dbnorms, nqueries, ncodes, m, h, d, nn));
    if (nqueries == 0) return LSQ_OK;
    LSQ_TRY(use_device(c));
    return lsq_adc_search_host(c->stream, &c->adc, dists, idx, lsq_input(codes, queries, codebooks, dbnorms, ncodes, m, d), nqueries, nn,
                               search_opts(c, &c->adc_stats));
}

// the PQ / OPQ scan: the host drop-in's checks (lsq_linscan.hip), then the device limits of lsq_linscan
static int linscan_pq_check(const char *fn, const void *a, const void *b, const void *c0, const void *d0, const void *e, int N, uint32_t NQ, int B,
                            int K, int dim1codes, int dim1queries, int subdim) {
    LSQ_TRY(lsq_linscan_pq_check(fn, a, b, c0, d0, e, N, NQ, B, K, dim1codes, dim1queries, subdim));
    if (B / 8 > LSQ_MAX_M) { lsq_set_error("%s: the device scan needs B/8 <= 16 (got B=%d: %d sub-spaces)", fn, B, B / 8); return LSQ_EINVAL; }
    if (NQ > (uint32_t)INT32_MAX) { lsq_set_error("%s: NQ=%u exceeds the device scan's limit of 2^31 - 1 queries", fn, NQ); return LSQ_EINVAL; }
    return LSQ_OK;
}

extern "C" int lsq_linscan_pq_dev(lsq_ctx *c, float *d_dists, uint32_t *d_res, const uint8_t *d_codes, const float *d_centers, const float *d_queries,
                                  int N, uint32_t NQ, int B, int K, int dim1codes, int dim1queries, int subdim) {
    if (!c) { lsq_set_error("lsq_linscan_pq_dev: null context"); return LSQ_EINVAL; }
    LSQ_TRY(linscan_pq_check("lsq_linscan_pq_dev", d_dists, d_res, d_codes, d_centers, d_queries, N, NQ, B, K, dim1codes, dim1queries, subdim));
    if (NQ == 0) return LSQ_OK;
    LSQ_TRY(use_device(c));
    return lsq_adc_search(c->stream, &c->adc, d_dists, reinterpret_cast<int *>(d_res),
                          pq_input(d_codes, dim1codes, d_centers, d_queries, dim1queries, N, B / 8, subdim), (int)NQ, K, search_opts(c, &c->adc_stats));
}

extern "C" int lsq_linscan_pq(lsq_ctx *c, float *dists, uint32_t *res, const uint8_t *codes, const float *centers, const float *queries, int N,
                              uint32_t NQ, int B, int K, int dim1codes, int dim1queries, int subdim) {
    if (!c) { lsq_set_error("lsq_linscan_pq: null context"); return LSQ_EINVAL; }
    LSQ_TRY(linscan_pq_check("lsq_linscan_pq", dists, res, codes, centers, queries, N, NQ, B, K, dim1codes, dim1queries, subdim));
    if (NQ == 0) return LSQ_OK;
    LSQ_TRY(use_device(c));
    return lsq_adc_search_host(c->stream, &c->adc, dists, reinterpret_cast<int *>(res), pq_input(codes, dim1codes, centers, queries, dim1queries, N, B / 8, subdim),
                               (int)NQ, K, search_opts(c, &c->adc_stats));
}

// exact k-NN: the host drop-in's checks (lsq_linscan.hip), then the device search (lsq_knn.hip under lsq_adc.hip's selection)
extern "C" int lsq_knn_exact_dev(lsq_ctx *c, float *d_dists, uint32_t *d_ids, const float *d_base, const float *d_queries, int n, int nq, int d, int ldb,
                                 int ldq, int nn) {
    if (!c) { lsq_set_error("lsq_knn_exact_dev: null context"); return LSQ_EINVAL; }
    LSQ_TRY(lsq_knn_exact_check("lsq_knn_exact_dev", d_dists, d_ids, d_base, d_queries, n, nq, d, ldb, ldq, nn));
    LSQ_TRY(use_device(c));
    return lsq_adc_search(c->stream, &c->adc, d_dists, reinterpret_cast<int *>(d_ids), exact_input(d_base, 0, ldb, d_queries, 0, ldq, n, d), nq, nn,
                          search_opts(c, &c->adc_stats));
}

extern "C" int lsq_knn_exact(lsq_ctx *c, float *dists, uint32_t *ids, const float *base, const float *queries, int n, int nq, int d, int ldb, int ldq,
                             int nn) {
    if (!c) { lsq_set_error("lsq_knn_exact: null context"); return LSQ_EINVAL; }
    LSQ_TRY(lsq_knn_exact_check("lsq_knn_exact", dists, ids, base, queries, n, nq, d, ldb, ldq, nn));
    LSQ_TRY(use_device(c));
    return lsq_adc_search_host(c->stream, &c->adc, dists, reinterpret_cast<int *>(ids), exact_input(base, 0, ldb, queries, 0, ldq, n, d), nq, nn,
                               search_opts(c, &c->adc_stats));
}

extern "C" int lsq_get_linscan_stats(lsq_ctx *c, lsq_linscan_stats *out) {
    if (!c || !out) { lsq_set_error("lsq_get_linscan_stats: null argument"); return LSQ_EINVAL; }
    *out = c->adc_stats;
    return LSQ_OK;
}

// ---- two-stage search on a resident index: the ADC scan (lsq_adc.hip), then the exact re-rank of its shortlists (lsq_rerank.hip) -------------------------
struct lsq_index {
    lsq_ctx *ctx = nullptr;
    int64_t n = 0;
    int d = 0, m = 0, base_u8 = 0;                      // base_u8: the FORMAT of the base rows (lsq_base_format: 0 f32, 1 uint8, LSQ_BASE_F16, LSQ_BASE_BF16)
    int64_t ldb = 0;
    const uint8_t *codes = nullptr;                    // device pointers: the index's own copies (host-buffer description) or the caller's (borrowed)
    const float *K = nullptr, *norms = nullptr;
    const void *base = nullptr;
    DevBuf own_codes, own_K, own_norms, own_base;
    int packed = 0, ncb = 0;                           // lsq_index_create_packed: codes = own_codes = rows of m + 1 bytes (code bytes, norm byte), norms = own_norms =
                                                       // the norm table padded to 256 floats; nothing else reads either
    lsq_linscan_stats scan{};                          // the selection statistics of the last lsq_index_search scan
    lsq_adc_state *adc = nullptr;                      // the scan's state of THIS index: never ctx->adc
    DevBuf rec_a, rec_b, seg, counter;                 // stage two: records, sorted records, segment bounds, the invalid-id counter
    DevBuf short_d, short_i;                           // stage one's shortlist [nq][L]
    DevBuf s_qscan, s_qexact, s_cand, s_dists, s_ids;  // staging of host-buffer calls, and of scan queries whose rows are not d floats apart
    DevBuf nrm_x, nrm_q;                               // lsq_index_knn's integer road: uint32 squared norms of the rows and of the queries, refilled at every call
    lsq_ivf_state *ivf = nullptr;                      // the inverted lists (lsq_ivf.hip): layout and scratch of THIS index; null until lsq_index_set_lists
    DevBuf s_qcoarse;                                  // lsq_index_search_ivf's staging of host q_coarse rows
    PhaseClock<3> clock;                               // a re-rank batch's gather and selection; lsq_index_knn's norm pass
    lsq_index_stats stats{};
    lsq_index_knn_info knn{};
    lsq_filter_state *filter = nullptr;                // the row filter (lsq_filter.hip): null until lsq_index_set_filter; owned copies of THIS index
    int64_t cap_rows = 0;                              // lsq_index_add: rows the flat arrays hold without another allocation (n until the first add / reserve)
    lsq_index_growth_info grow{};
    DevBuf g_codes, g_nc, g_rows;                      // lsq_index_add on a packed index: staging of host codes and norm bytes, the new rows packed
    PhaseClock<4> gclock;                              // an add's append, merge and filter phases
    lsq_index_compact_info cinfo{};                    // lsq_index_remove / _compact
    DevBuf c_old, c_new;                               // lsq_index_compact into host arrays: the maps on the device
    PhaseClock<3> cclock;                              // a remove's tombstones; a compact's gather and layout phases
    lsq_range_state *range = nullptr;                  // range search (lsq_range.hip): its scratch and the HELD result of the last one; null until the first
    DevBuf s_radius;                                   // lsq_index_range_search's staging of host radii
    DevBuf r_lor, r_ids, r_out, r_q;                   // the decode (lsq_recon.hip): the row -> list map [n], staged host ids, a host call's staged output chunk,
                                                       // lsq_index_search_rows' decoded queries [nq][d]
    bool r_lor_valid = false;                          // r_lor answers for the inverted layout in force (lsq_index_set_lists / _add / _compact clear it)
    lsq_index_recon_info rinfo{};
    PhaseClock<3> rclock;                              // a decode's map and decode phases
    DevBuf h_counts;                                   // lsq_index_narrow_base: the three counters of the convert
    lsq_narrow_counts hcounts{};                       // ... read back, and its time
    double narrow_ms = 0.0;
    PhaseClock<2> hclock;
    lsq_snapshot_io_info sinfo{};                      // the last lsq_index_save, or the lsq_index_load that made this index
};

// the filter as a scan over all rows takes it: nothing without one; else the compact road -- the ascending list of allowed rows -- where the measured rule
// says so (lsq_filter_compact_by_default; sort_over_scan: the call's constant) or forced, the dense road -- the bitmap beside every row -- otherwise.
// *road: 0 unfiltered, 1 dense, 2 compact
static void index_apply_filter(lsq_index *ix, lsq_search_input *in, int *road, int64_t sort_over_scan) {
    *road = 0;
    if (!lsq_filter_active(ix->filter)) return;
    const lsq_filter_view v = lsq_filter_get(ix->filter);
    const bool compact = v.force == LSQ_FILTER_FORCE_COMPACT || (v.force == 0 && lsq_filter_compact_by_default(ix->n, v.allowed, sort_over_scan));
    if (compact) { in->filter_rows = v.rows; in->filter_count = (int)v.allowed; }
    else in->filter_bits = v.bits;
    *road = compact ? 2 : 1;
}

extern "C" int lsq_index_destroy(lsq_index *ix) {
    if (!ix) return LSQ_OK;
    (void)hipSetDevice(ix->ctx->device);
    (void)hipStreamSynchronize(ix->ctx->stream);
    DevBuf *bufs[] = {&ix->own_codes, &ix->own_K, &ix->own_norms, &ix->own_base, &ix->rec_a, &ix->rec_b, &ix->seg, &ix->counter, &ix->short_d, &ix->short_i,
                      &ix->s_qscan, &ix->s_qexact, &ix->s_cand, &ix->s_dists, &ix->s_ids, &ix->nrm_x, &ix->nrm_q, &ix->s_qcoarse, &ix->g_codes, &ix->g_nc, &ix->g_rows,
                      &ix->c_old, &ix->c_new, &ix->s_radius, &ix->r_lor, &ix->r_ids, &ix->r_out, &ix->r_q, &ix->h_counts};
    for (DevBuf *b : bufs) b->release();
    lsq_range_free(ix->range);
    ix->gclock.release();
    ix->cclock.release();
    ix->rclock.release();
    ix->hclock.release();
    lsq_adc_free(ix->adc);
    lsq_ivf_free(ix->ivf);
    lsq_filter_free(ix->filter);
    ix->clock.release();
    delete ix;
    return LSQ_OK;
}

static int index_adopt(lsq_index *ix, DevBuf &own, const void *src, size_t bytes, int on_device, const void **dst) {
    if (on_device) { *dst = src; return LSQ_OK; }
    LSQ_TRY(own.ensure(bytes));
    LSQ_HIP(hipMemcpyAsync(own.p, src, bytes, hipMemcpyHostToDevice, ix->ctx->stream));
    *dst = own.p;
    return LSQ_OK;
}

extern "C" int lsq_index_create(lsq_index **out, lsq_ctx *c, const lsq_index_desc *desc) {
    if (!out) { lsq_set_error("lsq_index_create: null out pointer"); return LSQ_EINVAL; }
    *out = nullptr;
    if (!c || !desc) { lsq_set_error("lsq_index_create: null %s", c ? "description" : "context"); return LSQ_EINVAL; }
    if (!desc->codes && !desc->base) { lsq_set_error("lsq_index_create: neither codes nor base rows"); return LSQ_EINVAL; }
    if (desc->n < 1 || desc->n > (int64_t)INT32_MAX - 1 || desc->d < 1) {
        lsq_set_error("lsq_index_create: needs 1 <= n <= 2^31 - 2 and d >= 1 (got n=%lld d=%d)", (long long)desc->n, desc->d);
        return LSQ_EINVAL;
    }
    if (desc->codes) {
        if (desc->h != LSQ_H || desc->m < 1 || desc->m > LSQ_MAX_M) {
            lsq_set_error("lsq_index_create: needs h == 256 and 1 <= m <= 16 (got h=%d m=%d)", desc->h, desc->m);
            return LSQ_EINVAL;
        }
        if (!desc->codebooks || !desc->dbnorms) { lsq_set_error("lsq_index_create: codes without codebooks or dbnorms"); return LSQ_EINVAL; }
    }
    if (desc->base && desc->ldb < desc->d) { lsq_set_error("lsq_index_create: needs ldb >= d (got ldb=%d d=%d)", desc->ldb, desc->d); return LSQ_EINVAL; }
    if (desc->base) if (const char *why = lsq_base_align_refusal(lsq_base_format(desc->base_u8), desc->base)) { lsq_set_error("lsq_index_create: %s", why); return LSQ_EINVAL; }
    LSQ_TRY(use_device(c));
    lsq_index *ix = new lsq_index();
    ix->ctx = c;
    ix->n = desc->n; ix->d = desc->d; ix->m = desc->codes ? desc->m : 0; ix->base_u8 = lsq_base_format(desc->base_u8); ix->ldb = desc->ldb;
    const size_t n = (size_t)desc->n, d = (size_t)desc->d;
    int rc = LSQ_OK;
    if (desc->codes) {
        rc = index_adopt(ix, ix->own_codes, desc->codes, n * (size_t)desc->m, desc->on_device, reinterpret_cast<const void **>(&ix->codes));
        if (rc == LSQ_OK) rc = index_adopt(ix, ix->own_K, desc->codebooks, sizeof(float) * (size_t)desc->m * LSQ_H * d, desc->on_device, reinterpret_cast<const void **>(&ix->K));
        if (rc == LSQ_OK) rc = index_adopt(ix, ix->own_norms, desc->dbnorms, sizeof(float) * n, desc->on_device, reinterpret_cast<const void **>(&ix->norms));
    }
    if (rc == LSQ_OK && desc->base)      // rows up to the d-th element of the last one
        rc = index_adopt(ix, ix->own_base, desc->base, ((n - 1) * (size_t)desc->ldb + d) * lsq_base_elem_bytes(ix->base_u8), desc->on_device, &ix->base);
    if (rc == LSQ_OK) rc = ix->counter.ensure(sizeof(unsigned long long));
    if (rc == LSQ_OK && hipStreamSynchronize(c->stream) != hipSuccess) { lsq_set_error("lsq_index_create: the upload failed"); rc = LSQ_EHIP; }
    if (rc != LSQ_OK) { (void)lsq_index_destroy(ix); return rc; }
    ix->cap_rows = ix->n;
    *out = ix;
    return LSQ_OK;
}

// The packed index: the caller's (codes, norm bytes) become rows the index owns, cbnorms a table of 256 floats; everything else is lsq_index_create's
extern "C" int lsq_index_create_packed(lsq_index **out, lsq_ctx *c, const lsq_index_packed_desc *desc) {
    const char *fn = "lsq_index_create_packed";
    if (!out) { lsq_set_error("%s: null out pointer", fn); return LSQ_EINVAL; }
    *out = nullptr;
    if (!c || !desc) { lsq_set_error("%s: null %s", fn, c ? "description" : "context"); return LSQ_EINVAL; }
    if (!desc->codes) { lsq_set_error("%s: no codes (a base-only index is lsq_index_create's)", fn); return LSQ_EINVAL; }
    if (desc->n < 1 || desc->n > (int64_t)INT32_MAX - 1 || desc->d < 1) {
        lsq_set_error("%s: needs 1 <= n <= 2^31 - 2 and d >= 1 (got n=%lld d=%d)", fn, (long long)desc->n, desc->d);
        return LSQ_EINVAL;
    }
    if (desc->h != LSQ_H || desc->m < 1 || desc->m > LSQ_MAX_M) { lsq_set_error("%s: needs h == 256 and 1 <= m <= 16 (got h=%d m=%d)", fn, desc->h, desc->m); return LSQ_EINVAL; }
    if (!desc->codebooks || !desc->norm_codes || !desc->cbnorms) { lsq_set_error("%s: codes without codebooks, norm_codes or cbnorms", fn); return LSQ_EINVAL; }
    if (desc->ncb < 1 || desc->ncb > 256) { lsq_set_error("%s: needs 1 <= ncb <= 256 (got %d)", fn, desc->ncb); return LSQ_EINVAL; }
    if (desc->base && desc->ldb < desc->d) { lsq_set_error("%s: needs ldb >= d (got ldb=%d d=%d)", fn, desc->ldb, desc->d); return LSQ_EINVAL; }
    if (desc->base) if (const char *why = lsq_base_align_refusal(lsq_base_format(desc->base_u8), desc->base)) { lsq_set_error("%s: %s", fn, why); return LSQ_EINVAL; }
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    lsq_index *ix = new lsq_index();
    ix->ctx = c;
    ix->n = desc->n; ix->d = desc->d; ix->m = desc->m; ix->base_u8 = lsq_base_format(desc->base_u8); ix->ldb = desc->ldb;
    ix->packed = 1; ix->ncb = desc->ncb;
    const size_t n = (size_t)desc->n, d = (size_t)desc->d, m = (size_t)desc->m;
    DevBuf s_codes, s_nc;                              // the host form's staging of what the pack kernel reads: gone when the call returns
    unsigned bad = 0;
    auto build = [&]() -> int {
        const uint8_t *dcodes = desc->codes, *dnc = desc->norm_codes;
        if (!desc->on_device) {
            LSQ_TRY(s_codes.ensure(n * m));
            LSQ_TRY(s_nc.ensure(n));
            LSQ_HIP(hipMemcpyAsync(s_codes.p, desc->codes, n * m, hipMemcpyHostToDevice, s));
            LSQ_HIP(hipMemcpyAsync(s_nc.p, desc->norm_codes, n, hipMemcpyHostToDevice, s));
            dcodes = s_codes.as<uint8_t>(); dnc = s_nc.as<uint8_t>();
        }
        LSQ_TRY(ix->own_codes.ensure(n * (m + 1) + 16));      // 16 bytes of slack past the last row, never read
        LSQ_TRY(ix->own_norms.ensure(sizeof(float) * 256));
        LSQ_TRY(ix->counter.ensure(sizeof(unsigned long long)));
        LSQ_HIP(hipMemsetAsync(ix->counter.p, 0, sizeof(unsigned long long), s));
        LSQ_HIP(hipMemsetAsync(ix->own_norms.p, 0, sizeof(float) * 256, s));       // entries >= ncb: never addressed
        LSQ_HIP(hipMemcpyAsync(ix->own_norms.p, desc->cbnorms, sizeof(float) * (size_t)desc->ncb, desc->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        LSQ_TRY(lsq_adc_launch_pack(s, dcodes, dnc, desc->n, desc->m, desc->ncb, ix->own_codes.as<uint8_t>(), ix->counter.as<unsigned>()));
        LSQ_HIP(hipMemcpyAsync(&bad, ix->counter.p, sizeof(bad), hipMemcpyDeviceToHost, s));
        ix->codes = ix->own_codes.as<uint8_t>();
        ix->norms = ix->own_norms.as<float>();
        LSQ_TRY(index_adopt(ix, ix->own_K, desc->codebooks, sizeof(float) * m * LSQ_H * d, desc->on_device, reinterpret_cast<const void **>(&ix->K)));
        if (desc->base)
            LSQ_TRY(index_adopt(ix, ix->own_base, desc->base, ((n - 1) * (size_t)desc->ldb + d) * lsq_base_elem_bytes(ix->base_u8), desc->on_device, &ix->base));
        if (hipStreamSynchronize(s) != hipSuccess) { lsq_set_error("%s: the upload failed", fn); return LSQ_EHIP; }
        if (bad) { lsq_set_error("%s: %u norm bytes lie outside [0, %d)", fn, bad, desc->ncb); return LSQ_EINVAL; }
        return LSQ_OK;
    };
    const int rc = build();
    if (rc != LSQ_OK && rc != LSQ_EINVAL) (void)hipStreamSynchronize(s);      // nothing in flight reads the staging when it goes
    s_codes.release(); s_nc.release();
    if (rc != LSQ_OK) { (void)lsq_index_destroy(ix); return rc; }
    ix->cap_rows = ix->n;
    *out = ix;
    return LSQ_OK;
}

extern "C" int lsq_index_get_packed_info(lsq_index *ix, lsq_index_packed_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_packed_info: null argument"); return LSQ_EINVAL; }
    *out = lsq_index_packed_info{};
    if (!ix->packed) return LSQ_OK;
    out->row_bytes = ix->m + 1;
    out->ivf_row_bytes = lsq_ivf_nlist(ix->ivf) > 0 ? ix->m + 5 : 0;
    out->ncb = ix->ncb;
    out->dword_rows = (ix->m + 1) % 4 == 0 ? 1 : 0;
    out->resident_bytes = ix->n * (int64_t)(ix->m + 1) + 4 * (int64_t)ix->ncb;
    return LSQ_OK;
}

extern "C" int lsq_index_get_scan_stats(lsq_index *ix, lsq_linscan_stats *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_scan_stats: null argument"); return LSQ_EINVAL; }
    *out = ix->scan;
    return LSQ_OK;
}

// stage two on device buffers: queries [nq][ldq], cand [nq][L] -> dists / ids [nq][nn], in batches of queries
static int index_rerank_dev(lsq_index *ix, float *d_dists, int *d_ids, const float *d_q, int64_t ldq, const int *d_cand, int nq, int L, int nn, int id_base) {
    lsq_ctx *c = ix->ctx;
    hipStream_t s = c->stream;
    // L record slots per query (L <= 2^28: every caller checks it before anything is launched); option "rerank_batch" only makes batches smaller
    int64_t qb = lsq_adc_batch_queries(L);
    if (c->rerank_batch > 0 && c->rerank_batch < qb) qb = c->rerank_batch;
    if (qb > nq) qb = nq;
    LSQ_TRY(ix->rec_a.ensure(sizeof(uint64_t) * (size_t)qb * L));
    LSQ_TRY(ix->rec_b.ensure(sizeof(uint64_t) * (size_t)qb * L));
    LSQ_TRY(ix->seg.ensure(sizeof(int) * 2 * (size_t)qb));
    LSQ_HIP(hipMemsetAsync(ix->counter.p, 0, sizeof(unsigned long long), s));
    const int idbits = lsq_adc_idbits(ix->n);
    for (int q0 = 0; q0 < nq; q0 += (int)qb) {
        const int nqb = (int)std::min<int64_t>(qb, nq - q0);
        LSQ_TRY(ix->clock.begin(c->profile != 0));
        LSQ_TRY(ix->clock.mark(s));
        LSQ_TRY(lsq_rerank_launch(s, ix->base, ix->base_u8, ix->ldb, ix->n, d_q, ldq, d_cand, q0, nqb, L, ix->d, id_base, ix->rec_a.as<uint64_t>(), idbits,
                                  ix->counter.as<unsigned long long>()));
        LSQ_TRY(ix->clock.mark(s));
        // records: (outside-the-base bit, distance key, row + 1); the gather hands out row + 1 - (1 - id_base)
        LSQ_TRY(lsq_adc_select(&ix->adc, s, ix->rec_a.as<uint64_t>(), ix->rec_b.as<uint64_t>(), ix->seg.as<int>(), nullptr, nullptr, nullptr, q0, nqb, L, nn,
                               d_dists, d_ids, idbits, 33 + idbits, 1 - id_base));
        LSQ_TRY(ix->clock.mark(s));
        float ms[2];
        LSQ_TRY(ix->clock.read(ms));                  // (untimed: zeros, and no wait)
        ix->stats.gather_ms += ms[0]; ix->stats.select_ms += ms[1];
        ix->stats.batches += 1;
    }
    unsigned long long bad = 0;
    LSQ_HIP(hipMemcpyAsync(&bad, ix->counter.p, sizeof(bad), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    ix->stats.invalid += (int64_t)bad;
    ix->stats.rows += (int64_t)nq * L - (int64_t)bad;
    return LSQ_OK;
}

// The buffers of one call on an index, said once for its four entry points (the recipe of the host forms): where the device reads the call's
// rows, where it writes the results, and how the call ends.  dev: the caller's pointers are device pointers (on_device)
struct IndexCall {
    lsq_index *ix;
    int nq;
    bool dev;
    float *dists = nullptr, *out_d = nullptr;
    int *ids = nullptr, *out_i = nullptr;
    size_t items = 0;
    // nq rows of `width` elements of `elem` bytes, ld elements apart, at src (host or device) -> device rows *dst, *ld_out apart.  stage = 0: read where they
    // lie.  Otherwise copied to buf: as they lie up to the width-th element of the last row (pack = 0), or compacted to `width` elements apart
    template <class T>
    int rows(DevBuf &buf, const T *src, size_t elem, int64_t ld, int width, bool pack, bool stage, const T **dst, int64_t *ld_out) {
        hipStream_t s = ix->ctx->stream;
        *dst = src; *ld_out = ld;
        if (!stage) return LSQ_OK;
        if (pack && ld != width) {
            LSQ_TRY(buf.ensure(elem * (size_t)nq * width));
            LSQ_HIP(hipMemcpy2DAsync(buf.p, elem * (size_t)width, src, elem * (size_t)ld, elem * (size_t)width, (size_t)nq, hipMemcpyDefault, s));
            *ld_out = width;
        } else {
            const size_t bytes = elem * ((size_t)(nq - 1) * (size_t)ld + (size_t)width);
            LSQ_TRY(buf.ensure(bytes));
            LSQ_HIP(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyDefault, s));
        }
        *dst = static_cast<const T *>(buf.p);
        return LSQ_OK;
    }
    // results [nq][nn]: the device form writes straight into the caller's arrays, the host form into the index's staging
    int outputs(float *caller_d, int *caller_i, int nn) {
        dists = out_d = caller_d; ids = out_i = caller_i; items = (size_t)nq * (size_t)nn;
        if (dev) return LSQ_OK;
        LSQ_TRY(ix->s_dists.ensure(sizeof(float) * items));
        LSQ_TRY(ix->s_ids.ensure(sizeof(int) * items));
        out_d = ix->s_dists.as<float>(); out_i = ix->s_ids.as<int>();
        return LSQ_OK;
    }
    // host form: the two fetches and the call's one wait of its own
    int finish() {
        if (!dev) {
            hipStream_t s = ix->ctx->stream;
            LSQ_HIP(hipMemcpyAsync(dists, out_d, sizeof(float) * items, hipMemcpyDeviceToHost, s));
            LSQ_HIP(hipMemcpyAsync(ids, out_i, sizeof(int) * items, hipMemcpyDeviceToHost, s));
            LSQ_HIP(hipStreamSynchronize(s));
        }
        ix->stats.queries += nq;
        return LSQ_OK;
    }
};

static int index_call_check(const char *fn, lsq_index *ix, const void *dists, const void *ids, int nq, int64_t ldq, int nn) {
    if (!ix) { lsq_set_error("%s: null index", fn); return LSQ_EINVAL; }
    if (nq < 0 || nn < 1 || ldq < ix->d) { lsq_set_error("%s: needs nq >= 0, nn >= 1, ldq >= d (got nq=%d nn=%d ldq=%lld d=%d)", fn, nq, nn, (long long)ldq, ix->d); return LSQ_EINVAL; }
    if (!dists || !ids) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    return LSQ_OK;
}

extern "C" int lsq_index_rerank(lsq_index *ix, float *dists, int *ids, const float *queries, const int *cand, int nq, int ldq, int L, int nn, int id_base,
                                int on_device) {
    LSQ_TRY(index_call_check("lsq_index_rerank", ix, dists, ids, nq, ldq, nn));
    if (!ix->base) { lsq_set_error("lsq_index_rerank: the index holds no base rows"); return LSQ_EINVAL; }
    LSQ_TRY(lsq_rerank_check("lsq_index_rerank", dists, ids, ix->base, queries, cand, ix->n, nq, ix->d, ix->ldb, ldq, L, nn, id_base));
    if (L > (1 << 28)) { lsq_set_error("lsq_index_rerank: needs L <= 2^28 candidates per query (got %d)", L); return LSQ_EINVAL; }      // a batch is >= 1 query
    if (nq == 0) return LSQ_OK;
    LSQ_TRY(use_device(ix->ctx));
    IndexCall call{ix, nq, on_device != 0};
    const float *dq = nullptr;
    const int *dc = nullptr;
    int64_t ld = 0, ldc = 0;
    LSQ_TRY(call.rows(ix->s_qexact, queries, sizeof(float), ldq, ix->d, false, !on_device, &dq, &ld));      // both as they lie
    LSQ_TRY(call.rows(ix->s_cand, cand, sizeof(int), L, L, false, !on_device, &dc, &ldc));
    LSQ_TRY(call.outputs(dists, ids, nn));
    LSQ_TRY(index_rerank_dev(ix, call.out_d, call.out_i, dq, ld, dc, nq, L, nn, id_base));
    return call.finish();
}

// the shortlist of a two-stage call -> *L, the length of stage one's lists
static int index_shortlist(const char *fn, int shortlist, int nn, int *L) {
    if (shortlist < 0 || (shortlist > 0 && shortlist < nn)) { lsq_set_error("%s: needs shortlist == 0 or shortlist >= nn (got shortlist=%d nn=%d)", fn, shortlist, nn); return LSQ_EINVAL; }
    *L = shortlist > 0 ? shortlist : nn;
    return LSQ_OK;
}

// The two-stage road, after the entry point's own checks: stage1(scan_d, scan_i, dqs, L) -> int fills lists [nq][L] of (distance, 1-based id) from the scan
// queries dqs [nq][d]; with a shortlist these are re-ranked to nn by exact distance (an id outside the base, stage one's (+inf, 0), is never dereferenced
// and comes last), without one they are the results
template <class Stage1>
static int index_two_stage(const char *fn, IndexCall &call, float *dists, int *ids, const float *q_scan, const float *q_exact, int ldq, int shortlist,
                           int nn, int L, Stage1 stage1) {
    lsq_index *ix = call.ix;
    const int nq = call.nq, d = ix->d;
    if (shortlist > 0 && !ix->base) { lsq_set_error("%s: a shortlist needs base rows, the index holds none", fn); return LSQ_EINVAL; }
    if (!q_scan || (shortlist > 0 && !q_exact)) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (nq == 0) return LSQ_OK;
    LSQ_TRY(use_device(ix->ctx));
    // stage one reads query rows d floats apart; the re-rank reads rows as they lie
    const float *dqs = nullptr, *dqe = nullptr;
    int64_t ld = 0, lde = 0;
    LSQ_TRY(call.rows(ix->s_qscan, q_scan, sizeof(float), ldq, d, true, !call.dev || ldq != d, &dqs, &ld));
    if (shortlist > 0) LSQ_TRY(call.rows(ix->s_qexact, q_exact, sizeof(float), ldq, d, false, !call.dev, &dqe, &lde));
    LSQ_TRY(call.outputs(dists, ids, nn));
    float *scan_d = call.out_d;
    int *scan_i = call.out_i;
    if (shortlist > 0) {
        LSQ_TRY(ix->short_d.ensure(sizeof(float) * (size_t)nq * L));
        LSQ_TRY(ix->short_i.ensure(sizeof(int) * (size_t)nq * L));
        scan_d = ix->short_d.as<float>();
        scan_i = ix->short_i.as<int>();
    }
    LSQ_TRY(stage1(scan_d, scan_i, dqs, L));
    if (shortlist > 0) LSQ_TRY(index_rerank_dev(ix, call.out_d, call.out_i, dqe, lde, scan_i, nq, L, nn, 1));
    return call.finish();
}

extern "C" int lsq_index_search(lsq_index *ix, float *dists, int *ids, const float *q_scan, const float *q_exact, int nq, int ldq, int shortlist, int nn,
                                int on_device) {
    LSQ_TRY(index_call_check("lsq_index_search", ix, dists, ids, nq, ldq, nn));
    if (!ix->codes) { lsq_set_error("lsq_index_search: the index holds no codes"); return LSQ_EINVAL; }
    int L = 0;
    LSQ_TRY(index_shortlist("lsq_index_search", shortlist, nn, &L));
    if (L > ix->n) { lsq_set_error("lsq_index_search: %s=%d exceeds the database size %lld", shortlist > 0 ? "shortlist" : "nn", L, (long long)ix->n); return LSQ_EINVAL; }
    if (shortlist > (1 << 28)) { lsq_set_error("lsq_index_search: needs shortlist <= 2^28 (got %d)", shortlist); return LSQ_EINVAL; }
    lsq_ctx *c = ix->ctx;
    IndexCall call{ix, nq, on_device != 0};
    return index_two_stage("lsq_index_search", call, dists, ids, q_scan, q_exact, ldq, shortlist, nn, L,
                           [&](float *scan_d, int *scan_i, const float *dqs, int len) -> int {      // the ADC scan of every row
        lsq_linscan_stats st{};
        lsq_search_input in = lsq_input(ix->codes, dqs, ix->K, ix->norms, (int)ix->n, ix->m, ix->d);
        if (ix->packed) { in.packed = 1; in.cstride = ix->m + 1; }      // rows with their norm byte; norms is the table
        int road = 0;
        index_apply_filter(ix, &in, &road, 64);
        lsq_filter_note_road(ix->filter, road);
        LSQ_TRY(lsq_adc_search(c->stream, &ix->adc, scan_d, scan_i, in, nq, len, search_opts(c, &st)));
        ix->scan = st;
        ix->stats.scan_ms += st.lut_ms + st.sample_ms + st.scan_ms + st.select_ms;
        return LSQ_OK;
    });
}

// exact k-NN over the resident base rows: lsq_knn_exact_dev's search (lsq_adc_search on the "exact" input) with the index's own scan state
extern "C" int lsq_index_knn(lsq_index *ix, float *dists, int *ids, const void *queries, int queries_u8, int nq, int ldq, int nn, int id_base,
                             int on_device) {
    if (!ix) { lsq_set_error("lsq_index_knn: null index"); return LSQ_EINVAL; }
    if (!ix->base) { lsq_set_error("lsq_index_knn: the index holds no base rows"); return LSQ_EINVAL; }
    if (!dists || !ids || !queries) { lsq_set_error("lsq_index_knn: null pointer"); return LSQ_EINVAL; }
    if (nq < 1 || ldq < ix->d) { lsq_set_error("lsq_index_knn: needs nq >= 1 and ldq >= d (got nq=%d ldq=%d d=%d)", nq, ldq, ix->d); return LSQ_EINVAL; }
    if (nn < 1 || nn > ix->n) { lsq_set_error("lsq_index_knn: needs 1 <= nn <= n (got nn=%d n=%lld)", nn, (long long)ix->n); return LSQ_EINVAL; }
    if (id_base != 0 && id_base != 1) { lsq_set_error("lsq_index_knn: id_base must be 0 or 1 (got %d)", id_base); return LSQ_EINVAL; }
    const int q_u8 = queries_u8 != 0;
    if (!q_u8 && ((uintptr_t)queries & 3) != 0) { lsq_set_error("lsq_index_knn: the f32 queries are not 4-byte aligned"); return LSQ_EINVAL; }
    if (ix->ldb > (int64_t)INT32_MAX) { lsq_set_error("lsq_index_knn: needs ldb <= 2^31 - 1"); return LSQ_EINVAL; }
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    const int n = (int)ix->n, d = ix->d;
    IndexCall call{ix, nq, on_device != 0};
    const void *dq = nullptr;
    int64_t ld = 0;
    LSQ_TRY(call.rows(ix->s_qexact, queries, q_u8 ? 1 : sizeof(float), ldq, d, false, !on_device, &dq, &ld));      // as they lie
    LSQ_TRY(call.outputs(dists, ids, nn));
    lsq_search_input in = exact_input(ix->base, ix->base_u8, (int)ix->ldb, dq, q_u8, ldq, n, d);
    in.id_base = id_base;
    const bool int_road = ix->base_u8 == 1 && q_u8 && d <= 258 && c->knn_u8_int;      // d 255^2 <= 2^24: (float)D is the chain's result
    lsq_index_knn_info info{};
    if (int_road) {
        // nothing is cached across calls: a borrowed base may have changed since the last one
        LSQ_TRY(ix->nrm_x.ensure(sizeof(uint32_t) * (size_t)n));
        LSQ_TRY(ix->nrm_q.ensure(sizeof(uint32_t) * (size_t)nq));
        LSQ_TRY(ix->clock.begin(c->profile != 0));
        LSQ_TRY(ix->clock.mark(s));
        LSQ_TRY(lsq_knn_launch_norms_u8(s, static_cast<const uint8_t *>(ix->base), ix->ldb, n, d, ix->nrm_x.as<uint32_t>()));
        LSQ_TRY(lsq_knn_launch_norms_u8(s, static_cast<const uint8_t *>(dq), ldq, nq, d, ix->nrm_q.as<uint32_t>()));
        LSQ_TRY(ix->clock.mark(s));
        float ms[2];
        LSQ_TRY(ix->clock.read(ms));
        info.norms_ms = ms[0];
        in.xnorms = ix->nrm_x.as<uint32_t>();
        in.qnorms = ix->nrm_q.as<uint32_t>();
    }
    lsq_linscan_stats st{};
    int road = 0;
    index_apply_filter(ix, &in, &road, 8);
    lsq_filter_note_road(ix->filter, road);
    LSQ_TRY(lsq_adc_search(s, &ix->adc, call.out_d, call.out_i, in, nq, nn, search_opts(c, &st)));
    LSQ_TRY(call.finish());
    info.queries = nq; info.rows = n; info.batches = st.batches; info.fallback_queries = st.fallback_queries; info.exhaustive = st.exhaustive;
    info.int_road = int_road ? 1 : 0;
    info.scan_ms = st.sample_ms + st.scan_ms; info.select_ms = st.select_ms;
    ix->knn = info;
    return LSQ_OK;
}

extern "C" int lsq_index_get_knn_info(lsq_index *ix, lsq_index_knn_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_knn_info: null argument"); return LSQ_EINVAL; }
    *out = ix->knn;
    return LSQ_OK;
}

extern "C" int lsq_index_get_stats(lsq_index *ix, lsq_index_stats *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_stats: null argument"); return LSQ_EINVAL; }
    *out = ix->stats;
    return LSQ_OK;
}

// the filter's bitmap in the order of the inverted layout: rebuilt whenever the lists or the filter change (a no-op while either is missing)
static int index_filter_layout(lsq_index *ix) {
    if (!ix->filter) return LSQ_OK;
    const int *ids = nullptr, *off = nullptr;
    lsq_ivf_layout(ix->ivf, &ids, &off);
    return lsq_filter_layout(ix->ctx->stream, ix->filter, ids, off, ix->n, lsq_ivf_nlist(ix->ivf));
}

// ---- inverted lists on the index (lsq_ivf.hip): the layout, then a search over each query's probed lists with stage two behind it ----------------------
extern "C" int lsq_index_set_lists(lsq_index *ix, const lsq_ivf_desc *desc) {
    if (!ix || !desc) { lsq_set_error("lsq_index_set_lists: null %s", ix ? "description" : "index"); return LSQ_EINVAL; }
    if (!ix->codes) { lsq_set_error("lsq_index_set_lists: the index holds no codes"); return LSQ_EINVAL; }
    if (desc->nlist < 1 || desc->nlist > (1 << 24)) { lsq_set_error("lsq_index_set_lists: needs 1 <= nlist <= 2^24 (got %d)", desc->nlist); return LSQ_EINVAL; }
    if (!desc->centroids || !desc->list_of_row) { lsq_set_error("lsq_index_set_lists: null pointer"); return LSQ_EINVAL; }
    LSQ_TRY(use_device(ix->ctx));
    ix->r_lor_valid = false;
    LSQ_TRY(lsq_ivf_set_lists(ix->ctx->stream, &ix->ivf, ix->codes, ix->norms, ix->packed, ix->n, ix->m, ix->d, desc));
    lsq_range_drop(ix->range);
    if (ix->cap_rows > ix->n) {                       // an index with capacity (lsq_index_reserve / _add): the layout's halves get it too
        int moved = 0;
        LSQ_TRY(lsq_ivf_reserve(ix->ctx->stream, ix->ivf, ix->cap_rows, &moved));
    }
    return index_filter_layout(ix);                   // a filter's layout-order bits follow the new lists
}

extern "C" int lsq_index_search_ivf(lsq_index *ix, float *dists, int *ids, const float *q_scan, const float *q_coarse, const float *q_exact, int nq, int ldq,
                                    int nprobe, int shortlist, int nn, int flags, int on_device) {
    LSQ_TRY(index_call_check("lsq_index_search_ivf", ix, dists, ids, nq, ldq, nn));
    if (!ix->codes) { lsq_set_error("lsq_index_search_ivf: the index holds no codes"); return LSQ_EINVAL; }
    const int nlist = lsq_ivf_nlist(ix->ivf);
    if (nlist < 1) { lsq_set_error("lsq_index_search_ivf: the index has no lists (call lsq_index_set_lists first)"); return LSQ_EINVAL; }
    if (flags & ~(LSQ_IVF_ADD_COARSE | LSQ_IVF_EVERY_RECORD | LSQ_IVF_TEST_BATCH)) { lsq_set_error("lsq_index_search_ivf: unknown flags %d", flags); return LSQ_EINVAL; }
    if (nprobe < 1 || nprobe > nlist) { lsq_set_error("lsq_index_search_ivf: needs 1 <= nprobe <= nlist (got nprobe=%d nlist=%d)", nprobe, nlist); return LSQ_EINVAL; }
    int L = 0;
    LSQ_TRY(index_shortlist("lsq_index_search_ivf", shortlist, nn, &L));
    if (L > (1 << 28)) { lsq_set_error("lsq_index_search_ivf: needs nn and shortlist <= 2^28 (got %d)", L); return LSQ_EINVAL; }
    lsq_ctx *c = ix->ctx;
    IndexCall call{ix, nq, on_device != 0};
    return index_two_stage("lsq_index_search_ivf", call, dists, ids, q_scan, q_exact, ldq, shortlist, nn, L,
                           [&](float *scan_d, int *scan_i, const float *dqs, int len) -> int {      // the scan of each query's probed lists
        const float *dqc = nullptr;                   // the coarse search reads rows as they lie
        int64_t ldc = 0;
        LSQ_TRY(call.rows(ix->s_qcoarse, q_coarse ? q_coarse : q_scan, sizeof(float), ldq, ix->d, false, !on_device, &dqc, &ldc));
        if (!lsq_filter_active(ix->filter))
            return lsq_ivf_search(c->stream, ix->ivf, &ix->adc, ix->K, scan_d, scan_i, dqs, dqc, ldc, nq, nprobe, len, flags, c->search, c->profile);
        // under a filter: the inverted layout is read as it lies, with the filter's bits in layout order (the dense road; the layout has no compact form)
        const lsq_filter_view v = lsq_filter_get(ix->filter);
        if (!v.lbits) { lsq_set_error("lsq_index_search_ivf: the filter has no bits in layout order (a failed lsq_index_set_lists / _set_filter?)"); return LSQ_EINVAL; }
        lsq_filter_note_road(ix->filter, 1);
        return lsq_ivf_search(c->stream, ix->ivf, &ix->adc, ix->K, scan_d, scan_i, dqs, dqc, ldc, nq, nprobe, len, flags, c->search, c->profile, &v);
    });
}

extern "C" int lsq_index_get_ivf_info(lsq_index *ix, lsq_ivf_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_ivf_info: null argument"); return LSQ_EINVAL; }
    lsq_ivf_get_info(ix->ivf, out);
    return LSQ_OK;
}

// ---- range search on the index (lsq_range.hip): every candidate row within a radius; the result is HELD by the index until fetched or dropped ----
extern "C" int lsq_index_range_search(lsq_index *ix, int64_t *lims, const float *q_scan, const float *q_coarse, const float *radius, int nq, int ldq,
                                      int nprobe, int flags, int on_device) {
    const char *fn = "lsq_index_range_search";
    if (!ix) { lsq_set_error("%s: null index", fn); return LSQ_EINVAL; }
    const int nlist = lsq_ivf_nlist(ix->ivf);
    if (const char *why = lsq_range_refusal(lims, q_scan, radius, ix->codes != nullptr, nlist, ix->d, nq, ldq, nprobe, flags)) {
        lsq_set_error("%s: %s (nq=%d ldq=%d d=%d nprobe=%d nlist=%d flags=%d)", fn, why, nq, ldq, ix->d, nprobe, nlist, flags);
        return LSQ_EINVAL;
    }
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    const bool dev = on_device != 0;
    lsq_range_call call;
    call.nq = nq; call.nprobe = nprobe; call.flags = flags;
    call.budget = lsq_range_budget(c->range_batch);
    call.timed = c->profile ? 1 : 0;
    call.in = lsq_input(ix->codes, nullptr, ix->K, ix->norms, (int)ix->n, ix->m, ix->d);
    if (ix->packed) { call.in.packed = 1; call.in.cstride = ix->m + 1; }      // rows with their norm byte; norms is the table
    const bool filtered = lsq_filter_active(ix->filter);
    if (nprobe == 0) {
        // the filter's road: compact when forced, or when at most half of the rows are allowed.  The selection-cost band of lsq_filter_compact_by_default
        // does not apply: nothing is selected here, the walk is all there is
        if (filtered) {
            const lsq_filter_view v = lsq_filter_get(ix->filter);
            const bool compact = v.force == LSQ_FILTER_FORCE_COMPACT || (v.force == 0 && v.allowed <= lsq_filter_crossover(ix->n));
            if (compact) { call.in.filter_rows = v.rows; call.in.filter_count = (int)v.allowed; }
            else call.in.filter_bits = v.bits;
            call.road = compact ? 2 : 1;
        }
    } else {
        if (filtered) {
            const lsq_filter_view v = lsq_filter_get(ix->filter);
            if (!v.lbits) { lsq_set_error("%s: the filter has no bits in layout order (a failed lsq_index_set_lists / _set_filter?)", fn); return LSQ_EINVAL; }
            call.lbits = v.lbits;
            call.road = 1;
        }
        call.ivf = ix->ivf; call.adc = &ix->adc; call.coarse = c->search;
    }
    std::vector<int64_t> staged;
    int64_t *h_lims = lims;
    if (dev) { staged.resize((size_t)nq + 1); h_lims = staged.data(); call.lims_dev = lims; }
    if (nq > 0) {
        // the scan reads query rows d floats apart, the coarse search rows as they lie; the host form stages both, and the radii
        IndexCall rows{ix, nq, dev};
        const float *dqs = nullptr, *dqc = nullptr, *drad = nullptr;
        int64_t ld = 0, ldc = 0, ldr = 0;
        LSQ_TRY(rows.rows(ix->s_qscan, q_scan, sizeof(float), ldq, ix->d, true, !dev || ldq != ix->d, &dqs, &ld));
        if (nprobe >= 1) LSQ_TRY(rows.rows(ix->s_qcoarse, q_coarse ? q_coarse : q_scan, sizeof(float), ldq, ix->d, false, !dev, &dqc, &ldc));
        LSQ_TRY(rows.rows(ix->s_radius, radius, sizeof(float), 1, 1, false, !dev, &drad, &ldr));
        call.in.Q = dqs; call.in.qstride = ix->d;
        call.q_coarse = dqc; call.ldc = ldc; call.radius = drad;
    }
    lsq_filter_note_road(ix->filter, call.road);
    LSQ_TRY(lsq_range_search(s, &ix->range, call, h_lims));
    ix->stats.queries += nq;
    return LSQ_OK;
}

extern "C" int lsq_index_range_fetch(lsq_index *ix, float *dists, int *ids, int64_t capacity, int on_device) {
    if (!ix) { lsq_set_error("lsq_index_range_fetch: null index"); return LSQ_EINVAL; }
    LSQ_TRY(use_device(ix->ctx));
    return lsq_range_fetch(ix->ctx->stream, ix->range, dists, ids, capacity, on_device);
}

extern "C" int lsq_index_get_range_info(lsq_index *ix, lsq_range_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_range_info: null argument"); return LSQ_EINVAL; }
    lsq_range_get_info(ix->range, out);
    return LSQ_OK;
}

// ---- row filters on the index (lsq_filter.hip): the allowed rows, owned; lsq_index_search, _search_ivf and _knn answer over them alone --------------------
extern "C" int lsq_index_set_filter(lsq_index *ix, const lsq_filter_desc *desc) {
    if (!ix) { lsq_set_error("lsq_index_set_filter: null index"); return LSQ_EINVAL; }
    if (!desc) { lsq_filter_clear(ix->filter); lsq_range_drop(ix->range); return LSQ_OK; }
    LSQ_TRY(use_device(ix->ctx));
    LSQ_TRY(lsq_filter_set(ix->ctx->stream, &ix->filter, ix->n, desc));
    lsq_range_drop(ix->range);
    return index_filter_layout(ix);
}

extern "C" int lsq_index_get_filter_info(lsq_index *ix, lsq_filter_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_filter_info: null argument"); return LSQ_EINVAL; }
    lsq_filter_get_info(ix->filter, ix->n, out);
    return LSQ_OK;
}

// ---- appending rows (lsq_grow.hip): the flat arrays in owned storage with capacity, the inverted layout merged, the filter extended ---------
// What depends on n, and what an add does about it: ix->n (committed last); the flat arrays (appended past n, invisible until then); lsq_ivf_state's
// layout, off and n (merged into the spare half, swapped at the commit); lsq_filter_state's bits / prefix / rows / n (rebuilt beside the one in force,
// swapped) and its layout-order bits (lsq_filter_layout again); the scan state's sample and record buffers, stage two's records, nrm_x and every staging
// buffer are sized from the call's own n at every call (DevBuf::ensure) and hold nothing across calls; idbits and the selection's road are computed per call
static size_t index_row_bytes(const lsq_index *ix) { return (size_t)(ix->packed ? ix->m + 1 : ix->m); }
static size_t index_base_elem(const lsq_index *ix) { return lsq_base_elem_bytes(ix->base_u8); }      // 4, 1 or 2
static bool index_borrows(const lsq_index *ix) {
    return (ix->codes && ix->codes != ix->own_codes.p) || (ix->codes && !ix->packed && ix->norms != ix->own_norms.p) || (ix->base && ix->base != ix->own_base.p);
}

// the flat arrays in owned storage that holds `cap` rows: borrowed ones are adopted (copied once), owned ones that are too small move with their contents
static int index_capacity(lsq_index *ix, int64_t cap, int *moved) {
    hipStream_t s = ix->ctx->stream;
    const size_t n = (size_t)ix->n, rowb = index_row_bytes(ix);
    const bool borrowed = index_borrows(ix);
    const size_t before[3] = {ix->own_codes.cap, ix->own_norms.cap, ix->own_base.cap};
    if (ix->codes) {
        LSQ_TRY(lsq_devbuf_grow(s, ix->own_codes, (size_t)cap * rowb + 16, n * rowb, ix->codes));      // 16 bytes of slack past the last row, never read
        ix->codes = ix->own_codes.as<uint8_t>();
        if (!ix->packed) {
            LSQ_TRY(lsq_devbuf_grow(s, ix->own_norms, sizeof(float) * (size_t)cap, sizeof(float) * n, ix->norms));
            ix->norms = ix->own_norms.as<float>();
        }
    }
    if (ix->base) {
        const size_t e = index_base_elem(ix);
        LSQ_TRY(lsq_devbuf_grow(s, ix->own_base, (size_t)cap * (size_t)ix->ldb * e, ((n - 1) * (size_t)ix->ldb + (size_t)ix->d) * e, ix->base));
        ix->base = ix->own_base.p;
    }
    if (before[0] != ix->own_codes.cap || before[1] != ix->own_norms.cap || before[2] != ix->own_base.cap) *moved = 1;
    if (borrowed) ix->grow.adopted = 1;
    if (cap > ix->cap_rows) ix->cap_rows = cap;
    return LSQ_OK;
}

static lsq_grow_shape index_shape(const lsq_index *ix) {
    lsq_grow_shape sh{};
    sh.n = ix->n; sh.d = ix->d; sh.has_codes = ix->codes != nullptr; sh.has_base = ix->base != nullptr; sh.packed = ix->packed; sh.base_u8 = ix->base_u8;
    sh.has_lists = lsq_ivf_nlist(ix->ivf) > 0;
    return sh;
}

extern "C" int lsq_index_reserve(lsq_index *ix, int64_t rows) {
    if (!ix) { lsq_set_error("lsq_index_reserve: null index"); return LSQ_EINVAL; }
    if (const char *why = lsq_grow_reserve_refusal(ix->n, rows)) { lsq_set_error("lsq_index_reserve: %s (rows=%lld n=%lld)", why, (long long)rows, (long long)ix->n); return LSQ_EINVAL; }
    LSQ_TRY(use_device(ix->ctx));
    const int64_t cap = rows > ix->cap_rows ? rows : ix->cap_rows;
    int moved = 0;
    LSQ_TRY(index_capacity(ix, cap, &moved));
    LSQ_TRY(lsq_ivf_reserve(ix->ctx->stream, ix->ivf, cap, &moved));
    LSQ_HIP(hipStreamSynchronize(ix->ctx->stream));
    ix->grow.reallocations += moved;
    return LSQ_OK;
}

extern "C" int lsq_index_add(lsq_index *ix, const lsq_index_add_desc *desc) {
    const char *fn = "lsq_index_add";
    if (!ix) { lsq_set_error("%s: null index", fn); return LSQ_EINVAL; }
    if (const char *why = lsq_grow_add_refusal(index_shape(ix), desc)) { lsq_set_error("%s: %s", fn, why); return LSQ_EINVAL; }
    if (desc->count == 0) return LSQ_OK;
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    const int64_t n = ix->n, count = desc->count;
    const size_t rowb = index_row_bytes(ix), m = (size_t)ix->m;
    const bool lists = lsq_ivf_nlist(ix->ivf) > 0;
    const hipMemcpyKind kind = desc->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    // 1. the range checks, on the device, by the kernels that read the entries: nothing of the index has been written when either refuses
    if (lists) {
        unsigned bad = 0;
        LSQ_TRY(lsq_ivf_add_check(s, ix->ivf, desc->list_of_row, desc->on_device, count, &bad));
        if (bad) { lsq_set_error("%s: %u entries of list_of_row lie outside [0, %d)", fn, bad, lsq_ivf_nlist(ix->ivf)); return LSQ_EINVAL; }
    }
    if (ix->packed) {                                 // the new rows through create_packed's interleave and norm-byte check, into scratch
        const uint8_t *dcodes = desc->codes, *dnc = desc->norm_codes;
        if (!desc->on_device) {
            LSQ_TRY(ix->g_codes.ensure((size_t)count * m));
            LSQ_TRY(ix->g_nc.ensure((size_t)count));
            LSQ_HIP(hipMemcpyAsync(ix->g_codes.p, desc->codes, (size_t)count * m, hipMemcpyHostToDevice, s));
            LSQ_HIP(hipMemcpyAsync(ix->g_nc.p, desc->norm_codes, (size_t)count, hipMemcpyHostToDevice, s));
            dcodes = ix->g_codes.as<uint8_t>(); dnc = ix->g_nc.as<uint8_t>();
        }
        LSQ_TRY(ix->g_rows.ensure((size_t)count * rowb));
        LSQ_HIP(hipMemsetAsync(ix->counter.p, 0, sizeof(unsigned long long), s));
        LSQ_TRY(lsq_adc_launch_pack(s, dcodes, dnc, count, ix->m, ix->ncb, ix->g_rows.as<uint8_t>(), ix->counter.as<unsigned>()));
        unsigned bad = 0;
        LSQ_HIP(hipMemcpyAsync(&bad, ix->counter.p, sizeof(bad), hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
        if (bad) { lsq_set_error("%s: %u norm bytes lie outside [0, %d)", fn, bad, ix->ncb); return LSQ_EINVAL; }
    }
    // 2. capacity (and adoption): the answers do not depend on where the arrays lie
    int moved = 0;
    const int64_t cap = n + count > ix->cap_rows ? lsq_grow_capacity(ix->cap_rows, n + count) : ix->cap_rows;
    LSQ_TRY(index_capacity(ix, cap, &moved));
    LSQ_TRY(ix->gclock.begin(c->profile != 0));
    LSQ_TRY(ix->gclock.mark(s));
    // 3. the flat arrays, past row n: not part of the index until n moves
    if (ix->codes) {
        uint8_t *at = ix->own_codes.as<uint8_t>() + (size_t)n * rowb;
        if (ix->packed) LSQ_HIP(hipMemcpyAsync(at, ix->g_rows.p, (size_t)count * rowb, hipMemcpyDeviceToDevice, s));
        else {
            LSQ_HIP(hipMemcpyAsync(at, desc->codes, (size_t)count * rowb, kind, s));
            LSQ_HIP(hipMemcpyAsync(ix->own_norms.as<float>() + n, desc->dbnorms, sizeof(float) * (size_t)count, kind, s));
        }
    }
    if (ix->base) {                                   // re-pitched on the way in: the owned base keeps the index's pitch
        const size_t e = index_base_elem(ix);
        LSQ_HIP(hipMemcpy2DAsync(static_cast<char *>(ix->own_base.p) + (size_t)n * (size_t)ix->ldb * e, (size_t)ix->ldb * e, desc->base, (size_t)desc->ldb * e,
                                 (size_t)ix->d * e, (size_t)count, kind, s));
    }
    LSQ_TRY(ix->gclock.mark(s));
    // 4. the inverted layout, merged into its spare half; 5. the filter, rebuilt beside the one in force
    if (lists)
        LSQ_TRY(lsq_ivf_add_merge(s, ix->ivf, ix->own_codes.as<uint8_t>() + (size_t)n * rowb, ix->packed ? nullptr : ix->own_norms.as<float>() + n, count, cap, &moved));
    LSQ_TRY(ix->gclock.mark(s));
    LSQ_TRY(lsq_filter_grow(s, ix->filter, n + count));
    LSQ_TRY(ix->gclock.mark(s));
    LSQ_HIP(hipStreamSynchronize(s));
    // 6. the commit
    if (lists) lsq_ivf_add_commit(ix->ivf, count);
    ix->r_lor_valid = false;
    lsq_filter_grow_commit(ix->filter, n + count);
    ix->n = n + count;
    lsq_range_drop(ix->range);                        // a held range result answers for the former rows
    float ms[3];
    LSQ_TRY(ix->gclock.read(ms));
    ix->grow.adds += 1; ix->grow.rows_added += count; ix->grow.reallocations += moved;
    ix->grow.merged_rows = lists ? n + count : 0;
    ix->grow.append_ms = ms[0]; ix->grow.merge_ms = ms[1]; ix->grow.filter_ms = ms[2];
    if (lists && moved) {                             // the half that was the layout is smaller than the new one: sized now (nothing to keep), so that the
        int again = 0;                                // adds that fit the capacity allocate nothing.  A failure here costs nothing: the next add asks again
        (void)lsq_ivf_reserve(s, ix->ivf, cap, &again);
    }
    return index_filter_layout(ix);                   // the filter's layout-order bits follow the new layout
}

extern "C" int lsq_index_get_growth_info(lsq_index *ix, lsq_index_growth_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_growth_info: null argument"); return LSQ_EINVAL; }
    *out = ix->grow;
    out->n = ix->n; out->capacity_rows = ix->cap_rows;
    return LSQ_OK;
}

// ---- removing rows (lsq_filter.hip: the tombstones; lsq_compact.hip: the rows leave) ----------------------------------------------------------
extern "C" int lsq_index_remove(lsq_index *ix, const int32_t *ids, int64_t count, int id_base, int on_device) {
    const char *fn = "lsq_index_remove";
    if (!ix) { lsq_set_error("%s: null index", fn); return LSQ_EINVAL; }
    if (const char *why = lsq_compact_remove_refusal(ids, count, id_base)) { lsq_set_error("%s: %s (count=%lld id_base=%d)", fn, why, (long long)count, id_base); return LSQ_EINVAL; }
    if (count == 0) return LSQ_OK;                    // a no-op: no filter is created
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    LSQ_TRY(ix->cclock.begin(c->profile != 0));
    LSQ_TRY(ix->cclock.mark(s));
    unsigned bad = 0;
    int64_t cleared = 0;
    LSQ_TRY(lsq_filter_remove(s, &ix->filter, ix->n, ids, count, id_base, on_device, &bad, &cleared));
    if (bad) { lsq_set_error("%s: %u ids lie outside [%d, %lld)", fn, bad, id_base, (long long)(id_base + ix->n)); return LSQ_EINVAL; }
    lsq_range_drop(ix->range);
    const int rc = index_filter_layout(ix);           // the layout-order bits follow the new filter
    LSQ_TRY(ix->cclock.mark(s));
    float ms[2];
    LSQ_TRY(ix->cclock.read(ms));
    ix->cinfo.removes += 1; ix->cinfo.rows_tombstoned += cleared; ix->cinfo.tombstone_ms = ms[0];
    return rc;
}

namespace {
struct ScopedBuf {                                     // a buffer of one call: what it holds when the call ends is freed (after a commit: the former array)
    DevBuf b;
    ~ScopedBuf() { b.release(); }
};
}  // namespace

// What depends on n, for a SHRINKING n (the audit of lsq_index_add, again): ix->n, cap_rows and the flat pointers (committed last, the arrays written
// beside); lsq_ivf_state's layout, off and n (written into the spare half, swapped at the commit); lsq_filter_state (cleared: the survivors are all
// allowed; its layout-order state reset); grow.n (read from ix->n); nrm_x, the scan state's buffers, stage two's records and every staging buffer are
// sized from the call's own n at every call and hold nothing across calls -- a smaller n finds them large enough
extern "C" int lsq_index_compact(lsq_index *ix, const lsq_index_compact_desc *desc) {
    const char *fn = "lsq_index_compact";
    if (!ix) { lsq_set_error("%s: null index", fn); return LSQ_EINVAL; }
    if (const char *why = lsq_compact_refusal(desc)) { lsq_set_error("%s: %s (flags=%d id_base=%d)", fn, why, desc->flags, desc->id_base); return LSQ_EINVAL; }
    const bool active = lsq_filter_active(ix->filter);
    const lsq_filter_view v = lsq_filter_get(ix->filter);
    if (const char *why = lsq_compact_allowed_refusal(active, v.allowed)) { lsq_set_error("%s: %s", fn, why); return LSQ_EINVAL; }
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    const int flags = desc ? desc->flags : 0, id_base = desc ? desc->id_base : 0;
    const bool shrink = (flags & LSQ_COMPACT_SHRINK) != 0, lists = lsq_ivf_nlist(ix->ivf) > 0;
    const int64_t n = ix->n, n2 = active ? v.allowed : n;
    const int64_t cap = lsq_compact_capacity(ix->cap_rows, n2, flags);
    const size_t rowb = index_row_bytes(ix), e = index_base_elem(ix);
    if (active && lists && !v.lbits) { lsq_set_error("%s: the filter has no bits in layout order (a failed lsq_index_set_lists / _set_filter?)", fn); return LSQ_EINVAL; }
    // the caller's maps: written on the device, into the caller's arrays or into scratch that is copied out
    int32_t *h_old = desc ? desc->old_of_new : nullptr, *h_new = desc ? desc->new_of_old : nullptr;
    int32_t *d_old = h_old, *d_new = h_new;
    const bool host_maps = desc && !desc->on_device;
    if (host_maps && h_old) { LSQ_TRY(ix->c_old.ensure(sizeof(int32_t) * (size_t)n2)); d_old = ix->c_old.as<int32_t>(); }
    if (host_maps && h_new) { LSQ_TRY(ix->c_new.ensure(sizeof(int32_t) * (size_t)n)); d_new = ix->c_new.as<int32_t>(); }
    auto maps = [&]() -> int {
        LSQ_TRY(lsq_compact_launch_maps(s, active ? v.bits : nullptr, v.pre, v.rows, n, n2, id_base, d_old, d_new));
        if (host_maps && h_old) LSQ_HIP(hipMemcpyAsync(h_old, d_old, sizeof(int32_t) * (size_t)n2, hipMemcpyDeviceToHost, s));
        if (host_maps && h_new) LSQ_HIP(hipMemcpyAsync(h_new, d_new, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        return LSQ_OK;
    };
    int64_t bytes = 0, shrunk = 0;
    float ms[2] = {0.0f, 0.0f};
    if (!active) {                                    // nothing leaves.  LSQ_COMPACT_SHRINK: owned storage with spare capacity is re-allocated to n rows
        if (shrink && ix->cap_rows > n && !index_borrows(ix)) {      // (each array: allocate, copy, swap, free -- the same rows wherever they lie)
            if (ix->codes) {
                LSQ_TRY(lsq_devbuf_fit(s, ix->own_codes, (size_t)n * rowb + 16, (size_t)n * rowb));
                ix->codes = ix->own_codes.as<uint8_t>();
                if (!ix->packed) {
                    LSQ_TRY(lsq_devbuf_fit(s, ix->own_norms, sizeof(float) * (size_t)n, sizeof(float) * (size_t)n));
                    ix->norms = ix->own_norms.as<float>();
                }
            }
            if (ix->base) {
                LSQ_TRY(lsq_devbuf_fit(s, ix->own_base, (size_t)n * (size_t)ix->ldb * e, ((size_t)(n - 1) * (size_t)ix->ldb + (size_t)ix->d) * e));
                ix->base = ix->own_base.p;
            }
            LSQ_TRY(lsq_ivf_fit(s, ix->ivf, n));
            ix->cap_rows = n;
            shrunk = 1;
        }
        LSQ_TRY(maps());
        LSQ_HIP(hipStreamSynchronize(s));
    } else {
        // 1. the flat arrays, gathered into fresh storage of `cap` rows: straight from the caller's arrays where the index borrows them
        ScopedBuf codes, norms, base;
        LSQ_TRY(ix->cclock.begin(c->profile != 0));
        LSQ_TRY(ix->cclock.mark(s));
        if (ix->codes) {
            LSQ_TRY(codes.b.ensure((size_t)cap * rowb + 16));       // 16 bytes of slack past the last row, never read
            LSQ_TRY(lsq_compact_launch_gather(s, ix->codes, codes.b.p, v.rows, (int64_t)rowb, n2, (int64_t)rowb, &bytes));
            if (!ix->packed) {
                LSQ_TRY(norms.b.ensure(sizeof(float) * (size_t)cap));
                LSQ_TRY(lsq_compact_launch_gather(s, ix->norms, norms.b.p, v.rows, 4, n2, 4, &bytes));
            }
        }
        if (ix->base) {                               // the pitch is kept; the last row ends at its d-th element, in the source as in the copy
            LSQ_TRY(base.b.ensure((size_t)cap * (size_t)ix->ldb * e));
            LSQ_TRY(lsq_compact_launch_gather(s, ix->base, base.b.p, v.rows, (int64_t)((size_t)ix->ldb * e), n2, (int64_t)((size_t)ix->d * e), &bytes));
        }
        LSQ_TRY(ix->cclock.mark(s));
        // 2. the inverted layout, into its spare half
        if (lists) {
            const int *lsel = nullptr;
            LSQ_TRY(lsq_filter_layout_rows(s, ix->filter, n, &lsel));
            LSQ_TRY(lsq_ivf_compact(s, ix->ivf, v, lsel, n2, cap, shrink, &bytes));
        }
        LSQ_TRY(ix->cclock.mark(s));
        LSQ_TRY(maps());
        LSQ_HIP(hipStreamSynchronize(s));             // the one wait: everything is written, nothing is in force
        LSQ_TRY(ix->cclock.read(ms));
        // 3. the commit
        if (index_borrows(ix)) ix->grow.adopted = 1;
        if (ix->codes) {
            std::swap(ix->own_codes, codes.b);
            ix->codes = ix->own_codes.as<uint8_t>();
            if (!ix->packed) { std::swap(ix->own_norms, norms.b); ix->norms = ix->own_norms.as<float>(); }
        }
        if (ix->base) { std::swap(ix->own_base, base.b); ix->base = ix->own_base.p; }
        if (lists) lsq_ivf_compact_commit(ix->ivf, n2);
        lsq_filter_clear(ix->filter);                 // every surviving row is allowed
        ix->n = n2;
        ix->cap_rows = cap;
        (void)index_filter_layout(ix);                // (no filter: the layout-order state is reset, nothing is launched)
        if (lists && shrink) (void)lsq_ivf_fit(s, ix->ivf, n2);      // the half that was the layout.  A failure costs nothing: the next add sizes it
        shrunk = shrink ? 1 : 0;
    }
    lsq_range_drop(ix->range);
    ix->r_lor_valid = false;
    ix->cinfo.n_before = n; ix->cinfo.n_after = n2;
    ix->cinfo.compactions += 1; ix->cinfo.rows_dropped += n - n2;
    ix->cinfo.moved_bytes = bytes; ix->cinfo.shrunk = shrunk;
    ix->cinfo.gather_ms = ms[0]; ix->cinfo.layout_ms = ms[1];
    return LSQ_OK;
}

extern "C" int lsq_index_get_compact_info(lsq_index *ix, lsq_index_compact_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_compact_info: null argument"); return LSQ_EINVAL; }
    *out = ix->cinfo;
    return LSQ_OK;
}

// ---- half-precision base rows (lsq_half.hip): the resident f32 rows narrowed in place of themselves, and the stored rows read back ---------------
// What depends on the base rows' format, and what a narrowing does about it: ix->base, ldb, base_u8 (committed last, after the one wait, the new rows written
// beside the old); own_base (swapped: an owned f32 base is freed here, a borrowed one is the caller's); cap_rows (kept: the new rows are sized for it).  The
// scan state, stage two's records, nrm_x and every staging buffer are sized per call and hold nothing across calls; the integer road of lsq_index_knn asks for
// uint8 rows at every call
extern "C" int lsq_index_narrow_base(lsq_index *ix, int format) {
    const char *fn = "lsq_index_narrow_base";
    if (!ix) { lsq_set_error("%s: null index", fn); return LSQ_EINVAL; }
    if (const char *why = lsq_narrow_base_refusal(ix->base != nullptr, ix->base_u8, format)) { lsq_set_error("%s: %s (format=%d)", fn, why, format); return LSQ_EINVAL; }
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    const size_t rows = (size_t)(ix->cap_rows > ix->n ? ix->cap_rows : ix->n), d = (size_t)ix->d;
    ScopedBuf half;                                   // what it holds when the call ends is freed: the new rows after a failure, the former owned rows after the commit
    LSQ_TRY(half.b.ensure(rows * d * 2));
    LSQ_TRY(ix->h_counts.ensure(3 * sizeof(unsigned long long)));
    LSQ_HIP(hipMemsetAsync(ix->h_counts.p, 0, 3 * sizeof(unsigned long long), s));
    LSQ_TRY(ix->hclock.begin(c->profile != 0));
    LSQ_TRY(ix->hclock.mark(s));
    LSQ_TRY(lsq_half_launch_narrow(s, static_cast<const float *>(ix->base), ix->ldb, half.b.p, ix->n, ix->d, format, ix->h_counts.as<unsigned long long>()));
    LSQ_TRY(ix->hclock.mark(s));
    unsigned long long cnt[3] = {0, 0, 0};
    LSQ_HIP(hipMemcpyAsync(cnt, ix->h_counts.p, sizeof(cnt), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));                 // the one wait: everything is written, nothing is in force
    float ms[1];
    LSQ_TRY(ix->hclock.read(ms));
    std::swap(ix->own_base, half.b);                  // the commit
    ix->base = ix->own_base.p;
    ix->ldb = ix->d;
    ix->base_u8 = format;
    lsq_range_drop(ix->range);
    ix->hcounts.to_inf = (int64_t)cnt[0]; ix->hcounts.to_zero = (int64_t)cnt[1]; ix->hcounts.nans = (int64_t)cnt[2];
    ix->narrow_ms = ms[0];
    return LSQ_OK;
}

extern "C" int lsq_index_get_base(lsq_index *ix, float *out, int64_t start, int64_t count, int64_t ldo, int on_device) {
    const char *fn = "lsq_index_get_base";
    if (!ix) { lsq_set_error("%s: null index", fn); return LSQ_EINVAL; }
    if (const char *why = lsq_get_base_refusal(ix->base != nullptr, ix->n, ix->d, start, count, ldo, out)) {
        lsq_set_error("%s: %s (start=%lld count=%lld ldo=%lld n=%lld d=%d)", fn, why, (long long)start, (long long)count, (long long)ldo, (long long)ix->n, ix->d);
        return LSQ_EINVAL;
    }
    if (count == 0) return LSQ_OK;
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    const size_t e = index_base_elem(ix), d = (size_t)ix->d;
    const char *first = static_cast<const char *>(ix->base) + (size_t)start * (size_t)ix->ldb * e;
    if (ix->base_u8 == 0) {                           // f32 rows: a copy, each row's d floats
        LSQ_HIP(hipMemcpy2DAsync(out, sizeof(float) * (size_t)ldo, first, sizeof(float) * (size_t)ix->ldb, sizeof(float) * d, (size_t)count,
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
        return LSQ_OK;
    }
    if (on_device) {                                  // one launch, straight into the caller's rows
        LSQ_TRY(lsq_half_launch_widen(s, first, ix->base_u8, ix->ldb, out, ldo, count, ix->d));
        LSQ_HIP(hipStreamSynchronize(s));
        return LSQ_OK;
    }
    // host form: chunks of rows widened d floats apart into the index's staging (lsq_index_reconstruct's), each row's d floats copied out
    const int64_t rows = lsq_base_chunk_rows(count, ix->d, c->recon_chunk);
    LSQ_TRY(ix->r_out.ensure(sizeof(float) * (size_t)rows * d));
    for (int64_t r0 = 0; r0 < count; r0 += rows) {
        const int64_t cn = std::min<int64_t>(rows, count - r0);
        LSQ_TRY(lsq_half_launch_widen(s, first + (size_t)r0 * (size_t)ix->ldb * e, ix->base_u8, ix->ldb, ix->r_out.as<float>(), ix->d, cn, ix->d));
        LSQ_HIP(hipMemcpy2DAsync(out + r0 * ldo, sizeof(float) * (size_t)ldo, ix->r_out.p, sizeof(float) * d, sizeof(float) * d, (size_t)cn, hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));             // the staging is written again by the next chunk
    }
    return LSQ_OK;
}

extern "C" int lsq_index_get_base_info(lsq_index *ix, lsq_index_base_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_base_info: null argument"); return LSQ_EINVAL; }
    *out = lsq_index_base_info{};
    if (!ix->base) return LSQ_OK;
    out->format = ix->base_u8;
    out->elem_bytes = (int64_t)index_base_elem(ix);
    out->ldb = ix->ldb;
    out->owned = ix->base == ix->own_base.p ? 1 : 0;
    out->resident_bytes = ((ix->n - 1) * ix->ldb + ix->d) * (int64_t)index_base_elem(ix);
    out->to_inf = ix->hcounts.to_inf; out->to_zero = ix->hcounts.to_zero; out->nans = ix->hcounts.nans;
    out->narrow_ms = ix->narrow_ms;
    return LSQ_OK;
}

// ---- decode from the index's own codes, and search by stored row (lsq_recon.hip) -------------------------------------------------------------
// What both entry points share, after their own checks: the selection checked (a bad id without PAD: LSQ_EINVAL before anything is written anywhere), the
// row -> list map brought up to date, and `emit(call, r0, cn, &road)` called for chunks of at most `chunk` rows of the selection -- call: the decode of the
// chunk, its output left to emit.  ids: host (ids_dev = false: checked here, staged) or device (the one kernel that reads them counts the bad ones)
template <class Emit>
static int index_decode(const char *fn, lsq_index *ix, const int32_t *ids, bool ids_dev, int64_t start, int64_t count, int id_base, int flags, int64_t chunk,
                        Emit emit) {
    lsq_ctx *c = ix->ctx;
    hipStream_t s = c->stream;
    const bool coarse = (flags & LSQ_RECON_ADD_COARSE) != 0, pad = (flags & LSQ_RECON_PAD_NAN) != 0;
    const int32_t *d_ids = ids;
    int64_t bad = 0;
    if (ids && !ids_dev) {
        bad = lsq_recon_count_bad_ids(ids, count, id_base, ix->n);
        if (bad && !pad) { ix->rinfo.invalid = bad; lsq_set_error("%s: %lld ids lie outside [%d, %lld)", fn, (long long)bad, id_base, (long long)(id_base + ix->n)); return LSQ_EINVAL; }
        LSQ_TRY(ix->r_ids.ensure(sizeof(int32_t) * (size_t)count));
        LSQ_HIP(hipMemcpyAsync(ix->r_ids.p, ids, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, s));
        d_ids = ix->r_ids.as<int32_t>();
    } else if (ids) {
        unsigned found = 0;
        LSQ_HIP(hipMemsetAsync(ix->counter.p, 0, sizeof(unsigned long long), s));
        LSQ_TRY(lsq_recon_launch_check_ids(s, ids, count, id_base, ix->n, ix->counter.as<unsigned>()));
        LSQ_HIP(hipMemcpyAsync(&found, ix->counter.p, sizeof(found), hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
        bad = found;
        if (bad && !pad) { ix->rinfo.invalid = bad; lsq_set_error("%s: %lld ids lie outside [%d, %lld)", fn, (long long)bad, id_base, (long long)(id_base + ix->n)); return LSQ_EINVAL; }
    }
    LSQ_TRY(ix->rclock.begin(c->profile != 0));
    LSQ_TRY(ix->rclock.mark(s));
    int rebuilt = 0;
    if (coarse && !ix->r_lor_valid) {
        const int *lids = nullptr, *loff = nullptr;
        lsq_ivf_layout(ix->ivf, &lids, &loff);
        LSQ_TRY(ix->r_lor.ensure(sizeof(int32_t) * (size_t)ix->n));
        LSQ_TRY(lsq_recon_launch_lor(s, lids, loff, ix->n, lsq_ivf_nlist(ix->ivf), ix->r_lor.as<int32_t>()));
        ix->r_lor_valid = true;
        rebuilt = 1;
    }
    LSQ_TRY(ix->rclock.mark(s));
    lsq_recon_call r;
    r.codes = ix->codes; r.ldc = (int64_t)index_row_bytes(ix); r.K = ix->K; r.d = ix->d; r.m = ix->m; r.n = ix->n;
    r.id_base = id_base; r.pad_nan = pad ? 1 : 0;
    if (coarse) { r.cent = lsq_ivf_centroids(ix->ivf); r.lor = ix->r_lor.as<int32_t>(); r.nlist = lsq_ivf_nlist(ix->ivf); }
    int road = 0;
    for (int64_t r0 = 0; r0 < count; r0 += chunk) {
        const int64_t cn = std::min<int64_t>(chunk, count - r0);
        r.ids = d_ids ? d_ids + r0 : nullptr; r.start = start + r0; r.count = cn;
        LSQ_TRY(emit(r, r0, cn, &road));
    }
    LSQ_TRY(ix->rclock.mark(s));
    LSQ_HIP(hipStreamSynchronize(s));
    float ms[2];
    LSQ_TRY(ix->rclock.read(ms));
    ix->rinfo.rows = count - bad; ix->rinfo.invalid = bad; ix->rinfo.map_rebuilt = rebuilt; ix->rinfo.map_rebuilds += rebuilt; ix->rinfo.road = road;
    ix->rinfo.calls += 1; ix->rinfo.map_ms = ms[0]; ix->rinfo.decode_ms = ms[1];
    return LSQ_OK;
}

extern "C" int lsq_index_reconstruct(lsq_index *ix, float *out, int64_t ldo, const int32_t *ids, int64_t start, int64_t count, int id_base, int flags,
                                     int on_device) {
    const char *fn = "lsq_index_reconstruct";
    if (!ix) { lsq_set_error("%s: null index", fn); return LSQ_EINVAL; }
    if (!ix->codes) { lsq_set_error("%s: the index holds no codes", fn); return LSQ_EINVAL; }
    if (ldo < ix->d) { lsq_set_error("%s: needs ldo >= d (got ldo=%lld d=%d)", fn, (long long)ldo, ix->d); return LSQ_EINVAL; }
    if (const char *why = lsq_recon_select_refusal(ids, start, count, id_base, ix->n, flags, lsq_ivf_nlist(ix->ivf) > 0)) {
        lsq_set_error("%s: %s (start=%lld count=%lld id_base=%d flags=%d n=%lld)", fn, why, (long long)start, (long long)count, id_base, flags, (long long)ix->n);
        return LSQ_EINVAL;
    }
    if (count > 0 && !out) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (((uintptr_t)out & 3) != 0) { lsq_set_error("%s: out is not 4-byte aligned", fn); return LSQ_EINVAL; }
    if (count == 0) return LSQ_OK;
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    const int d = ix->d;
    if (on_device)                                    // one launch, straight into the caller's rows
        return index_decode(fn, ix, ids, true, ids ? 0 : start, count, id_base, flags, count, [&](lsq_recon_call &r, int64_t r0, int64_t cn, int *road) -> int {
            r.out = out + r0 * ldo; r.ldo = ldo;
            return lsq_recon_launch(s, r, road);
        });
    // host form: chunks of rows decoded d floats apart into the index's staging, each row's d floats copied out
    const int64_t rows = lsq_recon_chunk_rows(count, d, c->recon_chunk);
    LSQ_TRY(ix->r_out.ensure(sizeof(float) * (size_t)rows * d));
    return index_decode(fn, ix, ids, false, ids ? 0 : start, count, id_base, flags, rows, [&](lsq_recon_call &r, int64_t r0, int64_t cn, int *road) -> int {
        r.out = ix->r_out.as<float>(); r.ldo = d;
        LSQ_TRY(lsq_recon_launch(s, r, road));
        LSQ_HIP(hipMemcpy2DAsync(out + r0 * ldo, sizeof(float) * (size_t)ldo, ix->r_out.p, sizeof(float) * (size_t)d, sizeof(float) * (size_t)d, (size_t)cn,
                                 hipMemcpyDeviceToHost, s));
        return LSQ_OK;
    });
}

// searches whose queries are stored rows: the rows decoded into r_q, then the existing entry point on those queries -- their checks, roads and statistics
extern "C" int lsq_index_search_rows(lsq_index *ix, float *dists, int *ids_out, const int32_t *rows, int nq, int id_base, int nn, int nprobe, int flags,
                                     int on_device) {
    const char *fn = "lsq_index_search_rows";
    LSQ_TRY(index_call_check(fn, ix, dists, ids_out, nq, ix ? ix->d : 0, nn));
    if (!ix->codes) { lsq_set_error("%s: the index holds no codes", fn); return LSQ_EINVAL; }
    if (nprobe < 0) { lsq_set_error("%s: needs nprobe >= 0 (got %d)", fn, nprobe); return LSQ_EINVAL; }
    if (id_base != 0 && id_base != 1) { lsq_set_error("%s: id_base must be 0 or 1 (got %d)", fn, id_base); return LSQ_EINVAL; }
    if (nq > 0 && !rows) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    const int nlist = lsq_ivf_nlist(ix->ivf);
    // what the search behind it would refuse is refused here, before the decode: nothing is launched for a call that cannot be answered
    if (nprobe == 0) {
        if (flags != 0) { lsq_set_error("%s: flags %d need nprobe >= 1", fn, flags); return LSQ_EINVAL; }
        if (nn > ix->n) { lsq_set_error("%s: nn=%d exceeds the database size %lld", fn, nn, (long long)ix->n); return LSQ_EINVAL; }
    } else {
        if (nlist < 1) { lsq_set_error("%s: the index has no lists (call lsq_index_set_lists first)", fn); return LSQ_EINVAL; }
        if (flags & ~(LSQ_IVF_ADD_COARSE | LSQ_IVF_EVERY_RECORD | LSQ_IVF_TEST_BATCH)) { lsq_set_error("%s: unknown flags %d", fn, flags); return LSQ_EINVAL; }
        if (nprobe > nlist) { lsq_set_error("%s: needs nprobe <= nlist (got nprobe=%d nlist=%d)", fn, nprobe, nlist); return LSQ_EINVAL; }
        if (nn > (1 << 28)) { lsq_set_error("%s: needs nn <= 2^28 (got %d)", fn, nn); return LSQ_EINVAL; }
    }
    if (nq == 0) return LSQ_OK;
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    LSQ_TRY(ix->r_q.ensure(sizeof(float) * (size_t)nq * ix->d));
    const int rflags = (nprobe >= 1 && (flags & LSQ_IVF_ADD_COARSE)) ? LSQ_RECON_ADD_COARSE : 0;
    LSQ_TRY(index_decode(fn, ix, rows, on_device != 0, 0, nq, id_base, rflags, nq, [&](lsq_recon_call &r, int64_t r0, int64_t cn, int *road) -> int {
        r.out = ix->r_q.as<float>() + r0 * ix->d; r.ldo = ix->d;
        return lsq_recon_launch(s, r, road);
    }));
    // the queries are device rows; a host call's dists / ids_out are host arrays: the entry points below stage query rows by address (hipMemcpyDefault), so
    // the host form reads r_q as it would read the caller's rows
    const float *q = ix->r_q.as<float>();
    if (nprobe == 0) return lsq_index_search(ix, dists, ids_out, q, nullptr, nq, ix->d, 0, nn, on_device);
    return lsq_index_search_ivf(ix, dists, ids_out, q, q, nullptr, nq, ix->d, nprobe, 0, nn, flags, on_device);
}

extern "C" int lsq_index_get_recon_info(lsq_index *ix, lsq_index_recon_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_recon_info: null argument"); return LSQ_EINVAL; }
    *out = ix->rinfo;
    return LSQ_OK;
}

// ---- snapshots: save, load, export, digest (lsq_snapshot.hip, lsq_snapshot_check.h) -------------------------------------------------------------
// The logical state of an index as the sections of lsq_snapshot_check.h.  A section is either canonical where it lies in HBM (direct) or derived on the
// device, chunk by chunk, into a staging chunk (derive(off, len, dst): bytes [off, off + len) of the section's stream to dst; off a multiple of 64).
namespace {
struct SnapSection {
    const void *direct = nullptr;
    std::function<int(int64_t, int64_t, void *)> derive;
};

// Two pinned chunks with their events, the device staging chunk, the digest's partials and one accumulator per section.  Slot j & 1 serves chunk j: its
// events say when the device is done with the pinned chunk (and, under option "profile", how long each phase took)
struct SnapStage {
    hipStream_t s = nullptr;
    char *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2][4] = {};
    bool busy[2] = {false, false};
    DevBuf dstage, partials, acc;
    int64_t chunk = 0;
    bool timed = false, loading = false;
    lsq_snapshot_io_info info{};
    int open(lsq_ctx *c, bool load, bool pinned, bool derived) {
        s = c->stream; timed = c->profile != 0; loading = load;
        chunk = c->snapshot_chunk > 0 ? c->snapshot_chunk : LSQ_SNAP_CHUNK_DEFAULT;
        chunk = std::max<int64_t>(LSQ_SNAP_ALIGN, chunk / LSQ_SNAP_ALIGN * LSQ_SNAP_ALIGN);
        if (pinned) {
            for (char *&p : pin) LSQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&p), (size_t)chunk, hipHostMallocDefault));
            for (auto &slot : ev) for (hipEvent_t &e : slot) LSQ_HIP(hipEventCreate(&e));
        }
        LSQ_TRY(partials.ensure(sizeof(unsigned long long) * LSQ_SNAP_PARTIALS));
        LSQ_TRY(acc.ensure(sizeof(unsigned long long) * 16));
        LSQ_HIP(hipMemsetAsync(acc.p, 0, sizeof(unsigned long long) * 16, s));
        if (derived) LSQ_TRY(dstage.ensure((size_t)chunk));
        info = lsq_snapshot_io_info{};
        info.op = load ? 2 : 1; info.chunk_bytes = chunk; info.host_staging_bytes = pinned ? 2 * chunk : 0;
        return LSQ_OK;
    }
    unsigned long long *slot(int k) { return acc.as<unsigned long long>() + k; }
    int mark(int sl, int e) {
        if (timed || e == 3) LSQ_HIP(hipEventRecord(ev[sl][e], s));
        return LSQ_OK;
    }
    int wait(int sl) {                               // the device is done with pinned chunk sl
        if (!busy[sl]) return LSQ_OK;
        LSQ_HIP(hipEventSynchronize(ev[sl][3]));
        busy[sl] = false;
        if (timed) {
            float a = 0, b = 0, c = 0;
            LSQ_HIP(hipEventElapsedTime(&a, ev[sl][0], ev[sl][1]));
            LSQ_HIP(hipEventElapsedTime(&b, ev[sl][1], ev[sl][2]));
            LSQ_HIP(hipEventElapsedTime(&c, ev[sl][2], ev[sl][3]));
            if (loading) { info.copy_ms += a; info.digest_ms += b; }
            else { info.derive_ms += a; info.digest_ms += b; info.copy_ms += c; }
        }
        return LSQ_OK;
    }
    int digests(int count, uint64_t *out) {          // the accumulators read back; waits
        unsigned long long h[16] = {0};
        LSQ_HIP(hipMemcpyAsync(h, acc.p, sizeof(unsigned long long) * (size_t)count, hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < count; ++k) out[k] = h[k];
        return LSQ_OK;
    }
    ~SnapStage() {
        if (s) (void)hipStreamSynchronize(s);       // nothing in flight touches the chunks when they go
        for (char *p : pin) if (p) (void)hipHostFree(p);
        for (auto &slot : ev) for (hipEvent_t e : slot) if (e) (void)hipEventDestroy(e);
        dstage.release(); partials.release(); acc.release();
    }
};
double snap_ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
}  // namespace

static void index_snap_scalars(lsq_index *ix, lsq_snapshot_info *s) {
    *s = lsq_snapshot_info{};
    s->n = ix->n; s->d = ix->d;
    s->has_codes = ix->codes != nullptr; s->has_base = ix->base != nullptr;
    s->m = s->has_codes ? ix->m : 0; s->h = s->has_codes ? LSQ_H : 0;
    s->packed = ix->packed ? 1 : 0; s->ncb = ix->packed ? ix->ncb : 0;
    s->base_format = s->has_base ? ix->base_u8 : 0;
    s->nlist = lsq_ivf_nlist(ix->ivf);
    if (lsq_filter_active(ix->filter)) {
        const lsq_filter_view v = lsq_filter_get(ix->filter);
        s->filter_active = 1; s->filter_force = v.force & (LSQ_FILTER_FORCE_DENSE | LSQ_FILTER_FORCE_COMPACT); s->allowed = v.allowed;
    }
}

// bytes [off, off + len) of the DENSE stream of the base rows (pitch d) gathered from rows ldb elements apart: a ragged first row, whole rows, a ragged last
static int index_snap_dense_base(lsq_index *ix, int64_t off, int64_t len, void *dstv, hipMemcpyKind kind) {
    hipStream_t s = ix->ctx->stream;
    const int64_t e = (int64_t)index_base_elem(ix), rb = (int64_t)ix->d * e, pitch = ix->ldb * e;
    const char *base = static_cast<const char *>(ix->base);
    char *dst = static_cast<char *>(dstv);
    int64_t row = off / rb, left = len;
    const int64_t col = off - row * rb;
    if (col) {
        const int64_t take = std::min(rb - col, left);
        LSQ_HIP(hipMemcpyAsync(dst, base + row * pitch + col, (size_t)take, kind, s));
        dst += take; left -= take; ++row;
    }
    const int64_t whole = left / rb;
    if (whole) {
        LSQ_HIP(hipMemcpy2DAsync(dst, (size_t)rb, base + row * pitch, (size_t)pitch, (size_t)rb, (size_t)whole, kind, s));
        dst += whole * rb; left -= whole * rb; row += whole;
    }
    if (left) LSQ_HIP(hipMemcpyAsync(dst, base + row * pitch, (size_t)left, kind, s));
    return LSQ_OK;
}

// the sources of the planned sections.  lor: a buffer of the call that receives the row -> list map (LIST_OF_ROW has no canonical copy in HBM: the layout
// holds its inverse)
static int index_snap_sources(lsq_index *ix, const lsq_snapshot_info &s, DevBuf &lor, SnapSection *src, bool *derived) {
    hipStream_t st = ix->ctx->stream;
    *derived = false;
    for (int k = 0; k < (int)s.nsections; ++k) {
        SnapSection &sec = src[k];
        switch (s.sections[k].kind) {
        case LSQ_SNAP_CODEBOOKS: sec.direct = ix->K; break;
        case LSQ_SNAP_CODES:
            if (!ix->packed) sec.direct = ix->codes;
            else sec.derive = [ix, st](int64_t off, int64_t len, void *dst) { return lsq_snap_launch_unpack(st, ix->codes, ix->n, ix->m, static_cast<uint8_t *>(dst), off, len, nullptr, 0, 0); };
            break;
        case LSQ_SNAP_DBNORMS: sec.direct = ix->norms; break;
        case LSQ_SNAP_NORM_CODES:
            sec.derive = [ix, st](int64_t off, int64_t len, void *dst) { return lsq_snap_launch_unpack(st, ix->codes, ix->n, ix->m, nullptr, 0, 0, static_cast<uint8_t *>(dst), off, len); };
            break;
        case LSQ_SNAP_CBNORMS: sec.direct = ix->norms; break;         // the norm table: its first ncb floats
        case LSQ_SNAP_BASE:
            if (ix->ldb == ix->d) sec.direct = ix->base;
            else sec.derive = [ix](int64_t off, int64_t len, void *dst) { return index_snap_dense_base(ix, off, len, dst, hipMemcpyDeviceToDevice); };
            break;
        case LSQ_SNAP_CENTROIDS: sec.direct = lsq_ivf_centroids(ix->ivf); break;
        case LSQ_SNAP_LIST_OF_ROW: {
            const int *lids = nullptr, *loff = nullptr;
            lsq_ivf_layout(ix->ivf, &lids, &loff);
            LSQ_TRY(lor.ensure(sizeof(int32_t) * (size_t)ix->n));
            LSQ_TRY(lsq_recon_launch_lor(st, lids, loff, ix->n, (int)s.nlist, lor.as<int32_t>()));
            sec.direct = lor.p;
            break;
        }
        case LSQ_SNAP_FILTER_BITS: sec.direct = lsq_filter_get(ix->filter).bits; break;
        }
        if (sec.derive) *derived = true;
    }
    return LSQ_OK;
}

// one section through the stage: derived (or read where it lies), digested into accumulator k and -- with a file -- copied out chunk by chunk, the copy of
// chunk j + 1 under the write of chunk j
static int index_snap_stream(SnapStage &st, const SnapSection &sec, int k, int64_t bytes, FILE *f, const char *name) {
    const int64_t step = (!f && sec.direct) ? std::max<int64_t>(bytes, 1) : st.chunk;      // nothing to stage: one launch over the section where it lies
    const int64_t nchunks = (bytes + step - 1) / step;
    auto issue = [&](int64_t j) -> int {
        const int sl = (int)(j & 1);
        const int64_t off = j * step, len = std::min(step, bytes - off);
        if (f) LSQ_TRY(st.mark(sl, 0));
        const void *src = sec.direct ? static_cast<const char *>(sec.direct) + off : st.dstage.p;
        if (!sec.direct) LSQ_TRY(sec.derive(off, len, st.dstage.p));
        if (f) LSQ_TRY(st.mark(sl, 1));
        LSQ_TRY(lsq_snap_launch_digest(st.s, src, (uint64_t)len, (uint64_t)off / 4, st.partials.as<unsigned long long>(), st.slot(k)));
        if (f) {
            LSQ_TRY(st.mark(sl, 2));
            LSQ_HIP(hipMemcpyAsync(st.pin[sl], src, (size_t)len, hipMemcpyDeviceToHost, st.s));
            LSQ_TRY(st.mark(sl, 3));
            st.busy[sl] = true;
        }
        return LSQ_OK;
    };
    if (nchunks > 0) LSQ_TRY(issue(0));
    for (int64_t j = 0; j < nchunks; ++j) {
        if (j + 1 < nchunks) LSQ_TRY(issue(j + 1));
        if (!f) continue;
        const int sl = (int)(j & 1);
        const int64_t len = std::min(step, bytes - j * step);
        LSQ_TRY(st.wait(sl));
        const auto t0 = std::chrono::steady_clock::now();
        if (fwrite(st.pin[sl], 1, (size_t)len, f) != (size_t)len) { lsq_set_error("lsq_index_save: section %s: short write: %s", name, strerror(errno)); return LSQ_EIO; }
        st.info.file_ms += snap_ms_since(t0);
    }
    st.info.chunks += nchunks; st.info.bytes += bytes; st.info.sections += 1;
    return LSQ_OK;
}

extern "C" int lsq_index_save(lsq_index *ix, const char *path, int flags) {
    const char *fn = "lsq_index_save";
    if (!ix || !path) { lsq_set_error("%s: null %s", fn, ix ? "path" : "index"); return LSQ_EINVAL; }
    if (flags != 0) { lsq_set_error("%s: flags must be 0 (got %d)", fn, flags); return LSQ_EINVAL; }
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    const auto t_call = std::chrono::steady_clock::now();
    lsq_snapshot_info s;
    lsq_snap_error err;
    index_snap_scalars(ix, &s);
    if (!lsq_snap_plan(&s, &err)) { lsq_set_error("%s: %s", fn, err.text); return LSQ_EINVAL; }
    ScopedBuf lor;
    SnapSection src[LSQ_SNAP_MAX_SECTIONS];
    bool derived = false;
    SnapStage st;                                     // (declared before the file: it waits for the device before the chunks go)
    LSQ_TRY(index_snap_sources(ix, s, lor.b, src, &derived));
    LSQ_TRY(st.open(c, false, true, derived));
    lsq_snap_temp temp(path);
    lsq_snap_file out;
    out.f = fopen(temp.tmp.c_str(), "wb");
    if (!out.f) { lsq_set_error("%s: cannot open %s: %s", fn, temp.tmp.c_str(), strerror(errno)); return LSQ_EIO; }
    temp.made = true;
    std::vector<unsigned char> head((size_t)lsq_snap_table_end(s.nsections), 0);      // its place is kept: the digests are known last
    if (fwrite(head.data(), 1, head.size(), out.f) != head.size()) { lsq_set_error("%s: short write to %s: %s", fn, temp.tmp.c_str(), strerror(errno)); return LSQ_EIO; }
    int64_t at = (int64_t)head.size();
    for (int k = 0; k < (int)s.nsections; ++k) {
        const char *name = lsq_snap_kind_name(s.sections[k].kind);
        if (!lsq_snap_write_pad(out.f, at, s.sections[k].offset)) { lsq_set_error("%s: section %s: short write: %s", fn, name, strerror(errno)); return LSQ_EIO; }
        LSQ_TRY(index_snap_stream(st, src[k], k, s.sections[k].bytes, out.f, name));
        at = s.sections[k].offset + s.sections[k].bytes;
    }
    uint64_t dig[LSQ_SNAP_MAX_SECTIONS];
    LSQ_TRY(st.digests((int)s.nsections, dig));
    for (int k = 0; k < (int)s.nsections; ++k) s.sections[k].digest = dig[k];
    lsq_snap_encode(&s, &head);
    if (fseeko(out.f, 0, SEEK_SET) != 0 || fwrite(head.data(), 1, head.size(), out.f) != head.size() || out.close() != 0) {
        lsq_set_error("%s: cannot finish %s: %s", fn, temp.tmp.c_str(), strerror(errno));
        return LSQ_EIO;
    }
    if (!temp.commit()) { lsq_set_error("%s: cannot rename %s to %s: %s", fn, temp.tmp.c_str(), path, strerror(errno)); return LSQ_EIO; }
    st.info.bytes = s.file_bytes;
    st.info.total_ms = snap_ms_since(t_call);
    ix->sinfo = st.info;
    return LSQ_OK;
}

extern "C" int lsq_index_digest(lsq_index *ix, lsq_snapshot_info *out) {
    const char *fn = "lsq_index_digest";
    if (!ix || !out) { lsq_set_error("%s: null argument", fn); return LSQ_EINVAL; }
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    lsq_snapshot_info s;
    lsq_snap_error err;
    index_snap_scalars(ix, &s);
    if (!lsq_snap_plan(&s, &err)) { lsq_set_error("%s: %s", fn, err.text); return LSQ_EINVAL; }
    ScopedBuf lor;
    SnapSection src[LSQ_SNAP_MAX_SECTIONS];
    bool derived = false;
    SnapStage st;
    LSQ_TRY(index_snap_sources(ix, s, lor.b, src, &derived));
    LSQ_TRY(st.open(c, false, false, derived));
    for (int k = 0; k < (int)s.nsections; ++k) LSQ_TRY(index_snap_stream(st, src[k], k, s.sections[k].bytes, nullptr, ""));
    uint64_t dig[LSQ_SNAP_MAX_SECTIONS];
    LSQ_TRY(st.digests((int)s.nsections, dig));
    for (int k = 0; k < (int)s.nsections; ++k) s.sections[k].digest = dig[k];
    std::vector<unsigned char> head;
    lsq_snap_encode(&s, &head);                       // the header's own digest: that of the file a save would write
    *out = s;
    return LSQ_OK;
}

extern "C" int lsq_index_export(lsq_index *ix, lsq_snapshot_arrays *out, int on_device) {
    const char *fn = "lsq_index_export";
    if (!ix || !out) { lsq_set_error("%s: null argument", fn); return LSQ_EINVAL; }
    lsq_ctx *c = ix->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t stream = c->stream;
    lsq_snapshot_info s;
    lsq_snap_error err;
    index_snap_scalars(ix, &s);
    if (!lsq_snap_plan(&s, &err)) { lsq_set_error("%s: %s", fn, err.text); return LSQ_EINVAL; }
    for (int64_t kind = 1; kind <= LSQ_SNAP_MAX_SECTIONS; ++kind) {      // everything is refused before anything is written
        bool present = false;
        for (int k = 0; k < (int)s.nsections; ++k) present = present || s.sections[k].kind == kind;
        if (lsq_snap_array(out, kind) && !present) { lsq_set_error("%s: the index has no %s", fn, lsq_snap_kind_name(kind)); return LSQ_EINVAL; }
    }
    ScopedBuf lor, whole;                             // the host form of a derived section: derived whole on the device, then fetched
    SnapSection src[LSQ_SNAP_MAX_SECTIONS];
    bool derived = false;
    LSQ_TRY(index_snap_sources(ix, s, lor.b, src, &derived));
    int rc = LSQ_OK;
    for (int k = 0; rc == LSQ_OK && k < (int)s.nsections; ++k) {
        void *dst = lsq_snap_array(out, s.sections[k].kind);
        const int64_t bytes = s.sections[k].bytes;
        if (!dst) continue;
        auto copy = [&](const void *from) -> int {
            LSQ_HIP(hipMemcpyAsync(dst, from, (size_t)bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
            return LSQ_OK;
        };
        if (src[k].direct) rc = copy(src[k].direct);
        else if (on_device) rc = src[k].derive(0, bytes, dst);
        else if (s.sections[k].kind == LSQ_SNAP_BASE) rc = index_snap_dense_base(ix, 0, bytes, dst, hipMemcpyDeviceToHost);
        else {
            rc = whole.b.ensure((size_t)bytes);
            if (rc == LSQ_OK) rc = src[k].derive(0, bytes, whole.b.p);
            if (rc == LSQ_OK) rc = copy(whole.b.p);
            if (rc == LSQ_OK && hipStreamSynchronize(stream) != hipSuccess) { lsq_set_error("%s: the copy failed", fn); rc = LSQ_EHIP; }      // `whole` is written again
        }
    }
    if (hipStreamSynchronize(stream) != hipSuccess && rc == LSQ_OK) { lsq_set_error("%s: the copy failed", fn); rc = LSQ_EHIP; }
    if (rc != LSQ_OK) return rc;
    lsq_snap_scalars_out(&s, out);
    return LSQ_OK;
}

extern "C" int lsq_index_get_snapshot_info(lsq_index *ix, lsq_snapshot_io_info *out) {
    if (!ix || !out) { lsq_set_error("lsq_index_get_snapshot_info: null argument"); return LSQ_EINVAL; }
    *out = ix->sinfo;
    return LSQ_OK;
}

// The load: header and table validated on the host (nothing allocated before), every section streamed through the pinned chunks into a device array of its
// own and digested THERE, the digests compared with the table, then the index built on those arrays by the roads every other index takes
extern "C" int lsq_index_load(lsq_index **out, lsq_ctx *c, const char *path, int flags) {
    const char *fn = "lsq_index_load";
    if (!out) { lsq_set_error("%s: null out pointer", fn); return LSQ_EINVAL; }
    *out = nullptr;
    if (!c || !path) { lsq_set_error("%s: null %s", fn, c ? "path" : "context"); return LSQ_EINVAL; }
    if (flags != 0) { lsq_set_error("%s: flags must be 0 (got %d)", fn, flags); return LSQ_EINVAL; }
    LSQ_TRY(use_device(c));
    const auto t_call = std::chrono::steady_clock::now();
    lsq_snap_file in;
    in.f = fopen(path, "rb");
    if (!in.f) { lsq_set_error("%s: cannot open %s: %s", fn, path, strerror(errno)); return LSQ_EIO; }
    lsq_snapshot_info s;
    lsq_snap_error err;
    if (const int rc = lsq_snap_read_header(in.f, &s, &err)) { lsq_set_error("%s: %s", fn, err.text); return rc; }
    ScopedBuf buf[LSQ_SNAP_MAX_SECTIONS];
    SnapStage st;
    LSQ_TRY(st.open(c, true, true, false));
    int64_t at = lsq_snap_table_end(s.nsections);
    for (int k = 0; k < (int)s.nsections; ++k) {
        const lsq_snapshot_section &sec = s.sections[k];
        const char *name = lsq_snap_kind_name(sec.kind);
        if (const int rc = lsq_snap_read_pad(in.f, at, sec.offset, name, &err)) { lsq_set_error("%s: %s", fn, err.text); return rc; }
        LSQ_TRY(buf[k].b.ensure((size_t)sec.bytes + 16));             // 16 bytes of slack past the last row, never read
        const int64_t nchunks = (sec.bytes + st.chunk - 1) / st.chunk;
        for (int64_t j = 0; j < nchunks; ++j) {
            const int sl = (int)(j & 1);
            const int64_t off = j * st.chunk, len = std::min(st.chunk, sec.bytes - off);
            LSQ_TRY(st.wait(sl));                                     // the upload of chunk j - 2 has left the pinned chunk
            const auto t0 = std::chrono::steady_clock::now();
            if (fread(st.pin[sl], 1, (size_t)len, in.f) != (size_t)len) { lsq_set_error("%s: section %s: read failed at byte %lld", fn, name, (long long)off); return LSQ_EIO; }
            st.info.file_ms += snap_ms_since(t0);
            char *dst = buf[k].b.as<char>() + off;
            LSQ_TRY(st.mark(sl, 0));
            LSQ_HIP(hipMemcpyAsync(dst, st.pin[sl], (size_t)len, hipMemcpyHostToDevice, st.s));
            LSQ_TRY(st.mark(sl, 1));
            LSQ_TRY(lsq_snap_launch_digest(st.s, dst, (uint64_t)len, (uint64_t)off / 4, st.partials.as<unsigned long long>(), st.slot(k)));
            LSQ_TRY(st.mark(sl, 2));
            LSQ_TRY(st.mark(sl, 3));
            st.busy[sl] = true;
        }
        st.info.chunks += nchunks; st.info.sections += 1;
        at = sec.offset + sec.bytes;
    }
    LSQ_TRY(st.wait(0));
    LSQ_TRY(st.wait(1));
    uint64_t dig[LSQ_SNAP_MAX_SECTIONS];
    LSQ_TRY(st.digests((int)s.nsections, dig));
    for (int k = 0; k < (int)s.nsections; ++k)
        if (dig[k] != s.sections[k].digest) {
            lsq_set_error("%s: section %s: digest mismatch (the table says %016llx, what arrived on the device gives %016llx)", fn, lsq_snap_kind_name(s.sections[k].kind),
                          (unsigned long long)s.sections[k].digest, (unsigned long long)dig[k]);
            return LSQ_EFORMAT;
        }
    auto find = [&](int64_t kind) -> DevBuf * {
        for (int k = 0; k < (int)s.nsections; ++k) if (s.sections[k].kind == kind) return &buf[k].b;
        return nullptr;
    };
    auto ptr = [&](int64_t kind) -> void * { DevBuf *b = find(kind); return b ? b->p : nullptr; };
    auto take = [&](int64_t kind, DevBuf &own) { if (DevBuf *b = find(kind)) { own = *b; *b = DevBuf{}; } };      // the index owns the array from here on
    lsq_index *ix = nullptr;
    if (!s.packed) {
        lsq_index_desc d{};
        d.n = s.n; d.d = (int)s.d; d.m = (int)s.m; d.h = (int)s.h;
        d.codes = static_cast<const uint8_t *>(ptr(LSQ_SNAP_CODES)); d.codebooks = static_cast<const float *>(ptr(LSQ_SNAP_CODEBOOKS));
        d.dbnorms = static_cast<const float *>(ptr(LSQ_SNAP_DBNORMS));
        d.base = ptr(LSQ_SNAP_BASE); d.base_u8 = (int)s.base_format; d.ldb = (int)s.d; d.on_device = 1;
        LSQ_TRY(lsq_index_create(&ix, c, &d));
        take(LSQ_SNAP_CODES, ix->own_codes);
        take(LSQ_SNAP_DBNORMS, ix->own_norms);
    } else {
        lsq_index_packed_desc d{};
        d.n = s.n; d.d = (int)s.d; d.m = (int)s.m; d.h = (int)s.h; d.ncb = (int)s.ncb;
        d.codes = static_cast<const uint8_t *>(ptr(LSQ_SNAP_CODES)); d.norm_codes = static_cast<const uint8_t *>(ptr(LSQ_SNAP_NORM_CODES));
        d.cbnorms = static_cast<const float *>(ptr(LSQ_SNAP_CBNORMS)); d.codebooks = static_cast<const float *>(ptr(LSQ_SNAP_CODEBOOKS));
        d.base = ptr(LSQ_SNAP_BASE); d.base_u8 = (int)s.base_format; d.ldb = (int)s.d; d.on_device = 1;
        LSQ_TRY(lsq_index_create_packed(&ix, c, &d));                 // a norm byte >= ncb: LSQ_EINVAL from the pack kernel's count
    }
    take(LSQ_SNAP_CODEBOOKS, ix->own_K);
    take(LSQ_SNAP_BASE, ix->own_base);
    int rc = LSQ_OK;
    if (s.nlist > 0) {
        lsq_ivf_desc d{};
        d.nlist = (int)s.nlist; d.centroids = static_cast<const float *>(ptr(LSQ_SNAP_CENTROIDS)); d.list_of_row = static_cast<const int32_t *>(ptr(LSQ_SNAP_LIST_OF_ROW));
        d.on_device = 1;
        rc = lsq_index_set_lists(ix, &d);                             // a list id outside [0, nlist): LSQ_EINVAL from the key kernel's count
    }
    if (rc == LSQ_OK && s.filter_active) {
        const int64_t words = (s.n + 31) / 32;
        uint32_t last = 0;
        if (hipMemcpy(&last, static_cast<const uint32_t *>(ptr(LSQ_SNAP_FILTER_BITS)) + (words - 1), 4, hipMemcpyDeviceToHost) != hipSuccess) { lsq_set_error("%s: the read-back failed", fn); rc = LSQ_EHIP; }
        if (rc == LSQ_OK && s.n % 32 && (last >> (s.n % 32)) != 0) { lsq_set_error("%s: section FILTER_BITS: bits at or past n are set", fn); rc = LSQ_EFORMAT; }
        lsq_filter_desc d{};
        d.form = LSQ_FILTER_BITS; d.data = ptr(LSQ_SNAP_FILTER_BITS); d.flags = (int)s.filter_force; d.on_device = 1;
        if (rc == LSQ_OK) rc = lsq_index_set_filter(ix, &d);
        if (rc == LSQ_OK && lsq_filter_get(ix->filter).allowed != s.allowed) {
            lsq_set_error("%s: section FILTER_BITS: %lld bits are set, the header says %lld", fn, (long long)lsq_filter_get(ix->filter).allowed, (long long)s.allowed);
            rc = LSQ_EFORMAT;
        }
    }
    if (rc != LSQ_OK) { (void)lsq_index_destroy(ix); return rc; }
    st.info.bytes = s.file_bytes;
    st.info.total_ms = snap_ms_since(t_call);
    ix->sinfo = st.info;
    *out = ix;
    return LSQ_OK;
}

// ---- the beam-search encoder on resident codebooks (lsq_beam.hip): a handle with its own copy of the codebooks, ||c||^2 and pair tables built once, and its own
// scratch.  Nothing of the context is read but its device, its stream and option "profile"; nothing of it is written --------------------------------------------
struct lsq_encoder {
    lsq_ctx *ctx = nullptr;
    int d = 0, m = 0;
    int64_t chunk = 65536;
    DevBuf K, sci, T;                                  // the codebooks' copy, ||c||^2, T[j][k][b][a] = 2 <c_kb, c_ja>
    DevBuf U;                                          // one chunk's row-major f32 unary planes [m][cn][256]
    DevBuf sX, sCodes, sScore;                         // staging of host-buffer calls: a chunk's rows, its int16 codes, its scores
    PhaseClock<3> clock;                               // a chunk's unaries and its beam search
    lsq_encoder_info info{};
};

extern "C" int lsq_encoder_destroy(lsq_encoder *en) {
    if (!en) return LSQ_OK;
    (void)hipSetDevice(en->ctx->device);
    (void)hipStreamSynchronize(en->ctx->stream);
    DevBuf *bufs[] = {&en->K, &en->sci, &en->T, &en->U, &en->sX, &en->sCodes, &en->sScore};
    for (DevBuf *b : bufs) b->release();
    en->clock.release();
    delete en;
    return LSQ_OK;
}

static int encoder_build(lsq_encoder *en, const float *codebooks, int on_device) {
    hipStream_t s = en->ctx->stream;
    const int mh = en->m * LSQ_H;
    LSQ_TRY(en->K.ensure(sizeof(float) * (size_t)mh * en->d));
    LSQ_TRY(en->sci.ensure(sizeof(float) * (size_t)mh));
    LSQ_TRY(en->T.ensure(sizeof(float) * (size_t)mh * mh));
    LSQ_HIP(hipMemcpyAsync(en->K.p, codebooks, sizeof(float) * (size_t)mh * en->d, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    // the path's own numbers: ||c||^2 as the unary GEMM adds it, and the table GEMM of prepare_tables (rows (k, b), columns (j, a))
    LSQ_TRY(lsq_launch_sqnorms(s, en->K.as<float>(), mh, en->d, en->sci.as<float>()));
    LSQ_TRY(lsq_launch_chain_gemm(s, en->K.as<float>(), en->K.as<float>(), nullptr, 2.0f, mh, mh, en->d, LSQ_H, (int64_t)en->m * LSQ_H * LSQ_H, LSQ_H,
                                  en->T.as<float>(), 0, mh, 0));
    LSQ_HIP(hipStreamSynchronize(s));
    return LSQ_OK;
}

extern "C" int lsq_encoder_create(lsq_encoder **out, lsq_ctx *c, const lsq_encoder_desc *desc) {
    if (!out) { lsq_set_error("lsq_encoder_create: null out pointer"); return LSQ_EINVAL; }
    *out = nullptr;
    if (!c || !desc) { lsq_set_error("lsq_encoder_create: null %s", c ? "description" : "context"); return LSQ_EINVAL; }
    if (desc->h != LSQ_H || desc->m < 1 || desc->m > LSQ_MAX_M || desc->d < 1) {
        lsq_set_error("lsq_encoder_create: needs h == 256, 1 <= m <= 16 and d >= 1 (got h=%d m=%d d=%d)", desc->h, desc->m, desc->d);
        return LSQ_EINVAL;
    }
    if (desc->chunk < 0) { lsq_set_error("lsq_encoder_create: needs chunk >= 0 (got %lld)", (long long)desc->chunk); return LSQ_EINVAL; }
    if (!desc->codebooks) { lsq_set_error("lsq_encoder_create: null codebooks"); return LSQ_EINVAL; }
    LSQ_TRY(use_device(c));
    lsq_encoder *en = new lsq_encoder();
    en->ctx = c;
    en->d = desc->d; en->m = desc->m;
    if (desc->chunk > 0) en->chunk = desc->chunk;
    const int rc = encoder_build(en, desc->codebooks, desc->on_device);
    if (rc != LSQ_OK) { (void)lsq_encoder_destroy(en); return rc; }
    *out = en;
    return LSQ_OK;
}

extern "C" int lsq_encoder_beam(lsq_encoder *en, const void *X, int x_u8, int64_t n, int beam, const int32_t *order, void *codes, float *score,
                                int on_device) {
    if (!en) { lsq_set_error("lsq_encoder_beam: null encoder"); return LSQ_EINVAL; }
    if (n < 0 || beam < 1 || beam > 32) { lsq_set_error("lsq_encoder_beam: needs n >= 0 and 1 <= beam <= 32 (got n=%lld beam=%d)", (long long)n, beam); return LSQ_EINVAL; }
    if (n > 0 && (!X || !codes)) { lsq_set_error("lsq_encoder_beam: null pointer"); return LSQ_EINVAL; }
    const int m = en->m, d = en->d;
    uint8_t ord[LSQ_MAX_M];
    unsigned seen = 0;
    for (int t = 0; t < m; ++t) {
        const int32_t o = order ? order[t] : t;
        if (o < 0 || o >= m || (seen >> o & 1u)) { lsq_set_error("lsq_encoder_beam: the visiting order is not a permutation of 0 .. %d", m - 1); return LSQ_EINVAL; }
        seen |= 1u << o;
        ord[t] = (uint8_t)o;
    }
    if (n == 0) return LSQ_OK;
    lsq_ctx *c = en->ctx;
    LSQ_TRY(use_device(c));
    hipStream_t s = c->stream;
    const size_t elem = x_u8 ? 1 : sizeof(float);
    lsq_encoder_info info{};
    info.vectors = n; info.beam = beam;
    for (int64_t off = 0; off < n; off += en->chunk) {
        const int64_t cn = std::min<int64_t>(en->chunk, n - off);
        const char *Xc = static_cast<const char *>(X) + (size_t)off * d * elem;
        void *out_codes = on_device ? static_cast<void *>(static_cast<uint8_t *>(codes) + off * m) : nullptr;
        float *out_score = on_device && score ? score + off : nullptr;
        if (!on_device) {
            LSQ_TRY(en->sX.ensure((size_t)cn * d * elem));
            LSQ_TRY(en->sCodes.ensure(sizeof(int16_t) * (size_t)cn * m));
            if (score) LSQ_TRY(en->sScore.ensure(sizeof(float) * (size_t)cn));
            LSQ_HIP(hipMemcpyAsync(en->sX.p, Xc, (size_t)cn * d * elem, hipMemcpyHostToDevice, s));
            Xc = en->sX.as<char>(); out_codes = en->sCodes.p; out_score = score ? en->sScore.as<float>() : nullptr;
        }
        LSQ_TRY(en->U.ensure(sizeof(float) * (size_t)m * (size_t)cn * LSQ_H));
        LSQ_TRY(en->clock.begin(c->profile != 0));
        LSQ_TRY(en->clock.mark(s));
        // row-major planes U[(j cn + i) 256 + a] = chain(x_i[t] * -2 K[j, a][t]) + ||c_ja||^2: the bits of lsq_get_unaries
        if (x_u8) LSQ_TRY(lsq_launch_chain_gemm(s, reinterpret_cast<const uint8_t *>(Xc), en->K.as<float>(), en->sci.as<float>(), -2.0f, cn, m * LSQ_H, d, LSQ_H,
                                                cn * (int64_t)LSQ_H, LSQ_H, en->U.as<float>(), 0, cn, 0));
        else LSQ_TRY(lsq_launch_chain_gemm(s, reinterpret_cast<const float *>(Xc), en->K.as<float>(), en->sci.as<float>(), -2.0f, cn, m * LSQ_H, d, LSQ_H,
                                           cn * (int64_t)LSQ_H, LSQ_H, en->U.as<float>(), 0, cn, 0));
        LSQ_TRY(en->clock.mark(s));
        LSQ_TRY(lsq_launch_beam(s, en->U.as<float>(), en->T.as<float>(), cn, m, beam, ord, out_codes, on_device ? 0 : 1, out_score));
        LSQ_TRY(en->clock.mark(s));
        float ms[2];
        LSQ_TRY(en->clock.read(ms));                  // (untimed: zeros, and no wait)
        info.unaries_ms += ms[0]; info.beam_ms += ms[1];
        if (!on_device) {        // in stream order: the next chunk's kernels overwrite the staging only after these copies
            LSQ_HIP(hipMemcpyAsync(static_cast<int16_t *>(codes) + off * m, en->sCodes.p, sizeof(int16_t) * (size_t)cn * m, hipMemcpyDeviceToHost, s));
            if (score) LSQ_HIP(hipMemcpyAsync(score + off, en->sScore.p, sizeof(float) * (size_t)cn, hipMemcpyDeviceToHost, s));
        }
        info.chunks += 1;
    }
    if (!on_device) LSQ_HIP(hipStreamSynchronize(s));
    en->info = info;
    return LSQ_OK;
}

extern "C" int lsq_encoder_get_info(lsq_encoder *en, lsq_encoder_info *out) {
    if (!en || !out) { lsq_set_error("lsq_encoder_get_info: null argument"); return LSQ_EINVAL; }
    *out = en->info;
    return LSQ_OK;
}

extern "C" int lsq_synchronize(lsq_ctx *c) {
    LSQ_TRY(use_device(c));
    LSQ_HIP(hipStreamSynchronize(c->stream));
    return LSQ_OK;
}

// ---- host-side pieces of the path -----------------------------------------------------------------
extern "C" int lsq_node_order(uint64_t seed, uint32_t it, int m, int randord, int32_t *order) {
    if (!order || m < 1 || m > LSQ_MAX_M) { lsq_set_error("lsq_node_order: bad arguments"); return LSQ_EINVAL; }
    for (int p = 0; p < m; ++p) order[p] = p;
    if (!randord) return LSQ_OK;
    for (int p = m - 1; p >= 1; --p) {        // Fisher-Yates on Philox words of domain PERM
        const uint32_t r = lsq_rng_word(seed, 0, it, LSQ_DOM_PERM, (uint32_t)(m - 1 - p));
        const int q = (int)lsq_mulhi32(r, (uint32_t)(p + 1));
        std::swap(order[p], order[q]);
    }
    return LSQ_OK;
}

extern "C" int lsq_splitarray(int64_t n, int nparts, int part, int64_t *start, int64_t *len) {
    if (n < 0 || nparts < 1 || part < 0 || part >= nparts || !start || !len) { lsq_set_error("lsq_splitarray: bad arguments"); return LSQ_EINVAL; }
    const int64_t per = n / nparts, xtra = n % nparts;      // first `xtra` parts get one more (utils.jl:152-177)
    *start = part < xtra ? part * (per + 1) : xtra * (per + 1) + (part - xtra) * per;
    *len = part < xtra ? per + 1 : per;
    return LSQ_OK;
}

extern "C" int lsq_randinit(uint64_t seed, uint64_t global_offset, int64_t n, int m, int h, int16_t *B) {
    if (n < 0 || m < 1 || h < 1 || h > 32767 || (!B && n > 0)) { lsq_set_error("lsq_randinit: bad arguments"); return LSQ_EINVAL; }
    for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j)
            B[i * m + j] = (int16_t)(1 + lsq_mulhi32(lsq_rng_word(seed, global_offset + (uint64_t)i, 0, LSQ_DOM_INIT, (uint32_t)j), (uint32_t)h));
    return LSQ_OK;
}

static int check_shape(const char *fn, int d, int64_t n, int m, int h) {
    if (d < 1 || n < 0 || m < 1 || m > LSQ_MAX_M) { lsq_set_error("%s: bad shape d=%d n=%lld m=%d (need d>=1, n>=0, 1<=m<=16)", fn, d, (long long)n, m); return LSQ_EINVAL; }
    if (h != LSQ_H) { lsq_set_error("%s: h=%d unsupported; this engine (like the reference GPU path) needs h == 256", fn, h); return LSQ_EINVAL; }
    return LSQ_OK;
}

// input codes must lie in 1..h (Julia 1-based).  A flat scan of n*m int16 (vectorised; ~1 ms per 10^6 x 8) done up front so
// that an invalid call neither spends the encode nor clobbers the caller's output buffer.
static int check_codes_host(const char *fn, const int16_t *B, int64_t n, int m, int h) {
    const int64_t total = n * (int64_t)m;
    unsigned bad = 0;
    for (int64_t q = 0; q < total; ++q) bad |= (unsigned)((unsigned)(uint16_t)(B[q] - 1) >= (unsigned)h);
    if (bad) { lsq_set_error("%s: input codes must lie in 1..%d", fn, h); return LSQ_ECODE; }
    return LSQ_OK;
}

// ---- device core ----------------------------------------------------------------------------------
static int prepare_tables(lsq_ctx *c, const float *dK, int d, int m) {
    Timer t(c, CAT_TABLES);
    c->tables_changed = 1;
    c->chunk_road.resident = false;      // the f32 tables the resident levels were taken of are about to change
    c->tables_valid = false;        // whoever knows the host copy of dK marks it valid again (host_codebooks)
    const int mh = m * LSQ_H;
    LSQ_TRY(c->sci.ensure(sizeof(float) * (size_t)mh));
    LSQ_TRY(c->T.ensure(sizeof(float) * (size_t)mh * mh));
    LSQ_TRY(lsq_launch_sqnorms(c->stream, dK, mh, d, c->sci.as<float>()));
    // rows r = (k,b), cols c = (j,a):  T[((j*m + k)*h + b)*h + a] = chain(K[k,b][t] * 2 K[j,a][t])
    LSQ_TRY(lsq_launch_chain_gemm(c->stream, dK, dK, nullptr, 2.0f, mh, mh, d, LSQ_H, (int64_t)m * LSQ_H * LSQ_H, LSQ_H, c->T.as<float>(), 0, mh, 0));
    if (c->schedule >= 3 && m > 1) {        // slice-major copy for the LDS-walk kernel's contiguous staging
        LSQ_TRY(c->Ts.ensure(sizeof(float) * (size_t)m * (m - 1) * LSQ_H * LSQ_H));
        LSQ_TRY(lsq_launch_tables_to_slices(c->stream, c->T.as<float>(), c->Ts.as<float>(), m, lsq_walk_slice_width(m)));
    }
    return LSQ_OK;
}

// A chunk's unaries start here: what the last chunk left is forgotten (the ONE reset of the chunk state).  -> the chunk builds levels for the filtered walk
static bool use_q16(const lsq_ctx *c, int64_t cn) { return c->schedule >= 6 && cn >= c->q16_min; }
static bool start_chunk(lsq_ctx *c, int64_t cn, int slice) {
    c->chunk_road = ChunkRoad{};
    return slice > 0 && use_q16(c, cn);
}

// The ONE map of the filter's device memory (lsq_q16_work): buffers sized for a chunk of cn vectors, the scratch block carved.  Layout of qscratch (bytes):
// [16] bad, [64, 208) the range keys and the four words after them, [256 ..) table ranges (3 m m floats), then from the next multiple of 256 row minima and
// column means (m m h floats each), the unary's column shift (m h floats), codebook means (m d floats).  nsample_rows > 0: room for the sample's sigma too.
static int q16_map(lsq_ctx *c, int d, int64_t cn, int m, int64_t nsample_rows) {
    LSQ_TRY(c->Uq.ensure(sizeof(uint16_t) * (size_t)m * (size_t)cn * LSQ_H));
    LSQ_TRY(c->Tq.ensure(sizeof(uint16_t) * (size_t)m * (size_t)(m > 1 ? m - 1 : 1) * LSQ_H * LSQ_H));
    const size_t off_bad = 16, off_qrange = 64, off_trange = 256;
    static_assert(off_qrange + sizeof(unsigned) * lsq_q16_work::Q_WORDS <= off_trange, "the range words end before the table ranges");
    const size_t off_rowmin = (off_trange + sizeof(float) * 3 * (size_t)m * m + 255) & ~(size_t)255;
    const size_t off_colmean = off_rowmin + sizeof(float) * (size_t)m * m * LSQ_H;
    const size_t off_colshift = off_colmean + sizeof(float) * (size_t)m * m * LSQ_H;
    const size_t off_means = off_colshift + sizeof(float) * (size_t)m * LSQ_H;
    LSQ_TRY(c->qscratch.ensure(off_means + sizeof(float) * (size_t)m * d));
    LSQ_TRY(c->qsigma.ensure(sizeof(float) * (size_t)cn * m));      // per-(vector, node) unary shift: levels only (lsq_icmq.hip)
    LSQ_TRY(c->qflag.ensure(sizeof(unsigned short) * (size_t)(cn + 2)));
    LSQ_TRY(c->qp.ensure(sizeof(lsq_q16_params)));
    if (nsample_rows > 0) LSQ_TRY(c->sSigmaS.ensure(sizeof(float) * (size_t)nsample_rows * m));
    char *sc = c->qscratch.as<char>();
    lsq_q16_work &w = c->qw;
    w = lsq_q16_work{};
    w.Tq = c->Tq.as<uint16_t>(); w.Uq = c->Uq.as<uint16_t>();
    w.bad = reinterpret_cast<int *>(sc + off_bad);
    w.qrange = reinterpret_cast<unsigned *>(sc + off_qrange);
    w.trange = reinterpret_cast<float *>(sc + off_trange);
    w.rowmin = reinterpret_cast<float *>(sc + off_rowmin);
    w.colmean = reinterpret_cast<float *>(sc + off_colmean);
    w.colshift = reinterpret_cast<float *>(sc + off_colshift);
    w.means = reinterpret_cast<float *>(sc + off_means);
    w.sigma = c->qsigma.as<float>();
    w.qflag = c->qflag.as<unsigned short>();
    w.P = c->qp.as<lsq_q16_params>();
    return LSQ_OK;
}

// q16 part of a chunk's unary build: the map, sampled value ranges -> parameters -> 16-bit slice tables.  Xsample != nullptr: the host-buffer pipeline
// (the sample was uploaded ahead of X: lsq_launch_q16_prepare's sample mode)
// XT (here and below): the element type of X -- float, or uint8_t for the 8-bit entry points (lsq_encode_icm_u8 and its kin): the rows stay 8-bit in the
// context's chunk buffers and the kernels widen them in registers (lsq_xload.h)
template <class XT>
static int q16_prepare_chunk(lsq_ctx *c, const XT *dX, const float *dK, int d, int64_t cn, int m, const XT *Xsample = nullptr, int64_t nsample_rows = 0) {
    Timer t(c, CAT_TABLES);
    LSQ_TRY(q16_map(c, d, cn, m, Xsample ? nsample_rows : 0));
    if (Xsample) { c->qw.Xsample = Xsample; c->qw.nsample_rows = nsample_rows; c->qw.sigma_sample = c->sSigmaS.as<float>(); }
    LSQ_TRY(lsq_launch_q16_prepare(c->stream, dX, cn, d, dK, c->sci.as<float>(), c->T.as<float>(), m, c->qw, c->tables_changed));
    c->tables_changed = 0;
    return LSQ_OK;
}

// the unary GEMM of rows [r0, r0 + rows) of a cn-vector chunk (dXc points at the chunk's first vector); q16: it also emits the u16 level planes
// row-major  (slice == 0): U[(j*cn + i)*h + a]                      = chain(x_i[t] * -2 K[j,a][t]) + sci[j,a]
// slice-major (slice = SL): U[j*cn*h + ((a/SL)*cn + i)*SL + a%SL]   (same values, LDS-slice schedule)
template <class XT>
static int unary_gemm(lsq_ctx *c, const XT *dXc, const float *dK, int d, int64_t cn, int m, int slice, int64_t r0, int64_t rows, bool q16) {
    lsq_gemm_q16 levels;
    if (q16) {
        const lsq_q16_work &w = c->qw;
        levels.Dq = w.Uq; levels.slice_q = lsq_q16_slice_width(m); levels.qp = w.P; levels.qflag = w.qflag; levels.sigma = w.sigma; levels.colshift = w.colshift;
    }
    return lsq_launch_chain_gemm(c->stream, dXc + (size_t)r0 * d, dK, c->sci.as<float>(), -2.0f, rows, m * LSQ_H, d, LSQ_H, cn * (int64_t)LSQ_H, LSQ_H,
                                 c->U.as<float>(), slice, cn, r0, q16 ? &levels : nullptr);
}

static int q16_verdict(lsq_ctx *c, bool q16, int64_t cn, int m);

// unaries of rows [r0, r0 + rows) of a cn-vector chunk (dX points at the chunk's first vector)
template <class XT>
static int build_unaries(lsq_ctx *c, const XT *dX, const float *dK, int d, int64_t cn, int m, int slice, int64_t r0, int64_t rows) {
    const bool q16 = start_chunk(c, cn, slice) && r0 == 0 && rows == cn;
    if (q16) LSQ_TRY(q16_prepare_chunk(c, dX, dK, d, cn, m));      // 16-bit filtered walk: the GEMM below then also emits the u16 planes
    {
        Timer t(c, CAT_UNARIES);
        LSQ_TRY(c->U.ensure(sizeof(float) * (size_t)m * (size_t)cn * LSQ_H));
        LSQ_TRY(unary_gemm(c, dX, dK, d, cn, m, slice, r0, rows, q16));
    }
    return q16_verdict(c, q16, cn, m);
}

// which road the chunk takes after its unary GEMM (filtered walk / f32 walk): on the host, or -- option "async" -- by a one-thread kernel
static int q16_verdict(lsq_ctx *c, bool q16, int64_t cn, int m) {
    if (q16 && c->async_mode) {
        // option "async": the same verdict taken by a one-thread kernel; both walks are enqueued and the word picks (run_sweeps)
        LSQ_TRY(c->road.ensure(2 * sizeof(unsigned)));
        LSQ_TRY(lsq_launch_q16_road(c->stream, c->qp.as<lsq_q16_params>(), c->road.as<unsigned>(), cn * (int64_t)m, c->fallback_div));
        c->chunk_road.filtered = true;
        c->chunk_road.on_device = true;
    } else if (q16) {
        // The chunk's verdict (three words, ONE host round trip per resident chunk -- 10^6 vectors, ~50 ms of work): usable bounds, and few enough
        // (vector, node) pairs outside the sampled level range.  Such pairs take the one-wave-per-vector f32 routine inside the filtered walk (~5x the
        // cost of a filtered update): above 1 / filter_fallback_div of the pairs -- heavy tails, a drifting or sorted chunk -- the f32 walk is the
        // faster road for the whole chunk (measured: Cauchy-scaled vectors 2.2 -> 13 M vectors/s).  Exactness depends on neither road.
        // The f32 unaries are there either way (the GEMM wrote both outputs), so the hand-over costs nothing but this read.
        int verdict[3] = {0, 0, 0};      // lsq_q16_params: ok, oor, nflag
        LSQ_HIP(hipMemcpyAsync(verdict, c->qp.p, sizeof(verdict), hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipStreamSynchronize(c->stream));
        if (verdict[0] == 1 && (int64_t)verdict[2] * c->fallback_div <= cn * (int64_t)m) c->chunk_road.filtered = true;
        else c->filter_fallback_chunks += 1;
        c->chunk_road.resident = c->chunk_road.filtered;
        c->chunk_road.cn = cn; c->chunk_road.m = m; c->chunk_road.row0 = c->call_row0;
    }
    return LSQ_OK;
}

// The FIRST chunk of a host-buffer call: X goes up panel by panel on the copy stream (a helper thread issues the pageable copies: each one blocks its
// caller for the length of the transfer) and every panel's sigma pass + unary GEMM runs on the compute stream as soon as the panel has landed -- the
// GEMM hides under the upload instead of following it (measured: 512 MB take 9.5 ms at 56 GB/s whichever way they are issued).
// The filtered walk's level parameters need value ranges BEFORE the first GEMM panel: the sample rows (the same every-rts-th 128-row panels the
// strided pass reads) are packed on the host and uploaded first, a few MB.  Same codes as the one-piece path: the parameters only steer the filter.
template <class XT>
static int build_unaries_from_host(lsq_ctx *c, const XT *Xh, XT *dXc, const float *dK, int d, int64_t cn, int m, int slice) {
    const bool q16 = start_chunk(c, cn, slice);
    const size_t row_bytes = sizeof(XT) * (size_t)d;
    int64_t prow = (int64_t)((uint64_t)c->panel_bytes / row_bytes) / 128 * 128;      // ~48 MB panels, whole 128-row tiles
    if (prow < 128) prow = 128;
    const int npan = (int)((cn + prow - 1) / prow);
    if (!c->copy_stream) LSQ_HIP(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    while ((int)c->panel_ev.size() < npan) {
        hipEvent_t e = nullptr;
        LSQ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->panel_ev.push_back(e);
    }
    if (q16) {
        int64_t rts = 1;
        const int spanels = lsq_q16_sample_rows(cn, d, &rts);
        int64_t ns = 0;
        for (int sp = 0; sp < spanels; ++sp) ns += std::min<int64_t>(128, cn - (int64_t)sp * rts * 128);
        c->sample_host.resize(((size_t)ns * row_bytes + sizeof(float) - 1) / sizeof(float));      // (bytes, whatever the element type)
        XT *sample = reinterpret_cast<XT *>(c->sample_host.data());
        int64_t at = 0;
        for (int sp = 0; sp < spanels; ++sp) {
            const int64_t r0 = (int64_t)sp * rts * 128, rows = std::min<int64_t>(128, cn - r0);
            memcpy(sample + (size_t)at * d, Xh + (size_t)r0 * d, (size_t)rows * row_bytes);
            at += rows;
        }
        LSQ_TRY(c->sSample.ensure((size_t)ns * row_bytes));
        LSQ_HIP(hipMemcpyAsync(c->sSample.p, sample, (size_t)ns * row_bytes, hipMemcpyHostToDevice, c->stream));
        LSQ_TRY(q16_prepare_chunk<XT>(c, dXc, dK, d, cn, m, c->sSample.as<XT>(), ns));
    }
    LSQ_TRY(c->U.ensure(sizeof(float) * (size_t)m * (size_t)cn * LSQ_H));
    std::atomic<int> landed{0};
    hipError_t herr = hipSuccess;
    std::thread feeder;
    try {
    feeder = std::thread([&]() {
        hipError_t e = hipSetDevice(c->device);
        for (int p = 0; p < npan && e == hipSuccess; ++p) {
            const int64_t r0 = (int64_t)p * prow, rows = std::min<int64_t>(prow, cn - r0);
            e = hipMemcpyAsync(dXc + (size_t)r0 * d, Xh + (size_t)r0 * d, (size_t)rows * row_bytes, hipMemcpyHostToDevice, c->copy_stream);
            if (e == hipSuccess) e = hipEventRecord(c->panel_ev[(size_t)p], c->copy_stream);
            if (e == hipSuccess) landed.store(p + 1, std::memory_order_release);
        }
        herr = e;
        if (e != hipSuccess) landed.store(npan + 1, std::memory_order_release);      // release the consumer: it checks herr after the join
    });
    } catch (...) {      // no thread to be had: nothing may escape the C ABI -- one-piece upload on the compute stream, then the ordinary build
        LSQ_HIP(hipMemcpyAsync(dXc, Xh, (size_t)cn * row_bytes, hipMemcpyHostToDevice, c->stream));
        if (q16) c->tables_changed = 1;      // the flags / counters the sample-mode prepare left behind are rebuilt by the full-chunk prepare inside build_unaries
        return build_unaries(c, dXc, dK, d, cn, m, slice, 0, cn);
    }
    int rc = LSQ_OK;
    for (int p = 0; p < npan && rc == LSQ_OK; ++p) {
        for (int spins = 0; landed.load(std::memory_order_acquire) <= p; ++spins) {      // a panel takes ~1 ms to go up: poll briefly, then sleep instead of burning the core
            if (spins < 64) std::this_thread::yield();
            else std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        if (landed.load(std::memory_order_acquire) > npan) break;                    // the feeder failed
        const int64_t r0 = (int64_t)p * prow, rows = std::min<int64_t>(prow, cn - r0);
        if (hipStreamWaitEvent(c->stream, c->panel_ev[(size_t)p], 0) != hipSuccess) { lsq_set_error("hipStreamWaitEvent failed"); rc = LSQ_EHIP; break; }
        Timer t(c, CAT_UNARIES);
        if (q16) rc = lsq_launch_unary_shift_panel(c->stream, dXc + (size_t)r0 * d, rows, d, m, c->qw, r0);
        if (rc == LSQ_OK) rc = unary_gemm(c, dXc, dK, d, cn, m, slice, r0, rows, q16);
    }
    feeder.join();
    if (herr != hipSuccess) { lsq_set_error("upload of X failed: %s", hipGetErrorString(herr)); return herr == hipErrorOutOfMemory ? LSQ_ENOMEM : LSQ_EHIP; }
    LSQ_TRY(rc);
    return q16_verdict(c, q16, cn, m);
}

// nsweeps sweeps over the chunk's m nodes in `order`.  stats: where the walk launches accumulate their statistics (the call's block, the probe's, or nullptr)
// ref_rec / ref_valid: the vectors' current records and validity masks (read-only during the sweeps), or nullptr
// first_sweep: position of the first of the nsweeps sweeps inside its ILS iteration (the per-position trace counters only)
static int run_sweeps(lsq_ctx *c, uint8_t *rec, unsigned short *valid, int64_t cn, int m, const int32_t *order, int nsweeps, unsigned long long *stats,
                      const uint8_t *ref_rec = nullptr, const unsigned short *ref_valid = nullptr, int first_sweep = 0) {
    if (nsweeps <= 0) return LSQ_OK;
    const int pos_base = first_sweep * m;
    Timer t(c, CAT_ICM);
    if (!c->fallback) { ref_rec = nullptr; ref_valid = nullptr; }
    std::vector<int32_t> seq((size_t)nsweeps * m);
    for (int sw = 0; sw < nsweeps; ++sw)
        for (int q = 0; q < m; ++q) seq[(size_t)sw * m + q] = order[q];
    // The road, decided once.  Schedule 3: the f32 walk, a launch per node update.  Schedule >= 4: a block owns its vectors through a launch of up to 64 node
    // updates (a whole ILS iteration where it fits) -- on the 16-bit filtered walk where the chunk's verdict named it, else on the f32 walk or, for a chunk so
    // small that every block of the walk kernel would be light (at most `light` vectors each), on icm_wave_kernel: a wave owns its vectors instead (no
    // compaction, no barriers, records and validity words in registers).
    enum { F32, WAVE, FILTERED } road = F32;
    int per_launch = 64;
    if (c->schedule < 4) per_launch = 1;
    else if (c->chunk_road.filtered && valid) {
        road = FILTERED;
        if (c->per_node) per_launch = 1;      // (profiling: per-sweep timings / counters)
    } else {
        int per_pass = 0, npass = 0;
        lsq_walk_geometry(cn, lsq_walk_pp(m, lsq_walk_slice_width(m)), &per_pass, &npass);
        const int light_max = c->light >= 0 ? c->light : 256;
        if (c->ablation == 0 && per_pass <= light_max && per_pass <= c->wave_max) road = WAVE;
    }
    // option "async": the filtered walk runs iff road[0] == 2, and the f32 walk enqueued behind it idles on the same word (road[0] != 0) or does the work
    const bool both = road == FILTERED && c->chunk_road.on_device;
    const float *U = c->U.as<float>(), *T = c->T.as<float>();
    int launched = 0;
    if (road == FILTERED)
        LSQ_TRY(lsq_launch_icm_walkq(c->stream, U, c->Uq.as<uint16_t>(), c->Tq.as<uint16_t>(), T, rec, valid, cn, m, seq.data(), (int)seq.size(), pos_base, per_launch,
                                     c->skip, stats, c->light, ref_rec, ref_valid, c->qp.as<lsq_q16_params>(), c->qflag.as<unsigned short>(),
                                     both ? c->road.as<unsigned>() : nullptr, &launched));
    if (road == WAVE)
        LSQ_TRY(lsq_launch_icm_wave(c->stream, U, T, rec, valid, cn, m, seq.data(), (int)seq.size(), pos_base, 64, c->skip, stats, ref_rec, ref_valid, &launched));
    if (road == F32 || both)
        LSQ_TRY(lsq_launch_icm_walk(c->stream, U, c->Ts.as<float>(), T, rec, valid, cn, m, seq.data(), (int)seq.size(), pos_base, both ? 64 : per_launch, c->skip, stats,
                                    c->ablation, c->light, ref_rec, ref_valid, both ? reinterpret_cast<const int *>(c->road.as<unsigned>()) : nullptr, &launched));
    c->icm_launches += launched;
    return LSQ_OK;
}

static void fold_walk_counters(lsq_ctx *c, const unsigned long long *act);
static int fold_pending(lsq_ctx *c);

struct EncodeParams {
    int d, m;
    const int64_t *ilsiters; int nr;
    int icmiter, npert, randord;
    uint64_t seed; uint32_t it0;
};

// One resident chunk: recCur holds the chunk's codes on entry; snapshots are emitted through `snap`.
template <class Snap, class XT>
static int encode_chunk(lsq_ctx *c, const XT *dXc, const float *dK, int64_t cn, uint64_t goff, const EncodeParams &P, int64_t I, Snap snap,
                        bool unaries_ready = false) {
    const int cs = lsq_code_stride(P.m);
    if (!unaries_ready) LSQ_TRY(build_unaries(c, dXc, dK, P.d, cn, P.m, lsq_walk_slice_width(P.m), 0, cn));
    LSQ_TRY(c->recNew.ensure((size_t)cn * cs));
    LSQ_TRY(c->prev.ensure(sizeof(float) * (size_t)cn));
    LSQ_TRY(c->vCur.ensure(sizeof(unsigned short) * (size_t)(cn + 8)));
    LSQ_TRY(c->vNew.ensure(sizeof(unsigned short) * (size_t)(cn + 8)));
    LSQ_HIP(hipMemsetAsync(c->vCur.p, 0, sizeof(unsigned short) * (size_t)cn, c->stream));      // nothing is known to be an argmin yet
    unsigned short *vcur = c->vCur.as<unsigned short>(), *vnew = c->vNew.as<unsigned short>();
    uint8_t *cur = c->recCur.as<uint8_t>(), *nw = c->recNew.as<uint8_t>();
    float *prev = c->prev.as<float>();
    unsigned long long *counters = c->counters.as<unsigned long long>();
    unsigned long long *totals = c->active.as<unsigned long long>(), *probed = nullptr;      // the walk statistics of the call, and of a probed first iteration
    // The perturbation of ILS iteration t (encode_icm.jl:55-70) rides on the exit of the cost kernel that precedes it: every lane there knows
    // its vector's final record and validity word, so the copy-and-perturb pass over the records and its launch are gone (lsq_perturb stays
    // as the stand-alone entry point).
    lsq_perturb_next pn;
    pn.on = 1; pn.m = P.m; pn.npert = P.npert; pn.seed = P.seed; pn.goff = goff; pn.dst = nw; pn.vdst = vnew;
    {
        Timer t(c, CAT_COST);
        pn.it = P.it0;
        LSQ_TRY(lsq_launch_cost(c->stream, dXc, dK, cur, cur, prev, counters, cn, P.d, P.m, 0, nullptr, vcur, I > 0 ? &pn : nullptr));   // encode_icm.jl:149
    }
    for (int64_t it = 0; it < I; ++it) {
        int32_t order[LSQ_MAX_M];
        LSQ_TRY(lsq_node_order(P.seed, P.it0 + (uint32_t)it, P.m, P.randord, order));
        // The probe: the walk counters of the chunk's first ILS iteration -- or, in a call of ONE iteration (the trainer's chained encoding_icm), of that
        // iteration's first sweep, the launch being split there -- are read back; a filter that decides too little hands the REST to the f32 walk.
        // Nothing is remembered across calls (round 3 kept a per-shape verdict: it could not tell two data sets of one shape apart).
        const bool probing = it == 0 && c->chunk_road.filtered && c->probe_div > 0 && (I > 1 || P.icmiter > 1);
        // a call of ONE iteration probes its first sweeps: two of them when there are at least three (after the first sweep of an iteration EVERY node of every
        // vector has just been recomputed, which dilutes the hard / recomputed ratio the threshold was calibrated on -- ADVICE r4), else one
        const int probe_sweeps = I > 1 ? P.icmiter : (P.icmiter >= 3 ? 2 : 1);
        if (probing) {
            LSQ_TRY(c->probe.ensure(sizeof(unsigned long long) * LSQ_WALK_COUNTERS));
            LSQ_HIP(hipMemsetAsync(c->probe.p, 0, sizeof(unsigned long long) * LSQ_WALK_COUNTERS, c->stream));
            probed = c->probe.as<unsigned long long>();
        }
        LSQ_TRY(run_sweeps(c, nw, vnew, cn, P.m, order, probing ? probe_sweeps : P.icmiter, probing ? probed : totals, cur, vcur, 0));
        if (probing && c->chunk_road.on_device) {
            // option "async": the same probe by a one-thread kernel (it also adds the probed launches' statistics to the call's)
            LSQ_TRY(lsq_launch_q16_probe(c->stream, probed, totals, c->road.as<unsigned>(), c->probe_div));
            LSQ_TRY(run_sweeps(c, nw, vnew, cn, P.m, order, P.icmiter - probe_sweeps, totals, cur, vcur, probe_sweeps));
        } else if (probing) {
            // Is the filter paying off on THIS chunk?  A level step blown up by a few extreme values (scale-mixture / heavy-tailed data) leaves most
            // node updates ambiguous: each then costs an exact refinement (or, past the block's 1024 records, the one-wave f32 routine) on top of the
            // level walk, and the f32 walk is several times faster (measured: Cauchy-scaled vectors 2.2 M vectors/s filtered, 13 M on the f32 walk).
            // The first ILS iteration's counters tell; the f32 unaries are resident either way, so the remaining iterations just change road.
            unsigned long long act[LSQ_WALK_COUNTERS] = {0};
            LSQ_HIP(hipMemcpyAsync(act, c->probe.p, sizeof(act), hipMemcpyDeviceToHost, c->stream));
            LSQ_HIP(hipStreamSynchronize(c->stream));
            fold_walk_counters(c, act);
            const unsigned long long hard = act[4 + LSQ_WALK_TRACE] + act[4 + LSQ_WALK_TRACE + 2];
            if ((double)hard * (double)c->probe_div > (double)act[0]) {      // the same arithmetic as q16_probe_kernel (option "async")
                c->chunk_road.filtered = false;
                c->filter_fallback_chunks += 1;
            }
            LSQ_TRY(run_sweeps(c, nw, vnew, cn, P.m, order, P.icmiter - probe_sweeps, totals, cur, vcur, probe_sweeps));      // the rest of a single-iteration call
        }
        {
            Timer t(c, CAT_COST);
            pn.it = P.it0 + (uint32_t)it + 1u;
            LSQ_TRY(lsq_launch_cost(c->stream, dXc, dK, nw, cur, prev, counters + 2 * it, cn, P.d, P.m, 1, vnew, vcur, it + 1 < I ? &pn : nullptr));
        }
        for (int r = 0; r < P.nr; ++r)
            if (P.ilsiters[r] == it + 1) {
                Timer t(c, CAT_OTHER);
                LSQ_TRY(lsq_launch_sum_f64(c->stream, prev, cn, c->obj.as<double>() + r));
                LSQ_TRY(snap(r, cur));
            }
    }
    return LSQ_OK;
}

static int validate_encode(const char *fn, int d, int64_t n, int m, int h, const int64_t *ilsiters, int nr, int icmiter, int npert, int64_t *I) {
    LSQ_TRY(check_shape(fn, d, n, m, h));
    if (!ilsiters || nr < 1) { lsq_set_error("%s: ilsiters must hold at least one entry", fn); return LSQ_EINVAL; }
    if (icmiter < 0 || npert < 0) { lsq_set_error("%s: icmiter and npert must be >= 0", fn); return LSQ_EINVAL; }
    *I = 0;
    for (int r = 0; r < nr; ++r) {
        if (ilsiters[r] < 1) { lsq_set_error("%s: ilsiters[%d] = %lld must be >= 1", fn, r, (long long)ilsiters[r]); return LSQ_EINVAL; }
        *I = std::max<int64_t>(*I, ilsiters[r]);
    }
    return LSQ_OK;
}

static int begin_call(lsq_ctx *c, int64_t I, int nr) {
    c->call_row0 = 0;
    c->chunk_road.resident = false;      // the per-call block (the level parameters among it) is zeroed below
    LSQ_TRY(c->counters.ensure(sizeof(unsigned long long) * 2 * (size_t)std::max<int64_t>(I, 1)));
    LSQ_TRY(c->obj.ensure(sizeof(double) * (size_t)std::max(nr, 1)));
    LSQ_TRY(c->bad.ensure(sizeof(int)));
    LSQ_TRY(c->active.ensure(sizeof(unsigned long long) * LSQ_WALK_COUNTERS));
    LSQ_TRY(c->road.ensure(2 * sizeof(unsigned)));
    LSQ_TRY(c->qp.ensure(sizeof(lsq_q16_params)));
    if (!c->async_mode) LSQ_TRY(fold_pending(c));             // statistics an earlier async call left on the device (synchronises)
    c->small_packed = c->counters.view && c->obj.view && c->bad.view && c->qp.view && c->active.view && c->road.view;
    if (c->small_packed) {
        // one fill: counters, sums, flags, level parameters (+ the walk counters and the road words unless async calls are still accumulating)
        LSQ_HIP(hipMemsetAsync(c->small.p, 0, c->pending_fold ? SMALL_ACTIVE : SMALL_READ_END, c->stream));
        return LSQ_OK;
    }
    if (!c->pending_fold) {                                  // consecutive async calls accumulate: folded by the next synchronising entry point
        LSQ_HIP(hipMemsetAsync(c->active.p, 0, sizeof(unsigned long long) * LSQ_WALK_COUNTERS, c->stream));
        LSQ_HIP(hipMemsetAsync(c->road.p, 0, 2 * sizeof(unsigned), c->stream));
    }
    LSQ_HIP(hipMemsetAsync(c->counters.p, 0, sizeof(unsigned long long) * 2 * (size_t)std::max<int64_t>(I, 1), c->stream));
    LSQ_HIP(hipMemsetAsync(c->obj.p, 0, sizeof(double) * (size_t)std::max(nr, 1), c->stream));
    LSQ_HIP(hipMemsetAsync(c->bad.p, 0, sizeof(int), c->stream));
    LSQ_HIP(hipMemsetAsync(c->qp.p, 0, sizeof(lsq_q16_params), c->stream));      // the level parameters' per-call counter (oor): the packed fill above covers it
    return LSQ_OK;
}

static void fold_walk_counters(lsq_ctx *c, const unsigned long long *act) {
    c->icm_node_updates += (int64_t)act[0];
    c->staged_blocks += (int64_t)act[1];
    c->light_blocks += (int64_t)act[2];
    c->filtered_blocks += (int64_t)act[3];
    c->filter_refined += (int64_t)act[4 + LSQ_WALK_TRACE];
    c->filter_exact += (int64_t)act[4 + LSQ_WALK_TRACE + 1];
    c->filter_f32 += (int64_t)act[4 + LSQ_WALK_TRACE + 2];
    for (int q = 0; q < LSQ_WALK_TRACE; ++q) c->trace[q] += (int64_t)act[4 + q];
}

// statistics of async calls (walk counters, chunks handed to the f32 walk) are still on the device: read, fold, clear -- synchronises the stream
static int fold_pending(lsq_ctx *c) {
    if (!c->pending_fold) return LSQ_OK;
    c->pending_fold = false;
    unsigned long long act[LSQ_WALK_COUNTERS] = {0};
    unsigned road[2] = {0u, 0u};
    LSQ_HIP(hipMemcpyAsync(act, c->active.p, sizeof(act), hipMemcpyDeviceToHost, c->stream));
    LSQ_HIP(hipMemcpyAsync(road, c->road.p, sizeof(road), hipMemcpyDeviceToHost, c->stream));
    LSQ_HIP(hipMemsetAsync(c->active.p, 0, sizeof(act), c->stream));
    LSQ_HIP(hipMemsetAsync(c->road.as<unsigned>() + 1, 0, sizeof(unsigned), c->stream));
    LSQ_HIP(hipStreamSynchronize(c->stream));
    fold_walk_counters(c, act);
    c->filter_fallback_chunks += (int64_t)road[1];
    return LSQ_OK;
}

static int finish_call(lsq_ctx *c, int64_t I, int nr, double *obj_sums, int64_t *stats) {
    if (c->async_mode) {
        // nothing waits: the sums and counters travel to the caller's buffers (device memory, or pinned host memory) in stream order
        LSQ_HIP(hipMemcpyAsync(obj_sums, c->obj.p, sizeof(double) * (size_t)nr, hipMemcpyDefault, c->stream));
        if (stats) LSQ_HIP(hipMemcpyAsync(stats, c->counters.p, sizeof(unsigned long long) * 2 * (size_t)I, hipMemcpyDefault, c->stream));      // counts < 2^63: the same bits as int64
        c->pending_fold = true;
        return LSQ_OK;
    }
    if (c->small_packed) {                                   // one copy of the block into pinned memory
        LSQ_HIP(hipMemcpyAsync(c->small_host, c->small.p, SMALL_READ_END, hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipStreamSynchronize(c->stream));
        memcpy(obj_sums, c->small_host + SMALL_OBJ, sizeof(double) * (size_t)nr);
        unsigned long long act[LSQ_WALK_COUNTERS];
        memcpy(act, c->small_host + SMALL_ACTIVE, sizeof(act));
        fold_walk_counters(c, act);
        if (stats) {
            const unsigned long long *cnt = reinterpret_cast<const unsigned long long *>(c->small_host + SMALL_COUNTERS);
            for (int64_t q = 0; q < 2 * I; ++q) stats[q] = (int64_t)cnt[q];
        }
        return LSQ_OK;
    }
    std::vector<unsigned long long> cnt(2 * (size_t)std::max<int64_t>(I, 1));
    LSQ_HIP(hipMemcpyAsync(obj_sums, c->obj.p, sizeof(double) * (size_t)nr, hipMemcpyDeviceToHost, c->stream));
    LSQ_HIP(hipMemcpyAsync(cnt.data(), c->counters.p, sizeof(unsigned long long) * cnt.size(), hipMemcpyDeviceToHost, c->stream));
    unsigned long long act[LSQ_WALK_COUNTERS] = {0};
    LSQ_HIP(hipMemcpyAsync(act, c->active.p, sizeof(act), hipMemcpyDeviceToHost, c->stream));
    LSQ_HIP(hipStreamSynchronize(c->stream));
    fold_walk_counters(c, act);
    if (stats) for (int64_t q = 0; q < 2 * I; ++q) stats[q] = (int64_t)cnt[(size_t)q];
    return LSQ_OK;
}

template <class XT>
static int encode_dev(lsq_ctx *c, const char *fn, const XT *dX, const uint8_t *dB0, const float *dK, int d, int64_t n, int m, int h,
                      const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, uint64_t seed,
                      uint64_t global_offset, uint8_t *dBs, double *obj_sums, int64_t *stats) {
    LSQ_TRY(use_device(c));
    int64_t I = 0;
    LSQ_TRY(validate_encode(fn, d, n, m, h, ilsiters, nr, icmiter, npert, &I));
    if (!dK || !obj_sums || (n > 0 && (!dX || !dB0 || !dBs))) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    LSQ_TRY(begin_call(c, I, nr));
    LSQ_TRY(prepare_tables(c, dK, d, m));
    const EncodeParams P{d, m, ilsiters, nr, icmiter, npert, randord, seed, 0u};
    const int cs = lsq_code_stride(m);
    for (int64_t off = 0; off < n; off += c->chunk) {
        const int64_t cn = std::min<int64_t>(c->chunk, n - off);
        c->call_row0 = off;
        LSQ_TRY(c->recCur.ensure((size_t)cn * cs));
        {
            Timer t(c, CAT_OTHER);
            LSQ_TRY(lsq_launch_codes_expand(c->stream, dB0 + off * m, cn, m, c->recCur.as<uint8_t>()));
        }
        auto snap = [&](int r, const uint8_t *cur) {
            return lsq_launch_codes_compact(c->stream, cur, cn, m, dBs + ((int64_t)r * n + off) * m);
        };
        LSQ_TRY(encode_chunk(c, dX + off * d, dK, cn, global_offset + (uint64_t)off, P, I, snap));
    }
    return finish_call(c, I, nr, obj_sums, stats);
}

extern "C" int lsq_encode_icm_dev(lsq_ctx *c, const float *dX, const uint8_t *dB0, const float *dK, int d, int64_t n, int m, int h,
                                  const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, uint64_t seed,
                                  uint64_t global_offset, uint8_t *dBs, double *obj_sums, int64_t *stats) {
    return encode_dev(c, "lsq_encode_icm_dev", dX, dB0, dK, d, n, m, h, ilsiters, nr, icmiter, npert, randord, seed, global_offset, dBs, obj_sums, stats);
}

// 8-bit data rows, device-resident (stands in for lsq_encode_icm_dev on the widened matrix: same codes, same sums, same counters; option "async" included)
extern "C" int lsq_encode_icm_u8_dev(lsq_ctx *c, const uint8_t *dX8, const uint8_t *dB0, const float *dK, int d, int64_t n, int m, int h,
                                     const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, uint64_t seed,
                                     uint64_t global_offset, uint8_t *dBs, double *obj_sums, int64_t *stats) {
    return encode_dev(c, "lsq_encode_icm_u8_dev", dX8, dB0, dK, d, n, m, h, ilsiters, nr, icmiter, npert, randord, seed, global_offset, dBs, obj_sums, stats);
}

// sK is claimed for this call -- as an input (K uploaded here, or K_prev by stage()) or as an output (LSQR, SPGL1, the seeding).  The ONE place that drops
// the host-table cache because sK changes.  It is the first thing such a call does that can fail: from here on sK / the tables are in flux, and a failure
// must not leave the cache claiming the OLD codebooks
static size_t codebook_bytes(int d, int m) { return sizeof(float) * (size_t)m * LSQ_H * d; }
static int claim_sK(lsq_ctx *c, int d, int m, const float *K = nullptr) {
    c->tables_valid = false;        // sK is about to hold other codebooks than the cached tables were built from
    LSQ_TRY(c->sK.ensure(codebook_bytes(d, m)));
    if (K) LSQ_HIP(hipMemcpyAsync(c->sK.p, K, codebook_bytes(d, m), hipMemcpyHostToDevice, c->stream));
    return LSQ_OK;
}

// The caller's host codebooks -> c->sK + tables.  Unchanged since the last host-buffer call of this context (same shape, same bytes): nothing is
// uploaded or rebuilt.
static int host_codebooks(lsq_ctx *c, const float *K, int d, int m) {
    const size_t count = (size_t)m * LSQ_H * d, kbytes = sizeof(float) * count;
    if (c->tables_valid && c->hostK_d == d && c->hostK_m == m && c->hostK.size() == count && memcmp(c->hostK.data(), K, kbytes) == 0) {
        c->table_reuses += 1;
        return LSQ_OK;
    }
    LSQ_TRY(claim_sK(c, d, m, K));
    LSQ_TRY(prepare_tables(c, c->sK.as<float>(), d, m));
    c->hostK.assign(K, K + count);        // (the pageable copy above has read K by the time it returns)
    c->hostK_d = d; c->hostK_m = m;
    c->tables_valid = true;
    return LSQ_OK;
}

// host-buffer core shared by lsq_encode_icm / lsq_encoding_icm
// `place` (multi-GPU shards): the shard's rows go to rows [row0, row0 + n) of snapshots that are ntot rows long, and the
// objective sums / counters are handed back raw so that the caller can combine the shards.
struct HostPlacement { int64_t ntot, row0; double *sums; int64_t *stats; };

template <class XT>
static int encode_host(lsq_ctx *c, const char *fn, const XT *X, const int16_t *B, const float *K, int d, int64_t n, int m, int h,
                       const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, uint64_t seed, uint32_t it0,
                       uint64_t global_offset, int verbose, int16_t *Bs, float *objs, const HostPlacement *place = nullptr) {
    LSQ_TRY(use_device(c));
    const AsyncOff sync_here(c);
    int64_t I = 0;
    LSQ_TRY(validate_encode(fn, d, n, m, h, ilsiters, nr, icmiter, npert, &I));
    if (!K || (!objs && !place) || (n > 0 && (!X || !B || !Bs))) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    const int64_t ntot = place ? place->ntot : n, row0 = place ? place->row0 : 0;
    LSQ_TRY(begin_call(c, I, nr));
    LSQ_TRY(host_codebooks(c, K, d, m));
    const float *dK = c->sK.as<float>();
    // The ONE range check of the input codes (1..h): a host scan, hidden under the table kernels just enqueued and done before anything
    // reads B or writes Bs -- an invalid call never touches the caller's output and the codes are not checked twice (ADVICE r2:
    // the device flag of codes_from_i16_kernel is only consulted by the fine-grained entry points, which have no host scan).
    {
        const int rc = check_codes_host(fn, B, n, m, h);
        if (rc != LSQ_OK) {      // the copy of K and the table kernels are in flight: the caller's K must not be read after this returns
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    const EncodeParams P{d, m, ilsiters, nr, icmiter, npert, randord, seed, it0};
    const int cs = lsq_code_stride(m);
    // Chunk c+1's X is uploaded on a second stream under the ILS iterations of chunk c (double-buffered staging).  The FIRST
    // chunk of a call goes up panel by panel under its own unary GEMM when it is at least upload_pipeline_min_bytes long
    // (build_unaries_from_host, round 5), else through the compute stream in one piece.
    if (n > c->chunk) {
        if (!c->copy_stream) LSQ_HIP(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        if (!c->copy_done) LSQ_HIP(hipEventCreateWithFlags(&c->copy_done, hipEventDisableTiming));
    }
    DevBuf *xb[2] = {&c->sX, &c->sX2};
    int which = 0;
    for (int64_t off = 0; off < n; off += c->chunk, which ^= 1) {
        const int64_t cn = std::min<int64_t>(c->chunk, n - off);
        c->call_row0 = off;
        LSQ_TRY(xb[which]->ensure(sizeof(XT) * (size_t)cn * d));
        LSQ_TRY(c->sB16.ensure(sizeof(int16_t) * (size_t)cn * m));
        LSQ_TRY(c->sOut16.ensure(sizeof(int16_t) * (size_t)cn * m * nr));
        LSQ_TRY(c->recCur.ensure((size_t)cn * cs));
        XT *dXc = xb[which]->as<XT>();
        const bool piped = off == 0 && c->pipeline_min_bytes > 0 && (int64_t)sizeof(XT) * cn * d >= c->pipeline_min_bytes;
        if (piped) {}                                                       // X goes up panel by panel under its own unary GEMM (below)
        else if (off == 0) LSQ_HIP(hipMemcpyAsync(dXc, X, sizeof(XT) * (size_t)cn * d, hipMemcpyHostToDevice, c->stream));
        else LSQ_HIP(hipStreamWaitEvent(c->stream, c->copy_done, 0));      // uploaded under the previous chunk's compute
        LSQ_HIP(hipMemcpyAsync(c->sB16.p, B + off * m, sizeof(int16_t) * (size_t)cn * m, hipMemcpyHostToDevice, c->stream));
        LSQ_TRY(lsq_launch_codes_from_i16(c->stream, c->sB16.as<int16_t>(), cn, m, h, c->recCur.as<uint8_t>(), c->bad.as<int>()));
        auto snap = [&](int r, const uint8_t *cur) {
            return lsq_launch_codes_to_i16(c->stream, cur, cn, m, c->sOut16.as<int16_t>() + (int64_t)r * cn * m);
        };
        if (piped) LSQ_TRY(build_unaries_from_host(c, X, dXc, dK, d, cn, m, lsq_walk_slice_width(m)));
        LSQ_TRY(encode_chunk(c, dXc, dK, cn, global_offset + (uint64_t)off, P, I, snap, piped));
        const int64_t noff = off + c->chunk;
        if (noff < n) {      // next chunk's X: its buffer was last read by chunk c-1, which completed at the previous synchronize
            const int64_t ncn = std::min<int64_t>(c->chunk, n - noff);
            LSQ_TRY(xb[which ^ 1]->ensure(sizeof(XT) * (size_t)ncn * d));
            LSQ_HIP(hipMemcpyAsync(xb[which ^ 1]->p, X + noff * d, sizeof(XT) * (size_t)ncn * d, hipMemcpyHostToDevice, c->copy_stream));
            LSQ_HIP(hipEventRecord(c->copy_done, c->copy_stream));
        }
        for (int r = 0; r < nr; ++r)
            LSQ_HIP(hipMemcpyAsync(Bs + ((int64_t)r * ntot + row0 + off) * m, c->sOut16.as<int16_t>() + (int64_t)r * cn * m,
                                   sizeof(int16_t) * (size_t)cn * m, hipMemcpyDeviceToHost, c->stream));
        LSQ_HIP(hipStreamSynchronize(c->stream));      // staging buffers are reused by the next chunk
    }
    std::vector<double> sums((size_t)nr, 0.0);
    std::vector<int64_t> stats(2 * (size_t)I, 0);
    LSQ_TRY(finish_call(c, I, nr, sums.data(), stats.data()));
    if (place) {
        for (int r = 0; r < nr; ++r) place->sums[r] = sums[(size_t)r];
        if (place->stats) for (size_t q = 0; q < stats.size(); ++q) place->stats[q] = stats[q];
        return LSQ_OK;
    }
    for (int r = 0; r < nr; ++r) objs[r] = (float)(n > 0 ? sums[(size_t)r] / (double)n : 0.0);
    if (verbose)
        for (int64_t it = 0; it < I; ++it)      // the two counters the reference prints (encode_icm_cuda.jl:199-204)
            printf(" ILS iteration %lld/%lld done. %5.2f%% new codes are equal. %5.2f%% new codes are better.\n", (long long)(it + 1),
                   (long long)I, n ? 100.0 * (double)stats[2 * it] / (double)n : 0.0, n ? 100.0 * (double)stats[2 * it + 1] / (double)n : 0.0);
    return LSQ_OK;
}

extern "C" int lsq_encode_icm(lsq_ctx *c, const float *RX, const int16_t *B, const float *K, int d, int64_t n, int m, int h,
                              const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, int nsplits, uint64_t seed,
                              uint64_t global_offset, int verbose, int16_t *Bs, float *objs) {
    if (nsplits < 1) { lsq_set_error("lsq_encode_icm: nsplits must be >= 1"); return LSQ_EINVAL; }
    return encode_host(c, "lsq_encode_icm", RX, B, K, d, n, m, h, ilsiters, nr, icmiter, npert, randord, seed, 0u, global_offset, verbose, Bs, objs);
}

// 8-bit data rows in host memory (stands in for lsq_encode_icm on the widened matrix): d bytes per row over the bus and in the chunk buffers
extern "C" int lsq_encode_icm_u8(lsq_ctx *c, const uint8_t *RX8, const int16_t *B, const float *K, int d, int64_t n, int m, int h,
                                 const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, int nsplits, uint64_t seed,
                                 uint64_t global_offset, int verbose, int16_t *Bs, float *objs) {
    if (nsplits < 1) { lsq_set_error("lsq_encode_icm_u8: nsplits must be >= 1"); return LSQ_EINVAL; }
    return encode_host(c, "lsq_encode_icm_u8", RX8, B, K, d, n, m, h, ilsiters, nr, icmiter, npert, randord, seed, 0u, global_offset, verbose, Bs, objs);
}

// ---- single-process multi-GPU: one context + one host thread per device, splitarray shards (utils.jl:152-177) -------
struct lsq_multi { std::vector<lsq_ctx *> ctx; };

extern "C" int lsq_multi_create(lsq_multi **out, const int *devices, int ndev) {
    if (!out || !devices || ndev < 1) { lsq_set_error("lsq_multi_create: need an output pointer and at least one device"); return LSQ_EINVAL; }
    *out = nullptr;
    lsq_multi *mg = new lsq_multi();
    for (int p = 0; p < ndev; ++p) {
        lsq_ctx *c = nullptr;
        const int rc = lsq_create(&c, devices[p]);
        if (rc != LSQ_OK) {
            for (lsq_ctx *q : mg->ctx) (void)lsq_destroy(q);
            delete mg;
            return rc;
        }
        mg->ctx.push_back(c);
    }
    *out = mg;
    return LSQ_OK;
}

extern "C" int lsq_multi_destroy(lsq_multi *mg) {
    if (!mg) return LSQ_OK;
    for (lsq_ctx *q : mg->ctx) (void)lsq_destroy(q);
    delete mg;
    return LSQ_OK;
}

extern "C" int lsq_multi_set_option(lsq_multi *mg, const char *key, int64_t value) {
    if (!mg) { lsq_set_error("null lsq_multi"); return LSQ_EINVAL; }
    for (lsq_ctx *q : mg->ctx) LSQ_TRY(lsq_set_option(q, key, value));
    return LSQ_OK;
}

template <class XT>
static int multi_encode(lsq_multi *mg, const char *fn, const XT *RX, const int16_t *B, const float *K, int d, int64_t n, int m, int h,
                        const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, uint64_t seed,
                        uint64_t global_offset, int verbose, int16_t *Bs, float *objs) {
    if (!mg || mg->ctx.empty()) { lsq_set_error("null lsq_multi"); return LSQ_EINVAL; }
    int64_t I = 0;
    LSQ_TRY(validate_encode(fn, d, n, m, h, ilsiters, nr, icmiter, npert, &I));
    if (!K || !objs || (n > 0 && (!RX || !B || !Bs))) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    const int G = (int)mg->ctx.size();
    std::vector<std::vector<double>> sums((size_t)G, std::vector<double>((size_t)nr, 0.0));
    std::vector<std::vector<int64_t>> stats((size_t)G, std::vector<int64_t>(2 * (size_t)I, 0));
    std::vector<int> rc((size_t)G, LSQ_OK);
    std::vector<std::string> err((size_t)G);
    std::vector<std::thread> th;
    for (int p = 0; p < G; ++p) {
        th.emplace_back([&, p]() {
            int64_t s0 = 0, len = 0;
            rc[(size_t)p] = lsq_splitarray(n, G, p, &s0, &len);        // contiguous shards, the first n mod G one longer
            if (rc[(size_t)p] == LSQ_OK && len > 0) {
                const HostPlacement place{n, s0, sums[(size_t)p].data(), stats[(size_t)p].data()};
                rc[(size_t)p] = encode_host(mg->ctx[(size_t)p], fn, RX + s0 * d, B + s0 * m, K, d, len, m, h, ilsiters, nr,
                                            icmiter, npert, randord, seed, 0u, global_offset + (uint64_t)s0, 0, Bs, nullptr, &place);
            }
            if (rc[(size_t)p] != LSQ_OK) err[(size_t)p] = lsq_last_error();      // the error string is thread-local
        });
    }
    for (auto &t : th) t.join();
    for (int p = 0; p < G; ++p)
        if (rc[(size_t)p] != LSQ_OK) { lsq_set_error("device shard %d: %s", p, err[(size_t)p].c_str()); return rc[(size_t)p]; }
    for (int r = 0; r < nr; ++r) {
        double tot = 0.0;
        for (int p = 0; p < G; ++p) tot += sums[(size_t)p][(size_t)r];
        objs[r] = (float)(n > 0 ? tot / (double)n : 0.0);
    }
    if (verbose)
        for (int64_t it = 0; it < I; ++it) {
            int64_t eq = 0, better = 0;
            for (int p = 0; p < G; ++p) { eq += stats[(size_t)p][2 * (size_t)it]; better += stats[(size_t)p][2 * (size_t)it + 1]; }
            printf(" ILS iteration %lld/%lld done. %5.2f%% new codes are equal. %5.2f%% new codes are better.\n", (long long)(it + 1),
                   (long long)I, n ? 100.0 * (double)eq / (double)n : 0.0, n ? 100.0 * (double)better / (double)n : 0.0);
        }
    return LSQ_OK;
}

extern "C" int lsq_multi_encode_icm(lsq_multi *mg, const float *RX, const int16_t *B, const float *K, int d, int64_t n, int m, int h,
                                    const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, uint64_t seed,
                                    uint64_t global_offset, int verbose, int16_t *Bs, float *objs) {
    return multi_encode(mg, "lsq_multi_encode_icm", RX, B, K, d, n, m, h, ilsiters, nr, icmiter, npert, randord, seed, global_offset, verbose, Bs, objs);
}

// 8-bit data rows (stands in for lsq_multi_encode_icm on the widened matrix)
extern "C" int lsq_multi_encode_icm_u8(lsq_multi *mg, const uint8_t *RX8, const int16_t *B, const float *K, int d, int64_t n, int m, int h,
                                       const int64_t *ilsiters, int nr, int icmiter, int npert, int randord, uint64_t seed,
                                       uint64_t global_offset, int verbose, int16_t *Bs, float *objs) {
    return multi_encode(mg, "lsq_multi_encode_icm_u8", RX8, B, K, d, n, m, h, ilsiters, nr, icmiter, npert, randord, seed, global_offset, verbose, Bs, objs);
}

// The ADC scan over a database sharded across the devices (splitarray shards, one host thread per device): every device returns its own nn nearest
// (fewer if its shard is smaller), ids become global, and the host merges the lists by (distance, id) -- std::pair's order, the reference's
// partial_sort order -- so the result is what ONE scan of the whole database returns, ties across shards included.
extern "C" int lsq_multi_linscan(lsq_multi *mg, float *dists, int *idx, const unsigned char *codes, const float *queries, const float *codebooks,
                                 const float *dbnorms, int nqueries, int ncodes, int m, int h, int d, int nn) {
    if (!mg || mg->ctx.empty()) { lsq_set_error("null lsq_multi"); return LSQ_EINVAL; }
    LSQ_TRY(linscan_check("lsq_multi_linscan", dists, idx, codes, queries, codebooks, dbnorms, nqueries, ncodes, m, h, d, nn));
    if (nqueries == 0) return LSQ_OK;
    const int G = (int)mg->ctx.size();
    std::vector<std::vector<float>> pd((size_t)G);
    std::vector<std::vector<int>> pi((size_t)G);
    std::vector<int> klen((size_t)G, 0), rc((size_t)G, LSQ_OK);
    std::vector<int64_t> start((size_t)G, 0);
    std::vector<std::string> err((size_t)G);
    std::vector<std::thread> th;
    for (int p = 0; p < G; ++p) {
        th.emplace_back([&, p]() {
            int64_t s0 = 0, len = 0;
            rc[(size_t)p] = lsq_splitarray(ncodes, G, p, &s0, &len);
            start[(size_t)p] = s0;
            if (rc[(size_t)p] != LSQ_OK || len == 0) return;
            const int k = (int)std::min<int64_t>(nn, len);
            klen[(size_t)p] = k;
            pd[(size_t)p].resize((size_t)nqueries * k);
            pi[(size_t)p].resize((size_t)nqueries * k);
            rc[(size_t)p] = lsq_linscan(mg->ctx[(size_t)p], pd[(size_t)p].data(), pi[(size_t)p].data(), codes + s0 * m, queries, codebooks, dbnorms + s0,
                                        nqueries, (int)len, m, h, d, k);
            if (rc[(size_t)p] != LSQ_OK) err[(size_t)p] = lsq_last_error();      // the error string is thread-local
        });
    }
    for (auto &t : th) t.join();
    for (int p = 0; p < G; ++p)
        if (rc[(size_t)p] != LSQ_OK) { lsq_set_error("device shard %d: %s", p, err[(size_t)p].c_str()); return rc[(size_t)p]; }
    // G-way merge per query; the lists are sorted by (distance, local id) and the shards are contiguous id ranges: (distance, global id) order
    // inside a list is the same.  NaN distances (sorted last by the device scan) lose every comparison here as well.
    auto less = [](float da, int ia, float db, int ib) {
        const bool na = da != da, nb = db != db;
        if (na != nb) return nb;
        if (!na && da != db) return da < db;
        return ia < ib;
    };
    const int nt = std::max(1, std::min<int>((int)std::thread::hardware_concurrency(), nqueries));
    std::vector<std::thread> mt;
    for (int t = 0; t < nt; ++t) {
        mt.emplace_back([&, t]() {
            std::vector<int> pos((size_t)G);
            for (int q = (int)((int64_t)nqueries * t / nt); q < (int)((int64_t)nqueries * (t + 1) / nt); ++q) {
                std::fill(pos.begin(), pos.end(), 0);
                for (int r = 0; r < nn; ++r) {
                    int best = -1;
                    float bd = 0.0f;
                    int bi = 0;
                    for (int p = 0; p < G; ++p) {
                        if (pos[(size_t)p] >= klen[(size_t)p]) continue;
                        const size_t e = (size_t)q * klen[(size_t)p] + (size_t)pos[(size_t)p];
                        const float dd = pd[(size_t)p][e];
                        const int ii = pi[(size_t)p][e] + (int)start[(size_t)p];
                        if (best < 0 || less(dd, ii, bd, bi)) { best = p; bd = dd; bi = ii; }
                    }
                    dists[(size_t)q * nn + r] = bd;
                    idx[(size_t)q * nn + r] = bi;
                    pos[(size_t)best] += 1;
                }
            }
        });
    }
    for (auto &t : mt) t.join();
    return LSQ_OK;
}

extern "C" int lsq_encoding_icm(lsq_ctx *c, const float *X, const int16_t *oldB, const float *K, int d, int64_t n, int m, int h,
                                int niter, int randord, int npert, uint64_t seed, uint32_t it, uint64_t global_offset, int16_t *outB) {
    const int64_t one = 1;
    float obj = 0.f;
    if (!c) { lsq_set_error("null lsq_ctx"); return LSQ_EINVAL; }
    // it = LSQ_IT_AUTO: the reference's caller keeps no iteration count (demos/demo_lsq.jl:48-51 just loops) -- the context does, so that
    // successive calls draw different perturbations; it advances only when the call succeeded
    const bool autoit = it == LSQ_IT_AUTO;
    const int rc = encode_host(c, "lsq_encoding_icm", X, oldB, K, d, n, m, h, &one, 1, niter, npert, randord, seed, autoit ? c->auto_it : it,
                               global_offset, 0, outB, &obj);
    if (rc == LSQ_OK && autoit && c->auto_it < LSQ_IT_AUTO - 1u) ++c->auto_it;
    return rc;
}

// ---- host-buffer calls (everything below that is neither the pipelined encode nor a search) ---------------------------------------------------------------
// A host form is: checks -> stage -> its launch sequence on device pointers -> fetch -> ONE wait.  The functions up to fetch_codes() are the
// stage / fetch / wait part (with claim_sK, next to host_codebooks); which buffer they fill is listed at lsq_ctx's staging buffers.

// what an entry checks first: the context, the shape, then `ok` (its pointers and counts)
static int entry_args(const char *fn, lsq_ctx *c, int d, int64_t n, int m, int h, bool ok, const char *what = "null pointer") {
    LSQ_TRY(use_device(c));
    LSQ_TRY(check_shape(fn, d, n, m, h));
    if (!ok) { lsq_set_error("%s: %s", fn, what); return LSQ_EINVAL; }
    return LSQ_OK;
}

static int stage_X(lsq_ctx *c, const float *X, int d, int64_t n) {        // -> sX, sized for at least one row; no rows, no copy
    LSQ_TRY(c->sX.ensure(sizeof(float) * (size_t)std::max<int64_t>(n, 1) * d));
    if (n > 0) LSQ_HIP(hipMemcpyAsync(c->sX.p, X, sizeof(float) * (size_t)n * d, hipMemcpyHostToDevice, c->stream));
    return LSQ_OK;
}

// The caller's int16 1-based codes -> records in recCur [, and tight [n][m] in sTight], range-checked on the device.  The wait that reads the verdict is here:
// a call with a bad code returns before any kernel of its own work is enqueued and before any output is written
static int stage_codes(lsq_ctx *c, const int16_t *B, int64_t n, int m, int h, bool tight = false) {
    LSQ_TRY(c->sB16.ensure(sizeof(int16_t) * (size_t)std::max<int64_t>(n, 1) * m));
    LSQ_TRY(c->recCur.ensure((size_t)std::max<int64_t>(n, 1) * lsq_code_stride(m)));
    LSQ_TRY(c->bad.ensure(sizeof(int)));
    LSQ_HIP(hipMemsetAsync(c->bad.p, 0, sizeof(int), c->stream));
    if (n > 0) {
        LSQ_HIP(hipMemcpyAsync(c->sB16.p, B, sizeof(int16_t) * (size_t)n * m, hipMemcpyHostToDevice, c->stream));
        LSQ_TRY(lsq_launch_codes_from_i16(c->stream, c->sB16.as<int16_t>(), n, m, h, c->recCur.as<uint8_t>(), c->bad.as<int>()));
    }
    int bad = 0;
    LSQ_HIP(hipMemcpyAsync(&bad, c->bad.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSQ_HIP(hipStreamSynchronize(c->stream));
    if (bad) { lsq_set_error("input codes must lie in 1..%d", h); return LSQ_ECODE; }
    if (tight) LSQ_TRY(c->sTight.ensure((size_t)std::max<int64_t>(n, 1) * m));
    if (tight && n > 0) LSQ_TRY(lsq_launch_codes_compact(c->stream, c->recCur.as<uint8_t>(), n, m, c->sTight.as<uint8_t>()));
    return LSQ_OK;
}

// sF32 is a call's block of small arrays: the slices the call names, in the order given, each on a 16-byte boundary.  A call carves ONCE (a second carve may
// move the block) and says in that line what its slices hold
struct Slice { size_t bytes; void *p = nullptr; template <class T> T *as() const { return static_cast<T *>(p); } };
static int carve_f32(lsq_ctx *c, std::initializer_list<Slice *> slices) {
    size_t total = 0;
    for (Slice *s : slices) total += (s->bytes + 15) & ~(size_t)15;
    LSQ_TRY(c->sF32.ensure(total));
    char *p = c->sF32.as<char>();
    for (Slice *s : slices) { s->p = p; p += (s->bytes + 15) & ~(size_t)15; }
    return LSQ_OK;
}

// a small array up (into a slice, or K_prev into the claimed sK); a result down -- a null dst is an output the caller did not ask for; the call's one trailing wait
static int stage(lsq_ctx *c, void *dst, const void *src, size_t bytes) { LSQ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream)); return LSQ_OK; }
static int fetch(lsq_ctx *c, void *dst, const void *src, size_t bytes) { if (dst) LSQ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); return LSQ_OK; }
static int finish(lsq_ctx *c) { LSQ_HIP(hipStreamSynchronize(c->stream)); return LSQ_OK; }

// the records in recNew (from_tight: sTight's [n][m], expanded into recNew first) -> int16 1-based in sB16 -> the caller's B
static int fetch_codes(lsq_ctx *c, int16_t *B, int64_t n, int m, bool from_tight = false) {
    LSQ_TRY(c->sB16.ensure(sizeof(int16_t) * (size_t)n * m));
    if (from_tight) LSQ_TRY(c->recNew.ensure((size_t)n * lsq_code_stride(m)));
    if (from_tight) LSQ_TRY(lsq_launch_codes_expand(c->stream, c->sTight.as<uint8_t>(), n, m, c->recNew.as<uint8_t>()));
    LSQ_TRY(lsq_launch_codes_to_i16(c->stream, c->recNew.as<uint8_t>(), n, m, c->sB16.as<int16_t>()));
    return fetch(c, B, c->sB16.p, sizeof(int16_t) * (size_t)n * m);
}

extern "C" int lsq_encode_icm_fully(lsq_ctx *c, int16_t *B, const float *X, const float *K, int d, int64_t n, int m, int h, int niter,
                                    int randord, int npert, int64_t idx_first, uint64_t seed, uint32_t it) {
    LSQ_TRY(use_device(c));
    const AsyncOff sync_here(c);
    LSQ_TRY(check_shape("lsq_encode_icm_fully", d, n, m, h));
    if (!K || niter < 0 || npert < 0 || idx_first < 1 || (n > 0 && (!B || !X))) { lsq_set_error("lsq_encode_icm_fully: bad arguments"); return LSQ_EINVAL; }
    const bool autoit = it == LSQ_IT_AUTO;      // the context's counter advances only when the call succeeds (as in lsq_encoding_icm)
    if (autoit) it = c->auto_it;
    if (n == 0) return LSQ_OK;
    if (n > c->chunk) { lsq_set_error("lsq_encode_icm_fully: n = %lld exceeds the resident chunk (%lld); raise option \"chunk\"", (long long)n, (long long)c->chunk); return LSQ_EINVAL; }
    LSQ_TRY(claim_sK(c, d, m, K));
    LSQ_TRY(stage_X(c, X, d, n));
    LSQ_TRY(stage_codes(c, B, n, m, h));
    LSQ_TRY(prepare_tables(c, c->sK.as<float>(), d, m));
    c->call_row0 = 0;
    LSQ_TRY(build_unaries(c, c->sX.as<float>(), c->sK.as<float>(), d, n, m, lsq_walk_slice_width(m), 0, n));
    LSQ_TRY(c->recNew.ensure((size_t)n * lsq_code_stride(m)));
    int32_t order[LSQ_MAX_M];
    LSQ_TRY(lsq_node_order(seed, it, m, randord, order));
    LSQ_TRY(c->vNew.ensure(sizeof(unsigned short) * (size_t)(n + 8)));
    LSQ_TRY(c->active.ensure(sizeof(unsigned long long) * LSQ_WALK_COUNTERS));
    LSQ_HIP(hipMemsetAsync(c->vNew.p, 0, sizeof(unsigned short) * (size_t)n, c->stream));
    LSQ_TRY(lsq_launch_perturb(c->stream, c->recCur.as<uint8_t>(), c->recNew.as<uint8_t>(), n, m, npert, seed, it, (uint64_t)(idx_first - 1), nullptr, nullptr));
    // (no statistics: the worker has no accept step and no probe memory -- always the configured road)
    LSQ_TRY(run_sweeps(c, c->recNew.as<uint8_t>(), c->vNew.as<unsigned short>(), n, m, order, niter, nullptr));
    LSQ_TRY(fetch_codes(c, B, n, m));
    LSQ_TRY(finish(c));
    if (autoit && c->auto_it < LSQ_IT_AUTO - 1u) ++c->auto_it;
    return LSQ_OK;
}

extern "C" int lsq_get_unaries(lsq_ctx *c, const float *X, const float *K, int d, int64_t n, int m, int h, float *U) {
    LSQ_TRY(entry_args("lsq_get_unaries", c, d, n, m, h, K && (n == 0 || (X && U))));
    if (n == 0) return LSQ_OK;
    LSQ_TRY(claim_sK(c, d, m, K));
    LSQ_TRY(stage_X(c, X, d, n));
    LSQ_TRY(c->sci.ensure(sizeof(float) * (size_t)m * LSQ_H));
    LSQ_TRY(lsq_launch_sqnorms(c->stream, c->sK.as<float>(), m * LSQ_H, d, c->sci.as<float>()));
    LSQ_TRY(build_unaries(c, c->sX.as<float>(), c->sK.as<float>(), d, n, m, 0, 0, n));
    LSQ_TRY(fetch(c, U, c->U.p, sizeof(float) * (size_t)m * n * LSQ_H));
    return finish(c);
}

extern "C" int lsq_get_binaries(lsq_ctx *c, const float *K, int d, int m, int h, float *T) {
    LSQ_TRY(entry_args("lsq_get_binaries", c, d, 0, m, h, K && T));
    LSQ_TRY(claim_sK(c, d, m, K));
    LSQ_TRY(prepare_tables(c, c->sK.as<float>(), d, m));
    LSQ_TRY(fetch(c, T, c->T.p, sizeof(float) * (size_t)m * m * LSQ_H * LSQ_H));
    return finish(c);
}

// veccost and qerror: K, X and the codes up, then the cost of the staged records -> prev[n]
static int cost_of_staged(lsq_ctx *c, const float *X, const int16_t *B, const float *K, int d, int64_t n, int m, int h) {
    LSQ_TRY(claim_sK(c, d, m, K));
    LSQ_TRY(stage_X(c, X, d, n));
    LSQ_TRY(stage_codes(c, B, n, m, h));
    LSQ_TRY(c->prev.ensure(sizeof(float) * (size_t)n));
    return lsq_launch_cost(c->stream, c->sX.as<float>(), c->sK.as<float>(), c->recCur.as<uint8_t>(), c->recCur.as<uint8_t>(), c->prev.as<float>(), nullptr, n, d,
                           m, 0, nullptr, nullptr);
}

extern "C" int lsq_veccost(lsq_ctx *c, const float *X, const int16_t *B, const float *K, int d, int64_t n, int m, int h, float *cost) {
    LSQ_TRY(entry_args("lsq_veccost", c, d, n, m, h, K && (n == 0 || (X && B && cost))));
    if (n == 0) return LSQ_OK;
    LSQ_TRY(cost_of_staged(c, X, B, K, d, n, m, h));
    LSQ_TRY(fetch(c, cost, c->prev.p, sizeof(float) * (size_t)n));
    return finish(c);
}

extern "C" int lsq_qerror(lsq_ctx *c, const float *X, const int16_t *B, const float *K, int d, int64_t n, int m, int h, double *out) {
    LSQ_TRY(entry_args("lsq_qerror", c, d, n, m, h, out && K && (n == 0 || (X && B))));
    *out = 0.0;
    if (n == 0) return LSQ_OK;
    LSQ_TRY(c->obj.ensure(sizeof(double)));
    LSQ_TRY(cost_of_staged(c, X, B, K, d, n, m, h));
    LSQ_HIP(hipMemsetAsync(c->obj.p, 0, sizeof(double), c->stream));
    LSQ_TRY(lsq_launch_sum_f64(c->stream, c->prev.as<float>(), n, c->obj.as<double>()));
    double sum = 0.0;
    LSQ_TRY(fetch(c, &sum, c->obj.p, sizeof(double)));
    LSQ_TRY(finish(c));
    *out = sum / (double)n;
    return LSQ_OK;
}

extern "C" int lsq_perturb(lsq_ctx *c, int16_t *B, int64_t n, int m, int h, int npert, uint64_t seed, uint32_t it, uint64_t global_offset) {
    LSQ_TRY(entry_args("lsq_perturb", c, 1, n, m, h, npert >= 0 && (n == 0 || B), "bad arguments"));
    if (n == 0) return LSQ_OK;
    LSQ_TRY(stage_codes(c, B, n, m, h));
    LSQ_TRY(c->recNew.ensure((size_t)n * lsq_code_stride(m)));
    LSQ_TRY(lsq_launch_perturb(c->stream, c->recCur.as<uint8_t>(), c->recNew.as<uint8_t>(), n, m, npert, seed, it, global_offset, nullptr, nullptr));
    LSQ_TRY(fetch_codes(c, B, n, m));
    return finish(c);
}

// ---- the pairs: a host form and its _dev twin are ONE function.  `host` says which memory its pointers name -- and which codes: int16 1-based in host
// memory, tight uint8 0-based on the device.  The checks come first, in the order both forms have always had; then the host form stages, both launch the
// same sequence on device pointers, and the host form fetches and waits. -------------------------------------------------------------------------------------
static int quantize_norms(const char *fn, lsq_ctx *c, bool host, const void *codes, const float *K, const float *cbnorms, int ncb, int d, int64_t n, int m, int h,
                          void *idx_out, float *dbnorms, float *norms) {
    LSQ_TRY(use_device(c));
    LSQ_TRY(check_shape(fn, d, n, m, h));
    if (ncb < 1 || ncb > LSQ_H) { lsq_set_error("%s: ncb=%d must lie in 1..256", fn, ncb); return LSQ_EINVAL; }
    if (!K || !cbnorms || (n > 0 && !codes)) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (!host) return lsq_launch_quantize_norms(c->stream, static_cast<const uint8_t *>(codes), m, K, cbnorms, ncb, n, d, m, static_cast<uint8_t *>(idx_out), nullptr, dbnorms, norms);
    if (n == 0) return LSQ_OK;
    Slice cb{sizeof(float) * LSQ_H}, db{sizeof(float) * (size_t)n}, nr{sizeof(float) * (size_t)n};      // sF32: the norm table | dbnorms | norms
    LSQ_TRY(claim_sK(c, d, m, K));
    LSQ_TRY(stage_codes(c, static_cast<const int16_t *>(codes), n, m, h));
    LSQ_TRY(carve_f32(c, {&cb, &db, &nr}));
    LSQ_TRY(c->sOut16.ensure(sizeof(int16_t) * (size_t)n));
    LSQ_TRY(stage(c, cb.p, cbnorms, sizeof(float) * (size_t)ncb));
    LSQ_TRY(lsq_launch_quantize_norms(c->stream, c->recCur.as<uint8_t>(), lsq_code_stride(m), c->sK.as<float>(), cb.as<float>(), ncb, n, d, m, nullptr,
                                      c->sOut16.as<int16_t>(), db.as<float>(), nr.as<float>()));
    LSQ_TRY(fetch(c, idx_out, c->sOut16.p, sizeof(int16_t) * (size_t)n));
    LSQ_TRY(fetch(c, dbnorms, db.p, db.bytes));
    LSQ_TRY(fetch(c, norms, nr.p, nr.bytes));
    return finish(c);
}

extern "C" int lsq_quantize_norms(lsq_ctx *c, const int16_t *B, const float *K, const float *cbnorms, int ncb, int d, int64_t n, int m, int h,
                                  int16_t *idx_out, float *dbnorms, float *norms) {
    return quantize_norms("lsq_quantize_norms", c, true, B, K, cbnorms, ncb, d, n, m, h, idx_out, dbnorms, norms);
}
extern "C" int lsq_quantize_norms_dev(lsq_ctx *c, const uint8_t *d_codes, const float *d_K, const float *d_cbnorms, int ncb, int d, int64_t n, int m,
                                      int h, uint8_t *d_idx_out, float *d_dbnorms, float *d_norms) {
    return quantize_norms("lsq_quantize_norms_dev", c, false, d_codes, d_K, d_cbnorms, ncb, d, n, m, h, d_idx_out, d_dbnorms, d_norms);
}

// the LSQR codebook update on the device (lsq_lsqr.hip).  dim2C: a structured update's map -- d x m bytes in Julia's column-major order ([m][d] here), every
// entry 0 or 1; in the memory `host` names -- or null = the unstructured update
static int check_cover(const char *fn, const uint8_t *dim2C, int d, int m) {
    for (int64_t e = 0; dim2C && e < (int64_t)d * m; ++e)
        if (dim2C[e] > 1) { lsq_set_error("%s: dim2C[%lld] = %d is neither 0 nor 1", fn, (long long)e, (int)dim2C[e]); return LSQ_EINVAL; }
    return LSQ_OK;
}

static int update_codebooks(const char *fn, lsq_ctx *c, bool host, const float *X, const void *codes, const uint8_t *dim2C, int d, int64_t n, int m, int h,
                            float *K_out, int *iterations) {
    LSQ_TRY(entry_args(fn, c, d, n, m, h, n >= 1 && X && codes && K_out, "bad arguments"));
    std::vector<uint8_t> cover;                                               // a _dev form's map: read back; checked and turned into the two lists on the host
    if (!host && dim2C) {
        cover.resize((size_t)d * m);
        LSQ_TRY(fetch(c, cover.data(), dim2C, cover.size()));
        LSQ_TRY(finish(c));
        dim2C = cover.data();
    }
    LSQ_TRY(check_cover(fn, dim2C, d, m));
    if (!host) return lsq_lsqr_update_codebooks(c->stream, &c->lsqr, X, static_cast<const uint8_t *>(codes), dim2C, d, n, m, K_out, iterations);
    LSQ_TRY(claim_sK(c, d, m));
    LSQ_TRY(stage_X(c, X, d, n));
    LSQ_TRY(stage_codes(c, static_cast<const int16_t *>(codes), n, m, h, true));
    LSQ_TRY(lsq_lsqr_update_codebooks(c->stream, &c->lsqr, c->sX.as<float>(), c->sTight.as<uint8_t>(), dim2C, d, n, m, c->sK.as<float>(), iterations));
    LSQ_TRY(fetch(c, K_out, c->sK.p, codebook_bytes(d, m)));
    return finish(c);
}

extern "C" int lsq_update_codebooks_dev(lsq_ctx *c, const float *d_X, const uint8_t *d_codes, int d, int64_t n, int m, int h, float *d_K_out,
                                        int *iterations) {
    return update_codebooks("lsq_update_codebooks_dev", c, false, d_X, d_codes, nullptr, d, n, m, h, d_K_out, iterations);
}
extern "C" int lsq_update_codebooks_gpu(lsq_ctx *c, const float *X, const int16_t *B, int d, int64_t n, int m, int h, float *K_out, int *iterations) {
    return update_codebooks("lsq_update_codebooks_gpu", c, true, X, B, nullptr, d, n, m, h, K_out, iterations);
}
// the structured update: update_codebooks_generic / update_codebooks_chain (src/codebook_update.jl:104-158); a null map is the unstructured call
extern "C" int lsq_update_codebooks_struct_dev(lsq_ctx *c, const float *d_X, const uint8_t *d_codes, const uint8_t *d_dim2C, int d, int64_t n, int m, int h,
                                               float *d_K_out, int *iterations) {
    return update_codebooks(d_dim2C ? "lsq_update_codebooks_struct_dev" : "lsq_update_codebooks_dev", c, false, d_X, d_codes, d_dim2C, d, n, m, h, d_K_out, iterations);
}
extern "C" int lsq_update_codebooks_struct_gpu(lsq_ctx *c, const float *X, const int16_t *B, const uint8_t *dim2C, int d, int64_t n, int m, int h, float *K_out,
                                               int *iterations) {
    return update_codebooks(dim2C ? "lsq_update_codebooks_struct_gpu" : "lsq_update_codebooks_gpu", c, true, X, B, dim2C, d, n, m, h, K_out, iterations);
}

// the SPGL1 (LASSO) codebook update (lsq_spgl1.hip).  Arguments first (no device needed to reject them), then the context: a NULL context on a machine
// without a device is LSQ_ENODEV; the pointers last
static int update_codebooks_spgl1(const char *fn, lsq_ctx *c, bool host, const float *X, const void *codes, int d, int64_t n, int m, int h, double tau,
                                  const float *K_init, int64_t S, const lsq_spgl1_params *p, float *K_out, lsq_spgl1_info *info) {
    LSQ_TRY(check_shape(fn, d, n, m, h));
    if (n < 1) { lsq_set_error("%s: n=%lld must be >= 1", fn, (long long)n); return LSQ_EINVAL; }
    if (!(tau >= 0.0)) { lsq_set_error("%s: tau=%g must be a number >= 0", fn, tau); return LSQ_EINVAL; }
    if (p && (p->opt_tol != p->opt_tol || p->opt_tol >= 1.0)) { lsq_set_error("%s: opt_tol=%g must be below 1", fn, p->opt_tol); return LSQ_EINVAL; }
    const double opt_tol = p && p->opt_tol > 0.0 ? p->opt_tol : 1e-4;
    const int64_t max_iter = p && p->max_iter > 0 ? p->max_iter : 10 * n * (int64_t)d;        // spgSetParms: iterations = 10 length(b)
    if (!c) {
        int count = 0;
        if (lsq_device_count(&count) != LSQ_OK || count <= 0) { lsq_set_error("%s: no HIP device visible (this library has no CPU fallback)", fn); return LSQ_ENODEV; }
        lsq_set_error("%s: null lsq_ctx", fn);
        return LSQ_EINVAL;
    }
    LSQ_TRY(use_device(c));
    if (!X || !codes || !K_out) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (!host) return lsq_spgl1_update_codebooks(c->stream, &c->spgl1, X, static_cast<const uint8_t *>(codes), d, n, m, tau, K_init, S, opt_tol, max_iter, K_out, info);
    Slice k0{K_init ? codebook_bytes(d, m) : 0};                                  // sF32: the start K_init
    LSQ_TRY(claim_sK(c, d, m));
    LSQ_TRY(carve_f32(c, {&k0}));
    LSQ_TRY(stage_X(c, X, d, n));
    if (K_init) LSQ_TRY(stage(c, k0.p, K_init, k0.bytes));
    LSQ_TRY(stage_codes(c, static_cast<const int16_t *>(codes), n, m, h, true));
    LSQ_TRY(lsq_spgl1_update_codebooks(c->stream, &c->spgl1, c->sX.as<float>(), c->sTight.as<uint8_t>(), d, n, m, tau, K_init ? k0.as<float>() : nullptr, S,
                                       opt_tol, max_iter, c->sK.as<float>(), info));
    LSQ_TRY(fetch(c, K_out, c->sK.p, codebook_bytes(d, m)));
    return finish(c);
}

extern "C" int lsq_update_codebooks_spgl1_dev(lsq_ctx *c, const float *d_X, const uint8_t *d_codes, int d, int64_t n, int m, int h, double tau,
                                              const float *d_K_init, int64_t S, const lsq_spgl1_params *params, float *d_K_out, lsq_spgl1_info *info) {
    return update_codebooks_spgl1("lsq_update_codebooks_spgl1_dev", c, false, d_X, d_codes, d, n, m, h, tau, d_K_init, S, params, d_K_out, info);
}
extern "C" int lsq_update_codebooks_spgl1(lsq_ctx *c, const float *X, const int16_t *B, int d, int64_t n, int m, int h, double tau, const float *K_init,
                                          int64_t S, const lsq_spgl1_params *params, float *K_out, lsq_spgl1_info *info) {
    return update_codebooks_spgl1("lsq_update_codebooks_spgl1", c, true, X, B, d, n, m, h, tau, K_init, S, params, K_out, info);
}

// The initialisers' data-parallel steps (lsq_init.hip).  Both are "unaries of a chunk, then one kernel": the unaries are the path's own
// (row-major f32 planes of the chain GEMM -- the bits lsq_get_unaries returns), so the codes are integer functions of exactly the numbers
// oracle/init_oracle.py works on.  B: int16 1-based [n][m] (host) or tight uint8 0-based (device)
static int init_codes(lsq_ctx *c, const char *fn, bool host, const float *X, const float *K, int d, int64_t n, int m, int h, void *B, float *minval, bool chain) {
    const bool short_chain = chain && m < 2;        // a _dev form says so before it looks at its pointers, a host form once it has rows: as they always did
    const char *needs_two = "a chain needs at least two codebooks";
    LSQ_TRY(entry_args(fn, c, d, n, m, h, host || !short_chain, needs_two));
    if (!K || (n > 0 && (!X || !B))) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (n == 0) return LSQ_OK;
    if (short_chain) { lsq_set_error("%s: %s", fn, needs_two); return LSQ_EINVAL; }
    Slice mins{host && minval ? sizeof(float) * (size_t)n * m : 0};              // sF32: the minima
    uint8_t *dB = static_cast<uint8_t *>(B);
    float *dmin = minval;
    if (host) {
        LSQ_TRY(claim_sK(c, d, m, K));
        LSQ_TRY(stage_X(c, X, d, n));
        LSQ_TRY(c->sTight.ensure((size_t)n * m));
        LSQ_TRY(carve_f32(c, {&mins}));
        X = c->sX.as<float>(); K = c->sK.as<float>(); dB = c->sTight.as<uint8_t>(); dmin = minval ? mins.as<float>() : nullptr;
    }
    if (chain) LSQ_TRY(prepare_tables(c, K, d, m));                   // ||c||^2 and the pair tables (the chain reads the m - 1 adjacent ones)
    else {
        c->tables_valid = false;
        LSQ_TRY(c->sci.ensure(sizeof(float) * (size_t)m * LSQ_H));
        LSQ_TRY(lsq_launch_sqnorms(c->stream, K, m * LSQ_H, d, c->sci.as<float>()));
    }
    for (int64_t off = 0; off < n; off += c->chunk) {
        const int64_t cn = std::min<int64_t>(c->chunk, n - off);
        LSQ_TRY(build_unaries(c, X + off * d, K, d, cn, m, 0, 0, cn));
        Timer t(c, CAT_OTHER);
        if (chain) LSQ_TRY(lsq_launch_viterbi(c->stream, c->U.as<float>(), c->T.as<float>(), cn, m, dB + off * m));
        else LSQ_TRY(lsq_launch_unary_argmin(c->stream, c->U.as<float>(), cn, m, dB + off * m, dmin ? dmin + off * m : nullptr));
    }
    if (!host) return LSQ_OK;
    LSQ_TRY(fetch_codes(c, static_cast<int16_t *>(B), n, m, true));
    LSQ_TRY(fetch(c, minval, mins.p, mins.bytes));
    return finish(c);
}

extern "C" int lsq_encode_viterbi_dev(lsq_ctx *c, const float *dX, const float *dK, int d, int64_t n, int m, int h, uint8_t *dB) {
    return init_codes(c, "lsq_encode_viterbi_dev", false, dX, dK, d, n, m, h, dB, nullptr, true);
}
extern "C" int lsq_encode_viterbi(lsq_ctx *c, const float *X, const float *K, int d, int64_t n, int m, int h, int16_t *B) {
    return init_codes(c, "lsq_encode_viterbi", true, X, K, d, n, m, h, B, nullptr, true);
}
extern "C" int lsq_assign_codewords_dev(lsq_ctx *c, const float *dX, const float *dK, int d, int64_t n, int m, int h, uint8_t *dB, float *d_minval) {
    return init_codes(c, "lsq_assign_codewords_dev", false, dX, dK, d, n, m, h, dB, d_minval, false);
}
extern "C" int lsq_assign_codewords(lsq_ctx *c, const float *X, const float *K, int d, int64_t n, int m, int h, int16_t *B, float *minval) {
    return init_codes(c, "lsq_assign_codewords", true, X, K, d, n, m, h, B, minval, false);
}

// Cluster means and k-means++ seeding (lsq_kmeans.hip).  The cover map of these entries is HOST memory in both forms: its d m bytes are checked before
// anything is launched, so a _dev call never waits for the device
static int kmeans_args(const char *fn, lsq_ctx *c, const uint8_t *dim2C, int d, int64_t n, int m, int h) {
    LSQ_TRY(entry_args(fn, c, d, n, m, h, dim2C != nullptr, "null dim2C (plain k-means is m = 1 with every dimension covered)"));
    LSQ_TRY(check_cover(fn, dim2C, d, m));
    for (int j = 0; j < m; ++j) {
        int cnt = 0;
        for (int t = 0; t < d; ++t) cnt += dim2C[(size_t)j * d + t];
        if (cnt == 0) { lsq_set_error("%s: codebook %d covers no dimension", fn, j); return LSQ_EINVAL; }
    }
    return LSQ_OK;
}

static int update_centers(const char *fn, lsq_ctx *c, bool host, const float *X, const void *codes, const uint8_t *dim2C, const float *K_prev, int d, int64_t n,
                          int m, int h, float *K_out, int *counts) {
    LSQ_TRY(kmeans_args(fn, c, dim2C, d, n, m, h));
    if (!K_out || (n > 0 && (!X || !codes))) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    if (n * (int64_t)m >= (int64_t)1 << 31) { lsq_set_error("%s: n * m = %lld exceeds 2^31 - 1", fn, (long long)(n * m)); return LSQ_EINVAL; }
    if (!host) return lsq_kmeans_update_centers(c->stream, &c->kmeans, X, static_cast<const uint8_t *>(codes), dim2C, K_prev, d, n, m, K_out, counts);
    Slice cnt{sizeof(int) * (size_t)m * LSQ_H};                                   // sF32: the cluster counts
    LSQ_TRY(claim_sK(c, d, m));
    LSQ_TRY(carve_f32(c, {&cnt}));
    LSQ_TRY(stage_X(c, X, d, n));
    if (K_prev) LSQ_TRY(stage(c, c->sK.p, K_prev, codebook_bytes(d, m)));          // K_prev in place: an empty cluster keeps the entry it finds
    LSQ_TRY(stage_codes(c, static_cast<const int16_t *>(codes), n, m, h, true));
    LSQ_TRY(lsq_kmeans_update_centers(c->stream, &c->kmeans, c->sX.as<float>(), c->sTight.as<uint8_t>(), dim2C, K_prev ? c->sK.as<float>() : nullptr, d, n, m,
                                      c->sK.as<float>(), cnt.as<int>()));
    LSQ_TRY(fetch(c, K_out, c->sK.p, codebook_bytes(d, m)));
    LSQ_TRY(fetch(c, counts, cnt.p, cnt.bytes));
    return finish(c);
}

extern "C" int lsq_update_centers_dev(lsq_ctx *c, const float *d_X, const uint8_t *d_codes, const uint8_t *dim2C, const float *d_K_prev, int d, int64_t n,
                                      int m, int h, float *d_K_out, int *d_counts) {
    return update_centers("lsq_update_centers_dev", c, false, d_X, d_codes, dim2C, d_K_prev, d, n, m, h, d_K_out, d_counts);
}
extern "C" int lsq_update_centers(lsq_ctx *c, const float *X, const int16_t *B, const uint8_t *dim2C, const float *K_prev, int d, int64_t n, int m, int h,
                                  float *K_out, int *counts) {
    return update_centers("lsq_update_centers", c, true, X, B, dim2C, K_prev, d, n, m, h, K_out, counts);
}

static int kmeanspp_seed(const char *fn, lsq_ctx *c, bool host, const float *X, const uint8_t *dim2C, const double *u, int d, int64_t n, int m, int h, float *K_out,
                         int64_t *idx_out, float *d2_out) {
    LSQ_TRY(kmeans_args(fn, c, dim2C, d, n, m, h));
    if (!u) { lsq_set_error("%s: null u", fn); return LSQ_EINVAL; }
    for (int e = 0; e < m * LSQ_H; ++e)
        if (!(u[e] >= 0.0 && u[e] < 1.0)) { lsq_set_error("%s: u[%d] = %g lies outside [0, 1)", fn, e, u[e]); return LSQ_EINVAL; }
    if (!K_out || (n > 0 && !X)) { lsq_set_error("%s: null pointer", fn); return LSQ_EINVAL; }
    Slice idx{sizeof(int64_t) * (size_t)m * LSQ_H}, d2{sizeof(float) * (size_t)n * m};      // sF32 (host form): the chosen rows' indices | d2
    float *dK = K_out, *dd2 = d2_out;
    int64_t *didx = idx_out;
    if (host) {
        if (n == 0) d2_out = nullptr;                                         // d2 is empty
        LSQ_TRY(claim_sK(c, d, m));
        LSQ_TRY(carve_f32(c, {&idx, &d2}));
        LSQ_TRY(stage_X(c, X, d, n));
        X = c->sX.as<float>(); dK = c->sK.as<float>(); didx = idx.as<int64_t>(); dd2 = d2_out ? d2.as<float>() : nullptr;
    }
    if (n == 0) {                                                             // no row to choose: zero codebooks, indices -1, d2 empty
        LSQ_HIP(hipMemsetAsync(dK, 0, codebook_bytes(d, m), c->stream));
        if (didx) LSQ_TRY(lsq_kmeans_fill_i64(c->stream, didx, (int64_t)m * LSQ_H, -1));
    } else LSQ_TRY(lsq_kmeans_seed(c->stream, &c->kmeans, X, dim2C, u, d, n, m, dK, didx, dd2));
    if (!host) return LSQ_OK;
    LSQ_TRY(fetch(c, K_out, dK, codebook_bytes(d, m)));
    LSQ_TRY(fetch(c, idx_out, didx, idx.bytes));
    LSQ_TRY(fetch(c, d2_out, dd2, d2.bytes));
    return finish(c);
}

extern "C" int lsq_kmeanspp_seed_dev(lsq_ctx *c, const float *d_X, const uint8_t *dim2C, const double *u, int d, int64_t n, int m, int h, float *d_K_out,
                                     int64_t *d_idx_out, float *d_d2_out) {
    return kmeanspp_seed("lsq_kmeanspp_seed_dev", c, false, d_X, dim2C, u, d, n, m, h, d_K_out, d_idx_out, d_d2_out);
}
extern "C" int lsq_kmeanspp_seed(lsq_ctx *c, const float *X, const uint8_t *dim2C, const double *u, int d, int64_t n, int m, int h, float *K_out,
                                 int64_t *idx_out, float *d2_out) {
    return kmeanspp_seed("lsq_kmeanspp_seed", c, true, X, dim2C, u, d, n, m, h, K_out, idx_out, d2_out);
}

// ---- device-side generators ---------------------------------------------------------------------
extern "C" int lsq_synth_data_u8_dev(lsq_ctx *c, uint64_t seed, uint64_t global_offset, int64_t n, int d, float *dX) {
    LSQ_TRY(use_device(c));
    if (n < 0 || d < 1 || (n > 0 && !dX)) { lsq_set_error("lsq_synth_data_u8_dev: bad arguments"); return LSQ_EINVAL; }
    return lsq_launch_synth_data_u8(c->stream, seed, global_offset, n, d, dX);
}
extern "C" int lsq_randinit_dev(lsq_ctx *c, uint64_t seed, uint64_t global_offset, int64_t n, int m, int h, uint8_t *dB) {
    LSQ_TRY(use_device(c));
    if (n < 0 || m < 1 || h < 1 || h > 256 || (n > 0 && !dB)) { lsq_set_error("lsq_randinit_dev: bad arguments"); return LSQ_EINVAL; }
    return lsq_launch_randinit(c->stream, seed, global_offset, n, m, h, dB);
}
extern "C" int lsq_synth_codebooks_dev(lsq_ctx *c, uint64_t seed, int m, int h, int d, float *dK) {
    LSQ_TRY(use_device(c));
    if (m < 1 || h < 1 || d < 1 || !dK) { lsq_set_error("lsq_synth_codebooks_dev: bad arguments"); return LSQ_EINVAL; }
    return lsq_launch_synth_codebooks(c->stream, seed, m, h, d, dK);
}
