// lsq_internal.h -- shared internals of liblsq_mi355x.so (gfx950 only; not a public header).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>

#include "../../include/lsq_mi355x.h"
#include "lsq_grow_check.h"
#include "lsq_compact_check.h"
#include "lsq_range_check.h"
#include "lsq_recon_check.h"
#include "lsq_half_check.h"
#include "lsq_snapshot_check.h"

#define LSQ_H 256          // candidates per codebook: one wave x float4 per lane
#define LSQ_MAX_M 16
#define LSQ_WALK_TRACE 64        // per-position (sweep * m + rank in the node order, mod 64) recomputed node updates
#define LSQ_WALK_COUNTERS (4 + LSQ_WALK_TRACE + 3)      // device counters of the walk kernel: [0] node updates recomputed, [1..3] staged / light / filtered block-node-updates, [4..67] trace, [68] node updates the filter refined exactly, [69] exact candidate evaluations of those, [70] node updates sent to f32 (outside the sampled level range)

// ---- tuning knobs -------------------------------------------------------------------------
// Tuning knobs (environment variables) exist in the tuning build only; the shipped library uses the measured defaults.
#ifdef LSQ_TUNING
#define LSQ_KNOB(name, def) ([] { static const int v_ = [] { const char *e_ = getenv(name); return e_ ? atoi(e_) : (def); }(); return v_; }())
#else
#define LSQ_KNOB(name, def) (def)
#endif

// ---- error plumbing ---------------------------------------------------------------------
void lsq_set_error(const char *fmt, ...);

#define LSQ_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            lsq_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorOutOfMemory) ? LSQ_ENOMEM : LSQ_EHIP;                        \
        }                                                                                      \
    } while (0)

#define LSQ_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != LSQ_OK) return rc_; \
    } while (0)

// ---- a device buffer that only grows (owned by a context or by one of its sub-states) --------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool view = false;          // a window into another allocation (the context's block of small per-call words): never freed here; outgrown -> an allocation of its own
    int ensure(size_t bytes) {
        if (bytes <= cap) return LSQ_OK;
        if (view) { p = nullptr; cap = 0; view = false; }
        if (p) { LSQ_HIP(hipFree(p)); p = nullptr; cap = 0; }
        if (bytes == 0) return LSQ_OK;
        LSQ_HIP(hipMalloc(&p, bytes));
        cap = bytes;
        return LSQ_OK;
    }
    void release() { if (p && !view) (void)hipFree(p); p = nullptr; cap = 0; view = false; }
    void window(void *base, size_t off, size_t bytes) { release(); p = static_cast<char *>(base) + off; cap = bytes; view = true; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// ---- the phase clock of a timed call (option "profile"): up to N marks on the stream, read as the N - 1 times between neighbours.  Owned by the state whose
// phases it times; the context's Timer (lsq_api.hip) is another thing: its pairs are resolved lazily, these before the call returns ----------------------
template <int N>
struct PhaseClock {
    hipEvent_t ev[N] = {};
    int marks = 0;
    bool timed = false;
    int begin(bool on) {        // a new run of marks; the events are made at the first timed one
        timed = on; marks = 0;
        if (timed) for (hipEvent_t &e : ev) if (!e) LSQ_HIP(hipEventCreate(&e));
        return LSQ_OK;
    }
    int mark(hipStream_t s) {
        if (timed && marks < N) LSQ_HIP(hipEventRecord(ev[marks++], s));
        return LSQ_OK;
    }
    int read(float *ms) {       // ms[N - 1]; waits for the last mark; 0 for the intervals that were not marked
        for (int e = 0; e + 1 < N; ++e) ms[e] = 0.0f;
        if (!timed || marks < 2) return LSQ_OK;
        LSQ_HIP(hipEventSynchronize(ev[marks - 1]));
        for (int e = 0; e + 1 < marks; ++e) LSQ_HIP(hipEventElapsedTime(&ms[e], ev[e], ev[e + 1]));
        return LSQ_OK;
    }
    void release() { for (hipEvent_t &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; } }
};

// ---- Philox4x32-10 (Random123; Salmon et al. SC'11), shared by host and device -----------
// Stream layout (build-defined, mirrored by oracle/lsq_oracle.c):
//   counter = (idx_lo, idx_hi, it, (domain << 16) | (word >> 2)),  key = (seed_lo, seed_hi),
//   word w of the stream = output[w & 3].
enum { LSQ_DOM_PERTURB = 1, LSQ_DOM_PERM = 2, LSQ_DOM_INIT = 3, LSQ_DOM_DATA = 4, LSQ_DOM_CODEBOOK = 5 };

struct lsq_u32x4 { uint32_t v[4]; };

__host__ __device__ inline lsq_u32x4 lsq_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                       uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    lsq_u32x4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

__host__ __device__ inline lsq_u32x4 lsq_rng_block(uint64_t seed, uint64_t idx, uint32_t it, uint32_t domain, uint32_t block) {
    return lsq_philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), it, (domain << 16) | block,
                             (uint32_t)seed, (uint32_t)(seed >> 32));
}

__host__ __device__ inline uint32_t lsq_rng_word(uint64_t seed, uint64_t idx, uint32_t it, uint32_t domain, uint32_t w) {
    return lsq_rng_block(seed, idx, it, domain, w >> 2).v[w & 3];
}

__host__ __device__ inline uint32_t lsq_mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// ---- 16-bit filtered walk: quantisation parameters (device memory, one per resident chunk) ---------------------------------
// Every term of a conditioned sum s[a] = U_j[a] + SUM_k T_jk[b_k][a] is ALSO held as a 16-bit level on ONE common step D_j per node:
//   U level = rint((u + g_j[a] + sigma_ij - loU) / D),  table level = rint((t - g_jk[a] - min of the centred row) / D)  (shifts shared by all
//   candidates of a node update, and per-candidate shifts moved from the tables to the unary: lsq_icmq.hip),  so that the sum of the m levels Q[a] fits 16 bits and s[a] = C_i + D * Q[a] up to (0.5 + 2^-5) D per term.  Rigorous
//   consequence (see icm_walkq_kernel): the exact fp32 argmin lies among the candidates with Q <= Qmin + window.  ok = 0 (non-finite or
//   degenerate bounds) sends the chunk to the fp32 walk instead.
struct lsq_q16_node {
    float loU, invD, D;        // U levels start at loU: the sampled range of the SHIFTED U_j widened by 1/8; tables use the exact range of their centred rows
    float hiq;                 // largest U level of the widened sampled range: a vector with a level outside [0, hiq] is flagged (beyond it the sum of
                               // the m levels could pass 65535 and wrap)
    int window;                // levels
    double slack;              // bound of |fp32 conditioned sum - real sum| + per-term level error, in s units: m (0.5 + 2^-5) D + eps
};
struct lsq_q16_params {
    int ok;
    int oor;                   // values the GEMM epilogue found outside the sampled level range (their vectors are flagged and take the f32 path)
    int nflag;                 // (vector, node) pairs flagged in this chunk: above 1 / filter_fallback_div of all pairs the host sends the whole chunk to the f32 walk
    lsq_q16_node node[LSQ_MAX_M];
};

// one kernel of each translation unit of the encode path: lsq_create asks for its attributes, which makes the runtime load that unit's code object
// THEN (HIP loads a unit's device code at its first use: ~10 ms that the first encode of a process would otherwise pay)
const void *lsq_probe_kernel_gemm();
const void *lsq_probe_kernel_icm();
const void *lsq_probe_kernel_icmq();

// ---- kernel launchers (implemented in the .hip files) ------------------------------------
// All pointers are device pointers; all launch on `s` and return immediately.

// D[off(r,c)] = chain_t( A[r][t] * (alpha * Bm[c][t]) ) (+ addv[c]);  r<M, c<N, t<Kd.
// off(r,c) = (c / h) * plane_stride + (c % h) + r * row_stride            (slice == 0, row-major planes)
//          = (c / h) * plane_stride + ((c % h) / slice) * (Mtot * slice) + (c % h) % slice + r * slice   (slice-major)
// Chain = k-ascending fmaf from +0.  The launch covers output rows [rbase, rbase + M) of a Mtot-row result (A points at
// row rbase): row r above counts from rbase -- lets the caller build the unaries panel by panel under the H2D copies.
// Optional second output (q != nullptr, q->Dq != nullptr): the same values as 16-bit fixed-point levels in slice-major u16 planes of slice width slice_q,
// Dq[(c / h) * Mtot * h + ((c % h) / slice_q) * Mtot * slice_q + r * slice_q + (c % h) % slice_q] = rint((v + colshift[c] + sigma[r][c / h] - qp->node[c / h].loU) * invD).
struct lsq_gemm_q16 {
    uint16_t *Dq = nullptr; int slice_q = 0;
    lsq_q16_params *qp = nullptr;
    unsigned short *qflag = nullptr;      // [Mtot] u16 (Mtot even-padded): bit j raised when a value of plane j fell outside the level range
    // sigma (optional, [Mtot][N / h] floats) / colshift (optional, [N] floats): per-(row, plane) and per-column shifts added to a value before its LEVEL is taken (and
    // in the range-only pass); the f32 output D is not shifted.  A shift common to all candidates of a node update cannot change its argmin (lsq_icmq.hip).
    const float *sigma = nullptr, *colshift = nullptr;
    // qrange != nullptr: range-only pass over every rts-th 128-row panel of A, nothing stored; qrange[2 j], [2 j + 1] = min / max keys
    unsigned *qrange = nullptr; int rts = 1;
};
int lsq_launch_chain_gemm(hipStream_t s, const float *A, const float *Bm, const float *addv, float alpha,
                          int64_t M, int N, int Kd, int h, int64_t plane_stride, int64_t row_stride, float *D, int slice,
                          int64_t Mtot, int64_t rbase, const lsq_gemm_q16 *q = nullptr);
// 8-bit data rows (A = X as uint8_t, Kd bytes apart): the same contract and, uint8 -> f32 being exact, the same bits as the call above on the widened rows
int lsq_launch_chain_gemm(hipStream_t s, const uint8_t *A, const float *Bm, const float *addv, float alpha,
                          int64_t M, int N, int Kd, int h, int64_t plane_stride, int64_t row_stride, float *D, int slice,
                          int64_t Mtot, int64_t rbase, const lsq_gemm_q16 *q = nullptr);
// sci[r] = chain_t(Kb[r][t]^2)
int lsq_launch_sqnorms(hipStream_t s, const float *Kb, int rows, int d, float *sci);

// Internal code records: cs bytes per vector (8 for m<=8, 16 for m<=16), byte j = code of codebook j.
static inline int lsq_code_stride(int m) { return m <= 8 ? 8 : 16; }

int lsq_launch_codes_expand(hipStream_t s, const uint8_t *tight, int64_t n, int m, uint8_t *rec);      // [n][m] -> [n][cs]
int lsq_launch_codes_compact(hipStream_t s, const uint8_t *rec, int64_t n, int m, uint8_t *tight);     // [n][cs] -> [n][m]
int lsq_launch_codes_from_i16(hipStream_t s, const int16_t *B, int64_t n, int m, int h, uint8_t *rec, int *bad_flag);
int lsq_launch_codes_to_i16(hipStream_t s, const uint8_t *rec, int64_t n, int m, int16_t *B);

// vsrc/vdst (optional): per-vector node-validity masks (bit j = code j is the argmin for the current other
// codes); a perturbation that changes a code clears the whole mask.
int lsq_launch_perturb(hipStream_t s, const uint8_t *src, uint8_t *dst, int64_t n, int m, int npert,
                       uint64_t seed, uint32_t it, uint64_t global_offset, const unsigned short *vsrc, unsigned short *vdst);
// LDS-walk schedule: one block walks all slices of its vector range; Ts = slice-major pair tables
constexpr int lsq_walk_slice_width(int m) { return m <= 8 ? 16 : 8; }      // f32 candidates per slice
constexpr int lsq_q16_slice_width(int m) { return 2 * lsq_walk_slice_width(m); }      // candidates per 16-bit slice: the same bytes per piece as the f32 walk
int lsq_launch_tables_to_slices(hipStream_t s, const float *T, float *Ts, int m, int sl);
// vectors per block pass of the f32 LDS-walk kernel: table + 10 B per vector must fit the 160 KiB LDS
constexpr int lsq_walk_pp(int M, int SL) {
    const int avail = 160 * 1024 - 256 - (M - 1) * LSQ_H * (SL / 4) * 16;      // bytes left beside the slice table
    const int pp = avail / 10 / 64 * 64;
    return pp > 4096 ? 4096 : pp;                                             // 4096 up to m = 14 (SL = 8), 4032 at m = 16
}
// geometry of a walk launch (f32 or filtered) over n vectors, 256 blocks: vectors per pass (<= the kernel's LDS budget pp), number of passes (= segments)
inline void lsq_walk_geometry(int64_t n, int pp, int *per_pass, int *npass) {
    const int64_t rounds = (n + 256 * (int64_t)pp - 1) / (256 * (int64_t)pp);          // passes per block
    int64_t per = rounds > 0 ? (n + 256 * rounds - 1) / (256 * rounds) : 1;
    per = per > pp ? pp : (per < 1 ? 1 : per);
    *per_pass = (int)per;
    *npass = (int)((n + per - 1) / per);
}
// valid (optional): validity masks, maintained by the kernel; use_skip: skip vectors whose bit j is set (exact);
// active_total (optional): += number of vectors actually recomputed; ablation != 0: timing-only variants (m = 8), garbage results.
// U is the slice-major unary buffer of ALL nodes; T (optional) the row-major tables for light blocks' L2 gathers; order[nnodes] = node updates run back to back inside the launch
// (a block owns its vectors for the whole launch): 1 entry = one node update, icmiter*m entries = a whole ILS iteration.
// The three walk launchers cut order[nnodes] into launches of at most max_per node updates (1 .. 64 = LSQ_WALK_MAX_NODES; lsq_wave.h holds the one splitter) and
// add the number of launches they made to *launched (optional).
int lsq_launch_icm_wave(hipStream_t s, const float *U, const float *T, uint8_t *rec, unsigned short *valid, int64_t n, int m, const int32_t *order,
                        int nnodes, int pos0, int max_per, int use_skip, unsigned long long *active_total, const uint8_t *ref_rec,
                        const unsigned short *ref_valid, int *launched);      // chunks in which every block would be light: a wave owns its vectors through the launch
int lsq_launch_icm_walk(hipStream_t s, const float *U, const float *Ts, const float *T, uint8_t *rec, unsigned short *valid, int64_t n, int m,
                        const int32_t *order, int nnodes, int pos0, int max_per, int use_skip, unsigned long long *active_total, int ablation, int light,
                        const uint8_t *ref_rec, const unsigned short *ref_valid, const int *idle_if_set, int *launched);
// idle_if_set (optional, device): the launch does nothing when *idle_if_set != 0 (the filtered walk handled it)
// 16-bit filtered walk (lsq_icmq.hip).  The device memory its host side passes around, mapped ONCE (carved by q16_map in lsq_api.hip; no launcher does pointer
// arithmetic of its own).  Per call: bad (1 int: a non-finite pair table), trange (3 floats per pair table), rowmin / colmean [m*m*256], colshift [m*256], means
// [m*d]; per chunk: sigma [n*m], qflag, Uq (the GEMM's u16 planes), qrange.  Tq: the 16-bit slice tables [m][256/SLQ][m-1][256][SLQ].
struct lsq_q16_work {
    // qrange: 2 * LSQ_MAX_M range keys (min / max per node), then four words
    enum { Q_NONFINITE = 2 * LSQ_MAX_M,      // raised by the range pass: a non-finite value in the sample
           Q_SIGMAX,                         // max |sigma| of the chunk -- or of its sample -- as the sigma pass collects it (bit pattern of a non-negative float)
           Q_SIGBOUND,                       // the |sigma| bound the parameters assumed (q16_params_kernel writes it): the panel passes flag vectors beyond it
           Q_PANEL_SINK,                     // where a panel pass's own maximum goes: nothing reads it, the parameters were fixed from the sample
           Q_WORDS };                        // q16_range_init_kernel fills exactly these
    uint16_t *Tq = nullptr, *Uq = nullptr;
    int *bad = nullptr;
    float *trange = nullptr;
    unsigned *qrange = nullptr;
    unsigned short *qflag = nullptr;
    lsq_q16_params *P = nullptr;
    float *rowmin = nullptr, *colmean = nullptr, *colshift = nullptr, *means = nullptr, *sigma = nullptr;
    // sample mode (the host-buffer pipeline): the rows the strided sample pass would read -- every rts-th 128-row panel, lsq_q16_sample_rows -- already compacted on
    // the device, in X's element type; the level parameters come from them alone (max |sigma| widened x2) and X itself is not touched: its sigma are computed panel
    // by panel as the panels land (lsq_launch_unary_shift_panel: vectors beyond the assumed |sigma| bound are flagged for the f32 routine)
    const void *Xsample = nullptr;
    int64_t nsample_rows = 0;
    float *sigma_sample = nullptr;
};
// lsq_launch_q16_prepare: per chunk, after the pair tables and before the unary GEMM -- bounds, parameters P and Tq; tables_changed = 1 on the first chunk of a call.
// XT: float, or uint8_t for 8-bit rows (the two instantiations lsq_icmq.hip provides)
template <class XT>
int lsq_launch_q16_prepare(hipStream_t s, const XT *X, int64_t n, int d, const float *K, const float *sci, const float *T, int m, const lsq_q16_work &w,
                           int tables_changed);
int lsq_q16_sample_rows(int64_t n, int d, int64_t *rts_out);      // -> number of 128-row sample panels; *rts_out = the panel stride
// sigma (and flags) of the chunk's rows [row0, row0 + rows), Xp pointing at the first of them
template <class XT>
int lsq_launch_unary_shift_panel(hipStream_t s, const XT *Xp, int64_t rows, int d, int m, const lsq_q16_work &w, int64_t row0);
// lsq_launch_icm_walkq: same contract as lsq_launch_icm_walk plus Uq, Tq and P; the caller launches it only after reading the chunk's verdict (P->ok, P->nflag) on
// the host -- or gives it a gate
int lsq_launch_icm_walkq(hipStream_t s, const float *U, const uint16_t *Uq, const uint16_t *Tq, const float *T, uint8_t *rec, unsigned short *valid,
                         int64_t n, int m, const int32_t *order, int nnodes, int pos0, int max_per, int use_skip, unsigned long long *active_total, int light,
                         const uint8_t *ref_rec, const unsigned short *ref_valid, const lsq_q16_params *P, const unsigned short *qflag,
                         const unsigned *gate, int *launched);
// option "async": the chunk's road decided on the device (lsq_icmq.hip): road[0] = 2 filtered walk / 0 f32 walk, road[1] = chunks handed over
int lsq_launch_q16_road(hipStream_t s, const lsq_q16_params *P, unsigned *road, int64_t pairs, int64_t fallback_div);
int lsq_launch_q16_probe(hipStream_t s, const unsigned long long *probe, unsigned long long *totals, unsigned *road, int64_t probe_div);
// gate (optional, device; option "async"): the launch runs only when *gate == 2 (the road word names the filtered walk)
// ref_rec / ref_valid (optional, read-only): the vectors' current records and their validity masks; a candidate that becomes
// equal to its current record inherits those bits (exact: validity depends on the code tuple only)
// light: blocks with <= light active vectors gather table columns from L2 instead of staging slices (-1 = default 256)
// cost of `rec`; mode 0: prev[i] = cost.  mode 1 (accept): if cost < prev[i] { cur[i] = rec[i]; prev[i] = cost }
// and counters[0] += (#cost == prev), counters[1] += (#cost < prev)   (counters: 2 x uint64 on device)
// perturbation for the NEXT ILS iteration fused into the cost kernel's exit (on = 0: none): dst / vdst receive the perturbed copy of every vector's
// final record / validity word (dst may be the candidate array the kernel has just judged)
struct lsq_perturb_next { int on; int m, npert; uint32_t it; uint64_t seed, goff; uint8_t *dst; unsigned short *vdst; int abl; };      // abl: timing-only ablations of the cost kernel (tuning build; 0 in the shipped library)
int lsq_launch_cost(hipStream_t s, const float *X, const float *K, const uint8_t *rec, uint8_t *cur, float *prev,
                    unsigned long long *counters, int64_t n, int d, int m, int mode,
                    const unsigned short *vnew, unsigned short *vcur,
                    const lsq_perturb_next *next = nullptr);      // accept also copies the validity mask
int lsq_launch_cost(hipStream_t s, const uint8_t *X, const float *K, const uint8_t *rec, uint8_t *cur, float *prev,
                    unsigned long long *counters, int64_t n, int d, int m, int mode,
                    const unsigned short *vnew, unsigned short *vcur,
                    const lsq_perturb_next *next = nullptr);      // 8-bit rows of X (lsq_xload.h): the same costs, bit for bit
// *sum += SUM_i v[i]  (f64)
int lsq_launch_sum_f64(hipStream_t s, const float *v, int64_t n, double *sum);

int lsq_launch_synth_data_u8(hipStream_t s, uint64_t seed, uint64_t global_offset, int64_t n, int d, float *X);
int lsq_launch_randinit(hipStream_t s, uint64_t seed, uint64_t global_offset, int64_t n, int m, int h, uint8_t *tight);
int lsq_launch_synth_codebooks(hipStream_t s, uint64_t seed, int m, int h, int d, float *K);

// ---- the initialisers' two data-parallel kernels (lsq_init.hip) ---------------------------------------------------------------
// U: row-major f32 unary planes [m][n][256] (the unary GEMM with slice = 0), T: the pair tables of prepare_tables; codes: tight [n][m] u8, 0-based.
int lsq_launch_viterbi(hipStream_t s, const float *U, const float *T, int64_t n, int m, uint8_t *codes);            // encode_chain.jl:2-89
int lsq_launch_unary_argmin(hipStream_t s, const float *U, int64_t n, int m, uint8_t *codes, float *minval);     // PQ.jl:12-41, kmeans.jl:6-75; minval optional [n][m]

// ---- the beam-search encoder (lsq_beam.hip): U, T as above; order[m] HOST bytes, checked to be a permutation of 0 .. m-1 before the launch; codes: tight
// [n][m] u8 0-based, or (codes_i16) int16 1-BASED [n][m]; score optional [n] (the rank-0 beam's S: ||x||^2 + S is the vector's cost) ----------------------------
int lsq_launch_beam(hipStream_t s, const float *U, const float *T, int64_t n, int m, int L, const uint8_t *order, void *codes, int codes_i16, float *score);

// ---- device ADC scan (lsq_adc.hip) ----------------------------------------------------------------------------------------------------
// distance keys of the scans' records: order-preserving (a < b  <=>  key(a) < key(b)), NaN last
__device__ inline uint32_t lsq_adc_key(float v) {
    if (v != v) return 0xffffffffu;
    const uint32_t b = __float_as_uint(v);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ inline float lsq_adc_unkey(uint32_t k) {
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
struct lsq_adc_state;      // buffers of the scan, owned by the context
void lsq_adc_free(lsq_adc_state *st);
// What one call searches.  LSQ: K = [m h][d] codebooks, tables -2<q, c>, + dbnorms[i], 1-based ids out.  PQ / OPQ: K = [m][h][d] sub-space centres
// (d = subdim), squared-distance tables, no norm term, 0-based ids out.  Exact k-NN: no codes, no tables; lsq_knn.hip computes the squared distances to
// the rows base[i * bstride ..] for the same selection, ids out in id_base (0 unless the caller says otherwise).  What the rows and the queries of an
// exact search are made of is said HERE and nowhere else: f32, or the un-widened bytes of a .bvecs set (base_u8 / q_u8; strides in elements).  xnorms
// [n] / qnorms [queries] (uint32 squared norms, lsq_knn_launch_norms_u8) select the integer road: set only for uint8 x uint8 with d <= 258.
enum lsq_search_kind { LSQ_SEARCH_LSQ, LSQ_SEARCH_PQ, LSQ_SEARCH_EXACT };
struct lsq_search_input {
    lsq_search_kind kind;
    const uint8_t *codes; int cstride;       // [n][cstride] u8 0-based, the first m bytes of a row used
    const void *Q; int qstride;              // query rows, qstride elements apart (f32 for the table scans)
    const float *K;
    const float *dbnorms;
    int n, m, d;
    const void *base; int bstride;           // exact: [n][bstride], the first d elements of a row used
    int base_u8 = 0, q_u8 = 0;               // exact: element types of base / Q (0: f32, 1: uint8; base also LSQ_BASE_F16 / LSQ_BASE_BF16 -- a FORMAT, normalised by lsq_base_format)
    const uint32_t *xnorms = nullptr, *qnorms = nullptr;
    int id_base = 0;                         // exact: ids leave as row + id_base
    int packed = 0;                          // LSQ: rows of cstride = m + 1 bytes, the last one the norm byte c_i; dbnorms = the norm table padded to 256 floats
    // a row filter (lsq_filter.hip), LSQ and exact kinds.  filter_bits: bit (i & 31) of word i >> 5 = row i is allowed -- the DENSE road: every row is read, a
    // filtered one leaves as the record of an id outside the base (or does not leave).  filter_rows [filter_count]: the allowed rows ascending -- the COMPACT
    // road: the scan walks them instead of 0 .. n-1 (filter_bits is then ignored).  Both null: no filter, the scans' unfiltered instantiations
    const uint32_t *filter_bits = nullptr;
    const int *filter_rows = nullptr;
    int filter_count = 0;
    bool filtered() const { return filter_bits != nullptr || filter_rows != nullptr; }
    int rows_walked() const { return filter_rows ? filter_count : n; }      // rows a full scan reads
    int query_width() const { return kind == LSQ_SEARCH_PQ ? m * d : d; }      // elements of a query row that are read
    int id_sub() const { return kind == LSQ_SEARCH_LSQ ? 0 : 1 - id_base; }    // ids leave as (the record's id field 1 .. n) - id_sub
    size_t base_elem() const { return lsq_base_elem_bytes(base_u8); }
    size_t query_elem() const { return q_u8 ? 1 : sizeof(float); }
};
// how a call searches: the test hooks of the selection (options "linscan_exhaustive", "linscan_rank"), where its statistics go, and whether its
// phases are timed (then stats is not null)
struct lsq_search_opts {
    int force_exhaustive = 0, rank_override = 0;
    lsq_linscan_stats *stats = nullptr;
    int timed = 0;
};
// every pointer of `in` a device pointer / a host pointer (staged: upload, search, download); dists, idx [nq][nn] likewise
int lsq_adc_search(hipStream_t s, lsq_adc_state **st, float *dists, int *idx, const lsq_search_input &in, int nq, int nn, const lsq_search_opts &opt);
int lsq_adc_search_host(hipStream_t s, lsq_adc_state **st, float *dists, int *idx, const lsq_search_input &in, int nq, int nn, const lsq_search_opts &opt);
// the exact scan of one batch in adc_scan_kernel's three modes (0: against tau, 1: every record, 2: sample keys); qsel optional.  Routes on in's element
// types and norms (lsq_knn.hip)
int lsq_knn_launch_scan(hipStream_t s, int mode, const lsq_search_input &in, const int *qsel, int q0, int nqb, int stride, int ns, const uint32_t *tau,
                        unsigned *count, int cap, uint64_t *out, int idbits);
int lsq_knn_launch_norms_u8(hipStream_t s, const uint8_t *X, int64_t ld, int n, int d, uint32_t *out);
// argument checks of exact k-NN (lsq_linscan.hip), shared by the host drop-in and the device search
int lsq_knn_exact_check(const char *fn, const void *dists, const void *ids, const void *base, const void *queries, int n, int nq, int d, int ldb,
                        int ldq, int nn);

// ---- exact re-rank of shortlists (lsq_rerank.hip): the distance producer of stage two, and the pieces of the scans' selection that serve it ---------
// records (distance key << idbits | row + 1) of queries q0 .. q0 + nqb - 1 to out[slot * L + s]; cand [.][L] ids in id_base; a candidate outside
// [id_base, id_base + n) is not dereferenced: bit 32 + idbits, the key of +inf and id field 0 (sort the records on 33 + idbits bits).  *invalid += those
int lsq_rerank_launch(hipStream_t s, const void *base, int base_u8, int64_t ldb, int64_t n, const float *Q, int64_t ldq, const int *cand, int q0, int nqb,
                      int L, int d, int id_base, uint64_t *out, int idbits, unsigned long long *invalid);
int lsq_rerank_check(const char *fn, const void *dists, const void *ids, const void *base, const void *queries, const void *cand, int64_t n, int nq, int d,
                     int64_t ldb, int64_t ldq, int L, int nn, int id_base);
// The selection of every producer of records (lsq_adc.hip: adc_segments_kernel, sort_segments, adc_gather_kernel) over nqb lists of `cap` slots: the
// first count[slot] records of a list (count null: all cap of them) are sorted on end_bit bits and the first nn handed out as dists / idx [query][nn],
// query = qsel[slot] or q0 + slot, idx = id field - id_sub.  fail (optional, with count): fail[slot] = 1 and nothing handed out for a list that holds
// fewer than nn records or overflowed.  seg: 2 nqb ints of scratch.  idbits: the width of the id field 1 .. n
int lsq_adc_idbits(int64_t n);
// queries per batch of a producer that fills per_query record slots for each: two record buffers of at most 2^28 entries (~2 GiB apiece, and hipcub counts
// items in int), at most 16384 queries (the hand-out's grid counts them in its y dimension), at least one
int64_t lsq_adc_batch_queries(int64_t per_query);
int lsq_adc_select(lsq_adc_state **st, hipStream_t s, const uint64_t *recs, uint64_t *sorted, int *seg, const unsigned *count, int *fail, const int *qsel,
                   int q0, int nqb, int cap, int nn, float *dists, int *idx, int idbits, int end_bit, int id_sub);

// rows[i] = (codes[i][0 .. m), norm_codes[i]), m + 1 bytes apart; *bad += norm bytes >= ncb (a count: nothing depends on it but the caller's verdict)
int lsq_adc_launch_pack(hipStream_t s, const uint8_t *codes, const uint8_t *norm_codes, int64_t n, int m, int ncb, uint8_t *rows, unsigned *bad);

// adc_lut_kernel's tables for another scan (lsq_ivf.hip): LUT[(slot / QT) * m * 256 * QT + e * QT + slot % QT] = entry e of the table of query q0 + slot (or
// qsel[slot]), QT = lsq_adc_lut_qt(m) queries per tile; LUT holds ceil(nqb / QT) tiles
inline int lsq_adc_lut_qt(int m) { return m <= 8 ? 16 : 8; }
int lsq_adc_launch_lut(hipStream_t s, const lsq_search_input &in, const int *qsel, int q0, int nqb, float *LUT);

// ---- inverted lists on a resident index (lsq_ivf.hip): the layout lsq_index_set_lists builds and the search over the probed lists -----------------------
struct lsq_ivf_state;
void lsq_ivf_free(lsq_ivf_state *st);
int lsq_ivf_nlist(const lsq_ivf_state *st);      // 0: no lists yet
void lsq_ivf_get_info(const lsq_ivf_state *st, lsq_ivf_info *out);
// codes [n][m], norms [n]: the index's device arrays (packed: rows [n][m + 1] and the norm table of 256 floats, which the index keeps alive); desc as
// lsq_index_set_lists takes it.  A bad list_of_row entry leaves the former lists as they were
int lsq_ivf_set_lists(hipStream_t s, lsq_ivf_state **st, const uint8_t *codes, const float *norms, int packed, int64_t n, int m, int d,
                      const lsq_ivf_desc *desc);
// device pointers: K [m*256][d], q_scan [nq][d], q_coarse [nq][ldc], dists / ids [nq][nn] (ADC distances, original ids 1-based, (+inf, 0) past the probed
// rows).  adc: the index's scan state (the coarse search and the selection run on it); coarse: how the coarse search runs (the context's hooks)
int lsq_ivf_search(hipStream_t s, lsq_ivf_state *st, lsq_adc_state **adc, const float *K, float *dists, int *ids, const float *q_scan,
                   const float *q_coarse, int64_t ldc, int nq, int nprobe, int nn, int flags, const lsq_search_opts &coarse, int timed,
                   const struct lsq_filter_view *flt = nullptr);      // flt (lsq_filter.hip): its layout-order bits restrict the answer to the allowed rows

// the coarse step of lsq_ivf_search on its own, for a scan outside lsq_ivf.hip (lsq_range.hip): the probed lists of nq queries in rank order and their
// coarse distances ([nq][nprobe], device, in st's scratch: valid until the next call on st), and the layout they index
struct lsq_ivf_probes {
    const int *probe; const float *coarse;
    const uint8_t *codes; const float *norms; const int *ids; const int *off;      // norms: per position, or (packed) the norm table of 256 floats
    int64_t n; int nlist, m, d, packed;
};
int lsq_ivf_coarse(hipStream_t s, lsq_ivf_state *st, lsq_adc_state **adc, const float *q_coarse, int64_t ldc, int nq, int nprobe, const lsq_search_opts &coarse,
                   int timed, lsq_ivf_probes *out, double *coarse_ms);

// ---- range search on a resident index (lsq_range.hip): every candidate row within a radius, held by the index until fetched or dropped ------------------
struct lsq_range_state;
void lsq_range_free(lsq_range_state *st);
void lsq_range_drop(lsq_range_state *st);            // the held result leaves and its memory is released (st may be null)
void lsq_range_get_info(const lsq_range_state *st, lsq_range_info *out);
// one call, every pointer a device pointer.  in: the rows as lsq_adc_search takes them (kind LSQ, Q = q_scan rows d floats apart, a filter's road already
// chosen); on the list road (nprobe >= 1) only Q, K, n, m, d of it are read and the rows are ivf's layout
struct lsq_range_call {
    lsq_search_input in;
    const float *radius = nullptr;                   // [nq]
    int nq = 0, nprobe = 0, flags = 0;
    lsq_ivf_state *ivf = nullptr; lsq_adc_state **adc = nullptr;      // list road: the lists, and the scan state the coarse search runs on
    const float *q_coarse = nullptr; int64_t ldc = 0;
    lsq_search_opts coarse;                          // how the coarse search runs (the context's hooks)
    const uint32_t *lbits = nullptr;                 // list road under a filter: its bits in layout order
    int64_t budget = 0;                              // records per fill batch (lsq_range_budget)
    int timed = 0, road = 0;
    int64_t *lims_dev = nullptr;                     // optional: lims [nq + 1] also written here
};
// h_lims [nq + 1]: HOST.  Drops the former held result first; on success the new one is held.  Waits for the device
int lsq_range_search(hipStream_t s, lsq_range_state **st, const lsq_range_call &call, int64_t *h_lims);
int lsq_range_fetch(hipStream_t s, lsq_range_state *st, float *dists, int *ids, int64_t capacity, int on_device);

// ---- row filters on a resident index (lsq_filter.hip): the set of allowed rows as the scans read it ---------------------------------------------------
struct lsq_filter_state;
void lsq_filter_free(lsq_filter_state *st);
// what a scan is handed: bits [ceil(n/32)] (bits at and past n are zero), rows [allowed] ascending; the layout-order bitmap lbits (bit p = allowed(ids[p]))
// and the exclusive prefix lpre [ceil(n/32) + 1] of its words' popcounts, both null without inverted lists.  A view is valid until the next set / clear
struct lsq_filter_view {
    const uint32_t *bits = nullptr;
    const int *rows = nullptr;
    int64_t allowed = 0;
    const uint32_t *lbits = nullptr;
    const int *lpre = nullptr;
    int force = 0;                           // LSQ_FILTER_FORCE_DENSE / LSQ_FILTER_FORCE_COMPACT / 0
    const int *pre = nullptr;                // the exclusive prefix [ceil(n/32) + 1] of the popcounts of bits' words (lsq_index_compact: a row's rank)
};
// desc as lsq_index_set_filter takes it (never null here).  A refusal leaves *st as it was.  The call waits for the device (the count comes back)
int lsq_filter_set(hipStream_t s, lsq_filter_state **st, int64_t n, const lsq_filter_desc *desc);
void lsq_filter_clear(lsq_filter_state *st);
bool lsq_filter_active(const lsq_filter_state *st);
lsq_filter_view lsq_filter_get(const lsq_filter_state *st);
// the layout-order bitmap and its prefix for the inverted layout ids [n] / off [nlist + 1] (device); nlist = 0 drops them.  Called whenever either changed
int lsq_filter_layout(hipStream_t s, lsq_filter_state *st, const int *ids, const int *off, int64_t n, int nlist);
void lsq_filter_note_road(lsq_filter_state *st, int road);      // the last search / knn call's road: 0 unfiltered, 1 dense, 2 compact
void lsq_filter_get_info(const lsq_filter_state *st, int64_t n, lsq_filter_info *out);
// The default road (measured: profiles/filter.jsonl).  Compact when allowed <= crossover = n / 2: walking |A| rows through one indirection beat
// reading n rows and their bits at every measured fraction from 1/2 down -- except in one band.  Up to LSQ_SELECT_SMALL_N rows the selection writes and
// sorts EVERY distance (lsq_adc.hip: ADC_SMALL_N), which costs sort_over_scan times a dense scan's step per (query, row): where the dense road would still
// be on the thresholded selection (n above the limit), the compact road pays only when allowed * sort_over_scan <= n.  sort_over_scan: 64 for the ADC scan
// (measured 70 at m = 8), 8 for exact k-NN (6.8 at d = 128, f32) -- one shape each, rounded
constexpr int64_t LSQ_SELECT_SMALL_N = 65536;
inline int64_t lsq_filter_crossover(int64_t n) { return n / 2; }
inline bool lsq_filter_compact_by_default(int64_t n, int64_t allowed, int64_t sort_over_scan) {
    if (allowed > lsq_filter_crossover(n)) return false;
    return !(n > LSQ_SELECT_SMALL_N && allowed <= LSQ_SELECT_SMALL_N && allowed * sort_over_scan > n);
}
// the inverted layout a filter's layout bits are built over: ids [n] original row of every position, off [nlist + 1]; both null without lists
void lsq_ivf_layout(const lsq_ivf_state *st, const int **ids, const int **off);

// ---- rows grouped by list (lsq_ivf.hip): the sort behind lsq_index_set_lists and lsq_partition_update.  Scratch of whoever groups: the staged list of a
// host-buffer call, the keys (list << 32 | row) before and after the sort, the sort's workspace and the range check's counter ------------------------------
struct lsq_row_groups {
    DevBuf s_lor, keys_a, keys_b, tmp, flag;
    void release() { s_lor.release(); keys_a.release(); keys_b.release(); tmp.release(); flag.release(); }
};
// the keys and the range check: *bad = entries outside [0, nlist), read back (the call waits); with *bad != 0 nothing may be sorted
int lsq_rows_keys(hipStream_t s, lsq_row_groups &g, const int32_t *list_of_row, int on_device, int64_t n, int nlist, unsigned *bad);
// *sorted = the keys list by list and, within a list, ascending by row (in g: valid until the next lsq_rows_keys on it)
int lsq_rows_sort(hipStream_t s, lsq_row_groups &g, int64_t n, int nlist, const uint64_t **sorted);
// off[l] = the first position of list l in the sorted keys, off[nlist] = n
int lsq_rows_offsets(hipStream_t s, const uint64_t *sorted, int64_t n, int nlist, int *off);

// ---- appending rows to a resident index (lsq_grow.hip: the new kernels; the states' own parts live beside the states, in lsq_ivf.hip and lsq_filter.hip) --
// a buffer grown WITH its contents: allocate `bytes`, copy the first `keep` bytes device to device on s, swap, free the old block (hipFree waits for the
// device, so the copy has landed).  The transient peak is old plus new.  A view, or a buffer already that large, is left alone
int lsq_devbuf_grow(hipStream_t s, DevBuf &b, size_t bytes, size_t keep, const void *src = nullptr);      // src: where the contents are now (null: in b)
// the merge of the inverted layout, out of place.  Old position q of list l moves to q + add_off[l]; the j-th sorted new key (list l, new row r = its low
// word) lands at off[l + 1] + j with id n + r; noff[l] = off[l] + add_off[l].  src / dst: the layout's code rows (rowb bytes), norms (null: packed) and ids;
// add_rows [count][rowb] / add_norms [count]: the new rows in the order they were appended.  dst buffers hold (n + count) rows and 16 bytes of slack
struct lsq_grow_merge {
    const uint8_t *src_codes; const float *src_norms; const int *src_ids; const int *off;
    uint8_t *dst_codes; float *dst_norms; int *dst_ids; int *noff;
    const int *add_off; const uint64_t *sorted; const uint8_t *add_rows; const float *add_norms;
    int64_t n, count; int nlist, rowb;
};
int lsq_grow_launch_merge(hipStream_t s, const lsq_grow_merge &g);
// words: bits n0 .. n1 - 1 set (the words past n0's own are whole: the caller zeroed or copied everything before n0, nothing after it matters before this)
int lsq_grow_launch_set_bits(hipStream_t s, uint32_t *words, int64_t n0, int64_t n1);
// the inverted lists' part (lsq_ivf.hip).  check: the keys of the `count` new rows and the range check (*bad: entries outside [0, nlist); the call waits) --
// nothing of the layout is touched.  reserve: both halves of the layout hold cap_rows rows (*realloc = 1 when anything was allocated).  merge: the layout of
// n + count rows written into the spare half (after check, same count); commit: the spare half becomes the layout
int lsq_ivf_add_check(hipStream_t s, lsq_ivf_state *st, const int32_t *list_of_row, int on_device, int64_t count, unsigned *bad);
int lsq_ivf_reserve(hipStream_t s, lsq_ivf_state *st, int64_t cap_rows, int *realloc);
int lsq_ivf_add_merge(hipStream_t s, lsq_ivf_state *st, const uint8_t *add_rows, const float *add_norms, int64_t count, int64_t cap_rows, int *realloc);
void lsq_ivf_add_commit(lsq_ivf_state *st, int64_t count);
// the filter's part (lsq_filter.hip): the filter of n_new rows -- the former bits and every row from the former n on -- built beside the one in force;
// commit puts it in force (the layout-order bits are then lsq_filter_layout's to rebuild).  Both do nothing without an active filter
int lsq_filter_grow(hipStream_t s, lsq_filter_state *st, int64_t n_new);
void lsq_filter_grow_commit(lsq_filter_state *st, int64_t n_new);

// ---- removing rows from a resident index (lsq_compact.hip: the new kernels; the states' own parts live beside the states) -----------------------------
// one stream gathered: dst row j = src row sel[j], rows rowb bytes apart in both, rows_out rows of which the last is lastb <= rowb bytes long.  dst is
// 16-byte aligned and holds the stream's bytes; every dword read of src holds a wanted byte.  *bytes (optional) += the destination bytes
int lsq_compact_launch_gather(hipStream_t s, const void *src, void *dst, const int *sel, int64_t rowb, int64_t rows_out, int64_t lastb, int64_t *bytes);
// the inverted layout of the survivors, out of place: position j of dst = position lsel[j] of src (lsel: the set bits of lbits, ascending), its id the rank
// of the old id under (bits, pre); noff[l] = the set bits of lbits below off[l]
struct lsq_compact_layout {
    const uint8_t *src_codes; const float *src_norms; const int *src_ids; const int *off;
    uint8_t *dst_codes; float *dst_norms; int *dst_ids; int *noff;
    const uint32_t *lbits; const int *lpre; const int *lsel; const uint32_t *bits; const int *pre;
    int64_t rows_out; int nlist, rowb;
};
int lsq_compact_launch_layout(hipStream_t s, const lsq_compact_layout &g, int64_t *bytes);
// the caller's maps in id_base (either may be null): new_of_old [n] (-1: removed), old_of_new [allowed].  bits == null: identities (rows is not read)
int lsq_compact_launch_maps(hipStream_t s, const uint32_t *bits, const int *pre, const int *rows, int64_t n, int64_t allowed, int id_base, int *old_of_new,
                            int *new_of_old);
// an owned buffer re-allocated to exactly `bytes` with its first `keep` bytes (allocate, copy, swap, free); nothing to do for an empty one or a view
int lsq_devbuf_fit(hipStream_t s, DevBuf &b, size_t bytes, size_t keep);
// the filter's part (lsq_filter.hip).  remove: the filter in force (or every row) minus the given rows, built beside it and put in force -- *bad: ids
// outside [id_base, id_base + n), then nothing has changed; *cleared: the bits newly cleared.  The call waits.  layout_rows: the set bits of the
// layout-order bitmap, ascending ([allowed] ints of the filter's scratch, valid until the next filter call)
int lsq_filter_remove(hipStream_t s, lsq_filter_state **st, int64_t n, const int32_t *ids, int64_t count, int id_base, int on_device, unsigned *bad,
                      int64_t *cleared);
int lsq_filter_layout_rows(hipStream_t s, lsq_filter_state *st, int64_t n, const int **lsel);
// the inverted lists' part (lsq_ivf.hip).  compact: the layout of the rows_out survivors written into the spare half (sized cap_rows; exact: re-allocated
// to just that); commit: the spare half becomes the layout of rows_out rows; fit: both halves re-allocated to exactly `rows` rows, contents kept
int lsq_ivf_compact(hipStream_t s, lsq_ivf_state *st, const lsq_filter_view &v, const int *lsel, int64_t rows_out, int64_t cap_rows, bool exact, int64_t *bytes);
void lsq_ivf_compact_commit(lsq_ivf_state *st, int64_t rows_out);
int lsq_ivf_fit(hipStream_t s, lsq_ivf_state *st, int64_t rows);

// ---- decode on the device (lsq_recon.hip): the vectors the codes stand for ---------------------------------------------------------------
// one decode, every pointer a device pointer: out row r (r < count; rows ldo floats apart) = the reconstruction of row ids[r] - id_base (ids != null) or
// start + r of codes (rows ldc >= m bytes apart, n of them addressable), from +0.0, codebooks ascending; cent != null: one more rounded add of
// cent[lor[row]] (both [..][d] / [n]).  An id outside [0, n) writes a row of 0x7FC00000 with pad_nan and nothing without (the caller has refused it before).
// No allocation, no wait: graph-capturable.  *road (optional): LSQ_RECON_ROAD_* of the launch
struct lsq_recon_call {
    const uint8_t *codes = nullptr; int64_t ldc = 0;
    const float *K = nullptr; int d = 0, m = 0;
    int64_t n = 0;
    const int32_t *ids = nullptr; int id_base = 0;
    int64_t start = 0, count = 0;
    float *out = nullptr; int64_t ldo = 0;
    const float *cent = nullptr; const int32_t *lor = nullptr; int nlist = 0;
    int pad_nan = 0;
};
int lsq_recon_launch(hipStream_t s, const lsq_recon_call &c, int *road);
// *bad (device, zeroed by the caller) += the ids outside [id_base, id_base + n)
int lsq_recon_launch_check_ids(hipStream_t s, const int32_t *ids, int64_t count, int id_base, int64_t n, unsigned *bad);
// lor [n] = the list of every original row, from the inverted layout ids [n] / off [nlist + 1]
int lsq_recon_launch_lor(hipStream_t s, const int *ids, const int *off, int64_t n, int nlist, int32_t *lor);
// the centroids of the inverted lists [nlist][d] (lsq_ivf.hip); null without lists
const float *lsq_ivf_centroids(const lsq_ivf_state *st);

// ---- half-precision base rows (lsq_half.hip): the streaming converts between f32 rows and rows of 2-byte (or 1-byte) elements -------------------
// dst row i (d halves apart: DENSE, 16-byte aligned) = narrow(src row i, lds floats apart; src 4-byte aligned), format LSQ_BASE_F16 / LSQ_BASE_BF16.  counts
// (device, zeroed by the caller) [0] += finite values that became +-inf, [1] += non-zero values that became +-0, [2] += NaNs.  No allocation, no wait
int lsq_half_launch_narrow(hipStream_t s, const float *src, int64_t lds, void *dst, int64_t n, int d, int format, unsigned long long *counts);
// dst row r (ldo floats apart, 4-byte aligned) = widen(src row r, lds elements apart) for count rows of d elements of `format` (1: uint8, or a half format)
int lsq_half_launch_widen(hipStream_t s, const void *src, int format, int64_t lds, float *dst, int64_t ldo, int64_t count, int d);

// ---- snapshots (lsq_snapshot.hip): the digest of a device byte range and the unpacking of packed rows ----------------------------------------
// *acc (device) += the digest of `bytes` bytes at p (any alignment) whose first byte is byte 0 of word first_word of its section: chunks of a section add up
// in stream order.  partials: LSQ_SNAP_PARTIALS 64-bit words of device scratch.  No allocation, no wait
constexpr int LSQ_SNAP_PARTIALS = 2048;
int lsq_snap_launch_digest(hipStream_t s, const void *p, uint64_t bytes, uint64_t first_word, unsigned long long *partials, unsigned long long *acc);
// packed rows [n][m + 1] -> bytes [c0, c0 + cbytes) of the codes stream [n][m] at codes_out and the norm bytes of rows [r0, r0 + rcount) at norms_out (either
// may be null: not wanted)
int lsq_snap_launch_unpack(hipStream_t s, const uint8_t *rows, int64_t n, int m, uint8_t *codes_out, int64_t c0, int64_t cbytes, uint8_t *norms_out, int64_t r0,
                           int64_t rcount);

// ---- what a handle that lives in a file of its own (lsq_partition.hip) needs of its context (lsq_api.hip): its device made current, the stream it is bound
// to now, option "profile".  Nothing of the context is written ------------------------------------------------------------------------------------------
int lsq_ctx_bind(lsq_ctx *c, hipStream_t *stream, int *profile);

// argument checks of the PQ / OPQ scan (lsq_linscan.hip), shared by the host drop-in and the device scan
int lsq_linscan_pq_check(const char *fn, const void *dists, const void *res, const void *codes, const void *centers, const void *queries, int N,
                         uint32_t NQ, int B, int K, int dim1codes, int dim1queries, int subdim);

// ---- quantize_norms on the device (lsq_norms.hip): codes [n][stride] u8 0-based; any of the four outputs may be null ----------------------
int lsq_launch_quantize_norms(hipStream_t s, const uint8_t *codes, int stride, const float *K, const float *cb, int ncb, int64_t n, int d, int m,
                              uint8_t *idx0, int16_t *idx1, float *dbnorms, float *norms);

// ---- LSQR codebook update on the device (lsq_lsqr.hip) ---------------------------------------------------------------------------------------
struct lsq_lsqr_state;
void lsq_lsqr_free(lsq_lsqr_state *st);
int lsq_lsqr_update_codebooks(hipStream_t s, lsq_lsqr_state **st, const float *dX, const uint8_t *dcodes, const uint8_t *cover, int d, int64_t n, int m,
                              float *dK, int *iters_out);      // cover: HOST bytes [m][d] (0 / 1) of a structured update, or null
// the rows of a code matrix sorted by (codebook j, code) once per call: keys and segment starts live in `buf` (shared by lsq_lsqr.hip and lsq_spgl1.hip)
int lsq_sort_rows_by_code(hipStream_t s, DevBuf &buf, const uint8_t *dcodes, int64_t n, int m, const uint64_t **sorted, const int64_t **seg);

// ---- cluster means and k-means++ seeding on the device (lsq_kmeans.hip) -------------------------------------------------------------------------------
struct lsq_kmeans_state;
void lsq_kmeans_free(lsq_kmeans_state *st);
// cover: HOST bytes [m][d] (0 / 1, no empty codebook); dKprev optional (may be dK); dcounts optional [m*256] int32
int lsq_kmeans_update_centers(hipStream_t s, lsq_kmeans_state **st, const float *dX, const uint8_t *dcodes, const uint8_t *cover, const float *dKprev, int d,
                              int64_t n, int m, float *dK, int *dcounts);
// u: HOST [m][256] doubles in [0, 1); didx optional [m][256] int64; dd2 optional [n][m] f32; n >= 1
int lsq_kmeans_seed(hipStream_t s, lsq_kmeans_state **st, const float *dX, const uint8_t *cover, const double *u, int d, int64_t n, int m, float *dK,
                    int64_t *didx, float *dd2);
int lsq_kmeans_fill_i64(hipStream_t s, int64_t *p, int64_t count, int64_t v);

// ---- SPGL1 (LASSO) codebook update on the device (lsq_spgl1.hip) ---------------------------------------------------------------------------------
struct lsq_spgl1_state;
void lsq_spgl1_free(lsq_spgl1_state *st);
// dX [n][d], dcodes [n][m] u8 0-based, dK0 [m*256][d] (optional warm start), dK [m*256][d] (output); all device pointers.  S < 0: no threshold.
int lsq_spgl1_update_codebooks(hipStream_t s, lsq_spgl1_state **st, const float *dX, const uint8_t *dcodes, int d, int64_t n, int m, double tau,
                               const float *dK0, int64_t S, double opt_tol, int64_t max_iter, float *dK, lsq_spgl1_info *info);
