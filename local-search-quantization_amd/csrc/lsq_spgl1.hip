// lsq_spgl1.hip -- the sparse codebook update ON THE DEVICE: SPGL1's LASSO mode for update_codebooks_spgl1(_threshold).
//
// Reference: src/codebook_update_sparse.jl calls MATLAB's spgl1(A, Xt(:), tau, [], prevKt(:)) on the operator of matlab/sparse_lsq_fun.m,
//     minimise 1/2 ||A k - b||^2  s.t.  ||k||_1 <= tau,   A = I_d (x) S,  S = sparsify_codes(B, h),  b = vec(X'),
// then keeps the S entries of the Float32 K largest in |K|.  SPGL1 itself is not vendored; this is a restatement of its single-tau mode from
// van den Berg & Friedlander, SIAM J. Sci. Comput. 31(2), 2008 (spgSetParms defaults), in float64:
//   - spectral projected gradient; the first step 1 / ||P(x - g) - x||_inf, then Barzilai-Borwein s's / s'y (stepMax when s'y <= 0), clamped;
//   - spgLineCurvy: x(step) = P(x - step scale gStep g), accepted when f < max(last 3 f) + 1e-4 step g's, at most 10 halvings, SPGL1's safeguard
//     that damps `scale` when two trials project to the same point; failing that, spgLine along the feasible direction P(x - gStep g) - x with
//     safeguarded quadratic interpolation; failing that too, the iterate is kept and stepMax is divided by 10 (at most 10 times);
//   - stop when |r'(r - b) + tau ||A'r||_inf| / max(1, f) <= optTol or ||r|| < optTol ||b||.
// The operator is never formed.  K is the [m h][d] matrix of the rest of the project (its flat index is Julia's column-major index of hcat(C...)):
//     (A k)[i][t]  = SUM_j k[j h + b_ij][t]          residual pass, codebooks ascending, one thread per (row, dimension)
//     (A'r)[c][t]  = SUM of r[i][t] over rows holding c   the rows sorted by code once per call (lsq_sort_rows_by_code, the LSQR path's sort):
//                                                       a thread walks its column's rows in ascending order, no atomics
// The projection onto the l1 ball sorts |v| (radix sort of the f64 bit patterns, descending) and scans the sorted values in a fixed order
// (SPGL1's oneProjector: theta = (c_k - tau) / k for the largest k with u_k > (c_k - tau) / k).  Every reduction adds fixed item sets in a fixed
// order and every maximum is exact, so a call returns the same bits every time.  The scalar logic runs in one-block kernels; the host reads one
// control word per line-search trial: the word after an accepted step also carries the gap test of the next iteration and the result of that
// iteration's first trial, enqueued before the read (one read per iteration when the first trial is accepted, the usual case).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <new>
#include <utility>

#include "lsq_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int EPT = 8;                 // elements per thread of the element-wise passes
constexpr int EB = 256 * EPT;          // elements per block
constexpr int GT = 64;                 // dimensions per block of the gradient pass
constexpr int MAXB = 1024;             // blocks of an element-wise pass at most (a fixed function of the size: a block strides over the rest)
constexpr int NSLOT = 6;               // partial-sum slots: 0 g's | g'dx | s's(BB) | |K|   1 s's | s'y(BB) | nnz   2 r'r   3 b'r   4 b'b   5 g'g

enum { RES_RETRY = 0, RES_ACCEPT = 1, RES_FAIL = 2 };
enum { STOP_NONE = 0, STOP_OPTIMAL = 1, STOP_LINE_ERROR = 2 };
enum { PROJ_COPY = 0, PROJ_ZERO = 1, PROJ_THETA = 2 };
enum { PH_THETA, PH_INIT, PH_GSTEP, PH_CURVY, PH_FEAS_BEGIN, PH_FEAS, PH_REVERT, PH_BB, PH_RECERT, PH_FINAL, PH_NNZ };
enum { V_LOAD = 0, V_XG = 1 };
enum { A_X = 0, A_DX = 1, A_CURVY = 2 };

struct SpgState {
    int ctl[4];                        // read by the host: [0] trial result, [1] stop, [2] the iterate is worse than the best one, [3] unused
    double tau, opt_tol, step_min, step_max, bnorm, nfl;
    double f, f_best, last[3], g_step, fmax;
    double f_new, rr_new, br_new;      // the trial's values, committed when the host accepts it
    double rr, br, gnorm, rel_gap;
    double step, scale, s_norm, gtd, alpha;
    double sum_abs_v, l1;
    unsigned long long kstar, gmax_bits, dxmax_bits;
    long long it, nnz, nnz_before;
    int n_safe, ls_k, line_errors_left, improved, proj;
};

__device__ inline double dmax_bits(unsigned long long b) { return __longlong_as_double((long long)b); }

// block-wide sums of Q values per thread in a fixed tree (256 threads); thread 0 writes part[slot[q] * MAXB + blk]
template <int Q>
__device__ inline void block_sums(double (&v)[Q], double *part, const int (&slot)[Q], int64_t blk) {
    __shared__ double red[Q][256];
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < Q; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < Q; ++q) red[q][tid] += red[q][tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) part[(int64_t)slot[q] * MAXB + blk] = red[q][0];
    }
}

__device__ inline void block_max_to(double v, unsigned long long *dst) {        // |values| >= 0: their bit patterns order like the values
    __shared__ unsigned long long mx[256];
    const int tid = threadIdx.x;
    mx[tid] = (unsigned long long)__double_as_longlong(v);
    __syncthreads();
    for (int w = blockDim.x >> 1; w > 0; w >>= 1) {
        if (tid < w && mx[tid + w] > mx[tid]) mx[tid] = mx[tid + w];
        __syncthreads();
    }
    if (tid == 0 && mx[0] > *(volatile unsigned long long *)dst) atomicMax(dst, mx[0]);
}

__global__ void spg_setup(SpgState *st, double tau, double opt_tol, double nfl) {
    st->ctl[0] = st->ctl[1] = st->ctl[2] = st->ctl[3] = 0;
    st->tau = tau; st->opt_tol = opt_tol; st->step_min = 1e-16; st->step_max = 1e5; st->nfl = nfl;
    st->line_errors_left = 10;
    st->kstar = st->gmax_bits = st->dxmax_bits = 0;
    st->it = 0; st->alpha = 1.0; st->improved = 0;
}

// v = K_init (or 0)  |  v = x - alpha g;  keys = bits of |v|;  slot 0: SUM |v|
__global__ __launch_bounds__(256) void spg_vkeys(const double *__restrict__ x, const double *__restrict__ g, const float *__restrict__ k0,
                                                 double *__restrict__ v, uint64_t *__restrict__ keys, int64_t N, const SpgState *st, int mode,
                                                 double *__restrict__ part) {
    const double alpha = st->alpha;
    double acc[1] = {0.0};
    for (int64_t base = (int64_t)blockIdx.x * EB; base < N; base += (int64_t)gridDim.x * EB) {
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int64_t e = base + k * 256 + threadIdx.x;
            if (e >= N) break;
            const double vv = mode == V_LOAD ? (k0 ? (double)k0[e] : 0.0) : x[e] - alpha * g[e];
            const double a = fabs(vv);
            v[e] = vv;
            keys[e] = (uint64_t)__double_as_longlong(a);
            acc[0] += a;
        }
    }
    block_sums<1>(acc, part, {0}, blockIdx.x);
}

// the sum of each 2048-item tile of the sorted |v| (thread t adds its 8 consecutive items, the block adds the 256 sums in a fixed tree)
__global__ __launch_bounds__(256) void spg_tile_sums(const uint64_t *__restrict__ sorted, int64_t N, double *__restrict__ tilesum) {
    double acc[1] = {0.0};
    const int64_t p0 = (int64_t)blockIdx.x * EB + (int64_t)threadIdx.x * EPT;
    for (int k = 0; k < EPT && p0 + k < N; ++k) acc[0] += __longlong_as_double((long long)sorted[p0 + k]);
    __shared__ double red[256];
    red[threadIdx.x] = acc[0];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) tilesum[blockIdx.x] = red[0];
}

// prefix sums c_p of the sorted |v| (tile prefix + the thread's exclusive prefix + its own items in order) and the largest k with u_k > (c_k - tau) / k
__global__ __launch_bounds__(256) void spg_scan_find(const uint64_t *__restrict__ sorted, int64_t N, const double *__restrict__ tilepre,
                                                     double *__restrict__ csum, SpgState *st) {
    if (st->proj != PROJ_THETA) return;
    const double tau = st->tau;
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * EB + (int64_t)tid * EPT;
    double u[EPT], tsum = 0.0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) { u[k] = p0 + k < N ? __longlong_as_double((long long)sorted[p0 + k]) : 0.0; tsum += u[k]; }
    __shared__ double sc[256];
    sc[tid] = tsum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                      // inclusive Hillis-Steele scan: a fixed association per position
        const double add = tid >= off ? sc[tid - off] : 0.0;
        __syncthreads();
        sc[tid] += add;
        __syncthreads();
    }
    double c = tilepre[blockIdx.x] + (tid > 0 ? sc[tid - 1] : 0.0);
    unsigned long long best = 0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int64_t p = p0 + k;
        if (p >= N) break;
        c += u[k];
        csum[p] = c;
        if (u[k] > (c - tau) / (double)(p + 1)) best = (unsigned long long)(p + 1);
    }
    __shared__ unsigned long long mx[256];
    mx[tid] = best;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && mx[tid + w] > mx[tid]) mx[tid] = mx[tid + w];
        __syncthreads();
    }
    if (tid == 0 && mx[0] != 0) atomicMax(&st->kstar, mx[0]);
}

// p = P(v).  A_X: out = p.  A_DX: v <- p - x (in place), slot 0: g'dx, max |dx|.  A_CURVY: out = p, slots 0, 1, 5: g's, s's, g'g  (s = p - x)
__global__ __launch_bounds__(256) void spg_apply(double *v, double *out, const double *x, const double *__restrict__ g,
                                                 const double *__restrict__ csum, int64_t N, SpgState *st, int mode, double *__restrict__ part) {
    const int proj = st->proj;
    double theta = 0.0;
    if (proj == PROJ_THETA) { const unsigned long long k = st->kstar; theta = k ? (csum[k - 1] - st->tau) / (double)k : 0.0; }
    double acc[3] = {0.0, 0.0, 0.0}, mx = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * EB; base < N; base += (int64_t)gridDim.x * EB) {
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int64_t e = base + k * 256 + threadIdx.x;
            if (e >= N) break;
            const double vv = v[e];
            double p;
            if (proj == PROJ_COPY) p = vv;
            else if (proj == PROJ_ZERO) p = 0.0;
            else p = fabs(vv) > theta ? copysign(fabs(vv) - theta, vv) : 0.0;
            if (mode == A_X) { out[e] = p; continue; }
            const double sd = p - x[e], ge = g[e];
            if (mode == A_DX) { v[e] = sd; acc[0] += ge * sd; mx = fmax(mx, fabs(sd)); }
            else { out[e] = p; acc[0] += ge * sd; acc[1] += sd * sd; acc[2] += ge * ge; }
        }
    }
    if (mode == A_X) return;
    if (mode == A_DX) { double a1[1] = {acc[0]}; block_sums<1>(a1, part, {0}, blockIdx.x); block_max_to(mx, &st->dxmax_bits); }
    else block_sums<3>(acc, part, {0, 1, 5}, blockIdx.x);
}

// xN = x + step dx  (the feasible-direction trials)
__global__ __launch_bounds__(256) void spg_feas_x(const double *__restrict__ x, const double *__restrict__ dx, double *__restrict__ xn, int64_t N,
                                                  const SpgState *st) {
    const double step = st->step;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < N) xn[e] = x[e] + step * dx[e];
}

// r = b - A k, row by row (codebooks ascending); slots 2, 3, 4: r'r, b'r, b'b
__global__ __launch_bounds__(256) void spg_residual(const float *__restrict__ X, const uint8_t *__restrict__ codes, const double *__restrict__ kv,
                                                    double *__restrict__ r, int64_t nd, int d, int m, double *__restrict__ part) {
    double acc[3] = {0.0, 0.0, 0.0};
    const bool narrow = nd < ((int64_t)1 << 32);
    for (int64_t base = (int64_t)blockIdx.x * EB; base < nd; base += (int64_t)gridDim.x * EB) {
        for (int k = 0; k < EPT; ++k) {
            const int64_t e = base + k * 256 + threadIdx.x;
            if (e >= nd) break;
            const int64_t i = narrow ? (int64_t)((uint32_t)e / (uint32_t)d) : e / d;
            const int t = (int)(e - i * d);
            const uint8_t *c = codes + i * m;
            double rec = 0.0;
            for (int j = 0; j < m; ++j) rec += kv[((int64_t)j * LSQ_H + c[j]) * d + t];
            const double b = (double)X[e];
            const double re = b - rec;
            r[e] = re;
            acc[0] += re * re; acc[1] += b * re; acc[2] += b * b;
        }
    }
    block_sums<3>(acc, part, {2, 3, 4}, blockIdx.x);
}

// g = -A'r: one thread per (column, dimension) walks the column's rows in ascending order; max |g|
__global__ __launch_bounds__(GT) void spg_gradient(const double *__restrict__ r, const uint64_t *__restrict__ sorted, const int64_t *__restrict__ seg,
                                                   int d, double *__restrict__ g, SpgState *st) {
    const int c = blockIdx.x, t = blockIdx.y * GT + threadIdx.x;
    double gv = 0.0;
    if (t < d) {
        const int64_t e0 = seg[c], e1 = seg[c + 1];
        double acc = 0.0;
        int64_t e = e0;
        for (; e + 8 <= e1; e += 8) {                                 // eight rows in flight; the additions stay in row order
            double u[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) u[q] = r[(int64_t)(uint32_t)sorted[e + q] * d + t];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc += u[q];
        }
        for (; e < e1; ++e) acc += r[(int64_t)(uint32_t)sorted[e] * d + t];
        gv = -acc;
        g[(int64_t)c * d + t] = gv;
    }
    block_max_to(fabs(gv), &st->gmax_bits);
}

// Barzilai-Borwein scalars: slots 0, 1: s's, s'y  (s = x - xo, y = g - go)
__global__ __launch_bounds__(256) void spg_bb(const double *__restrict__ x, const double *__restrict__ xo, const double *__restrict__ g,
                                              const double *__restrict__ go, int64_t N, double *__restrict__ part) {
    double acc[2] = {0.0, 0.0};
    for (int64_t base = (int64_t)blockIdx.x * EB; base < N; base += (int64_t)gridDim.x * EB) {
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int64_t e = base + k * 256 + threadIdx.x;
            if (e >= N) break;
            const double sd = x[e] - xo[e], y = g[e] - go[e];
            acc[0] += sd * sd; acc[1] += sd * y;
        }
    }
    block_sums<2>(acc, part, {0, 1}, blockIdx.x);
}

// K = (float) x;  slot 0: SUM |K| (of the f32 values), slot 1: nnz.  convert = 0: count the non-zeros of K only
__global__ __launch_bounds__(256) void spg_finish(const double *__restrict__ x, float *__restrict__ K, int64_t N, int convert, double *__restrict__ part) {
    double acc[2] = {0.0, 0.0};
    for (int64_t base = (int64_t)blockIdx.x * EB; base < N; base += (int64_t)gridDim.x * EB) {
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int64_t e = base + k * 256 + threadIdx.x;
            if (e >= N) break;
            float kv;
            if (convert) { kv = (float)x[e]; K[e] = kv; } else kv = K[e];
            acc[0] += fabs((double)kv);
            acc[1] += kv != 0.0f ? 1.0 : 0.0;
        }
    }
    block_sums<2>(acc, part, {0, 1}, blockIdx.x);
}

// hard threshold: keys (|K| bits << 32 | ~index) sorted descending = larger |K| first, the lower index first on ties; positions >= S become +0
__global__ __launch_bounds__(256) void spg_tkeys(const float *__restrict__ K, int64_t N, uint64_t *__restrict__ keys) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const uint32_t a = __float_as_uint(K[e]) & 0x7fffffffu;
    keys[e] = ((uint64_t)a << 32) | (uint64_t)(0xffffffffu - (uint32_t)e);
}
__global__ __launch_bounds__(256) void spg_tzero(const uint64_t *__restrict__ sorted, int64_t S, int64_t N, float *__restrict__ K) {
    const int64_t p = S + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    K[0xffffffffu - (uint32_t)sorted[p]] = 0.0f;
}

__global__ __launch_bounds__(256) void spg_copy_best(const double *__restrict__ x, double *__restrict__ xb, int64_t N, const SpgState *st) {
    if (!st->improved) return;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < N) xb[e] = x[e];
}

// ---- scalar logic ---------------------------------------------------------------------------------------------------------------------------
__device__ void stop_and_begin(SpgState *st) {
    st->gnorm = dmax_bits(st->gmax_bits);
    const double gap = (st->rr - st->br) + st->tau * st->gnorm;            // r'(r - b) + tau ||A'r||_inf
    st->rel_gap = fabs(gap) / fmax(1.0, st->f);
    const double rnorm = sqrt(st->rr);
    if (st->rel_gap <= st->opt_tol || rnorm < st->opt_tol * st->bnorm) st->ctl[1] = STOP_OPTIMAL;
    st->ctl[2] = st->f > st->f_best;
    // spgLineCurvy's start
    st->step = 1.0; st->scale = 1.0; st->s_norm = 0.0; st->n_safe = 0; st->ls_k = 0;
    st->fmax = fmax(fmax(st->last[0], st->last[1]), st->last[2]);
    st->alpha = st->g_step;
    st->ctl[0] = RES_RETRY;
}

__device__ void end_iteration(SpgState *st) {                             // function history and the best iterate
    st->it += 1;
    st->last[st->it % 3] = st->f;
    st->improved = st->f < st->f_best;
    if (st->improved) st->f_best = st->f;
}

// one block of 256 threads: sums of slots 0, 1, 5 over nbA blocks and of slots 2, 3, 4 over nbB blocks (<= MAXB each) in a fixed order, the prefix
// sums of the tiles (PH_THETA), then thread 0's step
__global__ __launch_bounds__(256) void spg_ctl(SpgState *st, const double *__restrict__ part, int nbA, int nbB, const double *__restrict__ tilesum,
                                               double *__restrict__ tilepre, int64_t ntiles, int phase) {
    const int tid = threadIdx.x;
    __shared__ double red[NSLOT][256];
    __shared__ double S[NSLOT];
    {
        double val[NSLOT][MAXB / 256];
#pragma unroll
        for (int q = 0; q < NSLOT; ++q) {
            const int nb = (q >= 2 && q <= 4) ? nbB : nbA;
#pragma unroll
            for (int k = 0; k < MAXB / 256; ++k) { const int b = tid + 256 * k; val[q][k] = b < nb ? part[(int64_t)q * MAXB + b] : 0.0; }
        }
#pragma unroll
        for (int q = 0; q < NSLOT; ++q) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < MAXB / 256; ++k) a += val[q][k];
            red[q][tid] = a;
        }
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w)
                for (int q = 0; q < NSLOT; ++q) red[q][tid] += red[q][tid + w];
            __syncthreads();
        }
        if (tid == 0)
            for (int q = 0; q < NSLOT; ++q) S[q] = red[q][0];
        __syncthreads();
    }
    if (phase == PH_THETA) {                                                // exclusive prefix sums of the tile sums: a thread adds a contiguous run
        const int64_t chunk = (ntiles + 255) / 256, q0 = tid * chunk, q1 = q0 + chunk < ntiles ? q0 + chunk : ntiles;
        double own = 0.0;
        for (int64_t q = q0; q < q1; ++q) own += tilesum[q];
        __shared__ double sc[256];
        sc[tid] = own;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const double add = tid >= off ? sc[tid - off] : 0.0;
            __syncthreads();
            sc[tid] += add;
            __syncthreads();
        }
        double c = tid > 0 ? sc[tid - 1] : 0.0;
        for (int64_t q = q0; q < q1; ++q) { tilepre[q] = c; c += tilesum[q]; }
    }
    if (threadIdx.x != 0) return;
    switch (phase) {
    case PH_THETA: {                                                        // after the keys and the tile sums: how to project
        st->sum_abs_v = S[0];
        st->proj = st->tau <= 0.0 ? PROJ_ZERO : (S[0] <= st->tau ? PROJ_COPY : PROJ_THETA);
        st->kstar = 0;
        st->dxmax_bits = 0;
        break;
    }
    case PH_INIT:                                                           // x0 projected, its residual and gradient
        st->rr = S[2]; st->br = S[3]; st->bnorm = sqrt(S[4]);
        st->f = 0.5 * S[2];
        st->last[0] = st->f; st->last[1] = -INFINITY; st->last[2] = -INFINITY;
        st->f_best = st->f; st->improved = 1;
        st->alpha = 1.0;                                                    // the first step's direction: P(x - g) - x
        break;
    case PH_GSTEP: {
        const double dxn = dmax_bits(st->dxmax_bits);
        st->g_step = dxn < 1.0 / st->step_max ? st->step_max : fmin(st->step_max, fmax(st->step_min, 1.0 / dxn));
        stop_and_begin(st);
        break;
    }
    case PH_CURVY: {                                                        // a trial of spgLineCurvy: x(step) and its residual
        const double fn = 0.5 * S[2];
        const double gts = st->scale * (st->g_step * S[0]);
        st->f_new = fn; st->rr_new = S[2]; st->br_new = S[3];
        if (gts >= 0.0) st->ctl[0] = RES_FAIL;
        else if (fn < st->fmax + 1e-4 * st->step * gts) st->ctl[0] = RES_ACCEPT;
        else if (st->ls_k >= 10) st->ctl[0] = RES_FAIL;
        else {
            st->ls_k += 1;
            st->step = st->step / 2.0;
            const double s_old = st->s_norm;
            st->s_norm = sqrt(S[1]) / st->nfl;
            if (fabs(st->s_norm - s_old) <= 1e-6 * st->s_norm) {           // two trials projected to (nearly) the same point: damp the direction
                const double gn = st->g_step * sqrt(S[5]) / st->nfl;
                st->scale = st->s_norm / gn / ldexp(1.0, st->n_safe);
                st->n_safe += 1;
            }
            st->ctl[0] = RES_RETRY;
        }
        st->alpha = st->ctl[0] == RES_FAIL ? st->g_step : st->step * st->scale * st->g_step;
        break;
    }
    case PH_FEAS_BEGIN:                                                     // the feasible direction dx = P(x - gStep g) - x is in place
        st->gtd = -fabs(S[0]);
        st->step = 1.0; st->ls_k = 0;
        break;
    case PH_FEAS: {                                                         // a trial of spgLine: x + step dx
        const double fn = 0.5 * S[2];
        st->f_new = fn; st->rr_new = S[2]; st->br_new = S[3];
        if (fn < st->fmax + 1e-4 * st->step * st->gtd) st->ctl[0] = RES_ACCEPT;
        else if (st->ls_k >= 10) st->ctl[0] = RES_FAIL;
        else {
            st->ls_k += 1;
            const double step = st->step;
            if (step <= 0.1) st->step = step / 2.0;
            else {
                double tmp = (-st->gtd * step * step) / (2.0 * (fn - st->f - step * st->gtd));
                if (!(tmp >= 0.1 && tmp <= 0.9 * step)) tmp = step / 2.0;      // NaN included
                st->step = tmp;
            }
            st->ctl[0] = RES_RETRY;
        }
        break;
    }
    case PH_REVERT: {                                                       // both searches failed: keep x, damp the largest BB step
        int stop = STOP_NONE;
        if (st->line_errors_left <= 0) stop = STOP_LINE_ERROR;
        else { st->step_max /= 10.0; st->line_errors_left -= 1; }
        st->g_step = fmin(st->step_max, st->g_step);
        end_iteration(st);
        stop_and_begin(st);
        if (stop != STOP_NONE && st->ctl[1] == STOP_NONE) st->ctl[1] = stop;
        break;
    }
    case PH_BB: {                                                           // an accepted step: commit it, Barzilai-Borwein step from s's / s'y
        st->f = st->f_new; st->rr = st->rr_new; st->br = st->br_new;
        const double sts = S[0], sty = S[1];
        st->g_step = sty <= 0.0 ? st->step_max : fmin(st->step_max, fmax(st->step_min, sts / sty));
        end_iteration(st);
        stop_and_begin(st);
        break;
    }
    case PH_RECERT:                                                         // the best iterate restored: its residual and gradient
        st->rr = S[2]; st->br = S[3]; st->f = 0.5 * S[2];
        st->gnorm = dmax_bits(st->gmax_bits);
        st->rel_gap = fabs((st->rr - st->br) + st->tau * st->gnorm) / fmax(1.0, st->f);
        break;
    case PH_FINAL:
        st->l1 = S[0];
        st->nnz_before = st->nnz = (long long)S[1];
        break;
    case PH_NNZ:
        st->nnz = (long long)S[1];
        break;
    }
}

}  // namespace

struct lsq_spgl1_state {
    DevBuf vec;       // x, x trial, x best, g, g new, v / dx, prefix sums (N doubles each), keys and sorted keys (N u64 each), sort temp
    DevBuf res;       // r and r trial (n d doubles each)
    DevBuf small;     // partial sums, tile sums and prefixes, the scalar state
    DevBuf rows;      // the rows sorted by code
    SpgState *host = nullptr;      // pinned mirror of the state
};

void lsq_spgl1_free(lsq_spgl1_state *st) {
    if (!st) return;
    st->vec.release();
    st->res.release();
    st->small.release();
    st->rows.release();
    if (st->host) (void)hipHostFree(st->host);
    delete st;
}

int lsq_spgl1_update_codebooks(hipStream_t s, lsq_spgl1_state **pst, const float *dX, const uint8_t *dcodes, int d, int64_t n, int m, double tau,
                               const float *dK0, int64_t S, double opt_tol, int64_t max_iter, float *dK, lsq_spgl1_info *info) {
    const int cols = m * LSQ_H;
    const int64_t N = (int64_t)cols * d, nd = n * (int64_t)d;
    if (N >= ((int64_t)1 << 31) || n * (int64_t)m >= ((int64_t)1 << 31)) {
        lsq_set_error("lsq_update_codebooks_spgl1: d m h = %lld or n m = %lld exceeds 2^31 - 1", (long long)N, (long long)(n * m));
        return LSQ_EINVAL;
    }
    if (!*pst) {
        *pst = new (std::nothrow) lsq_spgl1_state();
        if (!*pst) { lsq_set_error("lsq_update_codebooks_spgl1: out of host memory"); return LSQ_ENOMEM; }
    }
    lsq_spgl1_state *st = *pst;
    if (!st->host) LSQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&st->host), sizeof(SpgState), hipHostMallocDefault));
    const int64_t ntiles = (N + EB - 1) / EB, nbN = std::min<int64_t>(ntiles, MAXB), nbR = std::min<int64_t>((nd + EB - 1) / EB, MAXB);
    const int64_t gy = (d + GT - 1) / GT;

    // buffers: vec = x, x trial, x best, g, g new, v / dx, prefix sums | keys, sorted keys | sort temp;  small = partials | tiles | state
    size_t sort_bytes = 0;
    LSQ_HIP(hipcub::DeviceRadixSort::SortKeysDescending(nullptr, sort_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)N, 0, 63, s));
    const size_t vN = (size_t)N * 8, off_tmp = (9 * vN + 255) & ~(size_t)255;
    LSQ_TRY(st->vec.ensure(off_tmp + sort_bytes));
    LSQ_TRY(st->res.ensure(2 * (size_t)nd * 8));
    const size_t off_tiles = (size_t)NSLOT * MAXB * 8, off_state = (off_tiles + 2 * (size_t)ntiles * 8 + 255) & ~(size_t)255;
    LSQ_TRY(st->small.ensure(off_state + sizeof(SpgState)));
    char *vb = st->vec.as<char>();
    double *x = reinterpret_cast<double *>(vb), *xn = reinterpret_cast<double *>(vb + vN), *xbest = reinterpret_cast<double *>(vb + 2 * vN);
    double *g = reinterpret_cast<double *>(vb + 3 * vN), *gn = reinterpret_cast<double *>(vb + 4 * vN);
    double *v = reinterpret_cast<double *>(vb + 5 * vN), *csum = reinterpret_cast<double *>(vb + 6 * vN);
    uint64_t *keys = reinterpret_cast<uint64_t *>(vb + 7 * vN), *sorted = reinterpret_cast<uint64_t *>(vb + 8 * vN);
    void *sort_tmp = vb + off_tmp;
    double *r = st->res.as<double>(), *rn = st->res.as<double>() + nd;
    double *part = st->small.as<double>();
    double *tilesum = reinterpret_cast<double *>(st->small.as<char>() + off_tiles), *tilepre = tilesum + ntiles;
    SpgState *dst = reinterpret_cast<SpgState *>(st->small.as<char>() + off_state);

    const uint64_t *rsorted = nullptr;
    const int64_t *seg = nullptr;
    LSQ_TRY(lsq_sort_rows_by_code(s, st->rows, dcodes, n, m, &rsorted, &seg));

    const dim3 gN((unsigned)nbN), gT((unsigned)ntiles), gR((unsigned)nbR), gG((unsigned)cols, (unsigned)gy), g256((unsigned)((N + 255) / 256));
    const int bA = (int)nbN, bR = (int)nbR;
    size_t sb = sort_bytes;

    auto ctl = [&](int phase, int nbA) {
        hipLaunchKernelGGL(spg_ctl, dim3(1), dim3(256), 0, s, dst, part, nbA, bR, tilesum, tilepre, ntiles, phase);
    };
    auto project = [&](int vmode, const float *k0) -> int {        // v = K_init | x - alpha g; the projection's theta (or copy / zero); apply follows
        hipLaunchKernelGGL(spg_vkeys, gN, dim3(256), 0, s, x, g, k0, v, keys, N, dst, vmode, part);
        LSQ_HIP(hipcub::DeviceRadixSort::SortKeysDescending(sort_tmp, sb, keys, sorted, (int)N, 0, 63, s));
        hipLaunchKernelGGL(spg_tile_sums, gT, dim3(256), 0, s, sorted, N, tilesum);
        ctl(PH_THETA, bA);
        hipLaunchKernelGGL(spg_scan_find, gT, dim3(256), 0, s, sorted, N, tilepre, csum, dst);
        return LSQ_OK;
    };
    auto gradient = [&](const double *rv, double *gout) -> int {
        LSQ_HIP(hipMemsetAsync(&dst->gmax_bits, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(spg_gradient, gG, dim3(GT), 0, s, rv, rsorted, seg, d, gout, dst);
        return LSQ_OK;
    };
    auto curvy_trial = [&]() -> int {                                // x trial = P(x - alpha g), its residual, the decision
        LSQ_TRY(project(V_XG, nullptr));
        hipLaunchKernelGGL(spg_apply, gN, dim3(256), 0, s, v, xn, x, g, csum, N, dst, (int)A_CURVY, part);
        hipLaunchKernelGGL(spg_residual, gR, dim3(256), 0, s, dX, dcodes, xn, rn, nd, d, m, part);
        ctl(PH_CURVY, bA);
        return LSQ_OK;
    };
    auto read_ctl = [&]() -> int {
        LSQ_HIP(hipMemcpyAsync(st->host->ctl, dst->ctl, sizeof(dst->ctl), hipMemcpyDeviceToHost, s));
        LSQ_HIP(hipStreamSynchronize(s));
        return LSQ_OK;
    };

    // start: x = P(K_init), r, g, f; the first step from ||P(x - g) - x||_inf; the gap test and the first trial
    hipLaunchKernelGGL(spg_setup, dim3(1), dim3(1), 0, s, dst, tau, opt_tol, sqrt((double)N));
    LSQ_TRY(project(V_LOAD, dK0));
    hipLaunchKernelGGL(spg_apply, gN, dim3(256), 0, s, v, x, x, g, csum, N, dst, (int)A_X, part);
    hipLaunchKernelGGL(spg_residual, gR, dim3(256), 0, s, dX, dcodes, x, r, nd, d, m, part);
    LSQ_TRY(gradient(r, g));
    ctl(PH_INIT, bA);
    hipLaunchKernelGGL(spg_copy_best, g256, dim3(256), 0, s, x, xbest, N, dst);
    LSQ_TRY(project(V_XG, nullptr));
    hipLaunchKernelGGL(spg_apply, gN, dim3(256), 0, s, v, v, x, g, csum, N, dst, (int)A_DX, part);
    ctl(PH_GSTEP, bA);
    if (max_iter > 0) LSQ_TRY(curvy_trial());
    LSQ_TRY(read_ctl());

    int status = LSQ_SPGL1_ITERATIONS;
    int64_t it = 0, trials = 0;
    for (;;) {
        const int stop = st->host->ctl[1];
        if (stop == STOP_OPTIMAL) { status = LSQ_SPGL1_OPTIMAL; break; }
        if (stop == STOP_LINE_ERROR) { status = LSQ_SPGL1_LINE_ERROR; break; }
        if (it >= max_iter) { status = LSQ_SPGL1_ITERATIONS; break; }
        ++it;
        ++trials;
        int result = st->host->ctl[0];
        while (result == RES_RETRY) {                                // spgLineCurvy's halvings
            LSQ_TRY(curvy_trial());
            LSQ_TRY(read_ctl());
            ++trials;
            result = st->host->ctl[0];
        }
        if (result == RES_FAIL) {                                    // spgLine along the feasible direction
            LSQ_TRY(project(V_XG, nullptr));
            hipLaunchKernelGGL(spg_apply, gN, dim3(256), 0, s, v, v, x, g, csum, N, dst, (int)A_DX, part);
            ctl(PH_FEAS_BEGIN, bA);
            do {
                hipLaunchKernelGGL(spg_feas_x, g256, dim3(256), 0, s, x, v, xn, N, dst);
                hipLaunchKernelGGL(spg_residual, gR, dim3(256), 0, s, dX, dcodes, xn, rn, nd, d, m, part);
                ctl(PH_FEAS, bA);
                LSQ_TRY(read_ctl());
                ++trials;
                result = st->host->ctl[0];
            } while (result == RES_RETRY);
        }
        if (result == RES_ACCEPT) {
            std::swap(x, xn);
            std::swap(r, rn);
            LSQ_TRY(gradient(r, gn));
            hipLaunchKernelGGL(spg_bb, gN, dim3(256), 0, s, x, xn, gn, g, N, part);      // xn holds the previous x now
            std::swap(g, gn);
            ctl(PH_BB, bA);
        } else {
            ctl(PH_REVERT, bA);
        }
        hipLaunchKernelGGL(spg_copy_best, g256, dim3(256), 0, s, x, xbest, N, dst);
        if (it < max_iter) LSQ_TRY(curvy_trial());                   // the next iteration's first trial, read together with this gap test
        LSQ_TRY(read_ctl());
    }
    if (status != LSQ_SPGL1_OPTIMAL && st->host->ctl[2]) {          // not certified and worse than the best iterate seen: return the best one
        x = xbest;
        hipLaunchKernelGGL(spg_residual, gR, dim3(256), 0, s, dX, dcodes, x, r, nd, d, m, part);
        LSQ_TRY(gradient(r, g));
        ctl(PH_RECERT, bA);
    }
    hipLaunchKernelGGL(spg_finish, gN, dim3(256), 0, s, x, dK, N, 1, part);
    ctl(PH_FINAL, bA);
    if (S >= 0 && S < N) {                                           // keep the S largest |K|
        hipLaunchKernelGGL(spg_tkeys, g256, dim3(256), 0, s, dK, N, keys);
        LSQ_HIP(hipcub::DeviceRadixSort::SortKeysDescending(sort_tmp, sb, keys, sorted, (int)N, 0, 63, s));
        hipLaunchKernelGGL(spg_tzero, dim3((unsigned)((N - S + 255) / 256)), dim3(256), 0, s, sorted, S, N, dK);
        hipLaunchKernelGGL(spg_finish, gN, dim3(256), 0, s, x, dK, N, 0, part);
        ctl(PH_NNZ, bA);
    }
    LSQ_HIP(hipGetLastError());
    LSQ_HIP(hipMemcpyAsync(st->host, dst, sizeof(SpgState), hipMemcpyDeviceToHost, s));
    LSQ_HIP(hipStreamSynchronize(s));
    if (info) {
        const SpgState &h = *st->host;
        info->status = status;
        info->iterations = it;
        info->line_search_trials = trials;
        info->f = h.f;
        info->rel_gap = h.rel_gap;
        info->l1 = h.l1;
        info->tau = tau;
        info->nnz_before_threshold = h.nnz_before;
        info->nnz = h.nnz;
    }
    return LSQ_OK;
}
