// lsq_beam.hip -- the BEAM-SEARCH encoder over the full pair tables (the classical encoder of additive quantisation and of residual quantisers), gfx950.
// The reference has no counterpart: its encodes start from randinit (src/encodings/encode_icm.jl:55-70) and its one exact DP is the chain's
// (src/encodings/encode_chain.jl:2-89).  Contract (include/lsq_mi355x.h, section "beam-search encoder"; restated by tests/beam_check.py) per vector i,
// visiting order o_0 .. o_{m-1}, beam width L:
//     stage 0      v(0, a) = U[o_0][i][a]
//     stage t >= 1 for every live beam p in rank order (score S_p, codes b^p):   s = U[o_t][i][.];   s[a] = s[a] + T[o_t][o_r][b^p_{o_r}][a]  for r = 0 .. t-1
//                  (plain f32 adds in stage order, no FMA);   v(p, a) = S_p + s[a]
//     selection    the min(L, L_t 256) smallest (v, p, a) in lexicographic order become the next beams in that order: a child's score is v, its codes the
//                  parent's plus b_{o_t} = a
//     output       the codes (and optionally the score) of the rank-0 beam after stage m - 1.
// It reads what viterbi_kernel reads: the row-major f32 unary planes U[(j n + i) 256 + a] of the path's own chain GEMM and the pair tables of the table
// GEMM, T[((j m + k) 256 + b) 256 + a] = 2 <c_kb, c_ja>.  Every table index is a code this kernel produced (0 .. 255 by construction: a = position & 255)
// or an entry of `order`, which the host validates as a permutation before anything is launched.
//
// The shape of the work (the DIRECT road: one wave per vector, a lane owns four candidates, a table row is one 16-byte load per lane = 1 KiB per wave,
// gathered from L2): stage t reads L_t t rows, so a vector reads L m (m - 1) / 2 KiB of table rows in all (m = 8, L = 16: 448 KiB).
//   beam_greedy_kernel   L = 1: no selection state at all -- the first minimum of the wave's 256 values per stage (lane_first_min + wave_first_min of
//                        lsq_init.hip), the codes in two wave-uniform 64-bit words.  Four vectors per 256-thread block.
//   beam_kernel<LMAX>    1 < L <= LMAX (2, 4, 8, 16, 32): one 64-thread block (one wave) per vector.  All L parents advance together, one pair table at a
//                        time: LMAX row loads in flight, the sums in registers (arrays indexed by fully unrolled loops only), every parent's adds in stage
//                        order.  The stage's L_t x 256 candidates go to LDS as order-preserving 32-bit keys
//                        (lsq_adc_key: a < b <=> key(a) < key(b); -0 is stored as +0 so that equal floats have equal keys; NaN is the largest key).  The
//                        position p 256 + a of a key IS the tie rule: the selection extracts the minimum of the 64-bit words (key << 32 | position) L
//                        times (two DPP reductions of 32-bit words: the key, then the position among the lanes that hold it).  Lane w owns the positions q 64 + ((w + q) & 63), q = 0 .. 4 L_t - 1 (a skewed column: the 64 lanes' reads of one q and
//                        one lane's column over q both touch 64 different banks) and keeps the minimum of its column in registers; an extraction is one
//                        wave reduction of those minima, the winner's slot is overwritten with the largest key and its column's minimum is found again
//                        by the whole wave (lane l reads q = l and q = l + 64) with a second reduction.  No per-thread arrays.  The last stage extracts
//                        one beam only.  Beams (score, 16 code bytes) live in LDS, double-buffered.
//                        LDS: 1 KiB of keys per beam + 40 bytes per beam = 34 048 bytes at L = 32 (4 waves per CU), 17 024 at L = 16 (9 per CU).
#include "lsq_internal.h"
#include "lsq_wave.h"

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

struct BeamOrder { uint8_t o[LSQ_MAX_M]; };               // kernel argument: the visiting order

constexpr uint32_t BEAM_TAKEN = 0xffffffffu;              // the largest key (NaN's): an extracted slot

__device__ inline uint32_t beam_key(float v) {
    if (v == 0.0f) v = 0.0f;                                // -0 -> +0: floats that compare equal share a key
    return lsq_adc_key(v);
}

// lexicographic (value, index) minimum over the wave == the strict-'<' scan from index 0 (lsq_init.hip)
__device__ inline void beam_first_min(float &v, int &a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oa = __shfl_xor(a, o, 64);
        if (ov < v || (ov == v && oa < a)) { v = ov; a = oa; }
    }
}

// minimum of a 32-bit word over the wave by DPP (the steps of lsq_wave.h's wave_min), wave-uniform result
template <int CTRL, int ROW_MASK>
__device__ inline uint32_t dpp_self_u32(uint32_t v) {        // disabled lanes keep their own value
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ inline uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ inline uint32_t wave_min_u32(uint32_t v) {
    v = umin32(v, dpp_self_u32<DPP_XOR1, 0xf>(v));
    v = umin32(v, dpp_self_u32<DPP_XOR2, 0xf>(v));
    v = umin32(v, dpp_self_u32<DPP_HALF_MIRROR, 0xf>(v));
    v = umin32(v, dpp_self_u32<DPP_MIRROR, 0xf>(v));
    v = umin32(v, dpp_self_u32<DPP_BCAST15, 0xa>(v));
    v = umin32(v, dpp_self_u32<DPP_BCAST31, 0xc>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// lexicographic minimum of the lanes' (key, position) pairs, wave-uniform: the smallest key, then the smallest position among the lanes that hold it
__device__ inline void wave_min_key_pos(uint32_t key, uint32_t pos, uint32_t &kmin, uint32_t &pmin) {
    kmin = wave_min_u32(key);
    pmin = wave_min_u32(key == kmin ? pos : 0xffffffffu);
}

__device__ inline f32x4 beam_row(const float *T, int64_t row, int lane) {
    return *reinterpret_cast<const f32x4 *>(T + row * LSQ_H + 4 * lane);
}

template <bool I16>
__device__ inline void beam_store_code(void *codes, int64_t at, int code) {
    if (I16) static_cast<int16_t *>(codes)[at] = (int16_t)(code + 1);        // the boundary's 1-based type
    else static_cast<uint8_t *>(codes)[at] = (uint8_t)code;
}

// L = 1: a wave per vector, nothing but the first minimum per stage
template <bool I16>
__global__ __launch_bounds__(256) void beam_greedy_kernel(const float *__restrict__ U, const float *__restrict__ T, int64_t n, int m, BeamOrder ord,
                                                          void *__restrict__ codes, float *__restrict__ score) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
        uint64_t lo = 0, hi = 0;                              // code of codebook k: byte k of (lo, hi), wave-uniform
        float S = 0.0f;
        for (int t = 0; t < m; ++t) {
            const int j = ord.o[t];
            f32x4 s = beam_row(U, (int64_t)j * n + i, lane);
            const int64_t Tj = (int64_t)j * m * LSQ_H;
#pragma unroll 4
            for (int r = 0; r < t; ++r) {
                const int k = ord.o[r];
                const int b = (int)(((k < 8 ? lo : hi) >> (8 * (k & 7))) & 255u);
                const f32x4 row = beam_row(T, Tj + (int64_t)k * LSQ_H + b, lane);
                s.x = s.x + row.x; s.y = s.y + row.y; s.z = s.z + row.z; s.w = s.w + row.w;
            }
            if (t > 0) { s.x = S + s.x; s.y = S + s.y; s.z = S + s.z; s.w = S + s.w; }
            float v = s.x; int a = 4 * lane;
            if (s.y < v) { v = s.y; a = 4 * lane + 1; }
            if (s.z < v) { v = s.z; a = 4 * lane + 2; }
            if (s.w < v) { v = s.w; a = 4 * lane + 3; }
            beam_first_min(v, a);
            a = __builtin_amdgcn_readfirstlane(a) & 255;
            S = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
            if (j < 8) lo |= (uint64_t)a << (8 * j); else hi |= (uint64_t)a << (8 * (j - 8));
        }
        if (lane < m) beam_store_code<I16>(codes, i * m + lane, (int)(((lane < 8 ? lo : hi) >> (8 * (lane & 7))) & 255u));
        if (lane == 0 && score) score[i] = S;
    }
}

__host__ __device__ constexpr int beam_lds_bytes(int L) { return L * LSQ_H * 4 + 2 * L * 4 + 2 * L * LSQ_MAX_M; }

// 2 <= L <= LMAX <= 32: a wave (= a block) per vector
template <int LMAX, bool I16>
__global__ __launch_bounds__(64) void beam_kernel(const float *__restrict__ U, const float *__restrict__ T, int64_t n, int m, int L, BeamOrder ord,
                                                  void *__restrict__ codes, float *__restrict__ score) {
    extern __shared__ uint32_t beam_lds[];
    uint32_t *keyS = beam_lds;                                               // [L][256] candidate keys of the stage
    float *scoreS = reinterpret_cast<float *>(keyS + L * LSQ_H);            // [2][L]
    uint8_t *codeS = reinterpret_cast<uint8_t *>(scoreS + 2 * L);           // [2][L][16]
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        int cur = 0, Lt = 1;
        for (int t = 0; t < m; ++t) {
            const int j = ord.o[t];
            const f32x4 u = beam_row(U, (int64_t)j * n + i, lane);
            const int64_t Tj = (int64_t)j * m * LSQ_H;
            if (t == 0) {                                                     // stage 0: the unaries themselves, one parent
                reinterpret_cast<u32x4_t *>(keyS)[lane] = (u32x4_t){beam_key(u.x), beam_key(u.y), beam_key(u.z), beam_key(u.w)};
            } else {                                                          // L_t = L parents: all of them advance together, one table at a time
                f32x4 s[LMAX];                                                // (indexed by unrolled loops only: registers)
#pragma unroll
                for (int p = 0; p < LMAX; ++p) s[p] = u;
                for (int r = 0; r < t; ++r) {                                 // stage order: a parent's adds are never reordered
                    const int k = ord.o[r];
                    const float *Tk = T + (Tj + (int64_t)k * LSQ_H) * LSQ_H + 4 * lane;
                    f32x4 row[LMAX];                                          // LMAX rows of 1 KiB in flight per wave
#pragma unroll
                    for (int p = 0; p < LMAX; ++p) {
                        const int pp = p < L ? p : L - 1;                     // beyond L: the last parent again, branch-free
                        const int b = __builtin_amdgcn_readfirstlane((int)codeS[(cur * L + pp) * LSQ_MAX_M + k]);
                        row[p] = *reinterpret_cast<const f32x4 *>(Tk + b * LSQ_H);
                    }
#pragma unroll
                    for (int p = 0; p < LMAX; ++p) {
                        s[p].x = s[p].x + row[p].x; s[p].y = s[p].y + row[p].y; s[p].z = s[p].z + row[p].z; s[p].w = s[p].w + row[p].w;
                    }
                }
#pragma unroll
                for (int p = 0; p < LMAX; ++p) {
                    const int pp = p < L ? p : L - 1;
                    const float S = scoreS[cur * L + pp];
                    reinterpret_cast<u32x4_t *>(keyS + pp * LSQ_H)[lane] =
                        (u32x4_t){beam_key(S + s[p].x), beam_key(S + s[p].y), beam_key(S + s[p].z), beam_key(S + s[p].w)};
                }
            }
            __syncthreads();
            // the minimum of the lane's skewed column; q ascending and strict '<': the smallest position among equal keys
            const int nq = 4 * Lt;
            uint32_t mk = keyS[lane], mpos = (uint32_t)lane;
            for (int q = 1; q < nq; ++q) {
                const uint32_t pos = (uint32_t)(q * 64 + ((lane + q) & 63));
                const uint32_t k = keyS[pos];
                if (k < mk) { mk = k; mpos = pos; }
            }
            const int Ln = t == m - 1 ? 1 : L;                               // beams leaving the stage (L <= 256 L_t always)
            const int nxt = cur ^ 1;
            for (int rank = 0; rank < Ln; ++rank) {
                uint32_t key, pos;                                           // pos < 256 L_t: every lane's column starts with a real slot
                wave_min_key_pos(mk, mpos, key, pos);
                const int p = (int)(pos >> 8), a = (int)(pos & 255u);
                if (lane < m) codeS[(nxt * L + rank) * LSQ_MAX_M + lane] = lane == j ? (uint8_t)a : codeS[(cur * L + p) * LSQ_MAX_M + lane];
                if (lane == 0) scoreS[nxt * L + rank] = lsq_adc_unkey(key);
                if (rank + 1 < Ln) {
                    if (lane == 0) keyS[pos] = BEAM_TAKEN;
                    __syncthreads();
                    const int w = (int)((pos - (pos >> 6)) & 63u);             // the lane that owns the slot: its column is read again by the whole wave
                    uint32_t ck = BEAM_TAKEN, cpos = 0xffffffffu;
                    if (lane < nq) {
                        cpos = (uint32_t)(lane * 64 + ((w + lane) & 63));
                        ck = keyS[cpos];
                    }
                    if (lane + 64 < nq) {                                    // the later slot wins only with a smaller key
                        const uint32_t at = (uint32_t)((lane + 64) * 64 + ((w + lane) & 63));
                        const uint32_t k2 = keyS[at];
                        if (k2 < ck) { ck = k2; cpos = at; }
                    }
                    uint32_t nk, npos;
                    wave_min_key_pos(ck, cpos, nk, npos);
                    if (lane == w) { mk = nk; mpos = npos; }
                }
            }
            __syncthreads();
            cur = nxt; Lt = Ln;
        }
        if (lane < m) beam_store_code<I16>(codes, i * m + lane, codeS[cur * L * LSQ_MAX_M + lane]);
        if (lane == 0 && score) score[i] = scoreS[cur * L];
        __syncthreads();                                                     // the next vector's first stage writes the buffer just read
    }
}

}  // namespace

int lsq_launch_beam(hipStream_t s, const float *U, const float *T, int64_t n, int m, int L, const uint8_t *order, void *codes, int codes_i16, float *score) {
    if (n <= 0) return LSQ_OK;
    if (m < 1 || m > LSQ_MAX_M || L < 1 || L > 32) { lsq_set_error("lsq_launch_beam: needs 1 <= m <= 16 and 1 <= beam <= 32 (got m=%d beam=%d)", m, L); return LSQ_EINVAL; }
    BeamOrder ord;
    unsigned seen = 0;
    for (int t = 0; t < LSQ_MAX_M; ++t) ord.o[t] = 0;
    for (int t = 0; t < m; ++t) {
        if (order[t] >= m || (seen >> order[t] & 1u)) { lsq_set_error("lsq_launch_beam: the visiting order is not a permutation of 0 .. m-1"); return LSQ_EINVAL; }
        seen |= 1u << order[t];
        ord.o[t] = order[t];
    }
    if (L == 1) {
        const int64_t want = (n + 3) / 4;
        const dim3 grid((unsigned)(want < 256 * 16 ? want : 256 * 16)), block(256);
        if (codes_i16) hipLaunchKernelGGL(beam_greedy_kernel<true>, grid, block, 0, s, U, T, n, m, ord, codes, score);
        else hipLaunchKernelGGL(beam_greedy_kernel<false>, grid, block, 0, s, U, T, n, m, ord, codes, score);
    } else {
        const dim3 grid((unsigned)(n < 256 * 16 ? n : 256 * 16)), block(64);
        const int lds = beam_lds_bytes(L);                                   // <= 34 048 bytes: below the 64 KiB that need no opt-in
#define BEAM_LAUNCH(LMAX_)                                                                                                          \
        do {                                                                                                                        \
            if (codes_i16) hipLaunchKernelGGL((beam_kernel<LMAX_, true>), grid, block, lds, s, U, T, n, m, L, ord, codes, score);  \
            else hipLaunchKernelGGL((beam_kernel<LMAX_, false>), grid, block, lds, s, U, T, n, m, L, ord, codes, score);           \
        } while (0)
        if (L <= 2) BEAM_LAUNCH(2);                                          // the instantiation holds LMAX parents' sums in registers
        else if (L <= 4) BEAM_LAUNCH(4);
        else if (L <= 8) BEAM_LAUNCH(8);
        else if (L <= 16) BEAM_LAUNCH(16);
        else BEAM_LAUNCH(32);
#undef BEAM_LAUNCH
    }
    LSQ_HIP(hipGetLastError());
    return LSQ_OK;
}
