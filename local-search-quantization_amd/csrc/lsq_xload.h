// lsq_xload.h -- row loaders of the data matrix X for the three kernels that read it on the encode path (chain_gemm_kernel's A operand,
// unary_shift_kernel, cost4_body).  The element type of X is a template parameter of those kernels: float (the default: one 16-byte load per
// four components, the code that has always run) or uint8_t (TEXMEX .bvecs base sets: one 4-byte load per four components, widened in registers).
//
// uint8 -> f32 is exact, so a kernel that widens after the load computes, bit for bit, what the f32 instantiation computes on the widened matrix:
// everything behind the load (the k-ascending MFMA chain, the DPP row sums, cost_one()'s tree) is shared source.
//
// Alignment rule of the 8-bit loader: four components travel as ONE dword load when d % 4 == 0 (every row then starts on the base's alignment) and the
// base pointer is 4-byte aligned (lsq_x_vec_ok).  In every other case -- odd d, or a base at any byte offset -- the same four components travel as
// four byte loads (global_load_ubyte zero-extends: the widening is one convert either way).  The f32 rule (16-byte alignment) does not apply: a
// .bvecs matrix, or a view into one, is as aligned as its first byte.
//
// A loaded-but-not-yet-widened quad stays PACKED (one VGPR) until it is consumed: the GEMM's register double buffer and the cost kernel's "x one
// step ahead" hold a quarter of the registers the f32 instantiation holds, and the convert sits next to the arithmetic, not next to the load (a
// convert right behind the load would put the wait for it in front of the work the load is meant to hide under).
//
// One more reader of X keeps a loader of its own: the exact re-rank (lsq_rerank.hip, rr_load16) fetches 16-byte PIECES of a 128-byte line, not quads,
// and so adds a 16-byte road to the dword / byte rule above.  It shares lsq_widen4 and the packed-until-consumed rule; a change to the alignment
// rule here has to be made there too.
//
// Half-precision rows (the BASE rows of a resident index only: lsq_rerank.hip, lsq_knn.hip, lsq_half.hip) follow the same rule.  lsq_f16 is
// IEEE binary16, lsq_bf16 the upper 16 bits of a binary32; widening either is exact -- subnormals included, nothing is flushed -- so an instantiation on
// them returns the bits of the f32 one on the widened matrix.  Two halves of one dword stay packed until consumed: lsq_widen2.
#pragma once

#include <stdint.h>

#include "lsq_half_check.h"

typedef float lsq_f32x4 __attribute__((ext_vector_type(4)));
typedef float lsq_f32x2 __attribute__((ext_vector_type(2)));

// the 2-byte element types: the stored bits, (T)0 and an exact (float) -- what a kernel templated on the row type asks of it.  The device converts with
// v_cvt_f32_f16 / a shift, the host with the integer rules of lsq_half_check.h: the same value either way
struct lsq_f16 {
    uint16_t b;
    lsq_f16() = default;
    __host__ __device__ explicit lsq_f16(int) : b(0) {}
    __host__ __device__ explicit operator float() const {
#if defined(__HIP_DEVICE_COMPILE__)
        return (float)__builtin_bit_cast(_Float16, b);
#else
        return lsq_widen_f16(b);
#endif
    }
};
struct lsq_bf16 {
    uint16_t b;
    lsq_bf16() = default;
    __host__ __device__ explicit lsq_bf16(int) : b(0) {}
    __host__ __device__ explicit operator float() const {
#if defined(__HIP_DEVICE_COMPILE__)
        return __uint_as_float((uint32_t)b << 16);
#else
        return lsq_widen_bf16(b);
#endif
    }
};

// two halves of one dword (component e in bits 16 e ..) -> two floats (exact).  bf16: a shift and a mask; f16: the two converts
template <typename T> __device__ inline lsq_f32x2 lsq_widen2(uint32_t w);
template <> __device__ inline lsq_f32x2 lsq_widen2<lsq_bf16>(uint32_t w) {
    lsq_f32x2 v;
    v.x = __uint_as_float(w << 16);
    v.y = __uint_as_float(w & 0xffff0000u);
    return v;
}
template <> __device__ inline lsq_f32x2 lsq_widen2<lsq_f16>(uint32_t w) {
    lsq_f32x2 v;
    v.x = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
    v.y = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
    return v;
}

// f32 -> half, round to nearest even (Identity N; the host's rule: lsq_narrow_f16 / lsq_narrow_bf16).  f16: (_Float16)x is v_cvt_f16_f32, which rounds to
// nearest even, keeps subnormals and overflows to inf -- NOT the packed convert that rounds toward zero.  bf16: the integer rule in plain C++, whose NaN and
// subnormal behaviour is the rule's by construction
template <typename T> __device__ inline uint32_t lsq_narrow1(float x);
template <> __device__ inline uint32_t lsq_narrow1<lsq_f16>(float x) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x); }
template <> __device__ inline uint32_t lsq_narrow1<lsq_bf16>(float x) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// host: may rows of X (row stride ld elements, ld % 4 == 0 required by the caller) be fetched four components per load?
static inline bool lsq_x_vec_ok(const float *X) { return ((uintptr_t)X & 15) == 0; }
static inline bool lsq_x_vec_ok(const uint8_t *X) { return ((uintptr_t)X & 3) == 0; }

// four 8-bit components of one dword -> four floats (exact).  Plain C++: the back end selects v_cvt_f32_ubyte0 .. 3 for a byte field converted to float.
__device__ inline lsq_f32x4 lsq_widen4(uint32_t w) {
    lsq_f32x4 v;
    v.x = (float)(w & 0xffu);
    v.y = (float)((w >> 8) & 0xffu);
    v.z = (float)((w >> 16) & 0xffu);
    v.w = (float)(w >> 24);
    return v;
}

// p[0 .. 3] as one packed dword (component e in byte e); p 4-byte aligned
__device__ inline uint32_t lsq_ld4_packed(const uint8_t *p) { return *reinterpret_cast<const uint32_t *>(p); }

// p[0 .. 3] widened; float: p 16-byte aligned, uint8_t: p 4-byte aligned
__device__ inline lsq_f32x4 lsq_ld4(const float *p) { return *reinterpret_cast<const lsq_f32x4 *>(p); }
__device__ inline lsq_f32x4 lsq_ld4(const uint8_t *p) { return lsq_widen4(lsq_ld4_packed(p)); }
// the same, streaming (the row is read once)
__device__ inline lsq_f32x4 lsq_ld4_nt(const float *p) { return __builtin_nontemporal_load(reinterpret_cast<const lsq_f32x4 *>(p)); }
__device__ inline lsq_f32x4 lsq_ld4_nt(const uint8_t *p) { return lsq_widen4(__builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p))); }
