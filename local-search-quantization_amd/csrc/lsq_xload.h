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
#pragma once

#include <stdint.h>

typedef float lsq_f32x4 __attribute__((ext_vector_type(4)));

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
