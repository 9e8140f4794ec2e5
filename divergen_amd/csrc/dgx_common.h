// Shared device helpers for libdgx (gfx950 only: wave64, MFMA 16x16x32 bf16).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/divergen_hip.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;  // 8 bf16 in 4 VGPRs (MFMA A/B fragment)
typedef __attribute__((ext_vector_type(4))) float f32x4;   // MFMA 16x16 C/D fragment
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;

__device__ __forceinline__ float bf2f(uint16_t v) { return __uint_as_float(((uint32_t)v) << 16); }

// fp32 -> bf16, round-to-nearest-even (NaN stays a quiet NaN): gfx950 has it in hardware (v_cvt_pk_bf16_f32)
typedef __bf16 dgx_bf2_t __attribute__((ext_vector_type(2)));
typedef float dgx_f2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
    const dgx_f2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, dgx_bf2_t));
}
__device__ __forceinline__ uint16_t f2bf(float f) { return (uint16_t)pack_bf2(f, 0.f); }

// ---- rows of fp32 / bf16 (uint16_t) storage as fp32: 4 elements (a quad) or 8 (a 16-byte bf16 chunk) per lane ----
// a quad as loaded (kept packed in registers: 2 registers for bf16, 4 for fp32) and its fp32 expansion
template <typename T> struct Raw4;
template <> struct Raw4<float> {
    typedef float4 type;
    static __device__ __forceinline__ float4 ld(const float* row, int i) { return reinterpret_cast<const float4*>(row)[i]; }
    static __device__ __forceinline__ float4 f(float4 r) { return r; }
    static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <> struct Raw4<uint16_t> {
    typedef uint2 type;
    static __device__ __forceinline__ uint2 ld(const uint16_t* row, int i) { return reinterpret_cast<const uint2*>(row)[i]; }
    static __device__ __forceinline__ float4 f(uint2 d) {
        return make_float4(__uint_as_float(d.x << 16), __uint_as_float(d.x & 0xffff0000u), __uint_as_float(d.y << 16), __uint_as_float(d.y & 0xffff0000u));
    }
    static __device__ __forceinline__ uint2 zero() { return make_uint2(0u, 0u); }
};
// quad i of a row
template <typename T> __device__ __forceinline__ float4 ld4(const T* row, int i) { return Raw4<T>::f(Raw4<T>::ld(row, i)); }
__device__ __forceinline__ void st4(float* row, int i, float4 v) { reinterpret_cast<float4*>(row)[i] = v; }
__device__ __forceinline__ void st4(uint16_t* row, int i, float4 v) {
    reinterpret_cast<uint2*>(row)[i] = make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w));
}
// v as it reads back after a store in type T
template <typename T> __device__ __forceinline__ float4 rnd4(float4 v) {
    if constexpr (sizeof(T) == 4) return v;
    else return Raw4<uint16_t>::f(make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)));
}

// 8 bf16 in a 16-byte register quad V (u32x4, or HIP's uint4 where a kernel's pointers are typed so) <-> 8 floats
template <class V> __device__ __forceinline__ void unpack8(const V r, float (&v)[8]) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}
template <class V = u32x4> __device__ __forceinline__ V pack8(const float (&v)[8]) {
    return V{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
}
// the 8 elements at p (16-byte aligned)
__device__ __forceinline__ void ld8(const uint16_t* p, float (&v)[8]) { unpack8(*reinterpret_cast<const uint4*>(p), v); }
__device__ __forceinline__ void ld8(const float* p, float (&v)[8]) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st8(uint16_t* p, const float (&v)[8]) { *reinterpret_cast<uint4*>(p) = pack8<uint4>(v); }
__device__ __forceinline__ void st8(float* p, const float (&v)[8]) {
    reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// sum over the 64 lanes, in every lane: xor butterfly 32, 16, .., 1 (the order is part of every result that uses it)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// D(16x16) += A(16x32) * B(32x16); lane l: a = A[l&15][slot (l>>4, 0..7)], b = B[slot][l&15],
// d[r] = D[(l>>4)*4 + r][l&15].  A and B use the same (lane-group, i) -> k slot map.
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// LDS transpose read (gfx950 ds_read_b64_tr_b16).  Measured semantics (tools/probes/tr_probe.hip): within
// each 16-lane group, lane p supplies the address of an 8-byte chunk (4 bf16); result lane i, element j is
// element (i & 3) of the chunk supplied by lane 4*j + (i >> 2).  With lane p pointing at row (p >> 2),
// columns 4*(p & 3).. of a row-major [4][16] block, lane i receives column i of that block (rows 0..3):
// exactly the k-contiguous MFMA operand layout, from an image stored the way global memory has it.
// The compiler builtin is used (not inline asm) so that constant offsets fold into the instruction's
// offset field and the waits are placed by the scheduler.
typedef short s16x4 __attribute__((ext_vector_type(4)));
#define DGX_LDS __attribute__((address_space(3)))
// LDS-qualified copy of a shared-memory pointer, opaque to the optimiser: everything derived from it is
// "base register + constant", which the backend folds into the DS instruction's 16-bit offset field instead
// of materialising (and spilling) one address register per unrolled access.
template <typename T>
__device__ __forceinline__ DGX_LDS T* lds_opaque(T* p) {
    DGX_LDS T* q = (DGX_LDS T*)p;
    asm volatile("" : "+v"(q));
    return q;
}
__device__ __forceinline__ s16x4 ds_read_tr16(DGX_LDS const uint16_t* lds_ptr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((DGX_LDS s16x4*)lds_ptr);
}
// This lane's chunk pointer inside a row-major bf16 LDS image (row stride `rs` elements) for a transpose
// read of the 4-row block starting at `row0`, columns c0 .. c0+15; p = lane & 15.
__device__ __forceinline__ DGX_LDS const uint16_t* tr_lane_ptr(const uint16_t* img, int rs, int row0, int c0, int p) {
    return lds_opaque(img + (row0 + (p >> 2)) * rs + c0 + 4 * (p & 3));
}
// MFMA operand (8 k-slots) = two 4-row blocks at element offsets offA / offB from the lane pointer.
__device__ __forceinline__ bf16x8 tr_frag(DGX_LDS const uint16_t* lane_ptr, int offA, int offB) {
    const s16x4 a = ds_read_tr16(lane_ptr + offA), b = ds_read_tr16(lane_ptr + offB);
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

#define DGX_LAUNCH_CHECK()                                 \
    do {                                                   \
        hipError_t e__ = hipGetLastError();                \
        if (e__ != hipSuccess) return -(int)e__ - 1000;    \
    } while (0)

static inline int dgx_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// Launch accounting (prof.hip): no-op unless dgx_prof_enable(1) was called.
struct DgxProfScope {
    DgxProfScope(int family, void* stream, double flops, double bytes);
    ~DgxProfScope();
    void *a, *b, *st;
    int fam;
};
