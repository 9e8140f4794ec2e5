// Rows of a row-major (R, ld) f32 | bf16 matrix in 16-byte chunks: the access split of the image-label loss kernels
// (image_label.hip, wsddn_loss.hip).
#pragma once
#include "dgx_common.h"

namespace {
template <typename T> struct Chunk;
template <> struct Chunk<float> { static constexpr int N = 4; };
template <> struct Chunk<uint16_t> { static constexpr int N = 8; };

template <typename T> __device__ __forceinline__ float il_ld1(const T* p);
template <> __device__ __forceinline__ float il_ld1<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float il_ld1<uint16_t>(const uint16_t* p) { return bf2f(*p); }

// N = 16 bytes of row elements starting at column c (a multiple of N).  vec: row base and leading dimension are 16-byte
// aligned, so one 16-byte access that stays inside the row's `lim` columns; otherwise element by element, columns >= lim skipped.
template <typename T> __device__ __forceinline__ void load_chunk(const T* row, int c, bool vec, int lim, float* f);
template <> __device__ __forceinline__ void load_chunk<float>(const float* row, int c, bool vec, int lim, float* f) {
    if (vec) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
        f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = (c + k < lim) ? row[c + k] : 0.0f;
    }
}
template <> __device__ __forceinline__ void load_chunk<uint16_t>(const uint16_t* row, int c, bool vec, int lim, float* f) {
    if (vec) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(row + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f[2 * k] = __uint_as_float(v[k] << 16);
            f[2 * k + 1] = __uint_as_float(v[k] & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = (c + k < lim) ? bf2f(row[c + k]) : 0.0f;
    }
}
template <typename T> __device__ __forceinline__ void store_chunk(T* row, int c, bool vec, int lim, const float* f);
template <> __device__ __forceinline__ void store_chunk<float>(float* row, int c, bool vec, int lim, const float* f) {
    if (vec) {
        const f32x4 v = {f[0], f[1], f[2], f[3]};
        *reinterpret_cast<f32x4*>(row + c) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c + k < lim) row[c + k] = f[k];
    }
}
template <> __device__ __forceinline__ void store_chunk<uint16_t>(uint16_t* row, int c, bool vec, int lim, const float* f) {
    if (vec) {
        const u32x4 v = {pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7])};
        *reinterpret_cast<u32x4*>(row + c) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (c + k < lim) row[c + k] = f2bf(f[k]);
    }
}
}  // namespace
