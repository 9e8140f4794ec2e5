// What the self copy-paste kernels (self_copy.hip: one paste step, and several sources folded first) and the background removal
// (remove_background.hip) share: 16 pixels per lane, the vector-or-byte row accesses, the per-object statistics (count, x_min, x_max,
// y_min, y_max) of a plane, the launch geometry on the host.
#pragma once
#include "dgx_common.h"

#define SC_MAX_M 99                                // selected objects per source image (the reference draws m < min(ns + 1, 100))
#define SCM_MAX_SRC DGX_SELF_COPY_MAX_SRC          // source images of one merge (INPUT.SCP_NUM_SRC with INPUT.SCP_MULTI_SRC)
constexpr int SCX = 16;                            // pixels per lane
constexpr int SC_MAX_OPG = 64;                     // destination objects per workgroup group (LDS statistics)

// 16 bytes of row y, columns x .. x + 15 of an (h, w) plane; zeros outside.  vec: w % 16 == 0 and a 16-byte aligned base, so a
// chunk that starts inside the row lies inside it.
__device__ __forceinline__ void sc_load16(const uint8_t* __restrict__ plane, int y, int x, int h, int w, bool vec, uint32_t (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0u;
    if (y >= h || x >= w) return;
    const uint8_t* p = plane + (int64_t)y * w + x;
    if (vec) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < SCX; ++q)
            if (x + q < w) v[q >> 2] |= (uint32_t)p[q] << (8 * (q & 3));
    }
}

__device__ __forceinline__ void sc_store16(uint8_t* __restrict__ plane, int y, int x, int W, bool vec, const uint32_t (&v)[4]) {
    uint8_t* p = plane + (int64_t)y * W + x;
    if (vec) {
        *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int q = 0; q < SCX; ++q)
            if (x + q < W) p[q] = (uint8_t)(v[q >> 2] >> (8 * (q & 3)));
    }
}

// per byte: 0x01 where the byte is non-zero
__device__ __forceinline__ uint32_t sc_nonzero(uint32_t w) {
    return ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) >> 7) & 0x01010101u;
}

// the statistics of an object nobody has touched yet: field f of (count, x_min, x_max, y_min, y_max)
__device__ __forceinline__ int32_t sc_stat_init(int f) { return f == 0 ? 0 : ((f == 1 || f == 3) ? 0x7fffffff : -1); }

// One lane's 16 pixels of one object (row y, columns x ..; inactive lanes pass v == 0) folded into the object's LDS record r[5]:
// reduced over the wave first, one LDS atomic set per wave that saw a pixel.  Every lane of the wave must call it.
__device__ __forceinline__ void sc_fold_stats(const uint32_t (&v)[4], int y, int x, int lane, int32_t* r) {
    uint32_t bits = 0;                             // bit q: pixel x + q is set
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t nz = sc_nonzero(v[q]);
        bits |= ((nz & 1u) | ((nz >> 7) & 2u) | ((nz >> 14) & 4u) | ((nz >> 21) & 8u)) << (4 * q);
    }
    int cnt = 0, x0 = 0x7fffffff, x1 = -1;
    if (bits) { cnt = __popc(bits); x0 = x + __ffs((int)bits) - 1; x1 = x + 31 - __clz((int)bits); }
    if (__any(cnt > 0)) {                          // wave-uniform
        int y0 = cnt ? y : 0x7fffffff, y1 = cnt ? y : -1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            cnt += __shfl_xor(cnt, d);
            x0 = min(x0, __shfl_xor(x0, d)); x1 = max(x1, __shfl_xor(x1, d));
            y0 = min(y0, __shfl_xor(y0, d)); y1 = max(y1, __shfl_xor(y1, d));
        }
        if (lane == 0) {
            atomicAdd(&r[0], cnt);
            atomicMin(&r[1], x0); atomicMax(&r[2], x1);
            atomicMin(&r[3], y0); atomicMax(&r[4], y1);
        }
    }
}

// the workgroup's LDS records of `n` objects -> their global records (one atomic set per workgroup and touched object)
__device__ __forceinline__ void sc_flush_stats(const int32_t* s, int n, int32_t* __restrict__ g) {
    for (int i = threadIdx.x; i < n * 5; i += blockDim.x) {
        const int f = i % 5;
        if (s[5 * (i / 5)] == 0) continue;
        if (f == 0) atomicAdd(g + i, s[i]);
        else if (f == 1 || f == 3) atomicMin(g + i, s[i]);
        else atomicMax(g + i, s[i]);
    }
}

// get_bboxes of an updated mask from its record (x_max + 1, y_max + 1; zeros when empty) into b; returns _copy_paste's verdict
// against the box the object had before: every |new - old| <= 10, or more than 300 pixels left.
__device__ __forceinline__ bool sc_resolve(const int32_t* s, const float* old, float (&b)[4]) {
    b[0] = b[1] = b[2] = b[3] = 0.0f;
    if (s[0] > 0) { b[0] = (float)s[1]; b[1] = (float)s[3]; b[2] = (float)(s[2] + 1); b[3] = (float)(s[4] + 1); }
    bool box_ok = true;
    for (int i = 0; i < 4; ++i) box_ok = box_ok && fabsf(b[i] - old[i]) <= 10.0f;
    return box_ok || s[0] > 300;
}

// ---- host side
static inline bool sc_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int64_t sc_pad4(int64_t n) { return (n + 3) & ~(int64_t)3; }
// workgroups of 256 lanes over n items, grid-stride beyond 2048
static inline int sc_blocks(int64_t n) { return (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048); }

// Launch geometry over nchunk 16-pixel chunks, one lane each: gx workgroups; a kernel that loops over planes splits them into `want`
// groups over grid.y so that small frames still fill the chip.
struct ScGrid {
    int gx, want;
    explicit ScGrid(int64_t nchunk) : gx(sc_blocks(nchunk)), want(gx >= 1024 ? 1 : (1024 + gx - 1) / gx) {}
    // n planes, at most cap per group (what the kernel's LDS holds): the grid, the planes per group in `per`.  n == 0: one empty group.
    dim3 split(int n, int cap, int& per) const {
        const int groups = want < n ? want : (n > 0 ? n : 1);
        per = n > 0 ? (n + groups - 1) / groups : 1;
        if (per > cap) per = cap;
        return dim3(gx, n > 0 ? (n + per - 1) / per : 1);
    }
};
