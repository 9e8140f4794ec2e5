// Self copy-paste (Simple Copy-Paste between two real images) for gfx950, bit-exact with the reference's single paste step
// (DG/divergen/data/transforms/custom_copypaste.py:343-389 _scp_src_to_dst, :428-506 _copy_paste / get_updated_masks,
// :413-426 get_bboxes; 'basic' blend).  Unlike the pool compositor (compositor.hip: K <= 31 small RGBA patches, one cover bit
// each) this pastes, in ONE step, up to 99 full-frame masks of a second image, pixels taken from that image at the same
// coordinates, onto a canvas (H, W) that may be larger than the destination and smaller or larger than the source.
//   k0 init     : per-object statistics reset, `composed` plane zeroed
//   k1 source   : the m selected source planes copied (cropped / zero-padded) to out_masks[n0 + j]; their union ORed into the
//                 per-pixel `composed` byte plane (16 pixels per lane, 16-byte reads / writes; the planes split into groups over
//                 grid.y so that small frames still fill the chip, one 32-bit atomic OR per non-zero word and group)
//   k2 dest     : per 16-pixel chunk the composed bytes are read once; the image select (grid.y == 0) and every destination
//                 object of the group: out = composed ? 0 : mask, count and extents of the surviving pixels folded per lane,
//                 reduced over the wave, then LDS, then one global atomic set per workgroup and touched object
//   k3 resolve  : one lane per destination object: mask-derived box, the occlusion filter
// Rows / columns beyond (h1, w1) of the destination or (hs, ws) of the source read as 0 without touching memory.
#include "self_copy_common.h"

__global__ void sc_init_kernel(int32_t* __restrict__ stats, int n0, uint32_t* __restrict__ composed, int64_t nwords) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < (int64_t)n0 * 5; i += step) stats[i] = sc_stat_init((int)(i % 5));
    for (int64_t i = i0; i < nwords; i += step) composed[i] = 0u;
}

struct ScFlags { bool dst_vec, src_vec, out_vec; };

__global__ __launch_bounds__(256) void sc_source_kernel(const uint8_t* __restrict__ src_masks, int ns, int hs, int ws,
                                                        const int32_t* __restrict__ sel, int m, int per_group, int n0, int H, int W,
                                                        int ncx, ScFlags fl, uint8_t* __restrict__ out_masks,
                                                        uint32_t* __restrict__ composed) {
    __shared__ int32_t s_sel[SC_MAX_M];
    const int ja = blockIdx.y * per_group, jb = min(m, ja + per_group);
    for (int j = ja + threadIdx.x; j < jb; j += blockDim.x) s_sel[j - ja] = sel ? sel[j] : j;      // no sel: plane j itself (paste-all)
    __syncthreads();
    const int64_t HW = (int64_t)H * W, shw = (int64_t)hs * ws, nchunk = (int64_t)H * ncx;
    for (int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ci < nchunk; ci += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(ci / ncx), x = (int)(ci - (int64_t)y * ncx) * SCX;
        uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll 4
        for (int j = ja; j < jb; ++j) {
            const int plane = s_sel[j - ja];
            uint32_t v[4];
            if (plane >= 0 && plane < ns) sc_load16(src_masks + plane * shw, y, x, hs, ws, fl.src_vec, v);      // (the host checks sel; a bad index reads nothing)
            else v[0] = v[1] = v[2] = v[3] = 0u;
            sc_store16(out_masks + (n0 + j) * HW, y, x, W, fl.out_vec, v);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] |= v[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t nz = sc_nonzero(acc[q]);
            if (nz) atomicOr(&composed[ci * 4 + q], nz);
        }
    }
}

__global__ __launch_bounds__(256) void sc_dest_kernel(const uint8_t* __restrict__ dst_image, const uint8_t* __restrict__ dst_masks,
                                                      int n0, int h1, int w1, const uint8_t* __restrict__ src_image, int hs, int ws,
                                                      int H, int W, int ncx, int per_group, ScFlags fl,
                                                      const uint32_t* __restrict__ composed, uint8_t* __restrict__ out_image,
                                                      uint8_t* __restrict__ out_masks, int32_t* __restrict__ stats) {
    __shared__ int32_t s[SC_MAX_OPG * 5];
    const int oa = blockIdx.y * per_group, ob = min(n0, oa + per_group);
    for (int i = threadIdx.x; i < (ob - oa) * 5; i += blockDim.x) s[i] = sc_stat_init(i % 5);
    __syncthreads();
    const int64_t HW = (int64_t)H * W, dhw = (int64_t)h1 * w1, shw = (int64_t)hs * ws, nchunk = (int64_t)H * ncx;
    const int lane = threadIdx.x & 63;
    // block-uniform trip count: the wave reduction below needs every lane of a wave in the loop
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < nchunk; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ci = base + threadIdx.x;
        const bool active = ci < nchunk;
        const int y = active ? (int)(ci / ncx) : 0, x = active ? (int)(ci - (int64_t)y * ncx) * SCX : 0;
        uint32_t keep[4] = {0u, 0u, 0u, 0u};       // 0xff where the destination survives
        if (active) {
            const uint4 c = reinterpret_cast<const uint4*>(composed)[ci];
            keep[0] = ~(c.x * 0xffu); keep[1] = ~(c.y * 0xffu); keep[2] = ~(c.z * 0xffu); keep[3] = ~(c.w * 0xffu);
            if (blockIdx.y == 0) {
                for (int ch = 0; ch < 3; ++ch) {
                    uint32_t d[4], sv[4], o[4];
                    sc_load16(dst_image + ch * dhw, y, x, h1, w1, fl.dst_vec, d);
                    if (~(keep[0] & keep[1] & keep[2] & keep[3])) sc_load16(src_image + ch * shw, y, x, hs, ws, fl.src_vec, sv);
                    else sv[0] = sv[1] = sv[2] = sv[3] = 0u;
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = (d[q] & keep[q]) | (sv[q] & ~keep[q]);
                    sc_store16(out_image + ch * HW, y, x, W, fl.out_vec, o);
                }
            }
        }
        for (int obj = oa; obj < ob; ++obj) {
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            if (active) {
                sc_load16(dst_masks + obj * dhw, y, x, h1, w1, fl.dst_vec, v);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] &= keep[q];
                sc_store16(out_masks + obj * HW, y, x, W, fl.out_vec, v);
            }
            sc_fold_stats(v, y, x, lane, s + 5 * (obj - oa));
        }
    }
    __syncthreads();
    sc_flush_stats(s, ob - oa, stats + (int64_t)oa * 5);
}

// get_bboxes of the updated mask (x_max + 1, y_max + 1; zeros when empty), then _copy_paste's filter: kept when every
// |new - old| <= 10 or more than 300 pixels survive.  m == 0: nothing was pasted, every object is valid.
__global__ void sc_resolve_kernel(const int32_t* __restrict__ stats, const float* __restrict__ boxes0, int n0, int m,
                                  float* __restrict__ out_boxes, uint8_t* __restrict__ out_valid) {
    const int obj = blockIdx.x * blockDim.x + threadIdx.x;
    if (obj >= n0) return;
    float b[4];
    const bool ok = sc_resolve(stats + 5 * obj, boxes0 + 4 * obj, b);
    for (int i = 0; i < 4; ++i) out_boxes[4 * obj + i] = b[i];
    out_valid[obj] = (m == 0 || ok) ? 1 : 0;
}

// max_m: 99 for one source image; 99 per merged source when the planes come out of dgx_self_copy_merge.  ident: the paste-all entry --
// sel is not read (plane j is source plane j), m == ns, and m is bounded by the grid and the 64-bit plane offsets alone.
static int sc_paste(const uint8_t* dst_image, const uint8_t* dst_masks, const float* dst_boxes0, int n0, int h1, int w1,
                    const uint8_t* src_image, const uint8_t* src_masks, int ns, int hs, int ws, const int32_t* sel, int m, int max_m,
                    bool ident, int H, int W, uint8_t* out_image, uint8_t* out_masks, float* out_boxes, uint8_t* out_valid, int32_t* workspace,
                    void* stream) {
    if (n0 < 0 || ns < 0 || m < 0 || m > max_m || h1 <= 0 || w1 <= 0 || H < h1 || W < w1 || (m > 0 && (ns <= 0 || hs <= 0 || ws <= 0)))
        return DGX_ERR_BAD_ARG;
    if (!dst_image || !out_image || !workspace || ((uintptr_t)workspace & 15) || (n0 > 0 && (!dst_masks || !dst_boxes0 || !out_boxes || !out_valid)) ||
        (m > 0 && (!src_image || !src_masks || (!sel && !ident))) || ((int64_t)n0 + m > 0 && !out_masks))
        return DGX_ERR_BAD_ARG;
    if ((int64_t)H * W >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;
    if (ident) {
        // grid.y = ceil(m / per) with per <= SC_MAX_M whatever the frame; rows n0 .. n0 + m - 1 of out_masks as int, their bytes as int64
        const int64_t rows = (int64_t)n0 + m;
        if (((int64_t)m + SC_MAX_M - 1) / SC_MAX_M > 65535 || rows > 0x7fffffff || rows > INT64_MAX / ((int64_t)H * W)) return DGX_ERR_UNSUPPORTED;
        sel = nullptr;
    }
    hipStream_t st = (hipStream_t)stream;
    if (m == 0) { hs = 0; ws = 0; }                // the source is never read
    const int ncx = (W + SCX - 1) / SCX;
    const int64_t nchunk = (int64_t)H * ncx, nstat = ((int64_t)n0 * 5 + 3) & ~(int64_t)3;
    uint32_t* composed = reinterpret_cast<uint32_t*>(workspace + nstat);
    auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    ScFlags fl;
    fl.dst_vec = (w1 % SCX) == 0 && al(dst_image) && al(dst_masks);
    fl.src_vec = ws > 0 && (ws % SCX) == 0 && al(src_image) && al(src_masks);
    fl.out_vec = (W % SCX) == 0 && al(out_image) && al(out_masks);
    const int64_t ninit = nchunk * 4 > (int64_t)n0 * 5 ? nchunk * 4 : (int64_t)n0 * 5;
    hipLaunchKernelGGL(sc_init_kernel, dim3((int)((ninit + 255) / 256 < 2048 ? (ninit + 255) / 256 : 2048)), dim3(256), 0, st,
                       workspace, n0, composed, nchunk * 4);
    // one lane per 16 pixels; the planes split into groups so that small frames still fill the chip
    const int gx = (int)((nchunk + 255) / 256 < 2048 ? (nchunk + 255) / 256 : 2048);
    const int want = gx >= 1024 ? 1 : (1024 + gx - 1) / gx;
    if (m > 0) {
        const int groups = want < m ? want : m;
        int per = (m + groups - 1) / groups;
        if (per > SC_MAX_M) per = SC_MAX_M;          // s_sel holds one group's indices (only a merged or a paste-all source has m > 99)
        hipLaunchKernelGGL(sc_source_kernel, dim3(gx, (m + per - 1) / per), dim3(256), 0, st, src_masks, ns, hs, ws, sel, m, per, n0,
                           H, W, ncx, fl, out_masks, composed);
    }
    {
        int groups = want < n0 ? want : n0;
        if (groups < 1) groups = 1;
        int per = n0 > 0 ? (n0 + groups - 1) / groups : 1;
        if (per > SC_MAX_OPG) per = SC_MAX_OPG;
        const int gy = n0 > 0 ? (n0 + per - 1) / per : 1;
        hipLaunchKernelGGL(sc_dest_kernel, dim3(gx, gy), dim3(256), 0, st, dst_image, dst_masks, n0, h1, w1, src_image, hs, ws, H, W,
                           ncx, per, fl, composed, out_image, out_masks, workspace);
    }
    if (n0 > 0)
        hipLaunchKernelGGL(sc_resolve_kernel, dim3((n0 + 63) / 64), dim3(64), 0, st, workspace, dst_boxes0, n0, m, out_boxes, out_valid);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_self_copy_paste(const uint8_t* dst_image, const uint8_t* dst_masks, const float* dst_boxes0, int n0, int h1, int w1,
                                   const uint8_t* src_image, const uint8_t* src_masks, int ns, int hs, int ws,
                                   const int32_t* sel, int m, int H, int W, uint8_t* out_image, uint8_t* out_masks,
                                   float* out_boxes, uint8_t* out_valid, int32_t* workspace, void* stream) {
    return sc_paste(dst_image, dst_masks, dst_boxes0, n0, h1, w1, src_image, src_masks, ns, hs, ws, sel, m, SC_MAX_M, false, H, W, out_image,
                    out_masks, out_boxes, out_valid, workspace, stream);
}

extern "C" int dgx_self_copy_paste_merged(const uint8_t* dst_image, const uint8_t* dst_masks, const float* dst_boxes0, int n0, int h1, int w1,
                                          const uint8_t* src_image, const uint8_t* src_masks, int ns, int hs, int ws,
                                          const int32_t* sel, int m, int H, int W, uint8_t* out_image, uint8_t* out_masks,
                                          float* out_boxes, uint8_t* out_valid, int32_t* workspace, void* stream) {
    return sc_paste(dst_image, dst_masks, dst_boxes0, n0, h1, w1, src_image, src_masks, ns, hs, ws, sel, m, SC_MAX_M * SCM_MAX_SRC, false, H, W,
                    out_image, out_masks, out_boxes, out_valid, workspace, stream);
}

// every plane of the source in order (CopyPaste(selected=False)): no sel, no bound of 99
extern "C" int dgx_self_copy_paste_all(const uint8_t* dst_image, const uint8_t* dst_masks, const float* dst_boxes0, int n0, int h1, int w1,
                                       const uint8_t* src_image, const uint8_t* src_masks, int ns, int hs, int ws, int H, int W,
                                       uint8_t* out_image, uint8_t* out_masks, float* out_boxes, uint8_t* out_valid, int32_t* workspace,
                                       void* stream) {
    return sc_paste(dst_image, dst_masks, dst_boxes0, n0, h1, w1, src_image, src_masks, ns, hs, ws, nullptr, ns, 0x7fffffff, true, H, W,
                    out_image, out_masks, out_boxes, out_valid, workspace, stream);
}
