// Self copy-paste (Simple Copy-Paste between two real images) for gfx950, bit-exact with the reference's single paste step
// (DG/divergen/data/transforms/custom_copypaste.py:343-389 _scp_src_to_dst, :428-506 _copy_paste / get_updated_masks,
// :413-426 get_bboxes; 'basic' blend).  Unlike the pool compositor (compositor.hip: K <= 31 small RGBA patches, one cover bit
// each) this pastes, in ONE step, up to 99 full-frame masks of a second image, pixels taken from that image at the same
// coordinates, onto a canvas (H, W) that may be larger than the destination and smaller or larger than the source.
//   k0 init     : per-object statistics reset, `composed` plane zeroed
//   k1 source   : the m selected source planes copied (cropped / zero-padded) to out_masks[off + j]; their union ORed into the
//                 per-pixel `composed` byte plane (16 pixels per lane, 16-byte reads / writes; the planes split into groups over
//                 grid.y so that small frames still fill the chip, one 32-bit atomic OR per non-zero word and group)
//   k2 dest     : per 16-pixel chunk the composed bytes are read once; the image select (grid.y == 0) and every destination
//                 object of the group: out = composed ? 0 : mask, count and extents of the surviving pixels folded per lane,
//                 reduced over the wave, then LDS, then one global atomic set per workgroup and touched object
//   k3 resolve  : one lane per destination object: mask-derived box, the occlusion filter
// Rows / columns beyond (h1, w1) of the destination or (hs, ws) of the source read as 0 without touching memory.
//
// Several source images (INPUT.SCP_NUM_SRC > 1, dgx_self_copy_merge below) run the SAME source and destination kernels once per
// temporary stage of CopyPaste.__call__ (custom_copypaste.py:274-297), with the canvas clip compiled in (CLIP): see there.
#include "self_copy_common.h"

struct ScFlags { bool dst_vec, src_vec, out_vec; };

// 0xff for the bytes of chunk (y, x .. x + 15) inside the canvas (h, w)
__device__ __forceinline__ bool sc_clip16(int y, int x, int h, int w, uint32_t (&cm)[4]) {
    const int n = y < h ? min(max(w - x, 0), SCX) : 0;      // bytes inside
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = min(max(n - 4 * q, 0), 4);
        cm[q] = k == 4 ? 0xffffffffu : ((1u << (8 * k)) - 1u);
    }
    return n > 0;
}

// Planes ja .. jb of the group -> out_masks[off + j], their union -> composed.  sel: the source plane of each j (nullptr: plane j
// itself, the paste-all and the merge).  CLIP: a merge stage -- every chunk is masked with the stage's canvas clip = (h, w), which an
// earlier kernel on the stream wrote; a chunk wholly outside is not read.  Without CLIP `clip` is not read.
template <bool CLIP>
__global__ __launch_bounds__(256) void sc_source_kernel(const uint8_t* __restrict__ src_masks, int ns, int hs, int ws,
                                                        const int32_t* __restrict__ sel, int m, int per_group, int off, int H, int W,
                                                        int ncx, ScFlags fl, const int32_t* __restrict__ clip,
                                                        uint8_t* __restrict__ out_masks, uint32_t* __restrict__ composed) {
    __shared__ int32_t s_sel[SC_MAX_M];
    const int ja = blockIdx.y * per_group, jb = min(m, ja + per_group);
    for (int j = ja + threadIdx.x; j < jb; j += blockDim.x) s_sel[j - ja] = sel ? sel[j] : j;
    __syncthreads();
    int h = 0, w = 0;
    if constexpr (CLIP) { h = clip[0]; w = clip[1]; }
    const int64_t HW = (int64_t)H * W, shw = (int64_t)hs * ws, nchunk = (int64_t)H * ncx;
    for (int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ci < nchunk; ci += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(ci / ncx), x = (int)(ci - (int64_t)y * ncx) * SCX;
        uint32_t cm[4], acc[4] = {0u, 0u, 0u, 0u};
        bool inside = true;
        if constexpr (CLIP) inside = sc_clip16(y, x, h, w, cm);
#pragma unroll 4
        for (int j = ja; j < jb; ++j) {
            const int plane = s_sel[j - ja];
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            if (inside && plane >= 0 && plane < ns) sc_load16(src_masks + plane * shw, y, x, hs, ws, fl.src_vec, v);      // (the host checks sel; a bad index reads nothing)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if constexpr (CLIP) v[q] &= cm[q];
                acc[q] |= v[q];
            }
            sc_store16(out_masks + (off + j) * HW, y, x, W, fl.out_vec, v);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t nz = sc_nonzero(acc[q]);
            if (nz) atomicOr(&composed[ci * 4 + q], nz);
        }
    }
}

// The destination (n0 planes of (h1, w1), its image) under the composed plane: out = (d & keep) | (source image & composed), keep =
// inside the canvas and not composed.  CLIP as in the source kernel; without it the canvas is the whole frame.
template <bool CLIP>
__device__ __forceinline__ void sc_dest(const uint8_t* dst_image, const uint8_t* dst_masks, int n0, int h1, int w1, const uint8_t* src_image,
                                        int hs, int ws, int H, int W, int ncx, int per_group, ScFlags fl, const int32_t* clip,
                                        const uint32_t* composed, uint8_t* out_image, uint8_t* out_masks, int32_t* stats) {
    __shared__ int32_t s[SC_MAX_OPG * 5];
    int h = 0, w = 0;
    if constexpr (CLIP) { h = clip[0]; w = clip[1]; }
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
            uint32_t cm[4] = {~0u, ~0u, ~0u, ~0u};
            if constexpr (CLIP) sc_clip16(y, x, h, w, cm);
            const uint4 c = reinterpret_cast<const uint4*>(composed)[ci];
            const uint32_t comp[4] = {c.x * 0xffu, c.y * 0xffu, c.z * 0xffu, c.w * 0xffu};      // (set inside the canvas only)
#pragma unroll
            for (int q = 0; q < 4; ++q) keep[q] = cm[q] & ~comp[q];
            if (blockIdx.y == 0) {
                for (int ch = 0; ch < 3; ++ch) {
                    uint32_t d[4], sv[4] = {0u, 0u, 0u, 0u}, o[4];
                    sc_load16(dst_image + ch * dhw, y, x, h1, w1, fl.dst_vec, d);
                    if (comp[0] | comp[1] | comp[2] | comp[3]) sc_load16(src_image + ch * shw, y, x, hs, ws, fl.src_vec, sv);
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = (d[q] & keep[q]) | (sv[q] & comp[q]);
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

// Two shells around sc_dest, because a merge runs it IN PLACE from its second stage on (dst_image == out_image, dst_masks ==
// out_masks: every lane reads the 16 bytes it writes, and nothing else).  __restrict__ on those four would be a false promise there,
// so the merge's shell has none; the paste never aliases and keeps the qualifier, which lets the compiler issue the reads of the next
// channel / plane before the stores of this one.  Dropping it for both would need a measurement the paste has no reason to risk.
__global__ __launch_bounds__(256) void sc_dest_kernel(const uint8_t* __restrict__ dst_image, const uint8_t* __restrict__ dst_masks,
                                                      int n0, int h1, int w1, const uint8_t* __restrict__ src_image, int hs, int ws,
                                                      int H, int W, int ncx, int per_group, ScFlags fl,
                                                      const uint32_t* __restrict__ composed, uint8_t* __restrict__ out_image,
                                                      uint8_t* __restrict__ out_masks, int32_t* __restrict__ stats) {
    sc_dest<false>(dst_image, dst_masks, n0, h1, w1, src_image, hs, ws, H, W, ncx, per_group, fl, nullptr, composed, out_image, out_masks, stats);
}

__global__ __launch_bounds__(256) void sc_dest_kernel_inplace(const uint8_t* acc_image, const uint8_t* acc_masks, int nacc, int ha, int wa,
                                                              const uint8_t* __restrict__ src_image, int hs, int ws, int Hb, int Wb,
                                                              int ncx, int per_group, ScFlags fl, const int32_t* __restrict__ clip,
                                                              const uint32_t* __restrict__ composed, uint8_t* out_image,
                                                              uint8_t* out_masks, int32_t* __restrict__ stats) {
    sc_dest<true>(acc_image, acc_masks, nacc, ha, wa, src_image, hs, ws, Hb, Wb, ncx, per_group, fl, clip, composed, out_image, out_masks, stats);
}

__global__ void sc_init_kernel(int32_t* __restrict__ stats, int n0, uint32_t* __restrict__ composed, int64_t nwords) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < (int64_t)n0 * 5; i += step) stats[i] = sc_stat_init((int)(i % 5));
    for (int64_t i = i0; i < nwords; i += step) composed[i] = 0u;
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
    const int64_t nchunk = (int64_t)H * ncx;
    uint32_t* composed = reinterpret_cast<uint32_t*>(workspace + sc_pad4((int64_t)n0 * 5));
    ScFlags fl;
    fl.dst_vec = (w1 % SCX) == 0 && sc_aligned16(dst_image) && sc_aligned16(dst_masks);
    fl.src_vec = ws > 0 && (ws % SCX) == 0 && sc_aligned16(src_image) && sc_aligned16(src_masks);
    fl.out_vec = (W % SCX) == 0 && sc_aligned16(out_image) && sc_aligned16(out_masks);
    const int64_t ninit = nchunk * 4 > (int64_t)n0 * 5 ? nchunk * 4 : (int64_t)n0 * 5;
    hipLaunchKernelGGL(sc_init_kernel, dim3(sc_blocks(ninit)), dim3(256), 0, st, workspace, n0, composed, nchunk * 4);
    const ScGrid grid(nchunk);
    int per;
    if (m > 0) {
        const dim3 g = grid.split(m, SC_MAX_M, per);      // s_sel holds one group's indices (only a merged or a paste-all source has m > 99)
        hipLaunchKernelGGL(sc_source_kernel<false>, g, dim3(256), 0, st, src_masks, ns, hs, ws, sel, m, per, n0, H, W, ncx, fl, nullptr,
                           out_masks, composed);
    }
    const dim3 g = grid.split(n0, SC_MAX_OPG, per);
    hipLaunchKernelGGL(sc_dest_kernel, g, dim3(256), 0, st, dst_image, dst_masks, n0, h1, w1, src_image, hs, ws, H, W, ncx, per, fl,
                       composed, out_image, out_masks, workspace);
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

// ---- Several source images (INPUT.SCP_NUM_SRC > 1): the temporary stages of CopyPaste.__call__
// (DG/divergen/data/transforms/custom_copypaste.py:274-297: the first non-empty source is the accumulator, every further source
// is pasted onto it by _scp_src_to_dst(acc, s, is_tmp_dst=True), :343-389, then _copy_paste, :428-506), bit-exact, all S - 1 stages
// on one stream without a host round trip.  The final paste of the accumulator onto the destination is dgx_self_copy_paste_merged.
// The accumulator lives in the outputs at the bounding size (Hb, Wb) of the sources.  A stage's canvas (h, w) = the ceil of the
// largest y2 / x2 among the accumulator's current boxes (the objects still valid) and the stage's source boxes; the reference crops
// or zero-pads all four arrays to it, permanently -- here it is a predicate: a pixel outside (h, w) is written as zero, in the image,
// in every accumulator plane and in the stage's source planes, so it is gone at every later stage as well.
//   k0 init     : statistics and `composed` planes of all stages reset, boxes copied, validity set; stage 1's canvas
//   per stage t = 1 .. S - 1 (source t onto the accumulator of sources 0 .. t - 1):
//   k1 source   : sc_source_kernel<true>, every plane of source t (no sel) -> out_masks rows off ..
//   k2 dest     : sc_dest_kernel_inplace over the accumulator planes: source 0 itself, (h_0, w_0), at stage 1; out_image / out_masks,
//                 (Hb, Wb), in place, later
//   k3 resolve  : one workgroup: mask-derived boxes, the occlusion filter against the boxes of the stage before; the next stage's canvas
// Integer atomics only: two runs give the same bytes.
struct ScmSrc { const uint8_t* image; const uint8_t* masks; int m, h, w, off; bool vec; };      // off: first row of the source in out_masks

// ceil of a box coordinate as a canvas extent
__device__ __forceinline__ int scm_ceil(float v) { return (int)fminf(fmaxf(ceilf(v), 0.0f), 1.0e9f); }

__global__ __launch_bounds__(256) void scm_init_kernel(int32_t* __restrict__ stats, int64_t nstat, int nstage, uint32_t* __restrict__ composed,
                                                       int64_t nwords, const float* __restrict__ boxes, int M, int n01,
                                                       float* __restrict__ out_boxes, uint8_t* __restrict__ out_valid,
                                                       int32_t* __restrict__ clip) {
    __shared__ int32_t s_hw[2];
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < nstat * nstage; i += step) stats[i] = sc_stat_init((int)((i % nstat) % 5));      // nstat records per stage
    for (int64_t i = i0; i < nwords; i += step) composed[i] = 0u;
    for (int64_t i = i0; i < (int64_t)M * 4; i += step) out_boxes[i] = boxes[i];
    for (int64_t i = i0; i < M; i += step) out_valid[i] = 1;
    if (blockIdx.x == 0) {                          // stage 1's canvas: the boxes of sources 0 and 1
        if (threadIdx.x < 2) s_hw[threadIdx.x] = 0;
        __syncthreads();
        for (int o = threadIdx.x; o < n01; o += blockDim.x) {
            atomicMax(&s_hw[0], scm_ceil(boxes[4 * o + 3]));
            atomicMax(&s_hw[1], scm_ceil(boxes[4 * o + 2]));
        }
        __syncthreads();
        if (threadIdx.x < 2) clip[threadIdx.x] = s_hw[threadIdx.x];
    }
}

// One workgroup.  The nacc accumulator objects of this stage: box of the updated mask, kept when _copy_paste keeps it against the box
// that came out of the stage before (an object once dropped stays dropped; its plane and box are still updated, nobody reads them).
// Then the next stage's canvas over the objects still valid and the next source's own boxes (rows nacc .. nnext - 1, untouched so
// far); nnext == 0: this was the last stage.
__global__ __launch_bounds__(256) void scm_resolve_kernel(const int32_t* __restrict__ stats, int nacc, int nnext, float* __restrict__ boxes,
                                                          uint8_t* __restrict__ valid, int32_t* __restrict__ clip_next) {
    __shared__ int32_t s_hw[2];
    if (threadIdx.x < 2) s_hw[threadIdx.x] = 0;
    __syncthreads();
    const int n = nnext > nacc ? nnext : nacc;
    for (int obj = threadIdx.x; obj < n; obj += blockDim.x) {
        float b[4];
        bool ok = true;
        if (obj < nacc) {
            ok = sc_resolve(stats + 5 * obj, boxes + 4 * obj, b) && valid[obj] != 0;
            for (int i = 0; i < 4; ++i) boxes[4 * obj + i] = b[i];
            if (!ok) valid[obj] = 0;
        } else {
            for (int i = 0; i < 4; ++i) b[i] = boxes[4 * obj + i];
        }
        if (ok && nnext > 0) { atomicMax(&s_hw[0], scm_ceil(b[3])); atomicMax(&s_hw[1], scm_ceil(b[2])); }
    }
    __syncthreads();
    if (nnext > 0 && threadIdx.x < 2) clip_next[threadIdx.x] = s_hw[threadIdx.x];
}

extern "C" int64_t dgx_self_copy_merge_workspace_words(int S, int M, int Hb, int Wb) {
    if (S < 2 || S > SCM_MAX_SRC || M < 0 || Hb <= 0 || Wb <= 0) return 0;
    const int64_t nchunk = (int64_t)Hb * ((Wb + SCX - 1) / SCX);
    return 2 * SCM_MAX_SRC + (S - 1) * (sc_pad4((int64_t)M * 5) + nchunk * 4);
}

extern "C" int dgx_self_copy_merge(const uint8_t* const* images, const uint8_t* const* masks, const int32_t* counts, const int32_t* sizes,
                                   int S, const float* boxes, int Hb, int Wb, uint8_t* out_image, uint8_t* out_masks, float* out_boxes,
                                   uint8_t* out_valid, int32_t* workspace, void* stream) {
    if (S < 2 || S > SCM_MAX_SRC || !images || !masks || !counts || !sizes || !boxes || !out_image || !out_masks || !out_boxes ||
        !out_valid || !workspace || ((uintptr_t)workspace & 15) || Hb <= 0 || Wb <= 0)
        return DGX_ERR_BAD_ARG;
    if ((int64_t)Hb * Wb >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;
    ScmSrc src[SCM_MAX_SRC];
    int M = 0;
    for (int i = 0; i < S; ++i) {
        ScmSrc& s = src[i];
        s.image = images[i]; s.masks = masks[i]; s.m = counts[i]; s.h = sizes[2 * i]; s.w = sizes[2 * i + 1]; s.off = M;
        if (!s.image || !s.masks || s.m < 1 || s.m > SC_MAX_M || s.h <= 0 || s.w <= 0 || s.h > Hb || s.w > Wb) return DGX_ERR_BAD_ARG;
        s.vec = (s.w % SCX) == 0 && sc_aligned16(s.image) && sc_aligned16(s.masks);
        M += s.m;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool out_vec = (Wb % SCX) == 0 && sc_aligned16(out_image) && sc_aligned16(out_masks);
    const int ncx = (Wb + SCX - 1) / SCX;
    const int64_t nchunk = (int64_t)Hb * ncx, nstat = sc_pad4((int64_t)M * 5);
    int32_t* clip = workspace;                                       // (h, w) per stage
    int32_t* stats = workspace + 2 * SCM_MAX_SRC;                    // (S - 1) x nstat
    uint32_t* composed = reinterpret_cast<uint32_t*>(stats + (S - 1) * nstat);      // (S - 1) x nchunk x 4
    const int64_t nwords = (S - 1) * nchunk * 4, ninit = nwords > (S - 1) * nstat ? nwords : (S - 1) * nstat;
    hipLaunchKernelGGL(scm_init_kernel, dim3(sc_blocks(ninit)), dim3(256), 0, st, stats, nstat, S - 1, composed, nwords, boxes, M,
                       src[0].m + src[1].m, out_boxes, out_valid, clip + 2);
    const ScGrid grid(nchunk);
    for (int t = 1; t < S; ++t) {
        const ScmSrc& s = src[t];
        const int nacc = s.off;
        int32_t* stats_t = stats + (t - 1) * nstat;
        uint32_t* composed_t = composed + (t - 1) * nchunk * 4;
        const bool first = t == 1;                 // the accumulator is source 0 itself; later the outputs, in place
        const ScFlags fl = {first ? src[0].vec : out_vec, s.vec, out_vec};
        int per;
        dim3 g = grid.split(s.m, SC_MAX_M, per);
        hipLaunchKernelGGL(sc_source_kernel<true>, g, dim3(256), 0, st, s.masks, s.m, s.h, s.w, nullptr, s.m, per, s.off, Hb, Wb, ncx, fl,
                           clip + 2 * t, out_masks, composed_t);
        g = grid.split(nacc, SC_MAX_OPG, per);
        hipLaunchKernelGGL(sc_dest_kernel_inplace, g, dim3(256), 0, st, first ? src[0].image : out_image, first ? src[0].masks : out_masks,
                           nacc, first ? src[0].h : Hb, first ? src[0].w : Wb, s.image, s.h, s.w, Hb, Wb, ncx, per, fl, clip + 2 * t,
                           composed_t, out_image, out_masks, stats_t);
        hipLaunchKernelGGL(scm_resolve_kernel, dim3(1), dim3(256), 0, st, stats_t, nacc, t + 1 < S ? nacc + s.m + src[t + 1].m : 0,
                           out_boxes, out_valid, clip + 2 * (t + 1 < S ? t + 1 : t));
    }
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
