// Self copy-paste from several source images (INPUT.SCP_NUM_SRC > 1) for gfx950: the temporary stages of CopyPaste.__call__
// (DG/divergen/data/transforms/custom_copypaste.py:274-297: the first non-empty source is the accumulator, every further source
// is pasted onto it by _scp_src_to_dst(acc, s, is_tmp_dst=True), :343-389, then _copy_paste, :428-506), bit-exact, all S - 1 stages
// on one stream without a host round trip.  The final paste of the accumulator onto the destination is dgx_self_copy_paste_merged.
// The accumulator lives in the outputs at the bounding size (Hb, Wb) of the sources.  A stage's canvas (h, w) = the ceil of the
// largest y2 / x2 among the accumulator's current boxes (the objects still valid) and the stage's source boxes; the reference crops
// or zero-pads all four arrays to it, permanently -- here it is a predicate: a pixel outside (h, w) is written as zero, in the image,
// in every accumulator plane and in the stage's source planes, so it is gone at every later stage as well.
//   k0 init     : statistics and `composed` planes of all stages reset, boxes copied, validity set; stage 1's canvas
//   per stage t = 1 .. S - 1 (source t onto the accumulator of sources 0 .. t - 1):
//   k1 source   : source t's planes clipped to the canvas -> out_masks, their union ORed into the stage's `composed` byte plane
//   k2 dest     : the image select (grid.y == 0) and every accumulator plane: out = inside the canvas and not composed ? plane : 0, in
//                 place (stage 1 reads source 0 itself); count and extents per lane -> wave -> LDS -> one global atomic set per workgroup
//   k3 resolve  : one workgroup: mask-derived boxes, the occlusion filter against the boxes of the stage before; the next stage's canvas
// Integer atomics only: two runs give the same bytes.
#include "self_copy_common.h"

struct ScmSrc { const uint8_t* image; const uint8_t* masks; int m, h, w, off; bool vec; };      // off: first row of the source in out_masks

// 0xff for the bytes of chunk (y, x .. x + 15) inside the canvas (h, w)
__device__ __forceinline__ bool scm_clip16(int y, int x, int h, int w, uint32_t (&cm)[4]) {
    const int n = y < h ? min(max(w - x, 0), SCX) : 0;      // bytes inside
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = min(max(n - 4 * q, 0), 4);
        cm[q] = k == 4 ? 0xffffffffu : ((1u << (8 * k)) - 1u);
    }
    return n > 0;
}

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

__global__ __launch_bounds__(256) void scm_source_kernel(ScmSrc s, int per_group, int Hb, int Wb, int ncx, bool out_vec,
                                                         const int32_t* __restrict__ clip, uint8_t* __restrict__ out_masks,
                                                         uint32_t* __restrict__ composed) {
    const int h = clip[0], w = clip[1];
    const int ja = blockIdx.y * per_group, jb = min(s.m, ja + per_group);
    const int64_t HW = (int64_t)Hb * Wb, shw = (int64_t)s.h * s.w, nchunk = (int64_t)Hb * ncx;
    for (int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ci < nchunk; ci += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(ci / ncx), x = (int)(ci - (int64_t)y * ncx) * SCX;
        uint32_t cm[4], acc[4] = {0u, 0u, 0u, 0u};
        const bool inside = scm_clip16(y, x, h, w, cm);
#pragma unroll 4
        for (int j = ja; j < jb; ++j) {
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            if (inside) sc_load16(s.masks + j * shw, y, x, s.h, s.w, s.vec, v);
#pragma unroll
            for (int q = 0; q < 4; ++q) { v[q] &= cm[q]; acc[q] |= v[q]; }
            sc_store16(out_masks + (s.off + j) * HW, y, x, Wb, out_vec, v);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t nz = sc_nonzero(acc[q]);
            if (nz) atomicOr(&composed[ci * 4 + q], nz);
        }
    }
}

// acc_image / acc_masks: the accumulator as the stage finds it -- source 0 itself, (ha, wa), at stage 1; out_image / out_masks,
// (Hb, Wb), later: then every lane reads the 16 bytes it writes, and nothing else (no __restrict__ on these four).
__global__ __launch_bounds__(256) void scm_dest_kernel(const uint8_t* acc_image, const uint8_t* acc_masks, int ha, int wa, bool acc_vec,
                                                       int nacc, ScmSrc s, int Hb, int Wb, int ncx, int per_group, bool out_vec,
                                                       const int32_t* __restrict__ clip, const uint32_t* __restrict__ composed,
                                                       uint8_t* out_image, uint8_t* out_masks, int32_t* __restrict__ stats) {
    __shared__ int32_t st[SC_MAX_OPG * 5];
    const int h = clip[0], w = clip[1];
    const int oa = blockIdx.y * per_group, ob = min(nacc, oa + per_group);
    for (int i = threadIdx.x; i < (ob - oa) * 5; i += blockDim.x) st[i] = sc_stat_init(i % 5);
    __syncthreads();
    const int64_t HW = (int64_t)Hb * Wb, ahw = (int64_t)ha * wa, shw = (int64_t)s.h * s.w, nchunk = (int64_t)Hb * ncx;
    const int lane = threadIdx.x & 63;
    // block-uniform trip count: the wave reduction needs every lane of a wave in the loop
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < nchunk; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ci = base + threadIdx.x;
        const bool active = ci < nchunk;
        const int y = active ? (int)(ci / ncx) : 0, x = active ? (int)(ci - (int64_t)y * ncx) * SCX : 0;
        uint32_t keep[4] = {0u, 0u, 0u, 0u};       // 0xff where the accumulator survives: inside the canvas and not composed
        if (active) {
            uint32_t cm[4];
            scm_clip16(y, x, h, w, cm);
            const uint4 c = reinterpret_cast<const uint4*>(composed)[ci];
            const uint32_t comp[4] = {c.x * 0xffu, c.y * 0xffu, c.z * 0xffu, c.w * 0xffu};      // (set inside the canvas only)
#pragma unroll
            for (int q = 0; q < 4; ++q) keep[q] = cm[q] & ~comp[q];
            if (blockIdx.y == 0) {
                for (int ch = 0; ch < 3; ++ch) {
                    uint32_t d[4], sv[4] = {0u, 0u, 0u, 0u}, o[4];
                    sc_load16(acc_image + ch * ahw, y, x, ha, wa, acc_vec, d);
                    if (comp[0] | comp[1] | comp[2] | comp[3]) sc_load16(s.image + ch * shw, y, x, s.h, s.w, s.vec, sv);
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = (d[q] & keep[q]) | (sv[q] & comp[q]);
                    sc_store16(out_image + ch * HW, y, x, Wb, out_vec, o);
                }
            }
        }
        for (int obj = oa; obj < ob; ++obj) {
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            if (active) {
                sc_load16(acc_masks + obj * ahw, y, x, ha, wa, acc_vec, v);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] &= keep[q];
                sc_store16(out_masks + obj * HW, y, x, Wb, out_vec, v);
            }
            sc_fold_stats(v, y, x, lane, st + 5 * (obj - oa));
        }
    }
    __syncthreads();
    sc_flush_stats(st, ob - oa, stats + (int64_t)oa * 5);
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

static int64_t scm_pad4(int64_t n) { return (n + 3) & ~(int64_t)3; }

extern "C" int64_t dgx_self_copy_merge_workspace_words(int S, int M, int Hb, int Wb) {
    if (S < 2 || S > SCM_MAX_SRC || M < 0 || Hb <= 0 || Wb <= 0) return 0;
    const int64_t nchunk = (int64_t)Hb * ((Wb + SCX - 1) / SCX);
    return 2 * SCM_MAX_SRC + (S - 1) * (scm_pad4((int64_t)M * 5) + nchunk * 4);
}

extern "C" int dgx_self_copy_merge(const uint8_t* const* images, const uint8_t* const* masks, const int32_t* counts, const int32_t* sizes,
                                   int S, const float* boxes, int Hb, int Wb, uint8_t* out_image, uint8_t* out_masks, float* out_boxes,
                                   uint8_t* out_valid, int32_t* workspace, void* stream) {
    if (S < 2 || S > SCM_MAX_SRC || !images || !masks || !counts || !sizes || !boxes || !out_image || !out_masks || !out_boxes ||
        !out_valid || !workspace || ((uintptr_t)workspace & 15) || Hb <= 0 || Wb <= 0)
        return DGX_ERR_BAD_ARG;
    if ((int64_t)Hb * Wb >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;
    auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    ScmSrc src[SCM_MAX_SRC];
    int M = 0;
    for (int i = 0; i < S; ++i) {
        ScmSrc& s = src[i];
        s.image = images[i]; s.masks = masks[i]; s.m = counts[i]; s.h = sizes[2 * i]; s.w = sizes[2 * i + 1]; s.off = M;
        if (!s.image || !s.masks || s.m < 1 || s.m > SC_MAX_M || s.h <= 0 || s.w <= 0 || s.h > Hb || s.w > Wb) return DGX_ERR_BAD_ARG;
        s.vec = (s.w % SCX) == 0 && al(s.image) && al(s.masks);
        M += s.m;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool out_vec = (Wb % SCX) == 0 && al(out_image) && al(out_masks);
    const int ncx = (Wb + SCX - 1) / SCX;
    const int64_t nchunk = (int64_t)Hb * ncx, nstat = scm_pad4((int64_t)M * 5);
    int32_t* clip = workspace;                                       // (h, w) per stage
    int32_t* stats = workspace + 2 * SCM_MAX_SRC;                    // (S - 1) x nstat
    uint32_t* composed = reinterpret_cast<uint32_t*>(stats + (S - 1) * nstat);      // (S - 1) x nchunk x 4
    const int64_t nwords = (S - 1) * nchunk * 4, ninit = nwords > (S - 1) * nstat ? nwords : (S - 1) * nstat;
    hipLaunchKernelGGL(scm_init_kernel, dim3((int)((ninit + 255) / 256 < 2048 ? (ninit + 255) / 256 : 2048)), dim3(256), 0, st,
                       stats, nstat, S - 1, composed, nwords, boxes, M, src[0].m + src[1].m, out_boxes, out_valid, clip + 2);
    // one lane per 16 pixels; the planes split into groups so that small frames still fill the chip
    const int gx = (int)((nchunk + 255) / 256 < 2048 ? (nchunk + 255) / 256 : 2048);
    const int want = gx >= 1024 ? 1 : (1024 + gx - 1) / gx;
    for (int t = 1; t < S; ++t) {
        const ScmSrc& s = src[t];
        const int nacc = s.off;
        int32_t* stats_t = stats + (t - 1) * nstat;
        uint32_t* composed_t = composed + (t - 1) * nchunk * 4;
        {
            const int groups = want < s.m ? want : s.m, per = (s.m + groups - 1) / groups;
            hipLaunchKernelGGL(scm_source_kernel, dim3(gx, (s.m + per - 1) / per), dim3(256), 0, st, s, per, Hb, Wb, ncx, out_vec,
                               clip + 2 * t, out_masks, composed_t);
        }
        {
            const int groups = want < nacc ? want : nacc;
            int per = (nacc + groups - 1) / groups;
            if (per > SC_MAX_OPG) per = SC_MAX_OPG;
            const bool first = t == 1;
            hipLaunchKernelGGL(scm_dest_kernel, dim3(gx, (nacc + per - 1) / per), dim3(256), 0, st, first ? src[0].image : out_image,
                               first ? src[0].masks : out_masks, first ? src[0].h : Hb, first ? src[0].w : Wb,
                               first ? src[0].vec : out_vec, nacc, s, Hb, Wb, ncx, per, out_vec, clip + 2 * t, composed_t, out_image,
                               out_masks, stats_t);
        }
        hipLaunchKernelGGL(scm_resolve_kernel, dim3(1), dim3(256), 0, st, stats_t, nacc, t + 1 < S ? nacc + s.m + src[t + 1].m : 0,
                           out_boxes, out_valid, clip + 2 * (t + 1 < S ? t + 1 : t));
    }
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
