// Background removal (INPUT.RM_BG_PROB) for gfx950, bit-exact with the reference's CopyPaste.remove_background
// (DG/divergen/data/transforms/custom_copypaste.py:101-109: image * any(gt_masks, dim=0)): every pixel outside the union of the
// image's own instance masks becomes 0 in all three channels.  One kernel, 16 pixels per lane through the row accesses of the self
// copy (self_copy_common.h): the n mask chunks are ORed in registers, the image is read only where the union has a pixel -- a chunk
// without one stores zeros unread -- and each lane reads its 16 pixels of a channel before it writes them, so out_image == image works.
// n == 0: the union is empty and the image comes out all zero (torch.any over an empty stack).
#include "self_copy_common.h"

struct RbFlags { bool img_vec, mask_vec, out_vec; };

// image / out_image may be the same array (no __restrict__ on these two)
__global__ __launch_bounds__(256) void rb_kernel(const uint8_t* image, const uint8_t* __restrict__ masks, int n, int h, int w, int ncx,
                                                 RbFlags fl, uint8_t* out_image) {
    const int64_t hw = (int64_t)h * w, nchunk = (int64_t)h * ncx;
    for (int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ci < nchunk; ci += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(ci / ncx), x = (int)(ci - (int64_t)y * ncx) * SCX;
        uint32_t keep[4] = {0u, 0u, 0u, 0u};       // 0xff where some mask has the pixel
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            uint32_t v[4];
            sc_load16(masks + j * hw, y, x, h, w, fl.mask_vec, v);
#pragma unroll
            for (int q = 0; q < 4; ++q) keep[q] |= v[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) keep[q] = sc_nonzero(keep[q]) * 0xffu;
        const bool any = (keep[0] | keep[1] | keep[2] | keep[3]) != 0u;
        for (int ch = 0; ch < 3; ++ch) {
            uint32_t d[4] = {0u, 0u, 0u, 0u};
            if (any) sc_load16(image + ch * hw, y, x, h, w, fl.img_vec, d);
#pragma unroll
            for (int q = 0; q < 4; ++q) d[q] &= keep[q];
            sc_store16(out_image + ch * hw, y, x, w, fl.out_vec, d);
        }
    }
}

extern "C" int dgx_remove_background(const uint8_t* image, const uint8_t* masks, int n, int h, int w, uint8_t* out_image, void* stream) {
    if (!image || !out_image || h <= 0 || w <= 0 || n < 0 || (n > 0 && !masks)) return DGX_ERR_BAD_ARG;
    if ((int64_t)h * w >= ((int64_t)1 << 31)) return DGX_ERR_UNSUPPORTED;
    const bool wide = (w % SCX) == 0;
    RbFlags fl;
    fl.img_vec = wide && sc_aligned16(image);
    fl.mask_vec = wide && sc_aligned16(masks);
    fl.out_vec = wide && sc_aligned16(out_image);
    const int ncx = (w + SCX - 1) / SCX;
    const int64_t nchunk = (int64_t)h * ncx;
    hipLaunchKernelGGL(rb_kernel, dim3(ScGrid(nchunk).gx), dim3(256), 0, (hipStream_t)stream, image, masks, n, h, w, ncx, fl, out_image);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
