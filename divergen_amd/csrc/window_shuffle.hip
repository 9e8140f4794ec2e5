// Window gather / scatter: pad + cyclic shift + window_partition folded into one index map
// (swintransformer.py:216-233, :239-251).  Pure HBM-bound copy: 16 bytes per lane, one token row
// per group of C*esize/16 lanes, no intermediate padded / rolled tensors.
#include "dgx_common.h"
#include "winmap.h"

template <bool GATHER>
__global__ __launch_bounds__(256) void window_shuffle_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int vecC, int64_t total,
                                                             WmMap m) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int v = (int)(i % vecC);
        const int64_t tok = wm_row_token<int64_t, WM_CLASSIC>(m, i / vecC);      // i / vecC: the window-order row
        const int64_t xi = tok * vecC + v;
        if (GATHER) {
            uint4 z = {0u, 0u, 0u, 0u};
            dst[i] = tok >= 0 ? src[xi] : z;
        } else if (tok >= 0) {
            dst[xi] = src[i];
        }
    }
}

static int window_shuffle(bool gather, const void* src, void* dst, int B, int H, int W, int C, int ws, int shift,
                          int dtype, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0) return DGX_OK;
    const int es = dtype == DGX_BF16 ? 2 : 4;
    if (!src || !dst || !wm_map_ok(B, H, W, ws, shift, WM_CLASSIC) || (C * es) % 16) return DGX_ERR_BAD_ARG;
    const int vecC = C * es / 16;
    const WmMap m = wm_map(B, H, W, ws, shift);
    const int64_t total = wm_classic_rows(m) * vecC;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (gather)
        hipLaunchKernelGGL(window_shuffle_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, (uint4*)dst, vecC,
                           total, m);
    else
        hipLaunchKernelGGL(window_shuffle_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, (uint4*)dst, vecC,
                           total, m);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_window_gather(const void* x, void* xw, int B, int H, int W, int C, int ws, int shift, int dtype,
                                 void* stream) {
    return window_shuffle(true, x, xw, B, H, W, C, ws, shift, dtype, stream);
}
extern "C" int dgx_window_scatter(const void* xw, void* x, int B, int H, int W, int C, int ws, int shift, int dtype,
                                  void* stream) {
    return window_shuffle(false, xw, x, B, H, W, C, ws, shift, dtype, stream);
}
