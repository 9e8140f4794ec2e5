// Row-wise L2 normalisation with a scale (gfx950): the arithmetic of the open-vocabulary box classifier,
//   y[r,:] = t * x[r,:] / max(||x[r,:]||_2, 1e-12)          F.normalize(x, p=2, dim=1, eps=1e-12) * t
// Reference: DG/divergen/modeling/roi_heads/zero_shot_classifier.py:47,78,83.
// HBM-bound streaming kernel: one wave per row, four rows per 256-thread workgroup, the row read ONCE in 16-byte lanes
// (8 bf16 per load; an fp32 row takes two loads per 8 elements) and kept in registers for every D the contract admits
// (D <= 4096 = 8 chunks of 8 elements per lane), the sum of squares in fp32, reduced across the wave with shuffles.
//   forward : x (R,D) bf16|f32 -> y bf16 (R,D), rnorm f32 (R) = 1 / max(||x||, 1e-12)        reads 2|4 B, writes 2 B per element
//   backward: g bf16, x, rnorm -> dx bf16 = t*rnorm*(g - xh*(xh.g)), xh = x*rnorm;  rows at the clamp: dx = t*rnorm*g
#include "dgx_common.h"

#define L2N_EPS 1e-12f
#define L2N_WAVES 4

// NJ = ceil(D / 512) chunks of 8 elements per lane.  Lanes beyond the row's last chunk load that last chunk again (a clamped
// index keeps the loads unpredicated and in flight together) and contribute zero.
template <typename XT, int NJ>
__global__ __launch_bounds__(64 * L2N_WAVES) void l2n_fwd_kernel(const XT* __restrict__ x, uint16_t* __restrict__ y,
                                                                 float* __restrict__ rnorm, int64_t R, int D, float t) {
    const int lane = threadIdx.x & 63;
    const int nc = D >> 3;
    for (int64_t row = (int64_t)blockIdx.x * L2N_WAVES + (threadIdx.x >> 6); row < R; row += (int64_t)gridDim.x * L2N_WAVES) {
        const XT* xr = x + row * D;
        float v[NJ][8];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
            ld8(xr + 8 * (c < nc ? c : nc - 1), v[j]);
        }
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (lane + 64 * j >= nc) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
            }
            ss += ((v[j][0] * v[j][0] + v[j][1] * v[j][1]) + (v[j][2] * v[j][2] + v[j][3] * v[j][3])) +
                  ((v[j][4] * v[j][4] + v[j][5] * v[j][5]) + (v[j][6] * v[j][6] + v[j][7] * v[j][7]));
        }
        const float rn = 1.0f / fmaxf(sqrtf(wave_sum(ss)), L2N_EPS);
        if (lane == 0) rnorm[row] = rn;
        const float s = t * rn;
        uint16_t* yr = y + row * D;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
            if (c < nc) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = v[j][e] * s;
                st8(yr + 8 * c, o);
            }
        }
    }
}

// A row is "at the clamp" when its saved rnorm is the forward's 1 / 1e-12 itself: max(||x||, eps) took eps, the scale is a
// constant there and only t * rnorm * g remains (torch's clamp_min backward).
template <typename XT, int NJ>
__global__ __launch_bounds__(64 * L2N_WAVES) void l2n_bwd_kernel(const uint16_t* __restrict__ g, const XT* __restrict__ x,
                                                                 const float* __restrict__ rnorm, uint16_t* __restrict__ dx,
                                                                 int64_t R, int D, float t) {
    const int lane = threadIdx.x & 63;
    const int nc = D >> 3;
    for (int64_t row = (int64_t)blockIdx.x * L2N_WAVES + (threadIdx.x >> 6); row < R; row += (int64_t)gridDim.x * L2N_WAVES) {
        const XT* xr = x + row * D;
        const uint16_t* gr = g + row * D;
        float v[NJ][8], gv[NJ][8];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j, ci = c < nc ? c : nc - 1;
            ld8(xr + 8 * (ci), v[j]);
            ld8(gr + 8 * (ci), gv[j]);
        }
        const float rn = rnorm[row];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (lane + 64 * j >= nc) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
            }
            dot += ((v[j][0] * gv[j][0] + v[j][1] * gv[j][1]) + (v[j][2] * gv[j][2] + v[j][3] * gv[j][3])) +
                   ((v[j][4] * gv[j][4] + v[j][5] * gv[j][5]) + (v[j][6] * gv[j][6] + v[j][7] * gv[j][7]));
        }
        const bool clamped = rn >= 1.0f / L2N_EPS;
        // xh . g = rn * dot;  dx = t*rn*(g - x*rn*(xh . g)) = s*g - x*(s*rn*rn*dot)
        const float s = t * rn;
        const float k = clamped ? 0.f : s * rn * (rn * wave_sum(dot));
        uint16_t* dr = dx + row * D;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
            if (c < nc) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = s * gv[j][e] - v[j][e] * k;
                st8(dr + 8 * c, o);
            }
        }
    }
}

static inline bool l2n_dim_ok(int D) { return D >= 8 && D <= 4096 && (D & 7) == 0; }
static inline int l2n_grid(int64_t R) {
    const int64_t b = (R + L2N_WAVES - 1) / L2N_WAVES;
    return (int)(b < 65536 ? b : 65536);
}

#define L2N_DISPATCH(KERNEL, XT, ...)                                                                                      \
    do {                                                                                                                   \
        const int nj = (D + 511) / 512;                                                                                    \
        const dim3 grid(l2n_grid(R)), block(64 * L2N_WAVES);                                                               \
        if (nj <= 1) hipLaunchKernelGGL((KERNEL<XT, 1>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);                \
        else if (nj <= 2) hipLaunchKernelGGL((KERNEL<XT, 2>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);           \
        else if (nj <= 4) hipLaunchKernelGGL((KERNEL<XT, 4>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);           \
        else hipLaunchKernelGGL((KERNEL<XT, 8>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);                        \
    } while (0)

extern "C" int dgx_l2norm_rows_fwd(const void* x, void* y_bf16, float* rnorm, int64_t R, int D, float t, int x_dtype,
                                   void* stream) {
    if (!l2n_dim_ok(D) || (x_dtype != DGX_F32 && x_dtype != DGX_BF16)) return DGX_ERR_UNSUPPORTED;
    if (R <= 0) return DGX_OK;
    if (!x || !y_bf16 || !rnorm) return DGX_ERR_BAD_ARG;
    if (x_dtype == DGX_BF16) L2N_DISPATCH(l2n_fwd_kernel, uint16_t, (const uint16_t*)x, (uint16_t*)y_bf16, rnorm, R, D, t);
    else L2N_DISPATCH(l2n_fwd_kernel, float, (const float*)x, (uint16_t*)y_bf16, rnorm, R, D, t);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_l2norm_rows_bwd(const void* g_bf16, const void* x, const float* rnorm, void* dx_bf16, int64_t R, int D,
                                   float t, int x_dtype, void* stream) {
    if (!l2n_dim_ok(D) || (x_dtype != DGX_F32 && x_dtype != DGX_BF16)) return DGX_ERR_UNSUPPORTED;
    if (R <= 0) return DGX_OK;
    if (!g_bf16 || !x || !rnorm || !dx_bf16) return DGX_ERR_BAD_ARG;
    if (x_dtype == DGX_BF16)
        L2N_DISPATCH(l2n_bwd_kernel, uint16_t, (const uint16_t*)g_bf16, (const uint16_t*)x, rnorm, (uint16_t*)dx_bf16, R, D, t);
    else
        L2N_DISPATCH(l2n_bwd_kernel, float, (const uint16_t*)g_bf16, (const float*)x, rnorm, (uint16_t*)dx_bf16, R, D, t);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
