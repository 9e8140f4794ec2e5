// The caption loss of an image-labelled step on the device (DG/divergen/modeling/roi_heads/detic_fast_rcnn.py:469-506 `_caption_loss`
// inside :342-434 `image_label_losses`, with the caption half of `forward` :452-458 and of zero_shot_classifier.py:73-87): per image
// the LAST valid row of the projected box features (the image box), L2-normalised and scaled by NORM_TEMP, its N dot products with the
// caption rows, BCE-with-logits against the one-hot of the image's own caption.  The n x N caption scores are never formed.
//   caption_prepare_kernel  one wave per caption row: (N, ld) fp32 [rank column cut] -> (N, D) rows divided by max(|c|, 1e-12)
//   caption_fwd_kernel      grid (block of 64 caption columns, image): last valid row, normalise, dots, BCE; leaves the logit
//                           gradients w_j (sigmoid(s_j) - t_j) * scale and the block's loss / gradient sums
//   caption_fold_kernel     one wave: column blocks and images in order -> out4, the sum of all logit gradients
//   caption_bwd_kernel      blocks [0, B): the gradient of image b's chosen row through the normalisation; blocks [B, ..): exact zeros
//                           in every other 16-byte chunk of the (R_alloc, ld) gradient.  One launch, no memset, no scatter.
// A small latency-bound kernel family (as wsddn_loss.hip): no MFMA.  All arithmetic is fp32 from the stored inputs; no floating-point
// atomics; every sum has a fixed order: two runs give the same bits.
#include "dgx_common.h"

#define CAP_MAX_IMAGES 32
struct CapImages {
    int B;
    int row0[CAP_MAX_IMAGES + 1];   // rows of image b: [row0[b], row0[b+1])
};

namespace {
constexpr int CAP_CB = 64;          // caption columns of one forward block
constexpr int CAP_THREADS = 256;
constexpr int CAP_WAVES = CAP_THREADS / 64;
constexpr int CAP_MAX_D = 4096;
constexpr float CAP_EPS = 1e-12f;   // F.normalize's eps

// sum over the block, in every thread: the wave butterfly, then the waves in order
__device__ __forceinline__ float cap_block_sum(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = sh[0];
#pragma unroll
    for (int k = 1; k < CAP_WAVES; ++k) s += sh[k];
    return s;
}

// the last row of [0, n) whose validity byte is set (every row when valid == NULL), -1 = none; wave-uniform
__device__ __forceinline__ int cap_last_valid(const uint8_t* valid, int r0, int n) {
    if (!valid) return n - 1;
    const int lane = threadIdx.x & 63;
    for (int base = n - 1; base >= 0; base -= 64) {
        const int r = base - lane;
        const unsigned long long m = __ballot(r >= 0 && valid[r0 + r] != 0);
        if (m) return base - (__ffsll((long long)m) - 1);
    }
    return -1;
}

// row[0, D) as fp32 into LDS (16-byte loads: the caller checked the alignment)
template <typename T> __device__ __forceinline__ void cap_load_row(const T* row, int D, float* dst) {
    for (int c = threadIdx.x * 8; c < D; c += CAP_THREADS * 8) {
        float v[8];
        ld8(row + c, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[c + k] = v[k];
    }
}
}  // namespace

__global__ __launch_bounds__(CAP_THREADS) void caption_prepare_kernel(const float* __restrict__ cap, int64_t ld, int N, int D,
                                                                      int norm_weight, float* __restrict__ out, bool vec) {
    const int row = blockIdx.x * CAP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* c = cap + (int64_t)row * ld;
    float* o = out + (int64_t)row * D;
    float ss = 0.0f;
    if (norm_weight) {
        if (vec)
            for (int q = lane; q < D / 4; q += 64) {
                const float4 v = reinterpret_cast<const float4*>(c)[q];
                ss += v.x * v.x; ss += v.y * v.y; ss += v.z * v.z; ss += v.w * v.w;
            }
        else
            for (int d = lane; d < D; d += 64) ss += c[d] * c[d];
        ss = wave_sum(ss);
    }
    const float nrm = fmaxf(sqrtf(ss), CAP_EPS);
    if (vec)
        for (int q = lane; q < D / 4; q += 64) {
            float4 v = reinterpret_cast<const float4*>(c)[q];
            if (norm_weight) { v.x /= nrm; v.y /= nrm; v.z /= nrm; v.w /= nrm; }
            reinterpret_cast<float4*>(o)[q] = v;
        }
    else
        for (int d = lane; d < D; d += 64) o[d] = norm_weight ? c[d] / nrm : c[d];
}

// ws: g (B, N) | lpart (B, ncb) | gpart (B, ncb) | norm (B) | gsum (1)
template <typename T>
__global__ __launch_bounds__(CAP_THREADS) void caption_fwd_kernel(const T* __restrict__ u, int64_t ldu, const uint8_t* __restrict__ valid,
                                                                  CapImages P, const float* __restrict__ cap, int N, int D, int target0,
                                                                  float temp, int norm_weight, const float* __restrict__ cls_bias,
                                                                  float neg_weight, float scale, int32_t* __restrict__ sel,
                                                                  float* __restrict__ ws) {
    __shared__ float h[CAP_MAX_D];
    __shared__ float sh[CAP_WAVES], shl[CAP_WAVES], shg[CAP_WAVES];
    const int b = blockIdx.y, cb = blockIdx.x, ncb = gridDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r0 = P.row0[b], n = P.row0[b + 1] - r0;
    const int j0 = cb * CAP_CB, j1 = min(N, j0 + CAP_CB);
    float* g = ws + (int64_t)b * N;
    float* lpart = ws + (int64_t)P.B * N;
    float* gpart = lpart + (int64_t)P.B * ncb;
    float* norms = gpart + (int64_t)P.B * ncb;
    const int pick = cap_last_valid(valid, r0, n);
    if (cb == 0 && tid == 0) sel[b] = pick;
    if (pick < 0) {                                   // no surviving row: the image contributes nothing (and still counts in B)
        for (int j = j0 + tid; j < j1; j += CAP_THREADS) g[j] = 0.0f;
        if (tid == 0) {
            lpart[b * ncb + cb] = 0.0f; gpart[b * ncb + cb] = 0.0f;
            if (cb == 0) norms[b] = 0.0f;
        }
        return;
    }
    cap_load_row<T>(u + (int64_t)(r0 + pick) * ldu, D, h);
    __syncthreads();
    if (norm_weight) {
        float ss = 0.0f;
        for (int d = tid; d < D; d += CAP_THREADS) ss += h[d] * h[d];
        const float nrm = sqrtf(cap_block_sum(ss, sh));
        if (cb == 0 && tid == 0) norms[b] = nrm;
        const float den = fmaxf(nrm, CAP_EPS);
        for (int d = tid; d < D; d += CAP_THREADS) h[d] = temp * (h[d] / den);      // each thread rewrites what it read
        __syncthreads();
    } else if (cb == 0 && tid == 0) {
        norms[b] = 0.0f;
    }
    const float bias = cls_bias ? cls_bias[0] : 0.0f;
    const int pos = target0 + b;
    float lsum = 0.0f, gsum = 0.0f;                   // lane 0 of each wave: its columns in ascending order
    for (int j = j0 + wave; j < j1; j += CAP_WAVES) {
        const float4* c = reinterpret_cast<const float4*>(cap + (int64_t)j * D);
        float acc = 0.0f;
        for (int q = lane; q < D / 4; q += 64) {
            const float4 v = c[q];
            acc += h[4 * q] * v.x; acc += h[4 * q + 1] * v.y; acc += h[4 * q + 2] * v.z; acc += h[4 * q + 3] * v.w;
        }
        const float s = wave_sum(acc) + bias;
        if (lane == 0) {
            // F.binary_cross_entropy_with_logits: max(s, 0) - s t + log1p(exp(-|s|)); its derivative sigmoid(s) - t, the positive's formed
            // as -sigmoid(-s): no cancellation at a saturated logit
            const float e = expf(-fabsf(s));
            const float soft = log1pf(e);
            const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
            const bool is_pos = j == pos;
            const float w = is_pos ? 1.0f : neg_weight;
            const float l = fmaxf(s, 0.0f) - (is_pos ? s : 0.0f) + soft;
            const float dg = is_pos ? -(s >= 0.0f ? small : big) : (s >= 0.0f ? big : small);
            const float gj = scale * (w * dg);
            g[j] = gj;
            lsum += w * l;
            gsum += gj;
        }
    }
    if (lane == 0) { shl[wave] = lsum; shg[wave] = gsum; }
    __syncthreads();
    if (tid == 0) {
        float l = shl[0], gg = shg[0];
        for (int k = 1; k < CAP_WAVES; ++k) { l += shl[k]; gg += shg[k]; }
        lpart[b * ncb + cb] = l;
        gpart[b * ncb + cb] = gg;
    }
}

// out4 = {image_loss part (scale applied), stats_l_caption (stat_scale applied), 0, 0}; ws gsum = the sum of all logit gradients
__global__ __launch_bounds__(64) void caption_fold_kernel(int B, int N, int ncb, float scale, float stat_scale, float* __restrict__ ws,
                                                          float* __restrict__ out4) {
    __shared__ float pl[CAP_MAX_IMAGES], pg[CAP_MAX_IMAGES];
    const float* lpart = ws + (int64_t)B * N;
    const float* gpart = lpart + (int64_t)B * ncb;
    const int i = threadIdx.x;
    if (i < B) {
        float l = 0.0f, g = 0.0f;
        for (int c = 0; c < ncb; ++c) { l += lpart[i * ncb + c]; g += gpart[i * ncb + c]; }
        pl[i] = l; pg[i] = g;
    }
    __syncthreads();
    if (i != 0) return;
    float l = 0.0f, g = 0.0f;
    for (int b = 0; b < B; ++b) { l += pl[b]; g += pg[b]; }
    out4[0] = l * scale;
    out4[1] = l * stat_scale;
    out4[2] = 0.0f;
    out4[3] = 0.0f;
    ws[(int64_t)B * N + 2 * (int64_t)B * ncb + B] = g;
}

template <typename T>
__global__ __launch_bounds__(CAP_THREADS) void caption_bwd_kernel(const T* __restrict__ u, int64_t ldu, CapImages P,
                                                                  const float* __restrict__ cap, int N, int D, float temp, int norm_weight,
                                                                  const int32_t* __restrict__ sel, const float* __restrict__ ws, int ncb,
                                                                  const float* __restrict__ upstream, T* __restrict__ du, int64_t ldg,
                                                                  int64_t R_alloc, float* __restrict__ dbias) {
    constexpr int E = 16 / (int)sizeof(T);            // elements of one 16-byte chunk
    __shared__ float uf[CAP_MAX_D], dh[CAP_MAX_D], part[CAP_MAX_D];
    __shared__ float sh[CAP_WAVES];
    __shared__ int chosen[CAP_MAX_IMAGES];
    const int tid = threadIdx.x, B = P.B;
    const float up = upstream ? upstream[0] : 1.0f;
    if ((int)blockIdx.x >= B) {
        // ---- exact zeros in every 16-byte chunk outside the chosen rows (pad rows and pad columns included)
        if (tid < CAP_MAX_IMAGES) {
            int r = -1;
            if (tid < B) {
                const int s = sel[tid], n = P.row0[tid + 1] - P.row0[tid];
                if (s >= 0 && s < n) r = P.row0[tid] + s;
            }
            chosen[tid] = r;
        }
        __syncthreads();
        const int64_t cpr = ldg / E, total = R_alloc * cpr;
        const int64_t stride = (int64_t)(gridDim.x - B) * CAP_THREADS;
        for (int64_t i = (int64_t)(blockIdx.x - B) * CAP_THREADS + tid; i < total; i += stride) {
            const int row = (int)(i / cpr);
            bool skip = false;
            for (int b = 0; b < B; ++b) skip |= chosen[b] == row;
            if (!skip) reinterpret_cast<uint4*>(du)[i] = make_uint4(0u, 0u, 0u, 0u);
        }
        return;
    }
    const int b = blockIdx.x;
    if (b == 0 && tid == 0 && dbias) dbias[0] = up * ws[(int64_t)B * N + 2 * (int64_t)B * ncb + B];
    const int r0 = P.row0[b], n = P.row0[b + 1] - r0, pick = sel[b];
    if (pick < 0 || pick >= n) return;                // (block-uniform) no chosen row: the zero blocks write the image's rows
    const float* g = ws + (int64_t)b * N;
    cap_load_row<T>(u + (int64_t)(r0 + pick) * ldu, D, uf);
    // ---- dh = sum_j g_j c_j: work item (q, js) = chunk q of the columns j = js, js + JS, ..; the JS partial sums meet in LDS in order
    const int Q = D / 4, JS = Q >= CAP_THREADS ? 1 : CAP_THREADS / Q;
    for (int w = tid; w < Q * JS; w += CAP_THREADS) {
        const int q = w % Q, js = w / Q;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = js; j < N; j += JS) {
            const float gj = g[j];
            const float4 v = reinterpret_cast<const float4*>(cap + (int64_t)j * D)[q];
            acc.x += gj * v.x; acc.y += gj * v.y; acc.z += gj * v.z; acc.w += gj * v.w;
        }
        float* p = part + js * D + 4 * q;
        p[0] = acc.x; p[1] = acc.y; p[2] = acc.z; p[3] = acc.w;
    }
    __syncthreads();
    for (int d = tid; d < D; d += CAP_THREADS) {
        float s = part[d];
        for (int js = 1; js < JS; ++js) s += part[js * D + d];
        dh[d] = s;
    }
    __syncthreads();
    // ---- through h = temp u / max(|u|, eps) (F.normalize): |u| > eps: temp (dh - uhat (uhat . dh)) / |u|, otherwise temp dh / eps
    float mul = up, dot = 0.0f, rn = 0.0f;
    bool proj = false;
    if (norm_weight) {
        float ss = 0.0f;
        for (int d = tid; d < D; d += CAP_THREADS) ss += uf[d] * uf[d];
        const float nrm = sqrtf(cap_block_sum(ss, sh));
        if (nrm > CAP_EPS) {
            proj = true;
            rn = 1.0f / nrm;
            float pd = 0.0f;
            for (int d = tid; d < D; d += CAP_THREADS) pd += (uf[d] * rn) * dh[d];
            dot = cap_block_sum(pd, sh);
            mul = up * temp * rn;
        } else {
            mul = up * temp / CAP_EPS;
        }
    }
    T* row = du + (int64_t)(r0 + pick) * ldg;
    for (int c = tid * 8; c < ldg; c += CAP_THREADS * 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int d = c + k;
            v[k] = d < D ? mul * (proj ? dh[d] - (uf[d] * rn) * dot : dh[d]) : 0.0f;
        }
        st8(row + c, v);
    }
}

static inline int cap_ncb(int N) { return (N + CAP_CB - 1) / CAP_CB; }
static inline bool cap_al16(const void* p, int64_t ld, size_t es) { return p && ((uintptr_t)p % 16 == 0) && ((ld * (int64_t)es) % 16 == 0); }

extern "C" int dgx_caption_prepare(const float* cap, int64_t ld_cap, int N, int D, int norm_weight, float* out, void* stream) {
    if (!cap || !out || N <= 0 || D < 8 || D > CAP_MAX_D || D % 8 || ld_cap < D || ((uintptr_t)out % 16)) return DGX_ERR_BAD_ARG;
    hipLaunchKernelGGL(caption_prepare_kernel, dim3((N + CAP_WAVES - 1) / CAP_WAVES), dim3(CAP_THREADS), 0, (hipStream_t)stream, cap, ld_cap,
                       N, D, norm_weight, out, cap_al16(cap, ld_cap, 4));
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int64_t dgx_caption_workspace_floats(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return (int64_t)B * N + 2 * (int64_t)B * cap_ncb(N) + B + 1;
}

extern "C" int dgx_caption_loss(const void* u, int64_t ld_u, int64_t R_alloc, const uint8_t* valid, int B, const int* row0,
                                const float* cap, int N, int D, int target0, float temp, int norm_weight, const float* cls_bias,
                                float neg_weight, float scale, float stat_scale, const float* upstream, int32_t* sel, float* out4,
                                float* ws, void* du, int64_t ld_du, float* dbias, int dtype, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const size_t es = dtype == DGX_BF16 ? 2 : 4;
    if (!u || !row0 || !cap || !sel || !ws || (!du && !out4) || (dtype != DGX_F32 && dtype != DGX_BF16)) return DGX_ERR_BAD_ARG;
    if (B <= 0 || B > CAP_MAX_IMAGES || D < 8 || D > CAP_MAX_D || D % 8 || N <= 0 || target0 < 0 || (int64_t)target0 + B > N)
        return DGX_ERR_BAD_ARG;
    if (ld_u < D || !cap_al16(u, ld_u, es) || ((uintptr_t)cap % 16)) return DGX_ERR_BAD_ARG;
    if (du && (ld_du < D || ld_du % 8 || !cap_al16(du, ld_du, es))) return DGX_ERR_BAD_ARG;
    CapImages P;
    P.B = B;
    if (row0[0] != 0) return DGX_ERR_BAD_ARG;
    for (int i = 0; i <= B; ++i) {
        P.row0[i] = row0[i];
        if (i > 0 && row0[i] < row0[i - 1]) return DGX_ERR_BAD_ARG;
    }
    if (row0[B] > R_alloc) return DGX_ERR_BAD_ARG;   // every image row lies inside the (R_alloc, ld) allocations of u and du
    const int ncb = cap_ncb(N);
#define CAP_LAUNCH(T)                                                                                                                  \
    do {                                                                                                                               \
        if (!du) {                                                                                                                     \
            hipLaunchKernelGGL(caption_fwd_kernel<T>, dim3(ncb, B), dim3(CAP_THREADS), 0, st, (const T*)u, ld_u, valid, P, cap, N, D,  \
                               target0, temp, norm_weight, cls_bias, neg_weight, scale, sel, ws);                                      \
            hipLaunchKernelGGL(caption_fold_kernel, dim3(1), dim3(64), 0, st, B, N, ncb, scale, stat_scale, ws, out4);                 \
        } else {                                                                                                                       \
            const int64_t chunks = R_alloc * (ld_du / (int64_t)(16 / es));                                                             \
            int zb = (int)((chunks + CAP_THREADS * 4 - 1) / (CAP_THREADS * 4));                                                        \
            zb = zb < 1 ? 1 : (zb > 1024 ? 1024 : zb);                                                                                 \
            hipLaunchKernelGGL(caption_bwd_kernel<T>, dim3(B + zb), dim3(CAP_THREADS), 0, st, (const T*)u, ld_u, P, cap, N, D, temp,   \
                               norm_weight, sel, ws, ncb, upstream, (T*)du, ld_du, R_alloc, dbias);                                    \
        }                                                                                                                              \
    } while (0)
    if (dtype == DGX_BF16) CAP_LAUNCH(uint16_t);
    else CAP_LAUNCH(float);
#undef CAP_LAUNCH
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
