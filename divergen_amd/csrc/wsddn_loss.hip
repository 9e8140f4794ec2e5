// The WSDDN image-label loss on the device (DG/divergen/modeling/roi_heads/detic_fast_rcnn.py:509-521 `_wsddn_loss` inside
// :342-434 `image_label_losses`): per image a softmax over its proposals, taken per class column, times the sigmoid class scores,
// summed to one score per class; the BCE of those scores against the one-hot of every label of the image.
//   wsddn_stats_kernel  grid (column block, image): threads own 16-byte column chunks and split the rows; the row splits meet in
//                       LDS with the (max, denominator, numerator, complement) merge.  Leaves max / denominator / S per (image, column), the
//                       block's all-negative BCE sum, and the arg-max row of every label whose column the block owns.
//   wsddn_fold_kernel   one workgroup: column blocks, labels and images in order -> out8.
//   wsddn_grad_kernel   grid (column block, image): one pass over logits and proposal scores, both dense gradients.
// All arithmetic is fp32 from the stored inputs; no floating-point atomics; every sum has a fixed order: two runs give the same bits.
// sigma and S are rounded to fp32 where the reference stores them (score.sigmoid(), the clamped img_score): 1 - sigma and 1 - S are
// formed from the rounded values, as torch's backward formulas do, so a score that saturates to 1.0f has the reference's gradient.
#include "dgx_common.h"
#include "row_chunk.h"

#define WS_MAX_IMAGES 32
struct WSImages {
    int B;
    int row0[WS_MAX_IMAGES + 1];   // rows of image b: [row0[b], row0[b+1])
    float H[WS_MAX_IMAGES], W[WS_MAX_IMAGES];
};

namespace {
constexpr int WS_CB = 64;          // columns of one block
constexpr int WS_THREADS = 256;

__device__ __forceinline__ float ws_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}
// torch.clamp(S, 1e-10, 1 - 1e-10) on an fp32 tensor: the bounds round to 1e-10f and exactly 1.0f
__device__ __forceinline__ float ws_clamp(float s) { return fminf(fmaxf(s, 1e-10f), 1.0f); }
__device__ __forceinline__ bool ws_inside(float s) { return s >= 1e-10f && s <= 1.0f; }
// F.binary_cross_entropy: logs clamped below at -100
__device__ __forceinline__ float ws_bce0(float sc) { return -fmaxf(logf(1.0f - sc), -100.0f); }
__device__ __forceinline__ float ws_bce1(float sc) { return -fmaxf(logf(sc), -100.0f); }

// (m, d, n, nc) += one row: d = sum exp(p - m), n = sum sigmoid(s) exp(p - m), nc = sum sigmoid(-s) exp(p - m).  The complement is
// carried so that an image score near 1 is formed as 1 - nc / d: its distance from 1 is what the BCE and its gradient divide by
__device__ __forceinline__ void ws_push(float& m, float& d, float& n, float& nc, float p, float s) {
    const float mn = fmaxf(m, p);
    if (mn == -INFINITY) return;
    const float a = expf(m - mn), b = expf(p - mn);
    const float e = expf(-fabsf(s));
    const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
    d = d * a + b;
    n = n * a + (s >= 0.0f ? big : small) * b;
    nc = nc * a + (s >= 0.0f ? small : big) * b;
    m = mn;
}

// block-wide arg-max of (key, idx): the largest key, the lowest idx among equal keys (torch.argmax); idx = INT_MAX = no entry
__device__ __forceinline__ int ws_block_argmax(float key, int idx, float* shf, int* shi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ok = __shfl_xor(key, o);
        const int oi = __shfl_xor(idx, o);
        if (oi != 0x7fffffff && (idx == 0x7fffffff || ok > key || (ok == key && oi < idx))) { key = ok; idx = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shf[threadIdx.x >> 6] = key; shi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    key = shf[0]; idx = shi[0];
#pragma unroll
    for (int k = 1; k < WS_THREADS / 64; ++k) {
        const float ok = shf[k];
        const int oi = shi[k];
        if (oi != 0x7fffffff && (idx == 0x7fffffff || ok > key || (ok == key && oi < idx))) { key = ok; idx = oi; }
    }
    return idx;
}
}  // namespace

// ws: stats (B, 3, C1) = {column maximum, softmax denominator, unclamped S}, then (B, ncb) all-negative BCE sums of the blocks
template <typename T>
__global__ __launch_bounds__(WS_THREADS) void wsddn_stats_kernel(const T* __restrict__ logits, int64_t ldl, const T* __restrict__ prop,
                                                                 int64_t ldp, const uint8_t* __restrict__ valid, WSImages P,
                                                                 const int32_t* __restrict__ label_off, const int32_t* __restrict__ labels,
                                                                 int C1, int32_t* __restrict__ sel_out, float* __restrict__ ws, bool vec_l,
                                                                 bool vec_p) {
    constexpr int N = Chunk<T>::N, TX = WS_CB / N, TY = WS_THREADS / TX;
    __shared__ float sh[4][TY][WS_CB];
    __shared__ float colm[WS_CB], cold[WS_CB];
    __shared__ float shf[WS_THREADS / 64];
    __shared__ int shi[WS_THREADS / 64];
    const int i = blockIdx.y, tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const int c0 = blockIdx.x * WS_CB, c = c0 + tx * N, ncb = gridDim.x;
    const int r0 = P.row0[i], n = P.row0[i + 1] - r0;
    const T* x = logits + (int64_t)r0 * ldl;
    const T* q = prop + (int64_t)r0 * ldp;
    float m[N], d[N], a[N], ac[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { m[k] = -INFINITY; d[k] = 0.0f; a[k] = 0.0f; ac[k] = 0.0f; }
    if (c < C1) {
        for (int r = ty; r < n; r += TY) {
            if (valid && !valid[r0 + r]) continue;
            float s[N], p[N];
            load_chunk<T>(x + (int64_t)r * ldl, c, vec_l, (int)ldl, s);
            load_chunk<T>(q + (int64_t)r * ldp, c, vec_p, (int)ldp, p);
#pragma unroll
            for (int k = 0; k < N; ++k)
                if (c + k < C1) ws_push(m[k], d[k], a[k], ac[k], p[k], s[k]);      // (a select: the pad columns may hold NaN)
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sh[0][ty][tx * N + k] = m[k]; sh[1][ty][tx * N + k] = d[k]; sh[2][ty][tx * N + k] = a[k]; sh[3][ty][tx * N + k] = ac[k];
    }
    __syncthreads();
    // ---- one thread per column: the row splits in order
    float neg = 0.0f;
    if (tid < WS_CB) {
        float M = -INFINITY;
        for (int y = 0; y < TY; ++y) M = fmaxf(M, sh[0][y][tid]);
        float D = 0.0f, A = 0.0f, AC = 0.0f;
        if (M != -INFINITY)
            for (int y = 0; y < TY; ++y) {
                const float my = sh[0][y][tid];
                if (my == -INFINITY) continue;
                const float e = expf(my - M);
                D += sh[1][y][tid] * e;
                A += sh[2][y][tid] * e;
                AC += sh[3][y][tid] * e;
            }
        const float S = D > 0.0f ? (A >= 0.5f * D ? 1.0f - AC / D : A / D) : 0.0f;
        colm[tid] = M;
        cold[tid] = D;
        if (c0 + tid < C1) {
            float* st = ws + (int64_t)i * 3 * C1;
            st[c0 + tid] = M;
            st[C1 + c0 + tid] = D;
            st[2 * C1 + c0 + tid] = S;
            if (D > 0.0f) neg = ws_bce0(ws_clamp(S));
        }
    }
    if (tid < 64) {                                   // WS_CB = one wave: a fixed shuffle tree
        neg = wave_sum(neg);
        if (tid == 0) ws[(int64_t)P.B * 3 * C1 + (int64_t)i * ncb + blockIdx.x] = neg;
    }
    __syncthreads();
    // ---- the arg-max row of every label whose column this block owns: sigmoid(s_rl) exp(p_rl - max), the common denominator left out
    const int l0 = label_off[i], L = label_off[i + 1] - l0;
    for (int j = 0; j < L; ++j) {
        const int lab = labels[l0 + j];
        if (lab < 0 || lab >= C1) {
            if (blockIdx.x == 0 && tid == 0) sel_out[l0 + j] = -1;
            continue;
        }
        if (lab < c0 || lab >= c0 + WS_CB) continue;
        const float M = colm[lab - c0];
        float key = -INFINITY;
        int idx = 0x7fffffff;
        if (cold[lab - c0] > 0.0f)
            for (int r = tid; r < n; r += WS_THREADS) {
                if (valid && !valid[r0 + r]) continue;
                const float k = ws_sigmoid(il_ld1<T>(x + (int64_t)r * ldl + lab)) * expf(il_ld1<T>(q + (int64_t)r * ldp + lab) - M);
                if (idx == 0x7fffffff || k > key) { key = k; idx = r; }      // rows ascend: the first maximum stays
            }
        const int pick = ws_block_argmax(key, idx, shf, shi);
        if (tid == 0) sel_out[l0 + j] = pick == 0x7fffffff ? -1 : pick;
    }
}

// out8 = {image_loss (weighted), stats_l_image, pool_stats, stats_select_size, stats_select_x, stats_select_y,
//         stats_max_label_score, -}: thread i folds image i (column blocks, then labels, in order), thread 0 the images in order
template <typename T>
__global__ __launch_bounds__(64) void wsddn_fold_kernel(const T* __restrict__ logits, int64_t ldl, const float* __restrict__ boxes,
                                                        WSImages P, const int32_t* __restrict__ label_off,
                                                        const int32_t* __restrict__ labels, int C1, int ncb, float weight,
                                                        const int32_t* __restrict__ sel, const float* __restrict__ ws,
                                                        float* __restrict__ out8) {
    __shared__ float part[WS_MAX_IMAGES];
    const int i = threadIdx.x, B = P.B;
    if (i < B) {
        const float* st = ws + (int64_t)i * 3 * C1;
        const int l0 = label_off[i], L = label_off[i + 1] - l0;
        float v = 0.0f;
        if (L > 0 && st[C1] > 0.0f) {                // st[C1]: the denominator of column 0 -- zero when the image has no valid row
            float neg = 0.0f;
            for (int b = 0; b < ncb; ++b) neg += ws[(int64_t)B * 3 * C1 + (int64_t)i * ncb + b];
            float acc = 0.0f;
            for (int j = 0; j < L; ++j) {
                const int lab = labels[l0 + j];
                if (lab < 0 || lab >= C1) continue;
                const float sc = ws_clamp(st[2 * C1 + lab]);
                acc += (neg - ws_bce0(sc) + ws_bce1(sc)) / (float)C1;
            }
            v = acc / (float)L;
        }
        part[i] = v;
    }
    __syncthreads();
    if (i != 0) return;
    float s = 0.0f;
    for (int b = 0; b < B; ++b) s += part[b];
    const float l = s / (float)B;
    out8[0] = l * weight;
    out8[1] = l;
    float stt[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = B - 1, found = 0; b >= 0 && !found; --b)
        for (int j = label_off[b + 1] - 1; j >= label_off[b]; --j) {
            const int pick = sel[j];
            if (pick < 0) continue;
            const int r = P.row0[b] + pick;
            const float* bx = boxes + 4 * (int64_t)r;
            stt[0] = (float)pick;                                                            // pool_stats
            stt[1] = (bx[2] - bx[0]) * (bx[3] - bx[1]) / (P.H[b] * P.W[b]);                  // stats_select_size
            stt[2] = (bx[0] + bx[2]) / 2.0f / P.W[b];                                        // stats_select_x
            stt[3] = (bx[1] + bx[3]) / 2.0f / P.H[b];                                        // stats_select_y
            stt[4] = ws_sigmoid(il_ld1<T>(logits + (int64_t)r * ldl + labels[j]));           // stats_max_label_score
            found = 1;
            break;
        }
    for (int k = 0; k < 5; ++k) out8[2 + k] = stt[k];
    out8[7] = 0.0f;
}

// dlogits[r,c] = K G_c p_rc sigma_rc (1 - sigma_rc),  dprop[r,c] = K G_c p_rc (sigma_rc - S_c),  p_rc = exp(prop_rc - max_c) / den_c,
// G_c = sum over the image's labels of (S_c - [c == label]) / max((1 - S_c) S_c, 1e-12) where lo <= S_c <= hi, else 0,
// K = weight / (B L (C+1)) * upstream.  Every element of the image's rows is written: zeros in invalid rows and pad columns.
template <typename T>
__global__ __launch_bounds__(WS_THREADS) void wsddn_grad_kernel(const T* __restrict__ logits, int64_t ldl, const T* __restrict__ prop,
                                                                int64_t ldp, const uint8_t* __restrict__ valid, WSImages P,
                                                                const int32_t* __restrict__ label_off, const int32_t* __restrict__ labels,
                                                                int C1, float weight, const float* __restrict__ stats,
                                                                const float* __restrict__ upstream, T* __restrict__ dlogits, int64_t ldgl,
                                                                T* __restrict__ dprop, int64_t ldgp, bool vec_l, bool vec_p, bool vec_gl,
                                                                bool vec_gp) {
    constexpr int N = Chunk<T>::N, TX = WS_CB / N, TY = WS_THREADS / TX;
    __shared__ float colm[WS_CB], colr[WS_CB], cols[WS_CB], colg[WS_CB];      // maximum, 1 / denominator, S, K G
    const int i = blockIdx.y, tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const int c0 = blockIdx.x * WS_CB, c = c0 + tx * N;
    const int r0 = P.row0[i], n = P.row0[i + 1] - r0;
    const int l0 = label_off[i], L = label_off[i + 1] - l0;
    if (tid < WS_CB) {
        const int cc = c0 + tid;
        float M = 0.0f, rD = 0.0f, S = 0.0f, G = 0.0f;
        if (cc < C1) {
            const float* st = stats + (int64_t)i * 3 * C1;
            const float D = st[C1 + cc];
            if (D > 0.0f && L > 0) {
                M = st[cc]; rD = 1.0f / D; S = st[2 * C1 + cc];
                int cnt = 0, hit = 0;                // labels that add a term; those that name this column
                for (int j = 0; j < L; ++j) {
                    const int lab = labels[l0 + j];
                    cnt += (lab >= 0 && lab < C1) ? 1 : 0;
                    hit += lab == cc ? 1 : 0;
                }
                if (ws_inside(S)) {
                    const float sc = ws_clamp(S);
                    const float K = weight / ((float)P.B * (float)L * (float)C1) * (upstream ? upstream[0] : 1.0f);
                    // sum over labels of (S - t): (cnt - hit) S - hit (1 - S), no cancellation inside a term
                    G = K * ((float)(cnt - hit) * sc - (float)hit * (1.0f - sc)) / fmaxf((1.0f - sc) * sc, 1e-12f);
                }
            }
        }
        colm[tid] = M; colr[tid] = rD; cols[tid] = S; colg[tid] = G;
    }
    __syncthreads();
    const T* x = logits + (int64_t)r0 * ldl;
    const T* q = prop + (int64_t)r0 * ldp;
    T* dx = dlogits + (int64_t)r0 * ldgl;
    T* dq = dprop + (int64_t)r0 * ldgp;
    for (int r = ty; r < n; r += TY) {
        float gs[N], gp[N];
#pragma unroll
        for (int k = 0; k < N; ++k) gs[k] = gp[k] = 0.0f;
        if (c < C1 && (!valid || valid[r0 + r])) {
            float s[N], p[N];
            load_chunk<T>(x + (int64_t)r * ldl, c, vec_l, (int)ldl, s);
            load_chunk<T>(q + (int64_t)r * ldp, c, vec_p, (int)ldp, p);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const int t = tx * N + k;
                if (c + k < C1 && colg[t] != 0.0f) {
                    const float sg = ws_sigmoid(s[k]);
                    const float w = colg[t] * (expf(p[k] - colm[t]) * colr[t]);
                    gs[k] = w * (sg * (1.0f - sg));
                    gp[k] = w * (sg - cols[t]);
                }
            }
        }
        if (c < ldgl) store_chunk<T>(dx + (int64_t)r * ldgl, c, vec_gl, (int)ldgl, gs);
        if (c < ldgp) store_chunk<T>(dq + (int64_t)r * ldgp, c, vec_gp, (int)ldgp, gp);
    }
}

static inline int ws_ncb(int C1) { return (C1 + WS_CB - 1) / WS_CB; }

extern "C" int64_t dgx_wsddn_workspace_floats(int R, int B, int C) {
    (void)R;
    if (B <= 0 || C < 0) return 0;
    return (int64_t)B * 3 * (C + 1) + (int64_t)B * ws_ncb(C + 1);
}

extern "C" int dgx_wsddn_loss(const void* logits, int64_t ld_logits, const void* prop, int64_t ld_prop, const uint8_t* valid,
                              const float* boxes, int B, const int* row0, const float* img_h, const float* img_w,
                              const int32_t* label_off, const int32_t* labels, int C, float weight, const float* col_stats_in,
                              const float* upstream, int32_t* sel_out, float* out8, void* dlogits, int64_t ld_dlogits, void* dprop,
                              int64_t ld_dprop, float* ws, int dtype, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!col_stats_in && !out8) return DGX_ERR_BAD_ARG;
    const int R = (B > 0 && B <= WS_MAX_IMAGES && row0) ? row0[B] : 0;
    if (B <= 0 || R <= 0) {                          // nothing to score: a zero loss, no gradient rows to write
        if (B > WS_MAX_IMAGES || (B > 0 && !row0)) return DGX_ERR_BAD_ARG;
        if (out8) (void)hipMemsetAsync(out8, 0, 8 * sizeof(float), st);
        return DGX_OK;
    }
    const bool grad = dlogits || dprop;
    if (!logits || !prop || !boxes || !img_h || !img_w || !label_off || C <= 0 || ld_logits < C + 1 || ld_prop < C + 1 ||
        (grad && (!dlogits || !dprop || ld_dlogits < C + 1 || ld_dprop < C + 1)) || (col_stats_in && !grad) ||
        (!col_stats_in && (!sel_out || !ws)) || (dtype != DGX_F32 && dtype != DGX_BF16))
        return DGX_ERR_BAD_ARG;
    WSImages P;
    P.B = B;
    if (row0[0] != 0) return DGX_ERR_BAD_ARG;        // the R rows are [0, row0[B]): every one of them belongs to an image
    for (int i = 0; i <= B; ++i) {
        P.row0[i] = row0[i];
        if (i > 0 && row0[i] < row0[i - 1]) return DGX_ERR_BAD_ARG;
    }
    for (int i = 0; i < B; ++i) { P.H[i] = img_h[i]; P.W[i] = img_w[i]; }
    const int C1 = C + 1, ncb = ws_ncb(C1);
    const size_t es = dtype == DGX_BF16 ? 2 : 4;
    auto al = [es](const void* p, int64_t ld) { return p && ((uintptr_t)p % 16 == 0) && ((ld * es) % 16 == 0); };
    const bool vec_l = al(logits, ld_logits), vec_p = al(prop, ld_prop), vec_gl = al(dlogits, ld_dlogits), vec_gp = al(dprop, ld_dprop);
    const int64_t ldmax = ld_dlogits > ld_dprop ? ld_dlogits : ld_dprop;
    const dim3 ggrid((unsigned)((ldmax + WS_CB - 1) / WS_CB), (unsigned)B);
#define WS_LAUNCH(T)                                                                                                                  \
    do {                                                                                                                              \
        if (!col_stats_in) {                                                                                                          \
            hipLaunchKernelGGL(wsddn_stats_kernel<T>, dim3(ncb, B), dim3(WS_THREADS), 0, st, (const T*)logits, ld_logits,             \
                               (const T*)prop, ld_prop, valid, P, label_off, labels, C1, sel_out, ws, vec_l, vec_p);                  \
            hipLaunchKernelGGL(wsddn_fold_kernel<T>, dim3(1), dim3(64), 0, st, (const T*)logits, ld_logits, boxes, P, label_off,      \
                               labels, C1, ncb, weight, sel_out, ws, out8);                                                           \
        }                                                                                                                             \
        if (grad)                                                                                                                     \
            hipLaunchKernelGGL(wsddn_grad_kernel<T>, ggrid, dim3(WS_THREADS), 0, st, (const T*)logits, ld_logits, (const T*)prop,     \
                               ld_prop, valid, P, label_off, labels, C1, weight, col_stats_in ? col_stats_in : ws, upstream,          \
                               (T*)dlogits, ld_dlogits, (T*)dprop, ld_dprop, vec_l, vec_p, vec_gl, vec_gp);                           \
    } while (0)
    if (dtype == DGX_BF16) WS_LAUNCH(uint16_t);
    else WS_LAUNCH(float);
#undef WS_LAUNCH
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
