// Image-label co-training on the device (DG/divergen/modeling/roi_heads/detic_roi_heads.py:341-365 `get_top_proposals` +
// `_add_image_box`; DG/divergen/modeling/roi_heads/detic_fast_rcnn.py:342-434 `image_label_losses`, :524-581 the five
// row-selection rules).  The reference slices Python lists per image and reads `.item()` per (image, label); here every list
// has a fixed length with a validity byte per row, one workgroup owns one image, and nothing goes back to the host:
//   dgx_ws_proposals      the first K valid proposals of each image in list order, clipped, [+ the centred image box]
//   dgx_image_label_loss  row selection per (image, label), the summed sigmoid BCE of the selected rows, the statistics of the
//                         last (image, label), and -- in the same or in a later launch -- the dense gradient of the logits
// The sum over images is folded by one thread in image order and the labels of an image are walked in list order: no
// floating-point atomics anywhere, two runs give the same bits.
#include "dgx_common.h"
#include "row_chunk.h"

#define IL_MAX_IMAGES 32
struct ILImages {
    int B;
    int row0[IL_MAX_IMAGES + 1];   // rows of image b: [row0[b], row0[b+1])
    float H[IL_MAX_IMAGES], W[IL_MAX_IMAGES];
    float box[IL_MAX_IMAGES][4];   // dgx_ws_proposals: the image box of each image
};

namespace {
constexpr int IL_PART = 8;         // per-image partials: loss / L, has statistics, the five statistics, unused

// softplus(x) = BCEWithLogits(x, 0); BCEWithLogits(x, 1) = softplus(x) - x
__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

// sum_{c < C1} softplus(row[c]) by one wave (every lane returns the sum)
template <typename T> __device__ __forceinline__ float wave_row_softplus(const T* row, int C1, bool vec, int ld, int lane) {
    constexpr int N = Chunk<T>::N;
    float a = 0.0f;
    for (int c = lane * N; c < C1; c += 64 * N) {
        float f[N];
        load_chunk<T>(row, c, vec, ld, f);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (c + k < C1) a += softplus(f[k]);      // a select, not a product: the pad columns may hold anything (NaN)
    }
    return wave_sum(a);
}

// block-wide (256 threads) integer sum / maximum; every thread returns the result
__device__ __forceinline__ int block_sum_i(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ __forceinline__ int block_max_i(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}
// block-wide arg-max of (key, idx): the largest key, the LOWEST idx among equal keys (torch.argmax); idx = INT_MAX = no entry
__device__ __forceinline__ int block_argmax(float key, int idx, float* shf, int* shi) {
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
    for (int k = 1; k < 4; ++k) {
        const float ok = shf[k];
        const int oi = shi[k];
        if (oi != 0x7fffffff && (idx == 0x7fffffff || ok > key || (ok == key && oi < idx))) { key = ok; idx = oi; }
    }
    return idx;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ dgx_ws_proposals
__global__ __launch_bounds__(256) void ws_proposals_kernel(const float* __restrict__ boxes, const float* __restrict__ logits,
                                                           const uint8_t* __restrict__ valid, ILImages P, int K, int Kout, int add_box,
                                                           float* __restrict__ oboxes, float* __restrict__ ologits,
                                                           uint8_t* __restrict__ ovalid) {
    __shared__ int wtot[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Ko = Kout + (add_box ? 1 : 0);
    const float Wd = P.W[i], Hd = P.H[i];
    int base = 0;                                   // rows written so far (the same value in every thread)
    for (int k0 = 0; k0 < K && base < Kout; k0 += 256) {
        const int k = k0 + tid;
        const bool v = k < K && (!valid || valid[(int64_t)i * K + k]);
        const unsigned long long m = __ballot(v);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[w] = __popcll(m);
        __syncthreads();
        int off = base + pre;
        for (int q = 0; q < w; ++q) off += wtot[q];
        if (v && off < Kout) {
            const float* b = boxes + 4 * ((int64_t)i * K + k);
            float* o = oboxes + 4 * ((int64_t)i * Ko + off);
            o[0] = fminf(fmaxf(b[0], 0.0f), Wd);     // Boxes.clip
            o[1] = fminf(fmaxf(b[1], 0.0f), Hd);
            o[2] = fminf(fmaxf(b[2], 0.0f), Wd);
            o[3] = fminf(fmaxf(b[3], 0.0f), Hd);
            ologits[(int64_t)i * Ko + off] = logits[(int64_t)i * K + k];
            ovalid[(int64_t)i * Ko + off] = 1;
        }
        base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    if (base > Kout) base = Kout;
    for (int o = base + tid; o < Kout; o += 256) {   // a short list: padding rows
        float* ob = oboxes + 4 * ((int64_t)i * Ko + o);
        ob[0] = ob[1] = ob[2] = ob[3] = 0.0f;
        ologits[(int64_t)i * Ko + o] = 0.0f;
        ovalid[(int64_t)i * Ko + o] = 0;
    }
    if (add_box && tid == 0) {
        float* ob = oboxes + 4 * ((int64_t)i * Ko + Kout);
        ob[0] = P.box[i][0]; ob[1] = P.box[i][1]; ob[2] = P.box[i][2]; ob[3] = P.box[i][3];
        ologits[(int64_t)i * Ko + Kout] = 1.0f;
        ovalid[(int64_t)i * Ko + Kout] = 1;
    }
}

extern "C" int dgx_ws_proposals(const float* boxes, const float* logits, const uint8_t* valid, int B, int K, const float* img_h,
                                const float* img_w, int ws_num_props, int add_image_box, double image_box_size, float* out_boxes,
                                float* out_logits, uint8_t* out_valid, void* stream) {
    if (B <= 0) return DGX_OK;
    if (B > IL_MAX_IMAGES || K < 0 || ws_num_props < 0 || !img_h || !img_w || !out_boxes || !out_logits || !out_valid ||
        (K > 0 && (!boxes || !logits)) || ws_num_props + (add_image_box ? 1 : 0) <= 0)
        return DGX_ERR_BAD_ARG;
    ILImages P;
    P.B = B;
    const double f = image_box_size;
    for (int i = 0; i < B; ++i) {
        P.H[i] = img_h[i];
        P.W[i] = img_w[i];
        const double w = img_w[i], h = img_h[i];     // detic_roi_heads.py:355-362, evaluated in double and rounded once
        P.box[i][0] = (float)(w * (1. - f) / 2.);
        P.box[i][1] = (float)(h * (1. - f) / 2.);
        P.box[i][2] = (float)(w * (1. - (1. - f) / 2.));
        P.box[i][3] = (float)(h * (1. - (1. - f) / 2.));
    }
    hipLaunchKernelGGL(ws_proposals_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, boxes, logits, valid, P, K, ws_num_props,
                       add_image_box ? 1 : 0, out_boxes, out_logits, out_valid);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

// ------------------------------------------------------------------------------------------------ dgx_image_label_loss
template <typename T>
__global__ __launch_bounds__(256) void image_label_kernel(const T* __restrict__ logits, int64_t ld, const uint8_t* __restrict__ valid,
                                                          const float* __restrict__ boxes, ILImages P,
                                                          const int32_t* __restrict__ label_off, const int32_t* __restrict__ labels,
                                                          int C1, int mode, float weight, const int32_t* __restrict__ sel_in,
                                                          const float* __restrict__ upstream, int32_t* __restrict__ sel_out,
                                                          T* __restrict__ dlogits, int64_t ldg, float* __restrict__ ws, bool vec_in,
                                                          bool vec_out) {
    constexpr int N = Chunk<T>::N;
    __shared__ int shi[4];
    __shared__ float shf[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = P.row0[i], n = P.row0[i + 1] - r0, R = P.row0[P.B];
    const int l0 = label_off[i], L = label_off[i + 1] - l0;
    const T* x = logits + (int64_t)r0 * ld;
    float* rowsum = ws;                              // (R) sum_c softplus of the rows that can be selected
    float* part = ws + R + (int64_t)i * IL_PART;
    const int32_t* sel = sel_in;

    if (!sel_in) {
        // ---- the valid rows of the image: how many, the first, the last
        int cnt = 0, last = -1, nfirst = -0x7fffffff;
        for (int r = tid; r < n; r += 256)
            if (!valid || valid[r0 + r]) { ++cnt; last = max(last, r); nfirst = max(nfirst, -r); }
        const int nvalid = block_sum_i(cnt, shi);
        last = block_max_i(last, shi);
        const int first = -block_max_i(nfirst, shi);
        const bool per_label = mode == DGX_IL_MAX_SCORE || mode == DGX_IL_MIN_LOSS;
        int fixed = -1;                              // the row every label takes (max_size / first / image)
        if (nvalid > 0 && !per_label) {
            if (mode == DGX_IL_FIRST) fixed = first;
            else if (mode == DGX_IL_IMAGE) fixed = last;
            else if (nvalid == 1) fixed = first;     // `sizes[:-1].argmax() if len(sizes) > 1 else 0`
            else {
                float key = -INFINITY;
                int idx = 0x7fffffff;
                for (int r = tid; r < n; r += 256) {
                    if (r == last || (valid && !valid[r0 + r])) continue;
                    const float* b = boxes + 4 * (int64_t)(r0 + r);
                    const float a = (b[2] - b[0]) * (b[3] - b[1]);      // Boxes.area
                    if (idx == 0x7fffffff || a > key) { key = a; idx = r; }      // rows ascend: the first maximum stays
                }
                fixed = block_argmax(key, idx, shf, shi);
            }
        }
        // ---- sum_c softplus(s_rc) of every row that can be selected, one wave per row
        for (int r = w; r < n; r += 4) {
            const bool need = per_label ? (!valid || valid[r0 + r]) : r == fixed;
            if (need) {
                const float s = wave_row_softplus<T>(x + (int64_t)r * ld, C1, vec_in, (int)ld, lane);
                if (lane == 0) rowsum[r0 + r] = s;
            }
        }
        __syncthreads();
        // ---- the labels of the image in list order
        float acc = 0.0f, st0 = 0.f, st1 = 0.f, st2 = 0.f, st3 = 0.f, st4 = 0.f, has = 0.f;
        for (int j = 0; j < L; ++j) {
            const int lab = labels[l0 + j];
            const bool ok = nvalid > 0 && lab >= 0 && lab < C1;
            int pick = ok ? fixed : -1;
            if (ok && per_label) {
                float key = -INFINITY;
                int idx = 0x7fffffff;
                for (int r = tid; r < n; r += 256) {
                    if (valid && !valid[r0 + r]) continue;
                    const float s = il_ld1<T>(x + (int64_t)r * ld + lab);
                    // max_score: the stored score; min_loss: arg-min of the row's BCE sum with target one-hot(label)
                    const float k = mode == DGX_IL_MAX_SCORE ? s : -(rowsum[r0 + r] - s);
                    if (idx == 0x7fffffff || k > key) { key = k; idx = r; }
                }
                pick = block_argmax(key, idx, shf, shi);
            }
            if (tid == 0) {
                sel_out[l0 + j] = pick;
                if (pick >= 0) {
                    const float s = il_ld1<T>(x + (int64_t)pick * ld + lab);
                    acc += rowsum[r0 + pick] - s;
                    const float* b = boxes + 4 * (int64_t)(r0 + pick);
                    has = 1.0f;
                    st0 = (float)pick;                                                   // pool_stats
                    st1 = (b[2] - b[0]) * (b[3] - b[1]) / (P.H[i] * P.W[i]);             // stats_select_size
                    st2 = (b[0] + b[2]) / 2.0f / P.W[i];                                 // stats_select_x
                    st3 = (b[1] + b[3]) / 2.0f / P.H[i];                                 // stats_select_y
                    st4 = 1.0f / (1.0f + expf(-s));                                      // stats_max_label_score
                }
            }
        }
        if (tid == 0) {
            part[0] = L > 0 ? acc / (float)L : 0.0f;
            part[1] = has; part[2] = st0; part[3] = st1; part[4] = st2; part[5] = st3; part[6] = st4; part[7] = 0.0f;
        }
        sel = sel_out;
        __syncthreads();                             // sel_out of this image is read back below by every wave
    }
    if (!dlogits) return;
    // ---- dense gradient: every row of the image written once, whole leading dimension
    const float coef = L > 0 ? weight / ((float)P.B * (float)L) * (upstream ? upstream[0] : 1.0f) : 0.0f;
    T* dx = dlogits + (int64_t)r0 * ldg;
    for (int r = w; r < n; r += 4) {
        int cnt = 0;
        for (int j = lane; j < L; j += 64) cnt += sel[l0 + j] == r ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        const T* xr = x + (int64_t)r * ld;
        T* dr = dx + (int64_t)r * ldg;
        for (int c = lane * N; c < ldg; c += 64 * N) {
            float f[N], g[N];
#pragma unroll
            for (int k = 0; k < N; ++k) g[k] = 0.0f;
            if (cnt > 0 && c < C1) {
                int hit[N];                          // labels that chose this row and name column c + k
#pragma unroll
                for (int k = 0; k < N; ++k) hit[k] = 0;
                for (int j = 0; j < L; ++j) {
                    if (sel[l0 + j] != r) continue;
                    const int d = labels[l0 + j] - c;
#pragma unroll
                    for (int k = 0; k < N; ++k) hit[k] += d == k ? 1 : 0;
                }
                load_chunk<T>(xr, c, vec_in, (int)ld, f);
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    // sum over the choosing labels of sigmoid(s) - [c == label] = (cnt - hit) sigmoid(s) - hit sigmoid(-s):
                    // no cancellation at a confident positive
                    const float e = expf(-fabsf(f[k]));
                    const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
                    const float sp = f[k] >= 0.0f ? big : small, sn = f[k] >= 0.0f ? small : big;
                    if (c + k < C1) g[k] = coef * ((float)(cnt - hit[k]) * sp - (float)hit[k] * sn);
                }
            }
            store_chunk<T>(dr, c, vec_out, (int)ldg, g);
        }
    }
}

// out8 = {image_loss (weighted), stats_l_image, pool_stats, stats_select_size, stats_select_x, stats_select_y,
//         stats_max_label_score, -}: the images in order, by one thread
__global__ __launch_bounds__(64) void image_label_fold_kernel(const float* __restrict__ part, int B, float weight, float* __restrict__ out8) {
    if (threadIdx.x != 0) return;
    float s = 0.0f, st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < B; ++i) {
        const float* p = part + (int64_t)i * IL_PART;
        s += p[0];
        if (p[1] != 0.0f)
            for (int k = 0; k < 5; ++k) st[k] = p[2 + k];
    }
    const float l = s / (float)B;
    out8[0] = l * weight;
    out8[1] = l;
    for (int k = 0; k < 5; ++k) out8[2 + k] = st[k];
    out8[7] = 0.0f;
}

extern "C" int64_t dgx_image_label_workspace_floats(int R, int B) { return (int64_t)(R > 0 ? R : 0) + (int64_t)IL_PART * (B > 0 ? B : 0); }

extern "C" int dgx_image_label_loss(const void* logits, int64_t ld_logits, const uint8_t* valid, const float* boxes, int B,
                                    const int* row0, const float* img_h, const float* img_w, const int32_t* label_off,
                                    const int32_t* labels, int C, int mode, float weight, const int32_t* sel_in,
                                    const float* upstream, int32_t* sel_out, float* out8, void* dlogits, int64_t ld_dlogits,
                                    float* ws, int dtype, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!sel_in && !out8) return DGX_ERR_BAD_ARG;
    const int R = (B > 0 && B <= IL_MAX_IMAGES && row0) ? row0[B] : 0;
    if (B <= 0 || R <= 0) {                          // nothing to select from: a zero loss, no gradient rows to write
        if (B > IL_MAX_IMAGES || (B > 0 && !row0)) return DGX_ERR_BAD_ARG;
        if (out8) (void)hipMemsetAsync(out8, 0, 8 * sizeof(float), st);
        return DGX_OK;
    }
    if (!logits || !boxes || !img_h || !img_w || !label_off || C <= 0 || ld_logits < C + 1 || mode < DGX_IL_MAX_SIZE ||
        mode > DGX_IL_MIN_LOSS || (!sel_in && (!sel_out || !ws)) || (dlogits && ld_dlogits < C + 1) || (sel_in && !dlogits) ||
        (dtype != DGX_F32 && dtype != DGX_BF16))
        return DGX_ERR_BAD_ARG;
    ILImages P;
    P.B = B;
    if (row0[0] != 0) return DGX_ERR_BAD_ARG;        // the R rows are [0, row0[B]): every one of them belongs to an image
    for (int i = 0; i <= B; ++i) {
        P.row0[i] = row0[i];
        if (i > 0 && row0[i] < row0[i - 1]) return DGX_ERR_BAD_ARG;
    }
    for (int i = 0; i < B; ++i) { P.H[i] = img_h[i]; P.W[i] = img_w[i]; }
    const size_t es = dtype == DGX_BF16 ? 2 : 4;
    const bool vec_in = ((uintptr_t)logits % 16 == 0) && ((ld_logits * es) % 16 == 0);
    const bool vec_out = dlogits && ((uintptr_t)dlogits % 16 == 0) && ((ld_dlogits * es) % 16 == 0);
    if (dtype == DGX_BF16)
        hipLaunchKernelGGL(image_label_kernel<uint16_t>, dim3(B), dim3(256), 0, st, (const uint16_t*)logits, ld_logits, valid, boxes, P,
                           label_off, labels, C + 1, mode, weight, sel_in, upstream, sel_out, (uint16_t*)dlogits, ld_dlogits, ws, vec_in,
                           vec_out);
    else
        hipLaunchKernelGGL(image_label_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)logits, ld_logits, valid, boxes, P,
                           label_off, labels, C + 1, mode, weight, sel_in, upstream, sel_out, (float*)dlogits, ld_dlogits, ws, vec_in,
                           vec_out);
    if (!sel_in) hipLaunchKernelGGL(image_label_fold_kernel, dim3(1), dim3(64), 0, st, ws + R, B, weight, out8);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
