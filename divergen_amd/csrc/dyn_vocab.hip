// Dynamic classifier (MODEL.DYNAMIC_CLASSIFIER): the per-batch vocabulary of DG/divergen/modeling/meta_arch/custom_rcnn.py:159-165,
// :226-247 on the device (gfx950).
//
//   dgx_dyn_class_sample  _sample_cls_inds: get_fed_loss_inds (utils.py:16-28: torch.unique + torch.multinomial) and the cls_id_map of
//                         :244-246.  One workgroup; the classes that appear come out of a bitmap in LDS (ascending, as torch.unique
//                         sorts), the drawn classes out of a radix select of the keys prob0[c] / expo[c] held in LDS (4 passes of
//                         8 bits, the scheme of topk_sort.hip) and a bitonic sort of the SELECTED keys only: O(C + k log^2 k), no
//                         ranking of every class against every other.  Integer atomics in LDS only: the result is a pure function of
//                         the inputs.
//   dgx_zs_gather         zs_weight[:, inds + background] -> the two bf16 GEMM operand images of the sub-vocabulary, re-normalised
//                         (zero_shot_classifier.py:77-79) -- index, permute, contiguous, normalise, cast, cat and transpose in one launch.
//   dgx_remap_labels      cls_id_map[gt_classes] (detic_fast_rcnn.py:172-173, :384) that leaves negative ("ignore") labels alone.
//   dgx_zs_logits_f32     the logits against that operand pair with the fp32 accumulators kept (zero_shot_classifier.py:84).
#include "dgx_common.h"

namespace {
constexpr int DV_THREADS = 1024;
constexpr int DV_WAVES = DV_THREADS / 64;
constexpr int DV_MAX_C1 = 32768;                 // C + 1: one bitmap word per thread
constexpr size_t DV_MAX_LDS = 150 * 1024;        // dynamic LDS (keys + sort buffer + bitmap) of the 160 KB of a CU; the rest is static

__host__ __device__ inline int dv_pow2ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// exclusive sum of one int per thread over the workgroup (wave scans + the 16 wave totals); `total` gets the sum.  Starts with
// a barrier (wsum may still be read from the previous call) and does NOT end with one: the last reads of wsum are unguarded, which is
// safe only because everything that writes wsum again -- another call of this function -- begins with that barrier.
__device__ __forceinline__ int block_exclusive_scan(int v, int* wsum /* DV_WAVES + 1 */, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    __syncthreads();                              // (wsum may still be read from a previous call)
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < DV_WAVES; ++q) {
        const int s = wsum[q];
        if (q < w) base += s;
        tot += s;
    }
    total = tot;
    return base + x - v;
}

__global__ __launch_bounds__(DV_THREADS) void dyn_class_sample_kernel(const int64_t* __restrict__ labels, int G, const float* __restrict__ prob0,
                                                                      const float* __restrict__ expo, int C, int num_classes, int S, int P,
                                                                      int64_t* __restrict__ inds, int64_t* __restrict__ cls_id_map,
                                                                      int32_t* __restrict__ n_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* sortb = reinterpret_cast<uint64_t*>(smem);                    // P (key << 32 | ~index) of the drawn classes
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem + (size_t)P * 8);     // C keys: the bits of prob0 / expo (> 0), 0 = not a candidate
    const int nwords = (C + 31) >> 5;
    uint32_t* bits = keys + C;                                              // nwords: class c appears among the labels
    __shared__ int hist[256];
    __shared__ int wsum[DV_WAVES + 1];
    __shared__ uint32_t s_prefix;
    __shared__ int s_remaining;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

    for (int i = tid; i < nwords; i += DV_THREADS) bits[i] = 0u;
    __syncthreads();
    for (int g = tid; g < G; g += DV_THREADS) {
        const int64_t c = labels[g];
        if (c >= 0 && c < C) atomicOr(&bits[(int)c >> 5], 1u << ((int)c & 31));
    }
    __syncthreads();
    // ---- the classes that appear, ascending: thread t owns word t (nwords <= DV_THREADS)
    const uint32_t word = tid < nwords ? bits[tid] : 0u;
    int a = 0;
    int pos = block_exclusive_scan(__popc(word), wsum, a);
    // keys of the candidates for the draw and their number M
    int m = 0;
    for (int c = tid; c < C; c += DV_THREADS) {
        const float p = prob0[c];
        uint32_t key = 0u;
        if (p > 0.0f && !((bits[c >> 5] >> (c & 31)) & 1u)) {
            const float q = p / expo[c];
            key = q > 0.0f ? __float_as_uint(q) : 0u;       // positive floats order as their bits; an underflow to 0 is no candidate
        }
        keys[c] = key;
        m += key != 0u;
    }
    int M = 0;
    block_exclusive_scan(m, wsum, M);
    const int need = S - a;
    const int k = need > 0 ? min(need, M) : 0;
    const int n = a + k;
    // every entry of cls_id_map = n, then the entries of the selected classes (same workgroup: ordered by the barrier)
    for (int c = tid; c <= num_classes; c += DV_THREADS) cls_id_map[c] = (int64_t)n;
    if (tid == 0) *n_out = n;
    __syncthreads();
    for (uint32_t rest = word; rest;) {
        const int b = __ffs((int)rest) - 1;
        rest &= rest - 1u;
        const int c = (tid << 5) + b;
        inds[pos] = (int64_t)c;
        cls_id_map[c] = (int64_t)pos;
        ++pos;
    }
    if (k == 0) return;                                     // (uniform)
    // ---- radix select of the k-th largest key
    if (tid == 0) { s_prefix = 0u; s_remaining = k; }
    uint32_t mask = 0u;
    const int c_up = (C + 63) & ~63;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        const int rem = s_remaining;
        for (int i = tid; i < c_up; i += DV_THREADS) {
            const uint32_t key = i < C ? keys[i] : 0u;
            const bool in = i < C && (key & mask) == prefix;
            const uint32_t digit = (key >> shift) & 255u;
            const uint64_t act = __ballot(in);
            if (act == 0ull) continue;
            const uint32_t d0 = __shfl(digit, __ffsll((long long)act) - 1);
            if (__ballot(in && digit != d0) == 0ull) {
                if (lane == __ffsll((long long)act) - 1) atomicAdd(&hist[d0], __popcll(act));
            } else if (in) {
                atomicAdd(&hist[digit], 1);
            }
        }
        __syncthreads();
        int tot;
        const int h = tid < 256 ? hist[255 - tid] : 0;       // thread t looks at bin 255 - t: sums from the top
        const int above = block_exclusive_scan(h, wsum, tot);
        if (tid < 256 && above + h >= rem && above < rem) {   // exactly one thread: the counts sum to >= rem by construction
            s_prefix = prefix | ((uint32_t)(255 - tid) << shift);
            s_remaining = rem - above;
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    const uint32_t kth = s_prefix;
    const int need_eq = s_remaining;       // how many of the keys EQUAL to the k-th are taken (lowest class index first)
    // ---- ordered compaction into the sort buffer: thread t owns the contiguous chunk t of the classes
    const int chunk = (C + DV_THREADS - 1) / DV_THREADS;
    const int i0 = tid * chunk, i1 = min(C, i0 + chunk);
    int gt = 0, eq = 0;
    for (int i = i0; i < i1; ++i) {
        const uint32_t key = keys[i];
        gt += key > kth;
        eq += key == kth;
    }
    int tot_gt, tot_eq;
    const int gt0 = block_exclusive_scan(gt, wsum, tot_gt);
    const int eq0 = block_exclusive_scan(eq, wsum, tot_eq);
    const int take_before = min(eq0, need_eq);
    int o = gt0 + take_before, eq_seen = eq0;
    for (int i = i0; i < i1; ++i) {
        const uint32_t key = keys[i];
        bool take = key > kth;
        if (key == kth) { take = eq_seen < need_eq; ++eq_seen; }
        if (take && o < P) sortb[o++] = ((uint64_t)key << 32) | (uint64_t)(0xffffffffu - (uint32_t)i);
    }
    const int Pk = dv_pow2ceil(k);          // <= P: k <= min(S, C)
    for (int i = k + tid; i < Pk; i += DV_THREADS) sortb[i] = 0ull;      // below every real entry
    __syncthreads();
    // ---- bitonic sort, descending: larger key first, equal keys lower class index first
    for (int size = 2; size <= Pk; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (Pk >> 1); t += DV_THREADS) {
                const int lo = ((t / stride) * (stride << 1)) + (t % stride), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t x = sortb[lo], y = sortb[hi];
                if ((x < y) == desc) { sortb[lo] = y; sortb[hi] = x; }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < k; j += DV_THREADS) {
        const int c = (int)(0xffffffffu - (uint32_t)(sortb[j] & 0xffffffffull));
        inds[a + j] = (int64_t)c;
        cls_id_map[c] = (int64_t)(a + j);
    }
}

// One workgroup per output row j of W (npad, D); element (d, c) of zs_weight, fp32 (D, C + 1), at src + d * sd + c.
__global__ __launch_bounds__(256) void zs_gather_kernel(const float* __restrict__ src, int64_t sd, int D, int C,
                                                        const int64_t* __restrict__ inds, int n, int npad, int normalize,
                                                        uint16_t* __restrict__ W, uint16_t* __restrict__ Wt) {
    __shared__ float red[4];
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t c = j < n ? inds[j] : -1;
    if (c < 0 || c > C) c = -1;                       // background row, pad rows (and an index outside the vocabulary): zeros
    float ss = 0.0f;
    if (c >= 0 && normalize) {
        for (int d = tid; d < D; d += 256) {
            const float v = src[(int64_t)d * sd + c];
            ss += v * v;
        }
    }
    ss = wave_sum(ss);
    if (lane == 0) red[w] = ss;
    __syncthreads();
    const float denom = fmaxf(sqrtf((red[0] + red[1]) + (red[2] + red[3])), 1e-12f);       // F.normalize: x / max(||x||, eps)
    for (int d = tid; d < D; d += 256) {
        float v = 0.0f;
        if (c >= 0) {
            v = src[(int64_t)d * sd + c];
            if (normalize) v = v / denom;
        }
        const uint16_t b = f2bf(v);
        W[(int64_t)j * D + d] = b;
        Wt[(int64_t)d * npad + j] = b;
    }
}

__global__ __launch_bounds__(256) void remap_labels_kernel(const int64_t* __restrict__ in, int64_t R, const int64_t* __restrict__ cls_id_map,
                                                           int num_classes, int64_t* __restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
        const int64_t c = in[r];
        out[r] = (c >= 0 && c <= num_classes) ? cls_id_map[c] : c;
    }
}
// fp32 logits of the narrow per-call vocabulary: y (R, n1) = x (R, D) W^T, x and W (npad, D) bf16, fp32 accumulation in ascending k, the
// result NOT rounded to bf16 (the 51 columns of a sampled vocabulary cost R x 51 x D multiply-adds: no MFMA tile is worth filling, and the
// loss of five selected rows of an image step sees the logits' last bf16 bit).  Workgroup = 16 rows x 64 columns, k in chunks of 128
// through LDS, widened to fp32 there and read 16 bytes at a time; thread (ty, tx) owns row ty and columns tx, tx + 16, tx + 32, tx + 48.
constexpr int ZL_ROWS = 16, ZL_COLS = 64, ZL_K = 128, ZL_LD = ZL_K + 4;
__global__ __launch_bounds__(256) void zs_logits_f32_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ W, int R, int D, int n1,
                                                           int npad, float* __restrict__ y, int64_t ldy) {
    __shared__ __attribute__((aligned(16))) float xs[ZL_ROWS][ZL_LD];
    __shared__ __attribute__((aligned(16))) float ws[ZL_COLS][ZL_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int r0 = blockIdx.x * ZL_ROWS, c0 = blockIdx.y * ZL_COLS;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += ZL_K) {
        for (int i = tid; i < ZL_ROWS * ZL_K; i += 256) {
            const int r = i / ZL_K, k = i % ZL_K;
            xs[r][k] = (r0 + r < R && k0 + k < D) ? bf2f(x[(int64_t)(r0 + r) * D + k0 + k]) : 0.f;
        }
        for (int i = tid; i < ZL_COLS * ZL_K; i += 256) {
            const int c = i / ZL_K, k = i % ZL_K;
            ws[c][k] = (c0 + c < npad && k0 + k < D) ? bf2f(W[(int64_t)(c0 + c) * D + k0 + k]) : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int k = 0; k < ZL_K; k += 4) {
            const float4 a = *reinterpret_cast<const float4*>(&xs[ty][k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 b = *reinterpret_cast<const float4*>(&ws[tx + 16 * j][k]);
                acc[j] += a.x * b.x;          // ascending k, one addition at a time
                acc[j] += a.y * b.y;
                acc[j] += a.z * b.z;
                acc[j] += a.w * b.w;
            }
        }
        __syncthreads();
    }
    const int r = r0 + ty;
    if (r < R) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + tx + 16 * j;
            if (c < n1) y[(int64_t)r * ldy + c] = acc[j];
        }
    }
}
}  // namespace

extern "C" int dgx_dyn_class_sample(const int64_t* labels, int G, const float* prob0, const float* expo, int C, int num_classes, int S,
                                    int64_t* inds, int64_t* cls_id_map, int32_t* n_out, void* stream) {
    if (!prob0 || !expo || !inds || !cls_id_map || !n_out || C <= 0 || num_classes < C || S < 0 || G < 0 || (G > 0 && !labels))
        return DGX_ERR_BAD_ARG;
    if (C + 1 > DV_MAX_C1) return DGX_ERR_UNSUPPORTED;
    const int P = dv_pow2ceil(S < C ? (S > 0 ? S : 1) : C);
    const size_t sm = (size_t)P * 8 + (size_t)C * 4 + (size_t)((C + 31) / 32) * 4;
    if (sm > DV_MAX_LDS) return DGX_ERR_UNSUPPORTED;
    // dynamic LDS above 64 KB is asked for on every such call: the attribute belongs to the current device, and no state is kept here
    if (sm > 64 * 1024 &&
        hipFuncSetAttribute((const void*)dyn_class_sample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DV_MAX_LDS) != hipSuccess)
        return DGX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dyn_class_sample_kernel, dim3(1), dim3(DV_THREADS), sm, (hipStream_t)stream, labels, G, prob0, expo, C, num_classes, S, P,
                       inds, cls_id_map, n_out);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_zs_gather(const float* zs, int D, int C, const int64_t* inds, int n, int normalize, void* W, void* Wt, void* stream) {
    if (!zs || !W || !Wt || D <= 0 || C <= 0 || n < 0 || (n > 0 && !inds)) return DGX_ERR_BAD_ARG;
    const int npad = (n + 1 + 7) & ~7;
    hipLaunchKernelGGL(zs_gather_kernel, dim3(npad), dim3(256), 0, (hipStream_t)stream, zs, (int64_t)(C + 1), D, C, inds, n, npad, normalize,
                       (uint16_t*)W, (uint16_t*)Wt);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_remap_labels(const int64_t* in, int64_t R, const int64_t* cls_id_map, int num_classes, int64_t* out, void* stream) {
    if (R <= 0) return DGX_OK;
    if (!in || !out || !cls_id_map || num_classes <= 0) return DGX_ERR_BAD_ARG;
    const int grid = (int)((R + 255) / 256 < 1024 ? (R + 255) / 256 : 1024);
    hipLaunchKernelGGL(remap_labels_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, R, cls_id_map, num_classes, out);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_zs_logits_f32(const void* x, const void* W, int R, int D, int n1, int npad, float* y, int64_t ldy, void* stream) {
    if (R <= 0) return DGX_OK;
    if (!x || !W || !y || D <= 0 || n1 <= 0 || npad < n1 || ldy < n1) return DGX_ERR_BAD_ARG;
    hipLaunchKernelGGL(zs_logits_f32_kernel, dim3((R + ZL_ROWS - 1) / ZL_ROWS, (n1 + ZL_COLS - 1) / ZL_COLS), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)x, (const uint16_t*)W, R, D, n1, npad, y, ldy);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
