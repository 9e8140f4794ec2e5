// LVIS AP scoring on the device (gfx950): the arithmetic of divergen_amd/evaluation/lvis_eval.py -- lvis-api's LVISEval, what
// D2/evaluation/lvis_evaluation.py:331-380 (_evaluate_predictions_on_lvis) calls -- bit for bit: the host evaluator is the
// yardstick (itself pinned to D2/layers/csrc/cocoeval/cocoeval.cpp at 1e-12, tests/test_oracle_eval.py).
//   dgx_rle_from_string  (host)  maskApi.c rleFrString, batched: the inverse of dgx_rle_to_string (mask_paste.hip)
//   dgx_rle_iou                  maskApi.c rleIou (iscrowd = 0) per (detection, ground truth) of every (image, category) group
//   dgx_box_iou_xywh_f64         lvis_eval.box_iou_xywh over the same groups
//   dgx_lvis_match               LVISEval._evaluate_img: every group x area range x IoU threshold in one launch
//   dgx_lvis_accumulate          LVISEval.run's curve per (category, area range, threshold)
//
// None of this is a bandwidth or MFMA kernel; all four are integer / latency bound, and exact by construction (64-bit integer
// sums, one IEEE division per result, no floating-point atomics, no order-dependent sum: two runs give the same bits).
//   rle_iou    : one wave per pair.  The lanes take the runs of the mask with FEWER runs and binary-search each run's two ends
//                in the other mask (lvis_eval._covered): runs_min * 2 * log2(runs_max) dependent 4-byte loads that hit L2 (all
//                detections of a group meet the same ground truths), then a 64-bit wave reduction.  12 bytes per run are read
//                per mask and pair, 8 bytes written per pair.
//   box_iou    : one lane per pair, 64 bytes read, 8 written, ~12 float64 operations with contraction off (a fused
//                multiply-add in w*h + w*h - inter changes the last bit of the quotient: tests/test_gpu_lvis_eval.py).
//   match      : one lane per (group, area range, threshold), the threshold fastest: the 10 lanes of a group and area range
//                read the same IoU row (one L1 line, broadcast) and diverge only where a threshold separates them.  The greedy
//                scan is sequential per lane, D_g * G_g steps of one 8-byte IoU load; ~10^6 groups x 40 lanes fill the chip.
//                The matched flags of the ground truths live in a workspace of A * T bytes per ground truth: no cap on G_g.
//                Writes 9 bytes per (area, threshold, detection).
//   accumulate : one 256-lane workgroup per (category, area range, threshold); two sweeps over the category's detections in
//                chunks of 256 (2 bytes read per detection and sweep through an 8-byte index): the totals, then right to left a
//                block scan of the true / false positives and a suffix maximum of the precision.  Each of the R recall points
//                is written by the one detection at which the recall first reaches it (np.searchsorted, side = "left").
#include "dgx_common.h"

namespace {
constexpr int EV_THREADS = 256;

// the group that owns flat pair p: iou_off[g] <= p < iou_off[g+1] (groups without pairs are stepped over)
__device__ __forceinline__ int64_t group_of_pair(const int64_t* __restrict__ iou_off, int64_t n_groups, int64_t p) {
    int64_t lo = 0, hi = n_groups;                       // first g with iou_off[g] > p, minus one
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (iou_off[mid + 1] > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// lvis_eval._covered: foreground pixels of a mask (n runs at s / e / cum) in [0, x)
__device__ __forceinline__ int64_t covered(const int32_t* __restrict__ s, const int32_t* __restrict__ e,
                                           const int32_t* __restrict__ cum, int64_t n, int32_t x) {
    int64_t lo = 0, hi = n;                              // k = runs that end at or before x (searchsorted, side = "right")
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (e[mid] > x) hi = mid; else lo = mid + 1;
    }
    int64_t c = lo > 0 ? (int64_t)cum[lo - 1] : 0;
    if (lo < n) {
        const int64_t part = (int64_t)x - (int64_t)s[lo];
        if (part > 0) c += part;
    }
    return c;
}

__global__ __launch_bounds__(EV_THREADS) void rle_iou_kernel(
    const int32_t* __restrict__ d_start, const int32_t* __restrict__ d_end, const int32_t* __restrict__ d_cum,
    const int64_t* __restrict__ d_run_off, const int32_t* __restrict__ g_start, const int32_t* __restrict__ g_end,
    const int32_t* __restrict__ g_cum, const int64_t* __restrict__ g_run_off, const int64_t* __restrict__ d_off,
    const int64_t* __restrict__ g_off, const int64_t* __restrict__ iou_off, int64_t n_groups, int64_t n_pairs,
    double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (EV_THREADS / 64);
    for (int64_t p = (int64_t)blockIdx.x * (EV_THREADS / 64) + (threadIdx.x >> 6); p < n_pairs; p += waves) {
        const int64_t g = group_of_pair(iou_off, n_groups, p);
        const int64_t G = g_off[g + 1] - g_off[g], local = p - iou_off[g];
        const int64_t dm = d_off[g] + local / G, gm = g_off[g] + local % G;
        const int64_t a0 = d_run_off[dm], an = d_run_off[dm + 1] - a0, b0 = g_run_off[gm], bn = g_run_off[gm + 1] - b0;
        const int64_t area_a = an > 0 ? (int64_t)d_cum[a0 + an - 1] : 0, area_b = bn > 0 ? (int64_t)g_cum[b0 + bn - 1] : 0;
        int64_t inter = 0;
        if (an > 0 && bn > 0) {
            // the intersection is symmetric and exact: walk the shorter run list, search the longer one
            const bool swap = bn < an;
            const int32_t *ws = swap ? g_start + b0 : d_start + a0, *we = swap ? g_end + b0 : d_end + a0;
            const int32_t *ss = swap ? d_start + a0 : g_start + b0, *se = swap ? d_end + a0 : g_end + b0;
            const int32_t* sc = swap ? d_cum + a0 : g_cum + b0;
            const int64_t wn = swap ? bn : an, sn = swap ? an : bn;
            for (int64_t r = lane; r < wn; r += 64) inter += covered(ss, se, sc, sn, we[r]) - covered(ss, se, sc, sn, ws[r]);
        }
        for (int o = 32; o > 0; o >>= 1) inter += __shfl_down(inter, o, 64);
        if (lane == 0) {
            const int64_t uni = area_a + area_b - inter;
            out[p] = uni > 0 ? (double)inter / (double)uni : 0.0;
        }
    }
}

__global__ __launch_bounds__(EV_THREADS) void box_iou_kernel(const double* __restrict__ d_box, const double* __restrict__ g_box,
                                                            const int64_t* __restrict__ d_off, const int64_t* __restrict__ g_off,
                                                            const int64_t* __restrict__ iou_off, int64_t n_groups, int64_t n_pairs,
                                                            double* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * EV_THREADS;
    for (int64_t p = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x; p < n_pairs; p += stride) {
        const int64_t g = group_of_pair(iou_off, n_groups, p);
        const int64_t G = g_off[g + 1] - g_off[g], local = p - iou_off[g];
        const double* a = d_box + 4 * (d_off[g] + local / G);
        const double* b = g_box + 4 * (g_off[g] + local % G);
        const double ax = a[0], ay = a[1], aw = a[2], ah = a[3], bx = b[0], by = b[1], bw = b[2], bh = b[3];
        // Python's min(p, q) = q < p ? q : p, max(p, q) = q > p ? q : p
        const double ax1 = ax + aw, bx1 = bx + bw, ay1 = ay + ah, by1 = by + bh;
        const double dx = (bx1 < ax1 ? bx1 : ax1) - (bx > ax ? bx : ax);
        const double dy = (by1 < ay1 ? by1 : ay1) - (by > ay ? by : ay);
        const double ix = dx > 0.0 ? dx : 0.0, iy = dy > 0.0 ? dy : 0.0;
        const double inter = ix * iy;
        const double pa = aw * ah, pb = bw * bh;
        const double uni = (pa + pb) - inter;
        out[p] = uni > 0 ? inter / uni : 0.0;
    }
}

__global__ __launch_bounds__(EV_THREADS) void lvis_match_kernel(
    const double* __restrict__ ious, const int64_t* __restrict__ d_off, const int64_t* __restrict__ g_off,
    const int64_t* __restrict__ iou_off, int64_t n_groups, int64_t n_dt, int64_t n_gt, const double* __restrict__ gt_area,
    const uint8_t* __restrict__ gt_ignore, const int64_t* __restrict__ gt_id, const double* __restrict__ dt_area,
    const uint8_t* __restrict__ dt_nel, const double* __restrict__ iou_thrs, int T, const double* __restrict__ area_rng, int A,
    uint8_t* __restrict__ matched, int64_t* __restrict__ dt_match, uint8_t* __restrict__ dt_ignore) {
    const int64_t idx = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x;
    if (idx >= n_groups * A * T) return;
    const int t = (int)(idx % T), a = (int)((idx / T) % A);
    const int64_t g = idx / ((int64_t)A * T);
    const int64_t d0 = d_off[g], D = d_off[g + 1] - d0, g0 = g_off[g], G = g_off[g + 1] - g0;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double thr = iou_thrs[t], thr0 = thr < 1 - 1e-10 ? thr : 1 - 1e-10;        // min(thr, 1 - 1e-10)
    const int64_t plane = (int64_t)a * T + t;
    uint8_t* gm = matched + plane * n_gt + g0;
    const double* garea = gt_area + g0;
    const uint8_t* gign = gt_ignore + g0;
    for (int64_t di = 0; di < D; ++di) {
        const double* row = ious + iou_off[g] + di * G;
        double best = thr0;
        int64_t m = -1;
        int m_ig = 0;
        // the ground truths in the order of np.argsort(ignore, kind="mergesort"): the unignored ones first, each kind in its own
        // order.  An unignored match ends the scan at the first free ignored ground truth: the second sweep is not entered.
        for (int sweep = 0; sweep < 2 && m < 0; ++sweep) {
            for (int64_t gi = 0; gi < G; ++gi) {
                const double ar = garea[gi];
                const int ig = (gign[gi] != 0 || ar < lo || ar > hi) ? 1 : 0;
                if (ig != sweep || gm[gi]) continue;
                const double v = row[gi];
                if (v < best) continue;
                best = v;                                 // a later equal IoU replaces the earlier one
                m = gi;
                m_ig = sweep;
            }
        }
        const int64_t o = plane * n_dt + d0 + di;
        int64_t id = 0;
        int ign = 0;
        if (m >= 0) {
            gm[m] = 1;
            id = gt_id[g0 + m];
            ign = m_ig;
        }
        if (id == 0) {                                    // unmatched: outside the area range, or the category is not exhaustive here
            const double da = dt_area[d0 + di];
            if (da < lo || da > hi || dt_nel[d0 + di] != 0) ign = 1;
        }
        dt_match[o] = id;
        dt_ignore[o] = (uint8_t)ign;
    }
}

// first r with thr[r] > x (thr ascending)
__device__ __forceinline__ int upper_bound_f64(const double* thr, int R, double x) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thr[mid] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(EV_THREADS) void lvis_accumulate_kernel(
    const uint8_t* __restrict__ dt_matched, const uint8_t* __restrict__ dt_ignore, int64_t n_dt, const int64_t* __restrict__ order,
    const int64_t* __restrict__ cat_off, int K, const int64_t* __restrict__ num_gt, const double* __restrict__ rec_thrs, int R, int T,
    int A, double* __restrict__ precision, double* __restrict__ recall) {
#pragma clang fp contract(off)
    __shared__ double s_thr[1024];
    __shared__ int s_tp[EV_THREADS], s_fp[EV_THREADS];
    __shared__ double s_mx[EV_THREADS];
    __shared__ int64_t s_tot[2];
    const int tid = threadIdx.x;
    const int t = blockIdx.x % T, a = (blockIdx.x / T) % A, k = blockIdx.x / (T * A);
    const int64_t ng = num_gt[(int64_t)k * A + a];
    if (ng == 0) return;                                  // stays -1
    const int64_t base = cat_off[k], n = cat_off[k + 1] - base;
    const int64_t plane = ((int64_t)a * T + t) * n_dt;
    const int64_t pstride = (int64_t)K * A;               // precision (T, R, K, A): step of r
    double* prec = precision + ((int64_t)t * R * K + k) * A + a;
    for (int r = tid; r < R; r += EV_THREADS) {
        s_thr[r] = rec_thrs[r];
        prec[r * pstride] = 0.0;                          // recall points never reached stay 0
    }
    if (n == 0) {
        if (tid == 0) recall[((int64_t)t * K + k) * A + a] = 0.0;
        return;
    }
    // sweep 1: the totals
    int64_t tp = 0, fp = 0;
    for (int64_t i = tid; i < n; i += EV_THREADS) {
        const int64_t d = plane + order[base + i];
        const int ig = dt_ignore[d] != 0, mt = dt_matched[d] != 0;
        tp += (mt && !ig);
        fp += (!mt && !ig);
    }
    for (int o = 32; o > 0; o >>= 1) {
        tp += __shfl_down(tp, o, 64);
        fp += __shfl_down(fp, o, 64);
    }
    if (tid == 0) s_tot[0] = s_tot[1] = 0;
    __syncthreads();
    if ((tid & 63) == 0) {                                // integer sums: the order of the four waves does not matter
        atomicAdd((unsigned long long*)&s_tot[0], (unsigned long long)tp);
        atomicAdd((unsigned long long*)&s_tot[1], (unsigned long long)fp);
    }
    __syncthreads();
    int64_t tp_hi = s_tot[0], fp_hi = s_tot[1];           // cumulative counts at the end of the current chunk
    const double dng = (double)ng;
    if (tid == 0) recall[((int64_t)t * K + k) * A + a] = (double)tp_hi / dng;
    const double eps = 2.220446049250313e-16;             // np.spacing(1)
    double carry = -1.0;                                  // maximum of the precision to the right of the current chunk
    // sweep 2: chunks from the right
    for (int64_t c0 = ((n - 1) / EV_THREADS) * EV_THREADS; c0 >= 0; c0 -= EV_THREADS) {
        const int64_t i = c0 + tid;
        const bool valid = i < n;
        int tpf = 0, fpf = 0;
        if (valid) {
            const int64_t d = plane + order[base + i];
            const int ig = dt_ignore[d] != 0, mt = dt_matched[d] != 0;
            tpf = (mt && !ig);
            fpf = (!mt && !ig);
        }
        __syncthreads();                                  // the previous chunk's reads of s_* are done
        s_tp[tid] = tpf;
        s_fp[tid] = fpf;
        __syncthreads();
        for (int o = 1; o < EV_THREADS; o <<= 1) {        // inclusive scan
            const int x = tid >= o ? s_tp[tid - o] : 0, y = tid >= o ? s_fp[tid - o] : 0;
            __syncthreads();
            s_tp[tid] += x;
            s_fp[tid] += y;
            __syncthreads();
        }
        const int ctp = s_tp[EV_THREADS - 1], cfp = s_fp[EV_THREADS - 1];
        const int64_t cum_tp = tp_hi - ctp + s_tp[tid], cum_fp = fp_hi - cfp + s_fp[tid];
        const double dtp = (double)cum_tp, dfp = (double)cum_fp;
        double pr = valid ? dtp / ((dfp + dtp) + eps) : -1.0;
        s_mx[tid] = pr;
        __syncthreads();
        for (int o = 1; o < EV_THREADS; o <<= 1) {        // inclusive suffix maximum
            const double x = tid + o < EV_THREADS ? s_mx[tid + o] : -1.0;
            __syncthreads();
            if (x > s_mx[tid]) s_mx[tid] = x;
            __syncthreads();
        }
        double v = s_mx[tid];
        if (carry > v) v = carry;
        const double left = s_mx[0];
        if (left > carry) carry = left;
        if (valid && (tpf || i == 0)) {
            // the recall reaches rec_thrs[r] first at i for rc[i-1] < rec_thrs[r] <= rc[i]
            const int r1 = upper_bound_f64(s_thr, R, dtp / dng);
            const int r0 = i == 0 ? 0 : upper_bound_f64(s_thr, R, (double)(cum_tp - tpf) / dng);
            for (int r = r0; r < r1; ++r) prec[r * pstride] = v;
        }
        tp_hi -= ctp;
        fp_hi -= cfp;
    }
}

inline unsigned ev_grid(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > 262144 ? 262144 : b));
}
}  // namespace

extern "C" int64_t dgx_rle_from_string(const char* buf, const int64_t* off, int64_t n, int64_t* counts, int64_t cap,
                                       int64_t* count_off) {
    if (n < 0 || (n > 0 && (!off || !count_off))) return 0;
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        count_off[i] = total;
        const int64_t first = total;
        for (int64_t p = off[i], end = off[i + 1]; p < end;) {
            uint64_t x = 0;
            int k = 0;
            bool more = true;
            while (more && p < end) {
                const int c = (int)(unsigned char)buf[p] - 48;
                if (5 * k < 64) x |= (uint64_t)(c & 0x1f) << (5 * k);
                more = (c & 0x20) != 0;
                ++p;
                ++k;
                if (!more && (c & 0x10) && 5 * k < 64) x |= ~(uint64_t)0 << (5 * k);
            }
            int64_t v = (int64_t)x;
            const int64_t m = total - first;
            if (m > 2 && total - 2 < cap) v += counts[total - 2];
            if (total < cap) counts[total] = v;
            ++total;
        }
    }
    if (n > 0) count_off[n] = total;
    return total <= cap ? total : -total;
}

extern "C" int dgx_rle_iou(const int32_t* d_start, const int32_t* d_end, const int32_t* d_cum, const int64_t* d_run_off,
                           const int32_t* g_start, const int32_t* g_end, const int32_t* g_cum, const int64_t* g_run_off,
                           const int64_t* d_off, const int64_t* g_off, const int64_t* iou_off, int64_t n_groups, int64_t n_pairs,
                           double* out, void* stream) {
    if (n_groups <= 0 || n_pairs <= 0) return n_groups < 0 || n_pairs < 0 ? DGX_ERR_BAD_ARG : DGX_OK;
    if (!d_run_off || !g_run_off || !d_off || !g_off || !iou_off || !out) return DGX_ERR_BAD_ARG;
    hipLaunchKernelGGL(rle_iou_kernel, dim3(ev_grid(n_pairs, EV_THREADS / 64)), dim3(EV_THREADS), 0, (hipStream_t)stream, d_start,
                       d_end, d_cum, d_run_off, g_start, g_end, g_cum, g_run_off, d_off, g_off, iou_off, n_groups, n_pairs, out);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_box_iou_xywh_f64(const double* d_box, const double* g_box, const int64_t* d_off, const int64_t* g_off,
                                    const int64_t* iou_off, int64_t n_groups, int64_t n_pairs, double* out, void* stream) {
    if (n_groups <= 0 || n_pairs <= 0) return n_groups < 0 || n_pairs < 0 ? DGX_ERR_BAD_ARG : DGX_OK;
    if (!d_box || !g_box || !d_off || !g_off || !iou_off || !out) return DGX_ERR_BAD_ARG;
    hipLaunchKernelGGL(box_iou_kernel, dim3(ev_grid(n_pairs, EV_THREADS)), dim3(EV_THREADS), 0, (hipStream_t)stream, d_box, g_box,
                       d_off, g_off, iou_off, n_groups, n_pairs, out);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_lvis_match(const double* ious, const int64_t* d_off, const int64_t* g_off, const int64_t* iou_off,
                              int64_t n_groups, int64_t n_dt, int64_t n_gt, const double* gt_area, const uint8_t* gt_ignore,
                              const int64_t* gt_id, const double* dt_area, const uint8_t* dt_nel, const double* iou_thrs, int T,
                              const double* area_rng, int A, uint8_t* workspace, int64_t workspace_bytes, int64_t* dt_match,
                              uint8_t* dt_ignore, void* stream) {
    if (n_groups < 0 || n_dt < 0 || n_gt < 0 || T <= 0 || A <= 0) return DGX_ERR_BAD_ARG;
    if (n_groups == 0 || n_dt == 0) return DGX_OK;
    if (!d_off || !g_off || !iou_off || !dt_area || !dt_nel || !iou_thrs || !area_rng || !dt_match || !dt_ignore) return DGX_ERR_BAD_ARG;
    const int64_t need = (int64_t)A * T * n_gt;
    if (n_gt > 0 && (!ious || !gt_area || !gt_ignore || !gt_id || !workspace || workspace_bytes < need)) return DGX_ERR_BAD_ARG;
    const int64_t lanes = n_groups * A * T, blocks = (lanes + EV_THREADS - 1) / EV_THREADS;
    if (blocks > 0x7fffffffll) return DGX_ERR_UNSUPPORTED;
    if (need > 0) {
        const hipError_t me = hipMemsetAsync(workspace, 0, (size_t)need, (hipStream_t)stream);
        if (me != hipSuccess) return -(int)me - 1000;
    }
    hipLaunchKernelGGL(lvis_match_kernel, dim3((unsigned)blocks), dim3(EV_THREADS), 0, (hipStream_t)stream, ious, d_off, g_off, iou_off,
                       n_groups, n_dt, n_gt, gt_area, gt_ignore, gt_id, dt_area, dt_nel, iou_thrs, T, area_rng, A, workspace, dt_match,
                       dt_ignore);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}

extern "C" int dgx_lvis_accumulate(const uint8_t* dt_matched, const uint8_t* dt_ignore, int64_t n_dt, const int64_t* order,
                                   const int64_t* cat_off, int K, const int64_t* num_gt, const double* rec_thrs, int R, int T, int A,
                                   double* precision, double* recall, void* stream) {
    if (K < 0 || n_dt < 0 || R <= 0 || R > 1024 || T <= 0 || A <= 0) return DGX_ERR_BAD_ARG;
    if (K == 0) return DGX_OK;
    if (!cat_off || !num_gt || !rec_thrs || !precision || !recall || (n_dt > 0 && (!dt_matched || !dt_ignore || !order)))
        return DGX_ERR_BAD_ARG;
    if ((int64_t)K * A * T > 0x7fffffffll) return DGX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lvis_accumulate_kernel, dim3((unsigned)(K * A * T)), dim3(EV_THREADS), 0, (hipStream_t)stream, dt_matched,
                       dt_ignore, n_dt, order, cat_off, K, num_gt, rec_thrs, R, T, A, precision, recall);
    DGX_LAUNCH_CHECK();
    return DGX_OK;
}
