// The geometry of the RoI pooling family (roi_align.hip) and the decisions of its launches as plain C++ in the manner of gemm_plan.h
// and wgrad_plan.h: the fp32 sequence of the sample positions, validity gates, clamps and weights (torchvision's published ROIAlign
// algorithm, oracle/roi_nms.c), the 1-D weight tables of the separable forms, the level rule, the reach test and bin ranges of the
// gather backward, and which kernel form / LDS size / tile shape a launch gets.  No HIP header: ROI_HD is __host__ __device__ under
// hipcc and empty under g++, so tests/native/roi_tables_check.cpp runs THIS code on the host with bounds-checked arrays in place of
// LDS.  Every float operation is written once, here, in the order the kernels execute it (-ffp-contract=off on both sides).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ROI_HD __host__ __device__ __attribute__((always_inline))
#else
#define ROI_HD
#endif

namespace roitab {
constexpr int MAX_LEVELS = 4;
constexpr int GT_TH = 8;          // gather backward: rows of a tile (4 on small problems, see plan_gather)
constexpr int GT_QB = 8;          //                  RoIs whose tables are resident at a time
constexpr int GT_PMAX = 16;       //                  largest pooled side
constexpr int GT_TWMAX = 32;      //                  widest tile (C = 64)
constexpr size_t LDS_BYTES = 64 * 1024;

struct Taps { int pos[4]; float w[4]; };

ROI_HD inline bool bilinear_taps(int H, int W, float y, float x, Taps& t) {
    if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) return false;
    if (y <= 0) y = 0;
    if (x <= 0) x = 0;
    int y_low = (int)y, x_low = (int)x, y_high, x_high;
    if (y_low >= H - 1) { y_high = y_low = H - 1; y = (float)y_low; } else y_high = y_low + 1;
    if (x_low >= W - 1) { x_high = x_low = W - 1; x = (float)x_low; } else x_high = x_low + 1;
    const float ly = y - y_low, lx = x - x_low, hy = 1.0f - ly, hx = 1.0f - lx;
    t.pos[0] = y_low * W + x_low;   t.w[0] = hy * hx;
    t.pos[1] = y_low * W + x_high;  t.w[1] = hy * lx;
    t.pos[2] = y_high * W + x_low;  t.w[2] = ly * hx;
    t.pos[3] = y_high * W + x_high; t.w[3] = ly * lx;
    return true;
}

ROI_HD inline int roi_imax(int a, int b) { return a > b ? a : b; }

struct RoiGeom { float sw, sh, bin_w, bin_h; int gw, gh; float count; int b; };

ROI_HD inline RoiGeom roi_geom(const float* roi, float scale, int ph, int pw, int sampling_ratio, bool aligned) {
    RoiGeom G;
    G.b = (int)roi[0];
    const float off = aligned ? 0.5f : 0.0f;
    G.sw = roi[1] * scale - off;
    G.sh = roi[2] * scale - off;
    const float ew = roi[3] * scale - off, eh = roi[4] * scale - off;
    float rw = ew - G.sw, rh = eh - G.sh;
    if (!aligned) { rw = fmaxf(rw, 1.0f); rh = fmaxf(rh, 1.0f); }
    G.bin_h = rh / (float)ph;
    G.bin_w = rw / (float)pw;
    G.gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / (float)ph);
    G.gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / (float)pw);
    G.count = (float)roi_imax(G.gh * G.gw, 1);
    return G;
}

// level = floor(canonical_level + log2(sqrt(area)/224 + 1e-8)) clamped (poolers.py:50-58); evaluated
// with exact power-of-two comparisons instead of log2 so it cannot straddle an integer: the level is decided by comparing the fp32
// value t = sqrtf(area) / 224 + 1e-8f with powers of two.  (An fp32 log2 rounds 4 + log2(t) up to the integer for t one or two ulps
// below a power of two; there, and only there, the two rules differ -- include/divergen_hip.h.)
ROI_HD inline int assign_level(const float* roi, int min_level, int num_levels) {
    const float area = (roi[3] - roi[1]) * (roi[4] - roi[2]);
    float t = sqrtf(area) / 224.0f + 1e-8f;
    int lv = 4;
    if (!(t > 0.0f)) return 0;  // degenerate / NaN: lowest level
    while (t >= 2.0f && lv < 64) { t *= 0.5f; ++lv; }
    while (t < 1.0f && lv > -64) { t *= 2.0f; --lv; }
    lv -= min_level;
    return lv < 0 ? 0 : (lv >= num_levels ? num_levels - 1 : lv);
}

// Separable form.  The bilinear weight of a sample on a pixel is hat(y)*hat(x) and a bin's samples
// form a tensor grid, so the total weight a bin puts on pixel (r,q) is WY[i][r]*WX[j][q] with 1-D
// tables built once per RoI in LDS (same clamping / validity rules as the per-sample form).  A bin
// then touches each pixel of its footprint once -- (bin_h+1)(bin_w+1) taps instead of
// 4*ceil(bin_h)*ceil(bin_w) -- and backward issues one atomic per footprint pixel per bin.
struct Span { int base, n; };

// Wt: any object with operator[](int) over floats (a float* in the kernels, a bounds-checked array in the host checker); row i of the
// table is Wt[i * stride_tbl ...].  The span of a bin is [min lo, max up] over its valid samples, found BEFORE accumulating: the
// samples of an inverted box (x2 < x1 with a fixed sampling ratio: a negative bin size) descend, so the first valid sample is not the
// lowest.  Ascending samples accumulate in the order and with the indices they always had.
template <class F> ROI_HD inline void build_axis_table(F Wt, Span* sp, int nb, int stride_tbl, float start, float bin, int g, int extent,
                                                       int tid, int tid0) {
    const int i = tid - tid0;
    if (i < 0 || i >= nb) return;
    F w = Wt + i * stride_tbl;
    for (int k = 0; k < stride_tbl; ++k) w[k] = 0.0f;
    int base = -1, hi = -1;
    for (int s = 0; s < g; ++s) {
        float y = start + i * bin + ((float)s + 0.5f) * bin / (float)g;
        if (y < -1.0f || y > (float)extent) continue;
        if (y <= 0) y = 0;
        int lo = (int)y, up;
        if (lo >= extent - 1) { up = lo = extent - 1; } else up = lo + 1;
        if (base < 0 || lo < base) base = lo;
        if (up > hi) hi = up;
    }
    for (int s = 0; s < g; ++s) {
        float y = start + i * bin + ((float)s + 0.5f) * bin / (float)g;
        if (y < -1.0f || y > (float)extent) continue;
        if (y <= 0) y = 0;
        int lo = (int)y, up;
        if (lo >= extent - 1) { up = lo = extent - 1; y = (float)lo; } else up = lo + 1;
        const float l = y - lo, h = 1.0f - l;
        w[lo - base] += h;
        w[up - base] += l;
    }
    sp[i].base = base < 0 ? 0 : base;
    sp[i].n = base < 0 ? 0 : hi - base + 1;
}

// ---- gather backward: the table rows of bin i restricted to the nw pixels from p0 (the float sequence of build_axis_table)
template <class F> ROI_HD inline void gather_axis_rows(F w, int nw, int i, float start, float bin, int g, int extent, int p0) {
    for (int k = 0; k < nw; ++k) w[k] = 0.0f;
    for (int s = 0; s < g; ++s) {
        float y = start + i * bin + ((float)s + 0.5f) * bin / (float)g;
        if (y < -1.0f || y > (float)extent) continue;
        if (y <= 0) y = 0;
        int lo = (int)y, up;
        if (lo >= extent - 1) { up = lo = extent - 1; y = (float)lo; } else up = lo + 1;
        const float l = y - lo, h = 1.0f - l;
        if ((unsigned)(lo - p0) < (unsigned)nw) w[lo - p0] += h;
        if ((unsigned)(up - p0) < (unsigned)nw) w[up - p0] += l;
    }
}

ROI_HD inline int clamp_bin(float v, int hi) { return (int)fminf(fmaxf(v, 0.0f), (float)hi); }

// Does the sample grid of G reach the th x tw tile at (y0, x0)?  A sample at y weighs rows floor(y) and floor(y)+1 (after clamping into
// the map): rows within [y-1, y+1].  The bins run from start to start + bin * n, downwards when the box is inverted: the test takes the
// lower and the upper end whichever way they run.
ROI_HD inline bool gather_hit(const RoiGeom& G, int ph, int pw, int y0, int x0, int th, int tw) {
    const float ya = G.sh, yb = G.sh + G.bin_h * ph, xa = G.sw, xb = G.sw + G.bin_w * pw;
    return G.gh > 0 && G.gw > 0 && fminf(ya, yb) - 1.0f <= (float)(y0 + th - 1) && fmaxf(ya, yb) + 1.0f >= (float)y0 &&
           fminf(xa, xb) - 1.0f <= (float)(x0 + tw - 1) && fmaxf(xa, xb) + 1.0f >= (float)x0;
}

// Bins [lo, hi) whose interval meets the pixel range [edge_lo, edge_hi], one bin of slack either side; every bin when the bin size is 0.
ROI_HD inline void gather_bin_range(float edge_lo, float edge_hi, float start, float bin, int nbins, int& lo, int& hi) {
    lo = 0; hi = nbins;
    if (bin != 0.0f) {
        const float a = floorf((edge_lo - start) / bin), b = floorf((edge_hi - start) / bin);
        lo = clamp_bin(fminf(a, b) - 1.0f, nbins);
        hi = clamp_bin(fmaxf(a, b) + 2.0f, nbins);
    }
}

// ---- host decisions ------------------------------------------------------------------------------------------------------------
// vector form (8 channels per lane, several bins in flight) or the separable one-lane-per-channel form
inline bool pool_wants_vec(int out_nhwc, int C, bool aligned16) {
    return out_nhwc && (C & 7) == 0 && C <= 2048 && 256 % (C >> 3) == 0 && aligned16;
}

// grid (R, nsplit) of bins_per_block bins each, table strides and dynamic LDS of launch_pool
struct PoolPlan {
    bool ok;                   // false: DGX_ERR_UNSUPPORTED (the NCHW tile does not fit LDS)
    int spy, spx, bpb, nsplit;
    size_t tbl, sm;            // bytes of the tables + spans; with the NCHW transpose tile
};
inline PoolPlan plan_pool(const int* Hs, const int* Ws, int num_levels, int C, int R, int ph, int pw, int out_nhwc) {
    PoolPlan p = {};
    const int bins = ph * pw;
    int spy = 0, spx = 0;
    for (int l = 0; l < num_levels; ++l) { spy = Hs[l] > spy ? Hs[l] : spy; spx = Ws[l] > spx ? Ws[l] : spx; }
    p.spy = spy + 1; p.spx = spx + 1;
    p.tbl = (size_t)(ph * p.spy + pw * p.spx) * 4 + (size_t)(ph + pw) * sizeof(Span);
    if (out_nhwc) {
        int nsplit = R >= 2048 ? 1 : (R >= 512 ? 2 : 4);
        if (nsplit > bins) nsplit = bins;
        p.bpb = (bins + nsplit - 1) / nsplit;
    } else {
        if (p.tbl + (size_t)C * 4 > LDS_BYTES) return p;
        p.bpb = (int)((LDS_BYTES - p.tbl) / ((size_t)C * 4));
        if (p.bpb > bins) p.bpb = bins;
    }
    p.nsplit = (bins + p.bpb - 1) / p.bpb;
    p.sm = p.tbl + (out_nhwc ? 0 : (size_t)p.bpb * C * 4);
    p.ok = p.sm <= LDS_BYTES;
    return p;
}

// gather backward: does the kernel take the shape at all
inline bool gather_supported(int C, int ph, int pw) {
    return !(C <= 0 || (C & 7) || 256 % (C >> 3) || 256 / (C >> 3) > GT_TWMAX || ph <= 0 || pw <= 0 || ph > GT_PMAX || pw > GT_PMAX);
}

// tile height: 8 rows, or 4 when that is what it takes to give every CU a tile (a tile's workgroup walks the RoIs that reach it
// one after the other: with the RoI heads' three levels at 1024^2 x 2 images the 32 tiles of the coarsest level take most of the
// boxes of an untrained model each, while 650 small-level tiles finish early -- 4-row tiles halve the longest walk's work)
struct GatherPlan {
    int tw, th, total;
    int tile0[MAX_LEVELS + 1], tiles_x[MAX_LEVELS], tiles_y[MAX_LEVELS];
};
inline GatherPlan plan_gather(const int* Hs, const int* Ws, int num_levels, int N, int C) {
    GatherPlan p = {};
    p.tw = 256 / (C >> 3);
    p.th = GT_TH;
    int64_t t8 = 0;
    for (int l = 0; l < num_levels; ++l) t8 += (int64_t)N * ((Ws[l] + p.tw - 1) / p.tw) * ((Hs[l] + 7) / 8);
    if (t8 < 4 * 256) p.th = 4;
    for (int l = 0; l < num_levels; ++l) {
        p.tile0[l] = p.total;
        p.tiles_x[l] = (Ws[l] + p.tw - 1) / p.tw;
        p.tiles_y[l] = (Hs[l] + p.th - 1) / p.th;
        p.total += N * p.tiles_x[l] * p.tiles_y[l];
    }
    p.tile0[num_levels] = p.total;
    return p;
}

// mask crop: slices of 256 bins per box (grid.y), at most 8: a slice then takes every 8th run of 256 bins
inline int mask_crop_slices(int S) { return (S * S + 255) / 256 < 8 ? (S * S + 255) / 256 : 8; }
}  // namespace roitab
