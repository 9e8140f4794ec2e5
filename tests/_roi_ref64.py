"""float64 restatements of the RoI pooling kernels (csrc/roi_align.hip, geometry in csrc/roi_tables.h): ROIAlign / the multi-level
ROIPooler forward, their scatter backward, the output-stationary gather backward with `accumulate` and `grad_scale`, the level rule and
the GT-mask crop -- the per-element a-priori bounds the GPU test holds the kernels to (tests/test_gpu_roi_numerics.py), the case tables
both test files use, and the mutants.  numpy on the CPU; no project kernel is called from here.  tests/test_host_roi_ref.py pins the
restatements on the oracle's C ROIAlign, on tests/golden/refcpp.npz and on D2's known-answer values, and on the geometry that
tests/native/roi_tables_check.cpp prints from the real header.

GEOMETRY IS DEFINED IN fp32.  The published ROIAlign sequence is an fp32 algorithm with validity gates (-1 <= y <= H), clamps and ceilf
sample grids, so sample positions, gates, lo / up and the weights l = y - lo, h = 1 - l are computed in numpy float32 one operation at
a time (`geom`, `axis_samples`), exactly the sequence of roi_tables.h.  From there on products and sums are float64.

Every restatement returns (ref, A, n): the float64 value, the SAME contraction over absolute values, and the number of fp32 operations
on the longest path of an element in the kernel's expression:
  forward        2 gh + 2 gw   the additions into one table entry of each axis (a sample adds h and l; at the clamped last row both land
                               on one entry)
                 + sy.n + sx.n the additions of the row sum and of the column sum (the widest spans of the RoI)
                 + 2           the products wx * v and wy * racc
                 + 1           the division by count                                     -> `FWD_N`
  scatter        2 gh + 2 gw + 3 (go / count, * wy, * wx) + the number of (RoI, bin) contributions the pixel receives (atomic additions
                               in any order)                                             -> per pixel
  gather         2 gh + 2 gw + 2 (/ count, * grad_scale on the x table) + 2 (wx * v, wy * gx) + the (RoI, i, j) additions of the
                 pixel into gx + its (RoI, i) additions into acc + 1 (prev + acc)        -> per pixel
Bounds, u = 2^-24, per element, no absolute floor:
  fp32 outputs   |got - ref| <= u |ref| + ACC_FACTOR n u A
  bf16 outputs   |got - ref| <= 2^-8 |ref| + ACC_FACTOR n u A (1 + 2^-8)
  elements no sample reaches, pixels no box reaches, levels_out and the mask-crop bits: exact (A = 0 gives a zero bound).
The mask crop is restated in the kernel's own per-sample fp32 order (`mask_crop32`): its thresholded bits must be equal.

ACC_FACTOR = 1.  Worst measured |err| / bound per kernel form and output on the MI355X: see MEASURED below (filled from the run of
tests/test_gpu_roi_numerics.py; measured against the float64 restatement, never against another kernel form).

Mutants (MUTANTS; the text beside each): wrong restatements of the kind the kernels could produce.  A mutant is DEFINED on a case when
its float64 value differs from the restatement's at all; it must then leave the bound somewhere."""
import math

import numpy as np

f32 = np.float32
U = 2.0 ** -24
EB = 2.0 ** -8
ACC_FACTOR = 1.0

MEASURED = """
ACC_FACTOR = 1: the MI355X run of tests/test_gpu_roi_numerics.py needed no factor.  Worst |err| / bound per kernel form and output of
that run (every box of BOXES and LEVEL_BOXES, sampling ratio 0 and 2, all cases of the tables):
  kernel form                         output        fp32     bf16    where (fp32)
  roi_align_vec_kernel  forward       out           0.302    0.996   vec_c2048, adaptive grid
  roi_align_sep_kernel  forward, NHWC out           0.285    0.996   sep_cl_c300, adaptive grid   (0.283 at R = 2048, C = 24)
  roi_align_sep_kernel  forward, NCHW out           0.301    0.996   sep_nchw_c96_s14 (two slices of the LDS transpose)
  roi_align_vec_kernel  forward       one-hot       0.107            pixel (0, 0) of level 0
  roi_align_vec_kernel  scatter       grad (fp32)   0.214    0.216   vec_c2048, ratio 2           (bf16 column: go in bf16)
  roi_align_sep_kernel  scatter, NHWC grad (fp32)   0.214    0.211   sep_cl_c300, ratio 2
  roi_align_sep_kernel  scatter, NCHW grad (fp32)   0.199    0.199   sep_nchw_c96_s14, ratio 2
  roi_pool_bwd_gather   TH = 4        maps          0.190    0.996   c2048_s7, ratio 2, accumulate, grad_scale 1/3
  roi_pool_bwd_gather   TH = 8        maps          0.166    0.996   4 x 128 x 128 x 256, ratio 2
  roi_pool_bwd_gather   TH = 4        one-hot       0.085
  layers/roi_ops (autograd)           out / grads   0.216 / 0.141    0.996 / 0.996
The bf16 figures are the one rounding itself (half an ulp at the bottom of a binade); what the accumulation adds shows in the fp32
outputs, which stay below a third of n u A.  levels_out equalled the rule on every box, the mask-crop bits equalled `mask_crop32`
(S = 16, 28, 48), every unreached element and pixel was an exact zero, every guard stayed intact, the gather was bit-reproducible,
and the vector and the separable channels-last forward were bit-equal at C = 64 in both dtypes.
"""
__doc__ += MEASURED

MUTANTS = {
    "gate_exclusive": "the validity gate exclusive: a sample exactly at -1 or exactly at H dropped",
    "no_last_clamp": "the last-row clamp missing: a sample beyond H - 1 keeps its fraction and loses the tap past the map",
    "count_valid": "count = the valid samples of the bin instead of gh * gw",
    "no_half": "the 0.5 offset of aligned boxes dropped",
    "minsize_aligned": "the 1-pixel minimum size applied to aligned boxes too",
    "round_grid": "the adaptive grid rounded to nearest instead of up",
    "log2_level": "the level from torch's fp32 floor(4 + log2(t))",
    "first_base": "the span from the first valid sample's lo to the last one's up (descending samples lose what lies below)",
    "span_last": "the last tap of every span dropped",
    "range_no_slack": "the gather's bin range without its bin of slack either side and without the pixel a sample reaches either side "
                      "(the slack alone only absorbs fp32 rounding of the quotient: in exact arithmetic the range is a superset without it)",
    "hit_no_pm1": "the gather's reach test without its +-1 pixel",
    "accum_overwrites": "accumulate = 1 overwrites the map",
    "gscale_both": "grad_scale applied on both tables",
    "batch_ignored": "the batch index ignored: every box pooled from / scattered to image 0",
    "crop_gt": "the crop threshold > instead of >=",
}

# ------------------------------------------------------------------ case tables
N_IMG = 2
LEVELS = [(21, 27), (11, 14), (6, 7)]          # (H, W) at scales 1/8, 1/16, 1/32: a 168 x 216 image
MIN_LEVEL = 3
SCALE0 = 0.125
SMALL = (3, 5)                                  # H < TH, W < TW of every gather tile

# named boxes (x1, y1, x2, y2) on the 21 x 27 map at scale 1/8; dyadic where a gate is meant to be hit so that every fp32 step is exact
BOXES = {
    "inside": (40.0, 32.0, 120.0, 96.0),
    "past_top": (40.0, -16.0, 120.0, 96.0),            # aligned, 7 bins, 2 samples: first sample at -2.0 (dropped), second at -1.0
    "past_left": (-16.0, 32.0, 96.0, 96.0),
    "past_bottom": (40.0, 72.0, 120.0, 184.0),         # last sample at 22.0 > H
    "past_right": (120.0, 32.0, 232.0, 96.0),          # last sample at 28.0 > W
    "outside_pos": (400.0, 400.0, 500.0, 500.0),
    "outside_neg": (-300.0, -300.0, -200.0, -200.0),
    "whole": (0.0, 0.0, 216.0, 168.0),
    "empty": (40.0, 40.0, 40.0, 40.0),
    "inverted": (200.0, 120.0, 100.0, 40.0),           # x 200 -> 100: descending samples with a fixed grid, no samples with the adaptive one
    "subpixel": (84.0, 84.0, 87.0, 87.0),              # 7 x 7 bins inside one pixel
    "at_minus1": (-8.0, -8.0, 104.0, 104.0),           # 7 bins of 2 px, 2 samples: the first sample exactly at -1.0 (valid)
    "at_extent": (112.0, 64.0, 224.0, 176.0),          # the last sample exactly at H = 21 and W = 27 (valid, clamped)
    "tile_edge": (68.0, 36.0, 132.0, 100.0),           # start 8.0 / 4.0, end 16.0 / 12.0: gather tile boundaries (TW = 8, TH = 4)
    "tile_edge_m1": (60.0, 28.0, 124.0, 92.0),
    "tile_edge_p1": (76.0, 44.0, 140.0, 108.0),
    "big_grid": (-40.0, -40.0, 260.0, 220.0),          # adaptive grid 5 x 6
    "thin": (50.0, 50.0, 53.0, 51.0),                  # aligned = 0: both sides below one pixel -> clamped to 1
}


def _ulps(v, k):
    v = f32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, f32(np.inf if k > 0 else -np.inf))
    return float(v)


def level_boxes():
    """name -> (box, steps): squares of side 224 * 2^k moved `steps` ulps, k = -2 .. 1; area 0; boxes clamped to the lowest / highest"""
    out = {}
    for k in (-2, -1, 0, 1):
        for st in (-2, -1, 0, 1, 2):
            s = _ulps(224.0 * 2.0 ** k, st)
            out["lvl_k%d_%+d" % (k, st)] = ((0.0, 0.0, s, s), st)
    out["lvl_area0"] = ((30.0, 30.0, 30.0, 90.0), 0)
    out["lvl_low"] = ((10.0, 10.0, 14.0, 14.0), 0)
    out["lvl_high"] = ((-500.0, -500.0, 1500.0, 1500.0), 0)
    return out


LEVEL_BOXES = level_boxes()


def rois_of(names, table=None, batch=None):
    """(R, 5) fp32 rois of the named boxes; batch index alternates unless given"""
    table = table or {**BOXES, **{k: v[0] for k, v in LEVEL_BOXES.items()}}
    r = np.zeros((len(names), 5), f32)
    for i, nm in enumerate(names):
        r[i, 0] = (i % N_IMG) if batch is None else batch[i]
        r[i, 1:] = table[nm]
    return r


def random_rois(seed, R, n_img=N_IMG, Wi=216.0, Hi=168.0):
    g = np.random.default_rng(seed)
    xy = g.random((R, 2)) * [Wi * 0.8, Hi * 0.8] - [Wi * 0.05, Hi * 0.05]
    wh = g.random((R, 2)) ** 2 * [Wi * 0.7, Hi * 0.7] + 0.5
    b = g.integers(0, n_img, (R, 1))
    return np.concatenate([b, xy, xy + wh], 1).astype(f32)


def cycled_rois(R, seed=7):
    """R rois: every named box first, random ones behind"""
    names = list(BOXES) + list(LEVEL_BOXES)
    head = rois_of(names)
    if R <= len(head):
        return head[:R].copy()
    return np.concatenate([head, random_rois(seed, R - len(head))], 0)


# forward / scatter forms through the C ABI: name -> dict(C, S, nhwc, form, levels: "multi" | "single" | "small", R, offset bytes)
FORWARD_FORMS = {
    "vec_c8": dict(C=8, S=7, nhwc=1, form="vec"),                       # nslots = 256 > 49 bins
    "vec_c64": dict(C=64, S=7, nhwc=1, form="vec"),
    "vec_c256": dict(C=256, S=7, nhwc=1, form="vec"),
    "vec_c2048": dict(C=2048, S=7, nhwc=1, form="vec"),                 # nslots = 1
    "sep_cl_c4": dict(C=4, S=7, nhwc=1, form="sep"),
    "sep_cl_c24": dict(C=24, S=7, nhwc=1, form="sep"),                  # 256 % 3 != 0
    "sep_cl_c40": dict(C=40, S=7, nhwc=1, form="sep"),
    "sep_cl_c300": dict(C=300, S=7, nhwc=1, form="sep"),                # the c += 256 loop
    "sep_cl_c64_off4": dict(C=64, S=7, nhwc=1, form="sep", offset=4),   # io not 16-byte aligned: falls through to the separable form
    "sep_nchw_c1": dict(C=1, S=7, nhwc=0, form="sep"),
    "sep_nchw_c300": dict(C=300, S=7, nhwc=0, form="sep"),
    "sep_nchw_c96_s14": dict(C=96, S=14, nhwc=0, form="sep"),           # two slices of the LDS transpose, the last one partial
    "single_aligned0": dict(C=24, S=7, nhwc=1, form="sep", levels="single", aligned=0),
    "single_aligned1": dict(C=64, S=7, nhwc=1, form="vec", levels="single", aligned=1),
    "small_map": dict(C=64, S=7, nhwc=1, form="vec", levels="small", aligned=1),
}
R_THRESHOLDS = (1, 511, 512, 2047, 2048)          # at C = 24: nsplit 4 | 4, 2 | 2, 1 (49 bins)
GATHER_FORMS = {
    "c64_s7": dict(C=64, S=7),
    "c256_s7": dict(C=256, S=7),
    "c256_s14": dict(C=256, S=14),
    "c512_s7": dict(C=512, S=7),
    "c2048_s7": dict(C=2048, S=7),
    "c256_small": dict(C=256, S=7, levels="small"),
    "c256_single_a0": dict(C=256, S=7, levels="single", aligned=0),
}
GATHER_TH8 = dict(C=256, N=4, H=128, W=128, S=7, R=40)      # 4 * 16 * 16 = 1024 tiles of 8 rows: the smallest that reaches TH = 8
CROP_CASES = {
    "s16": dict(S=16, H=37, W=53),                    # one slice
    "s28": dict(S=28, H=37, W=53),                    # four slices
    "s48": dict(S=48, H=37, W=53),                    # 2304 bins > 8 x 256: the second trip
}


# ------------------------------------------------------------------ bounds
def f32_bound(ref, A, n):
    return U * np.abs(ref) + ACC_FACTOR * n * U * A


def bf16_bound(ref, A, n):
    return EB * np.abs(ref) + ACC_FACTOR * n * U * A * (1.0 + EB)


def bound_of(dtype_name, ref, A, n):
    return bf16_bound(ref, A, n) if dtype_name == "bf16" else f32_bound(ref, A, n)


def ratios(got, ref, bnd):
    """per element |got - ref| / bound: 0 where equal, inf for a non-finite result or an error over a zero bound"""
    got, ref, bnd = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bnd, np.float64)
    assert got.shape == ref.shape == bnd.shape, (got.shape, ref.shape, bnd.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.maximum(bnd, 1e-300))
    return np.where(np.isfinite(r), r, np.inf)


def worst_ratio(got, ref, bnd):
    return float(ratios(got, ref, bnd).max()) if np.size(ref) else 0.0


def report(kernel, case, outputs):
    """outputs: name -> worst ratio.  Prints `RATIO roi <kernel> <case> <output>=<worst |err| / bound> ...`, then asserts."""
    print("RATIO roi %s %s %s" % (kernel, case, " ".join("%s=%.3f" % kv for kv in outputs.items())))
    assert all(v <= 1.0 for v in outputs.values()), (kernel, case, outputs)


def to_bf16(a):
    """fp32 array rounded to bf16 (nearest even), returned as fp32"""
    b = np.ascontiguousarray(a, f32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(f32).reshape(np.shape(a))


# ------------------------------------------------------------------ geometry, fp32 one operation at a time
def level_of(roi, min_level, num_levels, mutant=None):
    """roi_tables.h assign_level: the fp32 value t = sqrtf(area) / 224 + 1e-8f compared with powers of two"""
    roi = np.asarray(roi, f32)
    with np.errstate(invalid="ignore"):
        area = f32(roi[3] - roi[1]) * f32(roi[4] - roi[2])
        t = f32(f32(np.sqrt(area)) / f32(224.0)) + f32(1e-8)
    if not t > 0:
        return 0
    if mutant == "log2_level":
        import torch
        lv = int(torch.floor(4 + torch.log2(torch.tensor(float(t), dtype=torch.float32))).item())
    else:
        lv = 4 + math.frexp(float(t))[1] - 1           # t = m 2^e, m in [0.5, 1): floor(log2 t) = e - 1, exactly
    return min(max(lv - min_level, 0), num_levels - 1)


def level_t(roi):
    roi = np.asarray(roi, f32)
    return f32(f32(np.sqrt(f32(roi[3] - roi[1]) * f32(roi[4] - roi[2]))) / f32(224.0)) + f32(1e-8)


class Geom:
    pass


def geom(roi, scale, ph, pw, sr, aligned, mutant=None):
    roi, scale = np.asarray(roi, f32), f32(scale)
    G = Geom()
    G.b = 0 if mutant == "batch_ignored" else int(roi[0])
    off = f32(0.5 if (aligned and mutant != "no_half") else 0.0)
    G.sw = f32(roi[1] * scale) - off
    G.sh = f32(roi[2] * scale) - off
    ew, eh = f32(roi[3] * scale) - off, f32(roi[4] * scale) - off
    rw, rh = f32(ew - G.sw), f32(eh - G.sh)
    if not aligned or mutant == "minsize_aligned":
        rw, rh = max(rw, f32(1.0)), max(rh, f32(1.0))
    G.bin_h, G.bin_w = f32(rh / f32(ph)), f32(rw / f32(pw))
    grid = (lambda v: int(np.rint(v))) if mutant == "round_grid" else (lambda v: int(np.ceil(v)))
    G.gh = sr if sr > 0 else grid(f32(rh / f32(ph)))
    G.gw = sr if sr > 0 else grid(f32(rw / f32(pw)))
    G.count = float(max(G.gh * G.gw, 1))
    return G


class Axis:
    """one axis of one RoI: W (nb, extent) float64 table summed from the fp32 l / h; W32 the same summed in fp32 in the kernel's order;
    adds (nb, extent) the additions into each entry; base / n the spans; valid (nb) the valid samples of each bin"""


def axis_table(start, binsz, g, extent, nb, mutant=None):
    T = Axis()
    T.W, T.W32 = np.zeros((nb, extent)), np.zeros((nb, extent), f32)
    T.adds = np.zeros((nb, extent), np.int64)
    T.valid = np.zeros(nb, np.int64)
    T.base, T.n = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    first, lastup = np.full(nb, -1), np.full(nb, -1)
    mn, mx = np.full(nb, 1 << 30), np.full(nb, -1)
    rows = np.arange(nb)
    i_f = rows.astype(f32)
    for s in range(max(g, 0)):
        y = f32(start) + i_f * f32(binsz) + (f32(s) + f32(0.5)) * f32(binsz) / f32(g)
        assert y.dtype == f32
        ok = ~((y <= -1.0) | (y >= extent)) if mutant == "gate_exclusive" else ~((y < -1.0) | (y > extent))
        y = np.where(y <= 0, f32(0), y)
        lo = y.astype(np.int64)
        last = lo >= extent - 1
        lo = np.where(last, extent - 1, lo)
        up = np.where(last, extent - 1, lo + 1)
        if mutant == "no_last_clamp":
            l = np.where(last, np.minimum(y - f32(extent - 1), f32(1.0)), y - lo.astype(f32)).astype(f32)
            h = (f32(1.0) - l).astype(f32)
            l = np.where(last, f32(0), l)
        else:
            y = np.where(last, lo.astype(f32), y)
            l = (y - lo.astype(f32)).astype(f32)
            h = (f32(1.0) - l).astype(f32)
        r = rows[ok]
        T.W[r, lo[ok]] += h[ok].astype(np.float64)
        T.W[r, up[ok]] += l[ok].astype(np.float64)
        T.W32[r, lo[ok]] += h[ok]
        T.W32[r, up[ok]] += l[ok]
        T.adds[r, lo[ok]] += 1
        T.adds[r, up[ok]] += 1
        T.valid[r] += 1
        first[r] = np.where(first[r] < 0, lo[ok], first[r])
        lastup[r] = up[ok]
        mn[r] = np.minimum(mn[r], lo[ok])
        mx[r] = np.maximum(mx[r], up[ok])
    has = mx >= 0
    if mutant == "first_base":
        mn, mx = first, lastup
    T.base = np.where(has, mn, 0)
    T.n = np.where(has, mx - mn + 1, 0)
    if mutant in ("first_base", "span_last"):
        cols = np.arange(extent)[None, :]
        hi = (T.base + T.n)[:, None] - (1 if mutant == "span_last" else 0)
        keep = (cols >= T.base[:, None]) & (cols < hi)
        T.W, T.W32 = T.W * keep, T.W32 * keep.astype(f32)
    return T


class RoiTables:
    pass


def roi_tables(roi, maps, scales, min_level, ph, pw, sr, aligned, mutant=None):
    """maps: [(H, W)] per level; one level: plain ROIAlign with scales[0] / aligned, else the pooler rule (aligned)"""
    t = RoiTables()
    t.lvl = level_of(roi, min_level, len(maps), mutant) if len(maps) > 1 else 0
    H, W = maps[t.lvl]
    t.G = geom(roi, scales[t.lvl], ph, pw, sr, aligned if len(maps) == 1 else True, mutant)
    t.Y = axis_table(t.G.sh, t.G.bin_h, t.G.gh, H, ph, mutant)
    t.X = axis_table(t.G.sw, t.G.bin_w, t.G.gw, W, pw, mutant)
    t.count = t.G.count
    if mutant == "count_valid":
        t.count = None          # per bin: valid_y[i] * valid_x[j]
    return t


def pooler_scales(nl, scale0=SCALE0):
    return [scale0 / (1 << l) for l in range(nl)]


def _count_of(t):
    if t.count is not None:
        return np.full((len(t.Y.valid), len(t.X.valid)), t.count)
    return np.maximum(t.Y.valid[:, None] * t.X.valid[None, :], 1).astype(np.float64)


def table_ops(t):
    return 2 * max(t.G.gh, 0) + 2 * max(t.G.gw, 0)


def FWD_N(t):
    """see the module docstring: table additions + span additions + two products + the division"""
    return table_ops(t) + int(t.Y.n.max()) + int(t.X.n.max()) + 2 + 1


# ------------------------------------------------------------------ forward
def forward64(feats, rois, scales, min_level, ph, pw, sr, aligned, mutant=None):
    """feats: list of (N, H, W, C) arrays (the values the kernel reads, any float dtype) -> (ref, A, n) of shape (R, ph, pw, C); n is per
    RoI, broadcast over its elements.  Also returns the per-RoI tables."""
    maps = [f.shape[1:3] for f in feats]
    f64 = [np.asarray(f, np.float64) for f in feats]
    R, C = len(rois), feats[0].shape[3]
    ref, A, n = np.zeros((R, ph, pw, C)), np.zeros((R, ph, pw, C)), np.zeros((R, 1, 1, 1))
    tabs = []
    for r in range(R):
        t = roi_tables(rois[r], maps, scales, min_level, ph, pw, sr, aligned, mutant)
        tabs.append(t)
        n[r] = FWD_N(t)
        if not (t.Y.n.any() and t.X.n.any()):
            continue
        ys, xs = np.nonzero(t.Y.W.any(0))[0], np.nonzero(t.X.W.any(0))[0]
        if not (len(ys) and len(xs)):
            continue
        y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
        f = f64[t.lvl][t.G.b, y0:y1, x0:x1]
        cnt = _count_of(t)[:, :, None]
        ref[r] = np.einsum("iy,jx,yxc->ijc", t.Y.W[:, y0:y1], t.X.W[:, x0:x1], f, optimize=True) / cnt
        A[r] = np.einsum("iy,jx,yxc->ijc", t.Y.W[:, y0:y1], t.X.W[:, x0:x1], np.abs(f), optimize=True) / cnt
    return ref, A, n, tabs


def forward32(feats, rois, scales, min_level, ph, pw, sr, aligned, order="rows"):
    """An fp32 evaluation of the contract: the fp32 tables in the kernel's order, then fp32 sums over the footprint, "rows" = the kernels'
    order (row sums, then the column of row sums), "cols" = columns first, "flat" = one running sum over all taps"""
    maps = [f.shape[1:3] for f in feats]
    R, C = len(rois), feats[0].shape[3]
    out = np.zeros((R, ph, pw, C), f32)
    for r in range(R):
        t = roi_tables(rois[r], maps, scales, min_level, ph, pw, sr, aligned)
        f = np.asarray(feats[t.lvl], f32)[t.G.b]
        for i in range(ph):
            for j in range(pw):
                acc = np.zeros(C, f32)
                yy = range(t.Y.base[i], t.Y.base[i] + t.Y.n[i])
                xx = range(t.X.base[j], t.X.base[j] + t.X.n[j])
                if order == "rows":
                    for y in yy:
                        racc = np.zeros(C, f32)
                        for x in xx:
                            racc = racc + t.X.W32[j, x] * f[y, x]
                        acc = acc + t.Y.W32[i, y] * racc
                elif order == "cols":
                    for x in xx:
                        cacc = np.zeros(C, f32)
                        for y in yy:
                            cacc = cacc + t.Y.W32[i, y] * f[y, x]
                        acc = acc + t.X.W32[j, x] * cacc
                else:
                    for y in reversed(yy):
                        for x in reversed(xx):
                            acc = acc + f32(t.Y.W32[i, y] * t.X.W32[j, x]) * f[y, x]
                out[r, i, j] = acc / f32(t.G.count)
    return out


# ------------------------------------------------------------------ backward
def _tile_masks(t, H, W, th, tw, ph, pw, mutant):
    """The gather's reach test and bin ranges as 0/1 masks on the tables (roi_tables.h gather_hit / gather_bin_range, fp32): MY (ph, H),
    MX (pw, W).  They must be no-ops on the true tables (tests/test_host_roi_ref.py); the two gather mutants make them bite."""
    G = t.G
    pm = f32(0.0 if mutant == "hit_no_pm1" else 1.0)
    slack_lo, slack_hi = (f32(0.0), f32(1.0)) if mutant == "range_no_slack" else (f32(1.0), f32(2.0))

    reach = 1 if mutant == "range_no_slack" else 0

    def clampb(v, hi):
        return int(min(max(v, f32(0.0)), f32(hi)))

    def brange(e_lo, e_hi, start, b, nb):
        if b == 0:
            return 0, nb
        a_, b_ = np.floor(f32(f32(e_lo - start) / b)), np.floor(f32(f32(e_hi - start) / b))
        return clampb(f32(min(a_, b_) - slack_lo), nb), clampb(f32(max(a_, b_) + slack_hi), nb)

    MY, MX = np.zeros((ph, H)), np.zeros((pw, W))
    ok = G.gh > 0 and G.gw > 0
    ya, yb = G.sh, f32(G.sh + f32(G.bin_h * f32(ph)))
    xa, xb = G.sw, f32(G.sw + f32(G.bin_w * f32(pw)))
    for y0 in range(0, H, th):
        if ok and f32(min(ya, yb) - pm) <= f32(y0 + th - 1) and f32(max(ya, yb) + pm) >= f32(y0):
            lo, hi = brange(f32(y0 - 1 + reach), f32(y0 + th - reach), G.sh, G.bin_h, ph)
            MY[lo:hi, y0:y0 + th] = 1
    for x0 in range(0, W, tw):
        if ok and f32(min(xa, xb) - pm) <= f32(x0 + tw - 1) and f32(max(xa, xb) + pm) >= f32(x0):
            for x in range(x0, min(x0 + tw, W)):
                lo, hi = brange(f32(f32(x) - f32(1.0 - reach)), f32(f32(x) + f32(1.0 - reach)), G.sw, G.bin_w, pw)
                MX[lo:hi, x] = 1
    return MY, MX


def backward64(go, rois, maps, n_img, scales, min_level, sr, aligned, mutant=None, tiles=None):
    """go (R, ph, pw, C) -> per level (grad (N, H, W, C), A, contributions (N, H, W): the (RoI, i, j) terms of the pixel,
    rows (N, H, W): its (RoI, i) terms), table ops (the largest 2 gh + 2 gw of a contributing RoI), and the tables.
    tiles = (th, tw): apply the gather's reach test and bin ranges (identity on a correct kernel)."""
    R, ph, pw, C = go.shape
    g64 = np.asarray(go, np.float64)
    out = [[np.zeros((n_img, H, W, C)), np.zeros((n_img, H, W, C)), np.zeros((n_img, H, W), np.int64), np.zeros((n_img, H, W), np.int64)]
           for H, W in maps]
    tops, tabs = 0, []
    for r in range(R):
        t = roi_tables(rois[r], maps, scales, min_level, ph, pw, sr, aligned, mutant)
        tabs.append(t)
        WY, WX = t.Y.W, t.X.W
        H, W = maps[t.lvl]
        if tiles is not None:
            MY, MX = _tile_masks(t, H, W, tiles[0], tiles[1], ph, pw, mutant)
            WY, WX = WY * MY, WX * MX
        ys, xs = np.nonzero(WY.any(0))[0], np.nonzero(WX.any(0))[0]
        if not (len(ys) and len(xs)):
            continue
        tops = max(tops, table_ops(t))
        y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
        gq = g64[r] / _count_of(t)[:, :, None]
        wy, wx = WY[:, y0:y1], WX[:, x0:x1]
        o = out[t.lvl]
        o[0][t.G.b, y0:y1, x0:x1] += np.einsum("iy,jx,ijc->yxc", wy, wx, gq, optimize=True)
        o[1][t.G.b, y0:y1, x0:x1] += np.einsum("iy,jx,ijc->yxc", wy, wx, np.abs(gq), optimize=True)
        o[2][t.G.b, y0:y1, x0:x1] += np.einsum("iy,jx->yx", (wy != 0).astype(np.int64), (wx != 0).astype(np.int64))
        o[3][t.G.b, y0:y1, x0:x1] += (wy != 0).sum(0)[:, None] * (wx != 0).any(0)[None, :]
    return out, tops, tabs


def scatter64(go, rois, maps, n_img, scales, min_level, sr, aligned, mutant=None):
    """dgx_roi_align_bwd / dgx_roi_pooler_bwd: per level (ref, A, n) with n per pixel = contributions + table ops + 3"""
    out, tops, tabs = backward64(go, rois, maps, n_img, scales, min_level, sr, aligned, mutant)
    return [(o[0], o[1], (o[2] + tops + 3)[..., None].astype(np.float64)) for o in out], tabs


def gather64(go, rois, maps, n_img, scales, min_level, sr, aligned, prev=None, gscale=1.0, tiles=None, mutant=None):
    """dgx_roi_pooler_bwd_gather_accum: prev = the maps' earlier contents when accumulate = 1 (None: accumulate = 0).
    n per pixel = (RoI, i, j) terms + (RoI, i) terms + table ops + 2 + 2 + 1"""
    out, tops, tabs = backward64(go, rois, maps, n_img, scales, min_level, sr, aligned, mutant, tiles)
    gs = float(f32(gscale))
    k = gs * gs if mutant == "gscale_both" else gs
    res = []
    for l, o in enumerate(out):
        ref, A = k * o[0], abs(gs) * o[1]
        if prev is not None:
            p = np.asarray(prev[l], np.float64)
            A = A + np.abs(p)
            if mutant != "accum_overwrites":
                ref = ref + p
        res.append((ref, A, (o[2] + o[3] + tops + 5)[..., None].astype(np.float64)))
    return res, tabs


def scatter32(go, rois, maps, n_img, scales, min_level, sr, aligned, reverse=False):
    """fp32 evaluation of the scatter contract: fp32 tables, g = go / count, (g * wy) * wx added in fp32 in RoI order (or reversed)"""
    R, ph, pw, C = go.shape
    out = [np.zeros((n_img, H, W, C), f32) for H, W in maps]
    order = range(R - 1, -1, -1) if reverse else range(R)
    for r in order:
        t = roi_tables(rois[r], maps, scales, min_level, ph, pw, sr, aligned)
        g = (np.asarray(go[r], f32) / f32(t.G.count)).astype(f32)
        bins = [(i, j) for i in range(ph) for j in range(pw)]
        for i, j in (reversed(bins) if reverse else bins):
            for y in range(t.Y.base[i], t.Y.base[i] + t.Y.n[i]):
                gy = g[i, j] * t.Y.W32[i, y]
                for x in range(t.X.base[j], t.X.base[j] + t.X.n[j]):
                    out[t.lvl][t.G.b, y, x] += gy * t.X.W32[j, x]
    return out


# ------------------------------------------------------------------ mask crop
def mask_crop32(masks, boxes, idx, S, mutant=None):
    """dgx_mask_crop in the kernel's own order: per bin an fp32 running sum over the samples (iy outer, ix inner), each sample
    ((w0 m0 + w1 m1) + w2 m2) + w3 m3 with the weights of bilinear_taps; acc / count >= 0.5.  -> (bits (R, S, S) uint8, avg fp32)"""
    M, H, W = masks.shape
    R = len(boxes)
    bits, avg = np.zeros((R, S, S), np.uint8), np.zeros((R, S, S), f32)
    ii = np.arange(S).astype(f32)
    for r in range(R):
        G = geom(np.concatenate([[0.0], boxes[r]]).astype(f32), 1.0, S, S, 0, True)
        m = masks[idx[r]].astype(f32)
        acc = np.zeros((S, S), f32)
        for iy in range(max(G.gh, 0)):
            y = G.sh + ii * G.bin_h + (f32(iy) + f32(0.5)) * G.bin_h / f32(G.gh)
            for ix in range(max(G.gw, 0)):
                x = G.sw + ii * G.bin_w + (f32(ix) + f32(0.5)) * G.bin_w / f32(G.gw)
                Y, X = np.broadcast_to(y[:, None], (S, S)), np.broadcast_to(x[None, :], (S, S))
                ok = ~((Y < -1.0) | (Y > H) | (X < -1.0) | (X > W))
                Y, X = np.where(Y <= 0, f32(0), Y), np.where(X <= 0, f32(0), X)
                yl, xl = Y.astype(np.int64), X.astype(np.int64)
                ylast, xlast = yl >= H - 1, xl >= W - 1
                yl, xl = np.where(ylast, H - 1, yl), np.where(xlast, W - 1, xl)
                yh, xh = np.where(ylast, H - 1, yl + 1), np.where(xlast, W - 1, xl + 1)
                Y, X = np.where(ylast, yl.astype(f32), Y), np.where(xlast, xl.astype(f32), X)
                ly, lx = (Y - yl.astype(f32)).astype(f32), (X - xl.astype(f32)).astype(f32)
                hy, hx = (f32(1.0) - ly).astype(f32), (f32(1.0) - lx).astype(f32)
                v = ((hy * hx) * m[yl, xl] + (hy * lx) * m[yl, xh]) + (ly * hx) * m[yh, xl]
                v = (v + (ly * lx) * m[yh, xh]).astype(f32)
                acc = np.where(ok, acc + v, acc).astype(f32)
        avg[r] = acc / f32(G.count)
        bits[r] = (avg[r] > 0.5) if mutant == "crop_gt" else (avg[r] >= 0.5)
    return bits, avg


def crop_inputs(case, seed=3):
    """masks (3, H, W) uint8, boxes (R, 4), idx (R): random blobs, boxes out of the image, repeated mask_idx, and two dyadic boxes over a
    half-plane mask whose bin averages are EXACTLY 0.5 along the edge (sums of dyadic values: exact in any order, so >= is what decides)"""
    c = CROP_CASES[case]
    S, H, W = c["S"], c["H"], c["W"]
    g = np.random.default_rng(seed + S)
    masks = np.zeros((3, H, W), np.uint8)
    masks[0] = g.random((H, W)) < 0.5
    yy, xx = np.mgrid[0:H, 0:W]
    masks[1] = ((yy - H / 2) ** 2 / (H / 3) ** 2 + (xx - W / 2) ** 2 / (W / 3) ** 2) < 1
    masks[2, :, 16:] = 1                                  # half-plane: ones from column 16
    boxes = [(-10.0, -8.0, 30.0, 20.0), (W - 12.0, H - 9.0, W + 14.0, H + 11.0), (3.25, 2.5, W - 4.75, H - 3.5),
             (5.0, 5.0, 5.0, 5.0), (-100.0, -100.0, -50.0, -50.0), (0.0, 0.0, float(W), float(H)),
             # in sample coordinates (x - 0.5) the half-plane is 0 up to 15, x - 15 up to 16, 1 beyond.  Bins of 1 pixel, one sample
             # each: bin 15 samples x = 15.5 -> exactly 0.5 (rows at fraction 0.5: hy lx + ly lx = 0.25 + 0.25)
             (0.5, 4.5, S + 0.5, S + 4.5),
             # bins of 2 pixels, 2 x 2 samples: bin 7 samples x = 15.0 and 16.0 -> (0 + 1) / 2 on whole rows
             (1.0, 2.0, 1.0 + 2.0 * S, 2.0 + 2.0 * S)]
    idx = [0, 1, 1, 0, 2, 1, 2, 2]
    return masks, np.asarray(boxes, f32), np.asarray(idx, np.int32)
