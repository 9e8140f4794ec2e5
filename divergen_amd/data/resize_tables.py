"""Host half of INPUT.DEVICE_RESIZE (numpy only; runs in a loader worker): the fixed-point coefficient tables of Pillow's 8-bit BILINEAR
resample, and the job table dgx_resize_bilinear_u8 (csrc/resize_u8.hip) reads.

Pillow (Resample.c, precompute_coeffs + normalize_coeffs_8bpc) for an axis in -> out, in C doubles = float64 here:
    scale = in / out;  fs = max(scale, 1);  support = fs;  ksize = 2 * ceil(support) + 1
    per output xx:  center = (xx + 0.5) * scale;  xmin = max(int(center - support + 0.5), 0);  xmax = min(int(center + support + 0.5), in)
                    w[x] = max(0, 1 - |(x + xmin - center + 0.5) * (1 / fs)|) for x < xmax - xmin, divided by their sum (added in order)
                    k[x] = int(w[x] * 2^22 + 0.5)                       (the int casts truncate toward zero)
An axis that keeps its size is skipped by Pillow; here it carries identity taps (n = 1, k = 2^22), which give the byte back exactly:
(2^21 + s * 2^22) >> 22 == s.  Tables are built for the outputs of a window [lo, hi) only: Pillow computes every output independently."""
import numpy as np

PRECISION_BITS = 22
JOB_WORDS = 13                      # int32 words of one job row (include/divergen_hip.h: dgx_resize_bilinear_u8)
TILE_W, TILE_H = 64, 16             # output tile of one workgroup (csrc/resize_u8.hip: RS_TILE_W / RS_TILE_H): tile0 counts these
FLIP, INTERLEAVED, PREMUL = 1, 2, 4


def axis_table(in_size, out_size, lo=0, hi=None):
    """-> (bounds (L, 2) int32 = (xmin, n), k (L, ksize) int32) for the outputs lo .. hi - 1 of an axis resampled in_size -> out_size."""
    in_size, out_size = int(in_size), int(out_size)
    hi = out_size if hi is None else int(hi)
    lo = int(lo)
    if in_size < 1 or out_size < 1 or not 0 <= lo < hi <= out_size:
        raise ValueError("axis_table: %d -> %d, window [%d, %d)" % (in_size, out_size, lo, hi))
    if in_size == out_size:
        idx = np.arange(lo, hi, dtype=np.int32)
        return np.stack([idx, np.ones_like(idx)], 1), np.full((hi - lo, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(lo, hi, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # astype truncates toward zero, as the C cast
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    w = 1.0 - np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where((x < n[:, None]) & (w > 0.0), w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                           # added left to right, as the C loop (trailing zeros add nothing)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(ww != 0.0, w / ww, w)
    k = np.where(w < 0.0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
    return np.stack([xmin, n], 1).astype(np.int32), k.astype(np.int32)


class ResizeJob:
    """One job of dgx_resize_bilinear_u8: `src` (h, w, C) uint8 resized to out_hw with Pillow's BILINEAR, the window of crop_hw at
    crop_yx of the result, mirrored when flip; written planar (C, ch, cw), or interleaved RGBA (ch, cw, 4) when `interleaved`.  The
    tables cover the window only.  RGBA premultiplies around the resample whenever a size changes, as Image.resize does on 'RGBA'."""

    def __init__(self, src, out_hw, crop_yx=(0, 0), crop_hw=None, flip=False, interleaved=False):
        src = np.ascontiguousarray(src, dtype=np.uint8)
        if src.ndim != 3 or src.shape[2] not in (3, 4) or (interleaved and src.shape[2] != 4):
            raise ValueError("ResizeJob: a source of shape %s (interleaved %s)" % (src.shape, interleaved))
        self.src = src
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.crop_yx = (int(crop_yx[0]), int(crop_yx[1]))
        self.crop_hw = (self.out_hw[0] - self.crop_yx[0], self.out_hw[1] - self.crop_yx[1]) if crop_hw is None else (int(crop_hw[0]), int(crop_hw[1]))
        self.flip, self.interleaved = bool(flip), bool(interleaved)
        (oy, ox), (ch, cw) = self.crop_yx, self.crop_hw
        self.v_bounds, self.v_k = axis_table(src.shape[0], self.out_hw[0], oy, oy + ch)
        self.h_bounds, self.h_k = axis_table(src.shape[1], self.out_hw[1], ox, ox + cw)

    @property
    def channels(self):
        return int(self.src.shape[2])

    @property
    def flags(self):
        premul = self.channels == 4 and self.out_hw != tuple(self.src.shape[:2])
        return (FLIP if self.flip else 0) | (INTERLEAVED if self.interleaved else 0) | (PREMUL if premul else 0)

    @property
    def out_bytes(self):
        return self.crop_hw[0] * self.crop_hw[1] * (4 if self.interleaved else self.channels)

    @property
    def tiles(self):
        return -(-self.crop_hw[1] // TILE_W) * -(-self.crop_hw[0] // TILE_H)


def assemble_jobs(jobs, dst_offsets):
    """ResizeJobs + the byte offset of each job's window in its destination buffer -> (src uint8, table int32 (J, JOB_WORDS), tab int32):
    the three arrays of one launch.  Sources are laid back to back, each on a 4-byte boundary."""
    rows, srcs, tabs = [], [], []
    src_off = tab_off = tile0 = 0
    for job, dst in zip(jobs, dst_offsets):
        parts = (job.h_bounds, job.h_k, job.v_bounds, job.v_k)
        h_off, v_off = tab_off, tab_off + parts[0].size + parts[1].size
        rows.append([src_off, job.src.shape[0], job.src.shape[1], job.channels, job.crop_hw[0], job.crop_hw[1], job.flags, int(dst),
                     h_off, parts[1].shape[1], v_off, parts[3].shape[1], tile0])
        tabs.extend(p.reshape(-1) for p in parts)
        tab_off += sum(p.size for p in parts)
        tile0 += job.tiles
        raw = job.src.reshape(-1)
        pad = (-raw.size) % 4
        srcs.append(raw)
        if pad:
            srcs.append(np.zeros(pad, dtype=np.uint8))
        src_off += raw.size + pad
    table = np.asarray(rows, dtype=np.int32).reshape(-1, JOB_WORDS)
    src = np.concatenate(srcs) if srcs else np.zeros(0, dtype=np.uint8)
    tab = np.concatenate(tabs).astype(np.int32) if tabs else np.zeros(0, dtype=np.int32)
    return src, table, tab
