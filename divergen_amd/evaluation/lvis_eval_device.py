"""LVIS average precision scored on the GPU (opt-in: TEST.LVIS_EVAL_DEVICE): the IoUs, the greedy matching and the precision /
recall accumulation of lvis_eval.LVISEval as four kernels of csrc/lvis_eval.hip (layers/eval_ops.py), bit for bit -- the Python
evaluator is the yardstick and stays the default.

What stays on the host: reading the json, LVISEval.__init__ itself (the federated filter, the max_dets cut, the areas, the
r / c / f groups: inherited, not restated), rasterising ground-truth polygons (ann_to_rle), and the bookkeeping that lays the
(image, category) groups out as CSR arrays.  Detection RLE strings are decoded by the batched host function dgx_rle_from_string
instead of character by character in the interpreter.
"""
import numpy as np
import torch

from .. import _lib as L
from ..layers import eval_ops as E
from .lvis_eval import LVISEval, rle_runs

_METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"]


def _runs_csr(counts, off):
    """Run lengths in CSR form (counts int64, off (n+1)) -> (start i32, end i32, cum i32, run_off i64): lvis_eval.rle_runs of
    every mask at once; cum is the foreground length up to and including the run (rle_runs' cum without its leading 0)."""
    lens = np.diff(off)
    total = int(off[-1])
    nrun = lens // 2
    run_off = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(nrun, out=run_off[1:])
    if total == 0:
        z = np.zeros(0, dtype=np.int32)
        return z, z.copy(), z.copy(), run_off
    ce = np.cumsum(counts)
    before = np.where(off[:-1] > 0, ce[np.maximum(off[:-1], 1) - 1], 0)          # the sum of everything before the mask
    edge = ce - np.repeat(before, lens)
    pos = np.arange(total, dtype=np.int64) - np.repeat(off[:-1], lens)
    first = (pos % 2 == 0) & (pos + 1 < np.repeat(lens, lens))                    # a start that has its end
    s = edge[first]
    t = edge[np.flatnonzero(first) + 1]
    cl = np.cumsum(t - s)
    nz = np.flatnonzero(nrun)                                                     # masks that own runs
    before_run = np.zeros(lens.size, dtype=np.int64)
    before_run[nz] = np.where(run_off[nz] > 0, cl[np.maximum(run_off[nz], 1) - 1], 0)
    cum = cl - np.repeat(before_run, nrun)
    return s.astype(np.int32), t.astype(np.int32), cum.astype(np.int32), run_off


class LVISEvalDevice(LVISEval):
    """LVISEval with run() on the device.  Same attributes (iou_thrs, rec_thrs, area_rng, cat_ids, img_ids, freq_groups,
    precision, recall) and the same summarize().

    The images are worked through in chunks of `chunk_images` (ascending image id).  Device memory is bounded by
      * the chunk: 12 bytes per foreground run of its masks, 8 bytes per (detection, ground truth) pair of its groups,
        and 9 + 1 bytes per (area range, threshold) for each of its detections and ground truths (match outputs, matched flags);
      * the detection count: 2 bytes per (area range, threshold) and detection (the matched / ignore bits kept for the
        accumulation: 80 bytes per detection) plus 8 for its place in the score order.
    """

    def __init__(self, gt_json, results, iou_type="segm", max_dets=300, chunk_images=256, time_kernels=False):
        self.chunk_images = int(chunk_images)
        self.device = torch.device("cuda")
        self.time_kernels, self.kernel_ms = bool(time_kernels), {}
        self._res_counts = None
        if iou_type == "segm":
            # every detection string is decoded once, in one call; LVISEval then sees plain run-length lists
            strs = [k for k, r in enumerate(results) if isinstance(r["segmentation"]["counts"], (str, bytes))]
            counts, off = E.rle_from_strings([results[k]["segmentation"]["counts"] for k in strs])
            decoded = dict(zip(strs, range(len(strs))))
            per, plain = [], []
            for k, r in enumerate(results):
                j = decoded.get(k)
                c = counts[off[j]:off[j + 1]] if j is not None else np.asarray(r["segmentation"]["counts"], dtype=np.int64)
                per.append(c)
                plain.append(dict(r, segmentation={"size": r["segmentation"]["size"], "counts": c.tolist()}))
            self._res_counts = per
            results = plain
        super().__init__(gt_json, results, iou_type, max_dets)
        if iou_type == "segm":
            for i, im in self.imgs.items():
                if int(im["height"]) * int(im["width"]) >= 2 ** 31:
                    raise L.DgxError("LVISEvalDevice: image %r is %d x %d: run positions are int32, H*W must stay below 2^31"
                                     % (i, im["height"], im["width"]))

    # ------------------------------------------------------------------------------------------- host layout
    def _layout(self):
        """The (image, category) groups in (image id, category id) order as flat arrays."""
        keys = set(k for k, v in self._gts.items() if v) | set(k for k, v in self._dts.items() if v)
        keys = sorted(k for k in keys if k[0] in self.imgs and k[1] in self.cats)
        cat_index = {c: i for i, c in enumerate(self.cat_ids)}
        img_index = {i: n for n, i in enumerate(self.img_ids)}
        segm = self.iou_type == "segm"
        g_img, g_cat, nD, nG = [], [], [], []
        gt_area, gt_ign, gt_id, gt_box, gt_counts = [], [], [], [], []
        dt_area, dt_score, dt_nel, dt_box, dt_counts = [], [], [], [], []
        for img, cat in keys:
            gts = self._gts[img, cat] if (img, cat) in self._gts else []
            dts = sorted(self._dts[img, cat], key=lambda x: -x["score"]) if (img, cat) in self._dts else []
            g_img.append(img_index[img])
            g_cat.append(cat_index[cat])
            nD.append(len(dts))
            nG.append(len(gts))
            nel = 1 if cat in self.img_nel[img] else 0
            for g in gts:
                gt_area.append(float(g["area"]))
                gt_ign.append(1 if g["ignore"] else 0)
                gt_id.append(int(g["id"]))
                if segm:
                    gt_counts.append(rle_runs(g["segmentation"]))
                else:
                    gt_box.append(g["bbox"])
            for d in dts:
                dt_area.append(float(d["area"]))
                dt_score.append(d["score"])
                dt_nel.append(nel)
                if segm:
                    dt_counts.append(self._res_counts[d["id"] - 1])
                else:
                    dt_box.append(d["bbox"])
        lay = {"g_img": np.asarray(g_img, dtype=np.int64), "g_cat": np.asarray(g_cat, dtype=np.int64)}
        nD, nG = np.asarray(nD, dtype=np.int64), np.asarray(nG, dtype=np.int64)
        for name, n in (("d_off", nD), ("g_off", nG), ("iou_off", nD * nG)):
            lay[name] = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(n, dtype=np.int64)])
        lay["gt_area"], lay["gt_ign"] = np.asarray(gt_area, dtype=np.float64), np.asarray(gt_ign, dtype=np.uint8)
        lay["gt_id"] = np.asarray(gt_id, dtype=np.int64)
        lay["dt_area"], lay["dt_nel"] = np.asarray(dt_area, dtype=np.float64), np.asarray(dt_nel, dtype=np.uint8)
        lay["dt_score"] = np.asarray(dt_score, dtype=np.float64)
        lay["dt_cat"], lay["gt_cat"] = np.repeat(lay["g_cat"], nD), np.repeat(lay["g_cat"], nG)
        if segm:
            z = np.zeros(0, dtype=np.int64)
            off = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum([c.size for c in dt_counts], dtype=np.int64)])
            lay["dt_runs"] = _runs_csr(np.concatenate(dt_counts) if dt_counts else z, off)
            nr = np.asarray([r[0].size for r in gt_counts], dtype=np.int64)
            cat = lambda i, dt: np.concatenate([np.asarray(r[i], dtype=np.int64) for r in gt_counts]).astype(dt) if gt_counts else z.astype(dt)
            lay["gt_runs"] = (cat(0, np.int32), cat(1, np.int32),
                              (np.concatenate([r[2][1:] for r in gt_counts]) if gt_counts else z).astype(np.int32),
                              np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(nr, dtype=np.int64)]))
        else:
            lay["dt_box"] = np.asarray(dt_box, dtype=np.float64).reshape(-1, 4)
            lay["gt_box"] = np.asarray(gt_box, dtype=np.float64).reshape(-1, 4)
        return lay

    def _up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _timed(self, name, fn, *args):
        if not self.time_kernels:
            return fn(*args)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*args)
        b.record()
        b.synchronize()
        self.kernel_ms[name] = self.kernel_ms.get(name, 0.0) + a.elapsed_time(b)
        return out

    # ------------------------------------------------------------------------------------------- run
    def run(self):
        T, K, A = len(self.iou_thrs), len(self.cat_ids), len(self.area_rng)
        lay = self._layout()
        dev = self.device
        n_dt, n_groups = int(lay["d_off"][-1]), int(lay["g_img"].size)
        thrs = self._up(np.asarray(self.iou_thrs, dtype=np.float64))
        rng = np.asarray(self.area_rng, dtype=np.float64).reshape(A, 2)
        rng_d = self._up(rng)
        matched = torch.zeros(A, T, n_dt, dtype=torch.uint8, device=dev)
        ignore = torch.zeros(A, T, n_dt, dtype=torch.uint8, device=dev)
        # chunks of images = contiguous ranges of groups, detections and ground truths
        step = max(self.chunk_images, 1)
        bounds = np.searchsorted(lay["g_img"], np.arange(0, len(self.img_ids) + step, step), side="left")
        for ga, gb in zip(bounds[:-1], bounds[1:]):
            ga, gb = int(ga), int(gb)
            if gb <= ga:
                continue
            d0, d1 = int(lay["d_off"][ga]), int(lay["d_off"][gb])
            g0, g1 = int(lay["g_off"][ga]), int(lay["g_off"][gb])
            if d1 == d0:
                continue                                  # no detection in the chunk: nothing to match
            n_pairs = int(lay["iou_off"][gb] - lay["iou_off"][ga])
            d_off, g_off = self._up(lay["d_off"][ga:gb + 1] - d0), self._up(lay["g_off"][ga:gb + 1] - g0)
            iou_off = self._up(lay["iou_off"][ga:gb + 1] - lay["iou_off"][ga])
            if self.iou_type == "segm":
                def cut(runs, m0, m1):
                    r0, r1 = int(runs[3][m0]), int(runs[3][m1])
                    return tuple(self._up(x[r0:r1]) for x in runs[:3]) + (self._up(runs[3][m0:m1 + 1] - r0),)
                ious = self._timed("rle_iou", E.rle_iou, cut(lay["dt_runs"], d0, d1), cut(lay["gt_runs"], g0, g1), d_off, g_off,
                                   iou_off, n_pairs)
            else:
                ious = self._timed("box_iou", E.box_iou_xywh, self._up(lay["dt_box"][d0:d1]), self._up(lay["gt_box"][g0:g1]), d_off,
                                   g_off, iou_off, n_pairs)
            m, ig = self._timed("match", E.lvis_match, ious, d_off, g_off, iou_off, self._up(lay["gt_area"][g0:g1]),
                                self._up(lay["gt_ign"][g0:g1]), self._up(lay["gt_id"][g0:g1]), self._up(lay["dt_area"][d0:d1]),
                                self._up(lay["dt_nel"][d0:d1]), thrs, rng_d)
            matched[:, :, d0:d1] = (m != 0).to(torch.uint8)
            ignore[:, :, d0:d1] = ig
        # per category: its detections by descending score, stable over (image id, visiting order) -- the global order
        order = np.lexsort((-lay["dt_score"], lay["dt_cat"])).astype(np.int64)
        cat_off = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(np.bincount(lay["dt_cat"], minlength=K), dtype=np.int64)])
        ga_, gi_ = lay["gt_area"], lay["gt_ign"]
        num_gt = np.zeros((K, A), dtype=np.int64)
        for a in range(A):
            keep = ~((gi_ != 0) | (ga_ < rng[a, 0]) | (ga_ > rng[a, 1]))
            num_gt[:, a] = np.bincount(lay["gt_cat"][keep], minlength=K)
        prec, rec = self._timed("accumulate", E.lvis_accumulate, matched, ignore, self._up(order), self._up(cat_off), self._up(num_gt),
                                self._up(np.asarray(self.rec_thrs, dtype=np.float64)))
        self.precision, self.recall = prec.cpu().numpy(), rec.cpu().numpy()
        self.n_groups, self.n_dt, self.n_gt, self.n_pairs = n_groups, n_dt, int(lay["g_off"][-1]), int(lay["iou_off"][-1])
        return self.summarize()


def evaluate_predictions_on_lvis_device(gt_json, results, iou_type, max_dets_per_image=300):
    """lvis_eval.evaluate_predictions_on_lvis with the scoring on the device: same arguments, same dict."""
    if len(results) == 0:
        return {m: float("nan") for m in _METRICS}
    if iou_type == "segm":
        results = [{k: v for k, v in r.items() if k != "bbox"} for r in results]
    out = LVISEvalDevice(gt_json, results, iou_type, max_dets_per_image).run()
    return {m: float(out[m] * 100) for m in _METRICS}
