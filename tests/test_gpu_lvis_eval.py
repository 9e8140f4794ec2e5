"""The device LVIS evaluator (TEST.LVIS_EVAL_DEVICE; csrc/lvis_eval.hip, evaluation/lvis_eval_device.py) against its yardsticks:
the reference's cocoeval.cpp answers of tests/golden/refcpp.npz (1e-12, what the Python evaluator is held to) and the Python
evaluator itself (bit for bit).  Nothing here is compared against the code under test."""
import ctypes
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from divergen_amd import _lib  # noqa: E402
from divergen_amd.evaluation import lvis_eval as LE  # noqa: E402

DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _offsets(sizes):
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(np.asarray(sizes, dtype=np.int64))])


def _group_offsets(shapes):
    """[(D, G)] -> d_off, g_off, iou_off."""
    return _offsets([s[0] for s in shapes]), _offsets([s[1] for s in shapes]), _offsets([s[0] * s[1] for s in shapes])


# ------------------------------------------------------------------------------------------------ reference's numbers
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_device_evaluator_equals_reference_cocoeval_cpp_and_python(seed, golden):
    from divergen_amd.evaluation.lvis_eval_device import LVISEvalDevice
    from tests.test_oracle_eval import _dataset
    gt, dets = _dataset(seed)
    dv = LVISEvalDevice(gt, dets, "bbox", 300)
    dv.run()
    z = golden("refcpp")
    prec, rec = z["cocoeval_precision_%d" % seed], z["cocoeval_recall_%d" % seed]
    assert prec.shape == dv.precision.shape and rec.shape == dv.recall.shape
    np.testing.assert_array_equal(prec > -1, dv.precision > -1)
    np.testing.assert_allclose(dv.precision, prec, rtol=0, atol=1e-12)
    np.testing.assert_allclose(dv.recall, rec, rtol=0, atol=1e-12)
    py = LE.LVISEval(gt, dets, "bbox", 300)
    py.run()
    np.testing.assert_array_equal(dv.precision, py.precision)
    np.testing.assert_array_equal(dv.recall, py.recall)


# ------------------------------------------------------------------------------------------------ box IoU bits
def _fma(a, b, c):
    """round(a * b + c) with one rounding.  math.fma where the interpreter has it; otherwise exact rationals (a longdouble's
    64-bit mantissa does not hold the 106-bit product, so it would not be a fused multiply-add)."""
    import math
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _contracted_ious(a, b):
    """box_iou_xywh the ways a compiler may contract `a[2] * a[3] + b[2] * b[3] - inter` (inter = ix * iy)."""
    ix = max(0.0, min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0]))
    iy = max(0.0, min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1]))
    inter = ix * iy
    unions = [_fma(a[2], a[3], b[2] * b[3]) - inter, _fma(b[2], b[3], a[2] * a[3]) - inter,
              _fma(-ix, iy, a[2] * a[3] + b[2] * b[3]), _fma(-ix, iy, _fma(a[2], a[3], b[2] * b[3]))]
    return [inter / u if u > 0 else 0.0 for u in unions]


def test_box_iou_bits_equal_python():
    from divergen_amd.layers import eval_ops as E
    rng = np.random.RandomState(3)
    shapes = [(100, 60), (1, 1), (57, 70), (0, 4), (3, 0), (1, 13)] + [(1, 1)] * 5
    d_off, g_off, iou_off = _group_offsets(shapes)
    nd, ng = int(d_off[-1]), int(g_off[-1])

    def boxes(n):
        return np.concatenate([rng.uniform(0, 100, (n, 2)), rng.uniform(1, 60, (n, 2))], axis=1)
    db, gb = boxes(nd), boxes(ng)
    # the constructed pairs are the last five 1 x 1 groups: half box (IoU exactly 0.5), three-quarter box, disjoint, zero area (union 0) x 2
    db[-5:] = [[10, 10, 10, 10], [0, 0, 30, 40], [0, 0, 5, 5], [3, 3, 0, 0], [1, 2, 0, 7]]
    gb[-5:] = [[10, 10, 20, 10], [0, 0, 40, 40], [50, 50, 5, 5], [3, 3, 0, 0], [1, 2, 0, 3]]
    want = np.concatenate([np.array([LE.box_iou_xywh(db[d], gb[g]) for d in range(d_off[k], d_off[k + 1]) for g in range(g_off[k], g_off[k + 1])],
                                    dtype=np.float64) for k in range(len(shapes))])
    assert want.size == int(iou_off[-1]) >= 10 ** 4
    assert want[-5:].tolist() == [0.5, 0.75, 0.0, 0.0, 0.0]
    # without pairs on which a fused multiply-add changes the last bit the test could not see a contracted build:
    # 789 of the 10 009 pairs here change under at least one contraction
    sensitive, p = 0, 0
    for k in range(len(shapes)):
        for d in range(d_off[k], d_off[k + 1]):
            for g in range(g_off[k], g_off[k + 1]):
                sensitive += any(v != want[p] for v in _contracted_ious(db[d], gb[g]))
                p += 1
    print("pairs that a contraction changes: %d of %d" % (sensitive, want.size))
    assert sensitive >= 100
    got = E.box_iou_xywh(_up(db), _up(gb), _up(d_off), _up(g_off), _up(iou_off), int(iou_off[-1])).cpu().numpy()
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ mask IoU bits
def _enc(m):
    flat = m.T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return {"size": list(m.shape), "counts": ([0] + counts) if flat[0] else counts}


def _runs(rles):
    """lvis_eval.rle_runs of each mask, laid out as the kernel reads them."""
    tr = [LE.rle_runs(r) for r in rles]
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0)).astype(np.int32)
    return (_up(cat([t[0] for t in tr])), _up(cat([t[1] for t in tr])), _up(cat([t[2][1:] for t in tr])),
            _up(_offsets([t[0].size for t in tr])))


def _mask_iou_case(dmasks, gmasks, shapes):
    from divergen_amd.layers import eval_ops as E
    d_off, g_off, iou_off = _group_offsets(shapes)
    assert d_off[-1] == len(dmasks) and g_off[-1] == len(gmasks)
    dr, gr = [_enc(m) for m in dmasks], [_enc(m) for m in gmasks]
    want = np.array([LE.rle_iou(dr[d], gr[g]) for k in range(len(shapes)) for d in range(d_off[k], d_off[k + 1])
                     for g in range(g_off[k], g_off[k + 1])], dtype=np.float64)
    got = E.rle_iou(_runs(dr), _runs(gr), _up(d_off), _up(g_off), _up(iou_off), int(iou_off[-1])).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    again = E.rle_iou(_runs(dr), _runs(gr), _up(d_off), _up(g_off), _up(iou_off), int(iou_off[-1])).cpu().numpy()
    np.testing.assert_array_equal(again, got)
    return want


def _special_masks(h, w):
    empty, full = np.zeros((h, w), bool), np.ones((h, w), bool)
    first, last = empty.copy(), empty.copy()
    first[0, 0] = True                                    # set at pixel 0: a leading zero run
    first[3:9, 2:7] = True
    last[h - 1, w - 1] = True                             # one pixel, the last of the column-major order
    return [empty, full, first, last]


@pytest.mark.parametrize("h,w", [(37, 53), (480, 640)])
def test_mask_iou_bits_equal_python(h, w):
    rng = np.random.RandomState(h)
    sp = _special_masks(h, w)
    rnd = []
    for p in (0.03, 0.4, 0.5, 0.9):
        m = rng.rand(h, w) < p
        m[0, 0] = p > 0.45
        rnd.append(m)
    blob = np.zeros((h, w), bool)
    blob[h // 4:h // 2, w // 3:w - 2] = True
    dm = sp + rnd + [blob]
    gm = [blob, rnd[2], rnd[0]] + sp + [rnd[1]]
    # every special and random mask against every other one, then two lone groups: empty x full and full x empty
    want = _mask_iou_case(dm + [sp[0], sp[1]], gm + [sp[1], sp[0]], [(len(dm), len(gm)), (1, 1), (1, 1)])
    assert want[-2:].tolist() == [0.0, 0.0] and (want == 1.0).sum() >= 4 and ((want > 0) & (want < 1)).sum() > 20
    if h * w > 2 * 4096 * 4:
        nruns = [LE.rle_runs(_enc(m))[0].size for m in (rnd[1], rnd[2])]
        assert min(nruns) > 4096                          # no lane can hold such a mask's runs


def test_mask_iou_group_wider_than_a_wave_both_ways():
    rng = np.random.RandomState(9)
    h, w = 37, 53
    D, G = 300, 130

    def blobs(n):
        out = []
        for _ in range(n):
            m = np.zeros((h, w), bool)
            y, x = rng.randint(0, h - 8), rng.randint(0, w - 8)
            m[y:y + rng.randint(2, 20), x:x + rng.randint(2, 24)] = True
            m ^= rng.rand(h, w) < 0.05
            out.append(m)
        return out
    want = _mask_iou_case(blobs(D) + blobs(2), blobs(G) + blobs(3), [(D, G), (2, 3)])
    assert want.size == D * G + 6 and (want > 0.3).sum() > 50


# ------------------------------------------------------------------------------------------------ matcher hard cases
H, W, MAX_DETS = 64, 96, 20


def _rect(box, as_string):
    x, y, w, h = (int(v) for v in box)
    m = np.zeros((H, W), bool)
    m[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = True
    rle = _enc(m)
    if as_string:
        c = np.asarray(rle["counts"], dtype=np.int32)
        buf = ctypes.create_string_buffer(8 * len(c))
        n = _lib.lib().dgx_rle_to_string(c.ctypes.data_as(ctypes.c_void_p), len(c), buf, 8 * len(c))
        rle["counts"] = buf.raw[:n].decode("ascii")
    return rle


def _hard_problem():
    """6 images x 8 categories at 64 x 96; rectangles, so that the box and the mask task see the same overlaps.  The crafted
    cases live in the rows above y = 44, random filler below."""
    rng = np.random.RandomState(11)
    images = [{"id": i, "height": H, "width": W, "neg_category_ids": [], "not_exhaustive_category_ids": []} for i in range(1, 7)]
    cats = [{"id": c, "frequency": "rcf"[c % 3]} for c in range(1, 9)]
    anns, dets = [], []

    def gt(img, cat, box, area=None, ignore=0, poly=False):
        x, y, w, h = box
        seg = [[x, y, x + w, y, x + w, y + h, x, y + h]] if poly else _rect(box, False)
        anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cat, "bbox": [float(v) for v in box],
                     "area": float(w * h) if area is None else area, "ignore": ignore, "segmentation": seg})

    def det(img, cat, box, score):
        dets.append({"image_id": img, "category_id": cat, "bbox": [float(v) for v in box], "score": score,
                     "segmentation": _rect(box, len(dets) % 3 != 0)})
    # category 1: IoU exactly 0.5; two ground truths at the same IoU; score ties within a group and across images
    gt(1, 1, (10, 10, 20, 10), poly=True)
    det(1, 1, (10, 10, 10, 10), 0.9)
    gt(1, 1, (15, 30, 20, 10))
    gt(1, 1, (25, 30, 20, 10))
    det(1, 1, (20, 30, 20, 10), 0.8)
    gt(2, 1, (30, 20, 16, 16), poly=True)
    det(2, 1, (30, 20, 16, 16), 0.9)
    det(2, 1, (31, 20, 16, 16), 0.9)
    # category 2: an ignored ground truth with the higher IoU behind an unignored match; a detection matched to ignored ground truth
    gt(1, 2, (40, 10, 20, 20))
    gt(1, 2, (42, 10, 20, 20), ignore=1)
    det(1, 2, (42, 10, 20, 20), 0.7)
    gt(2, 2, (5, 5, 10, 10), ignore=1)
    det(2, 2, (5, 5, 10, 10), 0.6)
    # category 3: detections without ground truth (a negative category of image 3), ground truth without detections (image 4)
    images[2]["neg_category_ids"].append(3)
    det(3, 3, (10, 10, 12, 12), 0.55)
    det(3, 3, (50, 20, 9, 14), 0.35)
    gt(4, 3, (20, 5, 30, 30))
    # category 4: areas exactly 32^2 and 96^2
    gt(1, 4, (0, 0, 32, 32), area=float(32 ** 2))
    det(1, 4, (0, 0, 32, 32), 0.5)
    gt(2, 4, (40, 0, 56, 64), area=float(96 ** 2))
    det(2, 4, (0, 0, 96, 96), 0.45)
    det(2, 4, (40, 0, 56, 64), 0.4)
    # category 5: not exhaustive on image 5, with an unmatched detection
    images[4]["not_exhaustive_category_ids"].append(5)
    gt(5, 5, (10, 10, 20, 20))
    det(5, 5, (10, 10, 20, 20), 0.8)
    det(5, 5, (60, 20, 20, 20), 0.75)
    # category 6: neither positive nor negative on image 6 -- dropped by the federated filter; present on image 1
    det(6, 6, (10, 10, 10, 10), 0.99)
    gt(1, 6, (70, 5, 10, 30))
    det(1, 6, (70, 6, 10, 30), 0.3)
    # category 7: more than MAX_DETS detections on image 6
    gt(6, 7, (10, 4, 30, 30))
    gt(6, 7, (50, 4, 30, 30))
    for k in range(MAX_DETS + 8):
        det(6, 7, (10 + 2 * k, 4 + k % 5, 30, 30), float(rng.rand()))
    # category 8: every ground truth larger than 32^2 -- no unignored ground truth in "small" only
    gt(3, 8, (0, 0, 40, 40))
    det(3, 8, (2, 0, 40, 40), 0.65)
    gt(4, 8, (50, 0, 40, 42), ignore=0)
    # filler below y = 44
    for img in range(1, 6):
        for cat in (1, 2, 3, 5, 7):
            if (img, cat) in ((3, 3), (4, 3)):
                continue
            for _ in range(rng.randint(0, 3)):
                w, h = rng.randint(4, 30), rng.randint(4, 18)
                x, y = rng.randint(0, W - w), rng.randint(44, H - h + 1)
                gt(img, cat, (x, y, w, h), ignore=int(rng.rand() < 0.15))
                if rng.rand() < 0.8:
                    det(img, cat, (x + rng.randint(-3, 4), y, max(w + rng.randint(-3, 4), 1), h), float(np.round(rng.rand(), 1)))
            for _ in range(rng.randint(0, 3)):
                w, h = rng.randint(4, 30), rng.randint(4, 18)
                det(img, cat, (rng.randint(0, W - w), rng.randint(44, H - h + 1), w, h), float(np.round(rng.rand(), 1)))
            if rng.rand() < 0.5 and cat not in images[img - 1]["neg_category_ids"]:
                images[img - 1]["neg_category_ids"].append(cat)
    return {"images": images, "categories": cats, "annotations": anns}, dets


@pytest.fixture(scope="module")
def hard():
    gt, dets = _hard_problem()
    out = {"gt": gt, "dets": dets}
    for task in ("bbox", "segm"):
        ev = LE.LVISEval(gt, dets, task, MAX_DETS)
        summary = ev.run()
        inter = {}
        for cat in ev.cat_ids:
            for img in ev.img_ids:
                g, d = ev._gts[img, cat], ev._dts[img, cat]
                if not g and not d:
                    continue
                iou = np.array([[ev._iou(x, y) for y in g] for x in d]).reshape(len(d), len(g)) if g and d else []
                inter[img, cat] = (iou, [ev._evaluate_img(img, cat, r, iou) for r in ev.area_rng])
        out[task] = (ev, summary, inter)
    return out


@pytest.mark.parametrize("task", ["bbox", "segm"])
def test_hard_problem_contains_every_case(hard, task):
    """Each situation the matcher and the accumulation must get right is present, read off the Python evaluator's own
    intermediate results (CPU only; the device is not involved)."""
    ev, _, inter = hard[task]
    gt, dets = hard["gt"], hard["dets"]
    groups = list(inter)
    assert any(ev._dts[k] and not ev._gts[k] for k in groups) and any(ev._gts[k] and not ev._dts[k] for k in groups)
    # score ties within a group and across images of one category
    assert any(len(set(d["score"] for d in ev._dts[k])) < len(ev._dts[k]) for k in groups)
    assert any(set(d["score"] for d in ev._dts[k1]) & set(d["score"] for d in ev._dts[k2])
               for k1 in groups for k2 in groups if k1[1] == k2[1] and k1[0] < k2[0])
    found = dict.fromkeys(["half", "equal", "ignored_ends_scan", "matched_to_ignored", "nel_unmatched"], False)
    for k in groups:
        iou, per_area = inter[k]
        gts, dts = ev._gts[k], ev._dts[k]
        e = per_area[0]
        if len(iou) == 0:
            continue
        ig = np.array([1 if g["ignore"] else 0 for g in gts])      # the "all" range: the ignore flags alone
        ids = np.array([g["id"] for g in gts])
        for di in range(len(dts)):
            m0, m1 = e["dt_matches"][0, di], e["dt_matches"][1, di]
            for gi in range(len(gts)):
                if iou[di, gi] == 0.5 and m0 == ids[gi] and m1 == 0:
                    found["half"] = True                  # matched at the first threshold, not at the second
                for gj in range(gi + 1, len(gts)):
                    if iou[di, gi] == iou[di, gj] >= 0.5 and not ig[gi] and not ig[gj] and m0 == ids[gj]:
                        found["equal"] = True             # the later of two equal IoUs wins
            for t in range(len(ev.iou_thrs)):
                m = e["dt_matches"][t, di]
                if m == 0:
                    continue
                mi = int(np.flatnonzero(ids == m)[0])
                if ig[mi]:
                    assert e["dt_ignore"][t, di]
                    found["matched_to_ignored"] = True
                else:
                    free = [gi for gi in range(len(gts)) if ig[gi] and ids[gi] not in e["dt_matches"][t, :di + 1]]
                    if any(iou[di, gi] > iou[di, mi] for gi in free):
                        found["ignored_ends_scan"] = True
            if k[1] in ev.img_nel[k[0]] and e["dt_matches"][0, di] == 0 and e["dt_ignore"][0, di]:
                found["nel_unmatched"] = True
    assert all(found.values()), found
    # areas exactly on the bounds count in both neighbouring ranges
    for bound, (lo, hi) in ((32 ** 2, (1, 2)), (96 ** 2, (2, 3))):
        hit = [a for a in gt["annotations"] if a["area"] == bound]
        assert hit
        for a in hit:
            k = (a["image_id"], a["category_id"])
            pos = [g["id"] for g in ev._gts[k]].index(a["id"])
            for rng_i in (lo, hi):
                gi_sorted = np.argsort([1 if (g["ignore"] or g["area"] < ev.area_rng[rng_i][0] or g["area"] > ev.area_rng[rng_i][1]) else 0
                                        for g in ev._gts[k]], kind="mergesort")
                assert inter[k][1][rng_i]["gt_ignore"][list(gi_sorted).index(pos)] == 0
    areas = [d["area"] for k in groups for d in ev._dts[k]]
    assert 32 ** 2 in areas and (task == "segm" or 96 ** 2 in areas)
    # the federated filter dropped a category; an image holds more than max_dets detections
    assert any(d["image_id"] in ev.imgs and not ev._dts.get((d["image_id"], d["category_id"])) for d in dets)
    per_img = np.bincount([d["image_id"] for d in dets])
    assert per_img.max() > MAX_DETS
    # a category without unignored ground truth in "small" only
    kk = [k for k in range(len(ev.cat_ids)) if (ev.precision[:, :, k, 1] == -1).all() and (ev.precision[:, :, k, 0] > -1).all()
          and any(g for (i, c), g in ev._gts.items() if c == ev.cat_ids[k])]
    assert kk


def _assert_same(dv, summary, ev, ev_summary):
    np.testing.assert_array_equal(dv.precision, ev.precision)
    np.testing.assert_array_equal(dv.recall, ev.recall)
    assert set(summary) == set(ev_summary)
    for name in ev_summary:
        assert summary[name] == ev_summary[name], name


@pytest.mark.parametrize("task", ["bbox", "segm"])
def test_hard_problem_bits_equal_python(hard, task):
    from divergen_amd.evaluation.lvis_eval_device import LVISEvalDevice
    ev, ev_summary, _ = hard[task]
    dv = LVISEvalDevice(hard["gt"], hard["dets"], task, MAX_DETS)
    summary = dv.run()
    assert (ev.precision > -1).any() and (ev.precision == -1).any()
    _assert_same(dv, summary, ev, ev_summary)
    assert dv.iou_thrs.tolist() == ev.iou_thrs.tolist() and dv.rec_thrs.tolist() == ev.rec_thrs.tolist()
    assert dv.cat_ids == ev.cat_ids and dv.img_ids == ev.img_ids and dv.freq_groups == ev.freq_groups and dv.area_rng == ev.area_rng


@pytest.mark.parametrize("task", ["bbox", "segm"])
@pytest.mark.parametrize("chunk", [1, 6])
def test_chunking_does_not_change_a_bit(hard, task, chunk):
    from divergen_amd.evaluation.lvis_eval_device import LVISEvalDevice
    ev, ev_summary, _ = hard[task]
    dv = LVISEvalDevice(hard["gt"], hard["dets"], task, MAX_DETS, chunk_images=chunk)
    _assert_same(dv, dv.run(), ev, ev_summary)


def test_evaluator_end_to_end_device_equals_python(hard, tmp_path):
    from divergen_amd.data.build import register_lvis_instances
    from divergen_amd.evaluation import LVISEvaluator
    from divergen_amd.structures import Boxes, Instances
    path = tmp_path / "hard.json"
    path.write_text(json.dumps(hard["gt"]))
    register_lvis_instances("lvis_eval_device_gpu_test", str(path), str(tmp_path))
    by_img = {}
    for d in hard["dets"]:
        by_img.setdefault(d["image_id"], []).append(d)
    out = {}
    for on in (False, True):
        ev = LVISEvaluator("lvis_eval_device_gpu_test", None, False, None, max_dets_per_image=MAX_DETS, device_eval=on)
        ev.reset()
        for img, ds in sorted(by_img.items()):
            b = torch.tensor([d["bbox"] for d in ds], dtype=torch.float32)
            b[:, 2:] += b[:, :2]
            rles = [{"size": [H, W], "counts": _rect(d["bbox"], True)["counts"].encode("ascii")} for d in ds]
            inst = Instances((H, W), pred_boxes=Boxes(b), scores=torch.tensor([d["score"] for d in ds], dtype=torch.float32),
                             pred_classes=torch.tensor([d["category_id"] - 1 for d in ds]), pred_masks_rle=rles)
            ev.process([{"image_id": img}], [{"instances": inst}])
        out[on] = ev.evaluate()
    assert set(out[True]) == set(out[False]) == {"bbox", "segm"}
    for task in ("bbox", "segm"):
        assert set(out[True][task]) == set(out[False][task])
        for name, v in out[False][task].items():
            assert v == v and out[True][task][name] == v, (task, name)
        assert out[False][task]["AP"] > 0
