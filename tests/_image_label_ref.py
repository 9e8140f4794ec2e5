"""numpy restatement, in float64, of what include/divergen_hip.h states for dgx_ws_proposals and dgx_image_label_loss, and of the
cascade hand-over an image-labelled step uses (dgx_cascade_refine without ground truth).  Test helper:
tests/test_host_image_labels.py pins it on the reference's own outputs (tests/golden/image_labels.npz, 1e-5 relative, selected
rows equal); the GPU tests hold the kernels to it.  `inputs()` is the frozen input set the golden file was generated from.

Exactness: what SELECTS a row is restated in the arithmetic the contract names -- box areas in fp32 (`(x2-x1)*(y2-y1)`), scores
as stored -- so equal keys tie exactly as they do on the device (lowest row wins); the min_loss criterion and every value are
float64 on the given (already rounded) inputs."""
import numpy as np

MODES = ("max_size", "max_score", "first", "image", "min_loss")
C = 37                       # classes of the golden case (C + 1 = 38 columns)
WEIGHT = 0.1
IMAGE_SIZES = [(200, 300), (240, 180), (128, 128), (256, 320), (100, 150)]
COUNTS = [1, 2, 0, 40, 9]
LABELS = [[5, 0, 36], [7], [3, 4], [int(v) for v in (1, 2, 3, 5, 8, 13, 21, 34, 36, 0, 4, 9, 16, 25, 35, 7, 14, 28, 21, 11)], []]
WS_K, WS_NUM_PROPS, IMAGE_BOX_SIZE = 12, 5, 0.9
BOX_WEIGHTS = [(10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0)]
SCALE_CLAMP = float(np.log(1000.0 / 16))


def softplus(x):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def area_f32(boxes):
    b = np.asarray(boxes, np.float32)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def image_label_loss(scores, valid, boxes, counts, image_sizes, labels, mode, weight):
    """scores (R, C+1) any float dtype (used as given, in float64), valid (R,) or None, boxes (R, 4), labels: per-image lists.
    -> dict(loss, l_image, sel [flat list, row relative to the image or -1], grad (R, C+1) float64, stats (5,), crit_gap)."""
    s = np.asarray(scores, np.float64)
    R, C1 = s.shape
    B = len(counts)
    valid = np.ones(R, bool) if valid is None else np.asarray(valid).astype(bool)
    boxes = np.asarray(boxes, np.float32)
    grad = np.zeros((R, C1), np.float64)
    sel, total, stats, gap = [], 0.0, np.zeros(5), np.inf
    r0 = 0
    for i, n in enumerate(counts):
        rows = [r for r in range(n) if valid[r0 + r]]
        L = len(labels[i])
        acc = 0.0
        for lab in labels[i]:
            if not rows or not (0 <= lab < C1):
                sel.append(-1)
                continue
            if mode == "first":
                pick = rows[0]
            elif mode == "image":
                pick = rows[-1]
            elif mode == "max_size":
                if len(rows) == 1:
                    pick = rows[0]
                else:
                    a = area_f32(boxes[r0:r0 + n])[rows[:-1]]
                    pick = rows[int(np.argmax(a))]                       # first maximum
            elif mode == "max_score":
                pick = rows[int(np.argmax(np.asarray(scores)[r0:r0 + n][rows, lab]))]
            elif mode == "min_loss":
                crit = softplus(s[r0:r0 + n][rows]).sum(1) - s[r0:r0 + n][rows, lab]
                pick = rows[int(np.argmin(crit))]
                if len(crit) > 1:
                    o = np.sort(crit)
                    gap = min(gap, (o[1] - o[0]) / abs(o[0]))
            else:
                raise ValueError(mode)
            sel.append(pick)
            row = s[r0 + pick]
            acc += softplus(row).sum() - row[lab]
            g = sigmoid(row)
            g[lab] -= 1.0
            grad[r0 + pick] += weight / (B * L) * g
            b = boxes[r0 + pick].astype(np.float64)
            h, w = image_sizes[i]
            stats = np.array([pick, (b[2] - b[0]) * (b[3] - b[1]) / (h * w), (b[0] + b[2]) / 2 / w, (b[1] + b[3]) / 2 / h,
                              sigmoid(row[lab])])
        if L:
            total += acc / L
        r0 += n
    l_image = total / B
    return dict(loss=weight * l_image, l_image=l_image, sel=sel, grad=grad, stats=stats, crit_gap=gap)


def image_box(size, f):
    h, w = size
    return np.array([w * (1. - f) / 2., h * (1. - f) / 2., w * (1. - (1. - f) / 2.), h * (1. - (1. - f) / 2.)], np.float64).astype(np.float32)


def clip(boxes, size):
    b = np.array(boxes, np.float32)
    h, w = size
    b[:, 0::2] = np.clip(b[:, 0::2], 0, w)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, h)
    return b


def ws_proposals(boxes, scores, valid, image_sizes, num_props, add_image_box, f):
    """boxes (B, K, 4), scores (B, K), valid (B, K) -> (B*Ko, 4) f32, (B*Ko,) f32, (B*Ko,) uint8."""
    B, K = scores.shape
    Ko = num_props + (1 if add_image_box else 0)
    ob, ol, ov = np.zeros((B, Ko, 4), np.float32), np.zeros((B, Ko), np.float32), np.zeros((B, Ko), np.uint8)
    for i in range(B):
        idx = [k for k in range(K) if valid is None or valid[i, k]][:num_props]
        ob[i, :len(idx)] = clip(boxes[i, idx], image_sizes[i])
        ol[i, :len(idx)] = scores[i, idx]
        ov[i, :len(idx)] = 1
        if add_image_box:
            ob[i, num_props], ol[i, num_props], ov[i, num_props] = image_box(image_sizes[i], f), 1.0, 1
    return ob.reshape(-1, 4), ol.reshape(-1), ov.reshape(-1)


def refine(boxes, deltas, valid, counts, image_sizes, weights, scale_clamp=SCALE_CLAMP):
    """One cascade hand-over without ground truth: apply_deltas (class-agnostic, box_regression.py:76-118) in float64, clip,
    valid &= non-empty."""
    b, d = np.asarray(boxes, np.float64), np.asarray(deltas, np.float64)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cx, cy = b[:, 0] + 0.5 * w, b[:, 1] + 0.5 * h
    dx, dy = d[:, 0] / weights[0], d[:, 1] / weights[1]
    dw, dh = np.minimum(d[:, 2] / weights[2], scale_clamp), np.minimum(d[:, 3] / weights[3], scale_clamp)
    pcx, pcy, pw, ph = dx * w + cx, dy * h + cy, np.exp(dw) * w, np.exp(dh) * h
    out = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 1)
    r0 = 0
    for n, (ih, iw) in zip(counts, image_sizes):
        out[r0:r0 + n, 0::2] = np.clip(out[r0:r0 + n, 0::2], 0, iw)
        out[r0:r0 + n, 1::2] = np.clip(out[r0:r0 + n, 1::2], 0, ih)
        r0 += n
    ok = (out[:, 2] - out[:, 0] > 0) & (out[:, 3] - out[:, 1] > 0)
    if valid is not None:
        ok &= np.asarray(valid).astype(bool)
    return out, ok.astype(np.uint8)


def random_boxes(rng, n, size, lo=8.0):
    h, w = size
    x1, y1 = rng.uniform(0, w - lo - 1, n), rng.uniform(0, h - lo - 1, n)
    x2, y2 = x1 + rng.uniform(lo, w - x1), y1 + rng.uniform(lo, h - y1)
    return np.stack([x1, y1, np.minimum(x2, w), np.minimum(y2, h)], 1).astype(np.float32)


def inputs():
    """The frozen inputs of tests/golden/image_labels.npz (numpy Generator PCG64, seed 20261018)."""
    rng = np.random.default_rng(20261018)
    R = sum(COUNTS)
    scores = (rng.standard_normal((R, C + 1)) * 2.0 - 1.0).astype(np.float32)
    boxes = np.concatenate([random_boxes(rng, n, s) for n, s in zip(COUNTS, IMAGE_SIZES)]).astype(np.float32)
    r3, r4 = COUNTS[0] + COUNTS[1], COUNTS[0] + COUNTS[1] + COUNTS[3]
    # an exact area tie for the maximum among all rows but the last of image 3 (rows 4 and 17: 192 x 100 and 100 x 192) ...
    boxes[r3 + 4] = [10.0, 20.0, 202.0, 120.0]
    boxes[r3 + 17] = [50.0, 30.0, 150.0, 222.0]
    boxes[r3:r4][np.setdiff1d(np.arange(40), [4, 17]), 2:] = np.minimum(
        boxes[r3:r4][np.setdiff1d(np.arange(40), [4, 17]), 2:], boxes[r3:r4][np.setdiff1d(np.arange(40), [4, 17]), :2] + 120.0)
    boxes[r4 - 1] = [0.0, 0.0, 320.0, 256.0]        # ... and the LAST row is larger than either: it must not be taken
    # ... and an exact score tie for the maximum of label 13 (rows 6 and 30 of image 3)
    scores[r3 + 6, 13] = scores[r3 + 30, 13] = 9.5
    deltas = [(rng.standard_normal((R, 4)) * 0.5).astype(np.float32) for _ in range(3)]
    deltas[0][r3 + 2] = [40.0, 0.0, 0.0, 0.0]       # pushed out of the image: clipped to an empty box, dropped from stage 1 on
    deltas[1][r3 + 11] = [0.0, -60.0, 0.0, 0.0]
    deltas[0][r4 + 3] = [0.0, 0.0, 9.0, 9.0]        # beyond the scale clamp
    wb = np.stack([random_boxes(rng, WS_K, s) for s in IMAGE_SIZES[:3]])
    wb[0, 1] = [-5.0, -3.0, 400.0, 150.0]           # clipped on every side of a 200 x 300 image
    wb[1, 0] = [170.0, 230.0, 190.0, 260.0]
    wv = np.ones((3, WS_K), np.uint8)
    wv[0, [0, 3]] = 0                                # holes in the list: the order of the others is kept
    wv[1, 3:] = 0                                    # a short list (3 < WS_NUM_PROPS): padded
    wv[2] = 0                                        # an empty list
    ws = np.sort(rng.uniform(0.05, 0.99, (3, WS_K)).astype(np.float32), axis=1)[:, ::-1].copy()
    return dict(scores=scores, boxes=boxes, deltas=deltas, ws_boxes=wb.astype(np.float32), ws_scores=ws, ws_valid=wv)


# ---------------------------------------------------------------------------------------------------- loader side
def dataset_dicts(sizes, ann, seed=7):
    """Synthetic dataset dicts of several sources, concatenated: `dataset_source`, width / height of both orientations,
    box sources with `annotations`, image sources with `pos_category_ids` (a long-tailed class distribution)."""
    rng = np.random.default_rng(seed)
    out = []
    for src, (n, a) in enumerate(zip(sizes, ann)):
        for k in range(n):
            w, h = (640, 480) if rng.random() < 0.6 else (480, 640)
            if rng.random() < 0.1:
                w = h = 512
            cats = sorted(set(int(c) for c in np.minimum(rng.geometric(0.12, size=int(rng.integers(1, 4))) - 1, 29)))
            d = {"file_name": "s%d_%d.jpg" % (src, k), "image_id": src * 100000 + k, "width": w, "height": h, "dataset_source": src}
            if a == "box":
                d["annotations"] = [{"category_id": c, "bbox": [1.0, 2.0, 30.0, 40.0], "bbox_mode": "XYWH_ABS"} for c in cats]
            else:
                d["annotations"] = []
                d["pos_category_ids"] = cats
            out.append(d)
    return out
