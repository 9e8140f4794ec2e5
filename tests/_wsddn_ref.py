"""numpy restatement, in float64, of what include/divergen_hip.h states for dgx_wsddn_loss: the loss, the arg-max rows, both dense
gradients and, per gradient element, the sum of the absolute values of its addends (the condition floor the tests' bounds are relative
to).  Test helper: tests/test_host_wsddn.py pins it on the reference's own outputs (tests/golden/wsddn.npz), the GPU tests hold the
kernel to it.  `inputs()` is the frozen input set the golden file was generated from.

Two values are rounded to float32 where the reference STORES them, because the rounding decides something discrete: sigma =
score.sigmoid() (at a logit of 20 it is exactly 1.0f, so torch's sigmoid backward sigma (1 - sigma) is exactly zero) and the image
score S = sum_r sigma p (the reference clamps that fp32 tensor to [1e-10, 1 - 1e-10], whose bounds round to 1e-10f and exactly 1.0f).
Everything else is float64 on the given (already rounded) inputs.

`mutant` names one deliberate mistake; the host test shows that each of them falls outside the bound the tests use."""
import numpy as np

import _image_label_ref as Z

MUTANTS = ("softmax_invalid", "mean_C", "dup_once", "clamp_grad", "tie_high")
LO, HI = float(np.float32(1e-10)), float(np.float32(1 - 1e-10))
assert HI == 1.0
C = Z.C
WEIGHT = Z.WEIGHT
COUNTS = Z.COUNTS
IMAGE_SIZES = Z.IMAGE_SIZES
LABELS = [Z.LABELS[0], Z.LABELS[1], Z.LABELS[2], Z.LABELS[3], [2, 30, 2]]
COL_ONE, COL_LOW, COL_HIGH, COL_TIE = 10, 17, 22, 13      # see inputs()


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def bce(s, t):
    """torch's binary_cross_entropy per element: the logs clamped below at -100."""
    with np.errstate(divide="ignore"):
        return -(t * np.maximum(np.log(s), -100.0) + (1.0 - t) * np.maximum(np.log(1.0 - s), -100.0))


def wsddn_loss(scores, prop, valid, boxes, counts, image_sizes, labels, weight, upstream=1.0, mutant=None):
    """scores, prop (R, C+1) any float dtype (used as given), valid (R,) or None, labels: per-image lists.
    -> dict(loss, l_image, sel [row relative to the image or -1], stats (5,), dscores, dprop, floor_s, floor_p (R, C+1) float64,
    S [per image: the (C+1,) image scores, None without valid rows])."""
    s, q = np.asarray(scores, np.float64), np.asarray(prop, np.float64)
    R, C1 = s.shape
    B = len(counts)
    valid = np.ones(R, bool) if valid is None else np.asarray(valid).astype(bool)
    boxes = np.asarray(boxes, np.float32)
    ds, dq, fs, fq = (np.zeros((R, C1)) for _ in range(4))
    sel, total, stats, Ss = [], 0.0, np.zeros(5), []
    mean_over = C1 - 1 if mutant == "mean_C" else C1
    r0 = 0
    for i, n in enumerate(counts):
        rows = np.array([r0 + r for r in range(n) if valid[r0 + r]], int)
        labs = list(labels[i])
        if mutant == "dup_once":
            labs = list(dict.fromkeys(labs))
        L = len(labs)
        if not len(rows):
            sel += [-1] * L
            Ss.append(None)
            r0 += n
            continue
        pool = np.arange(r0, r0 + n) if mutant == "softmax_invalid" else rows
        e = np.exp(q[rows] - q[pool].max(0))
        p = e / np.exp(q[pool] - q[pool].max(0)).sum(0)
        sg = f32(Z.sigmoid(s[rows]))
        S = f32((sg * p).sum(0))
        Ss.append(S)
        Sc = np.clip(S, LO, HI)
        inside = np.ones(C1, bool) if mutant == "clamp_grad" else (S >= LO) & (S <= HI)
        acc = 0.0
        K = weight / (B * max(L, 1)) / mean_over * upstream
        for lab in labs:
            if not (0 <= lab < C1):
                sel.append(-1)
                continue
            t = np.zeros(C1)
            t[lab] = 1.0
            acc += bce(Sc, t).sum() / mean_over
            key = sg[:, lab] * p[:, lab]
            k = int(np.argmax(key)) if mutant != "tie_high" else len(key) - 1 - int(np.argmax(key[::-1]))
            pick = int(rows[k] - r0)
            sel.append(pick)
            G = np.where(inside, (Sc - t) / np.maximum((1.0 - Sc) * Sc, 1e-12), 0.0)
            a_s, a_q1, a_q2 = K * G * p * sg * (1.0 - sg), K * G * p * sg, -K * G * p * S
            ds[rows] += a_s
            dq[rows] += a_q1 + a_q2
            fs[rows] += np.abs(K * G * p * sg) * (1.0 + sg)      # the two addends of sigma (1 - sigma), formed from the stored sigma
            fq[rows] += np.abs(a_q1) + np.abs(a_q2)
            b = boxes[r0 + pick].astype(np.float64)
            h, w = image_sizes[i]
            stats = np.array([pick, (b[2] - b[0]) * (b[3] - b[1]) / (h * w), (b[0] + b[2]) / 2 / w, (b[1] + b[3]) / 2 / h,
                              float(Z.sigmoid(s[r0 + pick, lab]))])
        if L:
            total += acc / L
        r0 += n
    l_image = total / B
    return dict(loss=weight * l_image, l_image=l_image, sel=sel, stats=stats, dscores=ds, dprop=dq, floor_s=fs, floor_p=fq, S=Ss)


def worst_ratio(got, ref, floor, rel):
    """max over elements of |got - ref| / (rel * max(|ref|, floor)); elements whose bound is zero must be equal (ratio inf otherwise)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = rel * np.maximum(np.abs(ref), floor)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def inputs():
    """The frozen inputs of tests/golden/wsddn.npz: the row layout, scores and boxes of tests/_image_label_ref.inputs(), proposal scores
    from numpy Generator PCG64 seed 20261019, two rows of the last image invalid, and the constructed cases:
      * image 0 (one row): a logit of 20 in COL_ONE, a column no label names: S is exactly 1.0f in any evaluation order;
      * image 3 (40 rows): COL_TIE (a label): rows 6 and 30 hold the same score and the same proposal score, the largest product;
        COL_LOW: every score near -32, S < 1e-10, the clamp cuts the gradient; COL_HIGH: every score near 7, S near 1 - 1e-3;
        label 21 twice."""
    d = Z.inputs()
    rng = np.random.default_rng(20261019)
    R = sum(COUNTS)
    scores = d["scores"].copy()
    prop = (rng.standard_normal((R, C + 1)) * 1.5).astype(np.float32)
    r3 = COUNTS[0] + COUNTS[1]
    r4 = r3 + COUNTS[3]
    scores[0, COL_ONE] = 20.0
    scores[r3 + 6, COL_TIE] = scores[r3 + 30, COL_TIE] = 9.5
    prop[r3 + 6, COL_TIE] = prop[r3 + 30, COL_TIE] = 6.0
    scores[r3:r4, COL_LOW] = (-32.0 + 0.25 * rng.standard_normal(40)).astype(np.float32)
    scores[r3:r4, COL_HIGH] = (7.0 + 0.05 * rng.standard_normal(40)).astype(np.float32)
    valid = np.ones(R, np.uint8)
    valid[r4 + 2] = valid[r4 + 7] = 0
    return dict(scores=scores, prop=prop, boxes=d["boxes"], valid=valid)


# ---------------------------------------------------------------------------------------------------- the GPU tests' inputs
def case_rows(rng, C1):
    """The row layout of tests/test_gpu_image_labels.py, call A: rows per image 1, 2, 0, 129 (+ 6 for an image without labels); labels
    per image 3, 1, 2 (on the image without rows), 20 with one duplicate, 0.  In the 129-row image rows 100 and 31 hold the same
    score (9.5) and proposal score (6.0, both exact in bf16) in the first label's column: the largest product, twice."""
    counts = [1, 2, 0, 129, 6]
    sizes = [(200, 300), (240, 180), (128, 128), (512, 640), (100, 150)]
    labs = sorted(int(v) for v in rng.choice(C1, 19, replace=False))
    labels = [[0, C1 - 1, int(C1 // 2)], [1], [2, 3], labs + [labs[4]], []]
    R = sum(counts)
    scores = (rng.standard_normal((R, C1)) * 2.0 - 1.0).astype(np.float32)
    prop = (rng.standard_normal((R, C1)) * 1.5).astype(np.float32)
    boxes = np.concatenate([Z.random_boxes(rng, n, s) for n, s in zip(counts, sizes)]).astype(np.float32)
    scores[3 + 100, labs[0]] = scores[3 + 31, labs[0]] = 9.5
    prop[3 + 100, labs[0]] = prop[3 + 31, labs[0]] = 6.0
    return counts, sizes, labels, scores, prop, boxes, None


def case_valid(rng, C1):
    """Call B of the same file: four images of 9 rows; validity bytes remove in turn the last row, a middle row, all rows, all rows
    but one."""
    counts, sizes = [9, 9, 9, 9], [(300, 300)] * 4
    labels = [[int(v) for v in rng.choice(C1, 3, replace=False)] for _ in range(4)]
    scores = (rng.standard_normal((36, C1)) * 2.0 - 1.0).astype(np.float32)
    prop = (rng.standard_normal((36, C1)) * 1.5).astype(np.float32)
    boxes = np.concatenate([Z.random_boxes(rng, 9, s) for s in sizes]).astype(np.float32)
    valid = np.ones(36, np.uint8)
    valid[8] = 0
    valid[9 + 4] = 0
    valid[18:27] = 0
    valid[27:36] = 0
    valid[27 + 5] = 1
    return counts, sizes, labels, scores, prop, boxes, valid


CASE_WIDTHS = (38, 1204, 1454)


def gpu_cases(C1):
    """Both calls for one width, from one generator (seed 300 + C1)."""
    rng = np.random.default_rng(300 + C1)
    return [case_rows(rng, C1), case_valid(rng, C1)]


def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))
