"""float64 restatement of the dynamic classifier (MODEL.DYNAMIC_CLASSIFIER) for the tests, and the inputs of its golden.

  * sample():  _sample_cls_inds (DG custom_rcnn.py:226-247, utils.py:16-28) as include/divergen_hip.h states it for
    dgx_dyn_class_sample: the distinct labels ascending, then the top of prob0 / expo (fp32 division: the keys are fp32), equal keys
    lower index first; cls_id_map.
  * logits() / box_losses() / image_loss(): the predictor on the sampled vocabulary in float64 (zero_shot_classifier.py:69-87,
    detic_fast_rcnn.py:160-304, :342-434).
The `mutant` switches break one rule each; tests/test_host_dynamic_classifier.py shows that each falls outside the bound."""
import numpy as np

import _image_label_ref as IL
import _zeroshot_ref as ZR

NUM_CLASSES, C_FREQ, D, IN = 37, 30, 64, 128
TEMP, USE_BIAS = 50.0, -4.6
SEED = 20261019
BOX_CASES = {"few": dict(S=8, R=48), "many": dict(S=4, R=40)}      # a < S: three classes appear; a > S: six do
IMAGE_LABELS = [[3], [5, 9, 3], [20]]
IMAGE_SIZES = [(200, 300), (240, 180), (128, 160)]
IMAGE_COUNTS = [12, 9, 7]
IMAGE_S = 8
IMAGE_MODES = ("max_size", "max_score")
IMAGE_WEIGHT = 0.1


def _bf(a):
    import torch
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def inputs():
    """Frozen inputs (numpy's legacy RandomState); everything a GEMM reads is bfloat16-representable."""
    rs = np.random.RandomState(SEED)
    d = {}
    d["emb"] = (rs.standard_normal((NUM_CLASSES, D)) * 0.3).astype(np.float32)       # the .npy of class embeddings (C, D)
    fw = (rs.randint(1, 400, C_FREQ).astype(np.float32)) ** 0.5
    fw[[6, 11, 17, 26]] = 0.0                                                         # a few zero weights: never drawn (6: a uniform draw of the 'few' case takes it)
    d["freq_weight"] = fw
    d["linear.weight"] = _bf(rs.standard_normal((D, IN)) * 0.08)
    d["linear.bias"] = _bf(rs.standard_normal(D) * 0.1)
    d["bbox_pred.0.weight"] = _bf(rs.standard_normal((IN, IN)) * 0.1)
    d["bbox_pred.0.bias"] = _bf(rs.standard_normal(IN) * 0.05)
    d["bbox_pred.2.weight"] = _bf(rs.standard_normal((4, IN)) * 0.02)
    d["bbox_pred.2.bias"] = _bf(rs.standard_normal(4) * 0.01)
    d["cls_bias"] = np.full((1,), USE_BIAS, np.float32)
    for name, cls in (("few", [4, 19, 7]), ("many", [1, 5, 8, 13, 21, 29])):
        R = BOX_CASES[name]["R"]
        gt = np.array(cls, np.int64)[rs.randint(0, len(cls), R)]
        gt[:len(cls)] = cls                                                           # every class occurs
        gt[rs.rand(R) < 0.35] = NUM_CLASSES                                           # rows labelled with the background
        gt[:len(cls)] = cls
        d[name + ".gt_classes"] = gt
        d[name + ".x"] = _bf(np.maximum(rs.standard_normal((R, IN)), 0.0))
        xy = rs.rand(R, 2) * 200
        wh = 8 + rs.rand(R, 2) * 100
        prop = np.concatenate([xy, xy + wh], 1)
        gtb = prop + rs.standard_normal((R, 4)) * 4
        gtb[:, 2:] = np.maximum(gtb[:, 2:], gtb[:, :2] + 1)
        d[name + ".prop"], d[name + ".gtb"] = prop.astype(np.float32), gtb.astype(np.float32)
    Ri = sum(IMAGE_COUNTS)
    d["image.x"] = _bf(np.maximum(rs.standard_normal((Ri, IN)), 0.0))
    boxes = []
    for n, (h, w) in zip(IMAGE_COUNTS, IMAGE_SIZES):
        xy = rs.rand(n, 2) * np.array([w, h]) * 0.5
        wh = 8 + rs.rand(n, 2) * np.array([w, h]) * 0.45
        boxes.append(np.concatenate([xy, xy + wh], 1))
    d["image.boxes"] = np.concatenate(boxes).astype(np.float32)
    return d


def sample(labels, prob0, expo, C, num_classes, S, mutant=None):
    """-> inds (n,) int64, cls_id_map (num_classes + 1,) int64, n."""
    labels = np.asarray(labels, np.int64).reshape(-1)
    app = np.unique(labels[(labels >= 0) & (labels < C)])
    a = len(app)
    more = np.zeros(0, np.int64)
    if a < S:
        p = np.asarray(prob0, np.float32)[:C].copy()
        if mutant == "uniform":          # freq_weight ignored
            p[:] = 1.0
        p[app] = 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            keys = np.where(p > 0, p / np.asarray(expo, np.float32)[:C], np.float32(0)).astype(np.float32)
        k = min(S - a, int((keys > 0).sum()))
        order = np.lexsort((np.arange(C), -keys.astype(np.float64)))      # key descending, index ascending
        more = order[:k].astype(np.int64)
    inds = np.concatenate([app, more])
    n = len(inds)
    cls_id_map = np.full(num_classes + 1, n, np.int64)
    cls_id_map[inds] = np.arange(n)
    if mutant == "bg":                   # background mapped to n - 1
        cls_id_map[num_classes] = n - 1
    return inds, cls_id_map, n


def remap(labels, cls_id_map, mutant=None):
    labels = np.asarray(labels, np.int64)
    out = np.where(labels >= 0, cls_id_map[np.clip(labels, 0, len(cls_id_map) - 1)], labels)
    if mutant == "ignore":               # -1 rows mapped to background (torch's cls_id_map[-1])
        out = cls_id_map[labels]
    return out


def zs_weight_of(emb):
    """(C, D) embeddings -> zs_weight (D, C + 1) fp32, as the classifier builds it."""
    import torch
    return ZR.zs_weight_of(torch.from_numpy(np.asarray(emb, np.float32))).numpy()


def sub_vocab(zs_weight, inds):
    """float64 (D, n + 1): the gathered columns re-normalised (F.normalize, eps 1e-12), the zero background last."""
    w = np.asarray(zs_weight, np.float64)[:, list(inds) + [zs_weight.shape[1] - 1]]
    return w / np.maximum(np.sqrt((w * w).sum(0, keepdims=True)), 1e-12)


def logits(x, d, zs_sub):
    h = np.asarray(x, np.float64) @ np.asarray(d["linear.weight"], np.float64).T + np.asarray(d["linear.bias"], np.float64)
    h = TEMP * h / np.maximum(np.sqrt((h * h).sum(1, keepdims=True)), 1e-12)
    return h @ zs_sub + float(d["cls_bias"][0])


def deltas(x, d):
    h = np.maximum(np.asarray(x, np.float64) @ np.asarray(d["bbox_pred.0.weight"], np.float64).T + np.asarray(d["bbox_pred.0.bias"], np.float64), 0)
    return h @ np.asarray(d["bbox_pred.2.weight"], np.float64).T + np.asarray(d["bbox_pred.2.bias"], np.float64)


def box_losses(lg, dl, gt, prop, gtb, weights=ZR.BOX_WEIGHTS):
    """Sigmoid CE over the n class columns summed / rows (rows labelled -1 are no rows); class-agnostic L1 over the foreground, mean;
    the logged accuracies (D2 fast_rcnn.py:88-114)."""
    n = lg.shape[1] - 1
    valid = gt >= 0
    B = max(int(valid.sum()), 1)
    target = np.zeros((len(gt), n + 1))
    target[np.arange(len(gt))[valid], gt[valid]] = 1
    ce = IL.softplus(lg[:, :n]) - lg[:, :n] * target[:, :n]
    loss_cls = float((ce * valid[:, None]).sum() / B)
    fg = valid & (gt < n)
    import torch
    tgt = ZR.get_deltas(torch.from_numpy(np.asarray(prop, np.float64)[fg]), torch.from_numpy(np.asarray(gtb, np.float64)[fg]), weights).numpy()
    l = np.abs(dl[fg] - tgt)
    pred = lg.argmax(1)
    nfg = max(int(fg.sum()), 1)
    stats = np.array([float(((pred == gt) & valid).sum()) / B, float(((pred == gt) & fg).sum()) / nfg, float(((pred == n) & fg).sum()) / nfg])
    return loss_cls, float(l.sum() / max(l.size, 1.0)), stats


def image_loss(lg, boxes, labels_remapped, mode):
    return IL.image_label_loss(lg, None, np.asarray(boxes, np.float64), IMAGE_COUNTS, IMAGE_SIZES, labels_remapped, mode, IMAGE_WEIGHT)
