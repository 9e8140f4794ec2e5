"""CPU restatement of the open-vocabulary box predictor (USE_ZEROSHOT_CLS) for the tests, and the inputs of its golden.

Two modes of the same arithmetic (DG zero_shot_classifier.py:69-87, detic_fast_rcnn.py:160-304,437-466):
  * fp32: what the reference computes -- pinned to tests/golden/zeroshot.npz by tests/test_host_zeroshot.py;
  * bf16 storage (`bf16=True`): every tensor the product STORES as bfloat16 is rounded there -- the `linear` output, the normalised
    rows, the class operand, the GEMM's logits (the fp32 scalar bias is added afterwards), the regressor's hidden rows and its deltas.

The inputs are drawn from numpy's legacy RandomState (a stream NumPy keeps frozen), so the two large weight matrices need not be
stored; every input is bfloat16-representable, so the product's bf16 shadows of them are exact.  The golden stores a checksum."""
import numpy as np
import torch
from torch.nn import functional as F

IN, D, C, R, C2 = 256, 512, 37, 70, 7
USE_BIAS, TEMP = -4.6, 50.0
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
GRAD_ROWS = slice(1, None, 2)        # rows of the two large weight gradients that the golden keeps (file size)
PARAMS = ("linear.weight", "linear.bias", "cls_bias", "bbox_pred.0.weight", "bbox_pred.0.bias", "bbox_pred.2.weight", "bbox_pred.2.bias")


def _bf(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float()


def inputs():
    rs = np.random.RandomState(20261018)
    d = {}
    d["x"] = _bf(np.maximum(rs.standard_normal((R, IN)), 0.0))                     # box-head features: post-ReLU
    d["linear.weight"] = _bf(rs.standard_normal((D, IN)) * 0.05)
    d["linear.bias"] = _bf(rs.standard_normal(D) * 0.1)
    d["bbox_pred.0.weight"] = _bf(rs.standard_normal((IN, IN)) * 0.08)
    d["bbox_pred.0.bias"] = _bf(rs.standard_normal(IN) * 0.05)
    d["bbox_pred.2.weight"] = _bf(rs.standard_normal((4, IN)) * 0.02)
    d["bbox_pred.2.bias"] = _bf(rs.standard_normal(4) * 0.01)
    d["cls_bias"] = torch.full((1,), USE_BIAS, dtype=torch.float32)
    d["emb"] = torch.from_numpy(rs.standard_normal((C, D)).astype(np.float32) * 0.3)       # (C, D): the .npy of class embeddings
    d["emb2"] = torch.from_numpy(rs.standard_normal((C2, D)).astype(np.float32) * 0.3)     # a second vocabulary
    gt = rs.randint(0, C, R)
    gt[rs.rand(R) < 0.4] = C                                                                # background rows
    d["gt_classes"] = torch.from_numpy(gt.astype(np.int64))
    xy = rs.rand(R, 2) * 200
    wh = 8 + rs.rand(R, 2) * 100
    prop = np.concatenate([xy, xy + wh], 1)
    gtb = prop + rs.standard_normal((R, 4)) * 4
    gtb[:, 2:] = np.maximum(gtb[:, 2:], gtb[:, :2] + 1)
    d["prop_boxes"] = torch.from_numpy(prop.astype(np.float32))
    d["gt_boxes"] = torch.from_numpy(gtb.astype(np.float32))
    return d


def checksum(d):
    return np.array([float(d[k].double().sum()) for k in sorted(d)], np.float64)


def rb(t, on):
    return t.to(torch.bfloat16).float() if on else t


def zs_weight_of(emb_cd, norm_weight=True):
    """(C, D) embeddings -> (D, C + 1): transpose, zero background column, column-normalise."""
    w = emb_cd.permute(1, 0).contiguous()
    w = torch.cat([w, w.new_zeros((w.shape[0], 1))], dim=1)
    return F.normalize(w, p=2, dim=0) if norm_weight else w


def classifier_logits(x, p, zs_weight=None, classifier=None, bf16=False, temp=TEMP):
    """zs_weight (D, C + 1) as stored, or classifier (C', D) = a per-call vocabulary -> (R, C + 1) | (R, C')."""
    h = rb(F.linear(x, p["linear.weight"], p["linear.bias"]), bf16)
    if classifier is not None:
        zs = F.normalize(classifier.permute(1, 0).contiguous(), p=2, dim=0)
    else:
        zs = zs_weight
    h = rb(temp * F.normalize(h, p=2, dim=1), bf16)
    y = rb(torch.mm(h, rb(zs, bf16)), bf16)
    return y + p["cls_bias"]


def box_deltas(x, p, bf16=False):
    h = rb(F.relu(F.linear(x, p["bbox_pred.0.weight"], p["bbox_pred.0.bias"])), bf16)
    return rb(F.linear(h, p["bbox_pred.2.weight"], p["bbox_pred.2.bias"]), bf16)


def get_deltas(src, tgt, weights=BOX_WEIGHTS):
    """Box2BoxTransform.get_deltas (D2 box_regression.py)."""
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tx, ty = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    wx, wy, ww, wh = weights
    return torch.stack((wx * (tx - sx) / sw, wy * (ty - sy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)), dim=1)


def losses(logits, deltas, gt_classes, prop, gtb):
    """Sigmoid CE without class weights (fed loss off) summed / B; class-agnostic L1 over the foreground rows, mean."""
    B, Cn = logits.shape[0], logits.shape[1] - 1
    target = logits.new_zeros(B, Cn + 1)
    target[torch.arange(B), gt_classes] = 1
    loss_cls = F.binary_cross_entropy_with_logits(logits[:, :-1], target[:, :Cn], reduction="none").sum() / B
    fg = ((gt_classes >= 0) & (gt_classes < Cn)).nonzero().squeeze(1)
    l = torch.abs(deltas[fg] - get_deltas(prop[fg], gtb[fg]))
    return loss_cls, l.sum() / max(l.numel(), 1.0)


def run(d, bf16=False, grads=True):
    """Forward (+ backward of loss_cls + loss_box_reg) of the whole output layer on the built-in vocabulary."""
    p = {k: d[k].clone().requires_grad_(grads) for k in PARAMS}
    x = d["x"].clone().requires_grad_(grads)
    logits = classifier_logits(x, p, zs_weight=zs_weight_of(d["emb"]), bf16=bf16)
    deltas = box_deltas(x, p, bf16=bf16)
    loss_cls, loss_box = losses(logits, deltas, d["gt_classes"], d["prop_boxes"], d["gt_boxes"])
    out = {"logits": logits.detach(), "deltas": deltas.detach(), "loss_cls": loss_cls.detach(), "loss_box_reg": loss_box.detach()}
    if grads:
        (loss_cls + loss_box).backward()
        out["g.x"] = x.grad
        for k in PARAMS:
            out["g." + k] = p[k].grad
    return out
