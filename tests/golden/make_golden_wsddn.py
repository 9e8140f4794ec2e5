"""Generate tests/golden/wsddn.npz: the WSDDN image-label loss and the proposal-score branch from the reference's own code.  Run in
the authoring container only:

    python tests/golden/make_golden_wsddn.py

On the frozen inputs of tests/_wsddn_ref.inputs() it runs the real DeticFastRCNNOutputLayers (DG/divergen/modeling/roi_heads/
detic_fast_rcnn.py) built with with_softmax_prop=True, image_label_loss='wsddn':
  * image_label_losses (:342-434 with `_wsddn_loss`, :509-521): image_loss, stats_l_image, the five logged statistics, the gradients
    of image_loss with respect to the scores and to the proposal scores, and the row each (image, label) returned.  The reference
    has no validity bytes: it is given the valid rows of each image, and the row it returns is mapped back to the full list;
  * the constructor: every `prop_score.*` parameter after init (names and shapes are what the tests read);
  * forward (:437-466) of a predictor with fixed weights on fixed rows: its three outputs.
It also measures how far the reference's OWN fp32 evaluation lies from the float64 restatement (tests/_wsddn_ref.py) in the form the
tests' bound has, |got - ref| <= rtol * max(|ref|, floor), on the golden inputs and on the inputs of the GPU tests, and records the
worst ratios: the tests' rtol comes from these numbers, never from the kernel's output.
`_wsddn_loss` returns its row as a 0-d tensor where the five other rules return `.item()`; image_label_losses then indexes Instances with
it, which this detectron2 refuses ("Indexing on Boxes with 0 failed to return a matrix").  The recording wrapper hands the same index
on as a Python int, as the other rules do; the loss, its gradients and the index itself are the reference's own.
The reference is imported through _refload; nothing of it is copied or restated.  Fixed zip timestamps: two runs give identical
bytes.  The cases the tests rely on are asserted to occur."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refload as R  # noqa: E402
import _wsddn_ref as W  # noqa: E402
from make_golden_blend import save_deterministic  # noqa: E402
from make_golden_image_labels import _more_stubs  # noqa: E402


def build(fr, channels=8, **kw):
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.box_regression import Box2BoxTransform
    return fr.DeticFastRCNNOutputLayers(ShapeSpec(channels=channels), box2box_transform=Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0)),
                                        num_classes=W.C, cls_agnostic_bbox_reg=True, smooth_l1_beta=0.0, use_sigmoid_ce=True,
                                        image_label_loss="wsddn", with_softmax_prop=True, image_loss_weight=W.WEIGHT, add_image_box=True,
                                        **kw)


def run_reference(pred, scores, prop, valid, boxes, counts, sizes, labels):
    """The reference on the valid rows -> loss, l_image, stats, gradients scattered back to all rows (float32), selected rows."""
    from detectron2.structures import Boxes, Instances
    valid = np.ones(len(scores), bool) if valid is None else np.asarray(valid).astype(bool)
    keep = np.nonzero(valid)[0]
    s = torch.from_numpy(np.ascontiguousarray(scores[keep])).clone().requires_grad_(True)
    q = torch.from_numpy(np.ascontiguousarray(prop[keep])).clone().requires_grad_(True)
    props, r0, alive = [], 0, []
    for n, size in zip(counts, sizes):
        rows = [r for r in range(n) if valid[r0 + r]]
        p = Instances(size)
        p.proposal_boxes = Boxes(torch.from_numpy(np.ascontiguousarray(boxes[[r0 + r for r in rows]]).reshape(-1, 4)))
        p.objectness_logits = torch.zeros(len(rows))
        props.append(p)
        alive.append(rows)
        r0 += n
    R._STORAGE.scalars.clear()
    log, rule = [], pred._wsddn_loss

    def recorded(*a):
        loss, ind = rule(*a)
        log.append(int(ind))
        return loss, int(ind)      # (see the module docstring: the 0-d tensor the rule returns cannot index Instances)
    pred._wsddn_loss = recorded
    try:
        losses = pred.image_label_losses((s, None, q), props, labels)
    finally:
        del pred._wsddn_loss
    assert set(losses) == {"image_loss", "loss_cls", "loss_box_reg"}
    assert float(losses["loss_cls"]) == 0.0 and float(losses["loss_box_reg"]) == 0.0
    losses["image_loss"].backward()
    st = R._STORAGE.scalars
    sel, it = [], iter(log)
    for rows, ls in zip(alive, labels):
        sel += [rows[next(it)] if rows else -1 for _ in ls]
    assert next(it, None) is None
    stats = np.array([st["pool_stats"], st["stats_select_size"], st["stats_select_x"], st["stats_select_y"], st["stats_max_label_score"]], np.float64)
    last = [rows for rows, ls in zip(alive, labels) if rows and ls][-1]
    stats[0] = last[int(stats[0])]          # pool_stats is the returned row: mapped back like the others
    ds, dq = np.zeros(scores.shape, np.float32), np.zeros(prop.shape, np.float32)
    ds[keep], dq[keep] = s.grad.numpy(), q.grad.numpy()
    return dict(loss=losses["image_loss"].detach().numpy(), l_image=np.float64(st["stats_l_image"]), stats=stats, dscores=ds, dprop=dq,
                sel=np.array(sel, np.int64))


def ratios(ref32, r64):
    """Worst |reference fp32 - float64| in units of 1e-5 * max(|float64|, floor)."""
    return dict(loss=abs(float(ref32["loss"]) - r64["loss"]) / (1e-5 * abs(r64["loss"])),
                dscores=W.worst_ratio(ref32["dscores"], r64["dscores"], r64["floor_s"], 1e-5),
                dprop=W.worst_ratio(ref32["dprop"], r64["dprop"], r64["floor_p"], 1e-5))


def main():
    _more_stubs()
    fr = R.ref("divergen.modeling.roi_heads.detic_fast_rcnn")
    d = W.inputs()
    out = {}
    torch.manual_seed(20261019)
    pred = build(fr)
    for n, v in pred.state_dict().items():
        if n.startswith("prop_score."):
            out["init." + n] = v.numpy().copy()
    assert sorted(k for k in out) == ["init.prop_score.0.bias", "init.prop_score.0.weight", "init.prop_score.2.bias", "init.prop_score.2.weight"]
    g = run_reference(pred, d["scores"], d["prop"], d["valid"], d["boxes"], W.COUNTS, W.IMAGE_SIZES, W.LABELS)
    out.update({"wsddn." + k: v for k, v in g.items()})
    r64 = W.wsddn_loss(d["scores"], d["prop"], d["valid"], d["boxes"], W.COUNTS, W.IMAGE_SIZES, W.LABELS, W.WEIGHT)
    # ---- the cases the tests lean on occur
    r3 = W.COUNTS[0] + W.COUNTS[1]
    off = sum(len(l) for l in W.LABELS[:3])
    assert sorted(W.COUNTS) == [0, 1, 2, 9, 40] and W.LABELS[3].count(21) == 2 and d["valid"].sum() == len(d["valid"]) - 2
    assert g["sel"][off + W.LABELS[3].index(W.COL_TIE)] == 6, "exact arg-max tie: the lower row"
    assert r64["sel"] == g["sel"].tolist()
    S0, S3 = r64["S"][0], r64["S"][3]
    assert S0[W.COL_ONE] == 1.0 and W.COL_ONE not in W.LABELS[0]
    assert 0 < S3[W.COL_LOW] < W.LO and abs((1 - S3[W.COL_HIGH]) - 1e-3) < 2e-4
    assert not g["dscores"][r3:r3 + 40, W.COL_LOW].any() and not g["dprop"][r3:r3 + 40, W.COL_LOW].any(), "the clamp cuts the gradient"
    assert g["dscores"][0, W.COL_ONE] == 0 and g["dprop"][0, W.COL_ONE] == 0, "the saturated column has a zero gradient"
    assert g["sel"][sum(len(l) for l in W.LABELS[:2]):off].tolist() == [-1, -1], "an image without rows"
    m = ratios(g, r64)
    print("golden inputs: reference fp32 vs float64, worst ratio at rtol 1e-5:", m)
    out["measured.golden"] = np.array([m["loss"], m["dscores"], m["dprop"]], np.float64)
    # ---- the same measurement on the inputs of the GPU tests, as stored in fp32 and in bf16
    worst = np.zeros(3)
    for C1 in W.CASE_WIDTHS:
        for rnd in (lambda a: a, W.bf16_round):
            for counts, sizes, labels, scores, prop, boxes, valid in W.gpu_cases(C1):
                sc, pr = rnd(scores), rnd(prop)
                pc = build(fr)
                pc.num_classes = C1 - 1
                g32 = run_reference(pc, sc, pr, valid, boxes, counts, sizes, labels)
                c64 = W.wsddn_loss(sc, pr, valid, boxes, counts, sizes, labels, W.WEIGHT)
                assert g32["sel"].tolist() == c64["sel"]
                mm = ratios(g32, c64)
                worst = np.maximum(worst, [mm["loss"], mm["dscores"], mm["dprop"]])
    print("GPU test inputs: reference fp32 vs float64, worst ratio at rtol 1e-5 (loss, dscores, dprop):", worst)
    out["measured.cases"] = worst
    # ---- forward with fixed weights (C + 1 = 38 outputs, 16 input channels)
    torch.manual_seed(7)
    p2 = build(fr, channels=16)
    with torch.no_grad():
        p2.prop_score[2].weight.normal_(0, 0.2)      # (the init's 0.001 would leave nothing to compare)
        p2.prop_score[2].bias.normal_(0, 0.2)
        x = torch.randn(11, 16)
        y = p2(x)
    assert len(y) == 3
    for n, v in p2.state_dict().items():
        out["fwd.param." + n] = v.numpy().copy()
    out["fwd.x"] = x.numpy()
    for n, v in zip(("scores", "deltas", "prop_scores"), y):
        out["fwd." + n] = v.numpy()
    save_deterministic(os.path.join(HERE, "wsddn.npz"), out)


if __name__ == "__main__":
    main()
