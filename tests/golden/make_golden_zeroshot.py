"""Generate tests/golden/zeroshot.npz: the open-vocabulary box predictor (MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS) from the reference's
own code.  Run in the authoring container only:

    python tests/golden/make_golden_zeroshot.py

The real ZeroShotClassifier (DG/divergen/modeling/roi_heads/zero_shot_classifier.py), the real DeticFastRCNNOutputLayers with
use_zeroshot_cls (detic_fast_rcnn.py:106-118, forward :437-466, losses :160-304, sigmoid CE with the federated loss off) and the
real reset_cls_test (DG/divergen/modeling/utils.py:32-63) run on the inputs of tests/_zeroshot_ref.inputs(): in 256, D 512, 37
classes, 70 rows, a second vocabulary of 7 classes, USE_BIAS -4.6.  Saved: the small inputs (the two large weight matrices come
from the frozen random stream of _zeroshot_ref.inputs(); their checksum is saved), fp32 logits on the built-in and on the per-call
vocabulary, scores and deltas of the whole output layer, loss_cls / loss_box_reg, the gradients of their sum with respect to x and
every parameter (of linear.weight and bbox_pred.0.weight every second row, _zeroshot_ref.GRAD_ROWS, to keep the file small),
zs_weight as constructed and after reset_cls_test, and the state dict's names and shapes.  The reference is imported through
_refload; nothing of it is copied or restated.  Fixed zip timestamps: two runs give identical bytes."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refload as R  # noqa: E402
import _zeroshot_ref as Z  # noqa: E402
from make_golden_blend import save_deterministic  # noqa: E402


def main():
    fr = R.ref("divergen.modeling.roi_heads.detic_fast_rcnn")
    zc = R.ref("divergen.modeling.roi_heads.zero_shot_classifier")
    ut = R.ref("divergen.modeling.utils")
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.box_regression import Box2BoxTransform
    from detectron2.structures import Boxes, Instances
    assert fr.ZeroShotClassifier is zc.ZeroShotClassifier
    d = Z.inputs()
    tmp = tempfile.mkdtemp()
    npy, npy2 = os.path.join(tmp, "emb.npy"), os.path.join(tmp, "emb2.npy")
    np.save(npy, d["emb"].numpy())
    np.save(npy2, d["emb2"].numpy())

    def predictor():
        cls = zc.ZeroShotClassifier(ShapeSpec(channels=Z.IN), num_classes=Z.C, zs_weight_path=npy, zs_weight_dim=Z.D,
                                    use_bias=Z.USE_BIAS, norm_weight=True, norm_temperature=Z.TEMP)
        pred = fr.DeticFastRCNNOutputLayers(ShapeSpec(channels=Z.IN), box2box_transform=Box2BoxTransform(weights=Z.BOX_WEIGHTS),
                                            num_classes=Z.C, cls_agnostic_bbox_reg=True, smooth_l1_beta=0.0, use_sigmoid_ce=True,
                                            use_fed_loss=False, use_zeroshot_cls=True, cls_score=cls)
        return pred

    pred = predictor()
    sd = pred.state_dict()
    out = {"sd_names": np.array(sorted(sd)), "sd_shapes": np.array([",".join(str(s) for s in sd[k].shape) for k in sorted(sd)]),
           "zs_weight": sd["cls_score.zs_weight"].clone(), "checksum": Z.checksum(d)}
    assert sorted(sd) == ["bbox_pred.0.bias", "bbox_pred.0.weight", "bbox_pred.2.bias", "bbox_pred.2.weight", "cls_score.cls_bias",
                          "cls_score.linear.bias", "cls_score.linear.weight", "cls_score.zs_weight"], sorted(sd)
    assert float(sd["cls_score.cls_bias"]) == np.float32(Z.USE_BIAS)
    with torch.no_grad():
        for k in Z.PARAMS:
            sd[k if k.startswith("bbox_pred") else "cls_score." + k].copy_(d[k])
    pred.load_state_dict(sd)
    for k in ("x", "emb", "emb2", "gt_classes", "prop_boxes", "gt_boxes", "cls_bias", "linear.bias", "bbox_pred.0.bias",
              "bbox_pred.2.weight", "bbox_pred.2.bias"):
        out["in." + k] = d[k]

    x = d["x"].clone().requires_grad_(True)
    # the classifier alone: built-in vocabulary, per-call vocabulary (detic_fast_rcnn.py:445-446)
    out["logits"] = pred.cls_score(x).detach()
    out["logits_call"] = pred.cls_score(x, classifier=d["emb2"]).detach()
    assert out["logits"].shape == (Z.R, Z.C + 1) and out["logits_call"].shape == (Z.R, Z.C2)
    # the output layer and its losses
    scores, deltas = pred(x)
    inst = Instances((400, 400))
    inst.proposal_boxes, inst.gt_boxes, inst.gt_classes = Boxes(d["prop_boxes"]), Boxes(d["gt_boxes"]), d["gt_classes"]
    losses = pred.losses((scores, deltas), [inst])
    assert set(losses) == {"loss_cls", "loss_box_reg"}
    (losses["loss_cls"] + losses["loss_box_reg"]).backward()
    out.update(scores=scores.detach(), deltas=deltas.detach(), loss_cls=losses["loss_cls"].detach(),
               loss_box_reg=losses["loss_box_reg"].detach())
    out["g.x"] = x.grad
    named = dict(pred.named_parameters())
    for k in Z.PARAMS:
        g = named[k if k.startswith("bbox_pred") else "cls_score." + k].grad
        out["g." + k] = g[Z.GRAD_ROWS] if k in ("linear.weight", "bbox_pred.0.weight") else g
    assert torch.equal(out["scores"], out["logits"]) and float(out["g.cls_bias"].abs()) > 0
    assert int((d["gt_classes"] == Z.C).sum()) > 10 and int((d["gt_classes"] < Z.C).sum()) > 10

    # reset_cls_test on a three-stage cascade: one shared tensor, roi_heads.num_classes set
    model = types.SimpleNamespace(device="cpu", roi_heads=types.SimpleNamespace(num_classes=Z.C, box_predictor=[pred, predictor(), predictor()]))
    ut.reset_cls_test(model, npy2, Z.C2)
    zs = [p.cls_score.zs_weight for p in model.roi_heads.box_predictor]
    assert model.roi_heads.num_classes == Z.C2 and zs[0] is zs[1] and zs[1] is zs[2] and zs[0].shape == (Z.D, Z.C2 + 1)
    out["zs_weight_reset"] = zs[0].clone()
    save_deterministic(os.path.join(HERE, "zeroshot.npz"), {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
