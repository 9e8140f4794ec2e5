"""Generate tests/golden/dynamic_classifier.npz: the dynamic classifier (MODEL.DYNAMIC_CLASSIFIER) from the reference's own code.
Run in the authoring container only:

    python tests/golden/make_golden_dynamic.py

On the frozen inputs of tests/_dyncls_ref.inputs() (num_classes 37, len(freq_weight) 30 with four zero weights, D 64, input width
128) it runs
  * the real CustomRCNN._sample_cls_inds -> get_fed_loss_inds (DG/divergen/modeling/meta_arch/custom_rcnn.py:226-247,
    DG/divergen/modeling/utils.py:16-28) for two box cases -- 'few': three classes appear, S 8, five are drawn; 'many': six appear,
    S 4, nothing is drawn -- and one image case (labels [[3], [5, 9, 3], [20]], S 8, uniform weights), each from torch's generator
    seeded with _dyncls_ref.SEED + case index; the Exponential(1) values the generator yields at that position are saved as `expo`;
  * the gather of custom_rcnn.py:161-163 and the real ZeroShotClassifier.forward(classifier=...) inside the real
    DeticFastRCNNOutputLayers (dynamic_classifier=True): logits and deltas;
  * the real .losses (box cases, rows labelled with the background included) with the logged accuracies, and the real
    .image_label_losses under max_size and max_score (image case).
Data only is stored: the seed, inputs, inds, cls_id_map, logits and losses.  The reference is imported through _refload; nothing of it
is copied or restated.  Fixed zip timestamps: two runs give identical bytes."""
import os
import sys
import tempfile
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refload as R  # noqa: E402
import _dyncls_ref as Z  # noqa: E402
from make_golden_blend import save_deterministic  # noqa: E402


def _more_stubs():
    R.install()
    rc = types.ModuleType("detectron2.modeling.meta_arch.rcnn")
    rc.GeneralizedRCNN = type("GeneralizedRCNN", (nn.Module,), {})
    sys.modules["detectron2.modeling.meta_arch.rcnn"] = rc
    R._ns("divergen.modeling.meta_arch", R.DG + "/modeling/meta_arch")
    R._ns("divergen.modeling.text")
    sys.modules["divergen.modeling.text.text_encoder"] = R._Permissive("divergen.modeling.text.text_encoder")


def main():
    _more_stubs()
    cr = R.ref("divergen.modeling.meta_arch.custom_rcnn")
    fr = R.ref("divergen.modeling.roi_heads.detic_fast_rcnn")
    zc = R.ref("divergen.modeling.roi_heads.zero_shot_classifier")
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.box_regression import Box2BoxTransform
    from detectron2.structures import Boxes, Instances
    d = Z.inputs()
    T = {k: torch.from_numpy(v) for k, v in d.items()}
    tmp = tempfile.mkdtemp()
    npy = os.path.join(tmp, "emb.npy")
    np.save(npy, d["emb"])

    def predictor(mode=""):
        cls = zc.ZeroShotClassifier(ShapeSpec(channels=Z.IN), num_classes=Z.NUM_CLASSES, zs_weight_path=npy, zs_weight_dim=Z.D,
                                    use_bias=Z.USE_BIAS, norm_weight=True, norm_temperature=Z.TEMP)
        pred = fr.DeticFastRCNNOutputLayers(ShapeSpec(channels=Z.IN), box2box_transform=Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0)),
                                            num_classes=Z.NUM_CLASSES, cls_agnostic_bbox_reg=True, smooth_l1_beta=0.0, use_sigmoid_ce=True,
                                            use_fed_loss=False, use_zeroshot_cls=True, cls_score=cls, dynamic_classifier=True,
                                            image_label_loss=mode, image_loss_weight=Z.IMAGE_WEIGHT, add_image_box=False)
        sd = pred.state_dict()
        with torch.no_grad():
            for k in ("linear.weight", "linear.bias", "cls_bias", "bbox_pred.0.weight", "bbox_pred.0.bias", "bbox_pred.2.weight", "bbox_pred.2.bias"):
                sd[k if k.startswith("bbox_pred") else "cls_score." + k].copy_(T[k])
        pred.load_state_dict(sd)
        return pred

    out = {"seed": np.int64(Z.SEED)}
    for k, v in d.items():
        out["in." + k] = v

    def sample(case, gt_instances, ann_type, S, C):
        me = types.SimpleNamespace(freq_weight=T["freq_weight"], num_classes=Z.NUM_CLASSES, num_sample_cats=S)
        torch.manual_seed(Z.SEED + case)
        out_expo = torch.empty(C + 1).exponential_(1)          # what the generator yields at this position
        torch.manual_seed(Z.SEED + case)
        inds, cls_id_map = cr.CustomRCNN._sample_cls_inds(me, gt_instances, ann_type)
        return inds, cls_id_map, out_expo

    pred = predictor()
    zs_weight = pred.cls_score.zs_weight
    out["zs_weight"] = zs_weight.clone().numpy()
    for case, name in enumerate(("few", "many")):
        S = Z.BOX_CASES[name]["S"]
        inst = Instances((400, 400))
        inst.proposal_boxes, inst.gt_boxes, inst.gt_classes = Boxes(T[name + ".prop"]), Boxes(T[name + ".gtb"]), T[name + ".gt_classes"]
        targets = Instances((400, 400))
        targets.gt_classes = T[name + ".gt_classes"][T[name + ".gt_classes"] < Z.NUM_CLASSES]       # the ground truth holds no background
        inds, cls_id_map, expo = sample(case, [targets], "box", S, Z.C_FREQ)
        ind_with_bg = inds.tolist() + [-1]
        cls_features = zs_weight[:, ind_with_bg].permute(1, 0).contiguous()
        info = (cls_features, (inds, cls_id_map), None)
        R._STORAGE.scalars.clear()
        scores, deltas = pred(T[name + ".x"], classifier_info=info)[:2]
        losses = pred.losses((scores, deltas), [inst], classifier_info=info)
        st = R._STORAGE.scalars
        out.update({name + ".inds": inds.numpy(), name + ".cls_id_map": cls_id_map.numpy(), name + ".expo": expo.numpy(),
                    name + ".logits": scores.detach().numpy(), name + ".deltas": deltas.detach().numpy(),
                    name + ".loss_cls": losses["loss_cls"].detach().numpy(), name + ".loss_box_reg": losses["loss_box_reg"].detach().numpy(),
                    name + ".stats": np.array([st["fast_rcnn/cls_accuracy"], st["fast_rcnn/fg_cls_accuracy"], st["fast_rcnn/false_negative"]],
                                              np.float64)})
        assert scores.shape == (Z.BOX_CASES[name]["R"], len(inds) + 1)
        assert int((T[name + ".gt_classes"] == Z.NUM_CLASSES).sum()) > 5
    assert len(out["few.inds"]) == 8 and list(out["few.inds"][:3]) == [4, 7, 19] and len(out["many.inds"]) == 6
    assert all(d["freq_weight"][c] > 0 for c in out["few.inds"][3:]) and out["few.inds"].max() < Z.C_FREQ
    # the case the 'freq_weight ignored' mutant of the host test leans on: a uniform draw from the same values takes a zero-weight class
    uni = Z.sample(d["few.gt_classes"][d["few.gt_classes"] < Z.NUM_CLASSES], np.ones(Z.C_FREQ + 1, np.float32), out["few.expo"], Z.C_FREQ,
                   Z.NUM_CLASSES, Z.BOX_CASES["few"]["S"])[0]
    assert any(d["freq_weight"][c] == 0 for c in uni) and list(uni) != list(out["few.inds"])

    # the image case
    gts = []
    for labels in Z.IMAGE_LABELS:
        t = Instances((10, 10))
        t.gt_classes = torch.zeros(0, dtype=torch.long)
        t._pos_category_ids = labels
        gts.append(t)
    inds, cls_id_map, expo = sample(2, gts, "image", Z.IMAGE_S, Z.NUM_CLASSES)
    assert len(inds) == Z.IMAGE_S and list(inds[:4].numpy()) == [3, 5, 9, 20]
    out.update({"image.inds": inds.numpy(), "image.cls_id_map": cls_id_map.numpy(), "image.expo": expo.numpy()})
    cls_features = zs_weight[:, inds.tolist() + [-1]].permute(1, 0).contiguous()
    info = (cls_features, (inds, cls_id_map), None)
    for mode in Z.IMAGE_MODES:
        pred = predictor(mode)
        scores, deltas = pred(T["image.x"], classifier_info=info)[:2]
        props, r0 = [], 0
        for n, size in zip(Z.IMAGE_COUNTS, Z.IMAGE_SIZES):
            p = Instances(size)
            p.proposal_boxes = Boxes(T["image.boxes"][r0:r0 + n])
            p.objectness_logits = torch.zeros(n)
            props.append(p)
            r0 += n
        R._STORAGE.scalars.clear()
        losses = pred.image_label_losses((scores, deltas), props, Z.IMAGE_LABELS, classifier_info=info)
        out["image.logits"] = scores.detach().numpy()
        out["image.%s.image_loss" % mode] = losses["image_loss"].detach().numpy()
        out["image.%s.stats_label" % mode] = np.float64(R._STORAGE.scalars["stats_label"])
        assert float(losses["loss_cls"]) == 0.0 and float(losses["image_loss"]) > 0
    save_deterministic(os.path.join(HERE, "dynamic_classifier.npz"), out)
    print({k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
