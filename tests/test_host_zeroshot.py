"""Host tests of the open-vocabulary box predictor (MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS): the CPU restatement against the
reference's own outputs (tests/golden/zeroshot.npz), the module's state dict and zs_weight, reset_cls_test, the refusals and the
unchanged default."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _zeroshot_ref as Z  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden):
    return golden("zeroshot")


@pytest.fixture(scope="module")
def data(gold):
    d = Z.inputs()
    assert np.array_equal(Z.checksum(d), gold["checksum"]), "the frozen input stream changed"
    for k in gold.files:
        if k.startswith("in."):
            assert np.array_equal(d[k[3:]].numpy(), gold[k]), k
    return d


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    return float((a.detach().double() - b.double()).norm() / b.double().norm())


def _predictor(tmp_path, d, **kw):
    from divergen_amd.modeling import ShapeSpec
    from divergen_amd.modeling.box_regression import Box2BoxTransform
    from divergen_amd.modeling.roi_heads.detic_fast_rcnn import DeticFastRCNNOutputLayers
    from divergen_amd.modeling.roi_heads.zero_shot_classifier import ZeroShotClassifier
    npy = str(tmp_path / "emb.npy")
    np.save(npy, d["emb"].numpy())
    cls = ZeroShotClassifier(ShapeSpec(channels=Z.IN), num_classes=Z.C, zs_weight_path=kw.pop("zs_weight_path", npy), zs_weight_dim=Z.D,
                             use_bias=Z.USE_BIAS, norm_weight=True, norm_temperature=Z.TEMP)
    args = dict(box2box_transform=Box2BoxTransform(weights=Z.BOX_WEIGHTS), num_classes=Z.C, cls_agnostic_bbox_reg=True,
                smooth_l1_beta=0.0, use_sigmoid_ce=True, use_fed_loss=False, use_zeroshot_cls=True, cls_score=cls)
    args.update(kw)
    return DeticFastRCNNOutputLayers(ShapeSpec(channels=Z.IN), **args)


def load_inputs(pred, d):
    sd = pred.state_dict()
    for k in Z.PARAMS:
        sd[k if k.startswith("bbox_pred") else "cls_score." + k] = d[k].clone()
    pred.load_state_dict(sd, strict=True)
    return pred


def test_restatement_fp32_reproduces_the_reference(gold, data):
    o = Z.run(data, bf16=False)
    for k in ("logits", "deltas", "loss_cls", "loss_box_reg", "g.x"):
        assert rel(o[k], T(gold[k])) <= 1e-5, k
    assert np.array_equal(gold["scores"], gold["logits"])
    for k in Z.PARAMS:
        g = o["g." + k]
        g = g[Z.GRAD_ROWS] if k in ("linear.weight", "bbox_pred.0.weight") else g
        assert rel(g, T(gold["g." + k])) <= 1e-5, k
    call = Z.classifier_logits(data["x"], data, classifier=data["emb2"])
    assert call.shape == (Z.R, Z.C2) and rel(call, T(gold["logits_call"])) <= 1e-5


def test_restatement_bf16_storage_stays_near_the_reference(gold, data):
    """The reference's arithmetic rounded to bfloat16 where the product stores bfloat16 stays within 2.5e-4 relative of the golden
    loss_cls -- which leaves the GPU test's 1e-3 a factor of four.  Measured on this fixture: loss_cls 1.28e-4, loss_box_reg 1.05e-4,
    worst logit error 0.027 (logits in -11.1 .. 2.7)."""
    o = Z.run(data, bf16=True, grads=False)
    e = abs(float(o["loss_cls"]) - float(gold["loss_cls"])) / abs(float(gold["loss_cls"]))
    print("bf16-storage loss_cls relative error %.3e" % e)
    assert e <= 2.5e-4
    # each rounding point does round: the stored tensors are bfloat16-representable
    lg = Z.classifier_logits(data["x"], dict(data, cls_bias=torch.zeros(1)), zs_weight=Z.zs_weight_of(data["emb"]), bf16=True)
    assert torch.equal(lg + data["cls_bias"], o["logits"])
    assert torch.equal(lg, lg.to(torch.bfloat16).float()) and torch.equal(o["deltas"], o["deltas"].to(torch.bfloat16).float())


def test_state_dict_names_shapes_and_strict_load(gold, data, tmp_path):
    pred = _predictor(tmp_path, data)
    sd = pred.state_dict()
    assert sorted(sd) == list(gold["sd_names"])
    assert [",".join(str(s) for s in sd[k].shape) for k in sorted(sd)] == list(gold["sd_shapes"])
    assert sd["cls_score.zs_weight"].dtype == torch.float32 and "cls_score.zs_weight" not in dict(pred.named_parameters())
    fresh = {k: torch.randn_like(v) for k, v in sd.items()}
    assert not _predictor(tmp_path, data).load_state_dict(fresh, strict=True).missing_keys
    # no arena group, no joint GEMM; the fused losses / cascade kernels stay available (sigmoid CE, four delta columns)
    assert pred.forward_joint(data["x"]) is None and pred.fused_supported
    assert all(not hasattr(p, "_dgx_group") for p in pred.parameters())
    from divergen_amd.layers.box_stage import box_stage_supported
    assert not box_stage_supported(types.SimpleNamespace(fcs=[pred.bbox_pred[0], pred.bbox_pred[0]]), pred)
    # the reference's initialisation of the regressor's last layer
    assert float(pred.bbox_pred[2].bias.detach().abs().max()) == 0 and 5e-4 < float(pred.bbox_pred[2].weight.detach().std()) < 2e-3


def test_host_forward_and_losses_match_the_reference(gold, data, tmp_path):
    pred = load_inputs(_predictor(tmp_path, data), data)
    x = data["x"].clone().requires_grad_(True)
    scores, deltas = pred(x)
    assert rel(scores, T(gold["scores"])) <= 1e-6 and rel(deltas, T(gold["deltas"])) <= 1e-6
    call, _ = pred(x, classifier_info=(data["emb2"], None, None))
    assert call.shape == (Z.R, Z.C2) and rel(call, T(gold["logits_call"])) <= 1e-6
    from divergen_amd.structures import Boxes, Instances
    from divergen_amd.utils.events import EventStorage
    inst = Instances((400, 400), proposal_boxes=Boxes(data["prop_boxes"]), gt_boxes=Boxes(data["gt_boxes"]), gt_classes=data["gt_classes"])
    with EventStorage(0):
        losses = pred.losses((scores, deltas), [inst])
    assert abs(float(losses["loss_cls"]) - float(gold["loss_cls"])) <= 1e-5 * float(gold["loss_cls"])
    assert abs(float(losses["loss_box_reg"]) - float(gold["loss_box_reg"])) <= 1e-5 * float(gold["loss_box_reg"])
    (losses["loss_cls"] + losses["loss_box_reg"]).backward()
    assert rel(x.grad, T(gold["g.x"])) <= 1e-5
    assert rel(pred.cls_score.cls_bias.grad, T(gold["g.cls_bias"])) <= 1e-5
    assert pred.cls_score.zs_weight.grad is None


def test_zs_weight_bit_equal_after_construction_and_reset(gold, data, tmp_path):
    from divergen_amd.modeling.utils import reset_cls_test
    preds = [_predictor(tmp_path, data) for _ in range(3)]
    assert np.array_equal(preds[0].cls_score.zs_weight.numpy(), gold["zs_weight"])
    model = types.SimpleNamespace(device=torch.device("cpu"), roi_heads=types.SimpleNamespace(num_classes=Z.C, box_predictor=preds))
    npy2 = str(tmp_path / "emb2.npy")
    np.save(npy2, data["emb2"].numpy())
    img0 = preds[0].cls_score.zs_image()[0]
    reset_cls_test(types.SimpleNamespace(module=model), npy2, Z.C2)              # a wrapped model
    zs = [p.cls_score.zs_weight for p in preds]
    assert model.roi_heads.num_classes == Z.C2 and zs[0] is zs[1] and zs[1] is zs[2]
    assert np.array_equal(zs[0].numpy(), gold["zs_weight_reset"])
    assert "cls_score.zs_weight" in preds[1].state_dict()
    # the cached operand image follows the buffer: replaced by the reset, rewritten by a load
    img1 = preds[0].cls_score.zs_image()[0]
    assert img0.shape == (40, Z.D) and img1.shape == (8, Z.D) and float(img1[Z.C2:].abs().max()) == 0
    assert torch.equal(img1[:Z.C2 + 1], zs[0].t().to(torch.bfloat16))
    sd = preds[0].state_dict()
    sd["cls_score.zs_weight"] = torch.ones_like(sd["cls_score.zs_weight"])
    preds[0].load_state_dict(sd)
    assert float(preds[0].cls_score.zs_image()[0][:Z.C2 + 1].float().min()) == 1.0
    # a tensor (D, C) instead of a path, back to the first vocabulary
    reset_cls_test(model, data["emb"].permute(1, 0).contiguous(), Z.C)
    assert model.roi_heads.num_classes == Z.C and np.array_equal(preds[2].cls_score.zs_weight.numpy(), gold["zs_weight"])
    with pytest.raises(ValueError, match="num_classes"):
        reset_cls_test(model, npy2, Z.C)


def test_refusals_name_their_keys(data, tmp_path):
    with pytest.raises(NotImplementedError, match="ZEROSHOT_WEIGHT_PATH 'rand'"):
        _predictor(tmp_path, data, zs_weight_path="rand")
    with pytest.raises(NotImplementedError, match="BBOX_REG_LOSS_TYPE"):
        _predictor(tmp_path, data, box_reg_loss_type="giou")
    pred = _predictor(tmp_path, data)
    with pytest.raises(NotImplementedError, match=r"classifier_info\[2\]"):
        pred(data["x"], classifier_info=(None, None, data["emb2"]))
    from divergen_amd.config import get_cfg
    from divergen_amd.modeling.utils import ResetClsTestsError, reset_cls_vocabularies
    cfg = get_cfg()
    assert reset_cls_vocabularies(cfg) is None
    cfg.MODEL.RESET_CLS_TESTS = True
    cfg.DATASETS.TEST = ("a", "b")
    cfg.MODEL.TEST_CLASSIFIERS, cfg.MODEL.TEST_NUM_CLASSES = ["a.npy"], [5, 6]
    with pytest.raises(ResetClsTestsError, match="TEST_CLASSIFIERS"):
        reset_cls_vocabularies(cfg)
    cfg.MODEL.TEST_CLASSIFIERS = ["a.npy", "b.npy"]
    assert reset_cls_vocabularies(cfg) == [("a", "a.npy", 5), ("b", "b.npy", 6)]


def test_config_builds_the_open_vocabulary_predictor_and_the_default_is_unchanged(data, tmp_path):
    from divergen_amd.config import get_cfg
    from divergen_amd.layers.linear_ops import Linear
    from divergen_amd.modeling import ShapeSpec
    from divergen_amd.modeling.roi_heads.detic_fast_rcnn import DeticFastRCNNOutputLayers
    from divergen_amd.modeling.roi_heads.zero_shot_classifier import ZeroShotClassifier
    root = os.path.dirname(HERE)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(root, "configs", "DiverGen_swinL.yaml"))
    cfg.merge_from_list(["MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", os.path.join(root, "configs", "metadata", "lvis_v1_train_cat_info.json")])
    assert cfg.MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS is False
    pred = DeticFastRCNNOutputLayers(cfg, ShapeSpec(channels=Z.IN))
    assert sorted(k for k, _ in pred.named_parameters()) == ["bbox_pred.bias", "bbox_pred.weight", "cls_score.bias", "cls_score.weight"]
    assert type(pred.cls_score) is Linear and type(pred.bbox_pred) is Linear and pred.cls_score.out_features == cfg.MODEL.ROI_HEADS.NUM_CLASSES + 1
    w, b = pred.cls_score.weight, pred.cls_score.bias
    assert w._dgx_group_members == (w, pred.bbox_pred.weight) and b._dgx_group_members == (b, pred.bbox_pred.bias)
    assert w._dgx_group[1:] == (0, 8) and pred.bbox_pred.weight._dgx_group[0] == w._dgx_group[0]
    assert pred.fused_supported and not pred.use_zeroshot_cls
    # the key on: the reference's from_config keys
    npy = str(tmp_path / "emb.npy")
    np.save(npy, data["emb"].numpy())
    cfg.merge_from_list(["MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", True, "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", npy,
                         "MODEL.ROI_HEADS.NUM_CLASSES", Z.C, "MODEL.ROI_BOX_HEAD.USE_BIAS", Z.USE_BIAS,
                         "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False])
    pred = DeticFastRCNNOutputLayers(cfg, ShapeSpec(channels=Z.IN))
    assert isinstance(pred.cls_score, ZeroShotClassifier) and float(pred.cls_score.cls_bias) == np.float32(Z.USE_BIAS)
    assert pred.cls_score.norm_temperature == 50.0 and pred.cls_score.zs_weight.shape == (512, Z.C + 1)
    cfg.MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP = True
    with pytest.raises(NotImplementedError, match="WITH_SOFTMAX_PROP"):
        DeticFastRCNNOutputLayers(cfg, ShapeSpec(channels=Z.IN))
