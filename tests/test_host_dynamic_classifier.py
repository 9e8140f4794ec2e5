"""Host-side tests of the dynamic classifier (MODEL.DYNAMIC_CLASSIFIER behind MODEL.DYNAMIC_VOCAB): the float64 restatement
(tests/_dyncls_ref.py) against the reference's own outputs (tests/golden/dynamic_classifier.npz), mutants of the restatement outside
the same bound, the key and refusal table, the module on CPU tensors, the ABI names.

Bound: 1e-5 relative -- what tests/test_host_zeroshot.py and tests/test_host_image_labels.py use for the reference's fp32 values
against a float64 evaluation."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _dyncls_ref as Z  # noqa: E402

RTOL = 1e-5
CASES = (("few", 0), ("many", 1))


def close(a, b, rtol=RTOL):
    return abs(float(a) - float(b)) <= rtol * abs(float(b))


def _box_case(g, name, mutant=None):
    """-> inds, cls_id_map, loss_cls, loss_box_reg, stats, logits of the restatement on a box case of the golden."""
    d = {k[3:]: g[k] for k in g.files if k.startswith("in.")}
    S = Z.BOX_CASES[name]["S"]
    gt = d[name + ".gt_classes"].copy()
    if mutant == "ignore":
        gt[-3:] = -1             # three ignore rows (what dgx_cascade_refine writes for an empty refined box)
    prob0 = np.concatenate([d["freq_weight"], [0.0]]).astype(np.float32)
    inds, cmap, n = Z.sample(gt[(gt >= 0) & (gt < Z.NUM_CLASSES)], prob0, g[name + ".expo"], Z.C_FREQ, Z.NUM_CLASSES, S, mutant=mutant)
    lg = Z.logits(d[name + ".x"], d, Z.sub_vocab(g["zs_weight"], inds))
    loss_cls, loss_box, stats = Z.box_losses(lg, Z.deltas(d[name + ".x"], d), Z.remap(gt, cmap, mutant=mutant), d[name + ".prop"], d[name + ".gtb"])
    return inds, cmap, loss_cls, loss_box, stats, lg


@pytest.mark.parametrize("name,case", CASES)
def test_restatement_against_reference_box(name, case, golden):
    g = golden("dynamic_classifier")
    inds, cmap, loss_cls, loss_box, stats, lg = _box_case(g, name)
    assert inds.tolist() == g[name + ".inds"].tolist() and cmap.tolist() == g[name + ".cls_id_map"].tolist()
    assert np.abs(lg - g[name + ".logits"]).max() <= RTOL * np.abs(g[name + ".logits"]).max()
    assert close(loss_cls, g[name + ".loss_cls"]) and close(loss_box, g[name + ".loss_box_reg"])
    np.testing.assert_allclose(stats, g[name + ".stats"], rtol=1e-6)
    # the cases the issue asks for are in the fixture
    a = len(np.unique(g["in." + name + ".gt_classes"][g["in." + name + ".gt_classes"] < Z.NUM_CLASSES]))
    assert (a < Z.BOX_CASES[name]["S"]) == (name == "few") and (g["in." + name + ".gt_classes"] == Z.NUM_CLASSES).sum() > 5
    # the recorded Exponential(1) values are what torch's generator yields at the sampler's position
    torch.manual_seed(int(g["seed"]) + case)
    assert torch.equal(torch.empty(Z.C_FREQ + 1).exponential_(1), torch.from_numpy(g[name + ".expo"]))


def _image_case(g, mode, mutant=None):
    d = {k[3:]: g[k] for k in g.files if k.startswith("in.")}
    flat = [c for ls in Z.IMAGE_LABELS for c in ls]
    inds, cmap, n = Z.sample(flat, np.concatenate([np.ones(Z.NUM_CLASSES), [0.0]]), g["image.expo"], Z.NUM_CLASSES, Z.NUM_CLASSES, Z.IMAGE_S,
                             mutant=mutant)
    lg = Z.logits(d["image.x"], d, Z.sub_vocab(g["zs_weight"], inds))
    labels = [[int(cmap[c]) for c in ls] for ls in Z.IMAGE_LABELS]
    return inds, cmap, lg, Z.image_loss(lg, d["image.boxes"], labels, mode)["loss"]


@pytest.mark.parametrize("mode", Z.IMAGE_MODES)
def test_restatement_against_reference_image(mode, golden):
    g = golden("dynamic_classifier")
    inds, cmap, lg, loss = _image_case(g, mode)
    assert inds.tolist() == g["image.inds"].tolist() and cmap.tolist() == g["image.cls_id_map"].tolist()
    assert np.abs(lg - g["image.logits"]).max() <= RTOL * np.abs(g["image.logits"]).max()
    assert close(loss, g["image.%s.image_loss" % mode])
    assert float(g["image.%s.stats_label" % mode]) == Z.IMAGE_LABELS[0][0]


@pytest.mark.parametrize("mutant", ["bg", "ignore", "uniform"])
def test_mutants_fall_outside_the_bound(mutant, golden):
    """background mapped to n - 1; -1 rows mapped to background; freq_weight ignored on a box step: each changes inds or moves a loss
    of the 'few' case outside the bound."""
    g = golden("dynamic_classifier")
    if mutant == "ignore":       # against the unmutated restatement on the same rows (the golden has no ignore rows)
        base = _box_case(g, "few", mutant=None)
        d_gt = g["in.few.gt_classes"].copy()
        d_gt[-3:] = -1
        d = {k[3:]: g[k] for k in g.files if k.startswith("in.")}
        lg = base[5]
        dl = Z.deltas(d["few.x"], d)
        good = Z.box_losses(lg, dl, Z.remap(d_gt, base[1]), d["few.prop"], d["few.gtb"])
        bad = Z.box_losses(lg, dl, Z.remap(d_gt, base[1], mutant="ignore"), d["few.prop"], d["few.gtb"])
        assert (Z.remap(d_gt, base[1])[-3:] == -1).all() and (Z.remap(d_gt, base[1], mutant="ignore")[-3:] == base[1][-1]).all()
        assert not close(bad[0], good[0])
        return
    inds, cmap, loss_cls, loss_box, stats, lg = _box_case(g, "few", mutant=mutant)
    changed = inds.tolist() != g["few.inds"].tolist() or cmap.tolist() != g["few.cls_id_map"].tolist()
    outside = not close(loss_cls, g["few.loss_cls"]) or not close(loss_box, g["few.loss_box_reg"])
    assert outside or (mutant == "uniform" and changed), mutant
    if mutant == "uniform":
        assert inds.tolist() != g["few.inds"].tolist()


# ------------------------------------------------------------------------------------------------ keys and refusals
def _cfg(tmp_path, monkeypatch, opts):
    from test_host_image_labels import _two_source_cfg
    return _two_source_cfg(tmp_path, monkeypatch, opts)[0]


def _plain_cfg(opts):
    from divergen_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "DiverGen_swinL.yaml"))
    cfg.merge_from_list(list(opts))
    return cfg


KEY = ["MODEL.DYNAMIC_VOCAB", True, "MODEL.DYNAMIC_CLASSIFIER", True, "MODEL.NUM_SAMPLE_CATS", 8]
ZS = ["MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", True, "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False]
TABLE = [
    (KEY + ["MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False], ["USE_ZEROSHOT_CLS"]),
    (KEY + ZS + ["MODEL.ROI_BOX_HEAD.USE_FED_LOSS", True], ["USE_FED_LOSS"]),
    (KEY + ZS + ["MODEL.ROI_BOX_HEAD.IGNORE_ZERO_CATS", True], ["IGNORE_ZERO_CATS"]),
    (KEY + ZS + ["MODEL.ROI_BOX_HEAD.WS_PROP_SCORE", True, "MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP", True], ["WITH_SOFTMAX_PROP"]),
    (KEY + ZS + ["WITH_IMAGE_LABELS", True, "MODEL.ROI_BOX_HEAD.WS_PROP_SCORE", True, "MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsddn"], ["IMAGE_LABEL_LOSS"]),
    (KEY + ZS + ["WITH_IMAGE_LABELS", True, "MODEL.ROI_BOX_HEAD.WS_PROP_SCORE", True, "MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsod"], ["IMAGE_LABEL_LOSS"]),
    (KEY + ZS + ["MODEL.WITH_CAPTION", True], ["WITH_CAPTION"]),
    (KEY + ZS + ["INPUT.ACTIVE_SELECT", True], ["ACTIVE_SELECT"]),
]


@pytest.mark.parametrize("opts,names", TABLE, ids=["%d-%s" % (i, t[1][0]) for i, t in enumerate(TABLE)])
def test_refusals_with_the_key_name_their_keys(opts, names):
    from divergen_amd.config import add_bsgal_config
    from divergen_amd.config.dynamic_vocab import check_dynamic_vocab
    from divergen_amd.config import get_cfg
    cfg = add_bsgal_config(get_cfg())
    cfg.merge_from_file(os.path.join(ROOT, "configs", "DiverGen_swinL.yaml"))
    cfg.merge_from_list(list(opts))
    with pytest.raises(NotImplementedError) as e:
        check_dynamic_vocab(cfg)
    for n in names + ["DYNAMIC_CLASSIFIER"]:
        assert n in str(e.value), (n, str(e.value))


def test_only_gt_proposals_is_refused_by_name():
    """BSGAL's held-out pass has no start-up key of its own (INPUT.ACTIVE_SELECT, which drives it, is in the table): the RoI heads and the
    meta-architecture refuse the call itself."""
    import types
    from divergen_amd.layers.dyn_vocab_ops import DynamicVocab
    from divergen_amd.modeling.roi_heads.detic_roi_heads import DeticCascadeROIHeads
    dyn = DynamicVocab(torch.zeros(4, dtype=torch.int64), torch.zeros(Z.NUM_CLASSES + 1, dtype=torch.int64), 4, Z.NUM_CLASSES)
    me = types.SimpleNamespace(training=True, with_image_labels=False)
    with pytest.raises(NotImplementedError, match="only_gt_proposals") as e:
        DeticCascadeROIHeads.forward(me, None, {}, [], [], ann_type="box", only_gt_proposals=True, classifier_info=(None, dyn, None))
    assert "DYNAMIC_CLASSIFIER" in str(e.value)


def test_refused_without_the_key_admitted_with_it(tmp_path, monkeypatch):
    from divergen_amd.config import get_cfg
    from divergen_amd.config.dynamic_vocab import check_dynamic_vocab
    from divergen_amd.config.image_labels import check_model_keys
    from divergen_amd.modeling import ShapeSpec
    from divergen_amd.modeling.roi_heads.detic_fast_rcnn import DeticFastRCNNOutputLayers
    assert get_cfg().MODEL.DYNAMIC_VOCAB is False and get_cfg().MODEL.DYNAMIC_CLASSIFIER is False
    npy = os.path.join(str(tmp_path), "emb.npy")
    np.save(npy, np.random.default_rng(3).standard_normal((Z.NUM_CLASSES, 512)).astype(np.float32))
    zs = ZS + ["MODEL.ROI_HEADS.NUM_CLASSES", Z.NUM_CLASSES, "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", npy, "MODEL.ROI_BOX_HEAD.USE_BIAS", -4.6]
    # without the key: refused by name, with image labels and by the open-vocabulary predictor
    with pytest.raises(NotImplementedError, match="DYNAMIC_CLASSIFIER"):
        check_model_keys(_cfg(tmp_path / "a", monkeypatch, ["MODEL.DYNAMIC_CLASSIFIER", True]))
    with pytest.raises(NotImplementedError, match="DYNAMIC_CLASSIFIER"):
        DeticFastRCNNOutputLayers(_plain_cfg(zs + ["MODEL.DYNAMIC_CLASSIFIER", True]), ShapeSpec(channels=8))
    # with it: admitted with and without WITH_IMAGE_LABELS
    on = _cfg(tmp_path / "b", monkeypatch, KEY + zs)
    check_model_keys(on)
    check_dynamic_vocab(on)
    DeticFastRCNNOutputLayers(on, ShapeSpec(channels=8))
    box_only = _plain_cfg(KEY + zs)
    check_dynamic_vocab(box_only)
    DeticFastRCNNOutputLayers(box_only, ShapeSpec(channels=8))
    # the shipped configurations and the key alone pass untouched
    for name in ("DiverGen_swinL.yaml", "baseline_swinL.yaml"):
        cfg = get_cfg()
        cfg.merge_from_file(os.path.join(ROOT, "configs", name))
        check_dynamic_vocab(cfg)
        check_model_keys(cfg)
    check_dynamic_vocab(_plain_cfg(["MODEL.DYNAMIC_VOCAB", True]))


# ------------------------------------------------------------------------------------------------ the module on CPU tensors
def _predictor(tmp, g, mode=""):
    from divergen_amd.modeling import ShapeSpec
    from divergen_amd.modeling.box_regression import Box2BoxTransform
    from divergen_amd.modeling.roi_heads.detic_fast_rcnn import DeticFastRCNNOutputLayers
    from divergen_amd.modeling.roi_heads.zero_shot_classifier import ZeroShotClassifier
    npy = os.path.join(str(tmp), "emb.npy")
    np.save(npy, g["in.emb"])
    cls = ZeroShotClassifier(ShapeSpec(channels=Z.IN), num_classes=Z.NUM_CLASSES, zs_weight_path=npy, zs_weight_dim=Z.D, use_bias=Z.USE_BIAS,
                             norm_weight=True, norm_temperature=Z.TEMP)
    p = DeticFastRCNNOutputLayers(ShapeSpec(channels=Z.IN), box2box_transform=Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0)),
                                  num_classes=Z.NUM_CLASSES, cls_agnostic_bbox_reg=True, smooth_l1_beta=0.0, use_sigmoid_ce=True,
                                  use_fed_loss=False, use_zeroshot_cls=True, cls_score=cls, image_label_loss=mode, image_loss_weight=Z.IMAGE_WEIGHT)
    sd = p.state_dict()
    for k in ("linear.weight", "linear.bias", "cls_bias", "bbox_pred.0.weight", "bbox_pred.0.bias", "bbox_pred.2.weight", "bbox_pred.2.bias"):
        sd[k if k.startswith("bbox_pred") else "cls_score." + k] = torch.from_numpy(g["in." + k]).clone()
    p.load_state_dict(sd, strict=True)
    return p


def _sampler_module(g, S):
    """CustomRCNN's sampler method on a bare object (the meta-architecture itself needs a backbone)."""
    import types
    from divergen_amd.modeling.meta_arch.custom_rcnn import CustomRCNN
    me = types.SimpleNamespace(freq_weight=torch.from_numpy(g["in.freq_weight"]), num_classes=Z.NUM_CLASSES, num_sample_cats=S,
                               device=torch.device("cpu"))
    return lambda inst, ann: CustomRCNN._sample_cls_inds(me, inst, ann)


@pytest.mark.parametrize("name,case", CASES)
def test_module_on_cpu_tensors_matches_the_golden_box(name, case, golden, tmp_path):
    from divergen_amd.structures import Boxes, Instances
    from divergen_amd.utils.events import EventStorage
    g = golden("dynamic_classifier")
    gt = torch.from_numpy(g["in." + name + ".gt_classes"])
    targets = Instances((400, 400), gt_classes=gt[gt < Z.NUM_CLASSES])
    torch.manual_seed(int(g["seed"]) + case)
    dyn = _sampler_module(g, Z.BOX_CASES[name]["S"])([targets], "box")
    n = dyn.resolve()
    assert dyn.inds[:n].tolist() == g[name + ".inds"].tolist() and dyn.cls_id_map.tolist() == g[name + ".cls_id_map"].tolist()
    pred = _predictor(tmp_path, g)
    info = (dyn.classifier(pred.cls_score), dyn, None)
    scores, deltas = pred(torch.from_numpy(g["in." + name + ".x"]), info)
    assert float((scores - torch.from_numpy(g[name + ".logits"])).abs().max()) <= 1e-5 * float(np.abs(g[name + ".logits"]).max())
    inst = Instances((400, 400), proposal_boxes=Boxes(torch.from_numpy(g["in." + name + ".prop"])), gt_boxes=Boxes(torch.from_numpy(g["in." + name + ".gtb"])),
                     gt_classes=gt)
    with EventStorage(0):
        losses = pred.losses((scores, deltas), [inst], classifier_info=info)
    assert close(losses["loss_cls"], g[name + ".loss_cls"]) and close(losses["loss_box_reg"], g[name + ".loss_box_reg"])


def test_module_on_cpu_tensors_matches_the_golden_image(golden):
    from divergen_amd.layers.dyn_vocab_ops import remap_labels
    from divergen_amd.structures import Instances
    g = golden("dynamic_classifier")
    gts = []
    for ls in Z.IMAGE_LABELS:
        t = Instances((10, 10), gt_classes=torch.zeros(0, dtype=torch.int64))
        t._pos_category_ids = ls
        gts.append(t)
    torch.manual_seed(int(g["seed"]) + 2)
    dyn = _sampler_module(g, Z.IMAGE_S)(gts, "image")
    n = dyn.resolve()
    assert n == Z.IMAGE_S and dyn.inds[:n].tolist() == g["image.inds"].tolist() and dyn.cls_id_map.tolist() == g["image.cls_id_map"].tolist()
    lab = torch.tensor([-1, 3, Z.NUM_CLASSES, 20, -1, 9])
    assert remap_labels(lab, dyn.cls_id_map, Z.NUM_CLASSES).tolist() == [-1, 0, n, 3, -1, 2]


def test_names_that_fail_without_the_feature():
    from divergen_amd import _lib
    from divergen_amd.csrc.build import SOURCES
    from divergen_amd.layers import dyn_vocab_ops
    hdr = open(os.path.join(ROOT, "include", "divergen_hip.h")).read()
    for s in ("dgx_dyn_class_sample", "dgx_zs_gather", "dgx_remap_labels", "dgx_zs_logits_f32"):
        assert s in _lib.SIGNATURES and ("int %s(" % s) in hdr, s
    assert "dyn_vocab.hip" in SOURCES
    assert os.path.exists(_lib.LIB_PATH) and hasattr(_lib.lib(), "dgx_zs_gather")      # (the refusal below is not a missing library)
    with pytest.raises(_lib.DgxError, match="GPU"):      # no CPU fallback behind the operand gather
        dyn_vocab_ops.zs_gather(torch.zeros(8, 5), torch.zeros(2, dtype=torch.int64), 2, 8, 4)
