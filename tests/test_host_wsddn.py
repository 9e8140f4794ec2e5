"""Host-side tests of the WSDDN image-label loss and the proposal-score branch (MODEL.ROI_BOX_HEAD.WS_PROP_SCORE): the float64
restatement (tests/_wsddn_ref.py) against the reference's own outputs (tests/golden/wsddn.npz), every mutant of the restatement outside
the same bound, the key and refusal table, the predictor's parameters, the ABI names.

Bound: |got - ref| <= rtol * max(|ref|, floor), floor = the restatement's sum of absolute addends.  tests/golden/make_golden_wsddn.py
measured the reference's own fp32 evaluation against the restatement in that form at rtol 1e-5: worst ratio 0.098 (loss), 0.128
(d scores), 0.122 (d proposal scores) on the golden inputs and 0.018 / 0.760 / 0.767 on the inputs of the GPU tests (fp32 and bf16
stored values, widths 38 / 1204 / 1454).  It stays inside, so rtol = 1e-5 (the project's bound for fp32) is kept."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _wsddn_ref as W  # noqa: E402

RTOL = 1e-5


def _restated(mutant=None):
    d = W.inputs()
    return W.wsddn_loss(d["scores"], d["prop"], d["valid"], d["boxes"], W.COUNTS, W.IMAGE_SIZES, W.LABELS, W.WEIGHT, mutant=mutant)


def _outside(r, g, base):
    """Which of the golden's values `r` misses (the floors are those of the unmutated restatement)."""
    miss = []
    if r["sel"] != g["wsddn.sel"].tolist():
        miss.append("sel")
    if abs(r["loss"] - g["wsddn.loss"]) > 1e-6 * abs(g["wsddn.loss"]) or abs(r["l_image"] - g["wsddn.l_image"]) > 1e-6 * abs(g["wsddn.l_image"]):
        miss.append("loss")
    if not np.allclose(r["stats"], g["wsddn.stats"], rtol=1e-6, atol=1e-7):
        miss.append("stats")
    if W.worst_ratio(r["dscores"], g["wsddn.dscores"], base["floor_s"], RTOL) > 1:
        miss.append("dscores")
    if W.worst_ratio(r["dprop"], g["wsddn.dprop"], base["floor_p"], RTOL) > 1:
        miss.append("dprop")
    return miss


def test_measured_reference_error_is_inside_the_bound(golden):
    g = golden("wsddn")
    assert g["measured.golden"].max() < 1 and g["measured.cases"].max() < 1, (g["measured.golden"], g["measured.cases"])


def test_restatement_against_reference(golden):
    """Loss and statistics to 1e-6 relative, selected rows equal, both gradients within rtol * max(|value|, floor) of the reference's
    fp32 gradients; the constructed cases are in the inputs."""
    g, r = golden("wsddn"), _restated()
    assert _outside(r, g, r) == []
    r3 = W.COUNTS[0] + W.COUNTS[1]
    assert r["S"][0][W.COL_ONE] == 1.0 and r["S"][3][W.COL_LOW] < W.LO and 5e-4 < 1 - r["S"][3][W.COL_HIGH] < 2e-3
    assert not r["dscores"][0, W.COL_ONE] and not r["dprop"][r3:r3 + 40, W.COL_LOW].any()
    # the saturated column of the one-row image: three labels, each 100 / (C + 1) from it
    d = W.inputs()
    plain = d["scores"].copy()
    plain[0, W.COL_ONE] = 0.0
    r0 = W.wsddn_loss(plain, d["prop"], d["valid"], d["boxes"], W.COUNTS, W.IMAGE_SIZES, W.LABELS, W.WEIGHT)
    want = (100.0 - np.log(2.0)) / (W.C + 1) / len(W.COUNTS)
    assert abs((r["l_image"] - r0["l_image"]) - want) < 1e-9


@pytest.mark.parametrize("mutant", W.MUTANTS)
def test_every_mutant_falls_outside_the_bound(mutant, golden):
    g, base = golden("wsddn"), _restated()
    miss = _outside(_restated(mutant), g, base)
    assert miss, mutant
    print(mutant, "misses", miss)


# ------------------------------------------------------------------------------------------------ keys and refusals
def _cfg(tmp_path, monkeypatch, opts):
    from test_host_image_labels import _two_source_cfg
    return _two_source_cfg(tmp_path, monkeypatch, opts)[0]


KEY = ["MODEL.ROI_BOX_HEAD.WS_PROP_SCORE", True]
TABLE = [
    (["MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsddn"], NotImplementedError, ["IMAGE_LABEL_LOSS", "WS_PROP_SCORE"]),
    (["MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsod"], NotImplementedError, ["IMAGE_LABEL_LOSS", "WS_PROP_SCORE"]),
    (["MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP", True], NotImplementedError, ["WITH_SOFTMAX_PROP", "WS_PROP_SCORE"]),
    (KEY + ["MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsddn"], ValueError, ["IMAGE_LABEL_LOSS", "WITH_SOFTMAX_PROP"]),
    (KEY + ["MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsod"], ValueError, ["IMAGE_LABEL_LOSS", "WITH_SOFTMAX_PROP"]),
    (KEY + ["MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "nonsense"], ValueError, ["IMAGE_LABEL_LOSS"]),
    (KEY + ["MODEL.ROI_BOX_HEAD.SOFTMAX_WEAK_LOSS", True], NotImplementedError, ["SOFTMAX_WEAK_LOSS"]),
    (KEY + ["MODEL.ROI_BOX_HEAD.ADD_FEATURE_TO_PROP", True], NotImplementedError, ["ADD_FEATURE_TO_PROP"]),
    (KEY + ["MODEL.WITH_CAPTION", True], NotImplementedError, ["WITH_CAPTION"]),
    (KEY + ["MODEL.DYNAMIC_CLASSIFIER", True], NotImplementedError, ["DYNAMIC_CLASSIFIER"]),
    (KEY + ["MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", False], NotImplementedError, ["USE_SIGMOID_CE"]),
]


@pytest.mark.parametrize("opts,exc,names", TABLE, ids=["%d-%s" % (i, t[2][0]) for i, t in enumerate(TABLE)])
def test_refusals_name_their_keys(opts, exc, names, tmp_path, monkeypatch):
    from divergen_amd.config.image_labels import check_model_keys
    cfg = _cfg(tmp_path, monkeypatch, opts)
    with pytest.raises(exc) as e:
        check_model_keys(cfg)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_admitted_with_the_key_and_untouched_without(tmp_path, monkeypatch):
    from divergen_amd.config import get_cfg
    from divergen_amd.config.image_labels import IMAGE_LABEL_LOSSES, check_loader_keys, check_model_keys
    assert IMAGE_LABEL_LOSSES == ("max_size", "max_score", "first", "image", "min_loss"), "the mode ids DGX_IL_* are ABI"
    assert get_cfg().MODEL.ROI_BOX_HEAD.WS_PROP_SCORE is False
    for loss in ("wsddn", "wsod", "max_size", "min_loss"):
        cfg = _cfg(tmp_path / loss, monkeypatch, KEY + ["MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP", True, "MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", loss])
        check_model_keys(cfg)
        check_loader_keys(cfg, 2)
    from test_gpu_loader import _mini_cfg
    shipped, _ = _mini_cfg(tmp_path / "s", 128, 0)
    check_model_keys(shipped)
    check_loader_keys(shipped, 2)
    check_model_keys(_cfg(tmp_path / "t", monkeypatch, []))
    check_model_keys(_cfg(tmp_path / "u", monkeypatch, KEY))


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.mark.parametrize("zeroshot", [False, True], ids=["linear", "zeroshot"])
def test_predictor_parameters_from_a_config(zeroshot, tmp_path, monkeypatch, golden):
    """prop_score.0.* / prop_score.2.* with the reference's names and shapes (and init: zero biases, std 0.001 on the last layer) when
    WITH_SOFTMAX_PROP is admitted; absent without it."""
    from divergen_amd.modeling import ShapeSpec
    from divergen_amd.modeling.roi_heads.detic_fast_rcnn import DeticFastRCNNOutputLayers
    g = golden("wsddn")
    opts = ["MODEL.ROI_HEADS.NUM_CLASSES", W.C]
    if zeroshot:
        npy = os.path.join(str(tmp_path), "emb.npy")
        np.save(npy, np.random.default_rng(3).standard_normal((W.C, 512)).astype(np.float32))
        opts += ["MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", True, "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", npy, "MODEL.ROI_BOX_HEAD.USE_BIAS", -4.6,
                 "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False]
    else:
        opts += ["MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False]
    on = _cfg(tmp_path / "on", monkeypatch, opts + KEY + ["MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP", True, "MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsddn"])
    pred = DeticFastRCNNOutputLayers(on, ShapeSpec(channels=8))
    sd = pred.state_dict()
    for n in ("prop_score.0.weight", "prop_score.0.bias", "prop_score.2.weight", "prop_score.2.bias"):
        assert tuple(sd[n].shape) == g["init." + n].shape, n
    assert tuple(sd["prop_score.2.weight"].shape) == (W.C + 1, 8)
    assert not sd["prop_score.0.bias"].any() and not sd["prop_score.2.bias"].any()
    assert 2e-4 < float(sd["prop_score.2.weight"].std()) < 3e-3 and float(sd["prop_score.0.weight"].abs().max()) <= np.sqrt(3.0 / 8) + 1e-6
    assert pred.wsddn and pred.with_softmax_prop
    off = _cfg(tmp_path / "off", monkeypatch, opts)
    assert not any(n.startswith("prop_score") for n in DeticFastRCNNOutputLayers(off, ShapeSpec(channels=8)).state_dict())
    with pytest.raises(RuntimeError, match="proposal scores"):
        pred.image_label_losses(None, None, None, [], [], [])


def test_names_that_fail_without_the_feature():
    from divergen_amd import _lib
    from divergen_amd.csrc.build import SOURCES
    from divergen_amd.layers import image_label_ops
    for s in ("dgx_wsddn_loss", "dgx_wsddn_workspace_floats"):
        assert s in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "divergen_hip.h")).read()
    assert "int dgx_wsddn_loss(" in hdr and "int64_t dgx_wsddn_workspace_floats(" in hdr
    assert "wsddn_loss.hip" in SOURCES and hasattr(image_label_ops, "wsddn_loss")
    import torch
    with pytest.raises(_lib.DgxError):
        image_label_ops.wsddn_loss(torch.zeros(2, 38), torch.zeros(2, 38), None, torch.zeros(2, 4), [2], [(10, 10)], [[1]], 0.1)
