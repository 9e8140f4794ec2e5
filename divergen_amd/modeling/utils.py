"""Test-time vocabularies of the open-vocabulary classifier.  Mirrors DG/divergen/modeling/utils.py:32-63."""
import torch

from .roi_heads.zero_shot_classifier import ZeroShotClassifier, build_zs_weight


class ResetClsTestsError(ValueError):
    """MODEL.RESET_CLS_TESTS with MODEL.TEST_CLASSIFIERS / MODEL.TEST_NUM_CLASSES that do not cover DATASETS.TEST."""


def reset_cls_test(model, cls_path, num_classes):
    """Evaluate `model` on another vocabulary: `cls_path` is the .npy of (C, D) class embeddings or a (D, C) tensor.  Sets
    roi_heads.num_classes and gives every cascade predictor's cls_score the SAME new zs_weight tensor (D, C + 1), built once as the
    constructor builds it.  Accepts a wrapped (`.module`) model."""
    m = model.module if hasattr(model, "module") else model
    preds = list(m.roi_heads.box_predictor)
    if not all(isinstance(getattr(p, "cls_score", None), ZeroShotClassifier) for p in preds):
        raise NotImplementedError("reset_cls_test needs MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS: this model's cls_score is a fixed Linear")
    zs_weight = build_zs_weight(cls_path, preds[0].cls_score.norm_weight)
    if zs_weight.shape[1] != num_classes + 1:
        raise ValueError("reset_cls_test: %d class embeddings for num_classes %d" % (zs_weight.shape[1] - 1, num_classes))
    if zs_weight.shape[0] != preds[0].cls_score.zs_weight.shape[0]:
        raise ValueError("reset_cls_test: embedding dimension %d, the classifier projects to %d"
                         % (zs_weight.shape[0], preds[0].cls_score.zs_weight.shape[0]))
    m.roi_heads.num_classes = num_classes
    zs_weight = zs_weight.to(torch.float32).to(m.device)
    for p in preds:
        p.cls_score.set_zs_weight(zs_weight)
    return zs_weight


def reset_cls_vocabularies(cfg):
    """[(dataset name, classifier path, number of classes)] of MODEL.RESET_CLS_TESTS (DG/train_net.py:88-93), or None when off."""
    if not cfg.MODEL.RESET_CLS_TESTS:
        return None
    names, paths, counts = list(cfg.DATASETS.TEST), list(cfg.MODEL.TEST_CLASSIFIERS), list(cfg.MODEL.TEST_NUM_CLASSES)
    if len(paths) < len(names) or len(counts) < len(names):
        raise ResetClsTestsError("MODEL.RESET_CLS_TESTS: MODEL.TEST_CLASSIFIERS (%d) and MODEL.TEST_NUM_CLASSES (%d) need one entry per "
                                 "DATASETS.TEST set (%d)" % (len(paths), len(counts), len(names)))
    return list(zip(names, paths, counts))


def text_vocabulary(encoder, names, prompt="a ", chunk=256):
    """Class embeddings of a list of names from the text encoder, as BS/bsgal/predictor.py:15-23 makes a custom test vocabulary:
    (C, embed_dim) fp32 on the host, one row per name of `prompt + name`.  Saved as .npy it is what ZEROSHOT_WEIGHT_PATH /
    MODEL.TEST_CLASSIFIERS read; `reset_cls_test(model, emb.permute(1, 0).contiguous(), C)` takes it as a tensor (the reference's
    own transpose).  The names run through the encoder `chunk` at a time."""
    names = list(names)
    if not names:
        raise ValueError("text_vocabulary: no names")
    rows = []
    for i in range(0, len(names), chunk):
        rows.append(encoder([prompt + n for n in names[i:i + chunk]]).detach().float().cpu())
    return torch.cat(rows, 0)
