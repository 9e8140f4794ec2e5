"""Shared fixtures of the caption-training tests: a two-layer test text encoder on disk (state dict + the BPE merges file of
tests/test_host_caption.py) and the two-source configuration (a generated box source + a generated captioned image source)."""
import gzip
import os

import torch

MERGES = ["#version: test", "l o", "lo w</w>", "e r</w>", "n e", "ne w", "new er</w>"]      # tests/test_host_caption.py
GEOMETRY = dict(embed_dim=512, context_length=77, vocab_size=520, transformer_width=64, transformer_heads=1, transformer_layers=2)


def write_text_encoder(dirpath, seed=11, **geometry):
    """-> (weights_path, bpe_path): CLIPTEXT's own initialisation under a forked generator, saved as a clip-style state dict."""
    from divergen_amd.modeling.text import CLIPTEXT
    os.makedirs(str(dirpath), exist_ok=True)
    bpe = os.path.join(str(dirpath), "merges.txt.gz")
    with gzip.open(bpe, "wb") as f:
        f.write("\n".join(MERGES).encode("utf-8"))
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        sd = CLIPTEXT(**dict(GEOMETRY, **geometry)).state_dict()
    weights = os.path.join(str(dirpath), "clip_text.pth")
    torch.save(dict(sd), weights)
    return weights, bpe


def caption_opts(weights, bpe, sync=False):
    return ["MODEL.CAPTION_TRAIN", True, "MODEL.WITH_CAPTION", True, "MODEL.TEXT_ENCODER_WEIGHTS", weights, "MODEL.TEXT_ENCODER_BPE", bpe,
            "MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX", True, "MODEL.SYNC_CAPTION_BATCH", bool(sync), "MODEL.CAP_BATCH_RATIO", 1 if sync else 4]


def two_source_cfg(tmp_path, monkeypatch, extra=(), ann="captiontag", key=True, num_classes=1203):
    """tests/test_host_image_labels._two_source_cfg with a captioned image source, the open-vocabulary classifier on a generated
    vocabulary of `num_classes` (1203: the generated box source draws LVIS category ids) and, with `key`, the caption keys."""
    import numpy as np
    from divergen_amd.data import build as B
    from divergen_amd.data.synthetic import write_mini_image_labels
    from tests.test_gpu_loader import _mini_cfg
    weights, bpe = write_text_encoder(tmp_path / "enc")
    npy = os.path.join(str(tmp_path), "emb.npy")
    np.save(npy, np.random.default_rng(3).standard_normal((num_classes, 512)).astype(np.float32))
    opts = ["WITH_IMAGE_LABELS", True, "DATALOADER.SAMPLER_TRAIN", "MultiDatasetSampler", "DATALOADER.MULTI_DATASET_GROUPING", True,
            "DATALOADER.FILTER_EMPTY_ANNOTATIONS", False, "DATALOADER.DATASET_ANN", ["box", ann], "DATALOADER.DATASET_RATIO", [1, 1],
            "DATALOADER.USE_RFS", [True, False], "DATASETS.TRAIN", ("lvis_v1_train", "cc_mini"), "MODEL.ROI_BOX_HEAD.WS_NUM_PROPS", 32,
            "MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", True, "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", npy, "MODEL.ROI_HEADS.NUM_CLASSES", num_classes,
            "MODEL.ROI_BOX_HEAD.USE_BIAS", -4.6, "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False]
    if key:
        opts += caption_opts(weights, bpe)
    else:
        opts += ["MODEL.WITH_CAPTION", True, "MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX", True]
    cfg, info = _mini_cfg(tmp_path, 128, 0, opts + list(extra))
    il = write_mini_image_labels(info["root"], split="cc_mini", n_images=8, n_cats=num_classes, seed=3, captions=True)
    B.register_lvis_instances("cc_mini", il["json"], il["image_root"])
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    return cfg, info, il
