"""Config surface of the reference: a yacs-style CfgNode tree with `_BASE_` YAML inheritance,
`KEY VALUE` list overrides and `configurable`/`from_config` construction.

Mirrors D2/config/{config.py,defaults.py} + CN/config.py:3-88 (add_centernet_config) +
DG/divergen/config.py:4-209 (add_divergen_config).  The default VALUES are data
(divergen_amd/config/defaults.json, dumped from the reference's config tree by
tests/golden/make_default_config.py); DiverGen's configs/*.yaml load unchanged.
"""
import ast
import copy
import functools
import inspect
import json
import os

import yaml

_DEFAULTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "defaults.json")
BASE_KEY = "_BASE_"


class CfgNode(dict):
    def __init__(self, init=None):
        super().__init__()
        object.__setattr__(self, "_frozen", False)
        for k, v in (init or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) and not isinstance(v, CfgNode) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        if object.__getattribute__(self, "_frozen"):
            raise AttributeError("Attempted to set %s on a frozen CfgNode" % k)
        self[k] = v

    def freeze(self):
        self._set_frozen(True)

    def defrost(self):
        self._set_frozen(False)

    def is_frozen(self):
        return object.__getattribute__(self, "_frozen")

    def _set_frozen(self, f):
        object.__setattr__(self, "_frozen", f)
        for v in self.values():
            if isinstance(v, CfgNode):
                v._set_frozen(f)

    def clone(self):
        c = CfgNode(copy.deepcopy(_plain(self)))
        return c

    def dump(self, **kw):
        return yaml.safe_dump(_plain(self), **kw)

    # ---- merging
    @staticmethod
    def load_yaml_with_base(filename):
        with open(filename) as f:
            cfg = yaml.safe_load(f) or {}
        if BASE_KEY in cfg:
            base = cfg.pop(BASE_KEY)
            if not os.path.isabs(base):
                base = os.path.join(os.path.dirname(filename), base)
            merged = CfgNode.load_yaml_with_base(base)
            _merge_dict(cfg, merged, strict=False)
            return merged
        return cfg

    def merge_from_file(self, filename, allow_unsafe=False):
        loaded = CfgNode.load_yaml_with_base(filename)
        loaded.pop("VERSION", None) if "VERSION" not in self else None
        self.merge_from_other_cfg(loaded)

    def merge_from_other_cfg(self, other):
        _merge_node(other, self, [])

    def merge_from_list(self, lst):
        assert len(lst) % 2 == 0, "Override list has odd length: %s" % (lst,)
        for full_key, v in zip(lst[0::2], lst[1::2]):
            d = self
            parts = full_key.split(".")
            for p in parts[:-1]:
                if p not in d:
                    raise KeyError("Non-existent config key: %s" % full_key)
                d = d[p]
            if parts[-1] not in d:
                raise KeyError("Non-existent config key: %s" % full_key)
            d[parts[-1]] = _coerce(_decode(v), d[parts[-1]], full_key)


def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, tuple):
        return [_plain(v) for v in x]
    if isinstance(x, list):
        return [_plain(v) for v in x]
    return x


def _decode(v):
    if not isinstance(v, str):
        return v
    try:
        return ast.literal_eval(v)
    except (ValueError, SyntaxError):
        return v


def _coerce(new, old, key):
    if old is None or new is None or type(new) == type(old):
        return new
    if isinstance(old, (list, tuple)) and isinstance(new, (list, tuple)):
        return type(old)(new) if isinstance(old, tuple) else list(new)
    if isinstance(old, float) and isinstance(new, int) and not isinstance(new, bool):
        return float(new)
    if isinstance(old, str) and not isinstance(new, str):
        raise ValueError("Type mismatch for %s: %r vs %r" % (key, new, old))
    if isinstance(old, bool) != isinstance(new, bool) or (isinstance(old, (int, float)) and isinstance(new, str)):
        raise ValueError("Type mismatch for %s: %r (%s) vs %r (%s)" % (key, new, type(new), old, type(old)))
    return new


def _merge_dict(src, dst, strict):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge_dict(v, dst[k], strict)
        else:
            dst[k] = v


def _merge_node(src, dst, path):
    for k, v in src.items():
        full = ".".join(path + [k])
        if k not in dst:
            raise KeyError("Non-existent config key: %s" % full)
        if isinstance(v, dict):
            if not isinstance(dst[k], dict):
                raise ValueError("Type mismatch for %s" % full)
            _merge_node(v, dst[k], path + [k])
        else:
            dst[k] = _coerce(_decode(v), dst[k], full)


def get_cfg():
    """Defaults of detectron2 + add_centernet_config + add_divergen_config (already merged)."""
    with open(_DEFAULTS) as f:
        cfg = CfgNode(json.load(f))
    # Keys of THIS build only (not in the reference tree; defaults keep the reference behaviour):
    #   INPUT.INST_POOL_SHARDS: directory of pool-*.dgxpool shards (divergen_amd/data/pool_store.py, built by
    #   tools/build_inst_pool.py); when set, pool instances are read from the shards instead of PIL-opened per sample.
    cfg.INPUT.INST_POOL_SHARDS = ""
    #   INPUT.CP_POISSON: admits 'possion' (Poisson blending) to INPUT.CP_METHOD.  Off by default: a 'possion' paste costs one
    #   conjugate-gradient solve on the device and rewrites the image frame, as the reference's poisson_edit does
    #   (divergen_amd/csrc/poisson_blend.hip); without the key 'possion' is refused at start-up.
    cfg.INPUT.CP_POISSON = False
    #   INPUT.SCP_MULTI_SRC: admits INPUT.SCP_NUM_SRC 2 .. 4 to the self-copy methods of INPUT.USE_COPY_METHOD: the sources are merged
    #   on the device first (dgx_self_copy_merge, divergen_amd/csrc/self_copy.hip), which costs one more read-back of validity bytes and boxes per
    #   sample; without the key SCP_NUM_SRC != 1 is refused at start-up.
    cfg.INPUT.SCP_MULTI_SRC = False
    #   INPUT.SCP_SRC_MODES: admits, to the self-copy methods of INPUT.USE_COPY_METHOD, INPUT.SCP_TYPE 'in_domain' / 'cas' / 'the_cls' /
    #   'the_cls_img' (the source image drawn per category) and INPUT.SCP_SRC_OBJ_SELECT False (every object of the source is pasted:
    #   dgx_self_copy_paste_all, no bound of 99), and makes INPUT.RM_BG_PROB > 0 remove the destination's background under EVERY copy
    #   method, as the reference does (divergen_amd/csrc/remove_background.hip); without the key the first two are refused at start-up
    #   and RM_BG_PROB is refused with a self-copy method and ignored otherwise.
    cfg.INPUT.SCP_SRC_MODES = False
    #   INPUT.DEVICE_RASTER: the loader workers ship the ground-truth polygons as sorted crossing lists (a few hundred int32 per object)
    #   instead of rasterising them into dense (N, H, W) byte masks; the training process fills the masks on the device, one launch per
    #   sample on the loader's side stream in front of the compositor (dgx_polygons_to_bitmask, divergen_amd/csrc/polygon_raster.hip), bit for bit
    #   what the worker would have filled.  Built for INPUT.USE_COPY_METHOD 'none' / 'syn_copy'; the self-copy methods and
    #   INPUT.ACTIVE_SELECT are refused with it at start-up.  Off by default: the worker rasterises, as before.
    cfg.INPUT.DEVICE_RASTER = False
    #   INPUT.DEVICE_RESIZE: the loader workers (training mapper only) skip both Pillow resizes.  A sample ships its decoded source image
    #   with the numbers of its resize-crop-flip and the fixed-point coefficient tables of the crop window; an instance-pool patch whose
    #   source has at most 4x the pixels of the resized patch ships its source crop.  The training process resizes on the device, one
    #   launch per sample on the loader's side stream in front of everything that reads pixels (dgx_resize_bilinear_u8,
    #   divergen_amd/csrc/resize_u8.hip), byte for byte Pillow's BILINEAR.  The np.random draws are unchanged.  Built for
    #   INPUT.USE_COPY_METHOD 'none' / 'syn_copy'; the self-copy methods and INPUT.ACTIVE_SELECT are refused with it at start-up.
    #   Off by default: the worker resizes, as before.
    cfg.INPUT.DEVICE_RESIZE = False
    #   MODEL.ROI_BOX_HEAD.WS_PROP_SCORE: admits, with WITH_IMAGE_LABELS, MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS 'wsddn' / 'wsod' (the softmax
    #   over an image's proposals times the sigmoid class scores: dgx_wsddn_loss, divergen_amd/csrc/wsddn_loss.hip) and the predictor
    #   branch it reads, MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP (prop_score: Linear-ReLU-Linear, two more GEMMs per cascade stage of an
    #   image step, parameters that a box step leaves at a zero gradient); without the key both are refused at start-up.
    cfg.MODEL.ROI_BOX_HEAD.WS_PROP_SCORE = False
    #   MODEL.DYNAMIC_VOCAB: admits MODEL.DYNAMIC_CLASSIFIER True with MODEL.NUM_SAMPLE_CATS (a vocabulary sampled per batch: the classes
    #   present plus frequency-weighted negatives; the classifier, its logits and the losses are NUM_SAMPLE_CATS + 1 columns wide), on
    #   the open-vocabulary classifier (MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS), with or without WITH_IMAGE_LABELS: four kernels
    #   (dgx_dyn_class_sample, dgx_zs_gather, dgx_remap_labels, dgx_zs_logits_f32; divergen_amd/csrc/dyn_vocab.hip, config/dynamic_vocab.py).  Without the
    #   key DYNAMIC_CLASSIFIER is refused at start-up.
    cfg.MODEL.DYNAMIC_VOCAB = False
    #   MODEL.CAPTION_TRAIN: admits MODEL.WITH_CAPTION True (the model owns the frozen CLIP text encoder and trains the open-vocabulary
    #   classifier on image captions), DATALOADER.DATASET_ANN 'caption' / 'captiontag', MODEL.SYNC_CAPTION_BATCH with
    #   MODEL.CAP_BATCH_RATIO (the caption rows of all ranks gathered on every step) and makes MODEL.ROI_BOX_HEAD.CAPTION_WEIGHT /
    #   NEG_CAP_WEIGHT take effect: dgx_caption_prepare, dgx_caption_loss (divergen_amd/csrc/caption_loss.hip, config/caption.py).
    #   Without the key all of these are refused at start-up, as before.
    #   MODEL.TEXT_ENCODER_WEIGHTS / MODEL.TEXT_ENCODER_BPE: the paths of clip's text state dict and BPE merges file (this build never
    #   downloads); the encoder's geometry is read from the state dict's shapes.
    cfg.MODEL.CAPTION_TRAIN = False
    cfg.MODEL.TEXT_ENCODER_WEIGHTS = ""
    cfg.MODEL.TEXT_ENCODER_BPE = ""
    #   SOLVER.ALLREDUCE_DTYPE: "fp32" (the reference's DDP: gradients all-reduced as they are) or "bf16" (gradient buckets go over
    #   xGMI as bf16, half the bytes per step; engine/ddp.py ArenaReducer(wire_dtype=...)).
    cfg.SOLVER.ALLREDUCE_DTYPE = "fp32"
    #   TEST.LVIS_EVAL_DEVICE: LVISEvaluator scores the gathered detections on the GPU (evaluation/lvis_eval_device.py: mask / box IoU,
    #   greedy matching and the precision / recall curves as kernels of divergen_amd/csrc/lvis_eval.hip, bit for bit what the Python
    #   evaluator computes) instead of in evaluation/lvis_eval.py.  Off by default: the Python evaluator stays the path, and the device
    #   module is not even imported.
    cfg.TEST.LVIS_EVAL_DEVICE = False
    return cfg


def add_centernet_config(cfg):
    """CN/config.py:3-88 -- keys are already part of get_cfg(); kept for call-site compatibility."""
    return cfg


def add_divergen_config(cfg):
    """DG/divergen/config.py:4-209 -- keys are already part of get_cfg()."""
    return cfg


def add_bsgal_config(cfg):
    """BS/bsgal/config.py:52-79,176-180: the keys BSGAL adds on top of the Detic / DiverGen tree (the gradient-based active
    selection of pasted batches); BS/configs/BSGAL/*.yaml load with these in place."""
    m, i = cfg.MODEL, cfg.INPUT
    for k, v in (("ACTIVE_MODE", "paste_or_zero"), ("ACTIVE_LOSS", "cls"), ("ACTIVE_LOSS_UPDATE", "all"), ("ACTIVE_SEED", 0),
                 ("ACTIVE_COMPARE", "default"), ("ACTIVE_TEST", "select"), ("ACTIVE_TEST_INS", "one"), ("ACTIVE_LR", 0.0001),
                 ("ACTIVE_OPTIMIZER", True), ("ACTIVE_OPTIMIZER_MODE", "sgd"), ("ACTIVE_PRED", False), ("ACTIVE_PRED_CHOOSE", ""),
                 ("ACTIVE_PRED_SUP", "all"), ("ACTIVE_ONLY_GT_TRAIN", False), ("ACTIVE_ONLY_GT_TEST", False),
                 ("ACTIVE_GRAD_COMPARE", False), ("ACTIVE_GRAD_NORM", True), ("ACTIVE_GRAD_SAVE", False),
                 ("ACTIVE_GRAD_UPDATE", "AVERAGE"), ("ONLY_PASTE_SUP", False), ("ACTIVE_FORWARD_ONCE", False),
                 ("ACTIVE_ONCE_MODE", "only_gt"), ("ACTIVE_EVAL", False), ("ACTIVE_DYNAMIC_THRES", 0.0), ("ACTIVE_TEST_BATCHSIZE", 4),
                 ("USE_XPASTE_BOX_LOSS", True), ("USE_XPASTE_MASK_LOSS", True)):
        if k not in m:
            m[k] = v
    for k, v in (("ACTIVE_SELECT", False), ("ACTIVE_SELECT_TYPE", "train"), ("SEPARATE_SYN", False), ("SEPERATE_SUP", False)):
        if k not in i:
            i[k] = v
    return cfg


def configurable(init_func=None, *, from_config=None):
    """D2/config/config.py `configurable`: allow `Cls(cfg, *args)` to build through
    `Cls.from_config(cfg, *args)` while still accepting explicit keyword construction."""
    def _called_with_cfg(*args, **kwargs):
        if len(args) and isinstance(args[0], CfgNode):
            return True
        return isinstance(kwargs.get("cfg"), CfgNode)

    if init_func is not None:
        @functools.wraps(init_func)
        def wrapped(self, *args, **kwargs):
            fc = type(self).from_config
            if _called_with_cfg(*args, **kwargs):
                explicit = fc(*args, **kwargs)
                init_func(self, **explicit)
            else:
                init_func(self, *args, **kwargs)
        return wrapped

    def wrapper(orig):
        @functools.wraps(orig)
        def wrapped(*args, **kwargs):
            if _called_with_cfg(*args, **kwargs):
                return orig(**from_config(*args, **kwargs))
            return orig(*args, **kwargs)
        return wrapped
    return wrapper
