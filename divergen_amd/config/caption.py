"""Start-up checks of caption training (MODEL.WITH_CAPTION, DATALOADER.DATASET_ANN 'caption' / 'captiontag', behind this build's key
MODEL.CAPTION_TRAIN): what the path needs is demanded, and what of the reference's recipe is not built is refused, by the name of its
key, before any data is read or any kernel runs.  Without the key nothing here applies: config/image_labels.py refuses
MODEL.WITH_CAPTION and the caption annotation types by name, as before."""

CAPTION_ANN_TYPES = ("caption", "captiontag")
REFUSED_ANN_TYPES = ("prop", "proptag")


def _refuse(key, why):
    raise NotImplementedError("%s: %s" % (key, why))


def caption_train(cfg):
    return bool(cfg.MODEL.get("CAPTION_TRAIN", False))


def with_caption(cfg):
    """MODEL.WITH_CAPTION as this build runs it: behind the key."""
    return caption_train(cfg) and bool(cfg.MODEL.WITH_CAPTION)


def check_model_keys(cfg):
    """The model side; a configuration without MODEL.CAPTION_TRAIN passes untouched."""
    if not caption_train(cfg):
        return
    m, h = cfg.MODEL, cfg.MODEL.ROI_BOX_HEAD
    if not m.WITH_CAPTION:
        if m.SYNC_CAPTION_BATCH:
            raise ValueError("MODEL.SYNC_CAPTION_BATCH needs MODEL.WITH_CAPTION True: there is no caption batch to gather")
        return
    if not cfg.WITH_IMAGE_LABELS:
        raise ValueError("MODEL.WITH_CAPTION needs WITH_IMAGE_LABELS True: a caption batch takes the image-labelled step "
                         "(DG detic_roi_heads.py:226-234)")
    if not h.USE_ZEROSHOT_CLS:
        raise ValueError("MODEL.WITH_CAPTION needs MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS True: the caption scores are "
                         "cls_score(x, classifier=captions) of the open-vocabulary classifier")
    if not h.ADD_IMAGE_BOX:
        raise ValueError("MODEL.WITH_CAPTION needs MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX True: the caption loss reads the image box's row "
                         "(the reference asserts it, DG detic_fast_rcnn.py:471)")
    for key in ("TEXT_ENCODER_WEIGHTS", "TEXT_ENCODER_BPE"):
        if not m.get(key, ""):
            raise ValueError("MODEL.WITH_CAPTION needs MODEL.%s: the path of %s (this build never downloads)"
                             % (key, "clip's text state dict" if key.endswith("WEIGHTS") else "clip's BPE merges file"))
    if m.DYNAMIC_CLASSIFIER:
        _refuse("MODEL.DYNAMIC_CLASSIFIER with MODEL.WITH_CAPTION", "the reference asserts the two apart (DG custom_rcnn.py:59)")
    if h.WITH_SOFTMAX_PROP or h.IMAGE_LABEL_LOSS in ("wsddn", "wsod"):
        _refuse("MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP / IMAGE_LABEL_LOSS 'wsddn' with MODEL.WITH_CAPTION",
                "the WSDDN loss would read the concatenated class | caption scores against class-wide proposal scores; not built")
    if int(m.CAP_BATCH_RATIO) < 1:
        raise ValueError("MODEL.CAP_BATCH_RATIO %r: at least 1" % (m.CAP_BATCH_RATIO,))


def check_text_encoder_dim(cfg, embed_dim):
    """The encoder's embed dim (read from its state dict) against the classifier's embedding width."""
    want = int(cfg.MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_DIM)
    if int(embed_dim) != want:
        raise ValueError("MODEL.TEXT_ENCODER_WEIGHTS: the text encoder's embed dim is %d, MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_DIM is %d: "
                         "caption rows and projected box features meet in one dot product" % (embed_dim, want))


def admitted_ann_types(cfg, base):
    """The DATALOADER.DATASET_ANN values check_loader_keys admits: `base`, plus the caption types behind the key."""
    return tuple(base) + (CAPTION_ANN_TYPES if caption_train(cfg) else ())


def check_loader_keys(cfg, anns, sizes):
    """The loader side, called from image_labels.check_loader_keys with the annotation types of DATASETS.TRAIN and the per-GPU batch of
    every source (one entry without DATALOADER.USE_DIFF_BS_SIZE); a configuration without the key passes untouched."""
    if not caption_train(cfg):
        return
    m = cfg.MODEL
    for a in anns:
        if a in REFUSED_ANN_TYPES:
            _refuse("DATALOADER.DATASET_ANN %r" % (a,), "proposal-supervised sources are not built (one of 'box', 'image', 'caption', "
                    "'captiontag')")
    if any(a in CAPTION_ANN_TYPES for a in anns) and not m.WITH_CAPTION:
        raise ValueError("DATALOADER.DATASET_ANN %s holds a caption source but MODEL.WITH_CAPTION is False: the model owns no text "
                         "encoder and would refuse the batch" % (list(anns),))
    if not (m.WITH_CAPTION and m.SYNC_CAPTION_BATCH):
        return
    # every rank gathers on every step and the gather needs one row count: a box step sends BS * CAP_BATCH_RATIO rows, any other BS
    ratio = int(m.CAP_BATCH_RATIO)
    if not cfg.DATALOADER.USE_DIFF_BS_SIZE:
        if ratio != 1 and any(a == "box" for a in anns) and any(a != "box" for a in anns):
            raise ValueError("MODEL.SYNC_CAPTION_BATCH without DATALOADER.USE_DIFF_BS_SIZE needs MODEL.CAP_BATCH_RATIO 1 (got %d): every "
                             "source has the same per-GPU batch, so a box step must send as many rows as a caption step" % ratio)
        return
    box = sorted(set(int(b) for a, b in zip(anns, sizes) if a == "box"))
    other = sorted(set(int(b) for a, b in zip(anns, sizes) if a != "box"))
    if len(box) > 1 or len(other) > 1 or (box and other and other[0] != ratio * box[0]):
        raise ValueError("MODEL.SYNC_CAPTION_BATCH: DATALOADER.DATASET_BS %s for DATALOADER.DATASET_ANN %s -- every non-box source's "
                         "per-GPU batch must equal MODEL.CAP_BATCH_RATIO (%d) x the box sources' batch, or the ranks' gather of "
                         "caption rows would wait for ever" % ([int(b) for b in sizes], list(anns), ratio))
