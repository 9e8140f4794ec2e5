"""Start-up checks of image-label co-training (WITH_IMAGE_LABELS, DATALOADER.SAMPLER_TRAIN 'MultiDatasetSampler'): what of the
reference's recipe is not built is refused by the name of its key, before any data is read or any kernel runs."""

ANN_TYPES = ("box", "image")
IMAGE_LABEL_LOSSES = ("max_size", "max_score", "first", "image", "min_loss")      # the mode ids DGX_IL_* of the ABI, in this order
WSDDN_LOSSES = ("wsddn", "wsod")          # the proposal-softmax loss (dgx_wsddn_loss), admitted by MODEL.ROI_BOX_HEAD.WS_PROP_SCORE
MAX_IMAGES_PER_GPU = 32          # REFINE_MAX_IMAGES of csrc/cascade_refine.hip, IL_MAX_IMAGES of csrc/image_label.hip


def _refuse(key, why):
    raise NotImplementedError("%s: %s" % (key, why))


def check_image_label_loss(loss, add_image_box, use_sigmoid_ce, ws_prop_score=False, with_softmax_prop=False):
    """The predictor's own conditions (its constructor and check_model_keys both come here)."""
    if loss in WSDDN_LOSSES:
        if not ws_prop_score:
            _refuse("MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS %r" % loss, "the WSDDN loss is admitted by MODEL.ROI_BOX_HEAD.WS_PROP_SCORE True only "
                    "(without the key: one of %s)" % (IMAGE_LABEL_LOSSES,))
        if not with_softmax_prop:
            raise ValueError("MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS %r needs MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP True: it reads the "
                             "proposal-score branch" % loss)
    elif loss not in IMAGE_LABEL_LOSSES:
        raise ValueError("MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS %r: one of %s" % (loss, IMAGE_LABEL_LOSSES))
    if loss == "image" and not add_image_box:
        raise ValueError("MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS 'image' needs MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX: it trains on the image box")
    if not use_sigmoid_ce:
        _refuse("MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE False", "WITH_IMAGE_LABELS needs the sigmoid classifier (the image-label loss is a sigmoid BCE)")


def check_filter_empty(filter_empty, dataset_ann):
    """An image-labelled source has no box annotations: filtering images without them would silently delete the whole source."""
    if filter_empty and any(a != "box" for a in dataset_ann):
        raise ValueError("DATALOADER.FILTER_EMPTY_ANNOTATIONS must be False with an image-labelled source in DATALOADER.DATASET_ANN %s: "
                         "its images have no box annotations, filtering would delete the whole source" % (list(dataset_ann),))


def check_model_keys(cfg):
    """The model side; a configuration without WITH_IMAGE_LABELS passes untouched (behind MODEL.CAPTION_TRAIN, config/caption.py
    first demands what MODEL.WITH_CAPTION needs -- WITH_IMAGE_LABELS among it)."""
    from .caption import check_model_keys as check_caption_keys, with_caption
    check_caption_keys(cfg)
    if not cfg.WITH_IMAGE_LABELS:
        return
    h = cfg.MODEL.ROI_BOX_HEAD
    ws_prop = bool(h.get("WS_PROP_SCORE", False))
    check_image_label_loss(h.IMAGE_LABEL_LOSS, h.ADD_IMAGE_BOX, h.USE_SIGMOID_CE, ws_prop, h.WITH_SOFTMAX_PROP)
    if h.WITH_SOFTMAX_PROP and not ws_prop:
        _refuse("MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP", "the proposal-score branch is admitted by MODEL.ROI_BOX_HEAD.WS_PROP_SCORE True only")
    for key, on in (("MODEL.ROI_BOX_HEAD.SOFTMAX_WEAK_LOSS", h.SOFTMAX_WEAK_LOSS),
                    ("MODEL.ROI_BOX_HEAD.ADD_FEATURE_TO_PROP", h.ADD_FEATURE_TO_PROP), ("MODEL.WITH_CAPTION", cfg.MODEL.WITH_CAPTION and not with_caption(cfg)),
                    ("MODEL.DYNAMIC_CLASSIFIER", cfg.MODEL.DYNAMIC_CLASSIFIER and not cfg.MODEL.get("DYNAMIC_VOCAB", False))):
        if on:
            _refuse(key, "not built: image-label co-training covers the five row-selection losses and, with MODEL.ROI_BOX_HEAD.WS_PROP_SCORE, "
                    "the WSDDN loss, on the sigmoid classifier only")
    method = cfg.INPUT.USE_COPY_METHOD
    if method in ("self_copy", "both") or str(method).startswith("p:"):
        _refuse("INPUT.USE_COPY_METHOD %r" % method, "self copy-paste draws a second BOX-annotated image; with WITH_IMAGE_LABELS the training set "
                "holds image-labelled samples ('none' or 'syn_copy')")
    if bool(cfg.INPUT.get("ACTIVE_SELECT", False)):
        _refuse("INPUT.ACTIVE_SELECT", "BSGAL's active selection is not built together with WITH_IMAGE_LABELS")
    w = list(cfg.MODEL.DATASET_LOSS_WEIGHT)
    if w and len(w) != len(cfg.DATASETS.TRAIN):
        raise ValueError("MODEL.DATASET_LOSS_WEIGHT: %d weights for %d DATASETS.TRAIN" % (len(w), len(cfg.DATASETS.TRAIN)))


def check_loader_keys(cfg, per_gpu):
    """The loader side, for DATALOADER.SAMPLER_TRAIN 'MultiDatasetSampler' and / or WITH_IMAGE_LABELS."""
    d = cfg.DATALOADER
    multi = d.SAMPLER_TRAIN == "MultiDatasetSampler"
    if not multi and not cfg.WITH_IMAGE_LABELS:
        return
    n = len(cfg.DATASETS.TRAIN)
    if d.USE_TAR_DATASET:
        _refuse("DATALOADER.USE_TAR_DATASET", "tar-file datasets are not built")
    for key in ("DATASET_ANN", "DATASET_RATIO", "USE_RFS") + (("DATASET_BS", "DATASET_INPUT_SIZE", "DATASET_INPUT_SCALE") if d.USE_DIFF_BS_SIZE else ()):
        if len(d[key]) < n:
            raise ValueError("DATALOADER.%s has %d entries for %d DATASETS.TRAIN" % (key, len(d[key]), n))
    from .caption import admitted_ann_types, check_loader_keys as check_caption_loader
    anns = list(d.DATASET_ANN)[:n]
    check_caption_loader(cfg, anns, [int(b) for b in list(d.DATASET_BS)[:n]] if d.USE_DIFF_BS_SIZE else [int(per_gpu)] * n)
    admitted = admitted_ann_types(cfg, ANN_TYPES)
    for a in anns:
        if a not in admitted:
            _refuse("DATALOADER.DATASET_ANN %r" % (a,), "one of %s (caption / prop / proptag annotation types are not built)" % (admitted,))
    if any(a != "box" for a in anns):
        if not cfg.WITH_IMAGE_LABELS:
            raise ValueError("DATALOADER.DATASET_ANN holds %s but WITH_IMAGE_LABELS is False: the model would refuse the batch"
                             % ", ".join(sorted(set(repr(a) for a in anns if a != "box"))))
        check_filter_empty(d.FILTER_EMPTY_ANNOTATIONS, list(d.DATASET_ANN)[:n])
    if cfg.WITH_IMAGE_LABELS and not multi:
        raise ValueError("WITH_IMAGE_LABELS needs DATALOADER.SAMPLER_TRAIN 'MultiDatasetSampler' (got %r): a batch must hold one "
                         "annotation type" % d.SAMPLER_TRAIN)
    if multi and not d.MULTI_DATASET_GROUPING:
        _refuse("DATALOADER.MULTI_DATASET_GROUPING False", "MultiDatasetSampler is built with per-source batches only "
                "(a mixed batch has no single annotation type)")
    if d.USE_DIFF_BS_SIZE and cfg.INPUT.CUSTOM_AUG != "EfficientDetResizeCrop":
        _refuse("DATALOADER.USE_DIFF_BS_SIZE with INPUT.CUSTOM_AUG %r" % cfg.INPUT.CUSTOM_AUG,
                "per-source input sizes are built for 'EfficientDetResizeCrop' (DATASET_INPUT_SIZE / DATASET_INPUT_SCALE) only")
    sizes = [int(b) for b in list(d.DATASET_BS)[:n]] if d.USE_DIFF_BS_SIZE else [int(per_gpu)]
    if max(sizes) > MAX_IMAGES_PER_GPU or min(sizes) < 1:
        raise ValueError("per-GPU batch %s: between 1 and REFINE_MAX_IMAGES = %d images (DATALOADER.DATASET_BS / SOLVER.IMS_PER_BATCH)"
                         % (sizes, MAX_IMAGES_PER_GPU))
