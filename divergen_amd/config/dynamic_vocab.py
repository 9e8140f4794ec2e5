"""Start-up checks of the dynamic classifier (MODEL.DYNAMIC_CLASSIFIER behind this build's key MODEL.DYNAMIC_VOCAB): what the
reference itself cannot run with it, and what is not built, is refused by the name of its key before any kernel runs."""


def _refuse(key, why):
    raise NotImplementedError("MODEL.DYNAMIC_CLASSIFIER with %s: %s" % (key, why))


def check_dynamic_vocab(cfg):
    """A configuration without MODEL.DYNAMIC_VOCAB or without MODEL.DYNAMIC_CLASSIFIER passes untouched."""
    m = cfg.MODEL
    if not (bool(m.get("DYNAMIC_VOCAB", False)) and m.DYNAMIC_CLASSIFIER):
        return
    h = m.ROI_BOX_HEAD
    if not h.USE_ZEROSHOT_CLS:
        _refuse("MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS False", "the sampled vocabulary is cut out of the open-vocabulary classifier's "
                "zs_weight (DG custom_rcnn.py:162-163)")
    if h.USE_FED_LOSS:
        _refuse("MODEL.ROI_BOX_HEAD.USE_FED_LOSS", "the reference asserts the two apart (DG detic_fast_rcnn.py:102): the sampled vocabulary "
                "IS the federated class set")
    if h.IGNORE_ZERO_CATS:
        _refuse("MODEL.ROI_BOX_HEAD.IGNORE_ZERO_CATS", "the reference's full-length frequency mask does not fit NUM_SAMPLE_CATS columns")
    if h.WITH_SOFTMAX_PROP or (cfg.WITH_IMAGE_LABELS and h.IMAGE_LABEL_LOSS in ("wsddn", "wsod")):
        _refuse("MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP / IMAGE_LABEL_LOSS 'wsddn'", "prop_score stays NUM_CLASSES + 1 wide and cannot be "
                "multiplied with the sampled columns in the reference")
    if m.WITH_CAPTION:
        _refuse("MODEL.WITH_CAPTION", "caption losses are not built (the reference asserts the two apart, DG custom_rcnn.py:59)")
    if bool(cfg.INPUT.get("ACTIVE_SELECT", False)):
        _refuse("INPUT.ACTIVE_SELECT", "BSGAL's held-out pass (only_gt_proposals) trains on the built-in vocabulary")
    if int(m.NUM_SAMPLE_CATS) < 1:
        raise ValueError("MODEL.NUM_SAMPLE_CATS %r: at least 1" % (m.NUM_SAMPLE_CATS,))
