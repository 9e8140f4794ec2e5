"""CustomRCNN meta-architecture.  Mirrors DG/divergen/modeling/meta_arch/custom_rcnn.py:24-207 over
D2/modeling/meta_arch/rcnn.py:24-243 for the box-supervised path the shipped configs train and, with WITH_IMAGE_LABELS, for
batches that carry image labels only (:128-136, :190-202).

Precision: the reference runs the backbone under fp16 autocast + GradScaler and the heads in fp32
(custom_rcnn.py:141-146).  This build has ONE precision: bf16 operands, fp32 accumulation in every GEMM / convolution /
attention kernel of backbone and heads (no loss scaling needed); losses, box decoding, targets and the optimizer state are
fp32.  cfg.FP16 False (no shipped configuration) is refused: there is no fp32-activation path and no eager fallback."""
import os

import torch
from torch import nn

from .. import META_ARCH_REGISTRY, build_backbone, build_proposal_generator, build_roi_heads
from ...config import configurable
from ...layers.conv_ops import preprocess_patch_rows
from ...layers.roi_ops import FeatureGradients
from ...structures import ImageList

# dgx_preprocess_patches; the composed normalise + pad + unfold form is the reference of its parity test
_FUSED_PREPROCESS = True


class _CaptureGradient(torch.autograd.Function):
    """Identity; its backward hands the incoming gradient to slot i of a FeatureGradients (no copy) and ends the pass there."""

    @staticmethod
    def forward(ctx, fg, i, x):
        ctx.fg, ctx.i = fg, i
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.fg.add(ctx.i, g)
        return None, None, None


class _JoinGradients(torch.autograd.Function):
    """Identity on the feature maps; its backward -- which autograd runs after every consumer of its outputs -- returns what the
    consumers left in the FeatureGradients (the RoI poolers add in place, layers/roi_ops.py; an EARLIER backward pass of the
    proposal generator, `early_proposal_backward`, through _CaptureGradient) plus whatever arrived the ordinary way."""

    @staticmethod
    def forward(ctx, fg, *feats):
        ctx.fg = fg
        ctx.set_materialize_grads(False)
        return tuple(f.view_as(f) for f in feats)

    @staticmethod
    def backward(ctx, *grads):
        out = []
        for i, g in enumerate(grads):
            e = ctx.fg.take(i)
            out.append(g if e is None else e if g is None else e.add_(g))
        return (None,) + tuple(out)


class _PassThrough(torch.autograd.Function):
    """Identity whose backward hands its gradients on unchanged: a place for `torch.autograd.backward(..., inputs=...)` to stop.
    (backward() EXECUTES the node that produced a non-leaf input; stopping at _JoinGradients' own outputs would run its backward --
    and empty the shared maps -- before the last consumer has written.)"""

    @staticmethod
    def forward(ctx, *feats):
        ctx.set_materialize_grads(False)
        return tuple(f.view_as(f) for f in feats)

    @staticmethod
    def backward(ctx, *grads):
        return grads


def _shared_gradient_maps(features):
    """features (dict of maps that require grad) -> (FeatureGradients, the same dict behind _JoinGradients with the slots announced)"""
    names = list(features.keys())
    fg = FeatureGradients(len(names))
    joined = _JoinGradients.apply(fg, *[features[k] for k in names])
    for i, (k, j) in enumerate(zip(names, joined)):
        j._dgx_grad_sink = (fg, i)
        _same_buffer(features[k], j)
    return fg, dict(zip(names, joined))


def _same_buffer(src, view):
    """`view` is `src` behind an identity node: a hipGraph segment that takes `src` as its static input as it stands
    (utils/graphs.py ALIAS_STATIC) may do so with `view`."""
    if getattr(src, "_dgx_static_output", False):
        view._dgx_static_output = True
    return view


class EarlyLosses(dict):
    """The loss dict of a forward that ALREADY back-propagated the proposal generator's part (early_proposal_backward): those
    entries are detached, their gradients sit in the arena / on the feature maps.  Correct only for exactly one backward of the
    plain, unweighted sum of the dict -- which is what engine.total_loss() builds; it marks the dict consumed, and the next
    early forward refuses to run while an unconsumed one is outstanding (a second forward before backward, a loop that sums
    the dict itself, per-loss weights or gradient accumulation would otherwise get wrong gradients without a word)."""
    consumed = False


@META_ARCH_REGISTRY.register()
class CustomRCNN(nn.Module):
    @configurable
    def __init__(self, *, backbone, proposal_generator, roi_heads, pixel_mean, pixel_std, input_format=None,
                 vis_period=0, fp16=False, with_image_labels=False, roi_head_name="", dataset_loss_weight=(),
                 dynamic_classifier=False, num_sample_cats=50, num_classes=None, freq_weight=None, with_caption=False,
                 sync_caption_batch=False, cap_batch_ratio=4, text_encoder=None, **unused):
        super().__init__()
        assert proposal_generator is not None
        # MODEL.WITH_CAPTION behind MODEL.CAPTION_TRAIN (custom_rcnn.py:58-62): the model owns the frozen text encoder, state-dict names
        # `text_encoder.*` as in the reference; SYNC_CAPTION_BATCH gathers the caption rows of every rank on every training step
        self.with_caption, self.sync_caption_batch, self.cap_batch_ratio = bool(with_caption), bool(sync_caption_batch), int(cap_batch_ratio)
        if self.with_caption:
            if dynamic_classifier:
                raise NotImplementedError("MODEL.DYNAMIC_CLASSIFIER with MODEL.WITH_CAPTION: the reference asserts the two apart")
            if text_encoder is None:
                raise ValueError("with_caption needs text_encoder (MODEL.TEXT_ENCODER_WEIGHTS / MODEL.TEXT_ENCODER_BPE)")
            self.text_encoder = text_encoder
            for v in self.text_encoder.parameters():
                v.requires_grad = False
        elif self.sync_caption_batch:
            raise ValueError("sync_caption_batch needs with_caption (MODEL.SYNC_CAPTION_BATCH / MODEL.WITH_CAPTION)")
        # MODEL.DYNAMIC_CLASSIFIER (custom_rcnn.py:50-55): a vocabulary of num_sample_cats classes sampled per batch.  freq_weight is a
        # plain attribute, as in the reference: the state dict does not change
        self.dynamic_classifier = bool(dynamic_classifier)
        if self.dynamic_classifier:
            if num_classes is None or freq_weight is None:
                raise ValueError("dynamic_classifier needs num_classes and freq_weight")
            self.freq_weight, self.num_classes, self.num_sample_cats = freq_weight, int(num_classes), int(num_sample_cats)
        # WITH_IMAGE_LABELS: every sample carries `ann_type` ('box' | 'image') and `pos_category_ids`, a batch holds one type
        self.with_image_labels = bool(with_image_labels)
        self.dataset_loss_weight = [float(w) for w in dataset_loss_weight]      # MODEL.DATASET_LOSS_WEIGHT, by `dataset_source`
        self.backbone, self.proposal_generator, self.roi_heads = backbone, proposal_generator, roi_heads
        self.input_format, self.vis_period, self.fp16, self.roi_head_name = input_format, vis_period, fp16, roi_head_name
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std).view(-1, 1, 1), False)
        if not fp16:
            raise NotImplementedError("cfg.FP16 False: this build computes in bf16 with fp32 accumulation on its own HIP kernels; "
                                      "an fp32-activation mode does not exist (every shipped configuration sets FP16: True)")
        # hipGraph capture of the static-shape backbone fwd+bwd (launch-bound otherwise: ~3.5k launches)
        self.return_proposal = False
        # Trainer opt-in (bench.py, train_net.py's plain loop): the proposal generator's losses are back-propagated from INSIDE the
        # forward, queued on the GPU before the RoI heads' one device->host read (the proposal sampler), so the device has that
        # backward to run while the host -- which loses its whole lead at that read -- issues the RoI heads.  The loss dict then carries
        # those losses DETACHED (their gradients are already in the arena / on the feature maps): only valid for a loop that calls
        # backward once on the plain sum of the dict, after a zero_grad.
        self.early_proposal_backward = False
        # The box cascade's losses likewise, right behind the cascade's forward and up to the feature maps: measured 0.3 ms/step SLOWER
        # (24.8-25.1 against 24.4-24.7 ms in one box: one more engine start costs more than the stretch it covers), so it stays off.
        self.early_box_backward = False

    @classmethod
    def from_config(cls, cfg):
        from ...config.dynamic_vocab import check_dynamic_vocab
        check_dynamic_vocab(cfg)
        dyn = {}
        if cfg.MODEL.DYNAMIC_CLASSIFIER and cfg.MODEL.get("DYNAMIC_VOCAB", False):        # (custom_rcnn.py:78-83)
            from ..roi_heads.detic_fast_rcnn import load_class_freq
            dyn = dict(dynamic_classifier=True, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES, num_sample_cats=cfg.MODEL.NUM_SAMPLE_CATS,
                       freq_weight=load_class_freq(cfg.MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH, cfg.MODEL.ROI_BOX_HEAD.FED_LOSS_FREQ_WEIGHT))
        from ...config.caption import check_model_keys as check_caption_keys, check_text_encoder_dim, with_caption
        check_caption_keys(cfg)
        if with_caption(cfg):
            from ..text import build_text_encoder
            # (the encoder's constructor draws initial values that the state dict then replaces: under a forked generator, so that the
            # rest of the model initialises exactly as it does without the encoder)
            with torch.random.fork_rng(devices=[]):
                enc = build_text_encoder(cfg.MODEL.TEXT_ENCODER_WEIGHTS, cfg.MODEL.TEXT_ENCODER_BPE, geometry_from_weights=True)
            check_text_encoder_dim(cfg, enc.embed_dim)
            dyn = dict(dyn, with_caption=True, text_encoder=enc, sync_caption_batch=bool(cfg.MODEL.SYNC_CAPTION_BATCH),
                       cap_batch_ratio=cfg.MODEL.CAP_BATCH_RATIO)
        backbone = build_backbone(cfg)
        shape = backbone.output_shape()
        return dict(**dyn, backbone=backbone, proposal_generator=build_proposal_generator(cfg, shape),
                    roi_heads=build_roi_heads(cfg, shape), input_format=cfg.INPUT.FORMAT, vis_period=cfg.VIS_PERIOD,
                    pixel_mean=cfg.MODEL.PIXEL_MEAN, pixel_std=cfg.MODEL.PIXEL_STD, fp16=cfg.FP16,
                    with_image_labels=cfg.WITH_IMAGE_LABELS, roi_head_name=cfg.MODEL.ROI_HEADS.NAME,
                    dataset_loss_weight=cfg.MODEL.DATASET_LOSS_WEIGHT)

    @property
    def device(self):
        return self.pixel_mean.device

    def preprocess_image(self, batched_inputs):
        """rcnn.py:220-227: H2D, (x - mean) / std, zero-pad to the backbone's divisibility."""
        images = [x["image"].to(self.device, non_blocking=True) for x in batched_inputs]
        if self._patch_rows_ok(images):
            # uint8 images -> PatchEmbed's GEMM operand in one pass (normalise + zero-pad + 4x4 unfold, bf16); the fp32 batch
            # tensor is only materialised if somebody asks for `.tensor`
            pr, sizes = preprocess_patch_rows(images, self.pixel_mean, self.pixel_std, self.backbone.size_divisibility)
            return ImageList(None, sizes, patch_rows=pr)
        images = [(x.float() - self.pixel_mean) / self.pixel_std for x in images]
        return ImageList.from_tensors(images, self.backbone.size_divisibility)

    def _patch_rows_ok(self, images):
        bu = getattr(self.backbone, "bottom_up", None)
        pe = getattr(bu, "patch_embed", None)
        return (_FUSED_PREPROCESS and pe is not None and pe.patch_size == (4, 4)
                and all(im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[0] == 3 for im in images))

    def _features(self, images):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if images.patch_rows is not None:
                return self.backbone(images.patch_rows)
            return self.backbone(images.tensor.to(memory_format=torch.channels_last))

    def forward(self, batched_inputs):
        if not self.training:
            return self.inference(batched_inputs)
        # BSGAL (BS/bsgal/modeling/meta_arch/custom_rcnn.py:278-780): with INPUT.ACTIVE_SELECT the loader hands the pasted
        # sample together with its un-pasted original and a held-out image; engine.bsgal.ActiveSelector (attached by the
        # trainer once the parameter arena exists) decides which of the two batches this step trains on
        sel = self.__dict__.get("active_selector")
        if sel is not None and len(batched_inputs) and "origin_image" in batched_inputs[0]:
            batched_inputs, paste = sel.select(batched_inputs)
            extra = sel.extra_losses()                                              # ACTIVE_COMPARE 'all': the original batch as well
            losses = self.training_losses(batched_inputs)
            losses = {k: v for k, v in losses.items() if "paste" not in k}          # :767 pop_loss_paste
            if extra is not None:                                                   # :772-774
                losses = {k: v + extra[k] for k, v in losses.items()}
            if sel.mode == "paste_or_zero" and not paste:                           # :769-771: the step trains on nothing
                losses = {k: v * 0.0 for k, v in losses.items()}
            return losses
        return self.training_losses(batched_inputs, early=self.early_proposal_backward and not self.return_proposal)

    def _annotation_type(self, batched_inputs, gt_instances):
        """custom_rcnn.py:128-136: the batch's one annotation type; `ann_type` / `pos_category_ids` copied onto the instances."""
        if not self.with_image_labels:
            return "box"
        for inst, x in zip(gt_instances, batched_inputs):
            if "ann_type" not in x or "pos_category_ids" not in x:
                raise KeyError("WITH_IMAGE_LABELS: every sample needs 'ann_type' and 'pos_category_ids' (the loader's mapper adds them)")
            inst._ann_type, inst._pos_category_ids = x["ann_type"], x["pos_category_ids"]
        types = set(x["ann_type"] for x in batched_inputs)
        assert len(types) == 1, "one annotation type per batch, got %s (DATALOADER.MULTI_DATASET_GROUPING)" % sorted(types)
        ann_type = types.pop()
        if ann_type not in ("box", "image") + (("caption", "captiontag") if self.with_caption else ()):
            raise NotImplementedError("ann_type %r: 'box' and 'image' are built, 'caption' / 'captiontag' with MODEL.WITH_CAPTION behind "
                                      "MODEL.CAPTION_TRAIN (DATALOADER.DATASET_ANN)" % (ann_type,))
        return ann_type

    def _caption_features(self, batched_inputs, ann_type):
        """custom_rcnn.py:148-157: one caption per sample drawn with torch.randint in batch order (the tokenizer's crop draws come after
        them, inside the encoder), encoded to (B, D) fp32; under SYNC_CAPTION_BATCH the rank column appended and the rows of every
        rank gathered -- every rank takes part on every training step, a step without captions sends zero rows and gets None."""
        feats = None
        if self.with_caption and "caption" in ann_type:
            for x in batched_inputs:
                if not x.get("captions"):
                    raise KeyError("a %r batch needs `captions` (a non-empty list of strings) on every sample" % (ann_type,))
            inds = [torch.randint(len(x["captions"]), (1,))[0].item() for x in batched_inputs]
            feats = self.text_encoder([x["captions"][i] for i, x in zip(inds, batched_inputs)]).float()
        if self.sync_caption_batch:
            from ...layers.caption_ops import all_gather_rows, sync_caption_features
            from ...utils import comm
            feats = sync_caption_features(feats, ann_type, len(batched_inputs), comm.get_rank(), self.cap_batch_ratio, all_gather_rows,
                                          dim=self.text_encoder.embed_dim, device=self.device)
        return feats

    def _weight_by_source(self, batched_inputs, losses):
        """custom_rcnn.py:197-202: MODEL.DATASET_LOSS_WEIGHT multiplies every loss by the weight of the batch's `dataset_source`."""
        if not self.dataset_loss_weight:
            return losses
        sources = set(x["dataset_source"] for x in batched_inputs)
        assert len(sources) == 1, "one dataset_source per batch, got %s" % sorted(sources)
        w = self.dataset_loss_weight[sources.pop()]
        for k in list(losses.keys()):
            losses[k] = losses[k] * w
        return losses

    def _sample_cls_inds(self, gt_instances, ann_type="box", gt_classes=None):
        """custom_rcnn.py:226-247 without a device->host read: one exponential_ draw of C + 1 values (what the reference's multinomial
        draws at this position of torch's random stream; it draws only when fewer than num_sample_cats classes appear, see below) and
        dgx_dyn_class_sample.  Box step: the
        concatenated gt_classes, weighted by freq_weight over its len(freq_weight) classes; image step: the images' pos_category_ids,
        uniform over num_classes -- there the column count is known from the lists."""
        from ...layers.dyn_vocab_ops import DynamicVocab, sample_classes, sampling_weights
        from ...utils.h2d import upload_i32
        dev = self.device
        n_host = None
        if ann_type == "box":
            if gt_classes is None:
                gt_classes = torch.cat([x.gt_classes for x in gt_instances]) if len(gt_instances) else torch.zeros(0, dtype=torch.int64, device=dev)
            C, weight = len(self.freq_weight), self.freq_weight
        else:
            flat = [int(c) for x in gt_instances for c in x._pos_category_ids]
            if flat and (max(flat) >= self.num_classes or min(flat) < 0):
                raise ValueError("pos_category_ids outside [0, %d)" % self.num_classes)       # (the reference's assert, :240)
            gt_classes = upload_i32(flat, dev).long() if flat else torch.zeros(0, dtype=torch.int64, device=dev)
            C, weight = self.num_classes, None
            n_host = max(min(self.num_sample_cats, C), len(set(flat)))
        prob0 = sampling_weights(weight, C, dev)
        if ann_type != "box" and len(set(flat)) >= self.num_sample_cats:
            expo = prob0        # nothing is drawn and the host knows it: no draw from the generator either, as in the reference (utils.py:20)
        else:
            # a box step draws on EVERY step -- the number of distinct classes is on the device -- where the reference's multinomial
            # draws only when fewer than num_sample_cats appear: on the other steps torch's random stream runs C + 1 values ahead of it
            expo = torch.empty_like(prob0).exponential_(1)
        inds, cls_id_map, n = sample_classes(gt_classes, prob0, expo, C, self.num_classes, self.num_sample_cats)
        return DynamicVocab(inds, cls_id_map, n_host if (n_host is not None and torch.is_tensor(n)) else n, self.num_classes)

    def _image_step_losses(self, images, features, gt_instances, classifier_info=(None, None, None), ann_type="image"):
        """An image-labelled batch (custom_rcnn.py:166-194): the proposal generator runs for its proposals only, without gradient
        tracking (no autograd graph is built or held) -- its losses are reported as exact zeros (the reference's `v * 0` of finite
        values), so neither its backward nor the early backward pass exist in this step; the RoI heads train the cascade's
        classifiers on the image labels."""
        with torch.no_grad():
            proposals, proposal_losses = self.proposal_generator(images, features, gt_instances)
        proposals, detector_losses = self.roi_heads(images, features, proposals, gt_instances, ann_type=ann_type,
                                                    classifier_info=classifier_info)
        losses = dict(detector_losses)
        losses.update({k: v.detach().float().reshape(()) * 0.0 for k, v in proposal_losses.items()})
        return proposals, losses

    def training_losses(self, batched_inputs, only_gt_proposals=False, early=False):
        """custom_rcnn.py:118-207 for the box-supervised path: the loss dict of one batch."""
        images = self.preprocess_image(batched_inputs)
        gt_instances = [x["instances"].to(self.device) for x in batched_inputs]
        ann_type = self._annotation_type(batched_inputs, gt_instances)
        early = early and not self.dataset_loss_weight      # (a weighted loss cannot have been back-propagated unweighted)
        features = self._features(images)
        from ...solver import join_transposes
        join_transposes()        # transposed weight images refreshed beside the backbone forward: first read by what follows
        grads_on = torch.is_grad_enabled() and all(f.requires_grad for f in features.values())
        # after the backbone, before the proposal generator: the reference's position in torch's random stream (:148-157).  With
        # SYNC_CAPTION_BATCH this gathers on every step, box steps included (their rows are zeros and the result is dropped)
        caption_features = self._caption_features(batched_inputs, ann_type) if self.with_caption else None
        if ann_type != "box":
            if only_gt_proposals:
                raise NotImplementedError("only_gt_proposals (BSGAL's held-out pass) on an image-labelled batch")
            with torch.autocast("cuda", dtype=torch.bfloat16):
                if grads_on:
                    fg, features = _shared_gradient_maps(features)
                ci = (None, self._sample_cls_inds(gt_instances, "image"), None) if self.dynamic_classifier else \
                    (None, None, caption_features if "caption" in ann_type else None)
                proposals, losses = self._image_step_losses(images, features, gt_instances, ci, ann_type)
            losses = self._weight_by_source(batched_inputs, losses)
            return (proposals, losses) if self.return_proposal else losses
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if grads_on:
                # the consumers of the FPN levels write ONE gradient map per level between them
                fg, joined = _shared_gradient_maps(features)
            if hasattr(self.roi_heads, "prepare_targets") and not only_gt_proposals:
                self.roi_heads.prepare_targets(gt_instances)
            ci = {}
            if self.dynamic_classifier:
                if only_gt_proposals:
                    raise NotImplementedError("MODEL.DYNAMIC_CLASSIFIER with only_gt_proposals (BSGAL's held-out pass)")
                # after the backbone, before the proposal generator: the reference's position in torch's random stream (:159-166)
                pre = self.roi_heads.__dict__.get("_gt_batch")
                cat = pre[2] if (pre is not None and pre[0] is gt_instances and sum(len(t) for t in gt_instances)) else None
                ci = dict(classifier_info=(None, self._sample_cls_inds(gt_instances, "box", cat), None))
            if early and grads_on:
                prev = self.__dict__.get("_early_outstanding")
                if prev is not None and not prev.consumed:
                    raise RuntimeError("early_proposal_backward: the previous forward's loss dict was never passed to engine.total_loss() "
                                       "(one backward of the plain sum per forward is the contract; switch model.early_proposal_backward "
                                       "off for loops that weight losses, accumulate gradients or run two forwards per backward)")
                stubs = {k: _same_buffer(f, _CaptureGradient.apply(fg, i, f.detach().requires_grad_(True)))
                         for i, (k, f) in enumerate(features.items())}
                proposals, proposal_losses = self.proposal_generator(images, stubs, gt_instances)
                pl_total = torch.stack([v.float().reshape(()) for v in proposal_losses.values()]).sum()
                self.roi_heads.__dict__["_before_host_read"] = pl_total.backward
                if self.early_box_backward and not only_gt_proposals and all(getattr(j, "_dgx_grad_sink", None) is not None for j in joined.values()):
                    # ... and the box cascade's losses right behind its forward, up to the feature maps the RoI heads see (roi_heads.forward)
                    names = list(joined.keys())
                    stops = _PassThrough.apply(*[joined[k] for k in names])
                    for k, t in zip(names, stops):
                        t._dgx_grad_sink = joined[k]._dgx_grad_sink
                        _same_buffer(joined[k], t)
                    joined = dict(zip(names, stops))
                    self.roi_heads.__dict__["_early_box_backward"] = list(stops)
                try:
                    proposals, detector_losses = self.roi_heads(images, joined, proposals, gt_instances, ann_type="box",
                                                                only_gt_proposals=only_gt_proposals, **ci)
                finally:
                    pending = self.roi_heads.__dict__.pop("_before_host_read", None)
                    self.roi_heads.__dict__.pop("_early_box_backward", None)
                if pending is not None:         # the RoI heads took a path without the fused sampler
                    pending()
                proposal_losses = {k: v.detach() for k, v in proposal_losses.items()}
            else:
                if grads_on:
                    features = joined
                proposals, proposal_losses = self.proposal_generator(images, features, gt_instances)
                proposals, detector_losses = self.roi_heads(images, features, proposals, gt_instances, ann_type="box",
                                                            only_gt_proposals=only_gt_proposals, **ci)
        losses = EarlyLosses() if (early and grads_on) else {}
        losses.update(detector_losses)
        losses.update(proposal_losses)
        losses = self._weight_by_source(batched_inputs, losses)
        if isinstance(losses, EarlyLosses):
            self.__dict__["_early_outstanding"] = losses
        return (proposals, losses) if self.return_proposal else losses

    @torch.no_grad()
    def inference(self, batched_inputs, do_postprocess=True):
        assert not self.training
        images = self.preprocess_image(batched_inputs)
        features = self._features(images)
        from ...solver import join_transposes
        join_transposes()        # (the mask head's deconvolution reads a transposed weight image)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            proposals, _ = self.proposal_generator(images, features, None)
            results, _ = self.roi_heads(images, features, proposals)
        if not do_postprocess:
            return results
        out = []
        for r, inp, size in zip(results, batched_inputs, images.image_sizes):
            out.append({"instances": detector_postprocess(r, inp.get("height", size[0]), inp.get("width", size[1]))})
        return out


def detector_postprocess(results, output_height, output_width, mask_threshold=0.5, mask_format="bitmask"):
    """D2/modeling/postprocessing.py: rescale boxes to the output resolution, paste masks.
    mask_format="rle" (not in the reference): leave the masks as `pred_masks_rle` COCO run-length dicts, encoded on the GPU
    straight from the SxS probabilities -- what the evaluator's results writer turns the bitmasks into anyway."""
    from ...structures import Boxes, Instances
    sx, sy = output_width / results.image_size[1], output_height / results.image_size[0]
    out = Instances((output_height, output_width), **results.get_fields())
    b = out.pred_boxes.tensor.clone()
    b[:, 0::2] *= sx
    b[:, 1::2] *= sy
    bx = Boxes(b)
    bx.clip(out.image_size)
    out.pred_boxes = bx
    keep = bx.nonempty()
    out = out[keep]
    if out.has("pred_masks") and mask_format == "rle":
        from ...layers.mask_ops import paste_masks_rle
        rles = paste_masks_rle(out.pred_masks[:, 0], out.pred_boxes.tensor, (output_height, output_width), mask_threshold)
        out.remove("pred_masks")
        out.pred_masks_rle = rles
    elif out.has("pred_masks"):
        out.pred_masks = paste_masks_in_image(out.pred_masks[:, 0], out.pred_boxes.tensor, (output_height, output_width),
                                              mask_threshold)
    return out


def paste_masks_in_image(masks, boxes, image_shape, threshold=0.5):
    """D2/layers/mask_ops.py:73 -- aligned bilinear paste of the SxS probability maps, on the GPU (dgx_paste_masks)."""
    from ...layers.mask_ops import paste_masks_in_image as _paste
    return _paste(masks, boxes, image_shape, threshold)
