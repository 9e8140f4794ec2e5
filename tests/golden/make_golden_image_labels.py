"""Generate tests/golden/image_labels.npz: image-label co-training (WITH_IMAGE_LABELS) from the reference's own code.  Run in the
authoring container only:

    python tests/golden/make_golden_image_labels.py

On the frozen inputs of tests/_image_label_ref.inputs() it runs
  * the real DeticFastRCNNOutputLayers.image_label_losses (DG/divergen/modeling/roi_heads/detic_fast_rcnn.py:342-434, :524-581)
    in the five modes max_size / max_score / first / image / min_loss: image_loss, stats_l_image, the five logged statistics, the
    gradient of image_loss with respect to the scores and the row each (image, label) selected (the index the reference's own
    rule returned -- see `record_selected`);
  * the real get_top_proposals + _add_image_box (DG detic_roi_heads.py:341-365);
  * the real predict_boxes -> _create_proposals_from_boxes (training) chained over three stages from given deltas, the original
    row of every survivor carried through in `objectness_logits`;
  * the real MultiDatasetSampler (DG/divergen/data/custom_dataset_dataloader.py:368-438) for two and three sources, RFS on and
    off, ranks 0 and 1 of 2; the batches MDAspectRatioGroupedDataset / DIFFMDAspectRatioGroupedDataset (:441-478) form from
    those streams; repeat_factors_from_tag_frequency (:481-504).
The reference is imported through _refload; nothing of it is copied or restated.  Fixed zip timestamps: two runs give identical
bytes.  The cases the tests rely on are asserted to occur."""
import importlib.util
import itertools
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refload as R  # noqa: E402
import _image_label_ref as Z  # noqa: E402
from make_golden_blend import save_deterministic  # noqa: E402

SAMPLER_CASES = [  # sizes, annotation types, ratio, use_rfs, repeat threshold, seed
    ((60, 35), ("box", "image"), (1, 1), (False, False), 0.001, 11),
    ((60, 35), ("box", "image"), (1, 4), (True, True), 0.05, 12),
    ((40, 25, 50), ("box", "image", "image"), (2, 1, 1), (True, False, True), 0.05, 13),
]
STREAM = 240
DIFF_BS = {2: [2, 4], 3: [2, 4, 3]}


def _more_stubs():
    R.install()
    rn = sys.modules["detectron2.modeling.backbone.resnet"]
    rn.BottleneckBlock = rn.ResNet = object
    sys.modules["detectron2.structures"].heatmaps_to_keypoints = None
    for nm in ("keypoint_head", "mask_head"):
        sys.modules["detectron2.modeling.roi_heads." + nm] = R._Permissive("detectron2.modeling.roi_heads." + nm)


def record_selected(pred, mode, log):
    """Wrap the reference's own selection rule of `mode` (an instance attribute over the bound method) so that every row index it
    returns is appended to `log`; nothing of the rule is restated."""
    name = "_%s_loss" % mode
    rule = getattr(pred, name)

    def recorded(*a):
        loss, ind = rule(*a)
        log.append(int(ind))
        return loss, ind
    setattr(pred, name, recorded)


def gen_losses(out, d):
    fr = R.ref("divergen.modeling.roi_heads.detic_fast_rcnn")
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.box_regression import Box2BoxTransform
    from detectron2.structures import Boxes, Instances
    for mode in Z.MODES:
        pred = fr.DeticFastRCNNOutputLayers(ShapeSpec(channels=8), box2box_transform=Box2BoxTransform(weights=Z.BOX_WEIGHTS[0]),
                                            num_classes=Z.C, cls_agnostic_bbox_reg=True, smooth_l1_beta=0.0, use_sigmoid_ce=True,
                                            image_label_loss=mode, image_loss_weight=Z.WEIGHT, add_image_box=True)
        scores = torch.from_numpy(d["scores"]).clone().requires_grad_(True)
        props, r0 = [], 0
        for n, size in zip(Z.COUNTS, Z.IMAGE_SIZES):
            p = Instances(size)
            p.proposal_boxes = Boxes(torch.from_numpy(d["boxes"][r0:r0 + n]))
            p.objectness_logits = torch.zeros(n)
            props.append(p)
            r0 += n
        R._STORAGE.scalars.clear()
        log = []
        record_selected(pred, mode, log)
        losses = pred.image_label_losses((scores, None), props, Z.LABELS)
        assert set(losses) == {"image_loss", "loss_cls", "loss_box_reg"}
        assert float(losses["loss_cls"]) == 0.0 and float(losses["loss_box_reg"]) == 0.0
        losses["image_loss"].backward()
        g = scores.grad.numpy()
        st = R._STORAGE.scalars
        out[mode + ".loss"] = losses["image_loss"].detach().numpy()
        out[mode + ".l_image"] = np.float64(st["stats_l_image"])
        out[mode + ".stats"] = np.array([st["pool_stats"], st["stats_select_size"], st["stats_select_x"], st["stats_select_y"],
                                         st["stats_max_label_score"]], np.float64)
        rows = np.nonzero(np.abs(g).sum(1))[0]
        out[mode + ".grad_rows"], out[mode + ".grad"] = rows.astype(np.int64), g[rows]
        sel, it = [], iter(log)           # an image without rows is skipped by the reference: -1 for each of its labels
        for n, ls in zip(Z.COUNTS, Z.LABELS):
            sel += [next(it) if n else -1 for _ in ls]
        assert next(it, None) is None
        out[mode + ".sel"] = np.array(sel, np.int64)
        mine = Z.image_label_loss(d["scores"], None, d["boxes"], Z.COUNTS, Z.IMAGE_SIZES, Z.LABELS, mode, Z.WEIGHT)
        if mode == "min_loss":
            assert mine["crit_gap"] > 1e-3, mine["crit_gap"]
    # the cases the tests lean on occur: exact area tie for the maximum (last row larger still), exact score tie for the maximum
    r3 = Z.COUNTS[0] + Z.COUNTS[1]
    a = Z.area_f32(d["boxes"][r3:r3 + 40])
    assert a[4] == a[17] == a[:-1].max() and a[-1] > a[4] and int(np.argmax(a[:-1])) == 4
    s13 = d["scores"][r3:r3 + 40, 13]
    assert s13[6] == s13[30] == s13.max() and int(np.argmax(s13)) == 6
    off = sum(len(l) for l in Z.LABELS[:3])
    assert out["max_size.sel"][off] == 4 and out["max_score.sel"][off + Z.LABELS[3].index(13)] == 6
    assert sorted(len(l) for l in Z.LABELS) == [0, 1, 2, 3, 20] and len(set(Z.LABELS[3])) == 19
    assert len({tuple(out[m + ".sel"]) for m in Z.MODES}) == 5, "the five modes select differently"


def gen_proposals(out, d):
    dr = R.ref("divergen.modeling.roi_heads.detic_roi_heads")
    from detectron2.structures import Boxes, Instances
    for add in (False, True):
        me = types.SimpleNamespace(ws_num_props=Z.WS_NUM_PROPS, add_image_box=add, image_box_size=Z.IMAGE_BOX_SIZE)
        me._add_image_box = types.MethodType(dr.DeticCascadeROIHeads._add_image_box, me)
        props = []
        for i in range(3):
            keep = d["ws_valid"][i].astype(bool)          # the reference's lists hold the valid rows only
            p = Instances(Z.IMAGE_SIZES[i])
            p.proposal_boxes = Boxes(torch.from_numpy(d["ws_boxes"][i][keep]).clone())
            p.objectness_logits = torch.from_numpy(d["ws_scores"][i][keep]).clone()
            props.append(p)
        res = dr.DeticCascadeROIHeads.get_top_proposals(me, props)
        tag = "ws_box." if add else "ws."
        out[tag + "counts"] = np.array([len(p) for p in res], np.int64)
        out[tag + "boxes"] = torch.cat([p.proposal_boxes.tensor for p in res]).numpy()
        out[tag + "logits"] = torch.cat([p.objectness_logits for p in res]).numpy()
    assert list(out["ws.counts"]) == [5, 3, 0] and list(out["ws_box.counts"]) == [6, 4, 1]


def gen_handover(out, d):
    fr = R.ref("divergen.modeling.roi_heads.detic_fast_rcnn")
    dr = R.ref("divergen.modeling.roi_heads.detic_roi_heads")
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.box_regression import Box2BoxTransform
    from detectron2.structures import Boxes, Instances
    me = types.SimpleNamespace(training=True)
    props, r0 = [], 0
    for n, size in zip(Z.COUNTS, Z.IMAGE_SIZES):
        p = Instances(size)
        p.proposal_boxes = Boxes(torch.from_numpy(d["boxes"][r0:r0 + n]).clone())
        p.objectness_logits = torch.arange(r0, r0 + n, dtype=torch.float32)          # the row's identity travels here
        props.append(p)
        r0 += n
    for k in range(2):
        pred = fr.DeticFastRCNNOutputLayers(ShapeSpec(channels=8), box2box_transform=Box2BoxTransform(weights=Z.BOX_WEIGHTS[k]),
                                            num_classes=Z.C, cls_agnostic_bbox_reg=True, smooth_l1_beta=0.0, use_sigmoid_ce=True)
        alive = torch.cat([p.objectness_logits for p in props]).long()
        deltas = torch.from_numpy(d["deltas"][k])[alive]
        boxes = pred.predict_boxes((None, deltas), props)
        props = dr.DeticCascadeROIHeads._create_proposals_from_boxes(me, boxes, Z.IMAGE_SIZES, [p.objectness_logits for p in props])
        out["stage%d.rows" % (k + 1)] = torch.cat([p.objectness_logits for p in props]).long().numpy()
        out["stage%d.boxes" % (k + 1)] = torch.cat([p.proposal_boxes.tensor for p in props]).numpy()
    R_ = sum(Z.COUNTS)
    assert len(out["stage1.rows"]) == R_ - 1 and len(out["stage2.rows"]) == R_ - 2, "one row dropped per hand-over"


def gen_loader(out):
    cdl = R.ref("divergen.data.custom_dataset_dataloader")
    spec = importlib.util.spec_from_file_location("ref_distributed_sampler", R.D2 + "/data/samplers/distributed_sampler.py")
    ds = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ds)
    cdl.RepeatFactorTrainingSampler = ds.RepeatFactorTrainingSampler
    for ci, (sizes, ann, ratio, rfs, thr, seed) in enumerate(SAMPLER_CASES):
        dicts = Z.dataset_dicts(sizes, ann, seed=seed)
        for rank in (0, 1):
            cdl.comm = types.SimpleNamespace(get_rank=lambda r=rank: r, get_world_size=lambda: 2, shared_random_seed=lambda: 1)
            s = cdl.MultiDatasetSampler(dicts, list(ratio), list(rfs), list(ann), repeat_threshold=thr, seed=seed)
            if rank == 0:
                out["sampler%d.weights" % ci] = s.weights.numpy()
            stream = [int(i) for i in itertools.islice(iter(s), STREAM)]
            out["sampler%d.rank%d" % (ci, rank)] = np.array(stream, np.int64)
            for tag, grouped in (("md", cdl.MDAspectRatioGroupedDataset([dicts[i] for i in stream], 3, len(sizes))),
                                 ("diff", cdl.DIFFMDAspectRatioGroupedDataset([dicts[i] for i in stream], DIFF_BS[len(sizes)], len(sizes)))):
                batches = [[b["image_id"] for b in batch] for batch in grouped]
                assert len(batches) > 20 and len({dicts_by_id(dicts)[b[0]]["dataset_source"] for b in batches}) == len(sizes)
                out["sampler%d.rank%d.%s.len" % (ci, rank, tag)] = np.array([len(b) for b in batches], np.int64)
                out["sampler%d.rank%d.%s.ids" % (ci, rank, tag)] = np.array([i for b in batches for i in b], np.int64)
    dicts = Z.dataset_dicts((80,), ("image",), seed=21)
    out["tag_rfs"] = cdl.repeat_factors_from_tag_frequency(dicts, 0.05).numpy()
    assert out["tag_rfs"].max() > 1.5 and out["tag_rfs"].min() == 1.0


def dicts_by_id(dicts):
    return {d["image_id"]: d for d in dicts}


def main():
    _more_stubs()
    d = Z.inputs()
    out = {}
    gen_losses(out, d)
    gen_proposals(out, d)
    gen_handover(out, d)
    gen_loader(out)
    save_deterministic(os.path.join(HERE, "image_labels.npz"), out)


if __name__ == "__main__":
    main()
