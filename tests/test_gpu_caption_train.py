"""GPU tests of caption training in the assembled model (MODEL.CAPTION_TRAIN, MODEL.WITH_CAPTION): one 'caption', one 'captiontag' and
one box step of the registry-built Swin-T model with a two-layer test text encoder, the same caption step under
MODEL.SYNC_CAPTION_BATCH in a one-rank process group, and a short training run on a box source + a 'captiontag' source.

Bound of the stage losses: the restatement (tests/_caption_loss_ref.py) on what the stage saw -- the projected rows u as stored (bf16),
the validity bytes, the prepared caption rows -- at rtol 1e-5 relative to max(|loss|, floor) (the bound of tests/test_gpu_caption_loss.py:
the kernel's arithmetic is fp32 from the stored inputs); the image-label part of a 'captiontag' stage is held to tests/_image_label_ref.py
at 1e-5 as in tests/test_gpu_image_labels.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _caption_fixtures as F  # noqa: E402
import _caption_loss_ref as C  # noqa: E402
import _image_label_ref as Z  # noqa: E402

DEV = "cuda"
RTOL = 1e-5
FREQ = os.path.join(ROOT, "configs", "metadata", "lvis_v1_train_cat_info.json")
LOSS_KEYS = {"%s_stage%d" % (n, k) for n in ("image_loss", "loss_cls", "loss_box_reg") for k in range(3)} | {
    "loss_mask", "loss_centernet_loc", "loss_centernet_agn_pos", "loss_centernet_agn_neg"}
NCLS = 37
CAPTIONS = [["low lower newer", "a row of lows"], ["newer new low", "low", "lower lower a new row"]]
LABELS = [[3, 11, NCLS - 1], [5]]


def _build(tmp, caption=True, sync=False):
    from divergen_amd.config import get_cfg
    from divergen_amd.modeling import build_model
    from divergen_amd.modeling.backbone.swintransformer import DropPath
    from divergen_amd.solver import build_optimizer
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "DiverGen_swinL.yaml"))
    os.makedirs(str(tmp), exist_ok=True)
    npy = os.path.join(str(tmp), "emb.npy")
    np.save(npy, np.random.default_rng(3).standard_normal((NCLS, 512)).astype(np.float32))
    opts = ["MODEL.SWIN.SIZE", "T", "WITH_IMAGE_LABELS", True, "MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "max_size", "MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX", True,
            "MODEL.ROI_BOX_HEAD.WS_NUM_PROPS", 32, "MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", FREQ, "MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", True,
            "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", npy, "MODEL.ROI_HEADS.NUM_CLASSES", NCLS, "MODEL.ROI_BOX_HEAD.USE_BIAS", -4.6,
            "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False, "MODEL.ROI_BOX_HEAD.CAPTION_WEIGHT", 0.5]
    if caption:
        opts += F.caption_opts(*F.write_text_encoder(os.path.join(str(tmp), "enc")), sync=sync)
    cfg.merge_from_list(opts)
    torch.manual_seed(42)
    model = build_model(cfg).train()
    for m in model.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    return cfg, model, build_optimizer(cfg, model)


def _batches(ann_type):
    from divergen_amd.data import synthetic_batch
    from divergen_amd.structures import BitMasks, Boxes, Instances
    box = synthetic_batch(2, 256, NCLS, device=DEV)
    for d in box:
        d.update(ann_type="box", pos_category_ids=[], dataset_source=0)
    cap = []
    for d, ls, cs in zip(synthetic_batch(2, 256, NCLS, device=DEV), LABELS, CAPTIONS):
        h, w = d["image"].shape[-2:]
        inst = Instances((h, w), gt_boxes=Boxes(torch.zeros(0, 4, device=DEV)), gt_classes=torch.zeros(0, dtype=torch.int64, device=DEV),
                         gt_masks=BitMasks(torch.zeros(0, h, w, dtype=torch.bool, device=DEV)))
        cap.append(dict(d, instances=inst, ann_type=ann_type, pos_category_ids=ls if ann_type == "captiontag" else [], dataset_source=1,
                        captions=cs))
    return box, cap


def _zero(params):
    return all(p.grad is None or not bool(p.grad.any()) for p in params)


def _observe(rh):
    seen = []
    rh.__dict__["stage_observer"] = lambda k, d: seen.append((k, {n: (v.detach().clone() if torch.is_tensor(v) else v) for n, v in d.items()}))
    return seen


def _check_stage(model, k, d, loss, ann_type, cfg, target0=0, neg_weight=1.0):
    """image_loss of stage k against the restatement on what the stage saw; returns the restated caption part."""
    h = cfg.MODEL.ROI_BOX_HEAD
    pred = model.roi_heads.box_predictor[k]
    cap = d["captions"]
    B = len(d["counts"])
    assert cap.n == cap.rows.shape[0] and cap.dim == 512 and cap.target0 == target0 and cap.neg_weight == neg_weight
    assert d["u"].dtype == torch.bfloat16 and d["u"].shape[1] == 512 and d["u"].shape[0] >= sum(d["counts"])
    valid = None if d["valid"] is None else d["valid"].cpu().numpy()
    # (the observed caption rows are the prepared ones: normalising them again changes nothing beyond the last bit, and u is normalised here)
    r = C.caption_loss(d["u"].double().cpu().numpy(), valid, d["counts"], cap.rows.double().cpu().numpy(), 512, target0, float(h.NORM_TEMP), True,
                       float(pred.cls_score.cls_bias.detach()), neg_weight, h.CAPTION_WEIGHT * h.IMAGE_LOSS_WEIGHT / B, h.CAPTION_WEIGHT / B)
    want, floor = r["loss"], r["floor_loss"]
    if ann_type == "captiontag":
        assert d["scores"].shape == (sum(d["counts"]), NCLS + 1)
        il = Z.image_label_loss(d["scores"].double().cpu().numpy(), valid, d["boxes"].cpu().numpy(), d["counts"], d["image_sizes"], LABELS, "max_size",
                                float(h.IMAGE_LOSS_WEIGHT))
        assert il["loss"] > 0
        want, floor = want + il["loss"], floor + il["loss"]
    else:
        assert d["scores"] is None, "a pure caption step forms no class scores"
    got = float(loss)
    print("stage %d %s image_loss %.9g restatement %.9g (caption part %.9g)" % (k, ann_type, got, want, r["loss"]))
    assert r["loss"] > 0 and abs(got - want) <= RTOL * max(abs(want), floor)
    return r


@pytest.mark.parametrize("ann_type", ["caption", "captiontag"])
def test_caption_step_of_the_assembled_model(ann_type, tmp_path):
    """One caption step: the loss keys of every step, image_loss_stage{k} equal to the restatement on what the stage saw, exact zeros for
    loss_cls / loss_box_reg / the proposal losses, stats_l_caption logged, gradients in cls_score.linear and cls_bias (none in bbox_pred,
    the mask head and the proposal generator), the text encoder bit-identical after the optimizer step."""
    from divergen_amd.engine import total_loss
    from divergen_amd.utils.events import EventStorage
    cfg, model, opt = _build(tmp_path)
    rh = model.roi_heads
    _, cap_batch = _batches(ann_type)
    seen = _observe(rh)
    enc_before = {n: p.detach().clone() for n, p in model.text_encoder.named_parameters()}
    assert not any(n.startswith("text_encoder.") for n in opt.arena.names)
    with EventStorage(0) as st:
        opt.zero_grad()
        torch.manual_seed(5)
        losses = model(cap_batch)
        total_loss(losses).backward()
        torch.cuda.synchronize()
        assert set(losses) == LOSS_KEYS, sorted(losses)
        assert len(seen) == 3
        for k, d in seen:
            assert d["counts"] == [33, 33]
            r = _check_stage(model, k, d, losses["image_loss_stage%d" % k].detach(), ann_type, cfg)
            assert r["sel"] == [32, 32] or d["valid"] is not None
        for n, v in losses.items():
            if not n.startswith("image_loss"):
                assert float(v) == 0.0 and bool(torch.isfinite(v)), n
        latest = st.latest()
        assert float(latest["stage2/stats_l_caption"][0]) > 0
        if ann_type == "caption":
            assert all(float(latest["stage2/" + n][0]) == 0.0 for n in ("stats_l_image", "pool_stats", "stats_select_size", "stats_max_label_score"))
        for k in range(3):
            cs = rh.box_predictor[k].cls_score
            assert not _zero([cs.linear.weight]) and not _zero([cs.cls_bias]), "cls_score %d" % k
            assert _zero(rh.box_predictor[k].bbox_pred.parameters()), "bbox_pred %d" % k
            assert not _zero(rh.box_head[k].parameters()), "box head %d" % k
        assert _zero(rh.mask_head.parameters()) and _zero(model.proposal_generator.parameters()) and not _zero(model.backbone.parameters())
        opt.step()
        torch.cuda.synchronize()
    for n, p in model.text_encoder.named_parameters():
        assert p.grad is None and torch.equal(p.detach(), enc_before[n]), n


def test_box_step_is_bit_equal_with_and_without_the_text_encoder(tmp_path):
    """A box step of the model built with WITH_CAPTION (SYNC off) against the same step of the model built without: every loss bit-equal."""
    from divergen_amd.engine import total_loss
    from divergen_amd.utils.events import EventStorage
    out = []
    for caption in (True, False):
        cfg, model, opt = _build(tmp_path / str(caption), caption=caption)
        box, _ = _batches("caption")
        with EventStorage(0):
            opt.zero_grad()
            torch.manual_seed(9)
            losses = model(box)
            total_loss(losses).backward()
            torch.cuda.synchronize()
        assert set(losses) == LOSS_KEYS
        out.append({k: v.detach().clone() for k, v in losses.items()})
        del model, opt
    for k in LOSS_KEYS:
        assert torch.equal(out[0][k], out[1][k]), k
        assert float(out[0][k]) == 0.0 if k.startswith("image_loss") else bool(torch.isfinite(out[0][k]))


def test_synced_caption_step_in_a_one_rank_group(tmp_path):
    """MODEL.SYNC_CAPTION_BATCH in a one-rank RCCL group: the gather runs (N = B rows with the rank column), the negatives carry
    NEG_CAP_WEIGHT, every stage matches the restatement; a box step with the flag on gathers too and still trains like one without."""
    import torch.distributed as dist
    from divergen_amd.engine import total_loss
    from divergen_amd.layers import caption_ops
    from divergen_amd.utils.events import EventStorage
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.setdefault("NCCL_MAX_NCHANNELS", "16")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        cfg, model, opt = _build(tmp_path, sync=True)
        box, cap_batch = _batches("caption")
        gathered = []
        plain = caption_ops.all_gather_rows
        caption_ops.all_gather_rows = lambda rows: (gathered.append(tuple(rows.shape)), plain(rows))[1]
        seen = _observe(model.roi_heads)
        try:
            with EventStorage(0):
                opt.zero_grad()
                torch.manual_seed(5)
                losses = model(cap_batch)
                total_loss(losses).backward()
                torch.cuda.synchronize()
                assert gathered == [(2, 513)] and set(losses) == LOSS_KEYS and len(seen) == 3
                for k, d in seen:
                    _check_stage(model, k, d, losses["image_loss_stage%d" % k].detach(), "caption", cfg, target0=0,
                                 neg_weight=float(cfg.MODEL.ROI_BOX_HEAD.NEG_CAP_WEIGHT))
                opt.zero_grad()
                torch.manual_seed(9)
                bl = model(box)
                total_loss(bl).backward()
                torch.cuda.synchronize()
                assert gathered == [(2, 513), (2, 513)], "a box step sends BS * CAP_BATCH_RATIO zero rows"
                assert set(bl) == LOSS_KEYS and all(bool(torch.isfinite(v)) for v in bl.values())
                assert all(float(bl["loss_cls_stage%d" % k]) > 0 and float(bl["image_loss_stage%d" % k]) == 0.0 for k in range(3))
        finally:
            caption_ops.all_gather_rows = plain
        synced_box = {k: v.detach().clone() for k, v in bl.items()}
        del model, opt
        cfg, model, opt = _build(tmp_path / "plain", sync=False)
        with EventStorage(0):
            opt.zero_grad()
            torch.manual_seed(9)
            bl = model(box)
        for k in LOSS_KEYS:
            assert torch.equal(bl[k].detach(), synced_box[k]), k
    finally:
        dist.destroy_process_group()


def test_do_train_on_a_box_and_a_captiontag_source(tmp_path, monkeypatch):
    """train_net.do_train for 6 iterations on a generated box source + a captioned image source ('captiontag'), 2 workers, DATASET_BS
    [2, 4]: both kinds of step occur, every step is finite, metrics.json carries stats_l_caption."""
    import json
    sys.path.insert(0, ROOT)
    import train_net
    from divergen_amd.modeling import build_model
    from divergen_amd.modeling.meta_arch.custom_rcnn import CustomRCNN
    cfg, info, _ = F.two_source_cfg(tmp_path, monkeypatch, extra=[
        "DATALOADER.NUM_WORKERS", 2, "DATALOADER.USE_DIFF_BS_SIZE", True, "DATALOADER.DATASET_BS", [2, 4], "DATALOADER.DATASET_INPUT_SIZE", [128, 128],
        "DATALOADER.DATASET_INPUT_SCALE", [[0.3, 1.2], [0.8, 1.2]], "SOLVER.MAX_ITER", 6, "SOLVER.CHECKPOINT_PERIOD", 100, "SOLVER.WARMUP_ITERS", 2,
        "SEED", 7])
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    kinds = []
    orig = CustomRCNN._annotation_type

    def spy(self, batched_inputs, gt):
        kinds.append((orig(self, batched_inputs, gt), len(batched_inputs)))
        return kinds[-1][0]
    monkeypatch.setattr(CustomRCNN, "_annotation_type", spy)
    torch.manual_seed(7)
    train_net.do_train(cfg, build_model(cfg))
    assert len(kinds) == 6 and {k for k, _ in kinds} == {"box", "captiontag"}, kinds
    assert all(n == (2 if k == "box" else 4) for k, n in kinds)
    rows = [json.loads(line) for line in open(os.path.join(str(tmp_path / "out"), "metrics.json"))]
    seen = set().union(*[set(r) for r in rows])
    assert {"image_loss_stage0", "image_loss_stage2", "loss_cls_stage0", "loss_mask", "total_loss"} <= seen, sorted(seen)
    assert any(k.endswith("stats_l_caption") for k in seen), sorted(seen)
    assert all(np.isfinite(r["total_loss"]) for r in rows if "total_loss" in r)
