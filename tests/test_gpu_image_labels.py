"""GPU tests of image-label co-training (WITH_IMAGE_LABELS): dgx_image_label_loss and dgx_ws_proposals against the float64
restatement (tests/_image_label_ref.py) and the reference's own outputs (tests/golden/image_labels.npz), the cascade hand-over
without ground truth, one image step and one box step of the assembled model, and a short training run on two sources."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _image_label_ref as Z  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
MODE_ID = {m: i for i, m in enumerate(Z.MODES)}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def run_kernel(scores_ld, C1, valid, boxes, counts, sizes, labels, mode, weight, upstream=None, sel_in=None, want_grad=True):
    """dgx_image_label_loss through the C ABI on a (R, ld) device tensor whose columns >= C1 are padding.  Returns out8, sel, and
    the FULL (R, ld) gradient buffer, which is filled with NaN before the launch: what the kernel leaves unwritten shows."""
    from divergen_amd import _lib as L
    lib = L.lib()
    R, ld = scores_ld.shape
    B = len(counts)
    row0 = (ctypes.c_int * (B + 1))(*np.concatenate([[0], np.cumsum(counts)]).astype(int).tolist())
    ih = (ctypes.c_float * B)(*[float(s[0]) for s in sizes])
    iw = (ctypes.c_float * B)(*[float(s[1]) for s in sizes])
    off = _i32(np.concatenate([[0], np.cumsum([len(l) for l in labels])]))
    flat = [l for ls in labels for l in ls]
    lab = _i32(flat) if flat else None
    out = torch.full((8,), float("nan"), device=DEV)
    sel = torch.full((max(len(flat), 1),), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(int(lib.dgx_image_label_workspace_floats(R, B)), 1), device=DEV)
    d = torch.full((max(R, 1), ld), float("nan"), dtype=scores_ld.dtype, device=DEV) if want_grad else None
    L.check(lib.dgx_image_label_loss(L.ptr(scores_ld) if R else None, ld, L.ptr(valid), L.ptr(boxes) if R else None, B, row0, ih, iw,
                                     L.ptr(off), L.ptr(lab), C1 - 1, MODE_ID[mode], float(weight), L.ptr(sel_in), L.ptr(upstream),
                                     None if sel_in is not None else L.ptr(sel), None if sel_in is not None else L.ptr(out), L.ptr(d), ld,
                                     None if sel_in is not None else L.ptr(ws), L.dtype_code(scores_ld), L.stream()), "dgx_image_label_loss")
    torch.cuda.synchronize()
    return out, sel, d


def padded(scores, ld, dtype):
    """(R, C1) float32 numpy -> (R, ld) device tensor of `dtype`, pad columns NaN; and the values as stored, in float64."""
    R, C1 = scores.shape
    t = torch.full((R, ld), float("nan"), dtype=dtype)
    t[:, :C1] = T(scores).to(dtype)
    return t.to(DEV), t[:, :C1].double().numpy()


def check_grad(d, ref, C1, dtype, counts, labels, sel, weight, scale=1.0, ref_is_fp32=False):
    """fp32: 1e-5 relative; bf16: one bf16 rounding, 2^-8 relative.  A row chosen by SEVERAL labels holds a sum of terms of magnitude
    up to coef = weight / (B L_i) each, which may cancel (n sigmoid(s) - 1): there the bound is relative to max(|value|, coef) --
    fp32 rounds each term, not the difference.  ref_is_fp32: the expected values are the reference's own fp32 gradient, which forms
    sigmoid(s) - 1 AFTER rounding sigmoid(s) to 2^-24: every selected row then carries that error of magnitude coef * 2^-24, so the
    same max(|value|, coef) bound applies to all of them.  Everything outside the selected rows and all pad columns: exactly zero."""
    d = d.float().cpu().numpy().astype(np.float64)
    ref = ref * scale
    assert np.all(d[:, C1:] == 0), "pad columns"
    rtol = 1e-5 if dtype == torch.float32 else 2.0 ** -8
    floor = np.zeros(d.shape[0])
    r0, k, B = 0, 0, len(counts)
    for n, ls in zip(counts, labels):
        rows = [sel[k + j] for j in range(len(ls)) if sel[k + j] >= 0]
        for r in set(rows):
            if rows.count(r) > 1 or ref_is_fp32:
                floor[r0 + r] = abs(scale) * weight / (B * len(ls))
        k += len(ls)
        r0 += n
    unsel = np.abs(ref).sum(1) == 0
    assert np.all(d[unsel] == 0), "unselected rows"
    tol = rtol * np.maximum(np.abs(ref), floor[:, None]) + 1e-30
    err = np.abs(d[:, :C1] - ref)
    assert np.all(err <= tol), "gradient: worst ratio %.3g" % float((err / tol).max())


def _case_rows(rng, C1):
    """Call A: rows per image 1, 2, 0, 129 (+ 6 for an image without labels); labels per image 3, 1, 2 (on the image without
    rows), 20 with one duplicate, 0.  In the 129-row image: an exact area tie for the maximum among all rows but the last, the last
    row largest; an exact score tie (9.5, exact in bf16) for the maximum of the first label."""
    counts = [1, 2, 0, 129, 6]
    sizes = [(200, 300), (240, 180), (128, 128), (512, 640), (100, 150)]
    labs = sorted(int(v) for v in rng.choice(C1, 19, replace=False))
    labels = [[0, C1 - 1, int(C1 // 2)], [1], [2, 3], labs + [labs[4]], []]
    R = sum(counts)
    scores = (rng.standard_normal((R, C1)) * 2.0 - 1.0).astype(np.float32)
    boxes = np.concatenate([Z.random_boxes(rng, n, s) for n, s in zip(counts, sizes)]).astype(np.float32)
    r3 = 3
    others = np.setdiff1d(np.arange(129), [70, 9])
    boxes[r3 + others, 2:] = np.minimum(boxes[r3 + others, 2:], boxes[r3 + others, :2] + 120.0)
    boxes[r3 + 70] = [10.0, 20.0, 202.0, 120.0]
    boxes[r3 + 9] = [50.0, 30.0, 150.0, 222.0]
    boxes[r3 + 128] = [0.0, 0.0, 640.0, 512.0]
    scores[r3 + 100, labs[0]] = scores[r3 + 31, labs[0]] = 9.5
    return counts, sizes, labels, scores, boxes, None


def _case_valid(rng, C1):
    """Call B: four images of 9 rows; validity bytes remove in turn the last row, a middle row, all rows, all rows but one."""
    counts, sizes = [9, 9, 9, 9], [(300, 300)] * 4
    labels = [[int(v) for v in rng.choice(C1, 3, replace=False)] for _ in range(4)]
    scores = (rng.standard_normal((36, C1)) * 2.0 - 1.0).astype(np.float32)
    boxes = np.concatenate([Z.random_boxes(rng, 9, s) for s in sizes]).astype(np.float32)
    boxes[8] = [0, 0, 300, 300]                      # the removed last row would have been the largest
    valid = np.ones(36, np.uint8)
    valid[8] = 0
    valid[9 + 4] = 0
    valid[18:27] = 0
    valid[27:36] = 0
    valid[27 + 5] = 1
    return counts, sizes, labels, scores, boxes, valid


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C1,ld", [(38, 40), (38, 38), (1204, 1208), (1454, 1464)])
@pytest.mark.parametrize("mode", Z.MODES)
def test_image_label_loss_against_float64(mode, C1, ld, dtype):
    """Selected rows equal, loss within 1e-5 relative of float64 on the stored inputs, gradient per check_grad, pad columns (NaN on
    input) and unselected rows exactly zero, two runs bit-identical; the gradient both from the forward launch and from a second
    launch that is given the selections and an upstream gradient on the device.  (38, 38): rows that are not 16-byte aligned in
    either dtype, logits and gradient both take the element-wise path."""
    rng = np.random.default_rng(100 + C1)
    for make in (_case_rows, _case_valid):
        counts, sizes, labels, scores, boxes, valid = make(rng, C1)
        x, stored = padded(scores, ld, dtype)
        v = T(valid).to(DEV) if valid is not None else None
        b = T(boxes).to(DEV)
        ref = Z.image_label_loss(stored, valid, boxes, counts, sizes, labels, mode, 0.1)
        out, sel, d = run_kernel(x, C1, v, b, counts, sizes, labels, mode, 0.1)
        nl = sum(len(l) for l in labels)
        assert sel[:nl].tolist() == ref["sel"], (mode, sel[:nl].tolist(), ref["sel"])
        o = out.double().cpu().numpy()
        assert abs(o[0] - ref["loss"]) <= 1e-5 * abs(ref["loss"]) and abs(o[1] - ref["l_image"]) <= 1e-5 * abs(ref["l_image"]), (o[:2], ref["loss"])
        np.testing.assert_allclose(o[2:7], ref["stats"], rtol=1e-5, atol=1e-7)
        check_grad(d, ref["grad"], C1, dtype, counts, labels, ref["sel"], 0.1)
        out2, sel2, d2 = run_kernel(x, C1, v, b, counts, sizes, labels, mode, 0.1)
        assert torch.equal(out, out2) and torch.equal(sel, sel2) and torch.equal(d.view(torch.uint8), d2.view(torch.uint8))
        up = torch.tensor([0.37], device=DEV)
        _, _, d3 = run_kernel(x, C1, v, b, counts, sizes, labels, mode, 0.1, upstream=up, sel_in=sel)
        check_grad(d3, ref["grad"], C1, dtype, counts, labels, ref["sel"], 0.1, scale=float(np.float32(0.37)))
    if make is _case_valid:
        assert ref["sel"][6:9] == [-1, -1, -1] and set(ref["sel"][9:12]) == {5}


@pytest.mark.parametrize("mode", Z.MODES)
def test_image_label_loss_against_reference(mode, golden):
    """The reference's own image_label_losses on the frozen inputs (contiguous 38-column fp32 scores: rows that are not 16-byte
    aligned take the element-wise path): loss and statistics to 1e-5, selected rows equal, gradient through the autograd node."""
    from divergen_amd.layers.image_label_ops import image_label_loss
    g, d = golden("image_labels"), Z.inputs()
    s = T(d["scores"]).to(DEV).requires_grad_(True)
    loss, out, sel = image_label_loss(s, None, T(d["boxes"]).to(DEV), Z.COUNTS, Z.IMAGE_SIZES, Z.LABELS, mode, Z.WEIGHT)
    (loss * 1.0).backward()
    assert sel.tolist() == g[mode + ".sel"].tolist()
    o = out.double().cpu().numpy()
    assert abs(o[0] - g[mode + ".loss"]) <= 1e-5 * abs(g[mode + ".loss"])
    assert abs(o[1] - g[mode + ".l_image"]) <= 1e-5 * abs(g[mode + ".l_image"])
    np.testing.assert_allclose(o[2:7], g[mode + ".stats"], rtol=1e-5, atol=1e-7)
    full = np.zeros(d["scores"].shape, np.float64)
    full[g[mode + ".grad_rows"]] = g[mode + ".grad"]
    check_grad(s.grad, full, Z.C + 1, torch.float32, Z.COUNTS, Z.LABELS, sel.tolist(), Z.WEIGHT, ref_is_fp32=True)


def test_image_label_loss_degenerate_and_refusals():
    """R <= 0 is safe and gives a zero loss; a broken contract is DGX_ERR_BAD_ARG; CPU tensors are refused."""
    from divergen_amd import _lib as L
    from divergen_amd.layers.image_label_ops import image_label_loss
    x = torch.zeros(0, 38, device=DEV, requires_grad=True)
    loss, out, sel = image_label_loss(x, None, torch.zeros(0, 4, device=DEV), [0, 0], [(10, 10)] * 2, [[1], []], "max_size", 0.1)
    loss.backward()
    assert float(loss.detach()) == 0.0 and out.tolist() == [0.0] * 8 and sel.tolist() == [-1]
    lib = L.lib()
    row0 = (ctypes.c_int * 2)(0, 4)
    f1 = (ctypes.c_float * 1)(10.0)
    buf = torch.zeros(4, 40, device=DEV)
    off, o8, s1, ws = _i32([0, 0]), torch.zeros(8, device=DEV), _i32([0]), torch.zeros(64, device=DEV)
    common = (L.ptr(buf), 40, None, L.ptr(buf), 1, row0, f1, f1, L.ptr(off), None)
    assert lib.dgx_image_label_loss(*common, 37, 9, 0.1, None, None, L.ptr(s1), L.ptr(o8), None, 0, L.ptr(ws), 0, L.stream()) == -1      # mode
    assert lib.dgx_image_label_loss(*common, 40, 0, 0.1, None, None, L.ptr(s1), L.ptr(o8), None, 0, L.ptr(ws), 0, L.stream()) == -1      # ld < C + 1
    assert lib.dgx_image_label_loss(*common, 37, 0, 0.1, None, None, None, L.ptr(o8), None, 0, L.ptr(ws), 0, L.stream()) == -1            # no sel_out
    assert lib.dgx_image_label_loss(*common[:4], 33, *common[5:], 37, 0, 0.1, None, None, L.ptr(s1), L.ptr(o8), None, 0, L.ptr(ws), 0, L.stream()) == -1
    row1 = (ctypes.c_int * 2)(1, 4)
    assert lib.dgx_image_label_loss(*common[:5], row1, *common[6:], 37, 0, 0.1, None, None, L.ptr(s1), L.ptr(o8), None, 0, L.ptr(ws), 0, L.stream()) == -1      # row0[0] != 0
    with pytest.raises(L.DgxError):
        image_label_loss(torch.zeros(2, 38), None, torch.zeros(2, 4), [2], [(10, 10)], [[1]], "first", 0.1)


# ------------------------------------------------------------------------------------------------ proposals, hand-over
@pytest.mark.parametrize("add", [False, True], ids=["plain", "image_box"])
def test_ws_proposals_against_reference(add, golden):
    """get_top_proposals / _add_image_box of the reference on lists with holes, a short list and an empty one: the valid rows equal the
    reference's rows in order, boxes to 1e-5; the padding is zero rows with valid = 0; K = 300 > one pass of the workgroup."""
    from divergen_amd.layers.image_label_ops import ws_proposals
    g, d = golden("image_labels"), Z.inputs()
    tag = "ws_box." if add else "ws."
    ob, ol, ov, Ko = ws_proposals(T(d["ws_boxes"]).to(DEV), T(d["ws_scores"]).to(DEV), T(d["ws_valid"]).to(DEV), Z.IMAGE_SIZES[:3],
                                  Z.WS_NUM_PROPS, add, Z.IMAGE_BOX_SIZE)
    assert Ko == Z.WS_NUM_PROPS + int(add)
    rb, rl, rv = Z.ws_proposals(d["ws_boxes"], d["ws_scores"], d["ws_valid"], Z.IMAGE_SIZES[:3], Z.WS_NUM_PROPS, add, Z.IMAGE_BOX_SIZE)
    assert ov.cpu().numpy().tolist() == rv.tolist()
    assert np.array_equal(ob.cpu().numpy(), rb) and np.array_equal(ol.cpu().numpy(), rl)
    keep = ov.cpu().numpy().astype(bool)
    assert [int(c) for c in keep.reshape(3, Ko).sum(1)] == g[tag + "counts"].tolist()
    np.testing.assert_allclose(ob.cpu().numpy()[keep], g[tag + "boxes"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(ol.cpu().numpy()[keep], g[tag + "logits"])
    # a long list: 300 candidates, every third one invalid, 128 wanted
    rng = np.random.default_rng(5)
    bx = np.stack([Z.random_boxes(rng, 300, (400, 500)) for _ in range(2)]) + np.float32(30.0)
    sc = rng.uniform(0, 1, (2, 300)).astype(np.float32)
    va = (np.arange(600).reshape(2, 300) % 3 != 0).astype(np.uint8)
    va[1, 150:] = 0
    ob, ol, ov, Ko = ws_proposals(T(bx).to(DEV), T(sc).to(DEV), T(va).to(DEV).view(torch.bool), [(400, 500)] * 2, 128, add, 1.0)
    rb, rl, rv = Z.ws_proposals(bx, sc, va, [(400, 500)] * 2, 128, add, 1.0)
    assert np.array_equal(ob.cpu().numpy(), rb) and np.array_equal(ol.cpu().numpy(), rl) and np.array_equal(ov.cpu().numpy(), rv)
    assert rv.reshape(2, Ko)[:, :128].sum(1).tolist() == [128, 100]


def test_handover_without_ground_truth_against_reference(golden):
    """predict_boxes -> _create_proposals_from_boxes of the reference over three stages, against dgx_cascade_refine with zero ground
    truth and valid_in: the rows the reference keeps are the rows with valid = 1, in order; their boxes to 1e-5."""
    from divergen_amd import _lib as L
    g, d = golden("image_labels"), Z.inputs()
    B, R = len(Z.COUNTS), sum(Z.COUNTS)
    row0 = (ctypes.c_int * (B + 1))(*np.concatenate([[0], np.cumsum(Z.COUNTS)]).astype(int).tolist())
    gt0 = (ctypes.c_int * (B + 1))(*([0] * (B + 1)))
    ih = (ctypes.c_float * B)(*[float(s[0]) for s in Z.IMAGE_SIZES])
    iw = (ctypes.c_float * B)(*[float(s[1]) for s in Z.IMAGE_SIZES])
    prop, valid = T(d["boxes"]).to(DEV), None
    rb, rv = d["boxes"], None
    for k in range(2):
        w = Z.BOX_WEIGHTS[k]
        dl = T(d["deltas"][k]).to(DEV)
        nb, nv = torch.empty(R, 4, device=DEV), torch.empty(R, dtype=torch.uint8, device=DEV)
        cls, gtb = torch.empty(R, dtype=torch.int64, device=DEV), torch.empty(R, 4, device=DEV)
        nfg = torch.empty(1, dtype=torch.int32, device=DEV)
        L.check(L.lib().dgx_cascade_refine(L.ptr(prop), L.ptr(dl), L.ptr(valid), B, row0, gt0, ih, iw, None, None, None, 0.6, Z.C,
                                           w[0], w[1], w[2], w[3], Z.SCALE_CLAMP, L.ptr(nb), L.ptr(nv), L.ptr(cls), L.ptr(gtb), None,
                                           L.ptr(nfg), 0, L.stream()), "dgx_cascade_refine")
        prop, valid = nb, nv
        rb, rv = Z.refine(rb, d["deltas"][k], rv, Z.COUNTS, Z.IMAGE_SIZES, w)
        alive = np.nonzero(nv.cpu().numpy())[0]
        assert alive.tolist() == g["stage%d.rows" % (k + 1)].tolist() == np.nonzero(rv)[0].tolist()
        np.testing.assert_allclose(nb.cpu().numpy()[alive], g["stage%d.boxes" % (k + 1)], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(rb[alive], g["stage%d.boxes" % (k + 1)], rtol=1e-5, atol=1e-5)
        assert int(nfg) == 0


# ------------------------------------------------------------------------------------------------ the assembled model
FREQ = os.path.join(ROOT, "configs", "metadata", "lvis_v1_train_cat_info.json")
LOSS_KEYS = {"%s_stage%d" % (n, k) for n in ("image_loss", "loss_cls", "loss_box_reg") for k in range(3)} | {
    "loss_mask", "loss_centernet_loc", "loss_centernet_agn_pos", "loss_centernet_agn_neg"}


def _build(tmp, zeroshot, mode="max_size"):
    from divergen_amd.config import get_cfg
    from divergen_amd.modeling import build_model
    from divergen_amd.modeling.backbone.swintransformer import DropPath
    from divergen_amd.solver import build_optimizer
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "DiverGen_swinL.yaml"))
    opts = ["MODEL.SWIN.SIZE", "T", "WITH_IMAGE_LABELS", True, "MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", mode, "MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX", True,
            "MODEL.ROI_BOX_HEAD.WS_NUM_PROPS", 32, "MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", FREQ]
    C = None
    if zeroshot:
        C = 37
        npy = os.path.join(str(tmp), "emb.npy")
        np.save(npy, np.random.default_rng(3).standard_normal((C, 512)).astype(np.float32))
        opts += ["MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", True, "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", npy, "MODEL.ROI_HEADS.NUM_CLASSES", C,
                 "MODEL.ROI_BOX_HEAD.USE_BIAS", -4.6, "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False]
    cfg.merge_from_list(opts)
    C = int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
    torch.manual_seed(42)
    model = build_model(cfg).train()
    for m in model.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    return cfg, model, build_optimizer(cfg, model), C


def _zero(params):
    return all(p.grad is None or not bool(p.grad.any()) for p in params)


@pytest.mark.parametrize("zeroshot", [False, True], ids=["linear", "zeroshot"])
def test_image_step_and_box_step_of_the_assembled_model(zeroshot, tmp_path):
    """One image-labelled step and one box step of the registry-built Swin-T model at 256 px: image_loss_stage{k} equals the
    restatement on the scores and boxes the stage saw (1e-5), the reported zeros are exact zeros, both steps carry the same key
    set; after the image step's backward the mask head and bbox_pred have exactly zero gradients while cls_score, the box-head FCs
    and the backbone do not."""
    from divergen_amd.data import synthetic_batch
    from divergen_amd.engine import total_loss
    from divergen_amd.structures import BitMasks, Boxes, Instances
    from divergen_amd.utils.events import EventStorage
    cfg, model, opt, C = _build(tmp_path, zeroshot)
    box_batch = synthetic_batch(2, 256, C, device=DEV)
    for d in box_batch:
        d.update(ann_type="box", pos_category_ids=[], dataset_source=0)
    labels = [[3, 11, C - 1], [5]]
    img_batch = []
    for d, ls in zip(synthetic_batch(2, 256, C, device=DEV), labels):
        h, w = d["image"].shape[-2:]
        inst = Instances((h, w), gt_boxes=Boxes(torch.zeros(0, 4, device=DEV)), gt_classes=torch.zeros(0, dtype=torch.int64, device=DEV),
                         gt_masks=BitMasks(torch.zeros(0, h, w, dtype=torch.bool, device=DEV)))
        img_batch.append(dict(d, instances=inst, ann_type="image", pos_category_ids=ls, dataset_source=1))
    seen = []
    model.roi_heads.__dict__["stage_observer"] = lambda k, d: seen.append((k, d))
    rh = model.roi_heads
    with EventStorage(0) as st:
        opt.zero_grad()
        losses = model(img_batch)
        total_loss(losses).backward()
        torch.cuda.synchronize()
        assert set(losses) == LOSS_KEYS, sorted(losses)
        assert len(seen) == 3
        for k, d in seen:
            assert d["counts"] == [33, 33] and d["scores"].shape == (66, C + 1)
            ref = Z.image_label_loss(d["scores"].detach().double().cpu().numpy(), None if d["valid"] is None else d["valid"].cpu().numpy(),
                                     d["boxes"].cpu().numpy(), d["counts"], d["image_sizes"], labels, "max_size", 0.1)
            got = float(losses["image_loss_stage%d" % k].detach())
            print("stage %d image_loss %.9g restatement %.9g" % (k, got, ref["loss"]))
            assert ref["loss"] > 0 and abs(got - ref["loss"]) <= 1e-5 * ref["loss"]
        for n, v in losses.items():
            if not n.startswith("image_loss"):
                assert float(v) == 0.0 and bool(torch.isfinite(v)), n
        assert _zero(rh.mask_head.parameters()), "mask head"
        for k in range(3):
            assert _zero(rh.box_predictor[k].bbox_pred.parameters()), "bbox_pred %d" % k
            assert not _zero(rh.box_predictor[k].cls_score.parameters()), "cls_score %d" % k
            assert not _zero(rh.box_head[k].parameters()), "box head %d" % k
        assert not _zero(model.backbone.parameters())
        assert _zero(model.proposal_generator.parameters()), "the proposal generator's losses are reported as zeros"
        opt.step()
        # a box step of the same model: same keys, image losses exactly zero, everything trains
        seen.clear()
        opt.zero_grad()
        bl = model(box_batch)
        total_loss(bl).backward()
        torch.cuda.synchronize()
        assert set(bl) == LOSS_KEYS
        for k in range(3):
            assert float(bl["image_loss_stage%d" % k].detach()) == 0.0 and float(bl["loss_cls_stage%d" % k].detach()) > 0
            assert not _zero(rh.box_predictor[k].bbox_pred.parameters())
        assert not _zero(rh.mask_head.parameters()) and not _zero(model.proposal_generator.parameters())
        assert all(bool(torch.isfinite(v)) for v in bl.values())
        if zeroshot:
            # a per-call vocabulary (classifier_info[0]) on an image step: 7 classes + background, image_loss from those scores
            emb2 = torch.from_numpy(np.random.default_rng(4).standard_normal((8, 512)).astype(np.float32)).to(DEV)
            plain = rh.forward
            rh.forward = lambda *a, **k: plain(*a, **dict(k, classifier_info=(emb2, None, None)))
            try:
                seen.clear()
                opt.zero_grad()
                small = [dict(d, pos_category_ids=ls) for d, ls in zip(img_batch, [[0, 6], [3]])]
                cl = model(small)
                total_loss(cl).backward()
                torch.cuda.synchronize()
            finally:
                del rh.forward
            assert set(cl) == LOSS_KEYS and len(seen) == 3
            for k, d in seen:
                assert d["scores"].shape == (66, 8)
                ref = Z.image_label_loss(d["scores"].detach().double().cpu().numpy(), None if d["valid"] is None else d["valid"].cpu().numpy(),
                                         d["boxes"].cpu().numpy(), d["counts"], d["image_sizes"], [[0, 6], [3]], "max_size", 0.1)
                got = float(cl["image_loss_stage%d" % k].detach())
                assert ref["loss"] > 0 and abs(got - ref["loss"]) <= 1e-5 * ref["loss"]
            assert not _zero(rh.box_predictor[0].cls_score.parameters())
            with pytest.raises(NotImplementedError, match="classifier_info"):
                rh.forward = lambda *a, **k: plain(*a, **dict(k, classifier_info=(emb2, None, None)))
                try:
                    model(box_batch)
                finally:
                    del rh.forward


def test_do_train_on_two_sources(tmp_path, monkeypatch):
    """train_net.do_train for 6 iterations on a generated box source + image-labelled source, 2 workers, DATASET_BS [2, 4]: both
    annotation types occur, losses are finite, metrics.json carries the image_loss_* keys, --resume continues."""
    import json
    sys.path.insert(0, ROOT)
    import train_net
    from divergen_amd.modeling import build_model
    from divergen_amd.modeling.meta_arch.custom_rcnn import CustomRCNN
    from test_host_image_labels import _two_source_cfg
    cfg, info = _two_source_cfg(tmp_path, monkeypatch, [
        "DATALOADER.NUM_WORKERS", 2, "DATALOADER.USE_DIFF_BS_SIZE", True, "DATALOADER.DATASET_BS", [2, 4], "DATALOADER.DATASET_INPUT_SIZE", [128, 128],
        "DATALOADER.DATASET_INPUT_SCALE", [[0.3, 1.2], [0.8, 1.2]], "SOLVER.MAX_ITER", 6, "SOLVER.CHECKPOINT_PERIOD", 100, "SOLVER.WARMUP_ITERS", 2,
        "SEED", 7, "MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX", True])
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    kinds = []
    orig = CustomRCNN._annotation_type

    def spy(self, batched_inputs, gt):
        kinds.append((orig(self, batched_inputs, gt), len(batched_inputs)))
        return kinds[-1][0]
    monkeypatch.setattr(CustomRCNN, "_annotation_type", spy)
    torch.manual_seed(7)
    opt = train_net.do_train(cfg, build_model(cfg))
    assert len(kinds) == 6 and {k for k, _ in kinds} == {"box", "image"}, kinds
    assert all(n == (2 if k == "box" else 4) for k, n in kinds)
    out = str(tmp_path / "out")
    rows = [json.loads(line) for line in open(os.path.join(out, "metrics.json"))]
    seen = set().union(*[set(r) for r in rows])
    assert {"image_loss_stage0", "image_loss_stage1", "image_loss_stage2", "loss_cls_stage0", "loss_mask", "total_loss"} <= seen, sorted(seen)
    assert all(np.isfinite(r["total_loss"]) for r in rows if "total_loss" in r)
    p_end = opt.arena.p.clone()
    cfg2 = cfg.clone()
    cfg2.defrost()
    cfg2.merge_from_list(["SOLVER.MAX_ITER", 9])
    opt2 = train_net.do_train(cfg2, build_model(cfg2), resume=True)
    ck = torch.load(os.path.join(out, "model_final.pth"), map_location="cpu", weights_only=False)
    # (the checkpoint of the first run says iteration 6; the loop counts from 1 and resumes behind it: iterations 8 and 9)
    assert ck["iteration"] == 9 and float((opt2.arena.p - p_end).abs().max()) > 0 and len(kinds) == 8
