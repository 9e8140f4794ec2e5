"""GPU tests of the WSDDN image-label loss (MODEL.ROI_BOX_HEAD.WS_PROP_SCORE, IMAGE_LABEL_LOSS 'wsddn', WITH_SOFTMAX_PROP):
dgx_wsddn_loss through the C ABI against the float64 restatement (tests/_wsddn_ref.py), the golden inputs against the reference's own
fp32 outputs (tests/golden/wsddn.npz), the proposal-score branch against the reference's forward, one image step and one box step
of the assembled model, and a short training run on two sources.

Tolerance.  Gradients: |got - ref| <= rtol * max(|ref|, floor), floor = the restatement's sum of absolute addends per element.
tests/golden/make_golden_wsddn.py measured the reference's OWN fp32 evaluation against the restatement in that form at rtol = 1e-5, on
the golden inputs and on the inputs of this file (tests/_wsddn_ref.gpu_cases: widths 38 / 1204 / 1454, values as stored in fp32 and in
bf16): worst ratio 0.098 (loss), 0.128 / 0.122 (the two gradients) on the golden inputs, 0.018 / 0.760 / 0.767 on the inputs here.  The
reference stays inside the bound, so the chosen rtol is 1e-5, the project's bound for fp32.  bf16 OUTPUTS add one bf16 rounding of the
value, 2^-8 |ref| (the project's figure: half an ulp of an 8-bit significand is at most 2^-8 of the value).  The loss is fp32 from the stored inputs in either dtype: 1e-5.
The golden inputs hold the hard cases (S below 1e-10, S near 1 - 1e-3, the exact-1.0f column, the constructed tie): there the kernel's
gradients are held to the restatement AND to the reference's fp32 gradients, both at rtol = 1e-5."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _wsddn_ref as W  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
RTOL = 1e-5


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def run_kernel(x, q, C1, valid, boxes, counts, sizes, labels, weight, upstream=None, stats_in=None, want_grad=True):
    """dgx_wsddn_loss through the C ABI on (R, ld) device tensors whose columns >= C1 are padding.  Returns out8, sel, the FULL (R, ld)
    gradient buffers (NaN-filled before the launch: what the kernel leaves unwritten shows) and the workspace."""
    from divergen_amd import _lib as L
    lib = L.lib()
    R, ld = x.shape
    B = len(counts)
    row0 = (ctypes.c_int * (B + 1))(*np.concatenate([[0], np.cumsum(counts)]).astype(int).tolist())
    ih = (ctypes.c_float * B)(*[float(s[0]) for s in sizes])
    iw = (ctypes.c_float * B)(*[float(s[1]) for s in sizes])
    off = _i32(np.concatenate([[0], np.cumsum([len(l) for l in labels])]))
    flat = [l for ls in labels for l in ls]
    lab = _i32(flat) if flat else None
    fwd = stats_in is None
    out = torch.full((8,), float("nan"), device=DEV)
    sel = torch.full((max(len(flat), 1),), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((max(int(lib.dgx_wsddn_workspace_floats(R, B, C1 - 1)), 1),), float("nan"), device=DEV)
    dl = torch.full((R, ld), float("nan"), dtype=x.dtype, device=DEV) if want_grad else None
    dp = torch.full((R, ld), float("nan"), dtype=x.dtype, device=DEV) if want_grad else None
    L.check(lib.dgx_wsddn_loss(L.ptr(x), ld, L.ptr(q), ld, L.ptr(valid), L.ptr(boxes), B, row0, ih, iw, L.ptr(off), L.ptr(lab), C1 - 1,
                               float(weight), L.ptr(stats_in), L.ptr(upstream), L.ptr(sel) if fwd else None, L.ptr(out) if fwd else None,
                               L.ptr(dl), ld, L.ptr(dp), ld, L.ptr(ws) if fwd else None, L.dtype_code(x), L.stream()), "dgx_wsddn_loss")
    torch.cuda.synchronize()
    return out, sel, dl, dp, ws


def padded(a, ld, dtype):
    """(R, C1) float32 numpy -> (R, ld) device tensor of `dtype`, pad columns NaN; and the values as stored, in float64."""
    R, C1 = a.shape
    t = torch.full((R, ld), float("nan"), dtype=dtype)
    t[:, :C1] = T(a).to(dtype)
    return t.to(DEV), t[:, :C1].double().numpy()


def check_grad(d, ref, floor, C1, dtype, valid, what):
    d = d.float().cpu().numpy().astype(np.float64)
    assert np.all(d[:, C1:] == 0), what + ": pad columns"
    if valid is not None:
        assert np.all(d[~np.asarray(valid).astype(bool)] == 0), what + ": invalid rows"
    tol = RTOL * np.maximum(np.abs(ref), floor) + (2.0 ** -8 * np.abs(ref) if dtype == BF16 else 0.0)
    err = np.abs(d[:, :C1] - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    print("%s: worst ratio %.3g" % (what, float(ratio.max())))
    assert np.all(err <= tol), "%s: worst ratio %.3g at %s" % (what, float(ratio.max()), np.unravel_index(int(np.argmax(ratio)), ratio.shape))


_REF = {}


def _reference(C1, dtype, k):
    """The restatement on the stored inputs of case k, computed once per (width, dtype)."""
    key = (C1, dtype, k)
    if key not in _REF:
        counts, sizes, labels, scores, prop, boxes, valid = W.gpu_cases(C1)[k]
        rnd = W.bf16_round if dtype == BF16 else (lambda a: a)
        sc, pr = rnd(scores), rnd(prop)
        r1 = W.wsddn_loss(sc, pr, valid, boxes, counts, sizes, labels, 0.1)
        _REF[key] = (counts, sizes, labels, sc, pr, boxes, valid, r1)
    return _REF[key]


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C1,ld", [(38, 40), (38, 38), (1204, 1208), (1454, 1464)])
def test_wsddn_loss_against_float64(C1, ld, dtype):
    """Both row layouts: arg-max rows equal, loss within 1e-5 relative of float64 on the stored inputs, both gradients within the
    per-element bound, pad columns (NaN on input) and invalid rows exact zeros in NaN-filled buffers, the forward-then-gradient pair
    bit-identical to the single call, two runs bit-identical, an upstream scalar on the device scales both gradients.  (38, 38): rows
    that are not 16-byte aligned in either dtype, all four matrices take the element-wise path."""
    for k in range(2):
        counts, sizes, labels, sc, pr, boxes, valid, ref = _reference(C1, dtype, k)
        x, stored = padded(sc, ld, dtype)
        q, stored_q = padded(pr, ld, dtype)
        assert np.array_equal(stored, sc.astype(np.float64)) and np.array_equal(stored_q, pr.astype(np.float64))
        v = T(valid).to(DEV) if valid is not None else None
        b = T(boxes).to(DEV)
        out, sel, dl, dp, ws = run_kernel(x, q, C1, v, b, counts, sizes, labels, 0.1)
        nl = sum(len(l) for l in labels)
        assert sel[:nl].tolist() == ref["sel"], (sel[:nl].tolist(), ref["sel"])
        o = out.double().cpu().numpy()
        print("case %d loss %.9g float64 %.9g" % (k, o[0], ref["loss"]))
        assert abs(o[0] - ref["loss"]) <= 1e-5 * abs(ref["loss"]) and abs(o[1] - ref["l_image"]) <= 1e-5 * abs(ref["l_image"]), (o[:2], ref["loss"])
        np.testing.assert_allclose(o[2:7], ref["stats"], rtol=1e-5, atol=1e-7)
        assert o[7] == 0
        check_grad(dl, ref["dscores"], ref["floor_s"], C1, dtype, valid, "d scores")
        check_grad(dp, ref["dprop"], ref["floor_p"], C1, dtype, valid, "d proposal scores")
        # two runs; forward launch, then the gradient launch on its column statistics
        out2, sel2, dl2, dp2, _ = run_kernel(x, q, C1, v, b, counts, sizes, labels, 0.1)
        same = lambda a, c: torch.equal(a.view(torch.uint8), c.view(torch.uint8))      # noqa: E731
        assert same(out, out2) and torch.equal(sel, sel2) and same(dl, dl2) and same(dp, dp2)
        out3, sel3, _, _, ws3 = run_kernel(x, q, C1, v, b, counts, sizes, labels, 0.1, want_grad=False)
        assert same(out, out3) and torch.equal(sel, sel3)
        _, _, dl4, dp4, _ = run_kernel(x, q, C1, v, b, counts, sizes, labels, 0.1, stats_in=ws3)
        assert same(dl, dl4) and same(dp, dp4)
        up = torch.tensor([0.37], device=DEV)
        _, _, dl5, dp5, _ = run_kernel(x, q, C1, v, b, counts, sizes, labels, 0.1, upstream=up, stats_in=ws3)
        f = float(np.float32(0.37))
        check_grad(dl5, ref["dscores"] * f, ref["floor_s"] * f, C1, dtype, valid, "d scores, upstream")
        check_grad(dp5, ref["dprop"] * f, ref["floor_p"] * f, C1, dtype, valid, "d proposal scores, upstream")
    assert ref["sel"][6:9] == [-1, -1, -1] and set(ref["sel"][9:12]) == {5}      # (the validity case: no row; the one row left)


def test_wsddn_loss_against_reference(golden):
    """The golden inputs (contiguous 38-column fp32 rows: the element-wise path; validity bytes) through the autograd node against the
    reference's own fp32 outputs: loss and statistics to 1e-5, rows equal, gradients to 1e-5 of max(|value|, floor) both against the
    float64 restatement of these inputs and against the reference's fp32 gradients.  The column that
    is exactly 1.0f: 100 / (C + 1) per label in the loss (checked through the total), gradients exactly zero; the column below 1e-10:
    gradients exactly zero."""
    from divergen_amd.layers.image_label_ops import wsddn_loss
    g, d = golden("wsddn"), W.inputs()
    s = T(d["scores"]).to(DEV).requires_grad_(True)
    q = T(d["prop"]).to(DEV).requires_grad_(True)
    loss, out, sel = wsddn_loss(s, q, T(d["valid"]).to(DEV), T(d["boxes"]).to(DEV), W.COUNTS, W.IMAGE_SIZES, W.LABELS, W.WEIGHT)
    (loss * 1.0).backward()
    assert sel.tolist() == g["wsddn.sel"].tolist()
    o = out.double().cpu().numpy()
    print("image_loss %.9g reference %.9g" % (o[0], float(g["wsddn.loss"])))
    assert abs(o[0] - g["wsddn.loss"]) <= 1e-5 * abs(g["wsddn.loss"]) and abs(o[1] - g["wsddn.l_image"]) <= 1e-5 * abs(g["wsddn.l_image"])
    np.testing.assert_allclose(o[2:7], g["wsddn.stats"], rtol=1e-5, atol=1e-7)
    r = W.wsddn_loss(d["scores"], d["prop"], d["valid"], d["boxes"], W.COUNTS, W.IMAGE_SIZES, W.LABELS, W.WEIGHT)
    assert sel.tolist() == r["sel"] and abs(o[0] - r["loss"]) <= 1e-5 * abs(r["loss"])
    check_grad(s.grad, r["dscores"], r["floor_s"], W.C + 1, torch.float32, d["valid"], "d scores vs float64")
    check_grad(q.grad, r["dprop"], r["floor_p"], W.C + 1, torch.float32, d["valid"], "d proposal scores vs float64")
    check_grad(s.grad, g["wsddn.dscores"].astype(np.float64), r["floor_s"], W.C + 1, torch.float32, d["valid"], "d scores vs reference")
    check_grad(q.grad, g["wsddn.dprop"].astype(np.float64), r["floor_p"], W.C + 1, torch.float32, d["valid"], "d proposal scores vs reference")
    r3 = W.COUNTS[0] + W.COUNTS[1]
    gs, gq = s.grad.cpu().numpy(), q.grad.cpu().numpy()
    assert gs[0, W.COL_ONE] == 0 and gq[0, W.COL_ONE] == 0 and not gs[r3:r3 + 40, W.COL_LOW].any() and not gq[r3:r3 + 40, W.COL_LOW].any()
    assert gs[0].any() and gq[r3:r3 + 40].any()
    # without the saturated logit the loss is lower by (100 - log 2) / (C + 1) / B per label over three labels of three
    plain = d["scores"].copy()
    plain[0, W.COL_ONE] = 0.0
    _, out0, _ = wsddn_loss(T(plain).to(DEV), q.detach(), T(d["valid"]).to(DEV), T(d["boxes"]).to(DEV), W.COUNTS, W.IMAGE_SIZES, W.LABELS, W.WEIGHT)
    want = (100.0 - np.log(2.0)) / (W.C + 1) / len(W.COUNTS)
    assert abs(float(out[1] - out0[1]) - want) <= 1e-5 * want + 1e-6 * float(out[1])


def test_wsddn_loss_degenerate_and_refusals():
    """R <= 0 is safe and gives a zero loss; a broken contract is DGX_ERR_BAD_ARG; CPU tensors are refused."""
    from divergen_amd import _lib as L
    from divergen_amd.layers.image_label_ops import wsddn_loss
    x = torch.zeros(0, 38, device=DEV, requires_grad=True)
    q = torch.zeros(0, 38, device=DEV, requires_grad=True)
    loss, out, sel = wsddn_loss(x, q, None, torch.zeros(0, 4, device=DEV), [0, 0], [(10, 10)] * 2, [[1], []], 0.1)
    loss.backward()
    assert float(loss.detach()) == 0.0 and out.tolist() == [0.0] * 8 and sel.tolist() == [-1]
    lib = L.lib()
    row0 = (ctypes.c_int * 2)(0, 4)
    f1 = (ctypes.c_float * 1)(10.0)
    buf = torch.zeros(4, 40, device=DEV)
    off, o8, s1, ws = _i32([0, 0]), torch.zeros(8, device=DEV), _i32([0]), torch.zeros(256, device=DEV)

    def call(ld=40, ldp=40, B=1, r=row0, C=37, sel=s1, dl=None, dp=None, stats=None, dtype=0):
        return lib.dgx_wsddn_loss(L.ptr(buf), ld, L.ptr(buf), ldp, None, L.ptr(buf), B, r, f1, f1, L.ptr(off), None, C, 0.1, L.ptr(stats), None,
                                  L.ptr(sel), L.ptr(o8), L.ptr(dl), 40, L.ptr(dp), 40, L.ptr(ws), dtype, L.stream())
    assert call() == 0
    assert call(C=40) == -1 and call(ldp=30) == -1      # ld < C + 1
    assert call(sel=None) == -1                         # a forward launch without sel_out
    assert call(B=33) == -1
    assert call(r=(ctypes.c_int * 2)(1, 4)) == -1       # row0[0] != 0
    assert call(dl=buf.clone()) == -1                   # one gradient buffer without the other
    assert call(stats=ws) == -1                         # column statistics without gradient buffers
    assert call(dtype=5) == -1
    torch.cuda.synchronize()
    with pytest.raises(L.DgxError):
        wsddn_loss(torch.zeros(2, 38), torch.zeros(2, 38), None, torch.zeros(2, 4), [2], [(10, 10)], [[1]], 0.1)
    with pytest.raises(L.DgxError, match="one dtype"):
        wsddn_loss(torch.zeros(2, 38, device=DEV), torch.zeros(2, 38, device=DEV, dtype=BF16), None, torch.zeros(2, 4, device=DEV), [2],
                   [(10, 10)], [[1]], 0.1)


# ------------------------------------------------------------------------------------------------ the predictor branch
def test_prop_score_branch_against_reference_forward(golden):
    """forward of the reference with fixed weights on fixed rows (16 features, 37 classes): in training, for the WSDDN reader, three
    outputs within the bound of the bf16 GEMMs (operands rounded to bf16, fp32 accumulation, bf16 result: 3 roundings of 2^-9 per
    product, bounded by 2^-7 sum |x| |w| per layer, the first layer's error carried through the second); two outputs elsewhere."""
    from divergen_amd.modeling import ShapeSpec
    from divergen_amd.modeling.box_regression import Box2BoxTransform
    from divergen_amd.modeling.roi_heads.detic_fast_rcnn import DeticFastRCNNOutputLayers
    g = golden("wsddn")
    pred = DeticFastRCNNOutputLayers(ShapeSpec(channels=16), box2box_transform=Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0)), num_classes=W.C,
                                     cls_agnostic_bbox_reg=True, use_sigmoid_ce=True, image_label_loss="wsddn", add_image_box=True,
                                     with_softmax_prop=True, ws_prop_score=True)
    sd = {k[len("fwd.param."):]: T(g[k]) for k in g.files if k.startswith("fwd.param.")}
    assert set(sd) == set(pred.state_dict()), (sorted(sd), sorted(pred.state_dict()))
    pred.load_state_dict(sd)
    pred = pred.to(DEV).train()
    x = T(g["fwd.x"]).to(DEV)
    assert len(pred(x)) == 2, "nobody reads the proposal scores: not computed"
    y = pred(x, with_prop_scores=True)
    pred.eval()
    assert len(pred(x)) == 2
    assert len(y) == 3 and tuple(y[2].shape) == (11, W.C + 1) and y[2].stride(0) == 40, "the second GEMM's own 40-column buffer"
    full = y[2].detach().as_strided((11, 40), (40, 1))
    assert not full[:, W.C + 1:].any(), "zero pad columns"
    ax = np.abs(g["fwd.x"]).astype(np.float64)
    P = {k: g["fwd.param." + k].astype(np.float64) for k in sd}
    e = 2.0 ** -7
    for name, got, w, b in (("scores", y[0], "cls_score.weight", "cls_score.bias"), ("deltas", y[1], "bbox_pred.weight", "bbox_pred.bias")):
        tol = e * (ax @ np.abs(P[w]).T + np.abs(P[b]))
        assert np.all(np.abs(got.detach().float().cpu().numpy() - g["fwd." + name]) <= tol), name
    eh = e * (ax @ np.abs(P["prop_score.0.weight"]).T + np.abs(P["prop_score.0.bias"]))
    h = np.maximum(g["fwd.x"].astype(np.float64) @ P["prop_score.0.weight"].T + P["prop_score.0.bias"], 0)
    tol = e * ((h + eh) @ np.abs(P["prop_score.2.weight"]).T + np.abs(P["prop_score.2.bias"])) + eh @ np.abs(P["prop_score.2.weight"]).T
    err = np.abs(y[2].detach().float().cpu().numpy() - g["fwd.prop_scores"])
    print("prop_scores: worst error / bound %.3g" % float((err / tol).max()))
    assert np.all(err <= tol)


# ------------------------------------------------------------------------------------------------ the assembled model
FREQ = os.path.join(ROOT, "configs", "metadata", "lvis_v1_train_cat_info.json")
LOSS_KEYS = {"%s_stage%d" % (n, k) for n in ("image_loss", "loss_cls", "loss_box_reg") for k in range(3)} | {
    "loss_mask", "loss_centernet_loc", "loss_centernet_agn_pos", "loss_centernet_agn_neg"}


def _build(tmp, zeroshot):
    from divergen_amd.config import get_cfg
    from divergen_amd.modeling import build_model
    from divergen_amd.modeling.backbone.swintransformer import DropPath
    from divergen_amd.solver import build_optimizer
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "DiverGen_swinL.yaml"))
    opts = ["MODEL.SWIN.SIZE", "T", "WITH_IMAGE_LABELS", True, "MODEL.ROI_BOX_HEAD.WS_PROP_SCORE", True, "MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsddn",
            "MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP", True, "MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX", True, "MODEL.ROI_BOX_HEAD.WS_NUM_PROPS", 32,
            "MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", FREQ]
    if zeroshot:
        npy = os.path.join(str(tmp), "emb.npy")
        np.save(npy, np.random.default_rng(3).standard_normal((37, 512)).astype(np.float32))
        opts += ["MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", True, "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", npy, "MODEL.ROI_HEADS.NUM_CLASSES", 37,
                 "MODEL.ROI_BOX_HEAD.USE_BIAS", -4.6, "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False]
    cfg.merge_from_list(opts)
    torch.manual_seed(42)
    model = build_model(cfg).train()
    for m in model.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    return cfg, model, build_optimizer(cfg, model), int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)


def _finite_nonzero(params):
    gs = [p.grad for p in params]
    return all(g is not None and bool(torch.isfinite(g).all()) for g in gs) and all(bool(g.any()) for g in gs)


def _zero(params):
    return all(p.grad is None or not bool(p.grad.any()) for p in params)


@pytest.mark.parametrize("zeroshot", [False, True], ids=["linear", "zeroshot"])
def test_image_step_and_box_step_of_the_assembled_model(zeroshot, tmp_path):
    """One image-labelled step and one box step of the registry-built Swin-T model at 256 px under 'wsddn': the same loss keys on both,
    image_loss_stage{k} finite and positive (and equal to the restatement on what the stage saw, 1e-5) on the image step and exactly
    zero on the box step; prop_score gradients finite and non-zero after the image step, exactly zero after the box step; the image
    step launches no vendor compute kernel and reads nothing back to the host; one optimizer step runs."""
    from torch.profiler import ProfilerActivity, profile

    from divergen_amd.data import synthetic_batch
    from divergen_amd.engine import total_loss
    from divergen_amd.structures import BitMasks, Boxes, Instances
    from divergen_amd.utils.events import EventStorage
    from test_gpu_model import library_compute_kernels
    cfg, model, opt, C = _build(tmp_path, zeroshot)
    box_batch = synthetic_batch(2, 256, C, device=DEV)
    for d in box_batch:
        d.update(ann_type="box", pos_category_ids=[], dataset_source=0)
    labels = [[3, 11, C - 1, 11], [5]]
    img_batch = []
    for d, ls in zip(synthetic_batch(2, 256, C, device=DEV), labels):
        h, w = d["image"].shape[-2:]
        inst = Instances((h, w), gt_boxes=Boxes(torch.zeros(0, 4, device=DEV)), gt_classes=torch.zeros(0, dtype=torch.int64, device=DEV),
                         gt_masks=BitMasks(torch.zeros(0, h, w, dtype=torch.bool, device=DEV)))
        img_batch.append(dict(d, instances=inst, ann_type="image", pos_category_ids=ls, dataset_source=1))
    seen = []
    rh = model.roi_heads
    rh.__dict__["stage_observer"] = lambda k, d: seen.append((k, {n: (v.detach().clone() if torch.is_tensor(v) else v) for n, v in d.items()}))
    prop_params = [p for k in range(3) for p in rh.box_predictor[k].prop_score.parameters()]
    assert len(prop_params) == 12
    with EventStorage(0):
        opt.zero_grad()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            losses = model(img_batch)
            total_loss(losses).backward()
            torch.cuda.synchronize()
        # no device->host read: the same step again (the first one uploaded the cached window / pooler tables, which synchronizes)
        # under torch's synchronization warnings -- a read-back (.item(), .tolist(), nonzero, a copy to pageable memory) is one
        opt.zero_grad()
        seen.clear()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                losses = model(img_batch)
                total_loss(losses).backward()
                n_step = sum("called a synchronizing" in str(w.message) for w in caught)
                float(losses["image_loss_stage0"].detach())      # (the probe: a read-back IS reported)
                n_probe = sum("called a synchronizing" in str(w.message) for w in caught) - n_step
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert n_probe >= 1, "the synchronization warnings do not report a read-back"
        assert n_step == 0, "synchronizing calls in the image step: %s" % [str(w.message) for w in caught]
        lib = library_compute_kernels(prof)
        assert not lib, "vendor / framework compute kernels in the image step: %s" % lib
        launched = {k.name for ev in prof.events() for k in ev.kernels}
        for must in ("wsddn_stats_kernel", "wsddn_fold_kernel", "wsddn_grad_kernel"):
            assert any(must in n for n in launched), must
        assert set(losses) == LOSS_KEYS, sorted(losses)
        assert len(seen) == 3
        for k, d in seen:
            assert d["counts"] == [33, 33] and d["scores"].shape == (66, C + 1) and d["prop_scores"].shape == (66, C + 1)
            ref = W.wsddn_loss(d["scores"].double().cpu().numpy(), d["prop_scores"].double().cpu().numpy(),
                               None if d["valid"] is None else d["valid"].cpu().numpy(), d["boxes"].cpu().numpy(), d["counts"],
                               d["image_sizes"], labels, 0.1)
            v = losses["image_loss_stage%d" % k].detach()
            got = float(v)
            print("stage %d image_loss %.9g restatement %.9g" % (k, got, ref["loss"]))
            assert bool(torch.isfinite(v)) and got > 0 and abs(got - ref["loss"]) <= 1e-5 * ref["loss"]
        for n, v in losses.items():
            if not n.startswith("image_loss"):
                assert float(v) == 0.0 and bool(torch.isfinite(v)), n
        assert _finite_nonzero(prop_params), "prop_score gradients after the image step"
        for k in range(3):
            assert not _zero(rh.box_predictor[k].cls_score.parameters()), "cls_score %d" % k
            assert not _zero(rh.box_head[k].parameters()), "box head %d" % k
        assert not _zero(model.backbone.parameters())
        before = [p.detach().clone() for p in prop_params]
        opt.step()
        torch.cuda.synchronize()
        assert any(not torch.equal(a, p.detach()) for a, p in zip(before, prop_params)), "the optimizer step moved prop_score"
        # a box step of the same model: same keys, image losses exactly zero, the branch is not evaluated: exactly zero gradients
        seen.clear()
        opt.zero_grad()
        bl = model(box_batch)
        total_loss(bl).backward()
        opt.arena.finish_grads()        # segments no first writer reached are zeroed now (what optimizer.step() does first)
        torch.cuda.synchronize()
        assert set(bl) == LOSS_KEYS
        for k in range(3):
            assert float(bl["image_loss_stage%d" % k].detach()) == 0.0 and float(bl["loss_cls_stage%d" % k].detach()) > 0
        assert all(bool(torch.isfinite(v)) for v in bl.values())
        assert all(p.grad is not None and not bool(p.grad.any()) for p in prop_params), "prop_score gradients after the box step"
        opt.step()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(p).all()) for p in prop_params)


def test_do_train_on_two_sources_with_wsddn(tmp_path, monkeypatch):
    """train_net.do_train for 6 iterations on a generated box source + image-labelled source with the key, IMAGE_LABEL_LOSS 'wsddn' and
    WITH_SOFTMAX_PROP: box and image steps both occur, every logged loss is finite, metrics.json carries the image_loss_* keys and every
    image step's image_loss is finite and positive."""
    import json
    sys.path.insert(0, ROOT)
    import train_net
    from divergen_amd.modeling import build_model
    from divergen_amd.modeling.meta_arch.custom_rcnn import CustomRCNN
    from test_host_image_labels import _two_source_cfg
    cfg, info = _two_source_cfg(tmp_path, monkeypatch, [
        "DATALOADER.NUM_WORKERS", 2, "DATALOADER.USE_DIFF_BS_SIZE", True, "DATALOADER.DATASET_BS", [2, 4], "DATALOADER.DATASET_INPUT_SIZE", [128, 128],
        "DATALOADER.DATASET_INPUT_SCALE", [[0.3, 1.2], [0.8, 1.2]], "SOLVER.MAX_ITER", 6, "SOLVER.CHECKPOINT_PERIOD", 100, "SOLVER.WARMUP_ITERS", 2,
        "SEED", 7, "MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX", True, "MODEL.ROI_BOX_HEAD.WS_PROP_SCORE", True, "MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsddn",
        "MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP", True])
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    kinds = []
    orig = CustomRCNN._annotation_type

    def spy(self, batched_inputs, gt):
        kinds.append(orig(self, batched_inputs, gt))
        return kinds[-1]
    monkeypatch.setattr(CustomRCNN, "_annotation_type", spy)
    from divergen_amd.modeling.roi_heads.detic_fast_rcnn import DeticFastRCNNOutputLayers
    image_losses, plain = [], DeticFastRCNNOutputLayers.image_label_losses

    def recorded(self, *a, **k):
        out = plain(self, *a, **k)
        image_losses.append(out["image_loss"].detach())
        return out
    monkeypatch.setattr(DeticFastRCNNOutputLayers, "image_label_losses", recorded)
    torch.manual_seed(7)
    model = build_model(cfg)
    assert any("prop_score.2.weight" in n for n, _ in model.named_parameters())
    train_net.do_train(cfg, model)
    assert len(kinds) == 6 and set(kinds) == {"box", "image"}, kinds
    rows = [json.loads(line) for line in open(os.path.join(str(tmp_path / "out"), "metrics.json"))]
    assert all(np.isfinite(r["total_loss"]) for r in rows if "total_loss" in r)
    assert {"image_loss_stage0", "image_loss_stage1", "image_loss_stage2", "total_loss"} <= set().union(*[set(r) for r in rows])
    vals = torch.stack(image_losses).tolist()
    assert len(vals) == 3 * kinds.count("image") and all(np.isfinite(v) and v > 0 for v in vals), vals
