"""GPU tests of the open-vocabulary box predictor (MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS): the row L2-normalisation kernel against
float64, the classifier and the whole output layer against the reference's outputs (tests/golden/zeroshot.npz) and the bf16-storage
restatement (tests/_zeroshot_ref.py), one training step of the assembled model and evaluation on a swapped vocabulary."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _zeroshot_ref as Z  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
EPS = 1e-12


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------ the kernel
def _rows(R, D, dtype, kind, seed):
    """(R, D) test rows as stored in `dtype`.  kind 'mixed': row 0 all zero, row 1 below the clamp (entries 1e-15), the rest
    ordinary with norms over three decades; a single row is of the kind named."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, D, generator=g) * torch.logspace(-1.5, 1.5, R)[torch.randperm(R, generator=g)][:, None]
    if kind == "zero" or (kind == "mixed" and R >= 3):
        x[0] = 0
    if kind == "tiny":
        x[0] = 1e-15
    if kind == "mixed" and R >= 3:
        x[1] = 1e-15 * torch.sign(torch.randn(D, generator=g))
    return x.to(dtype)


CASES = [(R, "mixed") for R in (5, 257)] + [(1, k) for k in ("zero", "tiny", "ordinary")]


def _fwd64(x, t):
    x64 = x.double()
    n = x64.pow(2).sum(1).sqrt()
    rn = 1.0 / n.clamp(min=EPS)
    return t * x64 * rn[:, None], rn, n


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("D", [8, 72, 512, 1024])
def test_l2norm_forward_against_float64(D, dtype):
    """y within one bf16 rounding (2^-8 relative) of the float64 value of the same stored inputs, rnorm within 1e-6; all-zero rows
    give y = 0 and rnorm = 1e12; R = 1, 5, 257: a partial workgroup, more than one workgroup; D = 8, 72: a partial wave, 512 and 1024:
    one and two loads per lane."""
    from divergen_amd import _lib as L
    for R, kind in CASES:
        for t in (1.0, 50.0):
            x = _rows(R, D, dtype, kind, 7 * R + D)
            xd = x.to(DEV)
            y = torch.full((R, D), float("nan"), dtype=BF16, device=DEV)
            rn = torch.full((R,), float("nan"), dtype=torch.float32, device=DEV)
            L.check(L.lib().dgx_l2norm_rows_fwd(L.ptr(xd), L.ptr(y), L.ptr(rn), R, D, t, L.dtype_code(xd), L.stream()), "fwd")
            y64, rn64, n64 = _fwd64(x, t)
            y, rn = y.cpu().double(), rn.cpu().double()
            err = (y - y64).abs() - 2.0 ** -8 * y64.abs()
            print("fwd D %d %s R %d %s t %g: worst y excess %.3e, rnorm rel %.3e" % (D, dtype, R, kind, t, float(err.max()),
                                                                                  float(((rn - rn64).abs() / rn64).max())))
            assert bool((err <= 0).all()), (R, kind, t)
            assert bool(((rn - rn64).abs() <= 1e-6 * rn64).all()), (R, kind, t)
            zero = n64 == 0
            assert bool((y[zero] == 0).all()) and bool(((rn[zero] - 1e12).abs() <= 1e6).all())
            if kind != "ordinary":
                nclamp = 2 if kind == "mixed" else 1
                assert bool((n64[:nclamp] <= EPS).all()) and bool((n64[nclamp:] > 1e-3).all())       # the rows meant to sit at the clamp do


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("D", [8, 72, 512, 1024])
def test_l2norm_backward_against_float64(D, dtype):
    """dx = t*rnorm*(g - xh*(xh.g)) against float64 from the same stored inputs, elementwise within
    2^-8*t*rnorm*(|g_i| + |xh_i|*|xh.g|) + 1e-6*t*rnorm*max|g| (the two subtracted terms bound the rounding of their difference);
    rows at the clamp against t*1e12*g within one bf16 rounding."""
    from divergen_amd import _lib as L
    for R, kind in CASES:
        for t in (1.0, 50.0):
            x = _rows(R, D, dtype, kind, 11 * R + D)
            g = torch.randn(R, D, generator=torch.Generator().manual_seed(R + D)).to(BF16)
            xd, gd = x.to(DEV), g.to(DEV)
            _, rn64, n64 = _fwd64(x, t)
            rn = rn64.float().to(DEV)           # the saved rnorm, as the forward stores it (fp32)
            y = torch.empty(R, D, dtype=BF16, device=DEV)
            L.check(L.lib().dgx_l2norm_rows_fwd(L.ptr(xd), L.ptr(y), L.ptr(rn), R, D, t, L.dtype_code(xd), L.stream()), "fwd")
            dx = torch.full((R, D), float("nan"), dtype=BF16, device=DEV)
            L.check(L.lib().dgx_l2norm_rows_bwd(L.ptr(gd), L.ptr(xd), L.ptr(rn), L.ptr(dx), R, D, t, L.dtype_code(xd), L.stream()), "bwd")
            dx = dx.cpu().double()
            g64, xh = g.double(), x.double() * rn64[:, None]
            dot = (xh * g64).sum(1, keepdim=True)
            scale = (t * rn64)[:, None]
            want = scale * (g64 - xh * dot)
            bound = 2.0 ** -8 * scale * (g64.abs() + xh.abs() * dot.abs()) + 1e-6 * scale * g64.abs().max(1, keepdim=True)[0]
            clamp = n64 <= EPS
            want[clamp] = t * 1e12 * g64[clamp]
            bound[clamp] = 2.0 ** -8 * t * 1e12 * g64[clamp].abs()
            print("bwd D %d %s R %d %s t %g: worst excess over the bound %.3e (bound there %.3e)"
                  % (D, dtype, R, kind, t, float(((dx - want).abs() - bound).max()), float(bound.flatten()[((dx - want).abs() - bound).argmax()])))
            assert bool(((dx - want).abs() <= bound).all()), (R, kind, t)


def test_l2norm_contract_is_refused_by_return_code_and_zero_rows_are_safe():
    from divergen_amd import _lib as L
    from divergen_amd.layers.norm_ops import l2_normalize_rows
    lib = L.lib()
    x = torch.randn(4, 4104, device=DEV)
    y = torch.full((4, 4104), 7.0, dtype=BF16, device=DEV)
    rn = torch.full((4,), 7.0, device=DEV)
    g = torch.ones(4, 4104, dtype=BF16, device=DEV)
    for D in (0, 4, 12, 4100, 4104):
        assert lib.dgx_l2norm_rows_fwd(L.ptr(x), L.ptr(y), L.ptr(rn), 4, D, 1.0, L.DGX_F32, L.stream()) == -2
        assert lib.dgx_l2norm_rows_bwd(L.ptr(g), L.ptr(x), L.ptr(rn), L.ptr(y), 4, D, 1.0, L.DGX_F32, L.stream()) == -2
    assert lib.dgx_l2norm_rows_fwd(L.ptr(x), L.ptr(y), L.ptr(rn), 4, 512, 1.0, 5, L.stream()) == -2
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and bool((rn == 7).all())               # nothing was launched
    assert lib.dgx_l2norm_rows_fwd(None, None, None, 0, 512, 1.0, L.DGX_F32, L.stream()) == 0
    assert lib.dgx_l2norm_rows_bwd(None, None, None, None, 0, 512, 1.0, L.DGX_F32, L.stream()) == 0
    e = torch.empty(0, 512, device=DEV, requires_grad=True)
    out = l2_normalize_rows(e, 50.0)
    out.sum().backward()
    assert out.shape == (0, 512) and out.dtype == BF16 and e.grad.shape == (0, 512)
    with pytest.raises(L.DgxError):
        l2_normalize_rows(torch.randn(3, 12, device=DEV), 1.0)
    # the autograd node: fp32 rows (a vocabulary) and bf16 rows against torch's own double-precision gradient
    for dtype in (torch.float32, BF16):
        a = (torch.randn(9, 72, generator=torch.Generator().manual_seed(1)).to(dtype)).to(DEV).requires_grad_(True)
        w = torch.randn(9, 72, generator=torch.Generator().manual_seed(2)).to(BF16).to(DEV)
        (l2_normalize_rows(a, 50.0).float() * w.float()).sum().backward()
        a64 = a.detach().double().cpu().requires_grad_(True)
        (50.0 * torch.nn.functional.normalize(a64, dim=1) * w.double().cpu()).sum().backward()
        assert a.grad.dtype == dtype and rel(a.grad, a64.grad) <= 2.0 ** -8


# ------------------------------------------------------------------------------------------------ the module
@pytest.fixture(scope="module")
def gold(golden):
    return golden("zeroshot")


@pytest.fixture(scope="module")
def data():
    return Z.inputs()


def _predictor(tmp, d, in_features=Z.IN):
    from divergen_amd.modeling import ShapeSpec
    from divergen_amd.modeling.box_regression import Box2BoxTransform
    from divergen_amd.modeling.roi_heads.detic_fast_rcnn import DeticFastRCNNOutputLayers
    from divergen_amd.modeling.roi_heads.zero_shot_classifier import ZeroShotClassifier
    npy = os.path.join(str(tmp), "emb.npy")
    np.save(npy, d["emb"].numpy())
    cls = ZeroShotClassifier(ShapeSpec(channels=in_features), num_classes=Z.C, zs_weight_path=npy, zs_weight_dim=Z.D, use_bias=Z.USE_BIAS,
                             norm_weight=True, norm_temperature=Z.TEMP)
    return DeticFastRCNNOutputLayers(ShapeSpec(channels=in_features), box2box_transform=Box2BoxTransform(weights=Z.BOX_WEIGHTS),
                                     num_classes=Z.C, cls_agnostic_bbox_reg=True, smooth_l1_beta=0.0, use_sigmoid_ce=True,
                                     use_fed_loss=False, use_zeroshot_cls=True, cls_score=cls)


@pytest.fixture(scope="module")
def pred(data, tmp_path_factory):
    p = _predictor(tmp_path_factory.mktemp("zs"), data)
    sd = p.state_dict()
    for k in Z.PARAMS:
        sd[k if k.startswith("bbox_pred") else "cls_score." + k] = data[k].clone()
    p.load_state_dict(sd, strict=True)
    return p.to(DEV)


def logit_bound(stored):
    """One bf16 step of the stored (pre-bias) logit: 2^-7 * max(|logit|, 1)."""
    return 2.0 ** -7 * stored.abs().clamp(min=1.0)


def test_classifier_logits_builtin_and_per_call_vocabulary(gold, data, pred):
    x = data["x"].to(DEV)
    nobias = dict(data, cls_bias=torch.zeros(1))
    with torch.no_grad():
        got = pred.cls_score(x).cpu()
        got_call = pred.cls_score(x, classifier=data["emb2"].to(DEV)).cpu()
    assert got.dtype == torch.float32 and got.shape == (Z.R, Z.C + 1) and got_call.shape == (Z.R, Z.C2)
    for name, g, kw in (("built-in", got, dict(zs_weight=Z.zs_weight_of(data["emb"]))), ("per-call", got_call, dict(classifier=data["emb2"]))):
        stored = Z.classifier_logits(data["x"], nobias, bf16=True, **kw)
        want = stored + data["cls_bias"]
        print("%s vocabulary: worst |logit error| / bound %.3f" % (name, float(((g - want).abs() / logit_bound(stored)).max())))
        assert bool(((g - want).abs() <= logit_bound(stored)).all()), name
    # the background column of the built-in vocabulary is the zero embedding: the bias alone
    assert bool((got[:, -1] == data["cls_bias"]).all())
    assert rel(got, T(gold["logits"])) < 2e-2 and rel(got_call, T(gold["logits_call"])) < 2e-2


def test_rows_equal_to_a_class_embedding_give_the_extreme_logits(data, tmp_path):
    """A feature row equal to +- a class embedding (identity projection): logit +-50 + bias on that class; the loss of such rows is
    finite and the restatement's, within the logit bound carried through the loss to second order."""
    from divergen_amd.utils.events import EventStorage
    p = _predictor(tmp_path, data, in_features=Z.D)
    with torch.no_grad():
        p.cls_score.linear.weight.copy_(torch.eye(Z.D))
        p.cls_score.linear.bias.zero_()
    p = p.to(DEV)
    e = data["emb"].to(BF16).float()
    x = torch.cat([e[3:4], -e[3:4], e[11:12] * 4, data["emb2"].to(BF16).float()[:5]])
    R = x.shape[0]
    gt = torch.tensor([3, 3, 11, Z.C, 0, 5, Z.C, 20])
    prm = {"linear.weight": torch.eye(Z.D), "linear.bias": torch.zeros(Z.D), "cls_bias": torch.zeros(1)}
    stored = Z.classifier_logits(x, prm, zs_weight=Z.zs_weight_of(data["emb"]), bf16=True)
    want = stored + data["cls_bias"]
    xd = x.to(DEV).requires_grad_(True)
    scores, deltas = p(xd)
    got = scores.detach().cpu()
    assert bool(((got - want).abs() <= logit_bound(stored)).all())
    for r, s in ((0, 1.0), (1, -1.0), (2, 1.0)):
        c = int(gt[r])
        assert abs(float(got[r, c]) - (s * 50.0 + Z.USE_BIAS)) <= 2.0 ** -7 * 50.0, (r, float(got[r, c]))
    prop = data["prop_boxes"][:R].to(DEV)
    with EventStorage(0):
        losses = p.losses_from_tensors(scores, deltas, gt.to(DEV), prop, prop.clone(), None)
    want_loss, _ = Z.losses(want, torch.zeros(R, 4), gt, data["prop_boxes"][:R], data["prop_boxes"][:R])
    # |loss(l + d) - loss(l)| <= sum(|sigmoid(l) - target| * |d| + d^2 / 8) / B: the BCE's first derivative at the restatement's logits
    # and the bound 1/4 on its second
    b = logit_bound(stored)[:, :-1]
    target = torch.nn.functional.one_hot(gt, Z.C + 1)[:, :Z.C].float()
    slack = float(((torch.sigmoid(want[:, :-1]) - target).abs() * b + b * b / 8).sum()) / R
    print("extreme rows: loss_cls %.6f, restatement %.6f, bound on the difference %.3e" % (float(losses["loss_cls"].detach()), float(want_loss), slack))
    assert bool(torch.isfinite(losses["loss_cls"])) and abs(float(losses["loss_cls"].detach()) - float(want_loss)) <= slack + 1e-5 * float(want_loss)
    losses["loss_cls"].backward()
    assert bool(torch.isfinite(xd.grad).all()) and bool(torch.isfinite(p.cls_score.cls_bias.grad).all())


def test_output_layer_losses_and_gradients_against_the_reference(gold, data, pred):
    """losses_from_tensors on the GPU: loss_cls / loss_box_reg within 1e-3 relative of the reference's, every gradient within 2 %
    relative L2 (the project's per-tensor bar, tests/test_gpu_model.py)."""
    from divergen_amd.utils.events import EventStorage
    for q in pred.parameters():
        q.grad = None
    x = data["x"].to(DEV).requires_grad_(True)
    scores, deltas = pred(x)
    assert rel(deltas, T(gold["deltas"])) < 2e-2
    with EventStorage(0):
        losses = pred.losses_from_tensors(scores, deltas, data["gt_classes"].to(DEV), data["prop_boxes"].to(DEV), data["gt_boxes"].to(DEV), None)
    for k in ("loss_cls", "loss_box_reg"):
        e = abs(float(losses[k]) - float(gold[k])) / abs(float(gold[k]))
        print("%s %.6f against %.6f: relative %.3e" % (k, float(losses[k]), float(gold[k]), e))
        assert e <= 1e-3, k
    (losses["loss_cls"] + losses["loss_box_reg"]).backward()
    named = dict(pred.named_parameters())
    got = {"x": x.grad}
    for k in Z.PARAMS:
        g = named[k if k.startswith("bbox_pred") else "cls_score." + k].grad
        got[k] = g[Z.GRAD_ROWS] if k in ("linear.weight", "bbox_pred.0.weight") else g
    for k, g in got.items():
        e = rel(g, T(gold["g." + k]))
        print("gradient %s: relative L2 %.3e" % (k, e))
        assert e <= 2e-2, k
    assert pred.cls_score.zs_weight.grad is None


# ------------------------------------------------------------------------------------------------ the assembled model
def _build(tmp, data):
    from divergen_amd.config import get_cfg
    from divergen_amd.modeling import build_model
    from divergen_amd.modeling.backbone.swintransformer import DropPath
    from divergen_amd.solver import build_optimizer
    npy = os.path.join(str(tmp), "emb.npy")
    np.save(npy, data["emb"].numpy())
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "DiverGen_swinL.yaml"))
    cfg.merge_from_list(["MODEL.SWIN.SIZE", "T", "MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", True, "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", npy,
                         "MODEL.ROI_HEADS.NUM_CLASSES", Z.C, "MODEL.ROI_BOX_HEAD.USE_BIAS", Z.USE_BIAS,
                         "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 1e-4])
    torch.manual_seed(42)
    model = build_model(cfg).train()
    for m in model.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    return cfg, model, build_optimizer(cfg, model)


def test_one_training_step_of_the_assembled_model(data, tmp_path):
    from torch.profiler import ProfilerActivity, profile
    from divergen_amd.data import synthetic_batch
    from divergen_amd.modeling.roi_heads.zero_shot_classifier import ZeroShotClassifier
    from divergen_amd.utils.events import EventStorage
    from test_gpu_model import library_compute_kernels
    cfg, model, opt = _build(tmp_path, data)
    p0 = model.roi_heads.box_predictor[0]
    assert isinstance(p0.cls_score, ZeroShotClassifier) and p0.cls_score.zs_weight.is_cuda
    watch = {"cls_bias": p0.cls_score.cls_bias, "linear.weight": p0.cls_score.linear.weight, "bbox_pred.0.weight": p0.bbox_pred[0].weight}
    before = {k: v.detach().clone() for k, v in watch.items()}
    zs_before = p0.cls_score.zs_weight.clone()
    batch = synthetic_batch(2, 256, Z.C, device=DEV)
    with EventStorage(0):
        opt.zero_grad()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            losses = model(batch)
            sum(losses.values()).backward()
            opt.step()
            torch.cuda.synchronize()
    assert set(losses) == {"loss_cls_stage0", "loss_box_reg_stage0", "loss_cls_stage1", "loss_box_reg_stage1", "loss_cls_stage2",
                           "loss_box_reg_stage2", "loss_mask", "loss_centernet_loc", "loss_centernet_agn_pos", "loss_centernet_agn_neg"}
    assert all(bool(torch.isfinite(v)) for v in losses.values()), losses
    for k, v in watch.items():
        assert not torch.equal(v.detach(), before[k]), "%s did not move" % k
    assert torch.equal(p0.cls_score.zs_weight, zs_before)
    lib = library_compute_kernels(prof)
    assert not lib, "vendor / framework compute kernels on the open-vocabulary path: %s" % lib
    launched = {k.name for ev in prof.events() for k in ev.kernels}
    for must in ("l2n_fwd_kernel", "l2n_bwd_kernel", "detic_"):
        assert any(must in n for n in launched), "expected libdgx kernel not launched: %s" % must


def test_evaluation_with_a_swapped_vocabulary(data, tmp_path, monkeypatch):
    """reset_cls_test to 7 classes, inference on one image: classes < 7; every stage's logits within the logit bound of the bf16-storage
    restatement on the stage's own input rows, and the final scores inside the envelope that bound gives when pushed through the
    sigmoid, the stage mean and the proposal-score product (all monotone); back to 37 classes: the first run's detections bit for bit."""
    from divergen_amd.data import synthetic_batch
    from divergen_amd.modeling.roi_heads import detic_roi_heads as RH
    from divergen_amd.modeling.utils import reset_cls_test
    cfg, model, _ = _build(tmp_path, data)
    model.eval()
    npy2 = os.path.join(str(tmp_path), "emb2.npy")
    np.save(npy2, data["emb2"].numpy())
    image = synthetic_batch(1, 256, Z.C, device=DEV)[:1]
    seen = {"stage": [], "final": None, "ps": None}
    for k, bp in enumerate(model.roi_heads.box_predictor):
        bp.register_forward_hook(lambda m, a, out, k=k: seen["stage"].append((k, a[0].detach().float().cpu(), out[0].detach().float().cpu())))
    orig_inf, orig_box = RH.fast_rcnn_inference, model.roi_heads._forward_box

    def spy_inference(boxes, scores, *a, **kw):
        inst, kept = orig_inf(boxes, scores, *a, **kw)
        seen["final"] = (scores[0].detach().cpu(), kept[0].cpu())
        return inst, kept

    def spy_box(features, proposals, *a, **kw):
        p = proposals[0]
        seen["ps"] = (p.get("scores") if p.has("scores") else p.get("objectness_logits")).detach().float().cpu()
        return orig_box(features, proposals, *a, **kw)
    monkeypatch.setattr(RH, "fast_rcnn_inference", spy_inference)
    monkeypatch.setattr(model.roi_heads, "_forward_box", spy_box)

    def run():
        seen["stage"] = []
        r = model.inference(image, do_postprocess=False)[0]
        torch.cuda.synchronize()
        return r

    def same(a, b):
        fa, fb = a.get_fields(), b.get_fields()
        return set(fa) == set(fb) and all(torch.equal(getattr(fa[k], "tensor", fa[k]), getattr(fb[k], "tensor", fb[k])) for k in fa)
    first = run()
    assert len(first) > 0 and int(first.pred_classes.max()) < Z.C
    zs = reset_cls_test(model, npy2, Z.C2)
    assert model.roi_heads.num_classes == Z.C2 and all(bp.cls_score.zs_weight is zs for bp in model.roi_heads.box_predictor)
    res = run()
    assert len(res) > 0 and int(res.pred_classes.max()) < Z.C2 and int(res.pred_classes.min()) >= 0
    assert res.pred_masks.shape[0] == len(res)
    # per stage: logits against the restatement on the rows this stage saw
    lo = hi = 0
    assert [k for k, _, _ in seen["stage"]] == [0, 1, 2]
    zs_cpu = zs.cpu()
    for k, xk, got in seen["stage"]:
        c = model.roi_heads.box_predictor[k].cls_score
        prm = {"linear.weight": c.linear.weight.detach().to(BF16).float().cpu(), "linear.bias": c.linear.bias.detach().to(BF16).float().cpu(),
               "cls_bias": torch.zeros(1)}
        stored = Z.classifier_logits(xk, prm, zs_weight=zs_cpu, bf16=True)
        bias = c.cls_bias.detach().float().cpu()
        b = logit_bound(stored)
        print("stage %d: %d rows, worst |logit error| / bound %.3f" % (k, xk.shape[0], float(((got - (stored + bias)).abs() / b).max())))
        assert got.shape == (xk.shape[0], Z.C2 + 1) and bool(((got - (stored + bias)).abs() <= b).all()), k
        lo, hi = lo + torch.sigmoid(stored + bias - b), hi + torch.sigmoid(stored + bias + b)
    lo, hi = lo / 3, hi / 3
    if cfg.MODEL.ROI_BOX_HEAD.MULT_PROPOSAL_SCORE:
        lo, hi = (lo * seen["ps"][:, None]) ** 0.5, (hi * seen["ps"][:, None]) ** 0.5
    final, kept = seen["final"]
    assert bool((final >= lo * (1 - 1e-5) - 1e-7).all()) and bool((final <= hi * (1 + 1e-5) + 1e-7).all())
    assert torch.equal(res.scores.cpu(), final[kept, res.pred_classes.cpu()])
    # back to the first vocabulary (a (D, C) tensor this time)
    reset_cls_test(model, data["emb"].permute(1, 0).contiguous(), Z.C)
    again = run()
    assert model.roi_heads.num_classes == Z.C and len(again) == len(first) and same(first, again)
