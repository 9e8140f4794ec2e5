"""GPU tests of the dynamic classifier (MODEL.DYNAMIC_CLASSIFIER behind MODEL.DYNAMIC_VOCAB; csrc/dyn_vocab.hip):
dgx_dyn_class_sample, dgx_zs_gather and dgx_remap_labels against the float64 restatement (tests/_dyncls_ref.py), the predictor on the
reference's golden (tests/golden/dynamic_classifier.npz), one box step and one image step of the assembled model."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _dyncls_ref as Z  # noqa: E402
import _zeroshot_ref as ZR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def _expo(C, seed):
    return torch.empty(C + 1).exponential_(1, generator=torch.Generator().manual_seed(seed))


def _weights(C, seed, keep=None):
    rs = np.random.RandomState(seed)
    w = (rs.randint(1, 500, C).astype(np.float32)) ** 0.5
    w[rs.rand(C) < 1.0 / 7] = 0.0                       # a seventh of the weights zero
    if keep is not None:                                # only `keep` positive-weight classes left
        w[:] = 0.0
        w[rs.permutation(C)[:keep]] = 3.0
    return np.concatenate([w, [0.0]]).astype(np.float32)


def _labels(C, distinct, seed, dup=True):
    rs = np.random.RandomState(seed)
    cls = rs.permutation(C)[:distinct]
    lab = np.concatenate([cls, cls[rs.randint(0, max(distinct, 1), 2 * distinct)]]) if (dup and distinct) else cls
    return rs.permutation(lab).astype(np.int64)


#            C,     num_classes, S, distinct, only this many positive weights
SAMPLER = [(37, 37, 8, 0, None), (30, 37, 8, 3, None), (37, 37, 4, 4, None), (37, 37, 4, 11, None), (37, 37, 8, 2, 3),
           (1203, 1453, 50, 5, None), (22047, 22047, 50, 7, None)]


@pytest.mark.parametrize("C,NC,S,distinct,keep", SAMPLER, ids=["C%d-S%d-a%d%s" % (c[0], c[2], c[3], "-few" if c[4] else "") for c in SAMPLER])
def test_sampler_against_the_restatement(C, NC, S, distinct, keep):
    from divergen_amd.layers.dyn_vocab_ops import sample_classes
    prob0 = _weights(C, C + S, keep)
    lab = _labels(C, distinct, C + 1)
    if keep is not None:        # the labels sit on zero-weight classes: a + #positive < S
        lab = np.nonzero(prob0[:C] == 0)[0][:distinct].astype(np.int64).repeat(2)
    expo = _expo(C, 100 + C)
    want_inds, want_map, n = Z.sample(lab, prob0, expo.numpy(), C, NC, S)
    runs = []
    for _ in range(2):
        inds, cmap, nd = sample_classes(torch.from_numpy(lab).to(DEV), torch.from_numpy(prob0).to(DEV), expo.to(DEV), C, NC, S)
        runs.append((inds.cpu(), cmap.cpu(), int(nd.cpu())))
    inds, cmap, got_n = runs[0]
    print("C %d S %d: a %d, n %d (restatement %d)" % (C, S, len(np.unique(lab)), got_n, n))
    assert got_n == n and inds[:n].tolist() == want_inds.tolist() and cmap.tolist() == want_map.tolist()
    assert runs[1][2] == n and torch.equal(runs[0][0][:n], runs[1][0][:n]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    a = len(np.unique(lab))
    if keep is not None:
        assert n == a + keep < S
    elif a >= S:
        assert n == a
    else:
        assert n == S


def test_sampler_limits_are_refused_by_return_code():
    from divergen_amd import _lib as L
    z = torch.zeros(4, device=DEV)
    i = torch.zeros(64, dtype=torch.int64, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = L.lib()
    assert lib.dgx_dyn_class_sample(None, 0, L.ptr(z), L.ptr(z), 32768, 32768, 8, L.ptr(i), L.ptr(i), L.ptr(n), L.stream()) == -2
    assert lib.dgx_dyn_class_sample(None, 0, L.ptr(z), L.ptr(z), 30000, 30000, 30000, L.ptr(i), L.ptr(i), L.ptr(n), L.stream()) == -2
    assert lib.dgx_dyn_class_sample(None, 0, L.ptr(z), L.ptr(z), 3, 2, 8, L.ptr(i), L.ptr(i), L.ptr(n), L.stream()) == -1
    assert lib.dgx_dyn_class_sample(None, 5, L.ptr(z), L.ptr(z), 3, 3, 8, L.ptr(i), L.ptr(i), L.ptr(n), L.stream()) == -1


@pytest.mark.parametrize("name,case,S,C", [("few", 0, 8, Z.C_FREQ), ("many", 1, 4, Z.C_FREQ), ("image", 2, Z.IMAGE_S, Z.NUM_CLASSES)])
def test_sampler_on_the_golden_seed(name, case, S, C, golden):
    """The golden's seed through a CPU exponential_ (torch's generator at the sampler's position): the reference's inds, in its order."""
    from divergen_amd.layers.dyn_vocab_ops import sample_classes, sampling_weights
    g = golden("dynamic_classifier")
    torch.manual_seed(int(g["seed"]) + case)
    expo = torch.empty(C + 1).exponential_(1)
    if name == "image":
        lab, w = torch.tensor([c for ls in Z.IMAGE_LABELS for c in ls]), None
    else:
        gt = torch.from_numpy(g["in." + name + ".gt_classes"])
        lab, w = gt[gt < Z.NUM_CLASSES], torch.from_numpy(g["in.freq_weight"])
    inds, cmap, n = sample_classes(lab.to(DEV), sampling_weights(w, C, torch.device(DEV, 0)), expo.to(DEV), C, Z.NUM_CLASSES, S)
    n = int(n.cpu())
    assert inds[:n].cpu().tolist() == g[name + ".inds"].tolist() and cmap.cpu().tolist() == g[name + ".cls_id_map"].tolist()


def _bf16_ulp(v):
    """One unit in the last place of bfloat16 at |v| (8 significand bits), for float64 v."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - 7)


@pytest.mark.parametrize("D", [64, 512])
@pytest.mark.parametrize("n1", [8, 9, 51])
def test_gather_against_float64(n1, D):
    from divergen_amd.layers.dyn_vocab_ops import zs_gather
    from divergen_amd.layers.linear_ops import pad8
    C, n = 203, n1 - 1
    rs = np.random.RandomState(n1 * 1000 + D)
    zs = ZR.zs_weight_of(torch.from_numpy(rs.standard_normal((C, D)).astype(np.float32) * 0.3))      # (D, C + 1), unit columns
    inds = np.concatenate([[0, C - 1], 1 + rs.permutation(C - 2)[:n - 2]]).astype(np.int64)
    inds = inds[rs.permutation(n)]
    source, zs64 = zs.contiguous().to(DEV), zs.double().numpy()
    W, Wt = zs_gather(source, torch.from_numpy(inds).to(DEV), n, D, C, True)
    npad = pad8(n1)
    assert W.shape == (npad, D) and Wt.shape == (D, npad) and W.dtype == BF16 and Wt.dtype == BF16
    W, Wt = W.cpu(), Wt.cpu()
    assert torch.equal(Wt, W.t().contiguous()), "Wt is not W transposed"
    assert not bool(W[n:].any()), "background / pad rows are not exact zeros"
    want = Z.sub_vocab(zs64, inds)[:, :n].T                                     # float64 (n, D)
    r = torch.from_numpy(want).to(torch.float32).to(BF16).double().numpy()       # its bf16 rounding
    err = np.abs(W[:n].double().numpy() - r) / _bf16_ulp(r)
    print("n+1 %d D %d: worst error %.3f bf16 ulp of the rounded float64 value, %d of %d elements differ" % (
        n1, D, err.max(), int((err > 0).sum()), err.size))
    assert err.max() <= 1.0


@pytest.mark.parametrize("R,D,n1", [(5, 64, 9), (70, 512, 51), (33, 200, 70)])
def test_fp32_logits_against_float64(R, D, n1):
    """dgx_zs_logits_f32 on bf16 operands: |y - float64| <= D * 2^-23 * sum_k |x_k w_k| (fp32 products are exact to 2^-24 relative, D
    sequential fp32 additions); rows and columns outside the tiles (R, n1 no multiples of 16 / 64; D none of 128) are covered."""
    from divergen_amd import _lib as L
    from divergen_amd.layers.linear_ops import pad8
    rs = np.random.RandomState(R + D + n1)
    npad = pad8(n1)
    x = torch.from_numpy(rs.standard_normal((R, D)).astype(np.float32) * 3).to(BF16)
    W = torch.from_numpy(rs.standard_normal((npad, D)).astype(np.float32) * 0.2).to(BF16)
    y = torch.full((R, n1 + 3), 7.0, dtype=torch.float32, device=DEV)
    xd, Wd = x.to(DEV), W.to(DEV)
    L.check(L.lib().dgx_zs_logits_f32(L.ptr(xd), L.ptr(Wd), R, D, n1, npad, L.ptr(y), n1 + 3, L.stream()), "dgx_zs_logits_f32")
    y = y.cpu()
    assert bool((y[:, n1:] == 7.0).all()), "columns past n1 were written"
    want = x.double() @ W.double().t()[:, :n1]
    bound = D * 2.0 ** -23 * (x.double().abs() @ W.double().abs().t()[:, :n1])
    err = (y[:, :n1].double() - want).abs()
    print("R %d D %d n1 %d: worst error / bound %.3f" % (R, D, n1, float((err / bound).max())))
    assert bool((err <= bound).all())


def test_remap_keeps_ignore_rows():
    from divergen_amd.layers.dyn_vocab_ops import remap_labels
    NC, R = 37, 300
    inds = np.array([4, 7, 19, 0, 10, 12, 22, 35], np.int64)
    n = len(inds)
    cmap = np.full(NC + 1, n, np.int64)
    cmap[inds] = np.arange(n)
    rs = np.random.RandomState(5)
    lab = inds[rs.randint(0, n, R)]
    lab[:n] = inds
    lab[rs.rand(R) < 0.3] = NC
    lab[rs.rand(R) < 0.2] = -1
    lab[-1], lab[-2] = -1, NC
    got = remap_labels(torch.from_numpy(lab).to(DEV), torch.from_numpy(cmap).to(DEV), NC).cpu().numpy()
    assert got.tolist() == Z.remap(lab, cmap).tolist()
    assert (got[lab == -1] == -1).all() and (got[lab == NC] == n).all() and got.max() == n and (lab == -1).sum() > 10


# ------------------------------------------------------------------------------------------------ the predictor on the golden
@pytest.fixture(scope="module")
def gold(golden):
    return golden("dynamic_classifier")


@pytest.fixture(scope="module")
def preds(gold, tmp_path_factory):
    from test_host_dynamic_classifier import _predictor
    return {m: _predictor(tmp_path_factory.mktemp("dyn" + m), gold, m).to(DEV) for m in ("",) + Z.IMAGE_MODES}


def _dyn(gold, name, cls_score):
    from divergen_amd.layers.dyn_vocab_ops import DynamicVocab
    n = len(gold[name + ".inds"])
    dyn = DynamicVocab(torch.from_numpy(gold[name + ".inds"]).to(DEV), torch.from_numpy(gold[name + ".cls_id_map"]).to(DEV), n, Z.NUM_CLASSES)
    return dyn, (dyn.classifier(cls_score), dyn, None)


def _check_logits(got, x, gold, name):
    """The bound tests/test_gpu_zeroshot.py uses for the per-call vocabulary: one bf16 step of the stored (pre-bias) logit of the
    bf16-storage restatement, 2^-7 * max(|logit|, 1); and 2 % relative L2 against the reference's fp32 logits."""
    d = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("in.")}
    zs = torch.from_numpy(gold["zs_weight"])
    rows = zs[:, gold[name + ".inds"].tolist() + [-1]].permute(1, 0).contiguous()
    stored = ZR.classifier_logits(x, dict(d, cls_bias=torch.zeros(1)), classifier=rows, bf16=True, temp=Z.TEMP)
    want = stored + d["cls_bias"]
    bound = 2.0 ** -7 * stored.abs().clamp(min=1.0)
    print("%s: worst |logit error| / bound %.3f" % (name, float(((got - want).abs() / bound).max())))
    assert bool(((got - want).abs() <= bound).all())
    ref = torch.from_numpy(gold[name + ".logits"])
    assert float((got - ref).norm() / ref.norm()) < 2e-2
    assert bool((got[:, -1] == d["cls_bias"]).all()), "the background column is the bias alone"


@pytest.mark.parametrize("name", ["few", "many"])
def test_predictor_box_losses_against_the_reference(name, gold, preds):
    from divergen_amd.utils.events import EventStorage
    pred = preds[""]
    dyn, info = _dyn(gold, name, pred.cls_score)
    x = torch.from_numpy(gold["in." + name + ".x"])
    scores, deltas = pred(x.to(DEV), info)
    assert scores.shape == (x.shape[0], dyn.n + 1) and scores.dtype == torch.float32
    _check_logits(scores.detach().cpu(), x, gold, name)
    gt = dyn.remap(torch.from_numpy(gold["in." + name + ".gt_classes"]).to(DEV))
    with EventStorage(0) as st:
        losses = pred.losses_from_tensors(scores, deltas, gt, torch.from_numpy(gold["in." + name + ".prop"]).to(DEV),
                                          torch.from_numpy(gold["in." + name + ".gtb"]).to(DEV), None)
        stats = [float(st.latest()["fast_rcnn/" + k][0]) for k in ("cls_accuracy", "fg_cls_accuracy", "false_negative")]
    for k in ("loss_cls", "loss_box_reg"):
        e = abs(float(losses[k]) - float(gold[name + "." + k])) / abs(float(gold[name + "." + k]))
        print("%s %s %.6f against %.6f: relative %.3e" % (name, k, float(losses[k]), float(gold[name + "." + k]), e))
        assert e <= 1e-3, k
    print("statistics", stats, gold[name + ".stats"].tolist())
    np.testing.assert_allclose(stats, gold[name + ".stats"], rtol=1e-6)
    (losses["loss_cls"] + losses["loss_box_reg"]).backward()
    assert bool(pred.cls_score.linear.weight.grad.abs().sum() > 0)
    pred.zero_grad()


@pytest.mark.parametrize("mode", Z.IMAGE_MODES)
def test_predictor_image_loss_against_the_reference(mode, gold, preds):
    from divergen_amd.layers.image_label_ops import label_csr
    from divergen_amd.utils.events import EventStorage
    pred = preds[mode]
    dyn, info = _dyn(gold, "image", pred.cls_score)
    x = torch.from_numpy(gold["in.image.x"])
    scores = pred(x.to(DEV), info)[0]
    _check_logits(scores.detach().cpu(), x, gold, "image")
    csr = label_csr(Z.IMAGE_LABELS, torch.device(DEV, 0))
    csr = (csr[0], dyn.remap(csr[1].long()).to(torch.int32), csr[2])
    assert csr[1].cpu().tolist() == [int(gold["image.cls_id_map"][c]) for ls in Z.IMAGE_LABELS for c in ls]
    with EventStorage(0):
        losses = pred.image_label_losses(scores, None, torch.from_numpy(gold["in.image.boxes"]).to(DEV), Z.IMAGE_COUNTS, Z.IMAGE_SIZES, None, csr=csr)
    want = float(gold["image.%s.image_loss" % mode])
    e = abs(float(losses["image_loss"]) - want) / want
    print("%s image_loss %.6f against %.6f: relative %.3e" % (mode, float(losses["image_loss"]), want, e))
    assert e <= 1e-3


# ------------------------------------------------------------------------------------------------ the assembled model
LOSS_KEYS = {"%s_stage%d" % (n, k) for n in ("image_loss", "loss_cls", "loss_box_reg") for k in range(3)} | {
    "loss_mask", "loss_centernet_loc", "loss_centernet_agn_pos", "loss_centernet_agn_neg"}
NC = 37


def _build(tmp, S, dynamic=True, uniform=False):
    from divergen_amd.config import get_cfg
    from divergen_amd.modeling import build_model
    from divergen_amd.modeling.backbone.swintransformer import DropPath
    from divergen_amd.solver import build_optimizer
    os.makedirs(str(tmp), exist_ok=True)
    npy, freq = os.path.join(str(tmp), "emb.npy"), os.path.join(str(tmp), "freq.json")
    np.save(npy, np.random.default_rng(3).standard_normal((NC, 512)).astype(np.float32))
    rs = np.random.RandomState(9)
    json.dump([{"id": i + 1, "image_count": 1 if uniform else int(rs.randint(1, 400))} for i in range(NC)], open(freq, "w"))
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "DiverGen_swinL.yaml"))
    cfg.merge_from_list(["MODEL.SWIN.SIZE", "T", "WITH_IMAGE_LABELS", True, "MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "max_size",
                         "MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX", True, "MODEL.ROI_BOX_HEAD.WS_NUM_PROPS", 32, "MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", freq,
                         "MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", True, "MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH", npy, "MODEL.ROI_HEADS.NUM_CLASSES", NC,
                         "MODEL.ROI_BOX_HEAD.USE_BIAS", -4.6, "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", False]
                        + (["MODEL.DYNAMIC_VOCAB", True, "MODEL.DYNAMIC_CLASSIFIER", True, "MODEL.NUM_SAMPLE_CATS", S] if dynamic else []))
    torch.manual_seed(42)
    model = build_model(cfg).train()
    for m in model.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    return cfg, model, build_optimizer(cfg, model)


def _batches():
    from divergen_amd.data import synthetic_batch
    from divergen_amd.structures import BitMasks, Boxes, Instances
    box_batch = synthetic_batch(2, 256, NC, device=DEV)
    for d in box_batch:
        d.update(ann_type="box", pos_category_ids=[], dataset_source=0)
    labels = [[3, 11, NC - 1], [5]]
    img_batch = []
    for d, ls in zip(synthetic_batch(2, 256, NC, device=DEV), labels):
        h, w = d["image"].shape[-2:]
        inst = Instances((h, w), gt_boxes=Boxes(torch.zeros(0, 4, device=DEV)), gt_classes=torch.zeros(0, dtype=torch.int64, device=DEV),
                         gt_masks=BitMasks(torch.zeros(0, h, w, dtype=torch.bool, device=DEV)))
        img_batch.append(dict(d, instances=inst, ann_type="image", pos_category_ids=ls, dataset_source=1))
    return box_batch, img_batch, labels


def _spy_sampler(model, log):
    plain = model._sample_cls_inds

    def spy(*a, **k):
        dyn = plain(*a, **k)
        log.append(dyn)
        return dyn
    model._sample_cls_inds = spy


def test_box_step_and_image_step_of_the_assembled_model(tmp_path):
    from divergen_amd.engine import total_loss
    from divergen_amd.utils.events import EventStorage
    S = 24          # more than the classes of the synthetic batch: classes are drawn on the box step as well
    cfg, model, opt = _build(tmp_path, S)
    assert model.dynamic_classifier and "freq_weight" not in model.state_dict() and not any("freq_weight" in k for k in model.state_dict())
    box_batch, img_batch, labels = _batches()
    rh = model.roi_heads
    seen, dyns = [], []
    rh.__dict__["stage_observer"] = lambda k, d: seen.append((k, d))
    _spy_sampler(model, dyns)

    def box_step(seed):
        seen.clear()
        dyns.clear()
        torch.manual_seed(seed)
        opt.zero_grad()
        losses = model(box_batch)
        total_loss(losses).backward()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in losses.items()}

    with EventStorage(0) as st:
        bl = box_step(7)
        assert set(bl) == LOSS_KEYS and all(bool(torch.isfinite(v)) for v in bl.values()), bl
        dyn = dyns[0]
        n = dyn.n
        gt_all = torch.cat([d["instances"].gt_classes for d in box_batch])
        a = int(torch.unique(gt_all).numel())
        assert a < S and n == S and len(seen) == 3
        inds = dyn.inds[:n].cpu()
        assert inds[:a].tolist() == torch.unique(gt_all).cpu().tolist()
        for k, d in seen:
            g = d["gt_classes"].cpu()
            _check_remap(d, dyn)
            assert int(g.max()) <= n and int(g.min()) >= -1 and bool((g[g >= 0] <= n).all())
            assert bool(((g >= 0) & (g < n)).any()) and bool((g == n).any())
            assert float(bl["loss_cls_stage%d" % k]) > 0 and float(bl["image_loss_stage%d" % k]) == 0.0
        print("n %d, a %d" % (n, a))
        for k in range(3):
            assert bool(rh.box_predictor[k].cls_score.linear.weight.grad.abs().sum() > 0), k
        # the columns of classes that were not sampled do not matter: overwritten, every loss is bit-identical
        zs = rh.box_predictor[0].cls_score.zs_weight
        others = torch.tensor([c for c in range(NC) if c not in set(inds.tolist())], device=DEV)
        assert len(others) == NC - n
        keep = zs.clone()
        with torch.no_grad():
            for k in range(3):
                rh.box_predictor[k].cls_score.zs_weight[:, others] = 7.0
        bl2 = box_step(7)
        with torch.no_grad():
            for k in range(3):
                rh.box_predictor[k].cls_score.zs_weight.copy_(keep)
        assert dyns[0].inds[:n].cpu().tolist() == inds.tolist()
        for k in bl:
            assert torch.equal(bl[k], bl2[k]), k
        # ignore rows: stage 0's deltas push every second box far out of the image, so the hand-over clips it to an empty box and
        # dgx_cascade_refine labels the row -1 in stages 1 and 2; the remap must leave exactly those rows at -1 (torch's
        # cls_id_map[-1] would make them background, n)
        def shove(m, i, o):
            d = o[1].clone()
            d[::2, 0] += 500.0
            return (o[0], d) + tuple(o[2:])
        hook = rh.box_predictor[0].register_forward_hook(shove)
        try:
            bl3 = box_step(7)
        finally:
            hook.remove()
        assert len(seen) == 3 and all(bool(torch.isfinite(v)) for v in bl3.values()), bl3
        counts = [_check_remap(d, dyns[0]) for _, d in seen]
        print("ignore rows per stage with every second stage-0 box shoved out of the image:", counts)
        assert counts[0] == 0 and counts[1] > 0 and counts[2] > 0
        # an image step: n from the lists, no device->host read in the new host calls
        seen.clear()
        dyns.clear()
        opt.zero_grad()
        torch.manual_seed(8)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            dyn_i = model._sample_cls_inds([_with_ids(d) for d in img_batch], "image")
            info = (dyn_i.classifier(rh.box_predictor[0].cls_score), dyn_i, None)
            from divergen_amd.layers.image_label_ops import label_csr
            csr = label_csr(labels, torch.device(DEV, 0))
            remapped = dyn_i.remap(csr[1].long()).to(torch.int32)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert dyn_i.n == S and info[0].n1 == S + 1
        want = [int(dyn_i.cls_id_map[c]) for ls in labels for c in ls]
        assert remapped.cpu().tolist() == want and want == [0, 2, 3, 1]
        dyns.clear()
        il = model(img_batch)
        total_loss(il).backward()
        torch.cuda.synchronize()
        assert set(il) == LOSS_KEYS and all(bool(torch.isfinite(v)) for v in il.values())
        for k in range(3):
            assert float(il["image_loss_stage%d" % k]) > 0 and float(il["loss_cls_stage%d" % k]) == 0.0
            assert bool(rh.box_predictor[k].cls_score.linear.weight.grad.abs().sum() > 0), k
        for k in range(3):          # logged inside each stage's scope, as the reference's image_label_losses does
            assert float(st.latest()["stage%d/stats_label" % k][0]) == labels[0][0]
        assert "stats_label" not in st.latest()


def _check_remap(d, dyn):
    """What the observer saw of one stage: labels after the remap against the labels before it.  -1 exactly where -1 was, the
    background (num_classes) at n, every other label at its column; -> the number of ignore rows."""
    full, g = d["gt_classes_full"].cpu(), d["gt_classes"].cpu()
    cmap, n = dyn.cls_id_map.cpu(), dyn.n
    assert torch.equal(g == -1, full == -1), "ignore rows were not kept by the remap"
    keep = full >= 0
    assert torch.equal(g[keep], cmap[full[keep]]) and bool((g[full == NC] == n).all()) and int(cmap[NC]) == n
    assert int(g.max()) <= n and int(g.min()) >= -1
    return int((g == -1).sum())


def _with_ids(d):
    inst = d["instances"]
    inst._pos_category_ids = d["pos_category_ids"]
    return inst


def test_full_vocabulary_sample_equals_the_restatement(tmp_path):
    """Uniform positive weights and NUM_SAMPLE_CATS = num_classes: every class is sampled, the sampled columns are a permutation of the
    vocabulary; loss_cls of each stage equals the float64 sigmoid CE over the FULL vocabulary (columns put back in class order, labels
    mapped back through inds) within 1e-3."""
    from divergen_amd.engine import total_loss
    from divergen_amd.utils.events import EventStorage
    cfg, model, opt = _build(tmp_path, NC, uniform=True)
    box_batch, _, _ = _batches()
    rh = model.roi_heads
    seen, dyns, scores = [], [], []
    rh.__dict__["stage_observer"] = lambda k, d: seen.append((k, d))
    _spy_sampler(model, dyns)
    hooks = [rh.box_predictor[k].register_forward_hook(lambda m, i, o: scores.append(o[0].detach())) for k in range(3)]
    with EventStorage(0):
        torch.manual_seed(11)
        losses = model(box_batch)
        total_loss(losses).backward()
        torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    dyn = dyns[0]
    assert dyn.n == NC and sorted(dyn.inds[:NC].cpu().tolist()) == list(range(NC))
    inds = dyn.inds[:NC].cpu().numpy()
    for (k, d), sc in zip(seen, scores):
        g = d["gt_classes"].cpu().numpy()
        R = len(g)
        lg = sc[:R].double().cpu().numpy()
        full = np.empty_like(lg)
        full[:, inds] = lg[:, :NC]
        full[:, NC] = lg[:, NC]
        lab = np.where(g < 0, g, np.where(g < NC, inds[np.clip(g, 0, NC - 1)], NC))
        want = Z.box_losses(full, np.zeros((R, 4)), lab, d["boxes"].cpu().numpy(), d["gt_boxes"].cpu().numpy())[0]
        got = float(losses["loss_cls_stage%d" % k].detach())
        print("stage %d loss_cls %.6f, float64 over the full vocabulary %.6f" % (k, got, want))
        assert abs(got - want) <= 1e-3 * want
