"""Generate tests/golden/caption_loss.npz: caption supervision of the box predictor (MODEL.WITH_CAPTION) from the reference's own code.
Run in the authoring container only:

    python tests/golden/make_golden_caption_loss.py

On the frozen inputs of tests/_caption_loss_ref.golden_inputs() it runs the real DeticFastRCNNOutputLayers (DG/divergen/modeling/
roi_heads/detic_fast_rcnn.py) with the real ZeroShotClassifier as its cls_score (USE_BIAS -2, NORM_WEIGHT, NORM_TEMP 50,
image_label_loss 'max_size', ADD_IMAGE_BOX, CAPTION_WEIGHT 0.5, NEG_CAP_WEIGHT 0.125): `forward` with classifier_info[2] (:437-466) and
`image_label_losses` (:342-434 with `_caption_loss`, :469-506) for
  * ann_type 'caption', 'captiontag' and, for the difference, 'image' on the same rows;
  * the synced form: comm.get_rank stubbed to rank 1, the gathered matrix of 3 ranks (rank 0's captions, this rank's, rank 2 all
    zeros: a rank on a box step), each row with its rank column.
Recorded: the concatenated scores, image_loss, stats_l_caption, stats_l_image and the gradients with respect to x, the projected rows
u = cls_score.linear(x) (kept by a forward hook on the reference's own module), cls_score.linear.* and cls_bias.  The real
CustomRCNN._sync_caption_features (DG custom_rcnn.py:210-223) runs for three simulated ranks (a box step with CAP_BATCH_RATIO 4, a
caption step, an image step): what every rank sent and what it got back.
It also measures the reference's OWN fp32 evaluation against the float64 restatement (tests/_caption_loss_ref.py) in the form the tests'
bound has, |got - ref| <= rtol * max(|ref|, floor) at rtol = 1e-5, on the golden inputs and on the inputs of the GPU tests
(_caption_loss_ref.GPU_CASES, values as stored in fp32 and in bf16; the reference is given the surviving rows of every image and an
identity `linear`, so that the rows it projects are the stored u), and records the worst ratios (`measured.*`): the tests' rtol comes
from these numbers, never from the kernel.  `measured.bf16_u` is how far the loss moves, relatively, when u is rounded to bf16.
The reference is imported through _refload; nothing of it is copied or restated.  Fixed zip timestamps: two runs give identical bytes."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refload as R  # noqa: E402
import _caption_loss_ref as C  # noqa: E402
from make_golden_blend import save_deterministic  # noqa: E402
from make_golden_dynamic import _more_stubs as _meta_stubs  # noqa: E402
from make_golden_image_labels import _more_stubs  # noqa: E402

TMP = tempfile.mkdtemp()


def predictor(fr, zc, Cin, D, zs, use_bias, norm_weight, sync, neg_cap_weight):
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.box_regression import Box2BoxTransform
    npy = os.path.join(TMP, "zs_%d_%d.npy" % (zs.shape[0], D))
    np.save(npy, zs)
    cls = zc.ZeroShotClassifier(ShapeSpec(channels=Cin), num_classes=zs.shape[0], zs_weight_path=npy, zs_weight_dim=D,
                                use_bias=use_bias, norm_weight=norm_weight, norm_temperature=C.TEMP)
    return fr.DeticFastRCNNOutputLayers(ShapeSpec(channels=Cin), box2box_transform=Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0)),
                                        num_classes=zs.shape[0], cls_agnostic_bbox_reg=True, smooth_l1_beta=0.0, use_sigmoid_ce=True,
                                        use_fed_loss=False, use_zeroshot_cls=True, cls_score=cls, image_label_loss="max_size",
                                        image_loss_weight=C.IMAGE_LOSS_WEIGHT, add_image_box=True, caption_weight=C.CAPTION_WEIGHT,
                                        neg_cap_weight=neg_cap_weight, sync_caption_batch=sync)


def run_reference(pred, x, counts, labels, cap, ann_type, rank=0):
    """forward + image_label_losses of the reference on rows x (sum(counts), Cin) -> dict of float32 arrays."""
    from detectron2.structures import Boxes, Instances
    comm = sys.modules["detectron2.utils.comm"]
    xt = torch.from_numpy(np.ascontiguousarray(x)).clone().requires_grad_(True)
    kept = []

    def keep_output(module, inputs, output):
        output.retain_grad()
        kept.append(output)
    hook = pred.cls_score.linear.register_forward_hook(keep_output)
    props = []
    g = torch.Generator().manual_seed(5)
    for n in counts:
        p = Instances((200, 300))
        xy = torch.rand(n, 2, generator=g) * 100
        p.proposal_boxes = Boxes(torch.cat([xy, xy + 5 + torch.rand(n, 2, generator=g) * 90], 1))
        p.objectness_logits = torch.zeros(n)
        props.append(p)
    ci = (None, None, torch.from_numpy(np.ascontiguousarray(cap)) if cap is not None else None)
    R._STORAGE.scalars.clear()
    for q in pred.parameters():
        q.grad = None
    old = comm.get_rank
    comm.get_rank = lambda: rank
    try:
        preds = pred(xt, ci)
        losses = pred.image_label_losses(preds, props, labels, classifier_info=ci, ann_type=ann_type)
    finally:
        comm.get_rank = old
        hook.remove()
    assert set(losses) == {"image_loss", "loss_cls", "loss_box_reg"}
    assert float(losses["loss_cls"]) == 0.0 and float(losses["loss_box_reg"]) == 0.0
    losses["image_loss"].backward()
    u = kept[0]
    du = sum(k.grad for k in kept if k.grad is not None)      # (forward calls cls_score once per score block: the same rows twice)
    named = dict(pred.named_parameters())
    st = R._STORAGE.scalars
    out = dict(scores=preds[0].detach().numpy(), deltas=preds[1].detach().numpy(), image_loss=losses["image_loss"].detach().numpy(),
               l_caption=np.float64(st.get("stats_l_caption", 0.0)), l_image=np.float64(st["stats_l_image"]),
               u=u.detach().numpy(), du=du.numpy(), dx=xt.grad.numpy(), dlin_w=named["cls_score.linear.weight"].grad.numpy(),
               dlin_b=named["cls_score.linear.bias"].grad.numpy())
    if "cls_score.cls_bias" in named:
        out["dbias"] = named["cls_score.cls_bias"].grad.numpy()
    for k in ("pool_stats", "stats_select_size", "stats_select_x", "stats_select_y", "stats_max_label_score"):
        out["stat." + k] = np.float64(st[k])
    return out


def restate(u, valid, counts, cap, D, target0, bias, neg_weight, norm_weight=True):
    s, ss = C.scales(len(counts))
    return C.caption_loss(u, valid, counts, cap, D, target0, C.TEMP, norm_weight, bias, neg_weight, s, ss)


def ratios(got, r64):
    """Worst |reference fp32 - float64| in units of 1e-5 * max(|float64|, floor): loss, du, d cls_bias."""
    m = [abs(float(got["image_loss"]) - r64["loss"]) / (1e-5 * max(abs(r64["loss"]), r64["floor_loss"])),
         C.worst_ratio(got["du"], r64["du"], r64["floor_du"], 1e-5)]
    m.append(abs(float(np.asarray(got["dbias"]).reshape(-1)[0]) - r64["dbias"]) / (1e-5 * max(abs(r64["dbias"]), r64["floor_dbias"])) if "dbias" in got else 0.0)
    return np.array(m, np.float64)


def measure_case(fr, zc, c, k, rnd):
    """The reference on GPU case k (values rounded by `rnd`) against the restatement -> (loss, du, dbias) ratios, bf16_u move."""
    B, N, D, target0, _, _, bias, negw, norm_weight = c
    d = C.case_inputs(c, k)
    u, cap, counts, valid = rnd(d["u"]), d["cap"], d["counts"], d["valid"].astype(bool)
    R_ = sum(counts)
    keep = np.nonzero(valid)[0]
    alive = [int(valid[o:o + n].sum()) for o, n in zip(np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(int), counts)]
    synced = not (N == B and target0 == 0 and negw == 1.0)
    rank = target0 // B
    assert rank * B == target0
    pred = predictor(fr, zc, D, D, C.unit_rows(np.random.default_rng(1), 3, D), bias if bias is not None else 0.0, norm_weight, synced, negw)
    with torch.no_grad():
        pred.cls_score.linear.weight.copy_(torch.eye(D))
        pred.cls_score.linear.bias.zero_()
    capm = np.concatenate([cap, np.full((N, 1), rank, np.float32)], 1) if synced else cap
    g = run_reference(pred, u[:R_][keep], alive, [[] for _ in counts], capm, "caption", rank)
    du = np.zeros((u.shape[0], D), np.float32)
    du[keep] = g["du"]
    g["du"] = du
    r64 = restate(u, d["valid"], counts, cap, D, target0, bias, negw, norm_weight)
    exact = restate(d["u"], d["valid"], counts, cap, D, target0, bias, negw, norm_weight)
    move = abs(r64["loss"] - exact["loss"]) / abs(exact["loss"])
    return ratios(g, r64), move


def gen_sync(cr, out):
    """CustomRCNN._sync_caption_features for three simulated ranks: a first pass records what each rank sends, a second hands every
    rank the full list."""
    comm = sys.modules["detectron2.utils.comm"]
    rng = np.random.default_rng(77)
    BS, D = 8, 512
    feats = torch.from_numpy(rng.standard_normal((BS, D)).astype(np.float32))
    steps = [("box", 2, None), ("caption", BS, feats), ("image", BS, None)]      # rank 0: 2 images x CAP_BATCH_RATIO 4
    sent = []
    old = (comm.get_rank, getattr(comm, "all_gather", None))
    try:
        for pass_ in (0, 1):
            for rank, (ann, bs, f) in enumerate(steps):
                me = types.SimpleNamespace(cap_batch_ratio=4, device="cpu")
                comm.get_rank = lambda rank=rank: rank
                comm.all_gather = (lambda t: (sent.append(t.clone()), [t])[1]) if pass_ == 0 else (lambda t: list(sent))
                got = cr.CustomRCNN._sync_caption_features(me, f, ann, bs)
                if pass_ == 1:
                    assert (got is None) == (f is None)
                    if got is not None:
                        out["sync.out_rank%d" % rank] = got.numpy()
    finally:
        comm.get_rank = old[0]
        if old[1] is not None:
            comm.all_gather = old[1]
    out["sync.features"] = feats.numpy()
    for r, t in enumerate(sent):
        out["sync.sent_rank%d" % r] = t.numpy()
    assert out["sync.out_rank1"].shape == (24, D + 1) and not out["sync.sent_rank0"][:, :D].any()


def main():
    _more_stubs()
    _meta_stubs()
    fr = R.ref("divergen.modeling.roi_heads.detic_fast_rcnn")
    zc = R.ref("divergen.modeling.roi_heads.zero_shot_classifier")
    cr = R.ref("divergen.modeling.meta_arch.custom_rcnn")
    d = C.golden_inputs()
    B, D = d["B"], d["D"]
    out = {}
    worst = np.zeros(3)
    gathered = np.concatenate([np.concatenate([d["cap_other"][:B], np.zeros((B, 1), np.float32)], 1),
                               np.concatenate([d["cap"], np.full((B, 1), 1.0, np.float32)], 1),
                               np.concatenate([np.zeros((B, D), np.float32), np.full((B, 1), 2.0, np.float32)], 1)], 0)
    assert d["rank"] == 1 and d["world"] == 3 and gathered.shape == (3 * B, D + 1)
    out["in.gathered"] = gathered
    for name, ann, cap, sync in (("caption", "caption", d["cap"], False), ("captiontag", "captiontag", d["cap"], False),
                                 ("image", "image", None, False), ("synced", "caption", gathered, True)):
        pred = predictor(fr, zc, d["Cin"], D, d["zs"], d["use_bias"], True, sync, C.NEG_CAP_WEIGHT)
        with torch.no_grad():
            pred.cls_score.linear.weight.copy_(torch.from_numpy(d["lin_w"]))
            pred.cls_score.linear.bias.copy_(torch.from_numpy(d["lin_b"]))
            torch.manual_seed(3)
            for q in pred.bbox_pred.parameters():
                q.normal_(0, 0.1)
        if name == "caption":
            for k, v in pred.state_dict().items():
                out["param." + k] = v.numpy().copy()
        g = run_reference(pred, d["x"], d["counts"], d["labels"], cap, ann, d["rank"] if sync else 0)
        out.update({name + "." + k: v for k, v in g.items()})
        if name in ("caption", "synced"):
            assert float(g["l_image"]) == 0.0
            r64 = restate(g["u"], None, d["counts"], cap, D, B * d["rank"] if sync else 0, d["use_bias"], C.NEG_CAP_WEIGHT if sync else 1.0)
            m = ratios(g, r64)
            print("golden %s: reference fp32 vs float64, worst ratio at rtol 1e-5 (loss, du, dbias):" % name, m)
            worst = np.maximum(worst, m)
            assert abs(float(g["l_caption"]) * C.IMAGE_LOSS_WEIGHT - float(g["image_loss"])) < 1e-6 * abs(float(g["image_loss"]))
    assert out["caption.scores"].shape == (sum(d["counts"]), d["C"] + 1 + B)
    assert out["synced.scores"].shape == (sum(d["counts"]), d["C"] + 1 + 3 * B)
    tag = float(out["captiontag.image_loss"])
    assert abs(tag - float(out["caption.image_loss"]) - float(out["image.image_loss"])) < 1e-5 * abs(tag)
    out["measured.golden"] = worst
    # ---- the same measurement on the inputs of the GPU tests, as stored in fp32 and in bf16; the bf16 move of the loss
    worst_c, move = np.zeros(3), 0.0
    for k, c in enumerate(C.GPU_CASES):
        for rnd in (lambda a: a, C.bf16_round):
            m, mv = measure_case(fr, zc, c, k, rnd)
            worst_c = np.maximum(worst_c, m)
            move = max(move, mv)
    print("GPU test inputs: reference fp32 vs float64, worst ratio at rtol 1e-5 (loss, du, dbias):", worst_c)
    print("loss moved by rounding u to bf16 (relative, worst case):", move)
    out["measured.cases"] = worst_c
    out["measured.bf16_u"] = np.float64(move)
    gen_sync(cr, out)
    save_deterministic(os.path.join(HERE, "caption_loss.npz"), out)


if __name__ == "__main__":
    main()
