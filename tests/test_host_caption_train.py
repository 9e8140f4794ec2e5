"""Host tests of caption training (MODEL.CAPTION_TRAIN: MODEL.WITH_CAPTION, DATALOADER.DATASET_ANN 'caption' / 'captiontag'): the key
and its start-up checks, the data path, the cross-rank caption batch, the caption draws, the float64 restatement of the caption loss
(tests/_caption_loss_ref.py) against the reference's own outputs (tests/golden/caption_loss.npz), the predictor's forward with
classifier_info[2], the model's state dict and the library's new symbols.

Bound of the restatement tests: |reference fp32 - float64| <= 1e-5 * max(|float64|, floor), the form and the rtol the golden generator
measured the reference's own evaluation in (`measured.*`: worst ratio 0.0065 on the golden inputs, 0.025 on the GPU tests' inputs)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _caption_fixtures as F  # noqa: E402
import _caption_loss_ref as C  # noqa: E402

RTOL = 1e-5
NEW_SYMBOLS = ("dgx_caption_prepare", "dgx_caption_workspace_floats", "dgx_caption_loss")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "caption_loss.npz"))


# ------------------------------------------------------------------------------------------------ key and start-up checks
def _check(cfg, per_gpu=2):
    from divergen_amd.config.image_labels import check_loader_keys, check_model_keys
    check_model_keys(cfg)
    check_loader_keys(cfg, per_gpu)


def test_key_defaults_and_the_two_source_configuration(tmp_path, monkeypatch):
    from divergen_amd.config import get_cfg
    d = get_cfg()
    assert d.MODEL.CAPTION_TRAIN is False and d.MODEL.TEXT_ENCODER_WEIGHTS == "" and d.MODEL.TEXT_ENCODER_BPE == ""
    for ann in ("captiontag", "caption"):
        cfg, _, _ = F.two_source_cfg(tmp_path / ann, monkeypatch, ann=ann)
        _check(cfg)
    # without the key the same configuration is refused by name, as before
    cfg, _, _ = F.two_source_cfg(tmp_path / "nokey", monkeypatch, key=False)
    with pytest.raises(NotImplementedError, match="WITH_CAPTION"):
        _check(cfg)
    cfg.merge_from_list(["MODEL.WITH_CAPTION", False])
    with pytest.raises(NotImplementedError, match="DATASET_ANN"):
        _check(cfg)


DIFF_BS = ["DATALOADER.USE_DIFF_BS_SIZE", True, "DATALOADER.DATASET_INPUT_SIZE", [128, 64], "DATALOADER.DATASET_INPUT_SCALE", [[0.9, 1.5], [0.8, 1.2]]]
REQUIRED = [
    (["WITH_IMAGE_LABELS", False], ValueError, "WITH_IMAGE_LABELS"),
    (["MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS", False], ValueError, "USE_ZEROSHOT_CLS"),
    (["MODEL.ROI_BOX_HEAD.ADD_IMAGE_BOX", False], ValueError, "ADD_IMAGE_BOX"),
    (["MODEL.TEXT_ENCODER_WEIGHTS", ""], ValueError, "TEXT_ENCODER_WEIGHTS"),
    (["MODEL.TEXT_ENCODER_BPE", ""], ValueError, "TEXT_ENCODER_BPE"),
    (["MODEL.WITH_CAPTION", False], ValueError, "WITH_CAPTION"),                       # a caption source without the model's half
    (["MODEL.DYNAMIC_CLASSIFIER", True, "MODEL.DYNAMIC_VOCAB", True], NotImplementedError, "DYNAMIC_CLASSIFIER"),
    (["MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP", True, "MODEL.ROI_BOX_HEAD.WS_PROP_SCORE", True], NotImplementedError, "WITH_SOFTMAX_PROP"),
    (["MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsddn", "MODEL.ROI_BOX_HEAD.WS_PROP_SCORE", True], NotImplementedError, "wsddn"),
    (["DATALOADER.DATASET_ANN", ["box", "prop"]], NotImplementedError, "DATASET_ANN"),
    (["DATALOADER.DATASET_ANN", ["box", "proptag"]], NotImplementedError, "DATASET_ANN"),
    (["MODEL.SYNC_CAPTION_BATCH", True, "MODEL.CAP_BATCH_RATIO", 4], ValueError, "CAP_BATCH_RATIO"),      # no USE_DIFF_BS_SIZE: ratio 1 only
    (["MODEL.SYNC_CAPTION_BATCH", True, "MODEL.CAP_BATCH_RATIO", 4, "DATALOADER.DATASET_BS", [2, 4]] + DIFF_BS, ValueError, "SYNC_CAPTION_BATCH"),
    (["MODEL.SYNC_CAPTION_BATCH", True, "MODEL.CAP_BATCH_RATIO", 4, "DATALOADER.DATASET_BS", [9, 36]] + DIFF_BS, ValueError, "REFINE_MAX_IMAGES"),
    (["MODEL.SYNC_CAPTION_BATCH", True, "MODEL.WITH_CAPTION", False, "DATALOADER.DATASET_ANN", ["box", "image"]], ValueError, "SYNC_CAPTION_BATCH"),
]


@pytest.mark.parametrize("opts,exc,key", REQUIRED, ids=["%s%d" % (r[2], i) for i, r in enumerate(REQUIRED)])
def test_every_requirement_and_refusal_names_its_key(opts, exc, key, tmp_path, monkeypatch):
    cfg, _, _ = F.two_source_cfg(tmp_path, monkeypatch, extra=opts)
    with pytest.raises(exc, match=key):
        _check(cfg)


def test_sync_batch_rule_admits_the_matching_sizes(tmp_path, monkeypatch):
    cfg, _, _ = F.two_source_cfg(tmp_path, monkeypatch, extra=["MODEL.SYNC_CAPTION_BATCH", True, "MODEL.CAP_BATCH_RATIO", 4,
                                                                "DATALOADER.DATASET_BS", [2, 8]] + DIFF_BS)
    _check(cfg)
    cfg.merge_from_list(["DATALOADER.USE_DIFF_BS_SIZE", False, "MODEL.CAP_BATCH_RATIO", 1])
    _check(cfg)


def test_encoder_geometry_comes_from_the_state_dict_and_its_dim_is_checked(tmp_path, monkeypatch):
    from divergen_amd.config.caption import check_text_encoder_dim
    from divergen_amd.modeling.text import build_text_encoder
    from divergen_amd.modeling.text.text_encoder import state_dict_geometry
    weights, bpe = F.write_text_encoder(tmp_path / "e", embed_dim=24, transformer_layers=3, vocab_size=530, context_length=40)
    want = dict(F.GEOMETRY, embed_dim=24, transformer_layers=3, vocab_size=530, context_length=40)
    assert state_dict_geometry(torch.load(weights)) == want
    enc = build_text_encoder(weights, bpe, geometry_from_weights=True)
    assert (enc.embed_dim, enc.context_length, enc.vocab_size, enc.transformer.width, enc.transformer.layers) == (24, 40, 530, 64, 3)
    with pytest.raises(RuntimeError):            # the existing behaviour stays: the ViT-B/32 geometry unless told otherwise
        build_text_encoder(weights, bpe)
    cfg, _, _ = F.two_source_cfg(tmp_path / "c", monkeypatch)
    with pytest.raises(ValueError, match="ZEROSHOT_WEIGHT_DIM"):
        check_text_encoder_dim(cfg, 24)
    check_text_encoder_dim(cfg, 512)


# ------------------------------------------------------------------------------------------------ data path
def test_loader_carries_captions(tmp_path, monkeypatch):
    """load_lvis_json copies `captions`; the mapper treats a caption sample as an image-labelled one (empty instances, no copy-paste
    draw of its own, pos_category_ids kept); pack_sample passes the strings through; a CPU loader yields 'caption' batches; the box
    source consumes np.random exactly as it does beside a plain image source."""
    from divergen_amd.data import build as B
    cfg, info, il = F.two_source_cfg(tmp_path, monkeypatch, ann="caption", extra=[
        "DATALOADER.DATASET_BS", [2, 4], "INPUT.INST_POOL", False] + DIFF_BS)
    recs = B.load_lvis_json(il["json"], il["image_root"])
    assert all(1 <= len(r["captions"]) <= 3 and all(isinstance(c, str) and 3 <= len(c.split()) <= 8 for c in r["captions"]) for r in recs)
    assert "captions" not in B.load_lvis_json(os.path.join(info["root"], "lvis", "lvis_v1_train.json"), info["root"])[0]
    dicts = B.get_detection_dataset_dicts_with_source(cfg.DATASETS.TRAIN, filter_empty=False, dataset_ann=cfg.DATALOADER.DATASET_ANN)
    plain = B.DatasetMapper(cfg, True)
    mapper = B.CopyPasteMapper(plain, cfg)
    mapper.set_dataset(dicts)
    mapper.pack = False
    np.random.seed(5)
    want = plain(dicts[14])
    state = np.random.get_state()
    np.random.seed(5)
    got = mapper(dicts[14])
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state())), "a caption sample made a copy-paste draw"
    assert torch.equal(got["image"], want["image"]) and "paste_pack" not in got
    assert got["ann_type"] == "caption" and got["captions"] == dicts[14]["captions"] and got["pos_category_ids"] == dicts[14]["pos_category_ids"]
    assert len(got["instances"]) == 0 and got["instances"].has("gt_masks")
    assert B.pack_sample(dict(got))["captions"] == got["captions"]
    # the box source beside a caption source and beside a plain image source: the same draws, the same pixels
    np.random.seed(6)
    box = mapper(dicts[2])
    after = np.random.get_state()
    cfg2 = cfg.clone()
    cfg2.defrost()
    cfg2.merge_from_list(["DATALOADER.DATASET_ANN", ["box", "image"], "MODEL.WITH_CAPTION", False])
    m2 = B.CopyPasteMapper(B.DatasetMapper(cfg2, True), cfg2)
    m2.set_dataset(dicts)
    m2.pack = False
    np.random.seed(6)
    box2 = m2(dicts[2])
    assert all(np.array_equal(a, b) for a, b in zip(after, np.random.get_state())) and torch.equal(box["image"], box2["image"])
    assert box["ann_type"] == "box" and "captions" not in box
    it = B.build_detection_train_loader(cfg, 2, "cpu", 3)
    seen = set()
    for _ in range(8):
        batch = next(it)
        (src, ann), = {(d["dataset_source"], d["ann_type"]) for d in batch}
        assert (src, ann, len(batch)) in ((0, "box", 2), (1, "caption", 4))
        if ann == "caption":
            assert all(isinstance(d["captions"], list) and d["captions"] and len(d["instances"]) == 0 for d in batch)
        seen.add(ann)
    assert seen == {"box", "caption"}


# ------------------------------------------------------------------------------------------------ the cross-rank caption batch
def test_sync_caption_features_equals_the_reference_for_three_ranks(gold):
    """Rank 0 on a box step (2 images x CAP_BATCH_RATIO 4), rank 1 on a caption step, rank 2 on an image step: what each sends and what it
    gets back equal the recording of the reference's _sync_caption_features; None where the reference returns None."""
    from divergen_amd.layers.caption_ops import sync_caption_features
    feats = torch.from_numpy(gold["sync.features"])
    steps = [("box", 2, None), ("caption", 8, feats), ("image", 8, None)]
    sent = []
    for rank, (ann, bs, f) in enumerate(steps):
        sync_caption_features(f, ann, bs, rank, 4, lambda rows: (sent.append(rows.clone()), [rows])[1], dim=512, device="cpu")
    for rank in range(3):
        assert torch.equal(sent[rank], torch.from_numpy(gold["sync.sent_rank%d" % rank])), rank
    for rank, (ann, bs, f) in enumerate(steps):
        got = sync_caption_features(f, ann, bs, rank, 4, lambda rows: list(sent), dim=512, device="cpu")
        if f is None:
            assert got is None
        else:
            assert torch.equal(got, torch.from_numpy(gold["sync.out_rank1"])) and got.shape == (24, 513)
    with pytest.raises(ValueError, match="SYNC_CAPTION_BATCH"):      # a rank that sends another row count: caught on the host
        sync_caption_features(feats, "caption", 8, 1, 4, lambda rows: [sent[0][:4], rows, sent[2]], dim=512, device="cpu")


def test_all_gather_rows_without_a_process_group_is_world_size_one():
    from divergen_amd.layers.caption_ops import all_gather_rows
    rows = torch.arange(6.0).reshape(2, 3)
    out = all_gather_rows(rows)
    assert len(out) == 1 and out[0] is rows


# ------------------------------------------------------------------------------------------------ caption draws
def test_caption_draws_replay_the_reference_stream(tmp_path):
    """One torch.randint per sample in batch order, then the tokenizer's crop draws (one per over-long caption, in order)."""
    from divergen_amd.modeling.meta_arch.custom_rcnn import CustomRCNN
    from divergen_amd.modeling.text import CLIPTEXT
    _, bpe = F.write_text_encoder(tmp_path)
    enc = CLIPTEXT(embed_dim=8, context_length=8, vocab_size=520, transformer_width=64, transformer_heads=1, transformer_layers=1, bpe_path=bpe)
    long_ = "newer newer newer newer newer newer newer newer newer low"
    batch = [{"captions": ["low", "lower low", long_]}, {"captions": [long_]}, {"captions": ["low lower", long_, "newer", "low"]}]
    log = {}

    class Spy:
        embed_dim = 8

        def __call__(self, caps):
            log["caps"], log["tokens"] = list(caps), enc.tokenize(caps, 8)
            return torch.zeros(len(caps), 8)
    me = types.SimpleNamespace(with_caption=True, sync_caption_batch=False, text_encoder=Spy())
    for seed in (0, 1, 2, 3):
        torch.manual_seed(seed)
        feats = CustomRCNN._caption_features(me, batch, "captiontag")
        torch.manual_seed(seed)
        inds = [torch.randint(len(x["captions"]), (1,))[0].item() for x in batch]
        caps = [x["captions"][i] for i, x in zip(inds, batch)]
        assert log["caps"] == caps and feats.shape == (3, 8) and feats.dtype == torch.float32
        assert torch.equal(log["tokens"], enc.tokenize(caps, 8))         # the crop draws come right after the caption draws
    assert CustomRCNN._caption_features(me, batch, "image") is None
    with pytest.raises(KeyError, match="captions"):
        CustomRCNN._caption_features(me, [{"captions": []}], "caption")


# ------------------------------------------------------------------------------------------------ restatement against the reference
def _restate(gold, name):
    d = C.golden_inputs()
    B, D = d["B"], d["D"]
    sync = name == "synced"
    cap = gold["in.gathered"] if sync else d["cap"]
    scale, stat = C.scales(B)
    kw = dict(u=gold[("caption" if name == "captiontag" else name) + ".u"], valid=None, counts=d["counts"], cap=cap, D=D,
              target0=B * d["rank"] if sync else 0, temp=C.TEMP, norm_weight=True, bias=d["use_bias"],
              neg_weight=C.NEG_CAP_WEIGHT if sync else 1.0, scale=scale, stat_scale=stat)
    return d, kw, C.caption_loss(**kw)


def _inside(got, ref, floor):
    return C.worst_ratio(got, ref, floor, RTOL) <= 1.0


@pytest.mark.parametrize("name", ["caption", "synced"])
def test_restatement_against_the_reference(name, gold):
    """image_loss, stats_l_caption, the gradients of u and cls_bias, and -- carried through u = linear(x) in float64 -- the gradients of
    x and cls_score.linear.*; the image without proposals contributes nothing and counts in B; each deliberate mistake falls outside."""
    d, kw, r = _restate(gold, name)
    assert r["sel"] == [4, 2, -1, 5]
    assert _inside(gold[name + ".image_loss"], r["loss"], r["floor_loss"])
    assert _inside(gold[name + ".l_caption"], r["l_caption"], r["floor_loss"] / C.IMAGE_LOSS_WEIGHT)
    assert float(gold[name + ".l_image"]) == 0.0 and all(float(gold[name + ".stat." + k]) == 0.0 for k in (
        "pool_stats", "stats_select_size", "stats_select_x", "stats_select_y", "stats_max_label_score"))
    assert _inside(gold[name + ".du"], r["du"], r["floor_du"])
    assert _inside(gold[name + ".dbias"], r["dbias"], r["floor_dbias"])
    W, x = d["lin_w"].astype(np.float64), d["x"].astype(np.float64)
    assert _inside(gold[name + ".dx"], r["du"] @ W, r["floor_du"] @ np.abs(W))
    assert _inside(gold[name + ".dlin_w"], r["du"].T @ x, r["floor_du"].T @ np.abs(x))
    assert _inside(gold[name + ".dlin_b"], r["du"].sum(0), r["floor_du"].sum(0))
    for mutant in C.MUTANTS:
        if mutant in ("no_neg_weight", "target_unsynced") and name != "synced":
            continue
        m = C.caption_loss(mutant=mutant, **kw)
        assert not (_inside(gold[name + ".image_loss"], m["loss"], m["floor_loss"]) and _inside(gold[name + ".du"], m["du"], m["floor_du"])), mutant


def test_restatement_against_the_reference_captiontag(gold):
    """'captiontag': image_loss and the gradient of u are the caption part plus the image-label part ('image' on the same rows)."""
    d, kw, r = _restate(gold, "captiontag")
    img_loss, img_du = float(gold["image.image_loss"]), gold["image.du"].astype(np.float64)
    assert img_loss > 0 and np.abs(img_du).max() > 0
    assert _inside(gold["captiontag.image_loss"], r["loss"] + img_loss, r["floor_loss"] + img_loss)
    assert _inside(gold["captiontag.l_caption"], r["l_caption"], r["floor_loss"] / C.IMAGE_LOSS_WEIGHT)
    assert abs(float(gold["captiontag.l_image"]) * C.IMAGE_LOSS_WEIGHT - img_loss) <= RTOL * img_loss
    assert _inside(gold["captiontag.du"], r["du"] + img_du, r["floor_du"] + np.abs(img_du))
    assert _inside(gold["captiontag.dbias"], r["dbias"] + float(gold["image.dbias"].reshape(-1)[0]),
                   r["floor_dbias"] + abs(float(gold["image.dbias"].reshape(-1)[0])))


def test_measured_bound_and_bf16_figure(gold):
    """The reference's own fp32 evaluation lies inside rtol 1e-5 on the golden and on the GPU tests' inputs: the tests' rtol is 1e-5.  The
    bf16 figure of the README is the one the generator recorded."""
    assert gold["measured.golden"].max() <= 1.0 and gold["measured.cases"].max() <= 1.0
    assert 0 < float(gold["measured.bf16_u"]) < 3e-3


# ------------------------------------------------------------------------------------------------ predictor forward
def _predictor(gold, tmp_path, sync):
    from divergen_amd.modeling import ShapeSpec
    from divergen_amd.modeling.box_regression import Box2BoxTransform
    from divergen_amd.modeling.roi_heads.detic_fast_rcnn import DeticFastRCNNOutputLayers
    from divergen_amd.modeling.roi_heads.zero_shot_classifier import ZeroShotClassifier
    d = C.golden_inputs()
    npy = os.path.join(str(tmp_path), "zs.npy")
    np.save(npy, d["zs"])
    cls = ZeroShotClassifier(ShapeSpec(channels=d["Cin"]), num_classes=d["C"], zs_weight_path=npy, zs_weight_dim=d["D"], use_bias=d["use_bias"],
                             norm_weight=True, norm_temperature=C.TEMP)
    pred = DeticFastRCNNOutputLayers(ShapeSpec(channels=d["Cin"]), box2box_transform=Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0)),
                                     num_classes=d["C"], cls_agnostic_bbox_reg=True, smooth_l1_beta=0.0, use_sigmoid_ce=True, use_zeroshot_cls=True,
                                     cls_score=cls, image_label_loss="max_size", add_image_box=True, with_caption=True,
                                     caption_weight=C.CAPTION_WEIGHT, neg_cap_weight=C.NEG_CAP_WEIGHT, sync_caption_batch=sync)
    sd = {k[len("param."):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("param.")}
    assert sorted(sd) == sorted(pred.state_dict())
    pred.load_state_dict(sd)
    return d, pred


@pytest.mark.parametrize("sync", [False, True], ids=["plain", "synced"])
def test_predictor_forward_with_caption_features_equals_the_reference(sync, gold, tmp_path):
    d, pred = _predictor(gold, tmp_path, sync)
    name = "synced" if sync else "caption"
    cap = torch.from_numpy(gold["in.gathered"] if sync else d["cap"])
    x = torch.from_numpy(d["x"])
    with torch.no_grad():
        scores, deltas = pred(x, (None, None, cap))
    ref = gold[name + ".scores"]
    assert scores.shape == ref.shape == (14, d["C"] + 1 + cap.shape[0])
    assert np.abs(scores.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.abs(deltas.numpy() - gold[name + ".deltas"]).max() <= 1e-5 * np.abs(gold[name + ".deltas"]).max()
    assert torch.equal(pred(x)[0], scores[:, :d["C"] + 1])
    plain = type(pred)(d_shape(d), box2box_transform=pred.box2box_transform, num_classes=d["C"], cls_agnostic_bbox_reg=True, use_sigmoid_ce=True,
                       use_zeroshot_cls=True, cls_score=pred.cls_score)
    with pytest.raises(NotImplementedError, match="WITH_CAPTION"):      # a predictor built without the feature refuses as before
        plain(x, (None, None, cap))


def d_shape(d):
    from divergen_amd.modeling import ShapeSpec
    return ShapeSpec(channels=d["Cin"])


def test_zero_shot_forward_is_the_composition_of_its_halves(gold, tmp_path):
    import torch.nn.functional as Fn
    d, pred = _predictor(gold, tmp_path, False)
    cs = pred.cls_score
    x = torch.from_numpy(d["x"])
    cap = torch.from_numpy(d["cap"])
    with torch.no_grad():
        for classifier in (None, cap):
            u = cs.project(x)
            assert torch.equal(cs(x, classifier), cs.score(u, classifier))
            # what forward computed before it was split, op for op
            h = Fn.linear(x, cs.linear.weight, cs.linear.bias)
            zs = cs.zs_weight if classifier is None else Fn.normalize(classifier.permute(1, 0).contiguous(), p=2, dim=0)
            y = torch.mm(cs.norm_temperature * Fn.normalize(h, p=2, dim=1), zs) + cs.cls_bias
            assert torch.equal(u, h) and torch.equal(cs(x, classifier), y)


# ------------------------------------------------------------------------------------------------ model state and ABI
def test_model_owns_a_frozen_text_encoder(tmp_path, monkeypatch):
    """State-dict names of a model built with WITH_CAPTION: the old keys plus text_encoder.*; every text_encoder parameter frozen and
    absent from the solver's parameter list; the embed dim is checked at start-up."""
    from divergen_amd.modeling import build_model
    from divergen_amd.solver import FlatArena
    cfg, _, _ = F.two_source_cfg(tmp_path, monkeypatch, extra=["MODEL.DEVICE", "cpu"], num_classes=37)
    torch.manual_seed(0)
    model = build_model(cfg)
    cfg0 = cfg.clone()
    cfg0.defrost()
    cfg0.merge_from_list(["MODEL.CAPTION_TRAIN", False, "MODEL.WITH_CAPTION", False, "DATALOADER.DATASET_ANN", ["box", "image"]])
    torch.manual_seed(0)
    old = build_model(cfg0)
    names, old_names = set(model.state_dict()), set(old.state_dict())
    enc = {n for n in names if n.startswith("text_encoder.")}
    assert names - enc == old_names and not any(n.startswith("text_encoder.") for n in old_names)
    sd, sd0 = model.state_dict(), old.state_dict()
    assert all(torch.equal(sd[n], sd0[n]) for n in old_names), "the encoder's construction moved the model's initial values"
    assert {n[len("text_encoder."):] for n in enc} == set(torch.load(cfg.MODEL.TEXT_ENCODER_WEIGHTS))
    assert model.text_encoder.transformer.layers == 2 and model.text_encoder.embed_dim == 512
    assert all(not p.requires_grad for p in model.text_encoder.parameters())
    arena = FlatArena(model)
    assert not any(n.startswith("text_encoder.") for n in arena.names) and set(arena.names) == set(FlatArena(old).names)
    assert model._annotation_type([{"ann_type": "caption", "pos_category_ids": []}], [types.SimpleNamespace()]) == "caption"
    with pytest.raises(NotImplementedError, match="ann_type"):
        old._annotation_type([{"ann_type": "caption", "pos_category_ids": []}], [types.SimpleNamespace()])
    weights, bpe = F.write_text_encoder(tmp_path / "narrow", embed_dim=24)
    cfg.merge_from_list(["MODEL.TEXT_ENCODER_WEIGHTS", weights])
    with pytest.raises(ValueError, match="ZEROSHOT_WEIGHT_DIM"):
        build_model(cfg)


def test_new_symbols_everywhere():
    from divergen_amd import _lib
    from divergen_amd.csrc.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "divergen_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "caption_loss.hip" in SOURCES
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(L, s) and s + "(" in hdr and s in integ, s


def test_refused_calls_return_minus_one_without_a_gpu():
    """The argument checks run before any launch and before any pointer is followed: B > 32, D not a multiple of 8 or outside 8..4096,
    target0 + B > N, a NULL pointer."""
    import ctypes
    from divergen_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=2, D=16, N=4, target0=0, u=p, cap=p, sel=p, ws=p, out=p):
        row0 = (ctypes.c_int * (B + 1))(*range(B + 1))
        return L.dgx_caption_loss(u, 16, 40, None, B, row0, cap, N, D, target0, 50.0, 1, None, 1.0, 1.0, 1.0, None, sel, out, ws, None, 0, None, 0, None)
    for kw in (dict(B=33), dict(B=0), dict(D=12), dict(D=0), dict(D=4104), dict(target0=3), dict(target0=-1), dict(N=0), dict(u=None),
               dict(cap=None), dict(sel=None), dict(ws=None), dict(out=None)):
        assert call(**kw) == -1, kw
    assert L.dgx_caption_prepare(None, 16, 4, 16, 1, p, None) == -1
    assert L.dgx_caption_prepare(p, 16, 4, 12, 1, p, None) == -1
    assert L.dgx_caption_prepare(p, 8, 4, 16, 1, p, None) == -1          # rows shorter than D
    assert L.dgx_caption_workspace_floats(0, 4) == 0 and L.dgx_caption_workspace_floats(2, 4) == 2 * 4 + 2 * 2 + 2 + 1
