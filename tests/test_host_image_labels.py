"""Host-side tests of image-label co-training (WITH_IMAGE_LABELS): the float64 restatement against the reference's own outputs
(tests/golden/image_labels.npz), the multi-dataset sampler and its grouped batches, the mapper's fields, the start-up refusals, the
reducer's ready-count vectors when ranks take different annotation types.  (That both step types report the same loss keys needs
the model's kernels: tests/test_gpu_image_labels.py checks it on the assembled model.)"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _image_label_ref as Z  # noqa: E402


def close(a, b, rtol=1e-5):
    return abs(float(a) - float(b)) <= rtol * abs(float(b))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("mode", Z.MODES)
def test_restatement_against_reference_losses(mode, golden):
    """float64 restatement vs the reference's image_label_losses: values to 1e-5 relative (the project's bound for float goldens),
    selected rows equal."""
    g, d = golden("image_labels"), Z.inputs()
    r = Z.image_label_loss(d["scores"], None, d["boxes"], Z.COUNTS, Z.IMAGE_SIZES, Z.LABELS, mode, Z.WEIGHT)
    assert r["sel"] == g[mode + ".sel"].tolist()
    assert close(r["loss"], g[mode + ".loss"]) and close(r["l_image"], g[mode + ".l_image"])
    np.testing.assert_allclose(r["stats"], g[mode + ".stats"], rtol=1e-5, atol=1e-7)
    rows = np.nonzero(np.abs(r["grad"]).sum(1))[0]
    assert rows.tolist() == g[mode + ".grad_rows"].tolist()
    # the golden gradient is fp32: where several labels share a row it sums terms of magnitude up to weight / (B L) that may cancel
    ref = g[mode + ".grad"].astype(np.float64)
    image_of = np.repeat(np.arange(len(Z.COUNTS)), Z.COUNTS)[rows]
    coef = np.array([Z.WEIGHT / (len(Z.COUNTS) * max(len(Z.LABELS[i]), 1)) for i in image_of])
    assert np.all(np.abs(r["grad"][rows] - ref) <= 1e-5 * np.maximum(np.abs(ref), coef[:, None]))


def test_restatement_against_reference_proposals_and_handover(golden):
    g, d = golden("image_labels"), Z.inputs()
    for add, tag in ((False, "ws."), (True, "ws_box.")):
        b, l, v = Z.ws_proposals(d["ws_boxes"], d["ws_scores"], d["ws_valid"], Z.IMAGE_SIZES[:3], Z.WS_NUM_PROPS, add, Z.IMAGE_BOX_SIZE)
        keep = v.astype(bool)
        Ko = Z.WS_NUM_PROPS + int(add)
        assert keep.reshape(3, Ko).sum(1).tolist() == g[tag + "counts"].tolist()
        np.testing.assert_allclose(b[keep], g[tag + "boxes"], rtol=1e-5, atol=1e-5)
        assert np.array_equal(l[keep], g[tag + "logits"])
        assert not b[~keep].any() and not l[~keep].any()
    rb, rv = d["boxes"], None
    for k in range(2):
        rb, rv = Z.refine(rb, d["deltas"][k], rv, Z.COUNTS, Z.IMAGE_SIZES, Z.BOX_WEIGHTS[k])
        alive = np.nonzero(rv)[0]
        assert alive.tolist() == g["stage%d.rows" % (k + 1)].tolist()
        np.testing.assert_allclose(rb[alive], g["stage%d.boxes" % (k + 1)], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ sampler, batches
SAMPLER_CASES = [((60, 35), ("box", "image"), (1, 1), (False, False), 0.001, 11),
                 ((60, 35), ("box", "image"), (1, 4), (True, True), 0.05, 12),
                 ((40, 25, 50), ("box", "image", "image"), (2, 1, 1), (True, False, True), 0.05, 13)]
DIFF_BS = {2: [2, 4], 3: [2, 4, 3]}


@pytest.mark.parametrize("ci", range(3))
def test_multi_dataset_sampler_and_grouped_batches_equal_reference(ci, golden):
    """Index streams of the reference's MultiDatasetSampler (ranks 0 and 1 of 2) and the batches its two grouped datasets form from
    them: equal, index by index and batch by batch."""
    import itertools
    from divergen_amd.data.samplers import GroupedBatchSampler, MultiDatasetSampler
    g = golden("image_labels")
    sizes, ann, ratio, rfs, thr, seed = SAMPLER_CASES[ci]
    dicts = Z.dataset_dicts(sizes, ann, seed=seed)
    for rank in (0, 1):
        s = MultiDatasetSampler(dicts, list(ratio), list(rfs), list(ann), thr, seed=seed, rank=rank, world_size=2)
        np.testing.assert_allclose(s.weights.numpy(), g["sampler%d.weights" % ci], rtol=1e-6)
        want = g["sampler%d.rank%d" % (ci, rank)].tolist()
        assert list(itertools.islice(iter(s), len(want))) == want
        for tag, bs in (("md", [3]), ("diff", DIFF_BS[len(sizes)])):
            lens = g["sampler%d.rank%d.%s.len" % (ci, rank, tag)].tolist()
            ids = g["sampler%d.rank%d.%s.ids" % (ci, rank, tag)].tolist()
            got = list(GroupedBatchSampler(want, dicts, bs))
            assert [len(b) for b in got] == lens
            assert [dicts[i]["image_id"] for b in got for i in b] == ids
            for b in got:
                assert len({dicts[i]["dataset_source"] for b_ in [b] for i in b_}) == 1
                assert len({dicts[i]["width"] > dicts[i]["height"] for i in b}) == 1


def test_tag_frequency_repeat_factors_equal_reference(golden):
    from divergen_amd.data.samplers import repeat_factors_from_tag_frequency
    rf = repeat_factors_from_tag_frequency(Z.dataset_dicts((80,), ("image",), seed=21), 0.05)
    assert np.array_equal(rf.numpy(), golden("image_labels")["tag_rfs"])


# ------------------------------------------------------------------------------------------------ mapper, loader
def _two_source_cfg(tmp_path, monkeypatch, extra=()):
    from divergen_amd.data import build as B
    from divergen_amd.data.synthetic import write_mini_image_labels
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 128, 0, ["WITH_IMAGE_LABELS", True, "DATALOADER.SAMPLER_TRAIN", "MultiDatasetSampler",
                                             "DATALOADER.MULTI_DATASET_GROUPING", True, "DATALOADER.FILTER_EMPTY_ANNOTATIONS", False,
                                             "DATALOADER.DATASET_ANN", ["box", "image"], "DATALOADER.DATASET_RATIO", [1, 1],
                                             "DATALOADER.USE_RFS", [True, False], "DATASETS.TRAIN", ("lvis_v1_train", "imagenet_lvis_mini"),
                                             "MODEL.ROI_BOX_HEAD.WS_NUM_PROPS", 32] + list(extra))
    il = write_mini_image_labels(info["root"], n_images=8, seed=3)
    B.register_lvis_instances("imagenet_lvis_mini", il["json"], il["image_root"])
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    return cfg, info


def test_mapper_fields_and_no_copy_paste_draw_for_image_samples(tmp_path, monkeypatch):
    """`ann_type` / `pos_category_ids` / `dataset_source` on every sample as plain keys; per-source EfficientDetResizeCrop with
    USE_DIFF_BS_SIZE; an image-labelled sample leaves CopyPasteMapper before any np.random draw of its own and carries empty
    instances; FILTER_EMPTY_ANNOTATIONS is refused by name with an image source."""
    from divergen_amd.data import build as B
    cfg, info = _two_source_cfg(tmp_path, monkeypatch, ["DATALOADER.USE_DIFF_BS_SIZE", True, "DATALOADER.DATASET_BS", [2, 4],
                                                        "DATALOADER.DATASET_INPUT_SIZE", [128, 64], "DATALOADER.DATASET_INPUT_SCALE", [[0.9, 1.5], [0.8, 1.2]]])
    dicts = B.get_detection_dataset_dicts_with_source(cfg.DATASETS.TRAIN, filter_empty=False, dataset_ann=cfg.DATALOADER.DATASET_ANN)
    assert [d["dataset_source"] for d in dicts] == [0] * 12 + [1] * 8
    with pytest.raises(ValueError, match="FILTER_EMPTY_ANNOTATIONS"):
        B.get_detection_dataset_dicts_with_source(cfg.DATASETS.TRAIN, filter_empty=True, dataset_ann=cfg.DATALOADER.DATASET_ANN)
    plain = B.DatasetMapper(cfg, True)
    mapper = B.CopyPasteMapper(plain, cfg)
    mapper.set_dataset(dicts)
    mapper.pack = False
    img = dicts[14]
    np.random.seed(5)
    want = plain(img)
    state = np.random.get_state()
    np.random.seed(5)
    got = mapper(img)
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(state, after)), "an image-labelled sample made a copy-paste draw"
    assert torch.equal(got["image"], want["image"]) and "paste_pack" not in got and "scp_src" not in got and "blob" not in got
    assert got["ann_type"] == "image" and got["dataset_source"] == 1 and got["pos_category_ids"] == img["pos_category_ids"] != []
    assert len(got["instances"]) == 0 and got["instances"].has("gt_masks") and 48 <= max(got["image"].shape[-2:]) <= 64
    np.random.seed(6)
    box = mapper(dicts[2])
    assert box["ann_type"] == "box" and box["dataset_source"] == 0 and box["pos_category_ids"] == [] and 110 <= max(box["image"].shape[-2:]) <= 128
    assert "paste_pack" in box
    packed = B.pack_sample(dict(box))
    assert packed["ann_type"] == "box" and packed["pos_category_ids"] == [] and packed["dataset_source"] == 0


def test_loader_batches_hold_one_source(tmp_path, monkeypatch):
    """build_detection_train_loader with MultiDatasetSampler on the CPU (no workers): every batch has one dataset_source and one
    annotation type, box batches have DATASET_BS[0] = 2 samples, image batches DATASET_BS[1] = 4; both types occur."""
    from divergen_amd.data import build as B
    cfg, info = _two_source_cfg(tmp_path, monkeypatch, ["DATALOADER.USE_DIFF_BS_SIZE", True, "DATALOADER.DATASET_BS", [2, 4],
                                                        "DATALOADER.DATASET_INPUT_SIZE", [128, 64], "DATALOADER.DATASET_INPUT_SCALE", [[0.9, 1.5], [0.8, 1.2]],
                                                        "INPUT.INST_POOL", False])
    it = B.build_detection_train_loader(cfg, 2, "cpu", 3)
    seen = set()
    for _ in range(8):
        batch = next(it)
        kinds = {(d["dataset_source"], d["ann_type"]) for d in batch}
        assert len(kinds) == 1
        (src, ann), = kinds
        assert (src, ann, len(batch)) in ((0, "box", 2), (1, "image", 4))
        seen.add(ann)
    assert seen == {"box", "image"}


# ------------------------------------------------------------------------------------------------ refusals
REFUSALS = [
    (["DATALOADER.DATASET_ANN", ["box", "caption"]], "DATASET_ANN"),
    (["MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsddn"], "IMAGE_LABEL_LOSS"),
    (["MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "wsod"], "IMAGE_LABEL_LOSS"),
    (["MODEL.ROI_BOX_HEAD.IMAGE_LABEL_LOSS", "image"], "ADD_IMAGE_BOX"),
    (["MODEL.ROI_BOX_HEAD.WITH_SOFTMAX_PROP", True], "WITH_SOFTMAX_PROP"),
    (["MODEL.ROI_BOX_HEAD.SOFTMAX_WEAK_LOSS", True], "SOFTMAX_WEAK_LOSS"),
    (["MODEL.ROI_BOX_HEAD.ADD_FEATURE_TO_PROP", True], "ADD_FEATURE_TO_PROP"),
    (["MODEL.WITH_CAPTION", True], "WITH_CAPTION"),
    (["MODEL.DYNAMIC_CLASSIFIER", True], "DYNAMIC_CLASSIFIER"),
    (["MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", False], "USE_SIGMOID_CE"),
    (["INPUT.USE_COPY_METHOD", "self_copy"], "USE_COPY_METHOD"),
    (["INPUT.USE_COPY_METHOD", "p:0.5"], "USE_COPY_METHOD"),
    (["INPUT.ACTIVE_SELECT", True], "ACTIVE_SELECT"),
    (["DATALOADER.USE_TAR_DATASET", True], "USE_TAR_DATASET"),
    (["DATALOADER.USE_DIFF_BS_SIZE", True, "INPUT.CUSTOM_AUG", "ResizeShortestEdge"], "USE_DIFF_BS_SIZE"),
    (["DATALOADER.MULTI_DATASET_GROUPING", False], "MULTI_DATASET_GROUPING"),
    (["DATALOADER.FILTER_EMPTY_ANNOTATIONS", True], "FILTER_EMPTY_ANNOTATIONS"),
    (["DATALOADER.USE_DIFF_BS_SIZE", True, "DATALOADER.DATASET_BS", [2, 33]], "REFINE_MAX_IMAGES"),
    (["DATALOADER.SAMPLER_TRAIN", "TrainingSampler"], "MultiDatasetSampler"),
]


@pytest.mark.parametrize("opts,key", REFUSALS, ids=[r[1] + str(i) for i, r in enumerate(REFUSALS)])
def test_every_refusal_names_its_key(opts, key, tmp_path, monkeypatch):
    from divergen_amd.config.image_labels import check_loader_keys, check_model_keys
    cfg, _ = _two_source_cfg(tmp_path, monkeypatch, opts)
    with pytest.raises((NotImplementedError, ValueError), match=key):
        check_model_keys(cfg)
        check_loader_keys(cfg, 2)


def test_shipped_configuration_passes_the_checks_untouched(tmp_path, monkeypatch):
    from divergen_amd.config.image_labels import check_loader_keys, check_model_keys
    from tests.test_gpu_loader import _mini_cfg
    cfg, _ = _mini_cfg(tmp_path, 128, 0)
    assert not cfg.WITH_IMAGE_LABELS
    check_model_keys(cfg)
    check_loader_keys(cfg, 2)
    good, _ = _two_source_cfg(tmp_path / "b", monkeypatch)
    check_model_keys(good)
    check_loader_keys(good, 2)


def test_names_that_fail_without_the_feature():
    """The sampler name, the ABI symbols and the constructor switch exist."""
    from divergen_amd import _lib
    from divergen_amd.data import samplers
    assert hasattr(samplers, "MultiDatasetSampler") and hasattr(samplers, "GroupedBatchSampler")
    for s in ("dgx_ws_proposals", "dgx_image_label_loss", "dgx_image_label_workspace_floats"):
        assert s in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "divergen_hip.h")).read()
    assert "int dgx_image_label_loss(" in hdr and "int dgx_ws_proposals(" in hdr


# ------------------------------------------------------------------------------------------------ reducer
def _ddp_ann_type_worker(rank, world, port, q, keyed):
    """Ranks on different annotation types in alternating steps: the 'box' branch uses the shared weight twice, the 'image' branch
    once (one ready signal per use)."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from divergen_amd.engine.ddp import ArenaReducer
    from divergen_amd.solver import FlatArena
    from tests.test_host_logic import _direct_linear
    torch.manual_seed(7)
    shared, head = torch.nn.Linear(8, 8, bias=False), torch.nn.Linear(8, 3)
    ar = FlatArena(torch.nn.ModuleList([shared, head]))
    red = ArenaReducer(ar, bucket_bytes=16)
    red.broadcast_parameters()
    x = torch.full((4, 8), 0.25 * (rank + 1))
    out, err = [], None
    try:
        for it in range(6):
            kind = "box" if (it + rank) % 2 == 0 else "image"
            if keyed:
                red.step_kind = kind
            ar.zero_grad()
            h = _direct_linear(x, shared.weight)
            if kind == "box":
                h = _direct_linear(torch.relu(h), shared.weight)
            head(h).sum().backward()
            scale = red.finish()
            out.append((ar.g.clone() * scale).numpy().copy())
    except RuntimeError as e:
        err = str(e)
    q.put((rank, out, err, sorted(str(k) for k in red._learned)))
    if err is None:
        dist.destroy_process_group()


def _run_world2(keyed):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ddp_ann_type_worker, args=(r, 2, port, q, keyed)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(30)
        if p.is_alive():
            p.terminate()
    return res


def test_reducer_keys_its_ready_counts_by_annotation_type_world2_gloo():
    """With the step's annotation type announced both ranks reduce to identical gradients in every step and learn one vector per
    type; without it the vector learned on the 'image' branch is held against the 'box' branch and finish() raises."""
    (_, g0, e0, k0), (_, g1, e1, k1) = _run_world2(True)
    assert e0 is None and e1 is None and len(g0) == 6
    for a, b in zip(g0, g1):
        assert np.array_equal(a, b) and np.abs(a).sum() > 0
    assert len(k0) == 2 and all("ann_type" in k for k in k0) and k0 == k1
    res = _run_world2(False)
    assert any(e is not None and "more often than in the first step" in e for _, _, e, _ in res)
