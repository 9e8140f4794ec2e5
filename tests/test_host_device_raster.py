"""INPUT.DEVICE_RASTER, host side (no GPU): emptiness decided from the crossings, the key-on mapper against the key-off mapper on the
same seeded samples, the start-up refusals, and the fill rule of dgx_polygons_to_bitmask (tests/_raster_ref.py) against the host
rasteriser it must match.  The reference everywhere is data/build.py:polygons_to_bitmask, pinned by tests/test_host_data.py."""
import numpy as np
import pytest
import torch

from tests._raster_ref import CANVASES, fill_model, polygon_set, sorted_crossings

BRANCHES = ("outside", "clip_left", "clip_top", "clip_right", "clip_bottom", "collinear", "subpixel", "odd", "duplicate", "carry")


@pytest.fixture(scope="module")
def polys():
    from divergen_amd.data.build import polygons_to_bitmask
    return [(H, W, p, tags, sorted_crossings(p, H, W), polygons_to_bitmask([p], H, W)) for H, W, p, tags in polygon_set()]


def test_polygon_set_covers_every_branch(polys):
    assert len(polys) >= 2000 and {(H, W) for H, W, *_ in polys} == set(CANVASES)
    seen = set().union(*[tags for _, _, _, tags, _, _ in polys])
    assert set(BRANCHES) <= seen, sorted(set(BRANCHES) - seen)
    # the tags say what they are meant to say: an odd list leaves the last pixel of the canvas set, an outside polygon leaves nothing
    for H, W, _, tags, pos, ref in polys:
        assert ("odd" in tags) == bool(pos.size & 1) == bool(ref[H - 1, W - 1] and pos.size & 1)
        if "outside" in tags:
            assert not ref.any()
        assert pos.dtype == np.int32 and (np.diff(pos) >= 0).all() and (pos.size == 0 or (0 <= pos[0] and pos[-1] < H * W))


def test_emptiness_from_crossings_equals_mask_any(polys):
    from divergen_amd.structures import PolygonCrossings, crossings_nonempty
    n_empty = 0
    for H, W, _, _, pos, ref in polys:
        assert crossings_nonempty(pos) == bool(ref.any())
        n_empty += not ref.any()
    assert 100 < n_empty < len(polys) - 100
    # an instance is non-empty iff one of its polygons is; filter_empty_instances reads exactly this
    for H, W in CANVASES:
        group = [(pos, ref) for h, w, _, _, pos, ref in polys if (h, w) == (H, W)]
        inst = [group[i:i + 3] for i in range(0, len(group) - 2, 3)] + [[]]
        pc = PolygonCrossings.from_lists([[pos for pos, _ in g] for g in inst], (H, W))
        want = [any(bool(ref.any()) for _, ref in g) for g in inst]
        assert pc.nonempty().tolist() == want and len(pc) == len(inst)


def test_fill_model_equals_host_rasteriser(polys):
    from divergen_amd.data.build import polygons_to_bitmask
    for H, W, _, _, pos, ref in polys:
        assert np.array_equal(fill_model([pos], H, W), ref)
    # OR over the polygons of one instance, never XOR: overlapping polygons
    H, W = 37, 70
    group = [(p, pos) for h, w, p, tags, pos, ref in polys if (h, w) == (H, W) and ref.sum() > 200][:6]
    assert len(group) == 6
    both = polygons_to_bitmask([p for p, _ in group], H, W)
    assert np.array_equal(fill_model([pos for _, pos in group], H, W), both)
    xor = np.zeros((H, W), bool)
    for _, pos in group:
        xor ^= fill_model([pos], H, W)
    assert not np.array_equal(xor, both)


def test_polygon_crossings_indexing_keeps_instances():
    from divergen_amd.structures import Boxes, Instances, PolygonCrossings
    a, b, c = np.array([1, 4], np.int32), np.array([2, 2, 7], np.int32), np.array([], np.int32)
    pc = PolygonCrossings.from_lists([[a], [], [b, c], [c]], (3, 4))
    assert len(pc) == 4 and pc.inst_off.tolist() == [0, 1, 1, 3, 4] and pc.poly_off.tolist() == [0, 2, 5, 5, 5]
    assert pc.nonempty().tolist() == [True, False, True, False]
    inst = Instances((3, 4), gt_boxes=Boxes(torch.zeros(4, 4)), gt_classes=torch.arange(4), gt_masks=pc)
    kept = inst[torch.tensor([True, False, True, False])]
    assert kept.gt_classes.tolist() == [0, 2] and len(kept.gt_masks) == 2
    assert [[p.tolist() for p in kept.gt_masks.polygons(i)] for i in range(2)] == [[[1, 4]], [[2, 2, 7], []]]
    assert len(inst[1].gt_masks) == 1 and inst[1].gt_masks.polygons(0) == [] and len(inst[1:3].gt_masks) == 2
    assert len(inst[torch.tensor([3, 0])].gt_masks.polygons(1)[0]) == 2
    with pytest.raises(ValueError):
        PolygonCrossings(a, np.array([0, 3]), np.array([0, 1]), (3, 4))


def _mapper(cfg, dicts):
    from divergen_amd.data import build as B
    m = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    m.set_dataset(dicts)
    return m


def test_same_sample_key_off_and_on(tmp_path, monkeypatch):
    """The same seeded samples through CopyPasteMapper ('syn_copy', packed) with the key off and on: the same instances kept, the same
    boxes and classes, the same np.random state afterwards; the key-on blob carries poly_pos / poly_off / inst_off and no gt_masks,
    is smaller, and its crossings fill (on the host) to exactly the key-off masks."""
    from divergen_amd.data import build as B
    from divergen_amd.structures import PolygonCrossings
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 128, 0)
    on = cfg.clone()
    on.merge_from_list(["INPUT.DEVICE_RASTER", True])
    assert cfg.INPUT.DEVICE_RASTER is False
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN)
    m_off, m_on = _mapper(cfg, dicts), _mapper(on, dicts)
    n_inst = 0
    for i, d in enumerate(dicts[:6]):
        outs = []
        for m in (m_off, m_on):
            np.random.seed(100 + i)
            m.inst_pool.seed(100 + i)
            packed = m(d)
            outs.append((packed, np.random.get_state()))
        (p_off, s_off), (p_on, s_on) = outs
        assert all(np.array_equal(a, b) for a, b in zip(s_off, s_on)), "the key changed the np.random consumption"
        names_off, names_on = [x[0] for x in p_off["blob_layout"]], [x[0] for x in p_on["blob_layout"]]
        assert names_off == ["image", "gt_masks", "gt_boxes", "gt_classes", "flat", "desc", "labels"]
        assert names_on == ["image", "poly_pos", "poly_off", "inst_off", "gt_boxes", "gt_classes", "flat", "desc", "labels"]
        assert p_on["blob"].numel() < p_off["blob"].numel()
        u_off, u_on = B.unpack_sample(dict(p_off), "cpu"), B.unpack_sample(dict(p_on), "cpu")
        assert torch.equal(u_off["image"], u_on["image"])
        i_off, i_on = u_off["instances"], u_on["instances"]
        assert len(i_off) == len(i_on) and torch.equal(i_off.gt_boxes.tensor, i_on.gt_boxes.tensor) and torch.equal(i_off.gt_classes, i_on.gt_classes)
        for k in ("flat", "desc", "labels"):
            assert torch.equal(u_off["paste_pack"][k], u_on["paste_pack"][k])
        pc = i_on.gt_masks
        assert isinstance(pc, PolygonCrossings) and pc.image_size == tuple(i_off.gt_masks.tensor.shape[1:])
        H, W = pc.image_size
        for j in range(len(pc)):
            assert np.array_equal(fill_model(pc.polygons(j), H, W), i_off.gt_masks.tensor[j].numpy())
        n_inst += len(pc)
        with pytest.raises(RuntimeError, match="DEVICE_RASTER"):       # no host fill behind the key
            m_on.finish(dict(p_on), "cpu")
    assert n_inst >= 10


def test_key_on_filters_like_key_off_and_passes_image_samples(tmp_path, monkeypatch):
    """USE_COPY_METHOD 'none' (samples are not packed): an instance whose polygon lies outside the crop is dropped with the key on as
    with it off; an image-labelled sample carries its empty BitMasks as before."""
    from divergen_amd.data import build as B
    from divergen_amd.structures import BitMasks, PolygonCrossings
    from tests.test_host_image_labels import _two_source_cfg
    cfg, info = _two_source_cfg(tmp_path, monkeypatch, ["INPUT.USE_COPY_METHOD", "none", "INPUT.INST_POOL", False, "INPUT.SCALE_RANGE", [1.6, 2.0]])
    on = cfg.clone()
    on.merge_from_list(["INPUT.DEVICE_RASTER", True])
    dicts = B.get_detection_dataset_dicts_with_source(cfg.DATASETS.TRAIN, filter_empty=False, dataset_ann=cfg.DATALOADER.DATASET_ANN)
    m_off, m_on = _mapper(cfg, dicts), _mapper(on, dicts)
    dropped = 0
    for i, d in enumerate(dicts):
        np.random.seed(7 + i)
        a = m_off(d)
        s_a = np.random.get_state()
        np.random.seed(7 + i)
        b = m_on(d)
        assert all(np.array_equal(x, y) for x, y in zip(s_a, np.random.get_state()))
        ia, ib = a["instances"], b["instances"]
        assert torch.equal(ia.gt_boxes.tensor, ib.gt_boxes.tensor) and torch.equal(ia.gt_classes, ib.gt_classes) and "blob" not in b
        if d["dataset_source"] == 1:
            assert b["ann_type"] == "image" and isinstance(ib.gt_masks, BitMasks) and len(ib) == 0
        else:
            assert isinstance(ib.gt_masks, PolygonCrossings) and len(ib.gt_masks) == len(ia)
            dropped += len(d["annotations"]) - len(ia)
    assert dropped > 0


def test_refusals_name_their_key(tmp_path, monkeypatch):
    from divergen_amd.data import build as B
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 64, 0)
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])

    def build(*extra):
        c = cfg.clone()
        c.merge_from_list(list(extra))
        return B.CopyPasteMapper(B.DatasetMapper(c, True), c)
    for method in ("self_copy", "both", "p:0.5"):
        assert build("INPUT.USE_COPY_METHOD", method).self_prob is not None               # accepted with the key off, as before
        with pytest.raises(NotImplementedError, match=r"INPUT\.DEVICE_RASTER.*INPUT\.USE_COPY_METHOD '%s'" % method):
            build("INPUT.USE_COPY_METHOD", method, "INPUT.DEVICE_RASTER", True)
    assert build("INPUT.ACTIVE_SELECT", True).active_select
    with pytest.raises(NotImplementedError, match=r"INPUT\.DEVICE_RASTER.*INPUT\.ACTIVE_SELECT"):
        build("INPUT.ACTIVE_SELECT", True, "INPUT.DEVICE_RASTER", True)
    for method in ("none", "syn_copy"):
        m = build("INPUT.USE_COPY_METHOD", method, "INPUT.DEVICE_RASTER", True, "INPUT.SCP_SRC_MODES", True, "INPUT.RM_BG_PROB", 0.5)
        assert m.device_raster and m.mapper.device_raster and m.rm_bg_prob == 0.5
    c = cfg.clone()
    c.merge_from_list(["INPUT.DEVICE_RASTER", True])
    assert B.DatasetMapper(c, True).device_raster and not B.DatasetMapper(c, False).device_raster      # evaluation maps no annotations
    # the fill is a GPU kernel: a CPU loader refuses the key at start-up and still builds without it
    c = cfg.clone()
    c.merge_from_list(["INPUT.INST_POOL", False, "INPUT.USE_COPY_METHOD", "none"])
    assert len(next(B.build_detection_train_loader(c, 2, "cpu", 3))) == 2
    c.merge_from_list(["INPUT.DEVICE_RASTER", True])
    with pytest.raises(NotImplementedError, match=r"INPUT\.DEVICE_RASTER"):
        B.build_detection_train_loader(c, 2, "cpu", 3)


def test_ring_slot_without_mask_planes():
    """The slot of the page-locked ring: unchanged with the key off (48 planes + 8 MB, 48 more per self-copy source); with the key on
    the image planes, the same 8 MB and the stated allowance for crossings, never more than the slot without the key."""
    from divergen_amd.data import build as B
    assert B.ring_slot_bytes(1024) == 1024 * 1024 * 48 + (8 << 20) and B.ring_slot_bytes(640, 2) == 640 * 640 * 144 + (8 << 20)
    assert B.ring_slot_bytes(1024, 0, True) == 1024 * 1024 * 3 + (8 << 20) + B.DEVICE_RASTER_CROSSING_BYTES < B.ring_slot_bytes(1024) // 3
    assert B.ring_slot_bytes(128, 0, True) == B.ring_slot_bytes(128)


def test_abi_declared_bound_and_built():
    import os
    from divergen_amd import _lib
    from divergen_amd.csrc.build import SOURCES
    from divergen_amd.layers import raster_ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "divergen_hip.h")).read()
    assert "int dgx_polygons_to_bitmask(" in hdr and "dgx_polygons_to_bitmask" in _lib.SIGNATURES and "polygon_raster.hip" in SOURCES
    assert "dgx_polygons_to_bitmask" in open(os.path.join(root, "INTEGRATION.md")).read()
    with pytest.raises(_lib.DgxError):                                     # no CPU fallback
        raster_ops.polygons_to_bitmask(torch.zeros(2, dtype=torch.int32), np.array([0, 2]), np.array([0, 1]), 5, 6)
