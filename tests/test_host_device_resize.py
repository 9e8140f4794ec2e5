"""INPUT.DEVICE_RESIZE, host side (no GPU): the numpy model of Pillow's 8-bit BILINEAR resize (tests/_pil_resize_ref.py) against the
installed Pillow, the product's coefficient tables against the model's, the key-on mapper against the key-off mapper on the same
seeded samples, the blob round trip, the start-up refusals and the ring slot.  Every comparison is on all bytes, no tolerance."""
import numpy as np
import pytest
import torch

from tests import _pil_resize_ref as M


def _pillow(img, out_h, out_w):
    from PIL import Image
    return np.asarray(Image.fromarray(img, "RGB" if img.shape[2] == 3 else "RGBA").resize((out_w, out_h), Image.BILINEAR))


def _random_case(rng, C, alpha):
    h, w, th, tw = (int(v) for v in rng.integers(1, 151, 4))
    img = rng.integers(0, 256, (h, w, C), dtype=np.uint8)
    if C == 4 and alpha == "binary":
        img[..., 3] = rng.choice(np.array([0, 255], dtype=np.uint8), (h, w))
    return img, th, tw


def test_model_equals_installed_pillow_rgb():
    rng = np.random.default_rng(0)
    for _ in range(60):
        img, th, tw = _random_case(rng, 3, None)
        assert np.array_equal(M.resize(img, th, tw), _pillow(img, th, tw)), (img.shape, th, tw)


def test_model_equals_installed_pillow_rgba():
    """Alpha planes of only 0 and 255 (no un-premultiply division) and mixed ones; the premultiply round trip alone over all 65 536
    (colour, alpha) pairs against Pillow's own convert."""
    from PIL import Image
    rng = np.random.default_rng(1)
    for k in range(40):
        img, th, tw = _random_case(rng, 4, "binary" if k % 2 else "mixed")
        assert np.array_equal(M.resize(img, th, tw), _pillow(img, th, tw)), (img.shape, th, tw)
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    pairs = np.stack([c, c, c, a], -1)
    pre = np.asarray(Image.fromarray(pairs, "RGBA").convert("RGBa"))
    assert np.array_equal(M.premultiply(pairs), pre)
    assert np.array_equal(M.unpremultiply(pre), np.asarray(Image.frombytes("RGBa", (256, 256), pre.tobytes()).convert("RGBA")))


@pytest.mark.parametrize("C", [3, 4])
def test_model_one_axis_unchanged_and_both_unchanged(C):
    rng = np.random.default_rng(2 + C)
    img = rng.integers(0, 256, (37, 70, C), dtype=np.uint8)
    for th, tw in ((37, 20), (37, 141), (12, 70), (80, 70), (37, 70)):
        assert np.array_equal(M.resize(img, th, tw), _pillow(img, th, tw)), (th, tw)
    # RGBA, both unchanged: a copy -- the premultiply round trip would have changed these pixels
    if C == 4:
        assert np.array_equal(M.resize(img, 37, 70), img) and not np.array_equal(M.unpremultiply(M.premultiply(img)), img)


@pytest.mark.parametrize("sf", [0.1, 0.37, 1.0, 1.93])
def test_model_on_the_mappers_shapes(sf):
    """480 x 640 at EfficientDetResizeCrop's scaled size for TRAIN_SIZE 1024 and this scale factor."""
    rng = np.random.default_rng(int(sf * 100))
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    s = min(sf * 1024 / 480, sf * 1024 / 640)
    th, tw = max(1, int(480 * s)), max(1, int(640 * s))
    assert np.array_equal(M.resize(img, th, tw), _pillow(img, th, tw))


def test_product_tables_equal_the_models():
    from divergen_amd.data.resize_tables import FLIP, INTERLEAVED, PREMUL, ResizeJob, assemble_jobs, axis_table
    rng = np.random.default_rng(3)
    pairs = [(int(a), int(b)) for a, b in rng.integers(1, 400, (150, 2))] + [(640, 102), (640, 1976), (480, 76), (480, 1482), (1000, 1), (1, 1000), (130, 13), (100, 16)]
    for i, o in pairs:
        bounds, k = axis_table(i, o)
        if i == o:                                       # a skipped pass: identity taps
            assert bounds.tolist() == [[x, 1] for x in range(o)] and k.tolist() == [[1 << 22]] * o
            continue
        mb, mk = M.coefficients(i, o)
        assert k.shape[1] == 2 * int(np.ceil(max(i / o, 1.0))) + 1 and bounds.dtype == k.dtype == np.int32
        assert bounds.tolist() == [list(b) for b in mb], (i, o)
        for r in range(o):
            assert k[r, :len(mk[r])].tolist() == mk[r] and not k[r, len(mk[r]):].any(), (i, o, r)
        lo, hi = o // 3, max(o // 3 + 1, o - o // 4)          # a window's table is the rows of the whole table
        wb, wk = axis_table(i, o, lo, hi)
        assert np.array_equal(wb, bounds[lo:hi]) and np.array_equal(wk, k[lo:hi])
    # jobs: the shipped table applied with the kernel's arithmetic gives Pillow's window
    for n in range(12):
        C = 3 if n % 2 == 0 else 4
        img, th, tw = _random_case(rng, C, "mixed")
        if n == 5:
            th, tw = img.shape[:2]
        oy, ox = int(rng.integers(0, th)), int(rng.integers(0, tw))
        ch, cw = int(rng.integers(1, th - oy + 1)), int(rng.integers(1, tw - ox + 1))
        job = ResizeJob(img, (th, tw), (oy, ox), (ch, cw), flip=bool(n & 2), interleaved=C == 4)
        assert job.flags == (FLIP if n & 2 else 0) | (INTERLEAVED if C == 4 else 0) | (PREMUL if C == 4 and n != 5 else 0)
        src, table, tab = assemble_jobs([job, job], [0, 64])
        assert table.shape == (2, 13) and table[1, 0] % 4 == 0 and table[1, 12] == job.tiles and table[1, 7] == 64
        want = _pillow(img, th, tw)[oy:oy + ch, ox:ox + cw]
        want = want[:, ::-1] if n & 2 else want
        for row in table:
            assert np.array_equal(M.apply_tables(src, row, tab), want), n
    with pytest.raises(ValueError):
        axis_table(10, 20, 5, 21)
    with pytest.raises(ValueError):
        ResizeJob(np.zeros((4, 4, 3), np.uint8), (8, 8), interleaved=True)


def _mapper(cfg, dicts):
    from divergen_amd.data import build as B
    m = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    m.set_dataset(dicts)
    return m


def _shipped(u):
    """The key-on sample after unpack_sample on the CPU -> (image (3, h, w), flat) from the shipped source, jobs and tables alone."""
    p = u["image"].pending
    src, jobs, tab = p["src"].numpy(), p["jobs_host"], p["tab_host"]
    assert np.array_equal(p["jobs"].numpy(), jobs) and np.array_equal(p["tab"].numpy(), tab)
    image = M.apply_tables(src, jobs[0], tab).transpose(2, 0, 1)
    flat = u["paste_pack"]["flat"].numpy().copy()
    for row in jobs[1:]:
        assert row[6] & 2 and not flat[row[7]:row[7] + row[4] * row[5] * 4].any()          # left unwritten by the worker
        flat[row[7]:row[7] + row[4] * row[5] * 4] = M.apply_tables(src, row, tab).reshape(-1)
    return image, flat, len(jobs) - 1


@pytest.mark.parametrize("raster", [False, True])
def test_same_sample_key_off_and_on(tmp_path, monkeypatch, raster):
    """The same seeded samples through CopyPasteMapper ('syn_copy', packed) with the key off and on: the same np.random state afterwards,
    the same boxes, classes, masks / crossings, paste descriptors and labels; the key-on blob carries rs_src / rs_jobs / rs_tab and no
    image, and the model applied to what it ships reproduces the key-off image and the key-off `flat` byte for byte; the blob round trip
    through pack_sample / unpack_sample on the CPU; no host resize behind the key."""
    from divergen_amd.data import build as B
    from divergen_amd.structures import DeviceResizeImage
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 128, 0, ["INPUT.DEVICE_RASTER", raster])
    on = cfg.clone()
    on.merge_from_list(["INPUT.DEVICE_RESIZE", True])
    assert cfg.INPUT.DEVICE_RESIZE is False
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN)
    m_off, m_on = _mapper(cfg, dicts), _mapper(on, dicts)
    assert m_on.inst_pool.device_resize and not m_off.inst_pool.device_resize
    left = total = 0
    for i, d in enumerate(dicts[:8]):
        outs = []
        for m in (m_off, m_on):
            np.random.seed(100 + i)
            m.inst_pool.seed(100 + i)
            packed = m(d)
            outs.append((packed, np.random.get_state()))
        (p_off, s_off), (p_on, s_on) = outs
        assert all(np.array_equal(a, b) for a, b in zip(s_off, s_on)), "the key changed the np.random consumption"
        names_off, names_on = [x[0] for x in p_off["blob_layout"]], [x[0] for x in p_on["blob_layout"]]
        assert names_off[0] == "image" and names_on[:3] == ["rs_src", "rs_jobs", "rs_tab"] and names_on[3:] == names_off[1:]
        assert p_on["blob_hw"] == p_off["blob_hw"]
        u_off, u_on = B.unpack_sample(dict(p_off), "cpu"), B.unpack_sample(dict(p_on), "cpu")
        assert isinstance(u_on["image"], DeviceResizeImage) and u_on["image"].shape == tuple(u_off["image"].shape)
        i_off, i_on = u_off["instances"], u_on["instances"]
        assert torch.equal(i_off.gt_boxes.tensor, i_on.gt_boxes.tensor) and torch.equal(i_off.gt_classes, i_on.gt_classes)
        if raster:
            assert all(np.array_equal(getattr(i_off.gt_masks, k), getattr(i_on.gt_masks, k)) for k in ("pos", "poly_off", "inst_off"))
        else:
            assert torch.equal(i_off.gt_masks.tensor, i_on.gt_masks.tensor)
        for k in ("desc", "labels"):
            assert torch.equal(u_off["paste_pack"][k], u_on["paste_pack"][k])
        assert u_off["paste_pack"]["K"] == u_on["paste_pack"]["K"] and p_off["paste_labels"] == p_on["paste_labels"]
        image, flat, n_left = _shipped(u_on)
        assert np.array_equal(image, u_off["image"].numpy()) and np.array_equal(flat, u_off["paste_pack"]["flat"].numpy())
        left, total = left + n_left, total + int(u_on["paste_pack"]["K"])
        with pytest.raises(RuntimeError, match="DEVICE_RESIZE"):
            m_on.finish(dict(p_on), "cpu")
    assert 0 < left < total          # some patches went to the device, some (sources above 4x the target) were resized by the worker


def test_image_labelled_and_unpacked_samples(tmp_path, monkeypatch):
    """USE_COPY_METHOD 'none' with WITH_IMAGE_LABELS and USE_DIFF_BS_SIZE-style sources (samples are not packed): the structure itself
    crosses; boxes, classes and the random state as with the key off; an image-labelled sample carries its structure and empty
    instances; the model on the shipped job gives the key-off image."""
    from divergen_amd.data import build as B
    from divergen_amd.data.resize_tables import assemble_jobs
    from divergen_amd.structures import DeviceResizeImage
    from tests.test_host_image_labels import _two_source_cfg
    cfg, info = _two_source_cfg(tmp_path, monkeypatch, ["INPUT.USE_COPY_METHOD", "none", "INPUT.INST_POOL", False, "INPUT.SCALE_RANGE", [0.3, 2.0]])
    on = cfg.clone()
    on.merge_from_list(["INPUT.DEVICE_RESIZE", True])
    dicts = B.get_detection_dataset_dicts_with_source(cfg.DATASETS.TRAIN, filter_empty=False, dataset_ann=cfg.DATALOADER.DATASET_ANN)
    m_off, m_on = _mapper(cfg, dicts), _mapper(on, dicts)
    kinds, flips = set(), set()
    for i, d in enumerate(dicts):
        np.random.seed(7 + i)
        a = m_off(d)
        s_a = np.random.get_state()
        np.random.seed(7 + i)
        b = m_on(d)
        assert all(np.array_equal(x, y) for x, y in zip(s_a, np.random.get_state()))
        assert "blob" not in b and isinstance(b["image"], DeviceResizeImage) and b["image"].shape == tuple(a["image"].shape)
        ia, ib = a["instances"], b["instances"]
        assert torch.equal(ia.gt_boxes.tensor, ib.gt_boxes.tensor) and torch.equal(ia.gt_classes, ib.gt_classes)
        assert torch.equal(ia.gt_masks.tensor, ib.gt_masks.tensor) and a.get("ann_type") == b.get("ann_type")
        src, table, tab = assemble_jobs([b["image"].job], [0])
        assert np.array_equal(M.apply_tables(src, table[0], tab).transpose(2, 0, 1), a["image"].numpy())
        kinds.add(b["ann_type"])
        flips.add(bool(table[0, 6] & 1))
        with pytest.raises(RuntimeError, match="DEVICE_RESIZE"):
            m_on.finish(b, "cpu")
    assert kinds == {"box", "image"} and flips == {False, True}


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
        with pytest.raises(NotImplementedError, match=r"INPUT\.DEVICE_RESIZE.*INPUT\.USE_COPY_METHOD '%s'" % method):
            build("INPUT.USE_COPY_METHOD", method, "INPUT.DEVICE_RESIZE", True)
    with pytest.raises(NotImplementedError, match=r"INPUT\.DEVICE_RESIZE.*INPUT\.ACTIVE_SELECT"):
        build("INPUT.ACTIVE_SELECT", True, "INPUT.DEVICE_RESIZE", True)
    for method in ("none", "syn_copy"):
        m = build("INPUT.USE_COPY_METHOD", method, "INPUT.DEVICE_RESIZE", True, "INPUT.DEVICE_RASTER", True, "INPUT.SCP_SRC_MODES", True,
                  "INPUT.RM_BG_PROB", 0.5)
        assert m.device_resize and m.mapper.device_resize and m.device_raster and m.rm_bg_prob == 0.5
    c = cfg.clone()
    c.merge_from_list(["INPUT.DEVICE_RESIZE", True])
    assert B.DatasetMapper(c, True).device_resize and not B.DatasetMapper(c, False).device_resize      # the training mapper only
    c = cfg.clone()
    c.merge_from_list(["INPUT.INST_POOL", False, "INPUT.USE_COPY_METHOD", "none", "INPUT.DEVICE_RESIZE", True])
    with pytest.raises(NotImplementedError, match=r"INPUT\.DEVICE_RESIZE"):
        B.build_detection_train_loader(c, 2, "cpu", 3)


def test_ring_slot_with_the_key():
    from divergen_amd.data import build as B
    for size in (64, 128, 640, 1024):
        for n_src in (0, 2):
            for raster in (False, True):
                off, on = B.ring_slot_bytes(size, n_src, raster), B.ring_slot_bytes(size, n_src, raster, True)
                assert off == B.ring_slot_bytes(size, n_src, raster, False) and on <= B.ring_slot_bytes(size, n_src)
    assert B.ring_slot_bytes(1024) == 1024 * 1024 * 48 + (8 << 20) and B.ring_slot_bytes(1024, 0, False, True) == B.ring_slot_bytes(1024)
    assert B.ring_slot_bytes(1024, 0, True, True) == B.ring_slot_bytes(1024, 0, True) + B.DEVICE_RESIZE_TABLE_BYTES


def test_abi_declared_bound_and_built():
    import os
    from divergen_amd import _lib
    from divergen_amd.csrc.build import SOURCES
    from divergen_amd.layers import resize_ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "divergen_hip.h")).read()
    assert "int dgx_resize_bilinear_u8(" in hdr and "dgx_resize_bilinear_u8" in _lib.SIGNATURES and "resize_u8.hip" in SOURCES
    assert hasattr(_lib.lib(), "dgx_resize_bilinear_u8")
    assert "dgx_resize_bilinear_u8" in open(os.path.join(root, "INTEGRATION.md")).read()
    with pytest.raises(_lib.DgxError):                                     # no CPU fallback
        resize_ops.resize_bilinear_u8(torch.zeros(12, dtype=torch.uint8), np.zeros((1, 13), np.int32), np.zeros(4, np.int32),
                                      image=torch.zeros(12, dtype=torch.uint8))
