"""GPU: dgx_resize_bilinear_u8 (INPUT.DEVICE_RESIZE) against the installed Pillow, every byte, no tolerance, and the key-on data path
against the key-off one, bit for bit.  Every kernel case writes into buffers pre-filled with a sentinel and compares the WHOLE buffers:
a byte the kernel leaves out of a window, or writes outside one, shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _source(rng, h, w, C, alpha="mixed"):
    img = rng.integers(0, 256, (h, w, C), dtype=np.uint8)
    if C == 4 and alpha == "binary":
        img[..., 3] = rng.choice(np.array([0, 255], dtype=np.uint8), (h, w))
    return img


def _pillow(src, out_hw, crop_yx, crop_hw, flip):
    from PIL import Image
    im = Image.fromarray(src, "RGB" if src.shape[2] == 3 else "RGBA").resize((out_hw[1], out_hw[0]), Image.BILINEAR)
    r = np.asarray(im)[crop_yx[0]:crop_yx[0] + crop_hw[0], crop_yx[1]:crop_yx[1] + crop_hw[1]]
    return np.ascontiguousarray(r[:, ::-1] if flip else r)


def _launch(specs, pads=None):
    """specs: [(src, out_hw, crop_yx, crop_hw | None, flip, interleaved)]; pads: bytes of sentinel in front of each job's window in its
    destination buffer (default 0, then 3, 5, 7, ... for planar jobs -- odd: off the 4-byte alignment -- and 8 for interleaved ones).
    -> (image buffer, flat buffer) as the kernel left them and as Pillow says they must be (numpy uint8), and the jobs."""
    from divergen_amd.data.resize_tables import ResizeJob, assemble_jobs
    from divergen_amd.layers.resize_ops import resize_bilinear_u8
    jobs = [ResizeJob(s, o, yx, hw, flip=f, interleaved=il) for s, o, yx, hw, f, il in specs]
    cur, offs = [0, 0], []
    for i, job in enumerate(jobs):
        b = int(job.interleaved)
        cur[b] += pads[i] if pads is not None else (8 if b else (0 if i == 0 else 2 * i + 1))
        offs.append(cur[b])
        cur[b] += job.out_bytes
    want = [np.full(cur[0] + 5, SENTINEL, np.uint8), np.full(cur[1] + 8, SENTINEL, np.uint8)]
    for job, off, (s, o, yx, hw, f, il) in zip(jobs, offs, specs):
        r = _pillow(s, o, yx, job.crop_hw, f)
        want[int(il)][off:off + job.out_bytes] = (r if il else r.transpose(2, 0, 1)).reshape(-1)
    src, table, tab = assemble_jobs(jobs, offs)
    got = [torch.full((w.size,), SENTINEL, dtype=torch.uint8, device="cuda") for w in want]
    resize_bilinear_u8(torch.from_numpy(src).cuda(), table, tab, image=got[0], flat=got[1])
    return [g.cpu().numpy() for g in got], want, (src, table, tab)


def _check(specs, pads=None):
    got, want, arrays = _launch(specs, pads)
    for g, w, name in zip(got, want, ("image", "flat")):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s: %d bytes differ, first at %d (got %d, want %d)" % (name, bad.size, bad[0], g[bad[0]], w[bad[0]])
    return got, arrays


SIZES = [((1, 1), (1, 1)), ((1, 1), (5, 7)), ((1, 9), (1, 4)), ((1, 9), (3, 20)), ((9, 1), (4, 1)), ((9, 1), (17, 2)),
         ((37, 70), (20, 33)), ((37, 70), (71, 135)),          # 1.92x / 1.93x up
         ((64, 130), (10, 13)),                                # 6.4x down (ksize 15) x 10x down (ksize 21); 64 source rows: two chunks
         ((64, 130), (100, 200)), ((100, 50), (16, 8)),        # 6.25x down, both axes (ksize 15)
         ((130, 64), (13, 70)),                                # 10x down vertically (ksize 21): the tile spans 130 source rows, five chunks
         ((37, 70), (37, 20)), ((37, 70), (50, 70)), ((37, 70), (37, 70))]      # horizontal pass only, vertical only, neither


@pytest.mark.parametrize("src_hw,out_hw", SIZES)
def test_sizes_rgb_planar_and_rgba_interleaved(src_hw, out_hw):
    """Every size pair as a planar 3-channel job, an interleaved RGBA job with alpha in {0, 255} and one with mixed alpha, plain and
    mirrored, all in one launch."""
    rng = np.random.default_rng(src_hw[0] * 1000 + src_hw[1] + out_hw[0])
    specs = []
    for flip in (False, True):
        specs.append((_source(rng, *src_hw, 3), out_hw, (0, 0), None, flip, False))
        specs.append((_source(rng, *src_hw, 4, "binary"), out_hw, (0, 0), None, flip, True))
        specs.append((_source(rng, *src_hw, 4, "mixed"), out_hw, (0, 0), None, flip, True))
    _, (_, table, _) = _check(specs)
    same = tuple(src_hw) == tuple(out_hw)
    assert [int(f) & 4 for f in table[:, 6]] == [0, 0 if same else 4, 0 if same else 4] * 2      # RGBA, both sizes unchanged: a copy


@pytest.mark.parametrize("flip", [False, True])
def test_crop_windows_off_the_tile_and_off_alignment(flip):
    """Windows of the scaled image that start and end off the 64 x 16 tile and off 4-byte alignment, 1 pixel wide and 1 pixel high
    among them, with destinations at odd byte offsets (byte stores) and at aligned ones (dword stores)."""
    rng = np.random.default_rng(5 + flip)
    rgb, rgba = _source(rng, 64, 130, 3), _source(rng, 64, 130, 4)
    windows = [((17, 63), (1, 70)), ((3, 5), (40, 1)), ((15, 61), (20, 67)), ((0, 0), (33, 129)), ((99, 199), (1, 1)), ((16, 64), (16, 64)),
               ((31, 1), (18, 131))]
    specs = [(rgb, (100, 200), yx, hw, flip, False) for yx, hw in windows] + [(rgba, (100, 200), yx, hw, flip, True) for yx, hw in windows]
    _check(specs)
    _check(specs, pads=[4 * i for i in range(len(windows))] + [1] + [4] * (len(windows) - 1))      # other offsets; RGBA off alignment (byte stores)
    _check([(rgba, (100, 200), (15, 61), (20, 67), flip, False)])                                    # planar with four channels


def test_one_launch_mixes_an_image_job_and_five_patch_jobs_and_repeats():
    rng = np.random.default_rng(11)
    specs = [(_source(rng, 48, 64, 3), (92, 123), (7, 20), (80, 96), True, False)]
    for k, (hw, out) in enumerate([((20, 31), (33, 40)), ((50, 50), (25, 26)), ((9, 70), (9, 70)), ((64, 12), (100, 5)), ((7, 7), (70, 75))]):
        specs.append((_source(rng, *hw, 4, "binary" if k % 2 else "mixed"), out, (0, 0), None, bool(k % 2), True))
    got, (_, table, _) = _check(specs)
    assert table.shape == (6, 13) and table[:, 12].tolist() == sorted(set(table[:, 12].tolist())) and table[0, 12] == 0
    again, _, _ = _launch(specs)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_full_size_image_job():
    """480 x 640 at scale factor 1.93 of TRAIN_SIZE 1024 (1482 x 1976), cropped to 1024^2, mirrored."""
    rng = np.random.default_rng(3)
    s = min(1.93 * 1024 / 480, 1.93 * 1024 / 640)
    out_hw = (max(1, int(480 * s)), max(1, int(640 * s)))
    assert out_hw == (1482, 1976)
    _check([(_source(rng, 480, 640, 3), out_hw, (229, 477), (1024, 1024), True, False)])


def test_invalid_job_tables_raise_and_launch_nothing():
    from divergen_amd import _lib as L
    from divergen_amd.data.resize_tables import ResizeJob, assemble_jobs
    from divergen_amd.layers.resize_ops import resize_bilinear_u8
    rng = np.random.default_rng(2)
    jobs = [ResizeJob(_source(rng, 20, 30, 3), (31, 47)), ResizeJob(_source(rng, 12, 10, 4), (9, 17), flip=True, interleaved=True)]
    src, table, tab = assemble_jobs(jobs, [0, 0])
    src_d = torch.from_numpy(src).cuda()
    image = torch.full((jobs[0].out_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    flat = torch.full((jobs[1].out_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")

    def bad(row, word, value, tab_edit=None):
        t, c = table.copy(), tab.copy()
        t[row, word] = value
        if tab_edit is not None:
            c[tab_edit[0]] = tab_edit[1]
        return t, c
    h_off, v_off = int(table[0, 8]), int(table[0, 10])
    cases = [bad(0, 0, src.size - 10),                     # source range past the buffer
             bad(1, 0, 2),                                 # an RGBA source off 4-byte alignment
             bad(1, 1, 13),                                # a source (the last one) taller than its bytes
             bad(0, 7, 1), bad(1, 7, 4),                   # destination range past the buffer
             bad(0, 4, 32),                                # a window taller than the tables and the destination
             bad(0, 4, -1), bad(0, 5, 0), bad(1, 1, 0),    # a negative / zero size
             bad(0, 3, 5), bad(0, 6, 8), bad(0, 6, 2),     # channels, flags, interleaved with three channels
             bad(0, 8, tab.size - 5), bad(0, 10, -1),      # coefficient range past the buffer / before it
             bad(0, 9, 0), bad(0, 11, 1000),               # ksize
             bad(1, 12, int(table[1, 12]) + 1),            # tile0
             bad(0, 0, 0, (h_off + 2 * 46 + 1, 3)),        # xmin + n > in: last column's n grows past the source's width
             bad(0, 0, 0, (h_off + 2 * 46, 30)),           # xmin itself past the source
             bad(0, 0, 0, (v_off, -1)),                    # a negative first row
             bad(0, 0, 0, (v_off + 1, 4))]                 # n > ksize
    for t, c in cases:
        with pytest.raises(L.DgxError):
            resize_bilinear_u8(src_d, t, c, image=image, flat=flat)
        # the C entry point holds the HOST copies to the buffers, whatever the device copies say
        t_d, c_d = torch.from_numpy(table).cuda(), torch.from_numpy(tab).cuda()
        rc = L.lib().dgx_resize_bilinear_u8(L.ptr(src_d), src.size, L.ptr(t_d), L.ptr(c_d), t.ctypes.data, c.ctypes.data, 2, c.size,
                                            L.ptr(image), image.numel(), L.ptr(flat), flat.numel(), L.stream())
        assert rc == -1
    with pytest.raises(L.DgxError):
        resize_bilinear_u8(src_d, table, tab, image=image[:-1], flat=flat)        # a destination one byte short
    with pytest.raises(L.DgxError):
        resize_bilinear_u8(src_d, table, tab, image=image, flat=None)             # an interleaved job without `flat`
    with pytest.raises(L.DgxError):
        resize_bilinear_u8(src_d, torch.from_numpy(table).cuda(), tab, image=image, flat=flat)      # the table to validate must be on the host
    with pytest.raises(L.DgxError):
        resize_bilinear_u8(src_d, table.astype(np.int64), tab, image=image, flat=flat)
    with pytest.raises(L.DgxError):
        resize_bilinear_u8(src_d, table, tab[:-1], image=image, flat=flat)        # tab shorter than the tables say
    torch.cuda.synchronize()
    assert bool((image == SENTINEL).all()) and bool((flat == SENTINEL).all())
    resize_bilinear_u8(src_d, table, tab, image=image, flat=flat)                 # and the good table runs
    assert np.array_equal(image.cpu().numpy().reshape(3, 31, 47), _pillow(jobs[0].src, (31, 47), (0, 0), (31, 47), False).transpose(2, 0, 1))
    assert np.array_equal(flat.cpu().numpy().reshape(9, 17, 4), _pillow(jobs[1].src, (9, 17), (0, 0), (9, 17), True))
    assert L.lib().dgx_resize_bilinear_u8(None, 0, None, None, None, None, 0, 0, None, 0, None, 0, L.stream()) == 0      # J == 0


def _mappers(tmp_path, monkeypatch, extra=()):
    from divergen_amd.data import build as B
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 128, 0, extra)
    on = cfg.clone()
    on.merge_from_list(["INPUT.DEVICE_RESIZE", True])
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN)
    ms = []
    for c in (cfg, on):
        m = B.CopyPasteMapper(B.DatasetMapper(c, True), c)
        m.set_dataset(dicts)
        ms.append(m)
    return ms[0], ms[1], dicts


def _same_sample(a, b):
    assert a["image"].is_cuda and b["image"].is_cuda and a["image"].dtype == b["image"].dtype == torch.uint8
    assert torch.equal(a["image"], b["image"])
    ia, ib = a["instances"], b["instances"]
    assert torch.equal(ia.gt_boxes.tensor, ib.gt_boxes.tensor) and torch.equal(ia.gt_classes, ib.gt_classes)
    assert ia.gt_masks.tensor.dtype == ib.gt_masks.tensor.dtype == torch.bool and torch.equal(ia.gt_masks.tensor, ib.gt_masks.tensor)
    assert ia.has("instance_source") == ib.has("instance_source")
    if ia.has("instance_source"):
        assert torch.equal(ia.instance_source, ib.instance_source)


@pytest.mark.parametrize("rm_bg", [False, True])
@pytest.mark.parametrize("raster", [False, True])
@pytest.mark.parametrize("method", ["none", "syn_copy"])
def test_finish_key_off_and_on_are_bit_equal(tmp_path, monkeypatch, method, raster, rm_bg):
    """CopyPasteMapper.finish, the loader's training-process half, on the same seeded samples with the key off and on: 'none' (the sample
    crosses unpacked: the structure itself is materialised) and 'syn_copy' (the blob: image job and patch jobs in one launch), with
    INPUT.DEVICE_RASTER off and on, and with INPUT.RM_BG_PROB 1 under INPUT.SCP_SRC_MODES (dgx_remove_background reads the image the
    resize has just written)."""
    from divergen_amd.structures import DeviceResizeImage
    extra = ["INPUT.USE_COPY_METHOD", method, "INPUT.DEVICE_RASTER", raster]
    if rm_bg:
        extra += ["INPUT.SCP_SRC_MODES", True, "INPUT.RM_BG_PROB", 1.0]
    m_off, m_on, dicts = _mappers(tmp_path, monkeypatch, extra)
    left = 0
    for i in range(4):
        outs = []
        for m in (m_off, m_on):
            np.random.seed(70 + i)
            if m.inst_pool is not None:
                m.inst_pool.seed(70 + i)
            w = m(dicts[i])
            if m is m_on and "blob" in w:
                left += {name: shape for name, _, shape, _ in w["blob_layout"]}["rs_jobs"][0] - 1      # jobs besides the image's
            elif m is m_on:
                assert isinstance(w["image"], DeviceResizeImage)
            outs.append(m.finish(w, "cuda"))
        _same_sample(*outs)
    assert method == "none" or left > 0          # some pool patch took the device way


def test_loader_with_workers_and_ring_key_on_equals_key_off_inline(tmp_path, monkeypatch):
    """build_detection_train_loader with the key ON, 2 worker processes writing into the page-locked ring, against the key-OFF mapper
    run inline with the workers' seeds: every batch bit-identical.  The tables the wrapper validates come from the ring slot's host
    side, the ones the kernel reads from the uploaded copy."""
    import itertools
    from divergen_amd.data import build as B
    from divergen_amd.data.samplers import RepeatFactorTrainingSampler
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 128, 2)
    on = cfg.clone()
    on.merge_from_list(["INPUT.DEVICE_RESIZE", True])
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    seed, per_gpu, nb, nw = 3, 2, 4, 2
    it = B.build_detection_train_loader(on, per_gpu, "cuda", seed)
    got = [next(it) for _ in range(nb)]
    torch.cuda.synchronize()
    ring = it.finish.__self__.ring
    assert ring is not None and ring.slot_bytes == (B.ring_slot_bytes(128, 0, False, True) + 4095) // 4096 * 4096 <= B.ring_slot_bytes(128) + 4095
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
    mapper = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    mapper.set_dataset(dicts)
    rf = RepeatFactorTrainingSampler.repeat_factors_from_category_frequency(dicts, cfg.DATALOADER.REPEAT_THRESHOLD)
    idx = list(itertools.islice(iter(RepeatFactorTrainingSampler(rf, seed=seed)), nb * per_gpu))
    for w in range(nw):
        np.random.seed((seed * 1009 + w) % (2 ** 31))
        mapper.inst_pool.seed((seed * 1009 + w) % (2 ** 31))
        for b in range(w, nb, nw):
            for j in range(per_gpu):
                want = mapper.finish(mapper(dicts[idx[b * per_gpu + j]]), "cuda")
                assert got[b][j]["file_name"] == want["file_name"]
                _same_sample(got[b][j], want)
