"""GPU: dgx_polygons_to_bitmask (INPUT.DEVICE_RASTER) against the host rasteriser it replaces, byte for byte, and the key-on data
path against the key-off one, bit for bit.  Reference: data/build.py:polygons_to_bitmask (pinned by tests/test_host_data.py).  Every
kernel case writes into a buffer pre-filled with 0xFF: a byte the kernel leaves out shows."""
import numpy as np
import pytest
import torch

from tests._raster_ref import CANVASES, polygon_set, sorted_crossings

pytestmark = pytest.mark.gpu


def _reference(instances, H, W):
    from divergen_amd.data.build import polygons_to_bitmask
    ref = np.zeros((len(instances), H, W), dtype=bool)
    for i, polys in enumerate(instances):
        polygons_to_bitmask(polys, H, W, out=ref[i])
    return torch.from_numpy(ref.view(np.uint8))


def _fill(instances, H, W, base_offset=0):
    """instances: per instance the list of its polygons (flat coordinate lists) -> (uint8 (N, H, W) from the kernel, the crossings)."""
    from divergen_amd.layers.raster_ops import polygons_to_bitmask
    from divergen_amd.structures import PolygonCrossings
    pc = PolygonCrossings.from_lists([[sorted_crossings(p, H, W) for p in polys] for polys in instances], (H, W))
    buf = torch.full((len(instances) * H * W + base_offset,), 0xFF, dtype=torch.uint8, device="cuda")
    out = buf[base_offset:].view(len(instances), H, W)
    got = polygons_to_bitmask(torch.from_numpy(pc.pos).cuda(), pc.poly_off, pc.inst_off, H, W, out=out)
    assert got.data_ptr() == out.data_ptr()
    return out, pc


def _check(instances, H, W, base_offset=0):
    out, pc = _fill(instances, H, W, base_offset)
    assert torch.equal(out.cpu(), _reference(instances, H, W))
    return out, pc


def _random_instances(rng, H, W, n_inst, max_polys=3):
    inst = []
    for _ in range(n_inst):
        polys = []
        for _ in range(int(rng.integers(1, max_polys + 1))):
            k = int(rng.integers(3, 12))
            cx, cy, r = rng.uniform(-0.1 * W, 1.1 * W), rng.uniform(-0.1 * H, 1.1 * H), rng.uniform(0.5, 0.7 * max(H, W))
            polys.append(np.stack([cx + r * rng.uniform(-1, 1, k), cy + r * rng.uniform(-1, 1, k)], 1).round(2).reshape(-1).tolist())
        inst.append(polys)
    return inst


def test_known_answer_polygons_5x6():
    box, tri, box2, outside = [1, 1, 4, 1, 4, 3, 1, 3], [0, 0, 5, 0, 0, 4], [4, 3, 6, 3, 6, 5, 4, 5], [10, 10, 12, 10, 12, 12]
    out, _ = _check([[box], [tri], [box, box2], [outside]], 5, 6)
    want = np.zeros((5, 6), np.uint8)
    want[1:3, 1:4] = 1
    assert np.array_equal(out[0].cpu().numpy(), want)
    assert out[1].cpu().tolist() == [[1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    want[3:5, 4:6] = 1
    assert np.array_equal(out[2].cpu().numpy(), want) and not out[3].any()


@pytest.mark.parametrize("hw", [(37, 70), (64, 130), (1, 9), (9, 1), (64, 64), (70, 260), (130, 516)])
def test_canvases_off_the_wave_and_the_tile(hw):
    """Widths that are no multiple of the 4 columns of a lane, of the 256 of a wave's row or of nothing at all; heights that are no
    multiple of a wave's 16 rows or a workgroup's 64; more than one tile each way ((130, 516): 3 x 3 tiles); and, on the widths that
    take the dword stores, an output base that is not 4-byte aligned (byte stores then)."""
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    inst = _random_instances(rng, H, W, 7)
    _check(inst, H, W)
    if W % 4 == 0:
        _check(inst, H, W, base_offset=1)


def test_one_sample_mixing_instances():
    H, W = 37, 70
    a = [5, 5, 40, 5, 40, 30, 5, 30]
    b = [20, 10, 60, 10, 60, 35, 20, 35]                    # overlaps a: OR keeps the overlap set, XOR would clear it
    outside = [100, 10, 130, 10, 130, 30]
    out, pc = _check([[], [a, b], [outside], [a, outside], []], H, W)
    assert pc.inst_off.tolist() == [0, 0, 2, 3, 5, 5]
    assert not out[0].any() and not out[2].any() and not out[4].any()
    assert bool(out[1, 20, 30]) and int(out[1].sum()) == 35 * 25 + 40 * 25 - 20 * 20 and torch.equal(out[3], _check([[a]], H, W)[0][0])
    # N == 0: success, nothing written, an empty result
    from divergen_amd import _lib as L
    from divergen_amd.layers.raster_ops import polygons_to_bitmask
    empty = polygons_to_bitmask(torch.zeros(0, dtype=torch.int32, device="cuda"), np.zeros(1, np.int64), np.zeros(1, np.int64), H, W)
    assert tuple(empty.shape) == (0, H, W) and empty.dtype == torch.uint8
    z = np.zeros(1, np.int64)
    assert L.lib().dgx_polygons_to_bitmask(None, 0, None, None, z.ctypes.data, z.ctypes.data, 0, 0, H, W, None, L.stream()) == 0


@pytest.mark.parametrize("hw", CANVASES)
def test_polygon_set_of_the_host_test(hw):
    """Every polygon of the host test's set as one instance of one sample -- the odd lists (the tail of the canvas set) and the
    crossings clipped to yd == H (parity carried into the next column) among them."""
    H, W = hw
    group = [(p, tags) for h, w, p, tags in polygon_set() if (h, w) == (H, W)]
    assert any("odd" in t for _, t in group) and any("carry" in t for _, t in group) and any("duplicate" in t for _, t in group)
    out, _ = _check([[p] for p, _ in group], H, W)
    odd = torch.tensor(["odd" in t for _, t in group])
    assert bool(out[odd][:, H - 1, W - 1].all()) and int(odd.sum()) > 0
    # and the same polygons three to an instance
    _check([[p for p, _ in group[i:i + 3]] for i in range(0, len(group), 3)], H, W)


def test_full_size_canvas_and_two_runs_give_the_same_bytes():
    H = W = 1024
    t = np.linspace(0, 2 * np.pi, 120, endpoint=False)
    r = np.where(np.arange(120) % 2 == 0, 400.0, 250.0)
    star = np.stack([512 + r * np.cos(t), 500 + r * np.sin(t)], 1).round(2).reshape(-1).tolist()
    corner = [1000.3, 1010.2, 1030.0, 1001.0, 1030.0, 1030.0, 990.0, 1030.0]        # past the bottom-right corner
    sliver = [3.2, 0, 5.9, 0, 5.9, 1024, 3.2, 1024]
    comb = [10, 40, 20, 40]                                 # five long teeth: ten crossings in each of a thousand columns, a list
    for k in range(5):                                      # too long for the kernel's LDS copy (4096): searched in global memory
        comb += [20, 100 + 150 * k, 1000.5, 110 + 150 * k, 1000.5, 150 + 150 * k, 20, 160 + 150 * k]
    comb += [20, 900, 10, 900]
    inst = [[star], [star, corner], [sliver, [600, 20, 990, 40, 800, 300]], [], [comb], [corner, comb, star]]
    out, pc = _check(inst, H, W)
    assert pc.pos.max() > 2 ** 20 - 2 * H and int(out[0].sum()) > 200000
    counts = np.diff(pc.poly_off)
    assert int(counts.max()) > 4096 > int(counts[counts > 0].min())          # both sides of the kernel's LDS limit
    again, _ = _fill(inst, H, W)
    assert torch.equal(out, again)


def test_bad_offsets_and_oversized_canvas_launch_nothing():
    from divergen_amd import _lib as L
    from divergen_amd.layers.raster_ops import polygons_to_bitmask
    H, W = 5, 6
    pos = torch.from_numpy(sorted_crossings([1, 1, 4, 1, 4, 3, 1, 3], H, W)).cuda()
    n = int(pos.numel())
    out = torch.full((1, H, W), 0xFF, dtype=torch.uint8, device="cuda")
    good = (np.array([0, n], np.int64), np.array([0, 1], np.int64))
    for poly_off, inst_off in ((np.array([0, n + 1], np.int64), good[1]),          # poly_off past len(pos)
                               (np.array([0, n - 1], np.int64), good[1]),
                               (good[0], np.array([0, 2], np.int64)),              # inst_off past P
                               (good[0], np.array([0, 0], np.int64)),
                               (np.array([0, n + 2, n], np.int64), np.array([0, 2], np.int64)),       # decreasing
                               (np.array([1, n], np.int64), good[1])):             # not starting at 0
        with pytest.raises(L.DgxError):
            polygons_to_bitmask(pos, poly_off, inst_off, H, W, out=out)
        # the C entry point holds the host offsets to the same sizes, whatever the device copies say
        d_poly, d_inst = torch.from_numpy(good[0]).cuda(), torch.from_numpy(good[1]).cuda()
        rc = L.lib().dgx_polygons_to_bitmask(L.ptr(pos), n, L.ptr(d_poly), L.ptr(d_inst), poly_off.ctypes.data, inst_off.ctypes.data,
                                             inst_off.size - 1, poly_off.size - 1, H, W, L.ptr(out), L.stream())
        assert rc == -1
    with pytest.raises(L.DgxError):
        polygons_to_bitmask(pos, torch.from_numpy(good[0]).cuda(), good[1], H, W, out=out)      # offsets to validate must be host arrays
    with pytest.raises(L.DgxError):
        polygons_to_bitmask(pos.to(torch.int64), good[0], good[1], H, W, out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xFF).all())
    # H * W >= 2^31: refused from the sizes alone, before anything is allocated
    before = torch.cuda.memory_allocated()
    with pytest.raises(L.DgxError, match="2\\^31"):
        polygons_to_bitmask(pos, good[0], good[1], 46341, 46341)
    assert torch.cuda.memory_allocated() == before
    assert L.lib().dgx_polygons_to_bitmask(L.ptr(pos), n, L.ptr(out), L.ptr(out), good[0].ctypes.data, good[1].ctypes.data, 1, 1,
                                           46341, 46341, L.ptr(out), L.stream()) == -2
    assert torch.equal(polygons_to_bitmask(pos, good[0], good[1], H, W, out=out).cpu(), _reference([[[1, 1, 4, 1, 4, 3, 1, 3]]], H, W))


def _mappers(tmp_path, monkeypatch, extra=()):
    from divergen_amd.data import build as B
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 128, 0, extra)
    on = cfg.clone()
    on.merge_from_list(["INPUT.DEVICE_RASTER", True])
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN)
    ms = []
    for c in (cfg, on):
        m = B.CopyPasteMapper(B.DatasetMapper(c, True), c)
        m.set_dataset(dicts)
        ms.append(m)
    return ms[0], ms[1], dicts


def _same_sample(a, b):
    assert torch.equal(a["image"], b["image"]) and a["image"].is_cuda
    ia, ib = a["instances"], b["instances"]
    assert torch.equal(ia.gt_boxes.tensor, ib.gt_boxes.tensor) and torch.equal(ia.gt_classes, ib.gt_classes)
    assert ia.gt_masks.tensor.dtype == ib.gt_masks.tensor.dtype == torch.bool and torch.equal(ia.gt_masks.tensor, ib.gt_masks.tensor)
    assert ia.has("instance_source") == ib.has("instance_source")
    if ia.has("instance_source"):
        assert torch.equal(ia.instance_source, ib.instance_source)


def test_end_to_end_key_off_and_on_are_bit_equal(tmp_path, monkeypatch):
    """Seeded samples of the generated mini split through mapper, pack, unpack and InstPool.composite with the key off and on: image,
    masks, boxes, classes bit for bit equal -- one sample without pastes and samples with."""
    from divergen_amd.data import build as B
    from divergen_amd.data.copypaste import InstPool
    from divergen_amd.structures import PolygonCrossings
    m_off, m_on, dicts = _mappers(tmp_path, monkeypatch)
    m_off.inst_pool.max_samples = m_on.inst_pool.max_samples = 3          # randint(0, 3): a third of the samples draw no paste
    ks = []
    for i in range(8):
        outs = []
        for m in (m_off, m_on):
            np.random.seed(40 + i)
            m.inst_pool.seed(40 + i)
            u = B.unpack_sample(m(dicts[i]), "cuda")
            assert isinstance(u["instances"].gt_masks, PolygonCrossings) == (m is m_on)
            outs.append(InstPool.composite(u, "cuda"))
        _same_sample(*outs)
        for x, y in zip(outs[0]["_uploaded"], outs[1]["_uploaded"]):      # the un-pasted sample on the device, masks included
            assert torch.equal(x, y)
        ks.append(int(outs[0]["instances"].instance_source.sum()))
    assert min(ks) == 0 and max(ks) > 0, ks


def test_loader_with_workers_and_ring_key_on_equals_key_off_inline(tmp_path, monkeypatch):
    """build_detection_train_loader with the key ON, 2 worker processes writing into the page-locked ring (sized without mask planes),
    against the key-OFF mapper run inline with the workers' seeds: every batch bit-identical.  The offsets the wrapper validates come
    from the ring slot's host side, the ones the kernel reads from the uploaded copy."""
    import itertools
    from divergen_amd.data import build as B
    from divergen_amd.data.samplers import RepeatFactorTrainingSampler
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 128, 2)
    on = cfg.clone()
    on.merge_from_list(["INPUT.DEVICE_RASTER", True])
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    seed, per_gpu, nb, nw = 3, 2, 4, 2
    it = B.build_detection_train_loader(on, per_gpu, "cuda", seed)
    got = [next(it) for _ in range(nb)]
    torch.cuda.synchronize()
    ring = it.finish.__self__.ring
    assert ring is not None and ring.slot_bytes == (B.ring_slot_bytes(128, 0, True) + 4095) // 4096 * 4096 <= B.ring_slot_bytes(128) + 4095
    assert B.ring_slot_bytes(1024, 0, True) == 3 * 1024 * 1024 + (12 << 20) and B.ring_slot_bytes(1024) == 48 * 1024 * 1024 + (8 << 20)
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


@pytest.mark.parametrize("method", ["none", "syn_copy"])
def test_finish_key_off_and_on_with_background_removal(tmp_path, monkeypatch, method):
    """CopyPasteMapper.finish, the loader's training-process half: 'none' (the sample crosses unpacked) and 'syn_copy', with
    INPUT.RM_BG_PROB 1 under INPUT.SCP_SRC_MODES -- dgx_remove_background reads the masks the fill has just written."""
    m_off, m_on, dicts = _mappers(tmp_path, monkeypatch, ["INPUT.USE_COPY_METHOD", method, "INPUT.SCP_SRC_MODES", True, "INPUT.RM_BG_PROB", 1.0])
    blank = 0
    for i in range(3):
        outs = []
        for m in (m_off, m_on):
            np.random.seed(70 + i)
            if m.inst_pool is not None:
                m.inst_pool.seed(70 + i)
            outs.append(m.finish(m(dicts[i]), "cuda"))
        _same_sample(*outs)
        blank += int((outs[1]["image"] == 0).all(0).sum())
    assert blank > 1000
