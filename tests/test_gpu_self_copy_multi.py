"""GPU: self copy-paste from several source images (INPUT.SCP_NUM_SRC > 1 with INPUT.SCP_MULTI_SRC).  dgx_self_copy_merge +
dgx_self_copy_paste_merged through layers.self_copy_merge / self_copy_paste_multi, bit-exact (torch.equal / np.array_equal, no tolerance
anywhere) against the reference's own CopyPaste.__call__ outputs (tests/golden/self_copy_multi.npz: image, masks, boxes, labels, the
validity of every merged plane and of every destination object) and against the numpy restatement (tests/_selfcopy_multi_ref.py) on
ragged geometries with more than one workgroup group of accumulator planes, and with more than 99 survivors; two runs give the same bytes;
every output byte of the valid rows written; argument errors; a loader-fed sample through finish(); nothing new runs with the key off.
Reference: DG/divergen/data/transforms/custom_copypaste.py:274-297, :343-389, :428-506."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _selfcopy_multi_ref as MR  # noqa: E402
import _selfcopy_ref as SR  # noqa: E402
from test_host_self_copy_multi import CASES, golden_case  # noqa: E402


def _gpu(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_paste_equal(out, ref, n0):
    """out: self_copy_paste_multi(lazy_masks=True); ref: dict(image, masks, boxes, labels, valid) of numpy arrays."""
    keep = out["keep"]
    assert torch.equal(out["image"], _t(ref["image"]))
    assert torch.equal(out["masks"].index_select(0, keep), _t(ref["masks"]))
    assert torch.equal(out["boxes"], _t(ref["boxes"])) and out["boxes"].dtype == torch.float32
    assert torch.equal(out["labels"], _t(ref["labels"]))
    dst_valid = torch.zeros(n0, dtype=torch.bool, device="cuda")
    dst_valid[keep[keep < n0]] = True
    assert torch.equal(dst_valid, _t(np.asarray(ref["valid"]).astype(bool)))


def _assert_merge_equal(acc, ref):
    """acc: layers.self_copy_merge; ref: _selfcopy_multi_ref.merge -- the accumulator = the valid rows, at the bounding size."""
    Hb, Wb = acc["image"].shape[-2:]
    assert torch.equal(acc["valid"].bool(), _t(ref["valid"]))
    rows = acc["valid"].nonzero().squeeze(1)
    assert torch.equal(acc["image"], _t(SR.pad_to_hw(ref["image"], Hb, Wb)))
    assert torch.equal(acc["masks"].index_select(0, rows), _t(SR.pad_to_hw(ref["masks"], Hb, Wb)))
    assert torch.equal(acc["boxes"].index_select(0, rows), _t(ref["boxes"])) and torch.equal(acc["labels"].index_select(0, rows), _t(ref["labels"]))


@pytest.mark.parametrize("case", CASES)
def test_merge_and_paste_equal_reference_golden(case):
    from divergen_amd.layers import self_copy_merge, self_copy_paste_multi
    z = np.load(os.path.join(GOLD, "self_copy_multi.npz"))
    g, dst, sources = golden_case(z, case)
    out = self_copy_paste_multi(*_gpu(*dst), [tuple(_gpu(*s)) for s in sources], lazy_masks=True)
    _assert_paste_equal(out, dict(image=g("out_image"), masks=g("out_masks"), boxes=g("out_boxes"), labels=g("out_labels"),
                                  valid=g("dst_valid")), len(dst[1]))
    assert tuple(out["image"].shape[-2:]) == tuple(g("out_hw"))
    taken = [s for s in sources if len(s[2])]
    if len(taken) >= 2:                                        # the merge alone: validity of every selected plane as the reference had it
        acc = self_copy_merge([tuple(_gpu(*s)) for s in taken])
        assert torch.equal(acc["valid"], _t(g("merge_valid")))
        _assert_merge_equal(acc, MR.merge(taken))
    else:
        assert case == "all_empty" and len(g("merge_valid")) == 0
    eager = self_copy_paste_multi(*_gpu(*dst), [tuple(_gpu(*s)) for s in sources])      # masks gathered
    assert "keep" not in eager and torch.equal(eager["masks"], _t(g("out_masks")))


def _scene(rng, n, h, w, big=False):
    """image, n blob masks (0/1 bytes; every ninth empty when n is large), boxes a little off the mask extents, labels."""
    from test_gpu_self_copy import _scene as scene
    img, masks, boxes, labels = scene(rng, n, h, w, big)
    boxes = (boxes + rng.uniform(-0.45, 0.45, boxes.shape) * (boxes.sum(1, keepdims=True) > 0)).clip(0).astype(np.float32)
    return img, masks, boxes, labels


# (destination size, [(m_i, source size), ...]): aligned and unaligned widths together, sources smaller and larger than each other,
# 70 + 45 accumulator planes (two workgroup groups of 64 at the last stage), a frame of several workgroups
RAGGED = [((64, 80), [(5, (64, 80)), (3, (64, 80))]),
          ((50, 37), [(4, (77, 101)), (6, (64, 80)), (2, (30, 24))]),
          ((96, 112), [(70, (60, 75)), (45, (72, 96)), (9, (66, 90))]),
          ((40, 48), [(3, (9, 33)), (2, (48, 64)), (31, (50, 61)), (1, (33, 47))]),
          ((300, 400), [(8, (260, 384)), (12, (288, 352))])]


def _ragged_problem(geom, seed):
    (h1, w1), srcs = geom
    rng = np.random.default_rng(seed)
    dst = _scene(rng, 6, h1, w1, big=True)
    sources = [_scene(rng, m, h, w, big=(i % 2 == 0)) for i, (m, (h, w)) in enumerate(srcs)]
    for s in sources:                                          # an object with an empty mask keeps a box: give it one inside the frame
        empty = s[2].sum(1) == 0
        s[2][empty] = np.array([1.5, 2.5, 7.25, 6.5], np.float32)
    return dst, sources


@pytest.mark.parametrize("geom", RAGGED)
def test_kernels_equal_restatement_on_ragged_sizes(geom):
    from divergen_amd.layers import self_copy_merge, self_copy_paste_multi
    dst, sources = _ragged_problem(geom, 7)
    ref = MR.self_copy_multi(*dst, sources)
    acc = self_copy_merge([tuple(_gpu(*s)) for s in sources])
    _assert_merge_equal(acc, ref["merge"])
    out = self_copy_paste_multi(*_gpu(*dst), [tuple(_gpu(*s)) for s in sources], lazy_masks=True)
    _assert_paste_equal(out, ref, len(dst[1]))


def _rect_source(rng, hw, rects, strays=()):
    """one rectangle (y0, y1, x0, x1) per object, boxes of the rectangles alone; strays (object, y, x): an 8 x 8 block the box leaves out"""
    masks = np.zeros((len(rects),) + hw, np.uint8)
    for i, (y0, y1, x0, x1) in enumerate(rects):
        masks[i, y0:y1, x0:x1] = 1
    boxes = np.array([[x0, y0, x1, y1] for y0, y1, x0, x1 in rects], np.float32)
    for i, y, x in strays:
        masks[i, y:y + 8, x:x + 8] = 1
    return rng.integers(0, 256, (3,) + hw, dtype=np.uint8), masks, boxes, rng.integers(0, 1203, len(rects)).astype(np.int64)


def test_merge_where_the_frame_alone_fills_the_chip():
    """Sources of 2048 x 2048: 2048 * 128 chunks are 1024 workgroups in x, so no kernel splits its planes over grid.y (one plane group),
    and stage 2 runs in place at that geometry.  Source 0 brings A, B, C, source 1 D, E, source 2 F, G.  Stage 1, canvas (1715, 1715)
    (no multiple of 16): D covers B whole (dropped); the blocks of A and D beyond the canvas are cut off.  Stage 2, in place, canvas
    (1730, 1730): F covers E whole (dropped), G takes the left of C, whose box moves by 250 with 75000 pixels left (kept)."""
    from divergen_amd.layers import self_copy_merge, self_copy_paste_multi
    rng = np.random.default_rng(2048)
    hw = (2048, 2048)
    sources = [_rect_source(rng, hw, [(100, 400, 100, 500), (600, 900, 600, 1000), (1200, 1500, 200, 700)], strays=[(0, 1800, 1800)]),
               _rect_source(rng, hw, [(550, 950, 550, 1050), (1700, 1715, 1700, 1715)], strays=[(0, 1900, 1900)]),
               _rect_source(rng, hw, [(1690, 1730, 1690, 1730), (1150, 1550, 150, 450)])]
    dst = _scene(rng, 6, 600, 800, big=True)
    ref = MR.self_copy_multi(*dst, sources)
    assert ref["merge"]["hw"] == [(1715, 1715), (1730, 1730)]
    valid = ref["merge"]["valid"]
    assert valid.tolist() == [True, False, True, True, False, True, True]      # B at stage 1, E at stage 2
    assert not valid[:5].all() and valid[:5].any()             # an accumulator object dropped, another kept
    acc = self_copy_merge([tuple(_gpu(*s)) for s in sources])
    _assert_merge_equal(acc, ref["merge"])
    out = self_copy_paste_multi(*_gpu(*dst), [tuple(_gpu(*s)) for s in sources], lazy_masks=True)
    _assert_paste_equal(out, ref, len(dst[1]))


def _grid_source(rng, h, w, cells, label0):
    """one 6 x 6 square per listed cell of the 8 x 8 grid of an (h, w) frame: objects that cannot cover each other"""
    per_row = w // 8
    masks = np.zeros((len(cells), h, w), np.uint8)
    for i, c in enumerate(cells):
        y, x = (c // per_row) * 8, (c % per_row) * 8
        masks[i, y + 1:y + 7, x + 1:x + 7] = 1
    return rng.integers(0, 256, (3, h, w), dtype=np.uint8), masks, SR.mask_boxes(masks), label0 + np.arange(len(cells), dtype=np.int64)


def test_more_than_99_survivors_take_the_merged_entry():
    """Two sources of 60 and 55 objects on separate grid cells, a third whose one object covers twelve of the first source's (eleven are dropped; the one at
    the origin stays, empty: its box moves to zeros by 7 only): 105 planes reach the final paste, more than dgx_self_copy_paste takes -- dgx_self_copy_paste_merged's bound (99 per merged source)."""
    from divergen_amd.layers import self_copy_paste_multi
    rng = np.random.default_rng(99)
    h, w = 96, 112                                             # 12 x 14 cells
    cover = np.zeros((1, h, w), np.uint8)
    cover[0, :8, :96] = 1                                      # cells 0 .. 11 of source 0
    sources = [_grid_source(rng, h, w, list(range(60)), 100), _grid_source(rng, h, w, list(range(60, 115)), 200),
               (rng.integers(0, 256, (3, h, w), dtype=np.uint8), cover, SR.mask_boxes(cover), np.array([300]))]
    dst = _scene(rng, 6, 80, 100, big=True)
    ref = MR.self_copy_multi(*dst, sources)
    assert int(ref["merge"]["valid"].sum()) == 60 - 11 + 55 + 1 > 99
    out = self_copy_paste_multi(*_gpu(*dst), [tuple(_gpu(*s)) for s in sources], lazy_masks=True)
    _assert_paste_equal(out, ref, len(dst[1]))


def _raw_merge(sources, Hb, Wb, sentinel):
    """dgx_self_copy_merge itself, outputs pre-filled with a sentinel -> return code and the four outputs."""
    from divergen_amd import _lib as L
    S, M = len(sources), sum(len(s[2]) for s in sources)
    imgs, masks = [_t(s[0]) for s in sources], [_t(s[1]) for s in sources]
    counts = np.array([len(s[2]) for s in sources], np.int32)
    sizes = np.array([s[0].shape[-2:] for s in sources], np.int32)
    boxes = _t(np.concatenate([s[2] for s in sources]).astype(np.float32))
    oi = torch.full((3, Hb, Wb), sentinel, dtype=torch.uint8, device="cuda")
    om = torch.full((max(M, 1), Hb, Wb), sentinel, dtype=torch.uint8, device="cuda")
    ob = torch.full((max(M, 1), 4), -7.0, dtype=torch.float32, device="cuda")
    ov = torch.full((max(M, 1),), sentinel, dtype=torch.uint8, device="cuda")
    words = int(L.lib().dgx_self_copy_merge_workspace_words(S, M, Hb, Wb))
    work = torch.empty(max(words, 16), dtype=torch.int32, device="cuda")
    arr = lambda ts: (ctypes.c_void_p * max(S, 1))(*[t.data_ptr() for t in ts])      # noqa: E731
    rc = L.lib().dgx_self_copy_merge(arr(imgs), arr(masks), counts.ctypes.data, sizes.ctypes.data, S, boxes.data_ptr(), Hb, Wb,
                                     oi.data_ptr(), om.data_ptr(), ob.data_ptr(), ov.data_ptr(), work.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return rc, oi, om[:M], ob[:M], ov[:M], words


@pytest.mark.parametrize("geom", [RAGGED[1], RAGGED[3]])
def test_every_output_byte_of_the_accumulator_is_written(geom):
    dst, sources = _ragged_problem(geom, 11)
    ref = MR.merge(sources)
    Hb, Wb = max(s[0].shape[1] for s in sources), max(s[0].shape[2] for s in sources)
    for sentinel in (0xA5, 0x01):          # two fills: a byte the kernels left alone cannot equal both
        rc, oi, om, ob, ov, words = _raw_merge(sources, Hb, Wb, sentinel)
        assert rc == 0 and words > 0
        assert set(ov.cpu().tolist()) <= {0, 1}
        _assert_merge_equal(dict(image=oi, masks=om, boxes=ob, valid=ov, labels=_t(np.concatenate([s[3] for s in sources]))), ref)


def test_two_runs_are_bit_identical():
    from divergen_amd.layers import self_copy_merge
    for geom in (RAGGED[2], RAGGED[4]):
        _, sources = _ragged_problem(geom, 3)
        dev = [tuple(_gpu(*s)) for s in sources]
        a, b = self_copy_merge(dev), self_copy_merge(dev)
        torch.cuda.synchronize()
        for k in ("image", "masks", "boxes", "labels", "valid"):      # every row, the dropped objects' included
            assert torch.equal(a[k], b[k]), k


def test_bad_arguments():
    from divergen_amd import _lib as L
    from divergen_amd.layers import self_copy_merge, self_copy_paste
    rng = np.random.default_rng(6)
    s = [_scene(rng, 3, 32, 48) for _ in range(5)]
    for bad in (s[:1], s):                                     # one source is not a merge; five are above the bound
        with pytest.raises(ValueError, match="2 to 4"):
            self_copy_merge([tuple(_gpu(*x)) for x in bad])
    none = (s[0][0], s[0][1][:0], s[0][2][:0], s[0][3][:0])
    with pytest.raises(ValueError, match="1 to 99"):
        self_copy_merge([tuple(_gpu(*s[0])), tuple(_gpu(*none))])
    assert _raw_merge(s[:2], 32, 48, 0)[0] == 0
    assert _raw_merge(s[:2], 31, 48, 0)[0] == -1               # a source larger than the outputs
    assert _raw_merge(s[:2], 32, 47, 0)[0] == -1
    assert _raw_merge(s[:1], 32, 48, 0)[0] == -1 and _raw_merge(s, 32, 48, 0)[0] == -1      # S outside [2, 4]
    big = _scene(rng, 100, 32, 48)
    assert _raw_merge([s[0], big], 32, 48, 0)[0] == -1         # m_i > 99
    assert L.lib().dgx_self_copy_merge_workspace_words(1, 4, 32, 48) == 0
    with pytest.raises(ValueError, match="at most 396"):       # the merged entry's bound, checked on the host like the plain one's
        self_copy_paste(*_gpu(*s[0]), *_gpu(*s[1]), np.zeros(397, np.int64), merged=True)
    with pytest.raises(L.DgxError):                            # no CPU fallback
        self_copy_merge([tuple(torch.from_numpy(a) for a in x) for x in s[:2]])


def _mapper(tmp_path, monkeypatch, extra):
    from divergen_amd.data import build as B
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 128, 0, ["INPUT.USE_COPY_METHOD", "self_copy"] + list(extra))
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
    mapper = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    mapper.set_dataset(dicts)
    return mapper, dicts


def test_loader_fed_sample_with_two_sources_equals_restatement(tmp_path, monkeypatch):
    """CopyPasteMapper with SCP_NUM_SRC 2: the worker half (one blob per sample), then finish() on the GPU == the restatement applied
    to what the same draws give unpacked; the Instances carry gt_boxes / gt_classes / gt_masks only."""
    mapper, dicts = _mapper(tmp_path, monkeypatch, ["INPUT.SCP_NUM_SRC", 2, "INPUT.SCP_MULTI_SRC", True])
    plain, _ = _mapper(tmp_path, monkeypatch, ["INPUT.SCP_NUM_SRC", 2, "INPUT.SCP_MULTI_SRC", True])
    plain.pack = False
    merged = 0
    for k in range(12):
        np.random.seed(40 + k)
        packed = mapper(dicts[k % len(dicts)])
        assert "blob" in packed and "scp_src" not in packed
        have = mapper.finish(packed, "cuda")
        np.random.seed(40 + k)
        raw = plain(dicts[k % len(dicts)])
        scp = raw["scp_src"]
        groups = scp if isinstance(scp, list) else [scp]
        ri = raw["instances"]
        ref = MR.self_copy_multi(raw["image"].numpy(), ri.gt_masks.tensor.numpy().astype(np.uint8), ri.gt_boxes.tensor.numpy(),
                                 ri.gt_classes.numpy(), [tuple(g[key].numpy() for key in ("image", "masks", "boxes", "labels")) for g in groups])
        hi = have["instances"]
        assert sorted(hi.get_fields()) == ["gt_boxes", "gt_classes", "gt_masks"] and "scp_src" not in have
        assert torch.equal(have["image"], _t(ref["image"])) and torch.equal(hi.gt_masks.tensor.view(torch.uint8), _t(ref["masks"]))
        assert torch.equal(hi.gt_boxes.tensor, _t(ref["boxes"])) and torch.equal(hi.gt_classes, _t(ref["labels"]))
        assert (have["height"], have["width"]) == tuple(have["image"].shape[-2:]) == tuple(hi.image_size)
        merged += int(isinstance(scp, list))
    assert merged > 0


def test_with_the_key_off_nothing_new_is_called(tmp_path, monkeypatch):
    """SCP_NUM_SRC 1 without INPUT.SCP_MULTI_SRC: finish() runs dgx_self_copy_paste alone -- the new entries are never reached."""
    from divergen_amd import _lib as L
    mapper, dicts = _mapper(tmp_path, monkeypatch, [])
    called = []
    for name in ("dgx_self_copy_merge", "dgx_self_copy_paste_merged", "dgx_self_copy_merge_workspace_words"):
        monkeypatch.setattr(L.lib(), name, lambda *a, _n=name: called.append(_n) or -1)
    real = L.lib().dgx_self_copy_paste
    monkeypatch.setattr(L.lib(), "dgx_self_copy_paste", lambda *a: called.append("dgx_self_copy_paste") or real(*a))
    pasted = 0
    for k in range(6):
        np.random.seed(60 + k)
        packed = mapper(dicts[k])
        assert "blob_scp_n" not in packed and [x[0] for x in packed["blob_layout"]][-4:] == ["scp_image", "scp_masks", "scp_boxes", "scp_labels"]
        pasted += int(dict((x[0], x[2]) for x in packed["blob_layout"])["scp_labels"][0] > 0)
        mapper.finish(packed, "cuda")
    torch.cuda.synchronize()
    assert pasted > 0 and set(called) == {"dgx_self_copy_paste"} and len(called) == pasted
