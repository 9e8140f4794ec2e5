"""CPU: the host half of self copy-paste (INPUT.USE_COPY_METHOD 'self_copy' / 'both' / 'p:<f>').
(a) the numpy restatement (tests/_selfcopy_ref.py) equals the reference's own CopyPaste.__call__ outputs (tests/golden/self_copy.npz),
    and numpy draws the recorded m / sel from the recorded seed;
(b) CopyPasteMapper on a generated mini split consumes np.random in the reference's order (mapper.py:873-936, custom_copypaste.py:393-411):
    destination, index, [rand], source through the same mapper, [pool], randint, choice;
(c) pack_sample / unpack_sample: a sample with a self-copy source round-trips; a 'syn_copy' sample packs to exactly the seven sections
    it always had;
(d) everything of the self-copy branch that is not built is refused at start-up by key -- and only under a self-copy method.
All comparisons are exact equality."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _selfcopy_ref as SR  # noqa: E402

CASES = ["equal", "grow_h", "grow_w", "grow_both", "src_cropped", "m0", "ns0", "filter", "n0_0", "both"]


def test_restatement_equals_reference_golden():
    z = np.load(os.path.join(GOLD, "self_copy.npz"))
    assert [str(c) for c in z["cases"]] == CASES
    grown = set()
    for c in CASES:
        g = lambda k: z["%s_%s" % (c, k)]      # noqa: E731
        ns = len(g("src_masks"))
        np.random.seed(int(g("seed")))                         # _select_object's draws
        m = np.random.randint(0, min(ns + 1, 100))
        sel = np.random.choice(ns, size=m, replace=False)
        assert m == int(g("m")) and np.array_equal(sel, g("sel")), c
        r = SR.self_copy(g("dst_image"), g("dst_masks"), g("dst_boxes"), g("dst_labels"), g("src_image"), g("src_masks"), g("src_boxes"),
                         g("src_labels"), sel)
        assert np.array_equal(r["image"], g("out_image")) and r["image"].dtype == np.uint8, c
        assert np.array_equal(r["masks"], g("out_masks")), c
        assert np.array_equal(r["boxes"], g("out_boxes")) and r["boxes"].dtype == np.float32, c
        assert np.array_equal(r["labels"], g("out_labels")), c
        assert tuple(r["image"].shape[-2:]) == tuple(g("out_hw"))
        h1, w1 = g("dst_image").shape[-2:]
        grown.add((int(g("out_hw")[0]) > h1, int(g("out_hw")[1]) > w1))
    assert grown == {(False, False), (True, False), (False, True), (True, True)}
    assert z["filter_out_labels"].tolist()[:4] == [102, 103, 104, 105]          # dropped: fully covered, small remainder with a moved box


def _cfg(tmp_path, method, extra=()):
    from tests.test_gpu_loader import _mini_cfg
    return _mini_cfg(tmp_path, 128, 0, ["INPUT.USE_COPY_METHOD", method] + list(extra))


def _mapper(cfg, info, monkeypatch, seed=None):
    from divergen_amd.data import build as B
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
    mapper = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    mapper.set_dataset(dicts)
    mapper.pack = False
    if seed is not None and mapper.inst_pool is not None:
        mapper.inst_pool.seed(seed)
    return mapper, dicts


@pytest.mark.parametrize("method", ["self_copy", "both", "p:0.5"])
def test_mapper_consumes_np_random_in_reference_order(tmp_path, monkeypatch, method):
    from divergen_amd.data import build as B
    cfg, info = _cfg(tmp_path, method)
    mapper, dicts = _mapper(cfg, info, monkeypatch, seed=1)
    hand, _ = _mapper(cfg, info, monkeypatch, seed=1)          # its DatasetMapper / InstPool, driven by hand below
    assert (mapper.inst_pool is None) == (method == "self_copy")
    took_self = took_syn = pasted = 0
    for k in range(10):
        d = dicts[k % len(dicts)]
        np.random.seed(100 + k)
        got = mapper(d)
        after_got = np.random.rand()
        # ---- the reference's order, by hand
        np.random.seed(100 + k)
        dst = hand.mapper(d)
        idx = np.random.randint(0, len(dicts))
        self_branch = True
        if method.startswith("p:"):
            self_branch = np.random.rand() < 0.5
        src = hand.mapper(dicts[idx]) if self_branch else None
        if method == "both" or not self_branch:
            dst = hand.inst_pool.prepare(dst)
        if self_branch:
            ns = len(src["instances"])
            m = np.random.randint(0, min(ns + 1, 100))
            sel = np.random.choice(ns, size=m, replace=False)
        assert after_got == np.random.rand(), (method, k)
        # ---- and what the mapper hands over
        assert torch.equal(got["image"], dst["image"]) and torch.equal(got["instances"].gt_masks.tensor, dst["instances"].gt_masks.tensor)
        assert ("paste_pack" in got) == ("paste_pack" in dst)
        if "paste_pack" in dst:
            for key in ("flat", "desc", "labels"):
                assert torch.equal(got["paste_pack"][key], dst["paste_pack"][key])
            took_syn += 1
        assert ("scp_src" in got) == self_branch
        if self_branch:
            took_self += 1
            s, si = got["scp_src"], src["instances"]
            assert got["scp_file_name"] == src["file_name"] and len(s["labels"]) == m
            h1, w1 = dst["image"].shape[-2:]
            if m:
                pasted += m
                st = torch.from_numpy(sel)
                H, W = SR.canvas_hw((h1, w1), si.gt_boxes.tensor[st].numpy())
                assert tuple(s["hw"]) == (H, W)
                assert torch.equal(s["boxes"], si.gt_boxes.tensor[st]) and torch.equal(s["labels"], si.gt_classes[st])
                assert torch.equal(s["masks"], si.gt_masks.tensor.view(torch.uint8)[st][:, :H, :W])
                assert torch.equal(s["image"], src["image"][:, :H, :W])
            else:
                assert tuple(s["hw"]) == (h1, w1) and s["masks"].shape[0] == 0
    assert took_self > 0 and pasted > 0
    if method == "self_copy":
        assert took_syn == 0
    elif method == "both":
        assert took_syn == took_self == 10
    else:
        assert took_syn > 0 and took_syn + took_self == 10


def test_p_one_always_and_p_zero_never_self_copies(tmp_path, monkeypatch):
    for method, want in (("p:1.0", True), ("p:0.0", False)):
        cfg, info = _cfg(tmp_path / method.replace(":", "_"), method)
        mapper, dicts = _mapper(cfg, info, monkeypatch, seed=2)
        np.random.seed(7)
        for k in range(8):
            got = mapper(dicts[k])
            assert ("scp_src" in got) == want and ("paste_pack" in got) == (not want)


def _sections(layout, blob):
    out = {}
    for name, dt, shape, off in layout:
        dtype = getattr(torch, dt)
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        out[name] = blob[off:off + n].view(dtype).view(shape)
    return out


def test_pack_unpack_with_and_without_source_section(tmp_path, monkeypatch):
    from divergen_amd.data import build as B
    cfg, info = _cfg(tmp_path, "both")
    mapper, dicts = _mapper(cfg, info, monkeypatch, seed=3)
    np.random.seed(12)
    n_src = 0
    for k in range(6):
        raw = mapper(dicts[k])
        packed = B.pack_sample(dict(raw))
        names = [x[0] for x in packed["blob_layout"]]
        assert names == ["image", "gt_masks", "gt_boxes", "gt_classes", "flat", "desc", "labels", "scp_image", "scp_masks", "scp_boxes", "scp_labels"]
        assert all(x[3] % 64 == 0 for x in packed["blob_layout"]) and "scp_src" not in packed and "image" not in packed
        back = B.unpack_sample(packed, torch.device("cpu"))
        assert torch.equal(back["image"], raw["image"])
        bi, ri = back["instances"], raw["instances"]
        assert torch.equal(bi.gt_masks.tensor, ri.gt_masks.tensor) and torch.equal(bi.gt_boxes.tensor, ri.gt_boxes.tensor)
        assert torch.equal(bi.gt_classes, ri.gt_classes) and bi.image_size == ri.image_size
        for key in ("flat", "desc", "labels"):
            assert torch.equal(back["paste_pack"][key], raw["paste_pack"][key])
        assert back["paste_pack"]["K"] == raw["paste_pack"]["K"]
        for key in ("image", "masks", "boxes", "labels"):
            assert torch.equal(back["scp_src"][key], raw["scp_src"][key]) and back["scp_src"][key].dtype == raw["scp_src"][key].dtype
        assert tuple(back["scp_src"]["hw"]) == tuple(raw["scp_src"]["hw"]) and back["scp_file_name"] == raw["scp_file_name"]
        n_src += int(raw["scp_src"]["labels"].shape[0])
    assert n_src > 0
    # 'syn_copy': no source section -- the blob and the dict are what they always were (bytes and layout assembled by hand here)
    cfg, info = _cfg(tmp_path / "syn", "syn_copy")
    mapper, dicts = _mapper(cfg, info, monkeypatch, seed=3)
    np.random.seed(12)
    raw = mapper(dicts[0])
    assert "scp_src" not in raw and raw["paste_pack"]["K"] >= 0
    packed = B.pack_sample(dict(raw))
    inst, pk = raw["instances"], raw["paste_pack"]
    tensors = [("image", raw["image"]), ("gt_masks", inst.gt_masks.tensor.view(torch.uint8)), ("gt_boxes", inst.gt_boxes.tensor),
               ("gt_classes", inst.gt_classes), ("flat", pk["flat"]), ("desc", pk["desc"]), ("labels", pk["labels"])]
    layout, chunks, off = [], [], 0
    for name, t in tensors:
        b = t.contiguous().view(-1).view(torch.uint8) if t.numel() else torch.zeros(0, dtype=torch.uint8)
        layout.append((name, str(t.dtype).replace("torch.", ""), tuple(t.shape), off))
        chunks += [b, torch.zeros((-b.numel()) % 64, dtype=torch.uint8)]
        off += b.numel() + (-b.numel()) % 64
    assert packed["blob_layout"] == layout and len(layout) == len(B._BLOB_FIELDS) == 7
    assert torch.equal(packed["blob"], torch.cat(chunks))
    expect_keys = (set(raw) - {"image", "instances", "paste_pack"}) | {"blob", "blob_layout", "blob_hw", "blob_K"}
    if np.asarray(pk["modes"]).any():
        expect_keys.add("blob_modes")
    assert set(packed) == expect_keys
    back = B.unpack_sample(packed, torch.device("cpu"))
    assert "scp_src" not in back and torch.equal(back["paste_pack"]["flat"], pk["flat"])


REFUSED = [("INPUT.SCP_TYPE", "in_domain"), ("INPUT.SCP_NUM_SRC", 2), ("INPUT.SCP_SRC_OBJ_SELECT", False), ("INPUT.BLANK_RATIO", 0.3),
           ("INPUT.ROTATE_SRC", True), ("INPUT.LIMIT_SRC_LSJ", True), ("INPUT.RM_BG_PROB", 0.5), ("INPUT.SCP_RFS", True),
           ("INPUT.USE_INSTABOOST", True), ("INPUT.USE_COLOR_JITTER", True), ("INPUT.ACTIVE_SELECT", True)]


def test_refusals_name_the_key_and_only_under_a_self_copy_method(tmp_path, monkeypatch):
    from divergen_amd.data import build as B
    cfg, info = _cfg(tmp_path, "syn_copy")
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])

    def build(method, key=None, value=None):
        c = cfg.clone()
        c.defrost()
        c.merge_from_list(["INPUT.USE_COPY_METHOD", method] + ([key, value] if key else []))
        return B.CopyPasteMapper(B.DatasetMapper(c, True), c)
    for method in ("self_copy", "both", "p:0.25"):
        m = build(method)
        assert m.self_prob == (0.25 if method.startswith("p:") else 1.0)
        for key, value in REFUSED:
            with pytest.raises(NotImplementedError, match=key.split(".")[1]):
                build(method, key, value)
    for key, value in REFUSED:                                  # the same keys start as they always did under 'syn_copy' / 'none'
        if key == "INPUT.SCP_NUM_SRC" or key == "INPUT.ACTIVE_SELECT":
            assert build("syn_copy", key, value).self_prob is None
            continue
        assert build("syn_copy", key, value).self_prob is None and build("none", key, value).self_prob is None
    for bad in ("p:", "p:abc", "p:1.5", "p:-0.1", "p:nan"):
        with pytest.raises(ValueError, match="USE_COPY_METHOD"):
            build(bad)
    with pytest.raises(NotImplementedError, match="USE_COPY_METHOD"):
        build("self")
    with pytest.raises(NotImplementedError):                    # 'possion' stays refused whatever the copy method
        build("both", "INPUT.CP_METHOD", ["possion"])


def test_finish_refuses_a_self_copy_without_the_gpu(tmp_path, monkeypatch):
    """No quiet fall-back: the paste itself is dgx_self_copy_paste; on a CPU device finish() raises instead of skipping it."""
    cfg, info = _cfg(tmp_path, "self_copy")
    mapper, dicts = _mapper(cfg, info, monkeypatch)
    np.random.seed(3)
    with pytest.raises(RuntimeError, match="dgx_self_copy_paste"):
        mapper.finish(mapper(dicts[0]), "cpu")
