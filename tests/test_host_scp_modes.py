"""CPU: the host half of INPUT.SCP_SRC_MODES (INPUT.SCP_TYPE 'in_domain' / 'cas' / 'the_cls' / 'the_cls_img', a source pasted whole,
INPUT.RM_BG_PROB under every copy method).
(a) the numpy restatement (tests/_scp_modes_ref.py) equals the reference's own CopyPaste(selected=False).__call__ and
    CopyPaste.remove_background outputs (tests/golden/scp_modes.npz);
(b) with the key off nothing moves: the refusals keep their words, RM_BG_PROB under 'syn_copy' draws nothing and changes no byte;
(c) with the key on: what is admitted, what is still refused and how the message names it;
(d) per_cat_map and the per-category source draws equal what the reference's own set_dataset / _filter_in_specific_cls produced on the
    same synthetic dataset (golden; all four types, the empty destination of 'in_domain');
(e) the worker consumes np.random in the reference's order (mapper.py:869-936): destination, rm_bg, indices, [rand], sources, [pool],
    [selection], checked on the generator's state after the call;
(f) the blob: `rm_bg` only when drawn, a source of 130 objects pasted whole, the 'in_domain' sample without any source.
Every piece of the golden comes from the reference's real code; nothing is pinned by a restatement alone.  All comparisons are exact."""
import copy
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _scp_modes_ref as MR  # noqa: E402

PASTE_ALL_CASES = ["ragged_a", "ragged_b", "ragged_c", "big130_n0", "big130_n70", "ns0", "n0_0", "both"]
KEY = ["INPUT.SCP_SRC_MODES", True]


def _gold():
    return np.load(os.path.join(GOLD, "scp_modes.npz"))


def test_restatement_equals_reference_golden():
    z = _gold()
    assert [str(c) for c in z["paste_all_cases"]] == PASTE_ALL_CASES
    for c in PASTE_ALL_CASES + ["rb_then_paste"]:
        g = lambda k: z["%s_%s" % (c, k)]      # noqa: E731
        first = MR.remove_background(g("dst_image"), g("dst_masks")) if c == "rb_then_paste" else g("dst_image")      # background first
        r = MR.paste_all(first, g("dst_masks"), g("dst_boxes"), g("dst_labels"), g("src_image"), g("src_masks"), g("src_boxes"), g("src_labels"))
        assert np.array_equal(r["image"], g("out_image")) and r["image"].dtype == np.uint8, c
        assert np.array_equal(r["masks"], g("out_masks")), c
        assert np.array_equal(r["boxes"], g("out_boxes")) and r["boxes"].dtype == np.float32, c
        assert np.array_equal(r["labels"], g("out_labels")), c
        assert tuple(r["image"].shape[-2:]) == tuple(g("out_hw"))
    assert len(z["big130_n70_src_masks"]) == 130 and len(z["big130_n70_dst_masks"]) == 70
    kept = z["big130_n70_out_labels"][:-130].tolist()
    assert 2000 not in kept and 2001 in kept            # the occlusion filter drops and keeps
    assert [str(c) for c in z["rb_cases"]] == ["rb_plain", "rb_overlap", "rb_n0"]
    for c in z["rb_cases"]:
        assert np.array_equal(MR.remove_background(z["%s_image" % c], z["%s_masks" % c]), z["%s_out" % c]), c
    assert not z["rb_n0_out"].any() and z["rb_n0_masks"].shape[0] == 0


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


def _builder(tmp_path, monkeypatch):
    from divergen_amd.data import build as B
    cfg, info = _cfg(tmp_path, "syn_copy")
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])

    def build(method, *pairs):
        c = cfg.clone()
        c.defrost()
        c.merge_from_list(["INPUT.USE_COPY_METHOD", method] + list(pairs))
        return B.CopyPasteMapper(B.DatasetMapper(c, True), c)
    return build


UNTOUCHED = [("INPUT.SCP_NUM_SRC", 2), ("INPUT.BLANK_RATIO", 0.3), ("INPUT.ROTATE_SRC", True), ("INPUT.LIMIT_SRC_LSJ", True), ("INPUT.SCP_RFS", True),
             ("INPUT.USE_INSTABOOST", True), ("INPUT.USE_COLOR_JITTER", True), ("INPUT.ACTIVE_SELECT", True)]


def test_key_off_keeps_every_refusal_word_for_word(tmp_path, monkeypatch):
    build = _builder(tmp_path, monkeypatch)
    words = {("INPUT.SCP_TYPE", "in_domain"): "INPUT.SCP_TYPE 'in_domain' with INPUT.USE_COPY_METHOD 'both': only '' (a random training image as the source)",
             ("INPUT.SCP_SRC_OBJ_SELECT", False): "INPUT.SCP_SRC_OBJ_SELECT False with INPUT.USE_COPY_METHOD 'both': only True",
             ("INPUT.RM_BG_PROB", 0.5): "INPUT.RM_BG_PROB 0.5 with INPUT.USE_COPY_METHOD 'both': background removal is not built"}
    for (key, value), text in words.items():
        for off in ([], ["INPUT.SCP_SRC_MODES", False]):
            with pytest.raises(NotImplementedError) as e:
                build("both", key, value, *off)
            assert str(e.value) == text
    for key, value in UNTOUCHED:                                # the key does not touch the other refusals
        said = []
        for extra in (["INPUT.SCP_SRC_MODES", False], KEY):
            with pytest.raises(NotImplementedError, match=key.split(".")[1]) as e:
                build("both", key, value, *extra)
            said.append(str(e.value))
        assert said[0] == said[1], key
    m = build("syn_copy", "INPUT.RM_BG_PROB", 0.5, "INPUT.SCP_TYPE", "cas", "INPUT.SCP_SRC_OBJ_SELECT", False)      # ignored there, as always
    assert m.rm_bg_prob == 0 and m.scp_type == "" and not m.paste_all and not m.src_modes


def test_key_off_rm_bg_prob_under_syn_copy_draws_nothing(tmp_path, monkeypatch):
    from divergen_amd.data import build as B
    packed, states = [], []
    for sub, extra in (("plain", []), ("rm", ["INPUT.RM_BG_PROB", 0.5])):
        cfg, info = _cfg(tmp_path / sub, "syn_copy", ["INPUT.SCP_SRC_MODES", False] + extra)
        mapper, dicts = _mapper(cfg, info, monkeypatch, seed=4)
        np.random.seed(21)
        packed.append([B.pack_sample(dict(mapper(dicts[k]))) for k in range(4)])
        states.append(np.random.get_state())
    assert np.array_equal(states[0][1], states[1][1]) and states[0][2] == states[1][2]
    for a, b in zip(*packed):
        assert set(a) == set(b) and "rm_bg" not in a and a["blob_layout"] == b["blob_layout"] and torch.equal(a["blob"], b["blob"])


def test_key_on_admits_and_refuses(tmp_path, monkeypatch):
    build = _builder(tmp_path, monkeypatch)
    for method in ("self_copy", "both", "p:0.25"):
        for t in ("in_domain", "cas"):
            m = build(method, "INPUT.SCP_TYPE", t, *KEY)
            assert m.scp_type == t and m.paste_all
        for t in ("the_cls", "the_cls_img"):
            m = build(method, "INPUT.SCP_TYPE", t, "INPUT.SCP_SELECT_CATS_LIST", [3, 4], *KEY)
            assert m.scp_type == t and not m.paste_all and m.select_cats == [3, 4]
        assert build(method, "INPUT.SCP_TYPE", "the_cls", "INPUT.SCP_SELECT_CATS_LIST", [3], "INPUT.SCP_SRC_OBJ_SELECT", False, *KEY).paste_all
        m = build(method, "INPUT.SCP_SRC_OBJ_SELECT", False, "INPUT.RM_BG_PROB", 1.0, *KEY)
        assert m.paste_all and m.scp_type == "" and m.rm_bg_prob == 1.0
        m = build(method, *KEY)                                  # the key alone changes nothing
        assert not m.paste_all and m.scp_type == "" and m.rm_bg_prob == 0
        # selected sources of a type merge like any others
        m = build(method, "INPUT.SCP_TYPE", "the_cls", "INPUT.SCP_SELECT_CATS_LIST", [1, 2, 3], "INPUT.SCP_NUM_SRC", 3, "INPUT.SCP_MULTI_SRC", True, *KEY)
        assert m.num_src == 3 and not m.paste_all
        for t in ("rc_only", "f_only"):
            with pytest.raises(NotImplementedError, match="SCP_TYPE.*reference's own mapper.*raises NotImplementedError"):
                build(method, "INPUT.SCP_TYPE", t, *KEY)
        with pytest.raises(NotImplementedError, match="SCP_TYPE 'nearest'"):
            build(method, "INPUT.SCP_TYPE", "nearest", *KEY)
        with pytest.raises(ValueError, match="RM_BG_PROB"):
            build(method, "INPUT.RM_BG_PROB", 1.5, *KEY)
        for t in ("the_cls", "the_cls_img"):
            with pytest.raises(ValueError, match="SCP_SELECT_CATS_LIST"):
                build(method, "INPUT.SCP_TYPE", t, *KEY)
            with pytest.raises(ValueError, match="SCP_SELECT_CATS_LIST.*SCP_NUM_SRC 3"):
                build(method, "INPUT.SCP_TYPE", t, "INPUT.SCP_SELECT_CATS_LIST", [1, 2], "INPUT.SCP_NUM_SRC", 3, "INPUT.SCP_MULTI_SRC", True, *KEY)
        for pairs, named in ((["INPUT.SCP_TYPE", "in_domain"], "SCP_TYPE"), (["INPUT.SCP_TYPE", "cas"], "SCP_TYPE"),
                             (["INPUT.SCP_SRC_OBJ_SELECT", False], "SCP_SRC_OBJ_SELECT")):
            with pytest.raises(NotImplementedError, match="INPUT.SCP_NUM_SRC 2 with INPUT.%s" % named):      # names both keys
                build(method, *pairs, "INPUT.SCP_NUM_SRC", 2, "INPUT.SCP_MULTI_SRC", True, *KEY)
        with pytest.raises(NotImplementedError, match="ACTIVE_SELECT"):      # (refused with a self-copy method anyway, in its old words)
            build(method, "INPUT.RM_BG_PROB", 0.5, "INPUT.ACTIVE_SELECT", True, *KEY)
    # RM_BG_PROB is no self-copy switch: it applies (and is checked) under 'syn_copy' / 'none' too
    for method in ("syn_copy", "none"):
        assert build(method, "INPUT.RM_BG_PROB", 0.5, *KEY).rm_bg_prob == 0.5
        assert build(method, "INPUT.RM_BG_PROB", 0.5, "INPUT.SCP_TYPE", "rc_only", *KEY).scp_type == ""      # no self copy, no type
        with pytest.raises(ValueError, match="RM_BG_PROB"):
            build(method, "INPUT.RM_BG_PROB", 1.01, *KEY)
    with pytest.raises(NotImplementedError, match="RM_BG_PROB.*ACTIVE_SELECT"):
        build("syn_copy", "INPUT.RM_BG_PROB", 0.5, "INPUT.ACTIVE_SELECT", True, *KEY)
    assert build("syn_copy", "INPUT.ACTIVE_SELECT", True, *KEY).active_select          # without RM_BG_PROB BSGAL starts as it did


def _bare_mapper(**attrs):
    from divergen_amd.data import build as B
    m = B.CopyPasteMapper.__new__(B.CopyPasteMapper)
    m.active_select, m.inst_pool, m.pack, m.ring = False, None, False, None
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_per_cat_map_and_source_draws_equal_the_reference(tmp_path):
    z = _gold()
    cats = json.loads(str(z["cls_dataset_cats"]))
    dataset = [{"file_name": "img%d" % i, "image_id": i, "annotations": [{"category_id": c, "id": 100 * i + k} for k, c in enumerate(cs)]}
               for i, cs in enumerate(cats)]
    frozen = copy.deepcopy(dataset)
    draws, calls = int(z["cls_mapper_draws"]), []

    def stand_in(d):
        calls.append((int(d["file_name"][3:]), [a["category_id"] for a in d["annotations"]]))
        np.random.rand(draws)
        return d
    cases = json.loads(str(z["cls_cases"]))
    assert {c["type"] for c in cases} == {"in_domain", "cas", "the_cls", "the_cls_img"} and {c["num_src"] for c in cases} == {1, 3}
    assert any(c["type"] == "in_domain" and c["dst_classes"] == [] and c["indices"] == [] for c in cases)
    for c in cases:
        m = _bare_mapper(scp_type=c["type"], num_src=c["num_src"], mapper=stand_in, select_cats=z["cls_select_cats"].tolist())
        m.set_dataset(dataset)
        assert [[k, v] for k, v in m.per_cat_map.items()] == json.loads(str(z["cls_per_cat_map"]))      # key order too ('cas' draws from it)
        del calls[:]
        np.random.seed(c["seed"])
        got = m._class_sources({"instances": types.SimpleNamespace(gt_classes=torch.tensor(c["dst_classes"], dtype=torch.int64))})
        assert np.random.rand() == c["after"], c
        assert [i for i, _ in calls] == c["indices"] and [a for _, a in calls] == c["mapped_cats"], c
        assert len(got) == len(c["indices"])
    assert dataset == frozen                                    # sources are filtered on deep copies


def _per_cat(dicts):
    pcm = {}
    for i, d in enumerate(dicts):
        for cid in set([a["category_id"] for a in d["annotations"]]):
            pcm.setdefault(cid, []).append(i)
    return pcm


def _replay(hand, dicts, d, method, scp_type, num_src, p_rm, select_cats, whole):
    """The documented order, by hand, on the second mapper's DatasetMapper / InstPool."""
    dst = hand.mapper(d)
    rm = bool(np.random.uniform(0.0, 1.0) <= p_rm) if p_rm > 0 else False
    idxs = [np.random.randint(0, len(dicts)) for _ in range(num_src)]
    take_self = np.random.rand() < float(method[2:]) if method.startswith("p:") else True
    srcs, pcm = [], _per_cat(dicts)
    if take_self and scp_type == "":
        srcs = [hand.mapper(dicts[i]) for i in idxs]
    elif take_self:
        pools = []
        if scp_type == "in_domain":
            cls_list = list(set(dst["instances"].gt_classes.tolist()))
            mine = [pcm[c] for c in cls_list]
            if mine:
                pools = [mine[np.random.randint(0, len(mine))] for _ in range(num_src)]
        else:
            cls_list = np.random.choice(list(pcm.keys()) if scp_type == "cas" else select_cats, num_src, replace=False)
            pools = [pcm[c] for c in cls_list]
        for pool in pools:
            dd = copy.deepcopy(dicts[pool[np.random.randint(0, len(pool))]])
            if scp_type != "the_cls_img":
                dd["annotations"] = [a for a in dd["annotations"] if a["category_id"] in cls_list]
            srcs.append(hand.mapper(dd))
    if hand.inst_pool is not None and (method == "both" or not take_self):
        dst = hand.inst_pool.prepare(dst)
    sels = []
    for src in srcs:
        ns = len(src["instances"])
        if whole:
            sels.append(np.arange(ns))
        else:
            m = np.random.randint(0, min(ns + 1, 100))
            sels.append(np.random.choice(ns, size=m, replace=False))
    return dst, rm, take_self, srcs, sels


ORDER = [("both", "in_domain", 1, 0.5, True), ("p:0.5", "the_cls", 1, 0.5, False), ("self_copy", "", 1, 1.0, True),
         ("both", "cas", 1, -1.0, True), ("self_copy", "the_cls_img", 2, 0.3, False)]


@pytest.mark.parametrize("method,scp_type,num_src,p_rm,whole", ORDER)
def test_worker_consumes_np_random_in_reference_order(tmp_path, monkeypatch, method, scp_type, num_src, p_rm, whole):
    probe, info = _cfg(tmp_path / "probe", "syn_copy")
    _, dicts = _mapper(probe, info, monkeypatch)
    select = sorted(_per_cat(dicts))[:3]
    extra = KEY + ["INPUT.SCP_TYPE", scp_type, "INPUT.RM_BG_PROB", p_rm, "INPUT.SCP_NUM_SRC", num_src, "INPUT.SCP_MULTI_SRC", num_src > 1,
                   "INPUT.SCP_SELECT_CATS_LIST", select, "INPUT.SCP_SRC_OBJ_SELECT", not (whole and scp_type == "")]
    cfg, info = _cfg(tmp_path, method, extra)
    mapper, dicts = _mapper(cfg, info, monkeypatch, seed=1)
    hand, _ = _mapper(cfg, info, monkeypatch, seed=1)
    assert mapper.paste_all == whole and mapper.scp_type == scp_type
    seen = {"rm": 0, "plain": 0, "self": 0, "pasted": 0, "none": 0}
    for k in range(12):
        d = dicts[k % len(dicts)] if k != 5 else dict(dicts[5], annotations=[])      # one destination without instances
        np.random.seed(300 + k)
        got = mapper(d)
        state = np.random.get_state()
        np.random.seed(300 + k)
        dst, rm, take_self, srcs, sels = _replay(hand, dicts, d, method, scp_type, num_src, p_rm, select, whole)
        want = np.random.get_state()
        assert np.array_equal(state[1], want[1]) and state[2] == want[2], (method, scp_type, k)
        assert ("rm_bg" in got) == rm and got.get("rm_bg", True) is True
        seen["rm" if rm else "plain"] += 1
        assert torch.equal(got["image"], dst["image"]) and ("paste_pack" in got) == ("paste_pack" in dst)
        if not take_self:
            assert "scp_src" not in got
            continue
        seen["self"] += 1
        if not srcs:                                            # 'in_domain', nothing to draw from: CopyPaste.__call__ returns its input
            assert scp_type == "in_domain" and len(dst["instances"]) == 0 and "scp_src" not in got and "scp_file_name" not in got
            seen["none"] += 1
            continue
        picked = [(s, sel) for s, sel in zip(srcs, sels) if len(sel)]
        groups = got["scp_src"] if isinstance(got["scp_src"], list) else [got["scp_src"]]
        if not picked:
            assert groups[0]["masks"].shape[0] == 0
            continue
        assert len(groups) == len(picked)
        for grp, (src, sel) in zip(groups, picked):
            si, st = src["instances"], torch.from_numpy(np.asarray(sel, dtype=np.int64))
            assert torch.equal(grp["labels"], si.gt_classes[st]) and torch.equal(grp["boxes"], si.gt_boxes.tensor[st])
            assert bool(grp.get("all", False)) == whole
            if whole:
                assert len(grp["labels"]) == len(si)
            seen["pasted"] += len(sel)
    assert seen["self"] > 0 and seen["pasted"] > 0
    if 0 < p_rm < 1:
        assert seen["rm"] > 0 and seen["plain"] > 0
    elif p_rm >= 1:
        assert seen["plain"] == 0
    else:
        assert seen["rm"] == 0
    if scp_type == "in_domain":
        assert seen["none"] == 1


def _sample(z, case, part, extra=False):
    from divergen_amd.structures import BitMasks, Boxes, Instances
    g = lambda k: z["%s_%s_%s" % (case, part, k)]      # noqa: E731
    h, w = g("image").shape[-2:]
    inst = Instances((h, w), gt_boxes=Boxes(torch.from_numpy(g("boxes"))), gt_classes=torch.from_numpy(g("labels")),
                     gt_masks=BitMasks(torch.from_numpy(g("masks").astype(bool))))
    if extra:
        inst.instance_source = torch.arange(len(inst), dtype=torch.int64)
    return {"image": torch.from_numpy(g("image")), "file_name": case + "_" + part, "instances": inst}


def test_blob_carries_a_source_of_130_objects_pasted_whole():
    from divergen_amd.data import build as B
    z = _gold()
    src = _sample(z, "big130_n70", "src")
    m = _bare_mapper(method="self_copy", self_prob=1.0, paste_all=True, pack=True, dataset=["src"], mapper=lambda name: src)
    state = np.random.get_state()
    packed = m._call_self_copy(_sample(z, "big130_n70", "dst"), [0])
    assert np.array_equal(state[1], np.random.get_state()[1])   # no selection draw
    names = [x[0] for x in packed["blob_layout"]]
    assert names == ["image", "gt_masks", "gt_boxes", "gt_classes", "scp_image", "scp_masks", "scp_boxes", "scp_labels"]
    assert packed["blob_scp_all"] is True and tuple(packed["blob_scp_hw"]) == (32, 48) and "scp_src" not in packed
    back = B.unpack_sample(packed, torch.device("cpu"))
    s = back["scp_src"]
    assert s["all"] is True and tuple(s["hw"]) == (32, 48) and s["masks"].shape == (130, 32, 48)
    assert np.array_equal(s["masks"].numpy(), z["big130_n70_src_masks"]) and np.array_equal(s["labels"].numpy(), z["big130_n70_src_labels"])
    assert np.array_equal(s["boxes"].numpy(), z["big130_n70_src_boxes"]) and np.array_equal(s["image"].numpy(), z["big130_n70_src_image"])
    # a selected source of the same mapper code carries no mark
    m.paste_all = False
    np.random.seed(2)
    packed = m._call_self_copy(_sample(z, "ragged_a", "dst"), [0])
    assert "blob_scp_all" not in packed and "all" not in B.unpack_sample(packed, torch.device("cpu"))["scp_src"]


def test_in_domain_sample_without_sources_keeps_its_fields(tmp_path, monkeypatch):
    from divergen_amd.data import build as B
    cfg, info = _cfg(tmp_path, "both", KEY + ["INPUT.SCP_TYPE", "in_domain"])
    mapper, dicts = _mapper(cfg, info, monkeypatch, seed=3)
    mapper.pack = True
    np.random.seed(9)
    dst = mapper.mapper(dict(dicts[2], annotations=[]))
    assert len(dst["instances"]) == 0
    dst["instances"].instance_source = torch.zeros(0, dtype=torch.int64)
    packed = mapper._call_self_copy(dst, [1])
    assert [x[0] for x in packed["blob_layout"]] == ["image", "gt_masks", "gt_boxes", "gt_classes", "flat", "desc", "labels"]
    assert "blob_scp_hw" not in packed and "blob_scp_n" not in packed and "scp_file_name" not in packed and "rm_bg" not in packed
    back = B.unpack_sample(packed, torch.device("cpu"))
    assert "scp_src" not in back and back["instances"].has("instance_source") and "paste_pack" in back
    out = mapper.finish(packed, "cpu")                          # no self copy: the Instances are not rebuilt
    assert out["instances"].has("instance_source") and "scp_src" not in out


def test_rm_bg_crosses_the_queue_only_when_drawn(tmp_path, monkeypatch):
    from divergen_amd.data import build as B
    cfg, info = _cfg(tmp_path, "syn_copy", KEY + ["INPUT.RM_BG_PROB", 0.5])
    mapper, dicts = _mapper(cfg, info, monkeypatch, seed=3)
    mapper.pack = True
    drawn = []
    for k in range(10):
        np.random.seed(40 + k)
        packed = mapper(dicts[k])
        np.random.seed(40 + k)
        mapper.mapper(dicts[k])
        flag = bool(np.random.uniform(0.0, 1.0) <= 0.5)
        assert ("rm_bg" in packed) == flag and "blob" in packed
        assert set(packed) - {"rm_bg"} >= {"blob", "blob_layout", "blob_hw", "blob_K"} and not any(k.startswith("blob_scp") for k in packed)
        back = B.unpack_sample(packed, torch.device("cpu"))
        assert ("rm_bg" in back) == flag and back.get("rm_bg", True) is True
        drawn.append(flag)
        if flag:                                                # no quiet fall-back: the pixels are dgx_remove_background's
            with pytest.raises(RuntimeError, match="dgx_remove_background"):
                mapper.finish(packed, "cpu")
        else:
            assert "rm_bg" not in mapper.finish(packed, "cpu")
    assert 0 < sum(drawn) < len(drawn)
    # 'none': no pool, no blob -- the flag rides on the plain sample
    cfg, info = _cfg(tmp_path / "none", "none", KEY + ["INPUT.RM_BG_PROB", 1.0])
    mapper, dicts = _mapper(cfg, info, monkeypatch)
    np.random.seed(1)
    got = mapper(dicts[0])
    assert got["rm_bg"] is True and "blob" not in got and "paste_pack" not in got
