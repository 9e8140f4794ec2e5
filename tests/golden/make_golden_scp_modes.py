"""Generate tests/golden/scp_modes.npz: what INPUT.SCP_SRC_MODES adds to the self copy, from the reference's own code.  Run in the
authoring container only:

    python tests/golden/make_golden_scp_modes.py

(a) the real CopyPaste(selected=False, cp_method=['basic']).__call__ (DG/divergen/data/transforms/custom_copypaste.py:242-341; the
    mapper constructs it so for INPUT.SCP_SRC_OBJ_SELECT False and INPUT.SCP_TYPE 'in_domain' / 'cas', mapper.py:764-770) on hand-built
    scenes: ragged destination / source sizes, a source with 130 objects (no cap of 99 without _select_object) on no and on 70
    destination objects, a source / a destination without objects, and the 'both' chain (InstPool._copy_paste, then the paste);
(b) the real CopyPaste.remove_background (:101-109): an ordinary scene, overlapping masks, no masks, and one followed by the paste;
(c) the real CopyPasteMapper.set_dataset (the per_cat_map part, mapper.py:829-835) and _filter_in_specific_cls (:782-815), called as
    unbound functions on a stand-in whose `mapper` records the dict it is given and consumes a fixed number of draws, over a
    12-image synthetic dataset: per case the seed, the class list, the indices drawn and the category ids each source was mapped with.
The reference is imported through _refload and make_golden_selfcopy's stand-ins; nothing of it is copied or restated.  Every case's
defining property is asserted here.  Fixed zip timestamps: two runs give identical bytes."""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload as R  # noqa: E402
from make_golden_blend import save_deterministic, soft_patch  # noqa: E402
from make_golden_selfcopy import BitMasks, ellipse, image, load_reference, rect, sample, tight  # noqa: E402

MAPPER_DRAWS = 3      # what the stand-in mapper consumes per call


def scene(rng, h, w, n):
    """n objects: ellipses and rectangles spread over (h, w)."""
    masks = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        cx, cy = rng.uniform(0.1, 0.9) * w, rng.uniform(0.1, 0.9) * h
        if i % 2:
            masks[i] = ellipse(h, w, cx, cy, max(1.0, 0.22 * w), max(1.0, 0.2 * h))
        else:
            masks[i] = rect(h, w, int(cx * 0.6), int(cy * 0.6), int(cx * 0.6 + 0.4 * w) + 1, int(cy * 0.6 + 0.35 * h) + 1)
    return image(rng, h, w), masks, tight(masks), rng.integers(0, 1203, n).astype(np.int64)


def grid_source(rng, h, w, cols, rows):
    """cols x rows small rectangles (2 x 2) on a grid: most of the frame stays uncovered, neighbours may touch."""
    masks = np.zeros((cols * rows, h, w), np.uint8)
    for r in range(rows):
        for c in range(cols):
            x0, y0 = (c * (w - 3)) // (cols - 1), (r * (h - 3)) // (rows - 1)
            masks[r * cols + c, y0:y0 + 2, x0:x0 + 2] = 1
    return image(rng, h, w), masks, tight(masks), (np.arange(cols * rows) * 7 % 1203).astype(np.int64)


def paste_all(cc, st, store, name, dst, src, pre=None):
    """CopyPaste(selected=False).__call__ on one destination and one source; `pre`: applied to the destination sample first."""
    d_img, d_m, d_b, d_l = dst
    s_img, s_m, s_b, s_l = src
    cp = cc.CopyPaste(selected=False, cp_method=["basic"])
    res = sample(st, d_img, d_m, d_b, d_l, name + "_dst")
    res["instances"].instance_source = torch.zeros(len(d_m), dtype=torch.int64)
    if pre is not None:
        res = pre(cp, res)
    res["mix_results"] = [sample(st, s_img, s_m, s_b, s_l, name + "_src")]
    state = np.random.get_state()[1].copy()
    out = cp(res)
    assert np.array_equal(state, np.random.get_state()[1])          # no draw without _select_object
    o = out["instances"]
    assert sorted(o.get_fields()) == ["gt_boxes", "gt_classes", "gt_masks"] and "mix_results" not in out
    g = {"dst_image": d_img, "dst_masks": d_m.astype(np.uint8), "dst_boxes": d_b.astype(np.float32), "dst_labels": np.asarray(d_l, np.int64),
         "src_image": s_img, "src_masks": s_m.astype(np.uint8), "src_boxes": s_b.astype(np.float32), "src_labels": np.asarray(s_l, np.int64),
         "out_image": out["image"].numpy(), "out_masks": o.gt_masks.tensor.numpy().astype(np.uint8),
         "out_boxes": o.gt_boxes.tensor.numpy(), "out_labels": o.gt_classes.numpy(), "out_hw": np.array([out["height"], out["width"]])}
    assert g["out_image"].dtype == np.uint8 and g["out_boxes"].dtype == np.float32 and g["out_labels"].dtype == np.int64
    assert tuple(g["out_image"].shape[-2:]) == tuple(g["out_hw"]) == tuple(g["out_masks"].shape[-2:])
    ns = len(s_m)
    assert np.array_equal(g["out_labels"][len(g["out_labels"]) - ns:], g["src_labels"])      # every source object, in its order
    for k, v in g.items():
        store["%s_%s" % (name, k)] = v
    return g


def gen_paste_all(cc, st, mp, store):
    rng = np.random.default_rng(130)
    cases = []
    # --- ragged sizes (destination, source) out of tests/test_gpu_self_copy.py's RAGGED list, and one pair of them the other way round
    for name, (dhw, shw) in (("ragged_a", ((30, 24), (50, 37))), ("ragged_b", ((3, 3), (9, 33))), ("ragged_c", ((48, 64), (30, 24)))):
        g = paste_all(cc, st, store, name, scene(rng, *dhw, 3), scene(rng, *shw, 5))
        assert tuple(g["out_hw"]) == (max(dhw[0], int(np.ceil(g["src_boxes"][:, 3].max()))), max(dhw[1], int(np.ceil(g["src_boxes"][:, 2].max()))))
        cases.append(name)
    # --- 130 source objects on 32 x 48: beyond the 99 _select_object would stop at
    h, w = 32, 48
    src = grid_source(rng, h, w, 13, 10)
    assert len(src[1]) == 130
    e = (image(rng, h, w), np.zeros((0, h, w), np.uint8), np.zeros((0, 4), np.float32), np.zeros(0, np.int64))
    g = paste_all(cc, st, store, "big130_n0", e, src)
    assert len(g["out_labels"]) == 130
    cases.append("big130_n0")
    d_m = np.zeros((70, h, w), np.uint8)
    d_m[0] = src[1][58]                                   # exactly under a source object, its box far from the origin -> dropped
    d_m[1] = 1                                            # the whole frame: far more than 300 pixels are left          -> kept
    for i in range(2, 70):
        x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 6))
        d_m[i, y0:y0 + int(rng.integers(2, 7)), x0:x0 + int(rng.integers(2, 9))] = 1
    d_l = (2000 + np.arange(70)).astype(np.int64)
    g = paste_all(cc, st, store, "big130_n70", (image(rng, h, w), d_m, tight(d_m), d_l), src)
    kept = g["out_labels"][:len(g["out_labels"]) - 130].tolist()
    assert 2000 not in kept and 2001 in kept and 1 <= len(kept) < 70, kept          # the occlusion filter drops and keeps
    cases.append("big130_n70")
    # --- a source / a destination without objects
    e = (image(rng, 20, 31), np.zeros((0, 20, 31), np.uint8), np.zeros((0, 4), np.float32), np.zeros(0, np.int64))
    g = paste_all(cc, st, store, "ns0", scene(rng, 30, 24, 3), e)
    assert np.array_equal(g["out_image"], g["dst_image"]) and np.array_equal(g["out_boxes"], g["dst_boxes"])
    e = (image(rng, 30, 24), np.zeros((0, 30, 24), np.uint8), np.zeros((0, 4), np.float32), np.zeros(0, np.int64))
    g = paste_all(cc, st, store, "n0_0", e, scene(rng, 30, 24, 4))
    assert len(g["out_labels"]) == 4
    cases += ["ns0", "n0_0"]
    # --- 'both': the pool pastes (InstPool._copy_paste, 'basic'), then the whole source on that result
    H, W = 48, 64
    d_img, d_m, d_b, d_l = scene(rng, H, W, 3)
    geom = [(14, 16, 10, 8), (12, 18, 30, 20), (10, 12, -4, -3), (12, 14, W - 9, H - 7)]
    patches = [(soft_patch(rng, ph, pw), x0, y0, 1000 + k) for k, (ph, pw, x0, y0) in enumerate(geom)]
    fake = types.SimpleNamespace(bbox_occluded_thr=10, mask_occluded_thr=300, cp_method=["basic"])
    cur = {"image": d_img.copy(), "gt_masks": d_m.copy(), "gt_bboxes": d_b.copy(), "gt_labels": d_l.copy(), "instance_source": np.zeros(len(d_m), np.int64)}
    for rgba, x0, y0, lab in patches:
        canvas = np.zeros((4, H, W), np.uint8)
        ph, pw = rgba.shape[:2]
        ys, xs, ye, xe = max(y0, 0), max(x0, 0), min(y0 + ph, H), min(x0 + pw, W)
        canvas[:, ys:ye, xs:xe] = rgba[ys - y0:ye - y0, xs - x0:xe - x0].transpose(2, 0, 1)
        cmask = (canvas[3:4] > 0).astype(np.uint8)
        cur = mp.InstPool._copy_paste(fake, cur, {"image": canvas, "gt_masks": cmask, "gt_bboxes": mp.get_bboxes(cmask), "gt_labels": np.array([lab], np.int64)})
    assert int(cur["instance_source"].sum()) >= 2
    store.update({"both_pre_image": d_img, "both_pre_masks": d_m, "both_pre_boxes": d_b, "both_pre_labels": d_l, "both_K": np.array(len(patches))})
    for k, (rgba, x0, y0, lab) in enumerate(patches):
        store["both_p%d_rgba" % k], store["both_p%d_xy" % k], store["both_p%d_label" % k] = rgba, np.array([x0, y0]), np.array([lab])
    paste_all(cc, st, store, "both", (cur["image"], cur["gt_masks"].astype(np.uint8), cur["gt_bboxes"], cur["gt_labels"]), scene(rng, 40, 70, 6))
    cases.append("both")
    store["paste_all_cases"] = np.array(cases)


def gen_remove_background(cc, st, store):
    rng = np.random.default_rng(869)
    cp = cc.CopyPaste(selected=False, cp_method=["basic"])
    cases = []

    def run(name, img, masks):
        res = sample(st, img, masks, tight(masks), np.arange(len(masks)), name)
        out = cp.remove_background(res)
        store["%s_image" % name], store["%s_masks" % name], store["%s_out" % name] = img, masks.astype(np.uint8), out["image"].numpy()
        assert store["%s_out" % name].dtype == np.uint8 and store["%s_out" % name].shape == img.shape
        cases.append(name)
        return store["%s_out" % name]
    img, masks, _, _ = scene(rng, 30, 24, 3)
    out = run("rb_plain", img, masks)
    assert 0 < int((out != 0).any(0).sum()) <= int(masks.any(0).sum()) < 30 * 24
    h, w = 33, 47
    masks = np.stack([rect(h, w, 2, 3, 30, 20), rect(h, w, 20, 10, 45, 31), ellipse(h, w, 25, 15, 9, 8)])
    out = run("rb_overlap", image(rng, h, w), masks)
    assert int((masks.sum(0) > 1).sum()) > 0
    out = run("rb_n0", image(rng, 9, 33), np.zeros((0, 9, 33), np.uint8))
    assert not out.any()
    store["rb_cases"] = np.array(cases)
    # --- the order: background first, then the paste (mapper.py:869-872 sits before :936)
    g = paste_all(cc, st, store, "rb_then_paste", scene(rng, 30, 24, 3), scene(rng, 50, 37, 4), pre=lambda c, r: c.remove_background(r))
    blank = ~(g["dst_masks"].any(0)) & ~(g["out_masks"][len(g["out_masks"]) - 4:, :30, :24].any(0))
    assert blank.any() and not g["out_image"][:, :30, :24][:, blank].any()


DATASET_CATS = [[3, 3, 1], [1], [2, 5], [5, 5, 7], [0], [9, 1, 2], [4], [7, 2], [8, 3], [], [1, 9], [5]]
SELECT_CATS = [2, 5, 7, 9]


def gen_class_sources(mp, store):
    dataset = [{"file_name": "img%d" % i, "image_id": i, "annotations": [{"category_id": c, "id": 100 * i + k} for k, c in enumerate(cats)]}
               for i, cats in enumerate(DATASET_CATS)]
    M = mp.CopyPasteMapper

    class StandIn:
        def __init__(self, scp_type):
            self.scp_type, self.rfs_choice, self.scp_select_cls, self.calls = scp_type, False, list(SELECT_CATS), []

        def mapper(self, d):
            self.calls.append((int(d["file_name"][3:]), [a["category_id"] for a in d["annotations"]]))
            np.random.rand(MAPPER_DRAWS)
            return d
    kw = {"in_domain": {}, "cas": {"cas": True}, "the_cls": {"specific_cls": True}, "the_cls_img": {"specific_cls": True, "filter_cls_inst": False}}
    cases, maps = [], {}
    for t in ("in_domain", "cas", "the_cls", "the_cls_img"):
        s = StandIn(t)
        before = copy.deepcopy(dataset)
        M.set_dataset(s, dataset)
        assert dataset == before and s.dataset is dataset
        maps[t] = [[int(k), [int(i) for i in v]] for k, v in s.per_cat_map.items()]
        differs = 0
        for num_src in (1, 3):
            for seed in (11, 12, 13):
                for dst_classes in ([5, 1, 5], [8]) if t == "in_domain" else ([4],):
                    s.calls = []
                    np.random.seed(seed)
                    res = {"instances": types.SimpleNamespace(gt_classes=torch.tensor(dst_classes, dtype=torch.int64))}
                    got = M._filter_in_specific_cls(s, res, num_src, **kw[t])
                    after = float(np.random.rand())
                    assert len(got) == len(s.calls) == num_src
                    np.random.seed(seed)
                    uniform = [int(np.random.randint(0, len(dataset))) for _ in range(num_src)]
                    differs += int([c[0] for c in s.calls] != uniform)
                    cases.append({"type": t, "num_src": num_src, "seed": seed, "dst_classes": dst_classes, "indices": [c[0] for c in s.calls],
                                  "mapped_cats": [c[1] for c in s.calls], "after": after})
        assert differs > 0, t                                 # not what the uniform draw at the same seed picks
    maps_all = list(maps.values())
    assert all(m == maps_all[0] for m in maps_all)
    # 'in_domain' on a destination without instances: no source, no draw
    s = StandIn("in_domain")
    M.set_dataset(s, dataset)
    np.random.seed(5)
    first = float(np.random.rand())
    np.random.seed(5)
    assert M._filter_in_specific_cls(s, {"instances": types.SimpleNamespace(gt_classes=torch.zeros(0, dtype=torch.int64))}, 3) == [] and not s.calls
    assert float(np.random.rand()) == first
    cases.append({"type": "in_domain", "num_src": 3, "seed": 5, "dst_classes": [], "indices": [], "mapped_cats": [], "after": first})
    assert any(c["mapped_cats"] and any(len(m) < len(DATASET_CATS[i]) for i, m in zip(c["indices"], c["mapped_cats"])) for c in cases)      # the filter drops
    assert all(m == DATASET_CATS[i] for c in cases if c["type"] == "the_cls_img" for i, m in zip(c["indices"], c["mapped_cats"]))
    store["cls_dataset_cats"] = np.array(json.dumps(DATASET_CATS))
    store["cls_select_cats"] = np.array(SELECT_CATS, np.int64)
    store["cls_mapper_draws"] = np.array(MAPPER_DRAWS)
    store["cls_per_cat_map"] = np.array(json.dumps(maps_all[0]))
    store["cls_cases"] = np.array(json.dumps(cases))


def main():
    cc, st = load_reference()
    mp = R.ref("divergen.data.custom_build_copypaste_mapper")
    store = {}
    gen_paste_all(cc, st, mp, store)
    gen_remove_background(cc, st, store)
    gen_class_sources(mp, store)
    save_deterministic(os.path.join(HERE, "scp_modes.npz"), store)


if __name__ == "__main__":
    main()
