"""Generate tests/golden/self_copy.npz: the reference's own CopyPaste.__call__ (DG/divergen/data/transforms/custom_copypaste.py:242-341:
_select_object, _scp_src_to_dst, _copy_paste, get_bboxes) constructed as the mapper constructs it (cp_method=['basic'], mapper.py:770),
on small hand-built scenes.  Run in the authoring container only:

    python tests/golden/make_golden_selfcopy.py

_refload.py replaces custom_copypaste with a permissive stub; here that entry is removed again and the REAL file is imported under the
few stand-ins it needs at import time (RandomRotation, cv2, coco_evaluation: none is called in the configuration generated) and a
plain BitMasks holder.  Stored per case: the np.random seed, the m / sel that _select_object drew from it, the inputs and every output.
The 'both' case chains the reference's InstPool._copy_paste (pool patches, 'basic') and then the self copy on that result.
Every case's defining property is asserted here.  Fixed zip timestamps: two runs give identical bytes."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload as R  # noqa: E402
from make_golden_blend import save_deterministic  # noqa: E402


class BitMasks:
    def __init__(self, tensor):
        self.tensor = torch.as_tensor(tensor)

    def __len__(self):
        return self.tensor.shape[0]


def load_reference():
    R.install()
    name = "divergen.data.transforms.custom_copypaste"
    sys.modules.pop(name, None)
    st = sys.modules["detectron2.structures"]
    st.BitMasks = BitMasks
    aug = types.ModuleType("detectron2.data.transforms.augmentation_impl")
    aug.RandomRotation = lambda *a, **k: None
    sys.modules[aug.__name__] = aug
    ev = types.ModuleType("detectron2.evaluation")
    ev.__path__ = []
    ce = types.ModuleType("detectron2.evaluation.coco_evaluation")
    ce.instances_to_coco_json = None
    sys.modules[ev.__name__], sys.modules[ce.__name__] = ev, ce
    mod = importlib.import_module(name)
    assert mod.__file__.startswith(R.DG), mod.__file__
    return mod, st


def ellipse(h, w, cx, cy, rx, ry):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2) <= 1).astype(np.uint8)


def rect(h, w, x0, y0, x1, y1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def image(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((np.stack([xx * 3, yy * 4, (xx + yy) * 2]) % 256).astype(np.uint8) ^ rng.integers(0, 64, (3, h, w), dtype=np.uint8))


def tight(masks, jitter=None):
    b = np.zeros((len(masks), 4), np.float32)
    for i, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        if len(xs):
            b[i] = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
    if jitter is not None:
        b = (b + jitter).astype(np.float32)
    return b


def sample(st, img, masks, boxes, labels, name):
    h, w = img.shape[-2:]
    inst = st.Instances((h, w))
    inst.gt_boxes = st.Boxes(torch.from_numpy(boxes.astype(np.float32).reshape(-1, 4)))
    inst.gt_classes = torch.from_numpy(np.asarray(labels, dtype=np.int64))
    inst.gt_masks = BitMasks(torch.from_numpy(masks.astype(bool).reshape(-1, h, w)))
    return {"image": torch.from_numpy(img.copy()), "file_name": name, "image_id": 1, "instances": inst}


def drawn(seed, ns):
    """What _select_object draws from this seed (custom_copypaste.py:398-402)."""
    np.random.seed(seed)
    m = np.random.randint(0, min(ns + 1, 100))
    return m, np.random.choice(ns, size=m, replace=False)


def find_seed(ns, want):
    for seed in range(1, 100000):
        m, sel = drawn(seed, ns)
        if want(m, sel):
            return seed
    raise RuntimeError("no seed")


def run_case(cc, st, store, name, dst, src, want):
    d_img, d_m, d_b, d_l = dst
    s_img, s_m, s_b, s_l = src
    ns = len(s_m)
    seed = find_seed(ns, want)
    m, sel = drawn(seed, ns)
    cp = cc.CopyPaste(cp_method=["basic"])
    res = sample(st, d_img, d_m, d_b, d_l, name + "_dst")
    res["instances"].instance_source = torch.zeros(len(d_m), dtype=torch.int64)
    res["mix_results"] = [sample(st, s_img, s_m, s_b, s_l, name + "_src")]
    np.random.seed(seed)
    out = cp(res)
    o = out["instances"]
    assert sorted(o.get_fields()) == ["gt_boxes", "gt_classes", "gt_masks"] and "mix_results" not in out
    g = {"dst_image": d_img, "dst_masks": d_m.astype(np.uint8), "dst_boxes": d_b.astype(np.float32), "dst_labels": np.asarray(d_l, np.int64),
         "src_image": s_img, "src_masks": s_m.astype(np.uint8), "src_boxes": s_b.astype(np.float32), "src_labels": np.asarray(s_l, np.int64),
         "seed": np.array(seed), "m": np.array(m), "sel": np.asarray(sel, np.int64),
         "out_image": out["image"].numpy(), "out_masks": o.gt_masks.tensor.numpy().astype(np.uint8),
         "out_boxes": o.gt_boxes.tensor.numpy(), "out_labels": o.gt_classes.numpy(), "out_hw": np.array([out["height"], out["width"]])}
    assert g["out_image"].dtype == np.uint8 and g["out_boxes"].dtype == np.float32 and g["out_labels"].dtype == np.int64
    assert tuple(g["out_image"].shape[-2:]) == tuple(g["out_hw"]) == tuple(g["out_masks"].shape[-2:])
    for k, v in g.items():
        store["%s_%s" % (name, k)] = v
    return g


def main():
    cc, st = load_reference()
    mp = R.ref("divergen.data.custom_build_copypaste_mapper")
    rng = np.random.default_rng(77)
    store, cases = {}, []

    def src_scene(h, w, boxes_from=None):
        masks = np.stack([ellipse(h, w, 0.30 * w, 0.35 * h, 0.18 * w, 0.2 * h), ellipse(h, w, 0.45 * w, 0.5 * h, 0.2 * w, 0.22 * h),
                          rect(h, w, int(0.6 * w), int(0.55 * h), int(0.95 * w), int(0.97 * h)), ellipse(h, w, 0.7 * w, 0.25 * h, 0.12 * w, 0.15 * h)])
        return image(rng, h, w), masks, tight(masks, rng.uniform(-0.45, 0.45, (4, 4))).clip(0), np.array([11, 502, 77, 1202])

    def dst_scene(h, w):
        masks = np.stack([ellipse(h, w, 0.4 * w, 0.45 * h, 0.25 * w, 0.3 * h), rect(h, w, int(0.55 * w), int(0.1 * h), int(0.9 * w), int(0.5 * h)),
                          ellipse(h, w, 0.2 * w, 0.8 * h, 0.12 * w, 0.12 * h)])
        return image(rng, h, w), masks, tight(masks, rng.uniform(-0.45, 0.45, (3, 4))).clip(0), np.array([3, 950, 41])

    def add(name, dst, src, want, check):
        g = run_case(cc, st, store, name, dst, src, want)
        check(g)
        cases.append(name)
        return g

    full = lambda m, sel: m >= 2      # noqa: E731
    # --- canvas geometry
    add("equal", dst_scene(64, 80), src_scene(64, 80), full, lambda g: tuple(g["out_hw"]) == (64, 80) or 1 / 0)
    add("grow_h", dst_scene(48, 80), src_scene(72, 80), lambda m, sel: m >= 1 and 2 in sel,
        lambda g: (g["out_hw"][0] > 48 and g["out_hw"][1] == 80) or 1 / 0)
    add("grow_w", dst_scene(64, 56), src_scene(64, 90), lambda m, sel: m >= 1 and 2 in sel,
        lambda g: (g["out_hw"][0] == 64 and g["out_hw"][1] > 56) or 1 / 0)
    add("grow_both", dst_scene(40, 50), src_scene(77, 93), lambda m, sel: m >= 1 and 2 in sel,
        lambda g: (g["out_hw"][0] > 40 and g["out_hw"][1] > 50) or 1 / 0)
    # --- source larger than the canvas: its boxes (the mapper's, not the mask extents) end before its masks do
    s_img, s_m, s_b, s_l = src_scene(96, 96)
    s_b = np.minimum(s_b, np.array([60, 50, 60, 50], np.float32))

    def cropped(g):
        H, W = g["out_hw"]
        assert (H, W) == (64, 80)
        sel = g["sel"]
        lost = [int(g["src_masks"][j].sum()) - int(g["out_masks"][len(g["out_masks"]) - len(sel) + k].sum()) for k, j in enumerate(sel)]
        assert max(lost) > 0, lost                      # a selected mask loses pixels to the crop
    add("src_cropped", dst_scene(64, 80), (s_img, s_m, s_b, s_l), lambda m, sel: m >= 2 and 2 in sel, cropped)
    # --- nothing pasted
    add("m0", dst_scene(64, 80), src_scene(64, 80), lambda m, sel: m == 0,
        lambda g: (len(g["sel"]) == 0 and np.array_equal(g["out_boxes"], g["dst_boxes"]) and np.array_equal(g["out_image"], g["dst_image"])) or 1 / 0)
    e = (image(rng, 50, 60), np.zeros((0, 50, 60), np.uint8), np.zeros((0, 4), np.float32), np.zeros(0, np.int64))
    add("ns0", dst_scene(64, 80), e, lambda m, sel: True, lambda g: (int(g["m"]) == 0 and tuple(g["out_hw"]) == (64, 80)) or 1 / 0)
    # --- the occlusion filter: one 96 x 96 destination, the source's union is a block over x < 48 plus a bar
    h = w = 96
    d_m = np.stack([rect(h, w, 5, 5, 40, 30),            # 0 fully covered                        -> dropped
                    rect(h, w, 30, 40, 60, 52),          # 1 partly: box moves 18 > 10, area 144 <= 300  -> dropped
                    rect(h, w, 20, 56, 90, 80),          # 2 partly: box moves 28 > 10, area 1008 > 300  -> kept
                    rect(h, w, 44, 84, 58, 92),          # 3 partly: box moves 4 <= 10, area 80          -> kept
                    np.zeros((h, w), np.uint8),          # 4 empty mask, box of zeros                    -> kept (box unchanged)
                    rect(h, w, 70, 5, 90, 25)])          # 5 untouched
    d_b = tight(d_m)
    s_m2 = np.stack([rect(h, w, 0, 0, 48, 96), rect(h, w, 40, 0, 48, 96), rect(h, w, 30, 60, 44, 70)])      # overlapping selected masks
    s2 = (image(rng, h, w), s_m2, tight(s_m2), np.array([9, 8, 7]))

    def filt(g):
        assert int(g["m"]) == 3
        n_kept = len(g["out_labels"]) - 3
        assert g["out_labels"][:n_kept].tolist() == [102, 103, 104, 105], g["out_labels"]
        assert g["out_boxes"][0].tolist() == [48, 56, 90, 80] and g["out_boxes"][1].tolist() == [48, 84, 58, 92]
        assert g["out_boxes"][2].tolist() == [0, 0, 0, 0] and int(g["out_masks"][0].sum()) == 42 * 24 and int(g["out_masks"][1].sum()) == 80
        assert int((g["src_masks"][g["sel"]].sum(0) > 1).sum()) > 0      # the selected masks overlap
    add("filter", (image(rng, h, w), d_m, d_b, np.arange(100, 106)), s2, lambda m, sel: m == 3, filt)
    # --- no destination object
    e = (image(rng, 64, 80), np.zeros((0, 64, 80), np.uint8), np.zeros((0, 4), np.float32), np.zeros(0, np.int64))
    add("n0_0", e, src_scene(64, 80), full, lambda g: (len(g["out_labels"]) == int(g["m"]) >= 2) or 1 / 0)
    # --- 'both': the pool pastes (InstPool._copy_paste, 'basic'), then the self copy on that result
    from make_golden_blend import soft_patch
    H, W = 60, 80
    d_img, d_m, d_b, d_l = dst_scene(H, W)
    d_b = tight(d_m)
    geom = [(22, 26, 18, 12), (20, 24, 30, 20), (16, 18, -6, -5), (20, 24, W - 15, H - 12)]
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
    assert int(cur["instance_source"].sum()) >= 3
    store.update({"both_pre_image": d_img, "both_pre_masks": d_m, "both_pre_boxes": d_b, "both_pre_labels": d_l, "both_K": np.array(len(patches))})
    for k, (rgba, x0, y0, lab) in enumerate(patches):
        store["both_p%d_rgba" % k], store["both_p%d_xy" % k], store["both_p%d_label" % k] = rgba, np.array([x0, y0]), np.array([lab])
    add("both", (cur["image"], cur["gt_masks"].astype(np.uint8), cur["gt_bboxes"], cur["gt_labels"]), src_scene(72, 90),
        lambda m, sel: m >= 2 and 2 in sel, lambda g: (g["out_hw"][0] > 60 and g["out_hw"][1] > 80) or 1 / 0)
    assert cases == ["equal", "grow_h", "grow_w", "grow_both", "src_cropped", "m0", "ns0", "filter", "n0_0", "both"]
    store["cases"] = np.array(cases)
    save_deterministic(os.path.join(HERE, "self_copy.npz"), store)


if __name__ == "__main__":
    main()
