"""Generate tests/golden/self_copy_multi.npz: the reference's own, unmodified CopyPaste.__call__
(DG/divergen/data/transforms/custom_copypaste.py:242-341) with SEVERAL mix_results (INPUT.SCP_NUM_SRC > 1), constructed as the mapper
constructs it (selected=True, blank_ratio -1, rotate_src False, cp_method=['basic'], mapper.py:770) on small hand-built samples.
Run in the authoring container only:

    python tests/golden/make_golden_self_copy_multi.py

The reference file is imported under the stand-ins of make_golden_selfcopy.load_reference.  Stored per case: the np.random seed, the
m / sel that _select_object drew from it for every source, the inputs and every output; and, read off the reference's own
_copy_paste calls (the bound method is wrapped on the instance so that its `valid_inds` can be seen; the code that runs is the
reference's): the canvas of every temporary stage, which of the selected planes reach the final paste, which destination objects
survive it.  Every case's defining property is asserted here, on the reference's output.  Fixed zip timestamps: two runs give
identical bytes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_blend import save_deterministic  # noqa: E402
from make_golden_selfcopy import ellipse, image, load_reference, rect, sample, tight  # noqa: E402


def drawn(seed, ns_list):
    """What _select_object draws from this seed for the sources in order (custom_copypaste.py:398-402)."""
    np.random.seed(seed)
    out = []
    for ns in ns_list:
        m = np.random.randint(0, min(ns + 1, 100))
        out.append((m, np.random.choice(ns, size=m, replace=False)))
    return out


def find_seed(ns_list, wants):
    for seed in range(1, 400000):
        if all(w(m, sel) for w, (m, sel) in zip(wants, drawn(seed, ns_list))):
            return seed
    raise RuntimeError("no seed")


def run_case(cc, st, store, name, dst, sources, wants):
    d_img, d_m, d_b, d_l = dst
    ns_list = [len(s[1]) for s in sources]
    seed = find_seed(ns_list, wants)
    draws = drawn(seed, ns_list)
    cp = cc.CopyPaste(selected=True, blank_ratio=-1, rotate_src=False, cp_method=["basic"])
    calls, inner = [], cp._copy_paste

    def spy(dst_results, src_results, ret_valid_idx=False):      # the reference's _copy_paste, asked for its valid_inds as well
        n_before, hw = len(dst_results["gt_bboxes"]), tuple(dst_results["img"].shape[-2:])
        res, valid = inner(dst_results, src_results, True)
        calls.append((n_before, len(src_results["gt_bboxes"]), hw, np.asarray(valid, dtype=bool).copy()))
        return (res, valid) if ret_valid_idx else res
    cp._copy_paste = spy
    res = sample(st, d_img, d_m, d_b, d_l, name + "_dst")
    res["instances"].instance_source = torch.zeros(len(d_m), dtype=torch.int64)
    res["mix_results"] = [sample(st, s[0], s[1], s[2], s[3], "%s_src%d" % (name, i)) for i, s in enumerate(sources)]
    np.random.seed(seed)
    out = cp(res)
    o = out["instances"]
    assert sorted(o.get_fields()) == ["gt_boxes", "gt_classes", "gt_masks"] and "mix_results" not in out
    # ---- bookkeeping from the recorded calls: rows = for every accumulator object its row among the M selected planes
    taken = [i for i, (m, _) in enumerate(draws) if m]
    M = sum(draws[i][0] for i in taken)
    assert len(calls) == len(taken)                       # len(taken) - 1 temporary stages + the final paste (none when all empty)
    rows, seen, tmp_hw = np.arange(draws[taken[0]][0]) if taken else np.zeros(0, np.int64), 0, []
    for k, i in enumerate(taken[1:]):
        n_before, n_src, hw, valid = calls[k]
        seen += draws[taken[k]][0]
        assert n_before == len(rows) and n_src == draws[i][0]
        rows = np.concatenate([rows[valid], seen + np.arange(n_src)])
        tmp_hw.append(hw)
    merge_valid = np.zeros(M, np.uint8)
    merge_valid[rows] = 1
    dst_valid = np.ones(len(d_m), np.uint8)
    if taken:
        n_before, n_src, _, valid = calls[-1]
        assert n_before == len(d_m) and n_src == len(rows)
        dst_valid = valid.astype(np.uint8)
    g = {"dst_image": d_img, "dst_masks": d_m.astype(np.uint8), "dst_boxes": d_b.astype(np.float32), "dst_labels": np.asarray(d_l, np.int64),
         "n_src": np.array(len(sources)), "seed": np.array(seed), "tmp_hw": np.asarray(tmp_hw, np.int64).reshape(-1, 2),
         "merge_valid": merge_valid, "dst_valid": dst_valid,
         "out_image": out["image"].numpy(), "out_masks": o.gt_masks.tensor.numpy().astype(np.uint8),
         "out_boxes": o.gt_boxes.tensor.numpy(), "out_labels": o.gt_classes.numpy(), "out_hw": np.array([out["height"], out["width"]])}
    for i, (s, (m, sel)) in enumerate(zip(sources, draws)):
        g.update({"src%d_image" % i: s[0], "src%d_masks" % i: s[1].astype(np.uint8), "src%d_boxes" % i: s[2].astype(np.float32),
                  "src%d_labels" % i: np.asarray(s[3], np.int64), "src%d_m" % i: np.array(m), "src%d_sel" % i: np.asarray(sel, np.int64)})
    assert g["out_image"].dtype == np.uint8 and g["out_boxes"].dtype == np.float32 and g["out_labels"].dtype == np.int64
    assert tuple(g["out_image"].shape[-2:]) == tuple(g["out_hw"]) == tuple(g["out_masks"].shape[-2:])
    assert len(g["out_labels"]) == int(dst_valid.sum()) + int(merge_valid.sum())
    for k, v in g.items():
        store["%s_%s" % (name, k)] = v
    return g


def main():
    cc, st = load_reference()
    rng = np.random.default_rng(2024)
    store, cases = {}, []

    def scene(h, w, labels, jitter=True):
        """four objects spread over an (h, w) frame, boxes a little off the mask extents as the mapper's are"""
        masks = np.stack([ellipse(h, w, 0.30 * w, 0.35 * h, 0.18 * w, 0.2 * h), ellipse(h, w, 0.45 * w, 0.55 * h, 0.2 * w, 0.22 * h),
                          rect(h, w, int(0.6 * w), int(0.5 * h), int(0.95 * w), int(0.95 * h)), ellipse(h, w, 0.7 * w, 0.25 * h, 0.12 * w, 0.15 * h)])
        boxes = tight(masks, rng.uniform(-0.45, 0.45, (4, 4)) if jitter else None).clip(0)
        return image(rng, h, w), masks, boxes, np.asarray(labels)

    def dst_scene(h, w):
        masks = np.stack([ellipse(h, w, 0.4 * w, 0.45 * h, 0.25 * w, 0.3 * h), rect(h, w, int(0.55 * w), int(0.1 * h), int(0.9 * w), int(0.5 * h)),
                          ellipse(h, w, 0.2 * w, 0.8 * h, 0.12 * w, 0.12 * h)])
        return image(rng, h, w), masks, tight(masks, rng.uniform(-0.45, 0.45, (3, 4))).clip(0), np.array([3, 950, 41])

    def one(h, w, mask, label):
        m = mask[None]
        return image(rng, h, w), m, tight(m), np.array([label])

    def add(name, dst, sources, wants, check):
        g = run_case(cc, st, store, name, dst, sources, wants)
        check(g)
        cases.append(name)

    several = lambda m, sel: m >= 2      # noqa: E731
    everything = lambda n: (lambda m, sel: m == n)      # noqa: E731
    nothing = lambda m, sel: m == 0      # noqa: E731

    # (a) two sources, no width a multiple of 16
    def chk_a(g):
        assert len(g["tmp_hw"]) == 1 and all(int(x.shape[-1]) % 16 for x in (g["dst_image"], g["src0_image"], g["src1_image"], g["out_image"]))
    add("s2_ragged", dst_scene(64, 83), [scene(70, 90, [11, 502, 77, 1202]), scene(60, 77, [5, 6, 7, 8])], [several, several], chk_a)

    # (b) three sources, the middle one selects nothing and is skipped
    def chk_b(g):
        assert int(g["src1_m"]) == 0 and int(g["src0_m"]) >= 2 and int(g["src2_m"]) >= 2 and len(g["tmp_hw"]) == 1
        assert not set(g["src1_labels"].tolist()) & set(g["out_labels"].tolist())
    add("s3_skip_mid", dst_scene(64, 80), [scene(64, 80, [11, 12, 13, 14]), scene(64, 80, [21, 22, 23, 24]), scene(72, 96, [31, 32, 33, 34])],
        [several, nothing, several], chk_b)

    # (c) the temporary canvas is smaller than a source frame: the boxes (the mapper's, not the mask extents) end before the masks
    # do, the crop to the stage's canvas is permanent, and the final canvas (the destination's size) is larger again
    s0, s1 = scene(96, 96, [41, 42, 43, 44]), scene(80, 96, [51, 52, 53, 54])
    s0 = (s0[0], s0[1], np.minimum(s0[2], np.array([58, 50, 58, 50], np.float32)), s0[3])
    s1 = (s1[0], s1[1], np.minimum(s1[2], np.array([52, 44, 52, 44], np.float32)), s1[3])

    def chk_c(g):
        (h, w), = [tuple(x) for x in g["tmp_hw"]]
        H, W = g["out_hw"]
        assert h < 80 and w < 96 and h < H and w < W and (H, W) == (64, 80), (h, w, H, W)
        n_dst = int(g["dst_valid"].sum())
        acc = g["out_masks"][n_dst:]
        assert not acc[:, h:, :].any() and not acc[:, :, w:].any()      # nothing of any source outside the temporary canvas ...
        full = np.concatenate([g["src0_masks"][g["src0_sel"]][:, :H, :W], g["src1_masks"][g["src1_sel"]][:, :H, :W]])
        assert full[:, h:, :].any() or full[:, :, w:].any()             # ... where a crop to the final canvas alone would have left pixels
    add("tmp_crop", dst_scene(64, 80), [s0, s1], [lambda m, sel: m >= 2 and 2 in sel, lambda m, sel: m >= 2 and 2 in sel], chk_c)

    # (d) an accumulator object whose box moves 8 at each of two stages (16 in total) with fewer than 300 pixels: kept both times,
    # because the box of the stage before is what each stage compares with
    h, w = 48, 64
    d0 = one(h, w, rect(h, w, 10, 10, 40, 18), 61)
    d1 = one(h, w, rect(h, w, 0, 0, 18, 30), 62)
    d2 = one(h, w, rect(h, w, 8, 0, 26, 24), 63)      # (leaves source 1's object its box)

    def chk_d(g):
        assert g["merge_valid"].tolist() == [1, 1, 1] and len(g["tmp_hw"]) == 2
        n_dst = int(g["dst_valid"].sum())
        assert g["out_labels"][n_dst:].tolist() == [61, 62, 63]
        assert g["out_boxes"][n_dst].tolist() == [26, 10, 40, 18] and int(g["out_masks"][n_dst].sum()) == 14 * 8 <= 300
        assert abs(26 - float(g["src0_boxes"][0, 0])) > 10
    far = (image(rng, h, w), rect(h, w, 44, 34, 60, 46)[None], tight(rect(h, w, 44, 34, 60, 46)[None]), np.array([9]))
    add("drift", far, [d0, d1, d2], [everything(1)] * 3, chk_d)

    # (e) dropped at a temporary stage: box moved by 20 with 160 pixels left; with exactly 300 left (dropped); with 301 left (kept)
    h, w = 64, 96
    c301 = rect(h, w, 4, 36, 54, 46)
    c301[46, 30] = 1
    e_m = np.stack([rect(h, w, 4, 4, 40, 14), rect(h, w, 4, 20, 54, 30), c301, rect(h, w, 66, 8, 90, 30)])
    e0 = (image(rng, h, w), e_m, tight(e_m), np.array([71, 72, 73, 74]))
    e1 = one(h, w, rect(h, w, 0, 0, 24, 60), 75)

    def chk_e(g):
        order = g["src0_sel"].tolist()
        left = {71: 160, 72: 300, 73: 301, 74: 24 * 22}
        kept = [lab for lab, v in zip(g["src0_labels"][order], g["merge_valid"][:4]) if v]
        assert sorted(kept) == [73, 74] and int(g["merge_valid"][4]) == 1
        n_dst = int(g["dst_valid"].sum())
        for lab, mk in zip(g["out_labels"][n_dst:], g["out_masks"][n_dst:]):
            if int(lab) in left:
                assert int(mk.sum()) == left[int(lab)], (lab, int(mk.sum()))
        covered = e1[1][0].astype(bool)
        for j, lab in enumerate(g["src0_labels"]):          # what was left of the two dropped ones, on the reference's numbers
            rest = g["src0_masks"][j].astype(bool) & ~covered
            assert int(rest.sum()) == left[int(lab)]
    add("drop_300_301", dst_scene(64, 96), [e0, e1], [everything(4), everything(1)], chk_e)

    # (f) the destination larger than every source, and smaller than every source
    def chk_big(g):
        assert tuple(g["out_hw"]) == (96, 112) and all(g["src%d_image" % i].shape[1] < 96 and g["src%d_image" % i].shape[2] < 112 for i in range(2))
    add("dst_larger", dst_scene(96, 112), [scene(60, 72, [81, 82, 83, 84]), scene(50, 80, [85, 86, 87, 88])],
        [lambda m, sel: m >= 2 and 2 in sel] * 2, chk_big)

    def chk_small(g):
        assert g["out_hw"][0] > 40 and g["out_hw"][1] > 48 and all(g["src%d_image" % i].shape[1] > 40 and g["src%d_image" % i].shape[2] > 48 for i in range(2))
    add("dst_smaller", dst_scene(40, 48), [scene(72, 90, [91, 92, 93, 94]), scene(80, 96, [95, 96, 97, 98])],
        [lambda m, sel: m >= 2 and 2 in sel] * 2, chk_small)

    # (g) no source selects anything (one has no object at all)
    none = (image(rng, 50, 60), np.zeros((0, 50, 60), np.uint8), np.zeros((0, 4), np.float32), np.zeros(0, np.int64))

    def chk_g(g):
        assert np.array_equal(g["out_image"], g["dst_image"]) and np.array_equal(g["out_boxes"], g["dst_boxes"]) and len(g["merge_valid"]) == 0
    add("all_empty", dst_scene(64, 80), [scene(64, 80, [1, 2, 3, 4]), none], [nothing, nothing], chk_g)

    # four sources (the bound of the build), every frame another size
    def chk_4(g):
        assert len(g["tmp_hw"]) == 3 and int(g["n_src"]) == 4
    add("s4", dst_scene(72, 96), [scene(64, 80, [101, 102, 103, 104]), scene(70, 90, [111, 112, 113, 114]), scene(48, 64, [121, 122, 123, 124]),
                                  scene(80, 112, [131, 132, 133, 134])], [several] * 4, chk_4)

    assert cases == ["s2_ragged", "s3_skip_mid", "tmp_crop", "drift", "drop_300_301", "dst_larger", "dst_smaller", "all_empty", "s4"]
    store["cases"] = np.array(cases)
    save_deterministic(os.path.join(HERE, "self_copy_multi.npz"), store)


if __name__ == "__main__":
    main()
