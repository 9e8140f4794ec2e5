"""Generate tests/golden/poisson_blend.npz: the reference's own InstPool._copy_paste -> blend_image -> poisson_edit
(DG/divergen/data/custom_build_copypaste_mapper.py:510-566, DG/divergen/data/transforms/custom_cp_method.py:5-22,
DG/divergen/data/transforms/possion_blending.py:27-64), all unmodified, with INPUT.CP_METHOD lists that name 'possion', on the small
seeded fixture of make_golden_blend.py (60 x 80; six pastes: interior, overlapping, the four corners and edges).  Run in the
authoring container only:

    python tests/golden/make_golden_poisson.py

Stored: the inputs, the method blend_image drew for every paste (`random.sample` wrapped by a recorder, `random` seeded as D2's
seed_all_rng seeds it), the image after every paste, the final masks / boxes / labels / instance_source, and per case
`ref_vs_restated_mismatches`: the number of bytes, summed over the steps, where the reference differs from tests/_poisson_ref.py run
on the reference's own previous image.  Every such difference is asserted to be +-1 here: the reference's sparse LU returns T - eps
on identity rows and lands a hair on either side of an integer elsewhere, then truncates, so no other solver reproduces it to the
byte.  cv2 is absent: poisson_edit only imports it; cv2.blur ('gaussian' in the mixed case) is make_golden_blend.py's stand-in.
The file is written with fixed zip timestamps: two runs give identical bytes."""
import importlib
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                        # tests/: _poisson_ref, _blend_ref
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository: oracle
import _refload as R  # noqa: E402
import make_golden_blend as MB  # noqa: E402
import _poisson_ref as PR  # noqa: E402

H, W = MB.H, MB.W
SEQ_DRAWS = 31
ALL = ["basic", "alpha", "gaussian", "possion"]
CASES = [("possion", ["possion"], 5), ("mixed4", ALL, 1)]
CODES = {"basic": 0, "alpha": 1, "gaussian": 2, "possion": 3}


def main():
    mp = R.ref("divergen.data.custom_build_copypaste_mapper")
    cm = R.ref("divergen.data.transforms.custom_cp_method")
    assert mp.blend_image is cm.blend_image
    # _refload parks a stub under the module's name (the loaders before this one never reached it): load the real file
    del sys.modules["divergen.data.transforms.possion_blending"]
    pb = importlib.import_module("divergen.data.transforms.possion_blending")
    assert pb.__file__.startswith(R.DG)
    cm.poisson_edit = pb.poisson_edit
    cm.cv2.blur = MB.blur_standin
    drawn = []

    def sample(population, k):
        out = random.sample(population, k)
        drawn.append(out[0])
        return out
    cm.random = types.SimpleNamespace(sample=sample)

    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:H, 0:W]
    img = (np.stack([xx * 3, yy * 4, (xx + yy) * 2]) % 256).astype(np.uint8) ^ rng.integers(0, 32, (3, H, W), dtype=np.uint8)
    n0 = 3
    masks = np.zeros((n0, H, W), np.uint8)
    for i, (cx, cy, rx, ry) in enumerate([(30, 25, 14, 10), (60, 40, 12, 15), (15, 48, 10, 8)]):
        masks[i] = (((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2) <= 1
    boxes = mp.get_bboxes(masks)
    labels = np.array([5, 17, 230], dtype=np.int64)
    geom = [(22, 26, 18, 12), (20, 24, 30, 20), (16, 18, -6, -5), (20, 24, W - 15, H - 12), (14, 16, W - 10, -4),
            (18, 20, -5, H - 9)]
    pastes = [(MB.soft_patch(rng, h, w), x0, y0, 1000 + k) for k, (h, w, x0, y0) in enumerate(geom)]
    store = {"hw": np.array([H, W]), "dst_image": img, "dst_masks": masks, "dst_boxes": boxes, "dst_labels": labels,
             "K": np.array(len(pastes)), "seq_draws": np.array(SEQ_DRAWS)}
    for k, (rgba, x0, y0, lab) in enumerate(pastes):
        store["src%d_rgba" % k], store["src%d_xy" % k], store["src%d_label" % k] = rgba, np.array([x0, y0]), np.array([lab])
    for name, methods, seed in CASES:
        fake = types.SimpleNamespace(bbox_occluded_thr=10, mask_occluded_thr=300, cp_method=list(methods))
        dst = {"image": img.copy(), "gt_masks": masks.copy(), "gt_bboxes": boxes.copy(), "gt_labels": labels.copy(),
               "instance_source": np.zeros(n0, dtype=np.int64)}
        random.seed(seed)
        del drawn[:]
        steps, mism, frame_changed = [], 0, []
        for rgba, x0, y0, lab in pastes:
            canvas, cmask = MB.place(rgba, x0, y0)
            before = dst["image"].copy()
            src = {"image": canvas, "gt_masks": cmask, "gt_bboxes": mp.get_bboxes(cmask), "gt_labels": np.array([lab], dtype=np.int64)}
            dst = mp.InstPool._copy_paste(fake, dst, src)
            steps.append(dst["image"])
            if drawn[-1] == "possion":
                mine, _, U = PR.solve(before, canvas[:3], cmask[0])
                d = dst["image"].astype(np.int64) - mine.astype(np.int64)
                assert np.abs(d).max() <= 1, (name, len(steps), np.abs(d).max())
                mism += int((d != 0).sum())
                fr = PR.unknowns(np.zeros((H, W), bool)) & (cmask[0] == 0)
                frame_changed.append(int((dst["image"] != before)[:, fr].sum()))
        print(name, "modes", drawn, "mismatches", mism, "frame bytes changed outside F per possion paste", frame_changed)
        store.update({"%s_methods" % name: np.array(methods), "%s_seed" % name: np.array(seed),
                      "%s_modes" % name: np.array([CODES[m] for m in drawn], dtype=np.uint8),
                      "%s_steps" % name: np.stack(steps), "%s_out_masks" % name: dst["gt_masks"].astype(np.uint8),
                      "%s_out_boxes" % name: dst["gt_bboxes"], "%s_out_labels" % name: dst["gt_labels"],
                      "%s_out_source" % name: dst["instance_source"],
                      "%s_ref_vs_restated_mismatches" % name: np.array(mism)})
        # the draw sequence itself, longer than one image's pastes: `random.sample(cp_method, 1)` SEQ_DRAWS times from the same seed
        random.seed(seed)
        del drawn[:]
        for _ in range(SEQ_DRAWS):
            sample(list(methods), 1)
        store["%s_seq" % name] = np.array([CODES[m] for m in drawn], dtype=np.uint8)
    assert set(store["mixed4_modes"].tolist()) == {0, 1, 2, 3}, store["mixed4_modes"]
    MB.save_deterministic(os.path.join(HERE, "poisson_blend.npz"), store)


if __name__ == "__main__":
    main()
