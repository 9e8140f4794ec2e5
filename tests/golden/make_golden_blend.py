"""Generate tests/golden/blend_modes.npz: the reference's own InstPool._copy_paste -> blend_image
(DG/divergen/data/custom_build_copypaste_mapper.py:510-566, DG/divergen/data/transforms/custom_cp_method.py:5-18) with
INPUT.CP_METHOD lists other than ['basic'], on a small seeded fixture.  Run in the authoring container only:

    python tests/golden/make_golden_blend.py

Stored: the inputs, the method blend_image drew for every paste (its `random.sample` is wrapped by a recorder, the same trick
make_golden.py uses for cv2.resize; `random` seeded as D2's seed_all_rng seeds it), the image after every paste and the final
masks / boxes / labels / instance_source.  'basic' and 'alpha' run the reference unmodified.  cv2 is absent: cv2.blur is a
stand-in written here (normalised 5x5 box, centre anchor, BORDER_REFLECT_101, m = (float)((double)count * (1.0 / 25))), so
'gaussian' parity vs cv2 is unpinned here.  The file is written with fixed zip timestamps: two runs give identical bytes."""
import io
import os
import random
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload as R  # noqa: E402

H, W = 60, 80
SEQ_DRAWS = 31
CASES = [("mixed", ["basic", "alpha", "gaussian"], 3), ("alpha", ["alpha"], 6), ("gaussian", ["gaussian"], 7),
         ("basic_alpha", ["basic", "alpha"], 8)]


def blur_standin(src, ksize):
    """cv2.blur(src float32 (H, W), (5, 5)) for a 0/1 mask: box sum over the reflect-101 neighbourhood, count / 25."""
    assert tuple(ksize) == (5, 5) and src.dtype == np.float32 and src.ndim == 2
    h, w = src.shape
    assert h >= 3 and w >= 3

    def refl(i, n):
        i = abs(i)
        return 2 * n - 2 - i if i >= n else i
    out = np.zeros((h, w), np.float32)
    for y in range(h):
        for x in range(w):
            cnt = 0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cnt += int(src[refl(y + dy, h), refl(x + dx, w)])
            out[y, x] = np.float32(np.float64(cnt) * (1.0 / 25))
    return out


def soft_patch(rng, h, w):
    """RGBA patch with a soft elliptical alpha edge: 255 inside, a ramp through 1..254, 0 in the corners."""
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.sqrt(((xx + 0.5 - w / 2) / (w / 2)) ** 2 + ((yy + 0.5 - h / 2) / (h / 2)) ** 2)
    rgba[..., 3] = np.clip((1.0 - d) * 700.0, 0, 255).astype(np.uint8)
    return rgba


def place(rgba, x0, y0):
    """pad_to_hw's integer-translate warpAffine: shifted copy, zero border -> image (4,H,W), mask (1,H,W)."""
    h, w = rgba.shape[:2]
    canvas = np.zeros((4, H, W), np.uint8)
    ys, xs, ye, xe = max(y0, 0), max(x0, 0), min(y0 + h, H), min(x0 + w, W)
    canvas[:, ys:ye, xs:xe] = rgba[ys - y0:ye - y0, xs - x0:xe - x0].transpose(2, 0, 1)
    return canvas, (canvas[3:4] > 0).astype(np.uint8)


def save_deterministic(path, arrs):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrs[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print("wrote %s %.1f KB keys=%d" % (os.path.basename(path), os.path.getsize(path) / 1024, len(arrs)))


def main():
    mp = R.ref("divergen.data.custom_build_copypaste_mapper")
    cm = R.ref("divergen.data.transforms.custom_cp_method")
    assert mp.blend_image is cm.blend_image
    cm.cv2.blur = blur_standin
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
    # overlapping interior pastes, then the four corners (every edge, negative offsets, overhang)
    geom = [(22, 26, 18, 12), (20, 24, 30, 20), (16, 18, -6, -5), (20, 24, W - 15, H - 12), (14, 16, W - 10, -4),
            (18, 20, -5, H - 9)]
    pastes = [(soft_patch(rng, h, w), x0, y0, 1000 + k) for k, (h, w, x0, y0) in enumerate(geom)]
    store = {"hw": np.array([H, W]), "dst_image": img, "dst_masks": masks, "dst_boxes": boxes, "dst_labels": labels,
             "K": np.array(len(pastes)), "seq_draws": np.array(SEQ_DRAWS)}
    for k, (rgba, x0, y0, lab) in enumerate(pastes):
        store["src%d_rgba" % k], store["src%d_xy" % k], store["src%d_label" % k] = rgba, np.array([x0, y0]), np.array([lab])
    codes = {"basic": 0, "alpha": 1, "gaussian": 2}
    for name, methods, seed in CASES:
        fake = types.SimpleNamespace(bbox_occluded_thr=10, mask_occluded_thr=300, cp_method=list(methods))
        dst = {"image": img.copy(), "gt_masks": masks.copy(), "gt_bboxes": boxes.copy(), "gt_labels": labels.copy(),
               "instance_source": np.zeros(n0, dtype=np.int64)}
        random.seed(seed)
        del drawn[:]
        steps = []
        for rgba, x0, y0, lab in pastes:
            canvas, cmask = place(rgba, x0, y0)
            src = {"image": canvas, "gt_masks": cmask, "gt_bboxes": mp.get_bboxes(cmask), "gt_labels": np.array([lab], dtype=np.int64)}
            dst = mp.InstPool._copy_paste(fake, dst, src)
            steps.append(dst["image"])
        store.update({"%s_methods" % name: np.array(methods), "%s_seed" % name: np.array(seed),
                      "%s_modes" % name: np.array([codes[m] for m in drawn], dtype=np.uint8),
                      "%s_steps" % name: np.stack(steps), "%s_out_masks" % name: dst["gt_masks"].astype(np.uint8),
                      "%s_out_boxes" % name: dst["gt_bboxes"], "%s_out_labels" % name: dst["gt_labels"],
                      "%s_out_source" % name: dst["instance_source"]})
        # the draw sequence itself, longer than one image's pastes: blend_image called SEQ_DRAWS times from the same seed
        random.seed(seed)
        del drawn[:]
        for _ in range(SEQ_DRAWS):
            cm.blend_image(np.zeros((3, 4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4), np.int64), list(methods))
        store["%s_seq" % name] = np.array([codes[m] for m in drawn], dtype=np.uint8)
    assert set(store["mixed_modes"].tolist()) == {0, 1, 2}, store["mixed_modes"]
    save_deterministic(os.path.join(HERE, "blend_modes.npz"), store)


if __name__ == "__main__":
    main()
