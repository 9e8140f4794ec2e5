"""Numpy restatement of the copy-paste blend modes (INPUT.CP_METHOD; DG/divergen/data/transforms/custom_cp_method.py:5-18) as
include/divergen_hip.h states them for dgx_copy_paste_blend.  Test helper: tests/test_host_blend_modes.py pins it on
tests/golden/blend_modes.npz (the reference's own blend_image), tests/test_gpu_blend_modes.py checks the kernel against it.
Masks, boxes, labels and instance_source come from oracle.compositor: they do not depend on the mode."""
import numpy as np

from oracle import compositor as OK

MODES = {"basic": 0, "alpha": 1, "gaussian": 2}
# m = cv2.blur of a 0/1 mask = count / 25, as float32 from the double product (OpenCV's generic double-sum path)
BLUR_TABLE = np.array([np.float32(np.float64(c) * (1.0 / 25)) for c in range(26)], dtype=np.float32)


def reflect101(i, n):
    """BORDER_REFLECT_101 index map for i in [-2, n + 1], n >= 3."""
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def blur5(footprint):
    """cv2.blur(F.astype('float32'), (5, 5)) of a 0/1 (H, W) mask: 5x5 box, centre anchor, reflect-101 at the image border."""
    H, W = footprint.shape
    assert H >= 3 and W >= 3, "reflect-101 needs 3 pixels per side"
    f = footprint.astype(np.int64)
    ry, rx = reflect101(np.arange(-2, H + 2), H), reflect101(np.arange(-2, W + 2), W)
    pad = f[ry][:, rx]
    rows = sum(pad[:, d:d + W] for d in range(5))
    cnt = sum(rows[d:d + H] for d in range(5))
    return BLUR_TABLE[cnt]


def blend(dst, src, alpha, mode):
    """One paste on the image left by the previous one.  dst u8 (3,H,W); src u8 (3,H,W) placed RGB (0 outside the rectangle);
    alpha u8 (H,W) placed alpha (0 outside).  Returns u8 (3,H,W), truncated like `.astype(dst_img.dtype)`."""
    mode = MODES.get(mode, mode)
    if mode == 0:
        return np.where(alpha > 0, src, dst).astype(np.uint8)
    if mode == 1:
        a = alpha.astype(np.float64) / 255.0
        r = dst.astype(np.float64) * (1.0 - a) + src.astype(np.float64) * a
        return r.astype(np.uint8)
    if mode == 2:
        m = blur5(alpha > 0)
        r = dst.astype(np.float32) * (np.float32(1) - m) + src.astype(np.float32) * m
        return r.astype(np.uint8)
    raise ValueError(mode)


def blend_chain(image, pastes, modes):
    """image u8 (3,H,W); pastes [(rgba (h,w,4), x0, y0, label)]; modes: names or codes.  Returns the image after every paste."""
    H, W = image.shape[1:]
    out, steps = image.copy(), []
    for (rgba, x0, y0, _), mode in zip(pastes, modes):
        placed, _ = OK.place(np.asarray(rgba), int(x0), int(y0), H, W)
        out = blend(out, placed[:3], placed[3], mode)
        steps.append(out)
    return steps


def composite(image, masks, boxes, labels, pastes, modes):
    """oracle.compositor.composite with the image blended per `modes`: the final dict (image, masks, boxes, labels, source)."""
    ref = OK.composite(image, masks, boxes, labels, pastes)
    steps = blend_chain(image, pastes, modes)
    ref["image"] = steps[-1] if steps else image.copy()
    return ref
