"""numpy restatement of one self copy-paste step (Simple Copy-Paste between two real images) as include/divergen_hip.h states it
for dgx_self_copy_paste and divergen_amd.layers.self_copy_paste returns it.  Test helper: tests/test_host_self_copy.py pins it on
the reference's own CopyPaste.__call__ outputs (tests/golden/self_copy.npz), tests/test_gpu_self_copy.py compares the kernel with it.
Semantics: DG/divergen/data/transforms/custom_copypaste.py:343-389 (_scp_src_to_dst), :413-426 (get_bboxes), :428-506 (_copy_paste)."""
import math

import numpy as np


def canvas_hw(dst_hw, sel_boxes):
    """max(destination size, ceil of the largest y2 / x2 among the selected source boxes)."""
    return max(int(dst_hw[0]), math.ceil(sel_boxes[..., 3].max())), max(int(dst_hw[1]), math.ceil(sel_boxes[..., 2].max()))


def pad_to_hw(data, h, w):
    """zero-pad or crop the planes of (c, h0, w0) to (c, h, w)."""
    out = np.zeros((data.shape[0], h, w), dtype=data.dtype)
    dh, dw = min(h, data.shape[1]), min(w, data.shape[2])
    out[:, :dh, :dw] = data[:, :dh, :dw]
    return out


def mask_boxes(masks):
    """(x_min, y_min, x_max + 1, y_max + 1) per mask, zeros for an empty one; float32."""
    boxes = np.zeros((len(masks), 4), dtype=np.float32)
    for i, mk in enumerate(masks):
        ys, xs = np.nonzero(mk)
        if len(xs):
            boxes[i] = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
    return boxes


def self_copy(dst_image, dst_masks, dst_boxes, dst_labels, src_image, src_masks, src_boxes, src_labels, sel):
    """One paste step.  dst_* / src_*: image uint8 (3,h,w), masks uint8 (n,h,w) 0/1, boxes f32 (n,4), labels i64 (n); sel: the
    selected source objects in paste order.  Returns dict(image, masks, boxes, labels, valid) with the surviving destination objects
    first, then the selected source objects with their own boxes; `valid`: the filter's verdict per destination object.
    m == 0: the inputs as they are."""
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    n0 = len(dst_masks)
    if len(sel) == 0:
        return dict(image=dst_image, masks=dst_masks, boxes=dst_boxes, labels=dst_labels, valid=np.ones(n0, dtype=bool))
    sb, sl, sm = src_boxes[sel], src_labels[sel], src_masks[sel]
    H, W = canvas_hw(dst_image.shape[-2:], sb)
    d_img, d_m = pad_to_hw(dst_image, H, W), pad_to_hw(dst_masks, H, W)
    s_img, s_m = pad_to_hw(src_image, H, W), pad_to_hw(sm, H, W)
    composed = s_m.any(axis=0)
    upd = np.where(composed[None], 0, d_m).astype(dst_masks.dtype)
    nb = mask_boxes(upd)
    valid = np.all(np.abs(nb - dst_boxes.astype(np.float32).reshape(-1, 4)) <= 10, axis=-1) | ((upd != 0).sum(axis=(1, 2)) > 300)
    image = np.where(composed[None], s_img, d_img).astype(dst_image.dtype)
    return dict(image=image, masks=np.concatenate([upd[valid], s_m]), boxes=np.concatenate([nb[valid], sb.astype(np.float32)]),
                labels=np.concatenate([dst_labels[valid], sl]), valid=valid)
