"""numpy restatement of self copy-paste from several source images (INPUT.SCP_NUM_SRC > 1) as include/divergen_hip.h states it for
dgx_self_copy_merge and divergen_amd.layers.self_copy_paste_multi returns it: the fold of CopyPaste.__call__
(DG/divergen/data/transforms/custom_copypaste.py:274-297) built on _selfcopy_ref.self_copy plus the temporary-stage canvas rule
(:343-353 with is_tmp_dst).  Test helper: tests/test_host_self_copy_multi.py pins it on the reference's own outputs
(tests/golden/self_copy_multi.npz), tests/test_gpu_self_copy_multi.py compares the kernels with it."""
import math

import numpy as np

import _selfcopy_ref as SR


def tmp_canvas(acc_boxes, src_boxes):
    """(h, w) of a temporary stage: the ceil of the largest y2 / x2 among the accumulator's boxes and the source's; no image size."""
    return (max(math.ceil(acc_boxes[..., 3].max()), math.ceil(src_boxes[..., 3].max())),
            max(math.ceil(acc_boxes[..., 2].max()), math.ceil(src_boxes[..., 2].max())))


def merge(sources):
    """sources: list of (image uint8 (3,h,w), masks uint8 (m,h,w), boxes f32 (m,4), labels i64 (m)) -- the SELECTED objects of each
    source image, in order; sources with m == 0 are skipped.  Returns None when none is left, else dict(image, masks, boxes, labels:
    the accumulator the final paste takes as its source; rows: for each accumulator object its row among the M = sum m_i planes of
    the sources that were not skipped; valid (M) bool; hw: the stage canvases)."""
    sources = [s for s in sources if len(s[2])]
    if not sources:
        return None
    img, masks, boxes, labels = sources[0]
    boxes, rows, hw = boxes.astype(np.float32), np.arange(len(boxes)), []
    for s_img, s_m, s_b, s_l in sources[1:]:
        h, w = tmp_canvas(boxes, s_b)
        hw.append((h, w))
        # both sides cropped / zero-padded to the canvas, for good; then one ordinary step (its canvas: max((h, w), the source's
        # boxes) = (h, w) again)
        r = SR.self_copy(SR.pad_to_hw(img, h, w), SR.pad_to_hw(masks, h, w), boxes, labels, SR.pad_to_hw(s_img, h, w),
                         SR.pad_to_hw(s_m, h, w), s_b, s_l, np.arange(len(s_b)))
        assert tuple(r["image"].shape[-2:]) == (h, w)
        img, masks, boxes, labels = r["image"], r["masks"], r["boxes"], r["labels"]
        seen = sum(len(x[2]) for x in sources[:len(hw)])      # planes of the sources before this one
        rows = np.concatenate([rows[r["valid"]], seen + np.arange(len(s_b))])
    M = sum(len(s[2]) for s in sources)
    valid = np.zeros(M, dtype=bool)
    valid[rows] = True
    return dict(image=img, masks=masks, boxes=boxes, labels=labels, rows=rows, valid=valid, hw=hw)


def self_copy_multi(dst_image, dst_masks, dst_boxes, dst_labels, sources):
    """The whole of CopyPaste.__call__ after the selection: merge, then the accumulator pasted onto the destination.  Returns
    _selfcopy_ref.self_copy's dict (valid: the destination objects') plus `merge` (merge's dict, None when every source is empty)."""
    acc = merge(sources)
    if acc is None:
        out = SR.self_copy(dst_image, dst_masks, dst_boxes, dst_labels, dst_image, dst_masks[:0], dst_boxes[:0], dst_labels[:0], [])
    else:
        out = SR.self_copy(dst_image, dst_masks, dst_boxes, dst_labels, acc["image"], acc["masks"], acc["boxes"], acc["labels"],
                           np.arange(len(acc["boxes"])))
    return dict(out, merge=acc)
