"""numpy restatement of what INPUT.SCP_SRC_MODES adds on the device, as include/divergen_hip.h states it for dgx_remove_background and
dgx_self_copy_paste_all.  Test helper: tests/test_host_scp_modes.py pins it on the reference's own CopyPaste.remove_background and
CopyPaste(selected=False).__call__ outputs (tests/golden/scp_modes.npz), tests/test_gpu_scp_modes.py compares the kernels with it.
Semantics: DG/divergen/data/transforms/custom_copypaste.py:101-109 (remove_background), :282-283 (no _select_object)."""
import numpy as np

import _selfcopy_ref as SR


def remove_background(image, masks):
    """image uint8 (3,h,w) where some mask (n,h,w; any non-zero byte) has the pixel, 0 elsewhere; n == 0: all zero."""
    return image * (masks != 0).any(axis=0).astype(image.dtype)[None]


def paste_all(dst_image, dst_masks, dst_boxes, dst_labels, src_image, src_masks, src_boxes, src_labels):
    """One paste step with every source object in its order (ns == 0: the inputs as they are)."""
    return SR.self_copy(dst_image, dst_masks, dst_boxes, dst_labels, src_image, src_masks, src_boxes, src_labels, np.arange(len(src_masks)))
