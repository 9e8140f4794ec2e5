"""Image-label co-training ops over libdgx (csrc/image_label.hip, csrc/wsddn_loss.hip): the weakly-supervised proposal lists, the
row-selection image-label losses and the WSDDN loss.
Fixed-length lists with a validity byte per row, host arrays for the per-image offsets and sizes, device CSR for the labels:
an image-labelled step carries no device->host read."""
import ctypes

import torch

from .. import _lib as L
from ..config.image_labels import IMAGE_LABEL_LOSSES, MAX_IMAGES_PER_GPU as MAX_IMAGES
from ..utils.h2d import upload_i32

IMAGE_LABEL_MODES = {name: i for i, name in enumerate(IMAGE_LABEL_LOSSES)}      # DGX_IL_* of include/divergen_hip.h


def _sizes(image_sizes):
    B = len(image_sizes)
    return ((ctypes.c_float * B)(*[float(s[0]) for s in image_sizes]), (ctypes.c_float * B)(*[float(s[1]) for s in image_sizes]))


def ws_proposals(boxes, scores, valid, image_sizes, ws_num_props, add_image_box, image_box_size):
    """get_top_proposals + _add_image_box (DG detic_roi_heads.py:341-365) for the whole batch: boxes (B, K, 4), scores (B, K),
    valid (B, K) bool / uint8 or None -> (B*Ko, 4) boxes, (B*Ko,) logits, (B*Ko,) uint8 validity, Ko."""
    B, K = int(boxes.shape[0]), int(boxes.shape[1])
    if B > MAX_IMAGES:
        raise L.DgxError("ws_proposals: %d images in one batch (at most %d)" % (B, MAX_IMAGES))
    Ko = int(ws_num_props) + (1 if add_image_box else 0)
    dev = boxes.device
    boxes, scores = boxes.detach().float().contiguous(), scores.detach().float().contiguous()
    if valid is not None:
        valid = (valid.view(torch.uint8) if valid.dtype == torch.bool else valid).contiguous()
    ob = torch.empty(B * Ko, 4, dtype=torch.float32, device=dev)
    ol = torch.empty(B * Ko, dtype=torch.float32, device=dev)
    ov = torch.empty(B * Ko, dtype=torch.uint8, device=dev)
    ih, iw = _sizes(image_sizes)
    L.check(L.lib().dgx_ws_proposals(L.ptr(boxes), L.ptr(scores), L.ptr(valid), B, K, ih, iw, int(ws_num_props), 1 if add_image_box else 0,
                                     float(image_box_size), L.ptr(ob), L.ptr(ol), L.ptr(ov), L.stream()), "dgx_ws_proposals")
    return ob, ol, ov, Ko


def label_csr(image_labels, device):
    """list of per-image label lists -> (label_off (B+1) i32, labels i32 or None) on `device` (one asynchronous upload)."""
    offs, flat = [0], []
    for ls in image_labels:
        flat.extend(int(l) for l in ls)
        offs.append(len(flat))
    both = upload_i32(offs + flat, device)
    n = len(offs)
    return both[:n], (both[n:] if flat else None), len(flat)


class _ImageLabelLoss(torch.autograd.Function):
    """image_loss of one cascade stage.  forward: selection + loss + statistics (no gradient written); backward: the dense
    gradient for the saved selections in one launch, the upstream gradient read on the device."""

    @staticmethod
    def forward(ctx, scores, valid, boxes, counts, image_sizes, label_off, labels, num_labels, mode, weight):
        if scores.dim() != 2 or scores.stride(1) != 1 or scores.stride(0) < scores.shape[1]:
            scores = scores.contiguous()
        R, C1 = int(scores.shape[0]), int(scores.shape[1])
        ld = int(scores.stride(0)) if R > 1 else C1     # (a single row has no stride to speak of)
        B = len(counts)
        if B > MAX_IMAGES:
            raise L.DgxError("image_label_loss: %d images in one batch (at most %d)" % (B, MAX_IMAGES))
        if sum(counts) != R:
            raise L.DgxError("image_label_loss: %d rows of scores for %d proposal rows" % (R, sum(counts)))
        dev = scores.device
        row0 = (ctypes.c_int * (B + 1))(*([0] + [sum(counts[:i + 1]) for i in range(B)]))
        ih, iw = _sizes(image_sizes)
        boxes = boxes.detach().float().contiguous()
        lib = L.lib()
        out = torch.empty(8, dtype=torch.float32, device=dev)
        sel = torch.full((max(num_labels, 1),), -1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(lib.dgx_image_label_workspace_floats(R, B)), 1), dtype=torch.float32, device=dev)
        args = (ld, L.ptr(valid), L.ptr(boxes) if R else None, B, row0, ih, iw, L.ptr(label_off), L.ptr(labels), C1 - 1, int(mode),
                float(weight))
        L.check(lib.dgx_image_label_loss(scores.data_ptr() if R else None, *args, None, None, L.ptr(sel), L.ptr(out), None, 0, L.ptr(ws),
                                         L.dtype_code(scores), L.stream()), "dgx_image_label_loss")
        ctx.args, ctx.keep = args, (valid, boxes, label_off, labels)      # the pointers in `args` stay alive with these
        ctx.save_for_backward(sel, scores)
        ctx.shape, ctx.ld, ctx.dt = (R, C1), ld, scores.dtype
        ctx.mark_non_differentiable(out, sel)
        return out[0], out, sel

    @staticmethod
    def backward(ctx, g, _o, _s):
        sel, scores = ctx.saved_tensors
        R, C1 = ctx.shape
        if R == 0:
            return (torch.zeros(0, C1, dtype=ctx.dt, device=sel.device),) + (None,) * 9
        ldg = -(-C1 // 8) * 8                            # 16-byte rows in either dtype
        d = torch.empty(R, ldg, dtype=ctx.dt, device=sel.device)
        g = g.detach().float().reshape(1).contiguous()
        L.check(L.lib().dgx_image_label_loss(scores.data_ptr(), *ctx.args, L.ptr(sel), L.ptr(g), None, None, L.ptr(d), ldg, None, L.dtype_code(d), L.stream()),
                "dgx_image_label_loss (gradient)")
        return (d[:, :C1],) + (None,) * 9


def image_label_loss(scores, valid, boxes, counts, image_sizes, image_labels, mode, weight, csr=None):
    """scores (R, C+1) f32 | bf16 (rows may be strided: a column slice of the joint predictor output), valid (R,) uint8 or None,
    boxes (R, 4), counts / image_sizes per image, image_labels: per-image lists of category ids.
    Returns (image_loss, out8, sel): out8 = [image_loss, stats_l_image, pool_stats, stats_select_size, stats_select_x,
    stats_select_y, stats_max_label_score, 0] on the device, sel the selected row per (image, label) (-1 = none)."""
    if not scores.is_cuda:
        raise L.DgxError("libdgx ops need GPU (ROCm) tensors; got a %s tensor -- no CPU fallback exists" % scores.device)
    if isinstance(mode, str):
        mode = IMAGE_LABEL_MODES[mode]
    off, lab, n = csr if csr is not None else label_csr(image_labels, scores.device)
    return _ImageLabelLoss.apply(scores, valid, boxes, list(counts), list(image_sizes), off, lab, n, mode, weight)


def _rows(t):
    """(tensor, leading dimension) of a row-major 2-d operand: strided rows (a column slice) are taken as they are."""
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]))


class _WsddnLoss(torch.autograd.Function):
    """image_loss of one cascade stage under IMAGE_LABEL_LOSS 'wsddn'.  forward: loss, arg-max rows and statistics, the column
    statistics kept; backward: both dense gradients from one launch over the two inputs, the upstream gradient read on the device."""

    @staticmethod
    def forward(ctx, scores, prop_scores, valid, boxes, counts, image_sizes, label_off, labels, num_labels, weight):
        if prop_scores.dtype != scores.dtype:
            raise L.DgxError("wsddn_loss: scores are %s, proposal scores %s -- one dtype for both" % (scores.dtype, prop_scores.dtype))
        (scores, ld), (prop_scores, ldp) = _rows(scores), _rows(prop_scores)
        R, C1 = int(scores.shape[0]), int(scores.shape[1])
        B = len(counts)
        if B > MAX_IMAGES:
            raise L.DgxError("wsddn_loss: %d images in one batch (at most %d)" % (B, MAX_IMAGES))
        if sum(counts) != R or tuple(prop_scores.shape) != (R, C1):
            raise L.DgxError("wsddn_loss: scores %s, proposal scores %s for %d proposal rows" % (tuple(scores.shape), tuple(prop_scores.shape), sum(counts)))
        dev = scores.device
        row0 = (ctypes.c_int * (B + 1))(*([0] + [sum(counts[:i + 1]) for i in range(B)]))
        ih, iw = _sizes(image_sizes)
        boxes = boxes.detach().float().contiguous()
        lib = L.lib()
        out = torch.empty(8, dtype=torch.float32, device=dev)
        sel = torch.full((max(num_labels, 1),), -1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(lib.dgx_wsddn_workspace_floats(R, B, C1 - 1)), 1), dtype=torch.float32, device=dev)
        head = (scores.data_ptr() if R else None, ld, prop_scores.data_ptr() if R else None, ldp, L.ptr(valid), L.ptr(boxes) if R else None,
                B, row0, ih, iw, L.ptr(label_off), L.ptr(labels), C1 - 1, float(weight))
        L.check(lib.dgx_wsddn_loss(*head, None, None, L.ptr(sel), L.ptr(out), None, 0, None, 0, L.ptr(ws), L.dtype_code(scores), L.stream()),
                "dgx_wsddn_loss")
        ctx.head, ctx.keep = head, (valid, boxes, label_off, labels)      # the pointers in `head` stay alive with these
        ctx.save_for_backward(ws, scores, prop_scores)
        ctx.shape, ctx.dt = (R, C1), scores.dtype
        ctx.mark_non_differentiable(out, sel)
        return out[0], out, sel

    @staticmethod
    def backward(ctx, g, _o, _s):
        ws, scores, prop_scores = ctx.saved_tensors
        R, C1 = ctx.shape
        if R == 0:
            z = torch.zeros(0, C1, dtype=ctx.dt, device=ws.device)
            return (z, z.clone()) + (None,) * 8
        ldg = -(-C1 // 8) * 8                            # 16-byte rows in either dtype
        d = torch.empty(2, R, ldg, dtype=ctx.dt, device=ws.device)
        g = g.detach().float().reshape(1).contiguous()
        L.check(L.lib().dgx_wsddn_loss(*ctx.head, L.ptr(ws), L.ptr(g), None, None, d[0].data_ptr(), ldg, d[1].data_ptr(), ldg, None,
                                       L.dtype_code(d), L.stream()), "dgx_wsddn_loss (gradient)")
        return (d[0][:, :C1], d[1][:, :C1]) + (None,) * 8


def wsddn_loss(scores, prop_scores, valid, boxes, counts, image_sizes, image_labels, weight, csr=None):
    """The WSDDN image-label loss (DG detic_fast_rcnn.py:509-521): scores, prop_scores (R, C+1) f32 | bf16 (rows may be strided),
    the other arguments as image_label_loss.  Returns (image_loss, out8, sel): out8 as image_label_loss, sel the arg-max row of
    sigmoid(score) x softmax-over-proposals(prop_score) per (image, label) (-1 = none)."""
    if not scores.is_cuda or not prop_scores.is_cuda:
        raise L.DgxError("libdgx ops need GPU (ROCm) tensors; got a %s tensor -- no CPU fallback exists"
                         % (scores.device if not scores.is_cuda else prop_scores.device))
    off, lab, n = csr if csr is not None else label_csr(image_labels, scores.device)
    return _WsddnLoss.apply(scores, prop_scores, valid, boxes, list(counts), list(image_sizes), off, lab, n, weight)
