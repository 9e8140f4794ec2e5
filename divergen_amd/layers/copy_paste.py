"""Instance copy-paste compositor on the GPU: the 'basic', 'alpha', 'gaussian' and (opt-in) 'possion' blends of all K pastes of an
image in one libdgx call (copy_paste), one 'possion' paste alone (poisson_blend), the self copy between two real images
(self_copy_paste; self_copy_paste_all for a source pasted whole) and from several source images (self_copy_merge, self_copy_paste_multi),
background removal (remove_background).  Reference: DG/divergen/data/custom_build_copypaste_mapper.py:488-566, :79-92; custom_cp_method.py:5-18."""
import numpy as np
import torch

from .. import _lib as L
from ..utils.h2d import upload_i32


BLEND_MODES = {"basic": 0, "alpha": 1, "gaussian": 2}      # the mode bytes of dgx_copy_paste_blend (include/divergen_hip.h)
BLEND_MODES_ALL = {**BLEND_MODES, "possion": 3}            # + the opt-in Poisson blend (the reference's spelling): dgx_copy_paste_blend_ws
POISSON = BLEND_MODES_ALL["possion"]
# the solver report at the head of the 'possion' workspace: PB_REPORT_RECORDS records of PB_REPORT_DOUBLES fp64 (csrc/poisson_blend.h)
POISSON_REPORT_RECORDS = 32
POISSON_REPORT_FIELDS = 4      # (iterations, ||r||_2, converged, |U|)


def host_modes(modes, K, allow_poisson=False):
    """modes (None | sequence of names or codes | uint8 array / CPU tensor) -> uint8 numpy (K,) in host memory, or None when every
    paste is 'basic' (then the compositor launches exactly the kernels of dgx_copy_paste).  allow_poisson: 'possion' / code 3 pass."""
    if modes is None:
        return None
    top = POISSON if allow_poisson else max(BLEND_MODES.values())      # the highest code admitted
    admitted = sorted((c, n) for n, c in BLEND_MODES_ALL.items() if c <= top)
    if isinstance(modes, torch.Tensor):
        modes = modes.cpu().numpy()
    if isinstance(modes, np.ndarray):
        if modes.dtype.kind not in "iu":
            raise ValueError("copy_paste: blend modes as an array must be integer codes, got dtype %s" % modes.dtype)
        vals = modes.reshape(-1).tolist()
    else:
        vals = list(modes)            # element by element: a mixed list of names and codes keeps its codes
    for v in vals:
        if isinstance(v, str) and BLEND_MODES_ALL.get(v, top + 1) > top:
            raise ValueError("copy_paste: unknown blend mode '%s' (%s)" % (v, ", ".join(sorted(n for _, n in admitted))))
    m = np.array([BLEND_MODES_ALL[v] if isinstance(v, str) else int(v) for v in vals], dtype=np.int64)
    if m.shape[0] != K:
        raise ValueError("copy_paste: %d blend modes for %d pastes" % (m.shape[0], K))
    if ((m < 0) | (m > top)).any():
        raise ValueError("copy_paste: blend mode codes are %s; got %s" % (", ".join("%d (%s)" % cn for cn in admitted), m.tolist()))
    return m.astype(np.uint8) if m.any() else None


class PackedPastes:
    """The K paste patches of one image as the kernel takes them: ONE flat uint8 buffer (the RGBA patches back to back) + the
    (K, 5) int32 descriptors (byte offset, h, w, x0, y0) + the K labels, all on the device; `modes`: the K blend-mode bytes
    (BLEND_MODES) in HOST memory, None = all 'basic'; `desc_host`: the descriptors once more as a host int32 array (K, 5) when the
    packer had them there (only a 'possion' paste needs them: its workspace is sized from the paste's rectangle), else None."""

    def __init__(self, flat, desc, labels, K, modes=None, desc_host=None):
        self.flat, self.desc, self.labels, self.K, self.modes, self.desc_host = flat, desc, labels, K, modes, desc_host

    def __len__(self):
        return self.K

    def host_desc(self):
        """The descriptors in host memory: `desc_host`, or else ONE device -> host copy of `desc`."""
        return self.desc_host if self.desc_host is not None else self.desc.cpu().numpy()


def _layout(pastes):
    """list of (rgba (h, w, 4), x0, y0, label) -> ((K, 5) int32 numpy descriptors (byte offset, h, w, x0, y0), bytes of the flat buffer,
    labels int64 numpy (K)).  A patch takes h * w * 4 bytes, so every patch starts on a 4-byte boundary without padding."""
    desc, off = [], 0
    for rgba, x0, y0, _ in pastes:
        h, w = int(rgba.shape[0]), int(rgba.shape[1])
        desc.append([off, h, w, int(x0), int(y0)])
        off += h * w * 4
    labels = np.array([int(np.asarray(p[3]).reshape(-1)[0]) for p in pastes], dtype=np.int64)
    return np.asarray(desc, dtype=np.int32).reshape(-1, 5), off, labels


def pack_pastes_host(pastes):
    """list of (rgba uint8 (h, w, 4) numpy, x0, y0, label) -> (flat uint8, desc int32 (K, 5), labels int64 (K)) as CPU tensors:
    what a LOADER WORKER hands the training process for one image (no device, no libdgx).  K = 0 gives a 4-byte flat buffer.  A patch that
    is still a structures.DeviceResizePatch (INPUT.DEVICE_RESIZE) gets its range of `flat` but no bytes: the resize kernel writes them."""
    from ..structures import DeviceResizePatch
    desc, nbytes, labels = _layout(pastes)
    host = np.zeros(max(nbytes, 4), dtype=np.uint8)
    for (rgba, _, _, _), d in zip(pastes, desc.tolist()):
        if isinstance(rgba, DeviceResizePatch):
            continue
        n = d[1] * d[2] * 4
        a = rgba.detach().cpu().numpy() if isinstance(rgba, torch.Tensor) else np.asarray(rgba)
        host[d[0]:d[0] + n] = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    return torch.from_numpy(host), torch.from_numpy(desc), torch.from_numpy(labels)


def pack_pastes(pastes, device, modes=None, allow_poisson=False):
    """list of (rgba uint8 (h, w, 4) numpy | tensor, x0, y0, label) -> PackedPastes.  modes: K blend modes (names or BLEND_MODES
    codes), None = all 'basic'; allow_poisson: `modes` may name 'possion' (checked here, so that a wrong name fails where it is
    given).  Host arrays (the loader's case: patches come out of the instance pool in host memory) are laid out in one host buffer
    and go up in ONE copy; patches that already live on the device are gathered with one concatenation.  Round 2 concatenated 2 K
    device chunks per image inside every step, which torch executes as one hipMemcpyAsync per chunk: 38 blit launches of ~10 us
    per image (0.8 ms per step on the loader stream)."""
    K = len(pastes)
    if modes is not None:
        host_modes(modes, K, allow_poisson)
    on_dev = [isinstance(r, torch.Tensor) and r.is_cuda for r, _, _, _ in pastes]
    if K and all(on_dev):
        desc, _, labels = _layout(pastes)
        flat = torch.cat([rgba.reshape(-1) for rgba, _, _, _ in pastes])
        return PackedPastes(flat, upload_i32(desc, device).view(-1, 5), upload_i32(labels, device).long(), K, modes, desc)
    flat, desc, labels = pack_pastes_host(pastes)
    desc_host = desc.numpy().copy()
    if torch.device(device).type != "cuda":
        return PackedPastes(flat, desc, labels, K, modes, desc_host)
    flat = flat.pin_memory().to(device, non_blocking=True)
    desc_t = upload_i32(desc.numpy(), device).view(-1, 5) if K else torch.zeros(0, 5, dtype=torch.int32, device=device)
    labels = upload_i32(labels.numpy(), device).long() if K else torch.zeros(0, dtype=torch.int64, device=device)
    return PackedPastes(flat, desc_t, labels, K, modes, desc_host)


def poisson_unknowns(desc_host, H, W):
    """Upper bound of |U| = |F| + frame for one paste descriptor (offset, h, w, x0, y0): the pixels of its rectangle inside the image
    plus the image frame, at most H * W."""
    _, h, w, x0, y0 = (int(v) for v in desc_host)
    ch, cw = min(y0 + h, H) - max(y0, 0), min(x0 + w, W) - max(x0, 0)
    return min(H * W, 2 * H + 2 * W - 4 + (ch * cw if ch > 0 and cw > 0 else 0))


def check_poisson_report(report, modes=None):
    """Read the solver report of copy_paste(..., allow_poisson=True) (a device -> host copy: not for the training path) and raise
    when a 'possion' paste did not converge within its iteration bound.  report: float64 (K, 4) = (iterations, ||r||_2, converged,
    |U|) per paste, zeros for pastes of other modes; modes: the K mode bytes (None: every paste with a non-zero row is checked).
    Returns the report as a numpy array."""
    rep = report.detach().cpu().numpy() if isinstance(report, torch.Tensor) else np.asarray(report)
    for k, (iters, resid, flag, n) in enumerate(rep.tolist()):
        solved = int(modes[k]) == POISSON if modes is not None else (n > 0 or iters > 0 or resid != 0)
        if solved and flag != 1.0:
            raise RuntimeError("copy_paste: the 'possion' solve of paste %d did not converge: %d iterations, |r| = %.3e, %d unknowns"
                               % (k, int(iters), resid, int(n)))
    return rep


def copy_paste(image, masks, boxes, labels, pastes, lazy_masks=False, modes=None, allow_poisson=False):
    """image uint8 (3,H,W), masks uint8 (n,H,W), boxes f32 (n,4), labels i64 (n) -- GPU tensors.
    pastes: list of (rgba uint8 numpy/tensor (h,w,4), x0, y0, label) applied in order, or a PackedPastes (pack_pastes).
    Returns dict(image, masks, boxes, labels, source) exactly like the sequential reference.  Mask bytes pass through (0/1 in,
    0/1 out).  lazy_masks: `masks` holds ALL n + K objects' rows and `keep` (i64) the rows of the surviving ones, in order --
    what structures.BitMasks(masks, index=keep) takes: the full-resolution rows of the survivors are then never gathered
    (the only consumer, crop_and_resize, reads a few rows through the index).
    modes: the K blend modes (names or BLEND_MODES codes, host memory); None takes the PackedPastes' own (None there = all 'basic').
    All 'basic' calls dgx_copy_paste; any other mix dgx_copy_paste_blend.  Masks / boxes / labels / source do not depend on them.
    allow_poisson: 'possion' / code 3 is accepted; with such a paste present the call is dgx_copy_paste_blend_ws with a workspace
    sized for the largest of them, and the result carries `poisson_report`, float64 (K, 4) on the device (check_poisson_report
    reads it; nothing here does).  A pack without host descriptors costs one device -> host copy of them."""
    K = len(pastes)
    dev = image.device
    n0, H, W = masks.shape[0], image.shape[1], image.shape[2]
    if K == 0:
        out = dict(image=image, masks=masks, boxes=boxes, labels=labels, source=torch.zeros(n0, dtype=torch.int64, device=dev))
        if lazy_masks:
            out["keep"] = torch.arange(n0, dtype=torch.int64, device=dev)
        return out
    pk = pastes if isinstance(pastes, PackedPastes) else pack_pastes(pastes, dev)
    hm = host_modes(modes if modes is not None else pk.modes, K, allow_poisson)
    image = image.contiguous().clone()
    masks = masks.contiguous()
    boxes0 = boxes.float().contiguous()
    nobj = n0 + K
    out_masks = torch.empty(nobj, H, W, dtype=torch.uint8, device=dev)
    out_boxes = torch.empty(nobj, 4, dtype=torch.float32, device=dev)
    out_valid = torch.empty(nobj, dtype=torch.uint8, device=dev)
    stats = torch.empty(nobj * (K + 1) * 5 + 3 + H * W, dtype=torch.int32, device=dev)
    args = (L.ptr(image), L.ptr(masks) if n0 else None, L.ptr(boxes0) if n0 else None, n0, H, W, L.ptr(pk.flat), L.ptr(pk.desc), K,
            L.ptr(out_masks), L.ptr(out_boxes), L.ptr(out_valid), L.ptr(stats))
    report = None
    if hm is None:
        entry = "dgx_copy_paste"
    elif not (hm == POISSON).any():
        entry, args = "dgx_copy_paste_blend", args + (hm.ctypes.data,)
    else:
        dh = pk.host_desc()
        work, nbytes = _poisson_work(H, W, max(poisson_unknowns(dh[k], H, W) for k in np.flatnonzero(hm == POISSON)), dev)
        entry, args = "dgx_copy_paste_blend_ws", args + (hm.ctypes.data, L.ptr(work), nbytes)
        report = work[:POISSON_REPORT_RECORDS * POISSON_REPORT_FIELDS].view(POISSON_REPORT_RECORDS, POISSON_REPORT_FIELDS)[:K]
    L.check(getattr(L.lib(), entry)(*args, L.stream()), entry)
    keep = out_valid.nonzero().squeeze(1)          # ONE compaction (and one device->host count) for the four per-object tensors
    all_labels = torch.cat([labels.to(torch.int64), pk.labels])
    source = torch.cat([torch.zeros(n0, dtype=torch.int64, device=dev), torch.ones(K, dtype=torch.int64, device=dev)])
    out = _compacted(image, out_masks, keep, lazy_masks, boxes=out_boxes, labels=all_labels, source=source)
    if report is not None:
        out["poisson_report"] = report
    return out


def _compacted(image, out_masks, keep, lazy_masks, **per_object):
    """The result dict of copy_paste / self_copy_paste: `image`, the per-object tensors (boxes, labels, ...) gathered by `keep` in
    the order given, then `masks` -- gathered too, or with lazy_masks all rows plus `keep`.  `keep` comes in computed: both callers
    take it (the one device -> host count) before they build their per-object tensors."""
    out = dict(image=image, **{name: t.index_select(0, keep) for name, t in per_object.items()})
    if lazy_masks:
        out["masks"], out["keep"] = out_masks, keep
    else:
        out["masks"] = out_masks.index_select(0, keep)
    return out


def _poisson_work(H, W, nmax, dev):
    """The 'possion' solver's workspace for up to nmax unknowns in an (H, W) image -> (fp64 tensor, the report at its head; its bytes)."""
    nbytes = int(L.lib().dgx_poisson_work_bytes(H, W, nmax))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev), nbytes


def poisson_blend(image, rgba, x0, y0, max_iter=-1):
    """ONE 'possion' paste (dgx_poisson_blend) on a copy of image uint8 (3,H,W) (GPU tensor); rgba uint8 (h,w,4) numpy / tensor.
    Returns (image, report float64 (4,) on the device = (iterations, ||r||_2, converged, |U|)).  max_iter < 0: the library's bound."""
    dev = image.device
    H, W = int(image.shape[1]), int(image.shape[2])
    pk = pack_pastes([(rgba, x0, y0, 0)], dev)
    d = np.ascontiguousarray(pk.desc_host[0], dtype=np.int32)
    work, nbytes = _poisson_work(H, W, poisson_unknowns(d, H, W), dev)
    image = image.contiguous().clone()
    L.check(L.lib().dgx_poisson_blend(L.ptr(image), L.ptr(pk.flat), d.ctypes.data, H, W, L.ptr(work), nbytes, int(max_iter),
                                      L.stream()), "dgx_poisson_blend")
    return image, work[:POISSON_REPORT_FIELDS]


SELF_COPY_MAX = 99      # dgx_self_copy_paste: m <= 99 (the reference draws m < min(ns + 1, 100))
SELF_COPY_MAX_SRC = 4   # dgx_self_copy_merge: S <= 4 source images (DGX_SELF_COPY_MAX_SRC): the bound of INPUT.SCP_NUM_SRC
# self_copy_paste's entry of libdgx and the most source objects it takes, by `merged`
_SELF_COPY_ENTRY = {False: ("dgx_self_copy_paste", SELF_COPY_MAX), True: ("dgx_self_copy_paste_merged", SELF_COPY_MAX * SELF_COPY_MAX_SRC)}


def self_copy_canvas(dst_hw, sel_boxes):
    """(H, W) of the canvas of one self copy (custom_copypaste.py:343-353): the destination size, grown to the ceil of the largest
    y2 / x2 among the SELECTED source boxes (host data: numpy / CPU tensor (m, 4), m > 0)."""
    import math
    b = sel_boxes.cpu().numpy() if isinstance(sel_boxes, torch.Tensor) else np.asarray(sel_boxes)
    return max(int(dst_hw[0]), math.ceil(b[..., 3].max())), max(int(dst_hw[1]), math.ceil(b[..., 2].max()))


def _nothing_pasted(image, masks, boxes, labels, lazy_masks):
    """The result of a self copy that pastes no object: the inputs as they are, every row of `masks` kept."""
    out = dict(image=image, masks=masks, boxes=boxes, labels=labels)
    if lazy_masks:
        out["keep"] = torch.arange(int(masks.shape[0]), dtype=torch.int64, device=image.device)
    return out


def self_copy_paste(image, masks, boxes, labels, src_image, src_masks, src_boxes, src_labels, sel, canvas_hw=None, lazy_masks=False,
                    merged=False):
    """Simple Copy-Paste between two real images, one paste step (CopyPaste._scp_src_to_dst + _copy_paste,
    DG/divergen/data/transforms/custom_copypaste.py:343-389, :428-506, 'basic' blend) in ONE dgx_self_copy_paste call.
    image uint8 (3,h1,w1), masks uint8 (n0,h1,w1), boxes f32 (n0,4), labels i64 (n0): the destination, GPU tensors.
    src_image uint8 (3,hs,ws), src_masks uint8 (ns,hs,ws), src_boxes f32 (ns,4), src_labels i64 (ns): the source, GPU tensors.
    sel: the m <= 99 source objects to paste, in paste order (host integers, each in [0, ns)).
    canvas_hw: (H, W) when the caller already holds it (the loader's workers do); None reads the selected boxes back.
    Returns dict(image, masks, boxes, labels) like copy_paste (no `source`): the surviving destination objects with the boxes of their
    updated masks, then the m selected source objects with their own boxes -- ONE compaction by out_valid.  m == 0: nothing is
    pasted, the inputs come back as they are (the reference keeps the destination's boxes then).
    lazy_masks: `masks` holds ALL n0 + m rows and `keep` (i64) the rows of the surviving objects, for BitMasks(masks, index=keep).
    merged: the source is the accumulator of self_copy_merge (dgx_self_copy_paste_merged: up to 99 objects per merged source)."""
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    m, ns = int(sel.shape[0]), int(src_masks.shape[0])
    entry, most = _SELF_COPY_ENTRY[bool(merged)]
    if m > most:
        raise ValueError("self_copy_paste: %d source objects selected, at most %d" % (m, most))
    if m and (int(sel.min()) < 0 or int(sel.max()) >= ns):
        raise ValueError("self_copy_paste: selected source index outside [0, %d): %s" % (ns, sel.tolist()))
    if m == 0:
        return _nothing_pasted(image, masks, boxes, labels, lazy_masks)
    sel_t = upload_i32(sel, image.device)
    sel_boxes = src_boxes.float().index_select(0, sel_t.long())
    sel_labels = src_labels.to(torch.int64).index_select(0, sel_t.long())
    return _self_copy_step(entry, image, masks, boxes, labels, src_image, src_masks, sel_t, sel_boxes, sel_labels, canvas_hw, lazy_masks)


def _self_copy_step(entry, image, masks, boxes, labels, src_image, src_masks, sel_t, sel_boxes, sel_labels, canvas_hw, lazy_masks):
    """The libdgx call of self_copy_paste (sel_t: the m selected planes, int32 on the device) and self_copy_paste_all (sel_t None: every
    plane of the source in order) and the ONE compaction after it.  sel_boxes / sel_labels: the m pasted objects' own, m > 0."""
    dev = image.device
    m, n0, ns = int(sel_boxes.shape[0]), int(masks.shape[0]), int(src_masks.shape[0])
    h1, w1 = int(image.shape[1]), int(image.shape[2])
    H, W = (int(v) for v in canvas_hw) if canvas_hw is not None else self_copy_canvas((h1, w1), sel_boxes)
    image, masks, boxes0 = image.contiguous(), masks.contiguous(), boxes.float().contiguous()
    src_image, src_masks = src_image.contiguous(), src_masks.contiguous()
    hs, ws = int(src_image.shape[1]), int(src_image.shape[2])
    if tuple(masks.shape[1:]) != (h1, w1) or tuple(src_masks.shape[1:]) != (hs, ws):
        raise ValueError("self_copy_paste: masks %s / %s do not match their images %s / %s" % (
            tuple(masks.shape), tuple(src_masks.shape), (h1, w1), (hs, ws)))
    out_image = torch.empty(3, H, W, dtype=torch.uint8, device=dev)
    out_masks = torch.empty(n0 + m, H, W, dtype=torch.uint8, device=dev)
    out_boxes = torch.empty(n0, 4, dtype=torch.float32, device=dev)
    out_valid = torch.empty(n0, dtype=torch.uint8, device=dev)
    work = torch.empty(((n0 * 5 + 3) & ~3) + H * ((W + 15) // 16) * 4, dtype=torch.int32, device=dev)
    chosen = () if sel_t is None else (L.ptr(sel_t), m)
    L.check(getattr(L.lib(), entry)(L.ptr(image), L.ptr(masks) if n0 else None, L.ptr(boxes0) if n0 else None, n0, h1, w1,
                                    L.ptr(src_image), L.ptr(src_masks), ns, hs, ws, *chosen, H, W,
                                    L.ptr(out_image), L.ptr(out_masks), L.ptr(out_boxes) if n0 else None,
                                    L.ptr(out_valid) if n0 else None, L.ptr(work), L.stream()), entry)
    keep = torch.cat([out_valid, torch.ones(m, dtype=torch.uint8, device=dev)]).nonzero().squeeze(1)      # ONE compaction
    all_boxes = torch.cat([out_boxes, sel_boxes])
    all_labels = torch.cat([labels.to(torch.int64), sel_labels])
    return _compacted(out_image, out_masks, keep, lazy_masks, boxes=all_boxes, labels=all_labels)


def self_copy_paste_all(image, masks, boxes, labels, src_image, src_masks, src_boxes, src_labels, canvas_hw=None, lazy_masks=False):
    """self_copy_paste with EVERY object of the source, in its order, in ONE dgx_self_copy_paste_all call: what the reference's
    CopyPaste(selected=False) pastes (INPUT.SCP_SRC_OBJ_SELECT False, INPUT.SCP_TYPE 'in_domain' / 'cas'; mapper.py:764-765,
    custom_copypaste.py:282-283).  No `sel` and no bound of 99: that bound is _select_object's draw, a source pasted whole brings all its
    ns objects.  Arguments and the returned dict as self_copy_paste; ns == 0: nothing is pasted, the inputs come back as they are."""
    ns = int(src_masks.shape[0])
    if int(src_boxes.shape[0]) != ns or int(src_labels.shape[0]) != ns:
        raise ValueError("self_copy_paste_all: %d source masks, %d boxes, %d labels" % (ns, int(src_boxes.shape[0]), int(src_labels.shape[0])))
    if ns == 0:
        return _nothing_pasted(image, masks, boxes, labels, lazy_masks)
    return _self_copy_step("dgx_self_copy_paste_all", image, masks, boxes, labels, src_image, src_masks, None, src_boxes.float(),
                           src_labels.to(torch.int64), canvas_hw, lazy_masks)


def remove_background(image, masks, out=None):
    """CopyPaste.remove_background (custom_copypaste.py:101-109; INPUT.RM_BG_PROB): image * any(masks, dim=0) in ONE
    dgx_remove_background call on the current stream.  image uint8 (3,h,w), masks uint8 / bool (n,h,w) (any non-zero byte counts as
    set; n == 0: an all-zero image) -- GPU tensors.  out: where the result goes, uint8 (3,h,w) contiguous; `out is image` works in
    place; None allocates.  Returns out."""
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[0] != 3:
        raise ValueError("remove_background: image must be uint8 (3, h, w), got %s %s" % (image.dtype, tuple(image.shape)))
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    if masks.dtype != torch.uint8 or masks.dim() != 3 or tuple(masks.shape[1:]) != tuple(image.shape[1:]):
        raise ValueError("remove_background: masks %s %s do not match the image %s" % (masks.dtype, tuple(masks.shape), tuple(image.shape)))
    if out is None:
        image = image.contiguous()
        out = torch.empty_like(image)
    elif out.dtype != torch.uint8 or tuple(out.shape) != tuple(image.shape) or out.device != image.device:
        raise ValueError("remove_background: out %s %s does not match the image %s" % (out.dtype, tuple(out.shape), tuple(image.shape)))
    n, h, w = int(masks.shape[0]), int(image.shape[1]), int(image.shape[2])
    masks = masks.contiguous()
    L.check(L.lib().dgx_remove_background(L.ptr(image), L.ptr(masks) if n else None, n, h, w, L.ptr(out), L.stream()), "dgx_remove_background")
    return out


def self_copy_merge(sources):
    """The temporary stages of Simple Copy-Paste from several source images (CopyPaste.__call__,
    DG/divergen/data/transforms/custom_copypaste.py:274-297: the first source is the accumulator, every further one is pasted onto it
    on a canvas taken from the boxes alone) in ONE dgx_self_copy_merge call: all S - 1 stages on the current stream, no host round trip.
    sources: 2 <= S <= 4 tuples (image uint8 (3,h_i,w_i), masks uint8 (m_i,h_i,w_i), boxes f32 (m_i,4), labels i64 (m_i)) of GPU
    tensors: the SELECTED objects of each source image in paste order, 1 <= m_i <= 99 (a source without one is left out by the caller,
    as the reference skips it).
    Returns dict(image (3,Hb,Wb), masks (M,Hb,Wb), boxes (M,4), labels (M), valid uint8 (M)) on the device, M = sum m_i, (Hb, Wb) the
    largest source size: the accumulator is the rows with valid == 1, in order; nothing is read back here."""
    S = len(sources)
    if not 2 <= S <= SELF_COPY_MAX_SRC:
        raise ValueError("self_copy_merge: %d sources, 2 to %d are built" % (S, SELF_COPY_MAX_SRC))
    dev = sources[0][0].device
    images = [s[0].contiguous() for s in sources]
    masks = [s[1].contiguous() for s in sources]
    counts = np.array([int(mk.shape[0]) for mk in masks], dtype=np.int32)
    sizes = np.array([[int(im.shape[1]), int(im.shape[2])] for im in images], dtype=np.int32)
    for i, (im, mk, s) in enumerate(zip(images, masks, sources)):
        if not 1 <= counts[i] <= SELF_COPY_MAX:
            raise ValueError("self_copy_merge: source %d brings %d objects, 1 to %d are built" % (i, counts[i], SELF_COPY_MAX))
        if tuple(mk.shape[1:]) != tuple(im.shape[1:]) or int(s[2].shape[0]) != counts[i] or int(s[3].shape[0]) != counts[i]:
            raise ValueError("self_copy_merge: source %d: masks %s / boxes %s / labels %s do not match its image %s" % (
                i, tuple(mk.shape), tuple(s[2].shape), tuple(s[3].shape), tuple(im.shape)))
    M, Hb, Wb = int(counts.sum()), int(sizes[:, 0].max()), int(sizes[:, 1].max())
    boxes = torch.cat([s[2].float().reshape(-1, 4) for s in sources]).contiguous()
    labels = torch.cat([s[3].to(torch.int64) for s in sources])
    ptrs = lambda ts: (L.c_p * S)(*[L.ptr(t) for t in ts])      # noqa: E731
    out_image = torch.empty(3, Hb, Wb, dtype=torch.uint8, device=dev)
    out_masks = torch.empty(M, Hb, Wb, dtype=torch.uint8, device=dev)
    out_boxes = torch.empty(M, 4, dtype=torch.float32, device=dev)
    out_valid = torch.empty(M, dtype=torch.uint8, device=dev)
    work = torch.empty(int(L.lib().dgx_self_copy_merge_workspace_words(S, M, Hb, Wb)), dtype=torch.int32, device=dev)
    L.check(L.lib().dgx_self_copy_merge(ptrs(images), ptrs(masks), counts.ctypes.data, sizes.ctypes.data, S, L.ptr(boxes), Hb, Wb,
                                        L.ptr(out_image), L.ptr(out_masks), L.ptr(out_boxes), L.ptr(out_valid), L.ptr(work), L.stream()),
            "dgx_self_copy_merge")
    return dict(image=out_image, masks=out_masks, boxes=out_boxes, labels=labels, valid=out_valid)


def self_copy_paste_multi(image, masks, boxes, labels, sources, lazy_masks=False):
    """Simple Copy-Paste from several source images onto the destination (image, masks, boxes, labels: as self_copy_paste takes them):
    self_copy_merge, ONE read-back of the M validity bytes and boxes (the sync copy_paste's `keep` costs as well), then self_copy_paste
    with the accumulated planes as the source and the survivors as `sel`, on the canvas self_copy_canvas gives for their boxes.
    sources: as self_copy_merge takes them, but any number >= 0 after the empty ones are dropped here: one source left is
    self_copy_paste itself, none is its m == 0 case.  Returns self_copy_paste's dict."""
    sources = [s for s in sources if int(s[1].shape[0])]
    if len(sources) < 2:
        if not sources:
            return self_copy_paste(image, masks, boxes, labels, image, masks[:0], boxes[:0], labels[:0], [], lazy_masks=lazy_masks)
        s_img, s_masks, s_boxes, s_labels = sources[0]
        return self_copy_paste(image, masks, boxes, labels, s_img, s_masks, s_boxes, s_labels, np.arange(int(s_masks.shape[0])),
                               lazy_masks=lazy_masks)
    acc = self_copy_merge(sources)
    host = torch.cat([acc["boxes"], acc["valid"].float().unsqueeze(1)], dim=1).cpu().numpy()      # the one read-back
    sel = np.flatnonzero(host[:, 4])
    canvas = self_copy_canvas(image.shape[-2:], host[sel, :4])
    return self_copy_paste(image, masks, boxes, labels, acc["image"], acc["masks"], acc["boxes"], acc["labels"], sel, canvas_hw=canvas,
                           lazy_masks=lazy_masks, merged=True)
