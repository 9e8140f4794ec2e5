"""Caption supervision ops over libdgx (csrc/caption_loss.hip): the caption rows of a step prepared once (dgx_caption_prepare), the
caption loss of one cascade stage on the PROJECTED box features (dgx_caption_loss) -- the n x N caption scores of the reference
(DG detic_fast_rcnn.py:452-458, :469-506) are never formed -- and the cross-rank caption batch of MODEL.SYNC_CAPTION_BATCH
(DG custom_rcnn.py:210-223).  Host array for the per-image row offsets, a validity byte per row: no device->host read."""
import ctypes

import torch

from .. import _lib as L
from ..config.image_labels import MAX_IMAGES_PER_GPU as MAX_IMAGES


def sync_caption_features(features, ann_type, BS, rank, ratio, gather, dim=512, device=None):
    """DG custom_rcnn.py:210-223 `_sync_caption_features` as a pure function.  features (B, D) fp32 or None (a step that drew no
    captions), `gather(rows)` -> the list of every rank's (rows_k, D + 1) tensor, this rank's included (all ranks take part on every
    step: a box step sends BS * ratio zero rows, an image step BS).  Returns the (sum rows_k, D + 1) matrix, the rank in its last
    column, or None when this rank drew no captions -- it still gathered.  The row counts are checked on the host before anything is
    launched on the result (this replaces the reference's rank-column assert)."""
    has = features is not None
    rows = int(BS) * int(ratio) if ann_type == "box" else int(BS)
    if has:
        if features.dim() != 2 or features.shape[0] != rows:
            raise ValueError("sync_caption_features: %s caption rows for a %r batch of %d" % (tuple(features.shape), ann_type, BS))
        dim, device = int(features.shape[1]), features.device
        features = features.float()
    else:
        features = torch.zeros(rows, int(dim), dtype=torch.float32, device=device)
    col = torch.full((rows, 1), float(rank), dtype=torch.float32, device=device)
    parts = gather(torch.cat([features, col], dim=1).contiguous())
    if not has:
        return None
    for k, p in enumerate(parts):
        if p.dim() != 2 or p.shape[1] != dim + 1 or p.shape[0] != rows:
            raise ValueError("MODEL.SYNC_CAPTION_BATCH: rank %d sent %s caption rows, this rank %s: every rank sends the same count "
                             "(MODEL.CAP_BATCH_RATIO x the box batch = every other source's batch)" % (k, tuple(p.shape), (rows, dim + 1)))
    return torch.cat([p.to(device) for p in parts], dim=0)


def all_gather_rows(rows):
    """The model's `gather`: torch.distributed.all_gather_into_tensor on the current stream; without a process group world size 1."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return [rows]
    W = dist.get_world_size()
    out = torch.empty(W * rows.shape[0], rows.shape[1], dtype=rows.dtype, device=rows.device)
    dist.all_gather_into_tensor(out, rows)
    return list(out.split(rows.shape[0], dim=0))


class PreparedCaptions:
    """The caption rows of one step as the loss kernel reads them: (N, D) fp32, L2-normalised when NORM_WEIGHT, the rank column of a
    synced batch cut off; target0 = the column of this rank's first caption; neg_weight = NEG_CAP_WEIGHT when synced, else 1."""

    def __init__(self, rows, n, dim, target0, neg_weight):
        self.rows, self.n, self.dim, self.target0, self.neg_weight = rows, int(n), int(dim), int(target0), float(neg_weight)


def prepare_captions(features, dim, norm_weight, synced=False, batch=None, rank=0, neg_cap_weight=1.0):
    """features (N, dim) fp32, or (N, dim + 1) with the rank column when `synced` -> PreparedCaptions (one launch per step; the three
    cascade stages share it).  batch = images of this rank's batch (the one-hot targets start at column batch * rank when synced)."""
    if not features.is_cuda:
        raise L.DgxError("libdgx ops need GPU (ROCm) tensors; got a %s tensor -- no CPU fallback exists" % features.device)
    f = features.detach().float().contiguous()
    N, ld = int(f.shape[0]), int(f.shape[1])
    if ld != dim + (1 if synced else 0):
        raise ValueError("caption features of width %d for embeddings of width %d%s" % (ld, dim, " + the rank column" if synced else ""))
    out = torch.empty(N, dim, dtype=torch.float32, device=f.device)
    L.check(L.lib().dgx_caption_prepare(L.ptr(f), ld, N, dim, 1 if norm_weight else 0, L.ptr(out), L.stream()), "dgx_caption_prepare")
    return PreparedCaptions(out, N, dim, (int(batch) * int(rank)) if synced else 0, neg_cap_weight if synced else 1.0)


class _CaptionLoss(torch.autograd.Function):
    """The caption part of image_loss of one cascade stage.  forward: chosen rows, loss and stats_l_caption, the logit gradients kept;
    backward: the whole gradient of u and d cls_bias from one launch, the upstream gradient read on the device."""

    @staticmethod
    def forward(ctx, u, cls_bias, valid, counts, cap, temp, norm_weight, scale, stat_scale):
        if u.dim() != 2 or u.stride(1) != 1 or u.stride(0) < u.shape[1] or (u.stride(0) * u.element_size()) % 16 or u.data_ptr() % 16:
            u = u.contiguous()
        R, D = int(u.shape[0]), cap.dim
        ld = int(u.stride(0)) if R > 1 else int(u.shape[1])
        B = len(counts)
        if B > MAX_IMAGES:
            raise L.DgxError("caption_loss: %d images in one batch (at most %d)" % (B, MAX_IMAGES))
        if sum(counts) > R or u.shape[1] < D:
            raise L.DgxError("caption_loss: u %s for %d proposal rows of width %d" % (tuple(u.shape), sum(counts), D))
        dev = u.device
        row0 = (ctypes.c_int * (B + 1))(*([0] + [sum(counts[:i + 1]) for i in range(B)]))
        lib = L.lib()
        out = torch.empty(4, dtype=torch.float32, device=dev)
        sel = torch.empty(B, dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(lib.dgx_caption_workspace_floats(B, cap.n)), 1), dtype=torch.float32, device=dev)
        bias = cls_bias.detach().float().contiguous() if cls_bias is not None else None
        head = (u.data_ptr(), ld, R, L.ptr(valid), B, row0, L.ptr(cap.rows), cap.n, D, cap.target0, float(temp), 1 if norm_weight else 0,
                L.ptr(bias), cap.neg_weight, float(scale), float(stat_scale))
        L.check(lib.dgx_caption_loss(*head, None, L.ptr(sel), L.ptr(out), L.ptr(ws), None, 0, None, L.dtype_code(u), L.stream()),
                "dgx_caption_loss")
        ctx.head, ctx.keep = head, (valid, cap, bias)      # the pointers in `head` stay alive with these
        ctx.save_for_backward(u, sel, ws)
        ctx.shape, ctx.has_bias = (R, int(u.shape[1])), cls_bias is not None
        ctx.mark_non_differentiable(out, sel)
        return out[0], out, sel

    @staticmethod
    def backward(ctx, g, _o, _s):
        u, sel, ws = ctx.saved_tensors
        R, W = ctx.shape
        ldg = -(-W // 8) * 8                             # 16-byte rows in either dtype
        du = torch.empty(R, ldg, dtype=u.dtype, device=u.device)
        db = torch.empty(1, dtype=torch.float32, device=u.device) if ctx.has_bias else None
        g = g.detach().float().reshape(1).contiguous()
        L.check(L.lib().dgx_caption_loss(*ctx.head, L.ptr(g), L.ptr(sel), None, L.ptr(ws), L.ptr(du), ldg, L.ptr(db), L.dtype_code(u),
                                         L.stream()), "dgx_caption_loss (gradient)")
        return (du[:, :W], db) + (None,) * 7


def caption_loss(u, cls_bias, valid, counts, cap, temp, norm_weight, scale, stat_scale):
    """u (R_alloc, >= D) f32 | bf16: cls_score.linear(x), rows of image b at [sum(counts[:b]), sum(counts[:b + 1])), rows past
    sum(counts) are padding; cls_bias the (1,) parameter or None; valid (R,) uint8 or None; cap a PreparedCaptions.
    Returns (loss, out4, sel): loss = scale * sum over images of the caption BCE of the image's last valid row, out4[1] =
    stat_scale * the same sum (stats_l_caption), sel the chosen row per image (-1 = none)."""
    if not u.is_cuda:
        raise L.DgxError("libdgx ops need GPU (ROCm) tensors; got a %s tensor -- no CPU fallback exists" % u.device)
    return _CaptionLoss.apply(u, cls_bias, valid, list(counts), cap, temp, norm_weight, scale, stat_scale)
