"""ZeroShotClassifier: Detic's open-vocabulary `cls_score` (MODEL.ROI_BOX_HEAD.USE_ZEROSHOT_CLS).  Mirrors
DG/divergen/modeling/roi_heads/zero_shot_classifier.py:9-87: a Linear into the embedding space, rows L2-normalised and scaled by
NORM_TEMP, multiplied with a fixed matrix of class text embeddings (one column per class + a zero background column), plus
an optional scalar bias.  State dict: linear.weight, linear.bias, zs_weight (D, C + 1) fp32 buffer, cls_bias (1,).

On the GPU: `linear` is the project's Linear, the normalisation dgx_l2norm_rows_fwd/bwd (layers/norm_ops.l2_normalize_rows), the
logits libdgx's MFMA GEMM against a bf16 (pad8(C + 1), D) image of zs_weight that is cached and rebuilt whenever zs_weight is
replaced or loaded.  The GEMM's bf16 result plus the fp32 scalar bias is returned as fp32."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from .. import ShapeSpec
from ...config import configurable
from ...layers.linear_ops import BF16, Linear, pad8
from ...layers.norm_ops import l2_normalize_rows


def build_zs_weight(embeddings, norm_weight=True):
    """(C, D) class embeddings (a .npy path or a tensor already transposed to (D, C), as reset_cls_test passes it) ->
    zs_weight (D, C + 1) fp32: transposed, a zero background column appended, columns L2-normalised when norm_weight
    (zero_shot_classifier.py:39-47, utils.py:39-59).  Host arithmetic, op for op the reference's: the result is bit-equal."""
    if isinstance(embeddings, str):
        w = torch.tensor(np.load(embeddings), dtype=torch.float32).permute(1, 0).contiguous()      # D x C
    else:
        w = embeddings
    w = torch.cat([w, w.new_zeros((w.shape[0], 1))], dim=1)                                         # D x (C + 1)
    if norm_weight:
        w = F.normalize(w, p=2, dim=0)
    return w


def _pad_rows(w16):
    """bf16 (N, D) -> (pad8(N), D) with zero rows, and its (D, pad8(N)) transpose: the two GEMM operands of the logits."""
    n = w16.shape[0]
    if n % 8:
        w16 = torch.cat([w16, w16.new_zeros(pad8(n) - n, w16.shape[1])], 0)
    w16 = w16.contiguous()
    return w16, w16.t().contiguous()


class _ZeroShotLogits(torch.autograd.Function):
    """fp32 (R, n) = bf16(x wimg^T)[:, :n] + cls_bias.  x bf16 (R, D); wimg bf16 (pad8(n), D), wimg_t its transpose: constants
    (zs_weight is a buffer).  Backward: dx through the own GEMM on the transposed image, d cls_bias = the sum of all logit
    gradients (the reference adds the scalar to every column, background included)."""

    @staticmethod
    def forward(ctx, x, wimg, wimg_t, cls_bias, n):
        from ...layers.gemm_ops import gemm_nt
        y = gemm_nt(x.contiguous(), wimg)
        out = y[:, :n].float()
        if cls_bias is not None:
            out = out + cls_bias.detach().float()
        ctx.save_for_backward(wimg_t)
        ctx.n, ctx.has_bias = n, cls_bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        from ...layers.gemm_ops import gemm_nt
        wimg_t, = ctx.saved_tensors
        n, npad = ctx.n, wimg_t.shape[1]
        dx = gb = None
        if ctx.needs_input_grad[0]:
            g16 = g.to(BF16)
            if npad != n:
                g16 = torch.cat([g16, g16.new_zeros(g16.shape[0], npad - n)], 1)
            dx = gemm_nt(g16.contiguous(), wimg_t)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            gb = g.sum(dtype=torch.float32).reshape(1)
        return dx, None, None, gb, None


class _ZeroShotLogitsF32(torch.autograd.Function):
    """_ZeroShotLogits for the prepared operand pair of a sampled vocabulary (layers/dyn_vocab_ops.PreparedVocab): the forward keeps the
    fp32 accumulators (dgx_zs_logits_f32) instead of the GEMM's bf16 result -- n is a few dozen columns, and an image step's loss reads
    five selected rows, where the last bf16 bit of a logit shows; the backward is _ZeroShotLogits' (the bf16 GEMM on the transposed image)."""

    @staticmethod
    def forward(ctx, x, wimg, wimg_t, cls_bias, n):
        from ... import _lib as L
        x = x.contiguous()
        R, D = x.shape
        out = torch.empty(R, n, dtype=torch.float32, device=x.device)
        L.check(L.lib().dgx_zs_logits_f32(L.ptr(x), L.ptr(wimg), R, D, n, wimg.shape[0], L.ptr(out), n, L.stream()), "dgx_zs_logits_f32")
        if cls_bias is not None:
            out = out + cls_bias.detach().float()
        ctx.save_for_backward(wimg_t)
        ctx.n, ctx.has_bias = n, cls_bias is not None
        return out

    backward = staticmethod(_ZeroShotLogits.backward)


class ZeroShotClassifier(nn.Module):
    @configurable
    def __init__(self, input_shape, *, num_classes, zs_weight_path, zs_weight_dim=512, use_bias=0.0, norm_weight=True,
                 norm_temperature=50.0):
        super().__init__()
        if isinstance(input_shape, int):
            input_shape = ShapeSpec(channels=input_shape)
        input_size = input_shape.channels * (input_shape.width or 1) * (input_shape.height or 1)
        if zs_weight_path == "rand":
            raise NotImplementedError("MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH 'rand' (a trainable random embedding matrix) is not "
                                      "built: no Detic configuration uses it; give the .npy of class embeddings")
        if zs_weight_dim % 8 or not 8 <= zs_weight_dim <= 4096:
            raise NotImplementedError("MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_DIM %d: the row normalisation kernel takes multiples of 8 "
                                      "in 8 .. 4096" % zs_weight_dim)
        self.norm_weight, self.norm_temperature = norm_weight, norm_temperature
        self.use_bias = use_bias < 0
        if self.use_bias:
            self.cls_bias = nn.Parameter(torch.ones(1) * use_bias)
        self.linear = Linear(input_size, zs_weight_dim)
        self.register_buffer("zs_weight", build_zs_weight(zs_weight_path, norm_weight))
        assert self.zs_weight.shape == (zs_weight_dim, num_classes + 1), self.zs_weight.shape

    @classmethod
    def from_config(cls, cfg, input_shape):
        h = cfg.MODEL.ROI_BOX_HEAD
        return dict(input_shape=input_shape, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES, zs_weight_path=h.ZEROSHOT_WEIGHT_PATH,
                    zs_weight_dim=h.ZEROSHOT_WEIGHT_DIM, use_bias=h.USE_BIAS, norm_weight=h.NORM_WEIGHT,
                    norm_temperature=h.NORM_TEMP)

    def set_zs_weight(self, zs_weight):
        """Replace the vocabulary (reset_cls_test): the tensor itself is kept, so several predictors can share one."""
        del self.zs_weight
        self.register_buffer("zs_weight", zs_weight)

    def zs_image(self):
        """bf16 (pad8(C + 1), D) operand image of zs_weight and its transpose; rebuilt when the buffer is another tensor, sits on
        another device or was written in place (load_state_dict, .to())."""
        w = self.zs_weight
        key = (id(w), w.data_ptr(), w._version, w.device, tuple(w.shape))
        cached = self.__dict__.get("_zs_image")
        if cached is None or cached[0] != key:
            cached = self.__dict__["_zs_image"] = (key,) + _pad_rows(w.detach().t().to(BF16))
        return cached[1], cached[2]

    def forward(self, x, classifier=None):
        """x (R, in) -> logits (R, C + 1); with `classifier` (C', D), the per-call vocabulary of detic_fast_rcnn.py:445-446, its
        rows are normalised per call and the result is (R, C').  `classifier` may also be the prepared operand pair of such a
        vocabulary (layers/dyn_vocab_ops.PreparedVocab, built by dgx_zs_gather: already normalised, cast, padded and transposed).
        The composition of its two halves: `project` and `score`."""
        return self.score(self.project(x), classifier)

    def project(self, x):
        """The first half of forward: u = linear(x), (R, D).  A caption step hands these rows to the caption loss as well
        (layers/caption_ops.caption_loss), which normalises the one row per image it reads itself."""
        if not x.is_cuda:
            return F.linear(x, self.linear.weight, self.linear.bias)      # host logic tests: the reference's arithmetic in torch
        return self.linear(x)

    def score(self, h, classifier=None):
        """The second half of forward: the projected rows normalised and scaled by NORM_TEMP, scored against the vocabulary."""
        from ...layers.dyn_vocab_ops import PreparedVocab
        prepared = classifier if isinstance(classifier, PreparedVocab) else None
        if not h.is_cuda:
            if prepared is not None:
                raise RuntimeError("a prepared vocabulary (PreparedVocab) holds GPU operand images; CPU tensors take the raw `classifier` rows")       # host logic tests: the reference's arithmetic in torch
            if classifier is not None:
                zs = classifier.permute(1, 0).contiguous()
                zs = F.normalize(zs, p=2, dim=0) if self.norm_weight else zs
            else:
                zs = self.zs_weight
            if self.norm_weight:
                h = self.norm_temperature * F.normalize(h, p=2, dim=1)
            y = torch.mm(h, zs)
            return y + self.cls_bias if self.use_bias else y
        if self.norm_weight:
            h = l2_normalize_rows(h, self.norm_temperature)
        elif h.dtype != BF16:
            h = h.to(BF16)
        if prepared is not None:
            n, wimg, wimg_t = prepared.n1, prepared.W, prepared.Wt
            if wimg.shape[1] != h.shape[1]:
                raise ValueError("prepared vocabulary of width %d for embeddings of width %d" % (wimg.shape[1], h.shape[1]))
        elif classifier is not None:
            c = classifier.detach().float().contiguous()
            n = c.shape[0]
            wimg, wimg_t = _pad_rows(l2_normalize_rows(c, 1.0) if self.norm_weight else c.to(BF16))
        else:
            n = self.zs_weight.shape[1]
            wimg, wimg_t = self.zs_image()
        with torch.autocast("cuda", enabled=False):
            fn = _ZeroShotLogitsF32 if prepared is not None else _ZeroShotLogits
            return fn.apply(h, wimg, wimg_t, self.cls_bias if self.use_bias else None, n)
