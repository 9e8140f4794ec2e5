"""Dynamic classifier ops over libdgx (csrc/dyn_vocab.hip): the sampled per-batch vocabulary, the two GEMM operand images of its
classifier and the label remap.  CPU tensors (host logic tests) take torch's ops with the same contract."""
import torch

from .. import _lib as L
from .linear_ops import BF16, pad8

_PROB0 = {}


def sampling_weights(weight, C, device):
    """prob0 (C + 1,) fp32 on `device`: `weight` (the frequency weights of a box step; None = uniform, an image step) with a zero for
    the background (utils.py:18-22).  Cached: the weights do not change between steps."""
    key = (C, str(device), None if weight is None else (weight.data_ptr(), weight._version))
    p = _PROB0.get(key)
    if p is None:
        p = torch.ones(C + 1, dtype=torch.float32, device=device) if weight is None else \
            torch.cat([weight.detach().float().to(device)[:C], torch.zeros(1, dtype=torch.float32, device=device)])
        p[C:].zero_()
        if len(_PROB0) > 16:
            _PROB0.clear()
        p = _PROB0[key] = p.contiguous()
    return p


def inds_capacity(G, num_classes, S):
    return max(int(S), min(int(G), int(num_classes)), 1)


def sample_classes(labels, prob0, expo, C, num_classes, S):
    """_sample_cls_inds (DG custom_rcnn.py:226-247) for labels i64 (G,), prob0 / expo fp32 (C + 1,): -> inds i64 (capacity,),
    cls_id_map i64 (num_classes + 1,), n.  On the GPU n is an int32 tensor of one element (dgx_dyn_class_sample: nothing is read
    back); on the CPU it is an int."""
    G = int(labels.numel())
    dev = prob0.device
    cap = inds_capacity(G, num_classes, S)
    if not prob0.is_cuda:
        lab = labels[(labels >= 0) & (labels < C)]
        app = torch.unique(lab)
        a = int(app.numel())
        more = app.new_zeros(0)
        if a < S:
            q = prob0[:C].clone()
            q[app] = 0
            keys = torch.where(q > 0, q / expo[:C], torch.zeros_like(q))
            k = min(S - a, int((keys > 0).sum()))
            if k > 0:
                order = torch.sort(keys, descending=True, stable=True)[1]        # equal keys: the lower index first
                more = order[:k]
        sel = torch.cat([app, more])
        n = int(sel.numel())
        inds = torch.zeros(cap, dtype=torch.int64)
        inds[:n] = sel
        cls_id_map = torch.full((num_classes + 1,), n, dtype=torch.int64)
        cls_id_map[sel] = torch.arange(n)
        return inds, cls_id_map, n
    labels = labels.contiguous()
    inds = torch.empty(cap, dtype=torch.int64, device=dev)
    cls_id_map = torch.empty(num_classes + 1, dtype=torch.int64, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(L.lib().dgx_dyn_class_sample(L.ptr(labels) if G else None, G, L.ptr(prob0), L.ptr(expo), int(C), int(num_classes), int(S),
                                         L.ptr(inds), L.ptr(cls_id_map), L.ptr(n), L.stream()), "dgx_dyn_class_sample")
    return inds, cls_id_map, n


def zs_gather(zs, inds, n, D, C, normalize=True):
    """W bf16 (pad8(n + 1), D) and Wt bf16 (D, pad8(n + 1)): the columns inds[:n] of zs_weight (fp32 (D, C + 1)), re-normalised, + the zero background row (dgx_zs_gather)."""
    npad = pad8(n + 1)
    W = torch.empty(npad, D, dtype=BF16, device=zs.device)
    Wt = torch.empty(D, npad, dtype=BF16, device=zs.device)
    if zs.dtype != torch.float32:
        raise L.DgxError("zs_gather reads the fp32 zs_weight (got %s)" % zs.dtype)
    L.check(L.lib().dgx_zs_gather(L.ptr(zs), int(D), int(C), L.ptr(inds) if n else None, int(n), 1 if normalize else 0,
                                  L.ptr(W), L.ptr(Wt), L.stream()), "dgx_zs_gather")
    return W, Wt


def remap_labels(labels, cls_id_map, num_classes):
    """cls_id_map[labels] that keeps negative ("ignore") labels as they are (dgx_remap_labels)."""
    if not labels.is_cuda:
        ok = (labels >= 0) & (labels <= num_classes)
        return torch.where(ok, cls_id_map[labels.clamp(0, num_classes)], labels)
    labels = labels.contiguous()
    out = torch.empty_like(labels)
    L.check(L.lib().dgx_remap_labels(L.ptr(labels), labels.numel(), L.ptr(cls_id_map), int(num_classes), L.ptr(out), L.stream()),
            "dgx_remap_labels")
    return out


class PreparedVocab:
    """The operand pair of a per-call vocabulary as ZeroShotClassifier.forward takes it in place of a raw `classifier` tensor:
    W bf16 (pad8(n1), D), Wt its transpose, n1 = the number of logit columns (sampled classes + background)."""

    def __init__(self, W, Wt, n1):
        self.W, self.Wt, self.n1 = W, Wt, int(n1)


class DynamicVocab:
    """classifier_info[1] of a dynamic-classifier step: (inds, cls_id_map) of the reference plus the column count n, which the host
    learns late on a box step (it rides in the proposal sampler's device->host read) and from the label lists on an image step."""

    def __init__(self, inds, cls_id_map, n, num_classes):
        self.inds, self.cls_id_map, self.num_classes = inds, cls_id_map, int(num_classes)
        self.n_dev = n if torch.is_tensor(n) else None
        self.n = None if torch.is_tensor(n) else int(n)
        self._ops = None

    def __iter__(self):         # the reference's `inds, cls_id_map = classifier_info[1]`
        return iter((self.inds if self.n is None else self.inds[:self.n], self.cls_id_map))

    def resolve(self, n=None):
        """n from the sampler's read (box step); without one, a read of its own (paths that have no read to share)."""
        if self.n is None:
            self.n = int(n) if n is not None else int(self.n_dev.item())
        return self.n

    def remap(self, labels):
        return remap_labels(labels, self.cls_id_map, self.num_classes)

    def classifier(self, cls_score):
        """classifier_info[0] for `cls_score` (a ZeroShotClassifier): the prepared pair on the GPU; on the CPU the reference's raw
        (n + 1, D) rows zs_weight[:, inds + [-1]].permute(1, 0) (DG custom_rcnn.py:161-163)."""
        n = self.resolve()
        zs = cls_score.zs_weight
        if not zs.is_cuda:
            idx = torch.cat([self.inds[:n], self.inds.new_full((1,), zs.shape[1] - 1)])
            return zs[:, idx].permute(1, 0).contiguous()
        if self._ops is None:
            W, Wt = zs_gather(zs.detach(), self.inds, n, zs.shape[0], zs.shape[1] - 1, cls_score.norm_weight)
            self._ops = PreparedVocab(W, Wt, n + 1)
        return self._ops

