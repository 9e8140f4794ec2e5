"""float64 restatements of the three fused loss kernels (csrc/detic_loss.hip, csrc/centernet_loss.hip, csrc/mask_loss.hip), written
from the contract in include/divergen_hip.h and the kernels' comments, the per-element a-priori error bounds the GPU tests hold the
kernels to (tests/test_gpu_loss_numerics.py), and the named inputs (`CASES`) both test files use.  Host only, plain torch / numpy; no
project kernel is called from here.  tests/test_host_loss_ref.py pins the restatements on the reference's goldens and on the project's
composed torch paths, shows that an fp32 CPU evaluation of the same formulas stays inside every bound, and that every listed mutant
of the restatement lands outside one.

Every restatement takes `dt` (float64 = the reference; float32 = "the same formulas in fp32", the host-side stand-in for a correct
kernel) and `mutant` (None, or the name of one deliberate error -- DETIC_MUTANTS / CENTERNET_MUTANTS).

Bounds (`bounds(ref, dtype)`), u = 2^-24.  They are derived from the kernels' expressions, never from their output:

  storage      fp32: u |ref|.  bf16: half the spacing of bf16 at ref, 2^(floor(log2 |ref|) - 8), which lies between 2^-9 |ref| (ref just
               below a power of two) and 2^-8 |ref| (ref just above one).  bf16 keeps 8 significant bits, so its unit roundoff is 2^-8:
               a flat 2^-9 |ref| is HALF of what round-to-nearest-even may legitimately commit (1 + 2^-8 + eps rounds to 1 + 2^-7, off
               by just under 2^-8) and a correctly rounding kernel -- and the fp32 CPU evaluation -- would fail it;
               test_host_loss_ref.py::test_bf16_storage_bound_is_the_half_ulp shows both facts.  Charged twice where a value is stored,
               re-read and stored again (the joint gradient buffer after dgx_detic_grad_scale, when compared with the reference's chain).
  evaluation   n_ops u (sum of the magnitudes of the terms that form the element), n_ops counted from the kernel's own expression and
               written next to each count.  Where a term goes through a function that amplifies an absolute error (log of 1 - p,
               a division by 1 - p) the error is carried through the derivative explicitly instead.  expf, logf, log1pf and powf
               count ULP_FN = 2 ulp each: ROCm's HIP math-function accuracy table is not installed with the ROCm tree the tests are
               built against, so the fallback figure is used.
  sums         (sum of the addends' own bounds) + chain u (sum of the addends' magnitudes), chain = the number of fp32 additions on
               the longest path of the kernel's reduction (per-thread stride, 6 wave-shuffle steps, 3 additions of the four-wave fold,
               then the fold kernel / tail kernel in the same way).
  exact        counts, the statistics built from them (counts divided in fp32: the same IEEE division), dsign, zero columns, rows of
               ignored RoIs and untouched sentinels have no bound.
  either way   a comparison that decides a branch on an fp32 value (sigmoid against the clamp ends for the clamp's gradient, the clamped
               sigmoid against ignore_high_fp) cannot be decided when the float64 value is closer to the threshold than the evaluation
               error of the sigmoid; such elements may come out on either side, and their bound additionally holds the size of the term
               that is switched.  A sigmoid that is clamped for certain is the clamp constant exactly, and is compared exactly.

`worst_ratio(got, ref, bound)`: max |got - ref| / bound (inf for a non-finite result; an element with bound 0 must be equal)."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
ULP_FN = 2                 # expf / logf / log1pf / powf, ulp (module docstring)
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
CASCADE_WEIGHTS = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))


def f32v(x):
    """the value a C float argument holds"""
    return float(np.float32(x))


def half_ulp_bf16(x):
    """half the spacing of bf16 (8 significant bits) at |x|: what one round-to-nearest-even may be off by"""
    x = x.double().abs()
    _, e = torch.frexp(x)                                  # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 9))


def storage(ref, dtype):
    return half_ulp_bf16(ref) if dtype == BF16 else U32 * ref.double().abs()


def round_t(x, dtype):
    """float64 -> the storage type -> float64"""
    return x.to(F32).to(dtype).double()


def worst_ratio(got, ref, bnd):
    """max over elements of |got - ref| / bound: <= 1 passes.  inf for a non-finite result; bound 0 demands equality."""
    got, ref, bnd = torch.as_tensor(got).double(), torch.as_tensor(ref).double(), torch.as_tensor(bnd).double()
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.expand_as(err).clamp_min(1e-300))
    return float(ratio.max())


# ============================================================================================ Detic box-head losses
DETIC_MUTANTS = ("background", "ignore_row", "norm_R", "weight_ge256", "target_shift", "src", "sign0", "argmax_larger")
JOINT_MUTANTS = ("pad_nonzero", "box_scale_on_logits")


def mutant_class(C):
    """the class index >= 256 whose weight the 'weight_ge256' mutant drops (None: the width has no such class)"""
    return C - 1 if C - 1 >= 256 else None


def box_targets(prop, gtb, weights, dt):
    """Box2Box deltas of gtb w.r.t. prop in the kernel's order of operations (detic_loss.hip: sw, sx, tw, tx, then the four targets)."""
    p, q = prop.to(dt), gtb.to(dt)
    wx, wy, ww, wh = (float(v) for v in weights)
    sw, sh = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    sx, sy = p[:, 0] + 0.5 * sw, p[:, 1] + 0.5 * sh
    tw, th = q[:, 2] - q[:, 0], q[:, 3] - q[:, 1]
    tx, ty = q[:, 0] + 0.5 * tw, q[:, 1] + 0.5 * th
    return torch.stack([wx * (tx - sx) / sw, wy * (ty - sy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)], 1)


def _div32(a, b):
    return float(np.float32(float(a)) / np.float32(float(b)))


def detic_ref64(logits, deltas, gt, class_w, prop, gtb, src, weights, dt=F64, mutant=None):
    """logits (R, C+1), deltas (R, 4): the values the kernel reads (bf16: already rounded).  Returns a dict: out16 (16; [15] is not
    written by the kernel and not compared), dlogits (R, C+1) unscaled, dsign (R, 4), part (R, 8) and, for bounds(), `aux`."""
    x = logits.to(dt)
    R, C1 = x.shape
    C = C1 - 1
    g = gt.long()
    row_on = g >= 0                                         # gt < 0: ignore row -- no loss, no gradient, not in the normaliser
    fg = row_on & (g < C)
    w = torch.ones(C, dtype=dt) if class_w is None else class_w.to(dt).clone()
    if mutant == "weight_ge256" and mutant_class(C) is not None:
        w[mutant_class(C)] = 1.0
    tc = g + 1 if mutant == "target_shift" else g
    t = torch.zeros(R, C, dtype=dt)
    hot = (tc >= 0) & (tc < C)
    t[torch.nonzero(hot)[:, 0], tc[hot]] = 1.0
    v = x[:, :C]
    m = torch.clamp(-v, min=0.0)
    ce = (1.0 - t) * v + m + torch.log(torch.exp(-m) + torch.exp(-v - m))          # BCE with logits, torch's stable form
    sig = 1.0 / (1.0 + torch.exp(-v))
    on = (torch.ones_like(row_on) if mutant == "ignore_row" else row_on).to(dt)[:, None]
    term = w * ce * on
    dl = torch.zeros(R, C1, dtype=dt)
    dl[:, :C] = w * (sig - t) * on                                                  # column C: no loss, zero gradient
    L = term.sum(1)
    if mutant == "background":
        vb, tb = x[:, C], (g == C).to(dt)
        L = L + (torch.clamp(vb, min=0.0) - vb * tb + torch.log1p(torch.exp(-vb.abs()))) * on[:, 0]
        dl[:, C] = (1.0 / (1.0 + torch.exp(-vb)) - tb) * on[:, 0]
    idx = torch.arange(C1)[None].expand(R, C1)
    ismax = x == x.max(1, keepdim=True).values
    if mutant == "argmax_larger":
        bi = torch.where(ismax, idx, torch.full_like(idx, -1)).max(1).values
    else:
        bi = torch.where(ismax, idx, torch.full_like(idx, C1)).min(1).values        # smallest index among equal maxima
    sel = fg.clone()
    if src is not None and mutant != "src":
        sel &= src.long() == 0
    tg = box_targets(prop, gtb, weights, dt)
    d = deltas.to(dt) - tg
    sg = torch.sign(d)                                                              # sign(0) = 0
    if mutant == "sign0":
        sg = torch.where(d == 0, torch.ones_like(sg), sg)
    sel_f = sel.to(dt)
    lb = d.abs().sum(1) * sel_f
    dsign = sg * sel_f[:, None]
    part = torch.stack([L, lb, sel_f, (row_on & (bi == g)).to(dt), ((bi == g) & fg).to(dt), ((bi == C) & fg).to(dt), fg.to(dt),
                        row_on.to(dt)], 1)
    out = torch.zeros(16, dtype=dt)
    out[:8] = part.sum(0)
    one = torch.ones((), dtype=dt)
    nrow = torch.maximum(out[7], one) if mutant != "norm_R" else torch.tensor(float(R), dtype=dt)
    den = torch.maximum(4.0 * out[2], one)
    nfg = torch.maximum(out[6], one)
    out[14], out[8], out[9], out[10] = 1.0 / nrow, out[0] / nrow, out[1] / den, 1.0 / den
    # the kernel's lines for out[11..13]: counts divided in fp32 (exact integers, one IEEE division) -- restated as such, so that
    # the statistics are compared exactly
    out[11], out[12], out[13] = _div32(out[3], nrow), _div32(out[4], nfg), _div32(out[5], nfg)
    res = {"kind": "detic", "out16": out, "dlogits": dl, "dsign": dsign, "part": part}
    if dt == F64 and mutant is None:
        u = U32
        wfull = w[None].expand(R, C)
        # one loss term  w ((1 - t) v + m + logf(expf(-m) + expf(-v - m))):  (1 - t) v, m and -v - m are exact; two expf (2 ulp each) and
        # their sum put <= 5 u (relative) on the log's argument = 5 u (absolute) on the log, logf itself 2 ulp, then + m, + (1 - t) v,
        # * w: 11 roundings at most, each relative to a partial result <= |(1 - t) v| + m + 1
        b_term = 11 * u * wfull * (((1.0 - t) * v).abs() + m + 1.0) * row_on.to(dt)[:, None]
        chain_r = math.ceil(C1 / 256) + 6 + 3                                       # strided loop, wave shuffle, four-wave fold
        b_L = b_term.sum(1) + chain_r * u * term.abs().sum(1)
        # gradient  w (1 / (1 + expf(-v)) - t):  expf 2 ulp, +, /, -, *: 6 roundings on terms of size w sig and w t
        b_dl = torch.zeros(R, C1, dtype=dt)
        b_dl[:, :C] = 6 * u * wfull * (sig + t) * row_on.to(dt)[:, None]
        # box targets.  x, y:  wx (tx - sx) / sw  with  tx = q0 + 0.5 tw:  tw, sw one rounding each, tx and sx one more, the difference,
        # the product, the quotient and  delta - target:  5 roundings on  wx / sw (0.5 (tw + sw) + |tx| + |sx|) + |target| + |delta|.
        # w, h:  ww logf(tw / sw):  3 roundings on the ratio = 3 u on the log, logf 2 ulp, the product and the difference:
        # 4 roundings on  ww + |target| + |delta|
        p, q, dd = prop.double(), gtb.double(), deltas.double()
        wts = [float(z) for z in weights]
        b_d = torch.zeros(R, 4, dtype=dt)
        for k in (0, 1):
            sw_, tw_ = p[:, 2 + k] - p[:, k], q[:, 2 + k] - q[:, k]
            sx_, tx_ = p[:, k] + 0.5 * sw_, q[:, k] + 0.5 * tw_
            b_d[:, k] = 5 * u * (wts[k] / sw_ * (0.5 * (tw_ + sw_) + tx_.abs() + sx_.abs()) + tg[:, k].abs() + dd[:, k].abs())
            b_d[:, 2 + k] = 4 * u * (wts[2 + k] + tg[:, 2 + k].abs() + dd[:, 2 + k].abs())
        b_lb = (b_d.sum(1) + 4 * u * d.abs().sum(1)) * sel_f                        # + the four additions of the row
        chain_f = math.ceil(R / 256) + 6 + 3                                        # fold kernel: strided loop, shuffle, four waves
        b0 = b_L.sum() + chain_f * u * L.abs().sum()
        b1 = b_lb.sum() + chain_f * u * lb.sum()
        res["aux"] = {"b_L": b_L, "b_lb": b_lb, "b_dl": b_dl, "b0": b0, "b1": b1, "nrow": nrow, "den": den,
                      "sign_safe": bool(((d == 0) | (d.abs() > 4 * b_d) | ~sel[:, None]).all())}
    return res


def detic_bounds(ref, dtype):
    a, out, u = ref["aux"], ref["out16"], U32
    b16 = torch.zeros(16, dtype=F64)                        # [2..7], [11..13]: exact
    b16[0], b16[1] = a["b0"], a["b1"]
    b16[8] = a["b0"] / a["nrow"] + 2 * u * out[8].abs()     # the division and the fp32 result
    b16[9] = a["b1"] / a["den"] + 2 * u * out[9].abs()
    b16[10], b16[14] = 2 * u * out[10].abs(), 2 * u * out[14].abs()
    bp = torch.zeros_like(ref["part"])
    bp[:, 0] = a["b_L"] + u * ref["part"][:, 0].abs()
    bp[:, 1] = a["b_lb"] + u * ref["part"][:, 1].abs()
    return {"out16": b16, "dlogits": a["b_dl"] + storage(ref["dlogits"], dtype), "dsign": torch.zeros_like(ref["dsign"]), "part": bp}


def detic_check(got, ref, dtype):
    """{output: worst ratio} of one detic result (dict out16, dlogits, dsign, part) against the reference: bounded outputs against
    bounds(), exact ones as 0 (equal) or inf.  Non-finite results give inf."""
    b = detic_bounds(ref, dtype)
    r = {k: worst_ratio(got[k], ref[k], b[k]) for k in ("dlogits", "dsign", "part")}
    r["out16"] = worst_ratio(got["out16"][:15], ref["out16"][:15], b["out16"][:15])
    return r


def joint_ld(C, product=False):
    """(ld, grad_cols) of the joint entry.  The product's buffer (layers/box_stage.py) is the output of one GEMM over the arena group
    cls_score | bbox_pred, whose row count solver.FlatArena rounds up to pad_to = 8 (layers/linear_ops.group_parameters):
    ld = grad_cols = 8 ceil((C + 1 + 4) / 8) -- 1208 for C = 1203, 48 for C = 40.  The other widths of the tests leave 8 columns
    behind grad_cols that the kernel must not touch."""
    gc = (C + 5 + 7) // 8 * 8
    return (gc, gc) if product else (gc + 8, gc)


def grad_scale_ref64(stored, rows, C, out16, g_cls, g_box, mutant=None):
    """dgx_detic_grad_scale on a buffer AS STORED (float64 of the storage type's values): columns [0, C + 1) times the fp32 product
    g_cls * out16[14], [C + 1, C + 5) times g_box * out16[10]; everything else untouched.  Returns the unrounded products: the kernel's
    result is round_T of them, one fp32 multiplication and one storage rounding away."""
    sc = float(np.float32(g_cls) * np.float32(float(out16[14])))
    sb = float(np.float32(g_box) * np.float32(float(out16[10])))
    res = stored.double().clone()
    res[:rows, :C + 1] *= sb if mutant == "box_scale_on_logits" else sc
    res[:rows, C + 1:C + 5] *= sb
    return res


def grad_scale_bound(expected, dtype):
    return storage(expected, dtype) + U32 * expected.abs()          # the multiplication, then the storage rounding


def detic_joint_ref64(ref, grad_cols, dtype, g_cls=1.0, g_box=1.0, mutant=None):
    """The (R, grad_cols) gradient buffer the strided entry writes: logit gradients | the four signs | zeros; and the buffer after
    dgx_detic_grad_scale, formed from the buffer as stored (round_T first).  Returns (buf, bound of buf, scaled, bound of scaled)."""
    dl, ds = ref["dlogits"], ref["dsign"]
    R, C1 = dl.shape
    buf = torch.zeros(R, grad_cols, dtype=F64)
    buf[:, :C1], buf[:, C1:C1 + 4] = dl, ds
    if mutant == "pad_nonzero" and grad_cols > C1 + 4:
        buf[R // 2, C1 + 4] = 1.0
    bb = torch.zeros_like(buf)
    bb[:, :C1] = detic_bounds(ref, dtype)["dlogits"]
    scaled = grad_scale_ref64(round_t(buf, dtype), R, C1 - 1, ref["out16"], g_cls, g_box, mutant)
    return buf, bb, scaled, grad_scale_bound(scaled, dtype)


# ---------------------------------------------------------------------------------------------- detic inputs
def _last_wave_col(C):
    """the largest class column whose thread (column % 256) sits in the last wave (192..255); C - 1 when the row has none"""
    for c in range(C - 1, -1, -1):
        if c % 256 >= 192:
            return c
    return C - 1


def detic_case(R, C1, variant, kind="mixed"):
    """fp32 master inputs of one case (cast logits / deltas to the type under test: `detic_cast`).  variant picks the class weights
    (None / 0-1 mask / fractional), src (None / mixed) and the cascade's box weights; kind: mixed, all_ignore, all_background."""
    C = C1 - 1
    g = torch.Generator().manual_seed(1000003 * R + 101 * C1 + variant)
    logits = torch.randn(R, C1, generator=g) * 2.0 - 2.0
    u = torch.rand(R, generator=g)
    gt = torch.randint(0, C, (R,), generator=g)
    gt[u < 0.4] = C
    gt[u < 0.15] = -1
    hi_cls = C - 2 if C - 2 >= 256 else C - 2                     # a foreground class above index 256 where the width has one
    fixed = {0: 5 if C > 5 else 0, 1: hi_cls, 2: C, 3: -1}
    if R == 1:
        fixed = {0: hi_cls}
    for r, c in fixed.items():
        if r < R:
            gt[r] = c
    xy = torch.rand(R, 2, generator=g) * 800.0
    wh = torch.rand(R, 2, generator=g) * 296.0 + 4.0
    prop = torch.cat([xy, xy + wh], 1)
    gxy = xy + torch.randn(R, 2, generator=g) * 0.1 * wh
    gwh = wh * torch.exp(torch.randn(R, 2, generator=g) * 0.2)
    gtb = torch.cat([gxy, gxy + gwh], 1)
    deltas = torch.randn(R, 4, generator=g)
    weights = CASCADE_WEIGHTS[variant % 3]
    if R >= 16:
        # hard logits.  row 4: +-30, +-80, 0 and -0.0 below and above column 256
        cols = [0, 1, 2, 6, 7, 8] + ([256, 257, 300, C - 1] if C > 300 else [C - 4, C - 3, C - 2, C - 1])
        logits[4, cols] = torch.tensor([30.0, -30.0, 80.0, -80.0, 0.0, -0.0, 30.0, -80.0, 80.0, -30.0])
        logits[5] = 0.5                                             # all equal: argmax 0
        gt[5] = 0
        far = 700 if C > 700 else C - 1
        logits[6, [3, far]] = 9.0                                   # tie between column 3 and a far class column
        gt[6] = 3
        logits[7, [10, C]] = 9.0                                    # tie between a class column and the background column
        gt[7] = 10
        lw = _last_wave_col(C)
        logits[8, lw] = 9.0                                         # the maximum only in the last wave's share of the row
        gt[8] = lw
        # row 9: target x = wx (36 - 32) / 32 exactly (every step exact in fp32 and float64) and the delta equal to it: sign 0
        prop[9], gtb[9] = torch.tensor([16.0, 32.0, 48.0, 96.0]), torch.tensor([20.0, 40.0, 52.0, 104.0])
        deltas[9, 0] = weights[0] * 4.0 / 32.0
        gt[9] = 7
        prop[10], gtb[10] = torch.tensor([300.0, 200.0, 301.0, 201.0]), torch.tensor([300.2, 199.7, 301.5, 201.1])     # 1-pixel proposal
        gt[10] = 11
    if kind == "all_ignore":
        gt[:] = -1
    elif kind == "all_background":
        gt[:] = C
    cw = None
    if variant % 3 == 1:                                            # federated 0/1 mask, the gt class masked out on some rows
        cw = (torch.rand(C, generator=g) < 0.5).float()
        for r in range(0, R, 3):
            if 0 <= int(gt[r]) < C:
                cw[int(gt[r])] = 0.0
        if R > 1 and 0 <= int(gt[1]) < C:
            cw[int(gt[1])] = 1.0
    elif variant % 3 == 2:
        cw = 0.25 + 1.5 * torch.rand(C, generator=g)
    if cw is not None and mutant_class(C) is not None:
        cw[mutant_class(C)] = 0.0 if variant % 3 == 1 else 0.3125
    src = None
    if variant % 2 == 1:
        src = torch.randint(0, 2, (R,), generator=g)
        src[0] = 1                                                  # a foreground row the filter deselects
        if R > 1:
            src[1] = 0
    return {"logits": logits, "deltas": deltas, "gt": gt, "class_w": cw, "prop": prop, "gtb": gtb, "src": src, "weights": weights}


def detic_cast(case, dtype):
    """the case with logits and deltas as the kernel reads them (rounded to dtype)"""
    c = dict(case)
    c["logits"], c["deltas"] = case["logits"].to(dtype), case["deltas"].to(dtype)
    return c


def detic_args(c):
    return (c["logits"], c["deltas"], c["gt"], c["class_w"], c["prop"], c["gtb"], c["src"], c["weights"])


_DETIC_SHAPES = [(64, 255), (64, 256), (64, 257), (64, 512), (64, 513), (1, 1204), (37, 1204), (300, 1204), (37, 41)]
DETIC_CASES = {"R%d_W%d" % (R, C1): (lambda R=R, C1=C1, i=i: detic_case(R, C1, 1 if C1 == 41 else i)) for i, (R, C1) in enumerate(_DETIC_SHAPES)}
DETIC_CASES["all_ignore_R37_W300"] = lambda: detic_case(37, 300, 2, "all_ignore")
DETIC_CASES["all_background_R37_W300"] = lambda: detic_case(37, 300, 1, "all_background")
PRODUCT_WIDTHS = (1204, 41)            # joint buffers laid out as the product's (ld = grad_cols = pad8(C + 5))


# ============================================================================================ CenterNet proposal losses
CENTERNET_MUTANTS = ("tie_one_side", "clamp_grad_outside", "uncared_counted", "dup_once", "ihf_le", "hm_channel0", "gamma_as_2")


def _giou(p, t, one_side=False):
    pl, pt, pr, pb = p.unbind(1)
    tl, tt, tr, tb = t.unbind(1)
    if one_side:
        mn, mx = (lambda a, b: torch.where(a <= b, a, b)), (lambda a, b: torch.where(a >= b, a, b))
    else:
        mn, mx = torch.minimum, torch.maximum                   # ties: the gradient is split evenly
    ta, pa = (tl + tr) * (tt + tb), (pl + pr) * (pt + pb)
    wi, hi = mn(pl, tl) + mn(pr, tr), mn(pb, tb) + mn(pt, tt)
    ac = (mx(pl, tl) + mx(pr, tr)) * (mx(pb, tb) + mx(pt, tt))
    ai = wi * hi
    au = ta + pa - ai
    return 1.0 - ((ai + 1.0) / (au + 1.0) - (ac - au) / ac)


def _cn_consts(cfg):
    c = f32v(cfg["clamp"])
    hi = float(np.float32(1.0) - np.float32(cfg["clamp"]))       # the kernel's 1.0f - c
    return c, hi, f32v(cfg["ignore_high_fp"]), f32v(cfg["gamma"]), f32v(cfg["beta"]), f32v(cfg["pos_mul"]), f32v(cfg["neg_mul"])


def centernet_ref64(reg_pred, reg_tgt, hms, logit, pos_idx, cared, cfg, dt=F64, mutant=None):
    """cfg: not_norm_reg, beta, gamma, clamp, ignore_high_fp, pos_mul, neg_mul.  Returns out (5): sum of regression weights, weighted
    GIoU sum, neg loss, pos loss, #cared positives; g_reg (M, 4), g_neg (M), g_pos (M): autograd of the elementwise formulation."""
    c, hi, thr, gamma, beta, pos_mul, neg_mul = _cn_consts(cfg)
    M = logit.numel()
    rp, lg = reg_pred.to(dt).clone().requires_grad_(True), logit.to(dt).clone().requires_grad_(True)
    hm, tg = hms.to(dt).reshape(M, -1), reg_tgt.to(dt)
    w = hm[:, 0] if mutant == "hm_channel0" else hm.max(1).values
    mask = tg.max(1).values >= 0                                 # rows without a regression target carry -1e8
    wt = (torch.ones_like(w) if cfg["not_norm_reg"] else w) * mask.to(dt)
    one = torch.ones_like(tg)
    loss = _giou(torch.where(mask[:, None], rp, one), torch.where(mask[:, None], tg, one), mutant == "tie_one_side")
    s_w, s_loc = wt.sum(), (loss * wt).sum()
    sg = torch.sigmoid(lg)
    pred = torch.clamp(sg, min=c, max=hi)                        # the gradient passes on the closed interval
    if mutant == "clamp_grad_outside":
        pred = sg + (pred - sg).detach()
    pw = (lambda x, e: x * x if e == 2.0 else x) if mutant == "gamma_as_2" else (lambda x, e: torch.pow(x, e))
    g_exp = 2.0 if mutant == "gamma_as_2" else gamma
    neg = torch.log(1.0 - pred) * pw(pred, g_exp) * torch.pow(1.0 - w, beta)
    if thr > 0:
        neg = neg * ((pred <= thr) if mutant == "ihf_le" else (pred < thr)).to(dt).detach()       # the kernel drops !(p < thr)
    s_neg = -neg.sum() * neg_mul
    idx = pos_idx.long() if pos_idx is not None else torch.zeros(0, dtype=torch.long)
    car = torch.ones(idx.numel(), dtype=torch.bool) if (cared is None or mutant == "uncared_counted") else cared.bool()
    if mutant == "dup_once":
        idx, car = torch.unique(idx[car]), torch.ones(int(torch.unique(idx[car]).numel()), dtype=torch.bool)
    q = pred[idx]
    s_pos = -(torch.log(q) * pw(1.0 - q, g_exp) * car.to(dt)).sum() * pos_mul           # duplicates in pos_idx add up
    g_reg = torch.autograd.grad(s_loc, rp, retain_graph=True)[0]
    g_neg = torch.autograd.grad(s_neg, lg, retain_graph=True)[0]
    g_pos = torch.autograd.grad(s_pos, lg, allow_unused=True)[0] if idx.numel() else None
    g_pos = torch.zeros(M, dtype=dt) if g_pos is None else g_pos
    out = torch.stack([s_w, s_loc, s_neg, s_pos, car.sum().to(dt)]).detach()
    res = {"kind": "centernet", "out": out, "g_reg": g_reg.detach(), "g_neg": g_neg.detach(), "g_pos": g_pos.detach()}
    if dt == F64 and mutant is None:
        res["aux"] = _centernet_aux(reg_pred, reg_tgt, hms, logit, idx, car, cfg)
    return res


def _centernet_aux(reg_pred, reg_tgt, hms, logit, idx, car, cfg):
    """the bound of every output, first order in u, along the kernel's expressions (cn_loss_rows_kernel / cn_loss_tail_kernel)"""
    c, hi, thr, gamma, beta, pos_mul, neg_mul = _cn_consts(cfg)
    u, F = U32, ULP_FN
    M = logit.numel()
    p, t, hm, x = reg_pred.double(), reg_tgt.double(), hms.double().reshape(M, -1), logit.double()
    w = hm.max(1).values
    mask = t.max(1).values >= 0
    wt = (torch.ones_like(w) if cfg["not_norm_reg"] else w) * mask.double()
    p = torch.where(mask[:, None], p, torch.ones_like(p))
    t = torch.where(mask[:, None], t, torch.ones_like(t))
    # ---- GIoU.  All extents are >= 0, so A, Bh, ta, pa, wi, hi, gw, gh, ac, ai are sums and products of non-negative numbers: <= 3 u
    # relative each.  au = ta + pa - ai >= max(ta, pa) >= ai: <= 11 u relative; au + 1: 12 u; I = (ai + 1) / (au + 1): 17 u;
    # G = (ac - au) / ac: (3 u ac + 11 u au) / ac + 5 u G <= 19 u; loss = 1 - (I - G) adds 2: 40 roundings on 1 + I + G, one more for * wt
    pl, pt, pr, pb = p.unbind(1)
    tl, tt, tr, tb = t.unbind(1)
    A, Bh = pl + pr, pt + pb
    ta, pa = (tl + tr) * (tt + tb), A * Bh
    wi, hi_ = torch.minimum(pl, tl) + torch.minimum(pr, tr), torch.minimum(pb, tb) + torch.minimum(pt, tt)
    gw, gh = torch.maximum(pl, tl) + torch.maximum(pr, tr), torch.maximum(pb, tb) + torch.maximum(pt, tt)
    ac, ai = gw * gh, wi * hi_
    au = ta + pa - ai
    I, G = (ai + 1.0) / (au + 1.0), (ac - au) / ac
    loc = (1.0 - (I - G)) * wt
    b_loc = 41 * u * (1.0 + I + G.abs()) * wt
    # gradient  (-dI + dG) wt,  dI = (dai (au + 1) - (ai + 1) dau) iu^2,  dG = -(dau ac - au dac) iac^2,  dau = dpa - dai:
    # dai = m * extent 4 u, dpa 1 u, dac 3 u, dau 6 u (dpa + dai); numerator of dI: 18 u magI, iu^2: 28 u -> 46 u magI iu^2;
    # numerator of dG: 16 u magG, iac^2: 9 u -> 25 u magG iac^2; the sum and * wt: 2 more on each
    iu2, iac2 = 1.0 / (au + 1.0) ** 2, 1.0 / ac ** 2

    def side(a, b):
        return torch.where(a < b, torch.ones_like(a), torch.where(a == b, torch.full_like(a, 0.5), torch.zeros_like(a)))

    b_reg = torch.zeros(M, 4, dtype=F64)
    for k, (m_, e_in, dpa, e_out) in enumerate(((side(pl, tl), hi_, Bh, gh), (side(pt, tt), wi, A, gw), (side(pr, tr), hi_, Bh, gh),
                                                (side(pb, tb), wi, A, gw))):
        dai, dac = m_ * e_in, (1.0 - m_) * e_out
        magI = dai * (au + 1.0) + (ai + 1.0) * (dpa + dai)
        magG = (dpa + dai) * ac + au * dac
        b_reg[:, k] = u * wt * (48 * magI * iu2 + 27 * magG * iac2)
    # ---- focal terms.  sg = 1 / (1 + expf(-x)): F + 2 roundings, relative
    sg = torch.sigmoid(x)
    e_sg = (F + 2) * u * sg
    pr_ = torch.clamp(sg, c, hi)
    e_pr = e_sg
    sure_clamped = (sg < c - 2 * e_sg) | (sg > hi + 2 * e_sg)           # then pr_ is the clamp constant exactly
    amb_clamp = ((sg - c).abs() <= 2 * e_sg) | ((sg - hi).abs() <= 2 * e_sg)
    om = 1.0 - pr_
    e_om = e_pr + u * om
    dp_pass = sg * (1.0 - sg)
    inside = (sg >= c) & (sg <= hi)
    rel_dp = (F + 2) * u + (e_sg + u * (1.0 - sg)) / (1.0 - sg) + u

    def focal(prob, e_prob, other, e_other, mul, extra):
        """-mul log(prob) other^gamma * extra and its derivative factor w.r.t. prob... the kernel's  l * pow(other, gamma) * extra  and
        dt = pow(other, gamma) / prob * sgn - gamma pow(other, gamma - 1) l  share this form for the positive (prob = q, other = 1 - q)
        and the negative (prob = 1 - p, other = p; the sign of d/dp flips) term."""
        l = torch.log(prob)
        e_l = e_prob / prob + F * u * l.abs()                            # the argument's error through 1 / prob, logf 2 ulp
        r_o = e_other / other
        og, og1 = other ** gamma, other ** (gamma - 1.0)
        rel_og, rel_og1 = gamma * r_o + F * u, (gamma - 1.0) * r_o + F * u          # powf: gamma x the argument's relative error + 2 ulp
        val = -l * og * extra * mul
        e_val = mul * extra * og * e_l + val.abs() * (rel_og + 3 * u)
        T1 = og / prob
        e_T1 = T1 * (rel_og + e_prob / prob + u)
        T2 = gamma * og1 * l
        e_T2 = gamma * og1 * e_l + T2.abs() * (rel_og1 + 2 * u)
        d = (T1 - T2) * extra                                            # |d val / d prob| / mul
        e_d = (e_T1 + e_T2 + u * (T1 + T2.abs())) * extra + d.abs() * 2 * u
        return val, e_val, d, e_d

    nw = (1.0 - w) ** beta
    rel_nw = (beta + F) * u                                              # 1 - w: one rounding, powf: beta x that + 2 ulp
    keep = (pr_ < thr) if thr > 0 else torch.ones_like(pr_, dtype=torch.bool)
    amb_ihf = ((pr_ - thr).abs() <= 2 * e_pr) & ~sure_clamped if thr > 0 else torch.zeros_like(keep)
    n_val, e_nval, n_d, e_nd = focal(om, e_om, pr_, e_pr, neg_mul, nw)
    e_nval = e_nval + n_val.abs() * rel_nw
    e_nd = e_nd + n_d.abs() * rel_nw
    g_pass = neg_mul * n_d * dp_pass                                    # |d neg / d logit| where everything passes
    e_gneg = neg_mul * dp_pass * e_nd + g_pass * (rel_dp + 2 * u)
    neg_add = n_val * keep
    b_neg = torch.where(keep | amb_ihf, e_nval, torch.zeros_like(e_nval)) + torch.where(amb_ihf, n_val.abs(), torch.zeros_like(n_val))
    live = keep & inside
    b_gneg = torch.where(live, e_gneg + U32 * g_pass, torch.zeros_like(g_pass)) + torch.where(amb_ihf | amb_clamp, g_pass + e_gneg, torch.zeros_like(g_pass))
    # positives
    ii = idx[car]
    b_gpos, pos_add, b_pos = torch.zeros(M, dtype=F64), torch.zeros(0, dtype=F64), torch.zeros(0, dtype=F64)
    if ii.numel():
        q, e_q = pr_[ii], e_pr[ii]
        omq = 1.0 - q
        p_val, e_pval, p_d, e_pd = focal(q, e_q, omq, e_q + u * omq, pos_mul, torch.ones_like(q))
        gp = pos_mul * p_d * dp_pass[ii]
        e_gp = pos_mul * dp_pass[ii] * e_pd + gp * (rel_dp[ii] + 2 * u)
        b_j = torch.where(inside[ii], e_gp, torch.zeros_like(gp)) + torch.where(amb_clamp[ii], gp + e_gp, torch.zeros_like(gp))
        g_j = torch.where(inside[ii] | amb_clamp[ii], gp, torch.zeros_like(gp))
        cnt = torch.zeros(M, dtype=F64).index_add_(0, ii, torch.ones_like(gp))
        mag = torch.zeros(M, dtype=F64).index_add_(0, ii, g_j)
        b_gpos = torch.zeros(M, dtype=F64).index_add_(0, ii, b_j) + (cnt + 1) * u * mag       # atomicAdd chain + the fp32 result
        pos_add, b_pos = p_val, e_pval
    blocks = (M + 255) // 256
    chain_rows = 6 + 4 + math.ceil(blocks / 256) + 6 + 4               # block_sum, the tail's strided loop (double), block_sum
    chain_pos = math.ceil(max(int(idx.numel()), 1) / 256) + 6 + 4

    def total(addends, b_add, chain):
        return float(b_add.sum() + chain * u * addends.abs().sum())
    b_out = torch.tensor([total(wt, torch.zeros_like(wt), chain_rows), total(loc, b_loc, chain_rows), total(neg_add, b_neg, chain_rows),
                          total(pos_add, b_pos, chain_pos), 0.0], dtype=F64)
    return {"out": b_out, "g_reg": b_reg, "g_neg": b_gneg, "g_pos": b_gpos}


def centernet_bounds(ref, dtype=F32):
    a = ref["aux"]
    return {"out": a["out"], "g_reg": a["g_reg"] + U32 * ref["g_reg"].abs(), "g_neg": a["g_neg"], "g_pos": a["g_pos"]}


def centernet_check(got, ref):
    b = centernet_bounds(ref)
    return {k: worst_ratio(got[k], ref[k], b[k]) for k in ("out", "g_reg", "g_neg", "g_pos")}


def logit_of(p):
    return math.log(p / (1.0 - p))


def centernet_case(M, P, C, gamma, beta, nnr, ihf, cared_kind, clamp=1e-4, seed=0):
    """reg_pred / reg_tgt / hms / logit / pos_idx / cared + cfg.  M >= 255: the placed rows of the module's tests (ROWS)."""
    g = torch.Generator().manual_seed(7001 * M + 131 * P + 17 * C + seed)
    reg_t = torch.rand(M, 4, generator=g) * 40.0
    if M > 1:
        reg_t[torch.rand(M, generator=g) < 0.7] = -1e8               # 70 % rows without a target
    reg_p = torch.rand(M, 4, generator=g) * 40.0
    hm = torch.rand(M, C, generator=g) ** 3
    logit = torch.randn(M, generator=g) * 4.0 - 2.0
    c32 = np.float32(clamp)
    x_hi = np.float32(logit_of(float(c32)) * -1.0)                    # log((1 - c) / c), nearest fp32
    placed = {}
    if M >= 255:
        base = torch.tensor([5.0, 7.0, 3.0, 2.0])
        for r, sides in enumerate(([0], [1], [2], [3], [0, 1, 2, 3])):   # rows 0..3: a tie on one side (l, t, r, b); row 4: on all four
            reg_t[r] = base
            reg_p[r] = base + torch.tensor([1.5, -1.0, 0.75, 2.0])
            reg_p[r, sides] = base[sides]
        reg_t[5], reg_p[5] = base * 2.0, base * 0.5                   # prediction inside target
        reg_t[6], reg_p[6] = base * 0.5, base * 2.0                   # target inside prediction
        reg_t[7], reg_p[7] = base * 1e-3, base.flip(0) * 1e-3         # extents of 1e-3
        reg_t[8], reg_p[8] = base * 1e3, base.flip(0) * 1e3           # and of 1e3
        hm[9], hm[10] = 0.0, 1.0                                      # heat map exactly 0 / exactly 1
        lo, up = np.nextafter(x_hi, np.float32(0)), np.nextafter(x_hi, np.float32(100))
        thr64 = float(np.float32(ihf)) if ihf > 0 else 0.85
        # upper clamp end: sigmoid(x) <= 1 - c passes the gradient.  x_hi_below: the fp32 logit next below log((1 - c) / c) (sigmoid inside the
        # interval in exact arithmetic), x_hi_above: next above (outside); likewise -x at the lower end, where below -x_hi is outside.  Within
        # one ulp of the logit the fp32 sigmoid cannot tell the sides apart (either-way elements); * (1 +- 2^-10) can
        placed = {"x_hi_below": float(lo), "x_hi": float(x_hi), "x_hi_above": float(up), "x_lo_above": -float(lo), "x_lo": -float(x_hi),
                  "x_lo_below": -float(up), "x_hi_in": float(x_hi) * (1 - 2.0 ** -10), "x_hi_out": float(x_hi) * (1 + 2.0 ** -10),
                  "x_lo_in": -float(x_hi) * (1 - 2.0 ** -10), "x_lo_out": -float(x_hi) * (1 + 2.0 ** -10), "p20": 20.0, "m20": -20.0,
                  # the clamped sigmoid next to ignore_high_fp: 2^-20 relative on either side, the closest the fp32 sigmoid decides
                  "ihf_below": logit_of(thr64 * (1 - 2.0 ** -20)), "ihf_above": logit_of(thr64 * (1 + 2.0 ** -20)),
                  "ihf_nearest": logit_of(thr64)}
        for i, v in enumerate(placed.values()):
            logit[16 + i] = float(np.float32(v))
    idx = torch.randint(0, M, (P,), generator=g)
    if P >= 37 and M >= 255:
        idx[:len(placed)] = torch.arange(16, 16 + len(placed))       # positives on the placed logits too
        idx[len(placed)] = 9
        idx[len(placed) + 1] = idx[len(placed) + 2] = 3               # an ordinary duplicate
    if P >= 300:
        idx[100:150] = 12 if M >= 255 else 0                          # one location 50 times
    cared = {"none": None, "all": torch.ones(P, dtype=torch.bool), "mixed": torch.rand(P, generator=g) < 0.8}[cared_kind]
    if cared_kind == "mixed" and P > 2:
        cared[0], cared[1] = True, False
    cfg = {"not_norm_reg": int(nnr), "beta": float(beta), "gamma": float(gamma), "clamp": float(c32), "ignore_high_fp": float(ihf),
           "pos_mul": 0.25, "neg_mul": 0.75}
    return {"reg_pred": reg_p, "reg_tgt": reg_t, "hms": hm, "logit": logit, "pos_idx": idx, "cared": cared, "cfg": cfg, "placed": placed}


def centernet_args(c):
    return (c["reg_pred"], c["reg_tgt"], c["hms"], c["logit"], c["pos_idx"], c["cared"], c["cfg"])


CLAMP_AT_IHF = float(np.float32(1.0) - np.float32(0.85))            # 1.0f - c == 0.85f exactly: every clamped-high sigmoid EQUALS ignore_high_fp
_CN = [  # M, P, C, gamma, beta, not_norm_reg, ignore_high_fp, cared
    (1, 0, 1, 2.0, 4.0, 0, 0.0, "none"), (1, 1, 3, 1.5, 2.0, 1, 0.85, "all"), (1, 300, 1, 3.0, 4.0, 0, 0.85, "mixed"),
    (255, 37, 1, 2.0, 4.0, 1, 0.85, "mixed"), (256, 300, 3, 3.0, 4.0, 0, 0.0, "mixed"), (256, 0, 1, 1.5, 2.0, 1, 0.85, "none"),
    (257, 1, 1, 1.5, 4.0, 0, 0.85, "none"), (257, 300, 3, 2.0, 2.0, 1, 0.85, "all"), (5000, 37, 1, 2.0, 4.0, 0, 0.85, "mixed"),
    (5000, 300, 3, 1.5, 4.0, 1, 0.0, "mixed"), (5000, 300, 1, 3.0, 2.0, 0, 0.85, "none"), (5000, 0, 3, 2.0, 4.0, 1, 0.0, "none"),
    (255, 1, 3, 3.0, 2.0, 0, 0.0, "all"), (5000, 1, 1, 2.0, 2.0, 1, 0.85, "all")]
CENTERNET_CASES = {"M%d_P%d_C%d_g%g_b%g_nnr%d_ihf%g_%s" % s: (lambda s=s: centernet_case(*s)) for s in _CN}
CENTERNET_CASES["clamp_at_ihf_M256_P37"] = lambda: centernet_case(256, 37, 1, 2.0, 4.0, 1, 0.85, "all", clamp=CLAMP_AT_IHF)


# ============================================================================================ mask BCE
def mask_bce_ref64(x, gt, dt=F64):
    """x (R, inner): the logits the kernel reads; gt (R * inner) in {0, 1}.  out (5): mean loss, #incorrect, #false positive,
    #false negative, #positive; grad (R * inner) = (sigmoid(x) - t) / n."""
    v = x.to(dt).reshape(-1)
    n = v.numel()
    tb = gt.reshape(-1) != 0
    t = tb.to(dt)
    e = torch.clamp(v, min=0.0) - v * t + torch.log1p(torch.exp(-v.abs()))
    sig = 1.0 / (1.0 + torch.exp(-v))
    inv_n = torch.tensor(1.0, dtype=dt) / torch.tensor(float(n), dtype=dt)
    wrong = (v > 0) != tb
    out = torch.stack([e.sum() * inv_n, wrong.sum().to(dt), (wrong & ~tb).sum().to(dt), (wrong & tb).sum().to(dt), tb.sum().to(dt)])
    res = {"kind": "mask", "out": out, "grad": (sig - t) * inv_n}
    if dt == F64:
        u = U32
        # one term  fmaxf(x, 0) - x t + log1pf(expf(-|x|)):  expf 2 ulp -> 2 u e on the argument -> <= 2 u l on the log, log1pf 2 ulp,
        # one subtraction, one addition: 6 roundings on  max(x, 0) + |x t| + l
        b_e = 6 * u * (torch.clamp(v, min=0.0) + (v * t).abs() + torch.log1p(torch.exp(-v.abs())))
        blocks = min((n + 1023) // 1024, 1024)
        chain = math.ceil(n / (blocks * 256)) + 6 + 3 + blocks          # grid-stride loop, shuffle, four waves, the final kernel's serial sum
        b_loss = (b_e.sum() + chain * u * e.abs().sum()) * inv_n + 3 * u * out[0].abs()      # 1 / n, the product, the fp32 result
        # gradient  (1 / (1 + expf(-x)) - t) inv_n:  sigmoid 4, the difference, inv_n, the product: 7 roundings on (sig + t) / n
        res["aux"] = {"out": torch.tensor([float(b_loss), 0, 0, 0, 0], dtype=F64), "grad": 7 * u * (sig + t) * inv_n}
    return res


def mask_bounds(ref, dtype):
    return {"out": ref["aux"]["out"], "grad": ref["aux"]["grad"] + storage(ref["grad"], dtype)}


def mask_case(R=1400, S=28):
    """(R, 2, S, S) logits whose class-1 slice is the strided gather view; n = R S S = 1 097 600 > 1024 * 1024: the capped grid strides"""
    g = torch.Generator().manual_seed(77)
    full = torch.randn(R, 2, S, S, generator=g) * 4.0
    full[0, 1, 0, :6] = torch.tensor([60.0, -60.0, 0.0, -0.0, 30.0, -30.0])
    gt = torch.rand(R, S, S, generator=g) > 0.6
    return {"full": full, "gt": gt, "cls": 1}


MASK_CASES = {"R1400_S28_strided": mask_case}
CASES = {"detic": DETIC_CASES, "centernet": CENTERNET_CASES, "mask": MASK_CASES}


def bounds(ref, dtype=F32):
    """per-element bounds of every compared output of a reference result (detic_ref64 / centernet_ref64 / mask_bce_ref64)"""
    return {"detic": detic_bounds, "centernet": centernet_bounds, "mask": mask_bounds}[ref["kind"]](ref, dtype)
