"""float64 restatements of the norm and GELU kernels (csrc/layernorm.hip, csrc/groupnorm.hip, csrc/gelu.hip), written from the contract in
include/divergen_hip.h and the kernels' comments, the per-element a-priori bounds tests/test_gpu_norm_numerics.py holds the kernels
to, and the named inputs (LN_CASES, PM_CASES, GN_CASES, GELU_CASES) both test files use.  Host only, plain torch / numpy; no project
kernel is called from here.  tests/test_host_norm_ref.py pins the restatements on torch's own float64 layer_norm / group_norm / gelu and
their autograd, shows that an fp32 evaluation of the same formulas stays inside every bound and that every listed mutant lands outside
one.

Every restatement takes `dt` (float64 = the reference; float32 = "the same formulas in fp32", the host-side stand-in for a correct
kernel) and `mutant` (None or one name of LN_MUTANTS / GN_MUTANTS / GELU_MUTANTS).

Bounds, in the vocabulary of tests/_loss_ref64.py (u = U32 = 2^-24), derived from the kernels' expressions, never from their output:

  storage      fp32: u |v|;  bf16: half the spacing of bf16 at |v| -- taken at |ref| + (the evaluation bound), since the value that is
               rounded is the kernel's, which may lie in the next binade.
  evaluation   n_ops u (sum of the magnitudes of the terms), n_ops counted from the kernel's expression and written beside each count.
  sums         (the addends' own bounds) + chain u (sum of the addends' magnitudes); chain = the fp32 additions on the longest path,
               written beside each count (per-lane quads, 6 shuffle steps, the 8-wave LDS fold of ln_fold_part, nblk/64 + 7 + 7 of
               ln_param_reduce_kernel; 256- or 8-stride per thread, block_sum or gn_fold32, the 8-lane slab fold for GroupNorm).
  statistics   the error of mean and rstd is carried into y and dx through the derivative: d_mu rs |gamma| and |x^| (d_rs / rs) |gamma|
               for y, rs^2 d_mu (|a2| + |x^| |a1|) and (d_rs / rs) rs (|g - a1| + 3 |x^ a2|) for dx -- never as a flat factor.  The
               centred variance of LayerNorm sees the mean's error as + d_mu^2 exactly (sum (x - mu^)^2 = sum (x - mu)^2 + C d_mu^2).
  functions    rsqrtf and erff: ULP_FN ulp, the project's fallback figure (tests/_loss_ref64.py), one ulp = the fp32 spacing at the
               value (ulp32) or 2 u relative.  __expf(a): 2 + |a| ulp -- __expf(a) is v_exp_f32(a * log2 e): one ulp for v_exp_f32, and
               the product a * log2 e carries a relative rounding error u, i.e. an ABSOLUTE error u |a log2 e| in the exponent, which
               is a relative error 2^(u |a| log2 e) - 1 ~ u |a| in the result: |a| / 2 ulp for the product and as much again for the
               rounded constant log2 e, together 1 + |a| ulp, and one more for the result's own rounding.  A result below the normal
               range may be flushed to zero: its whole value is then allowed as error.
  cancel       GroupNorm's variance is E[d^2] - E[d]^2 with d = x - x0 (x0 the group's first element).  The summation error of both
               terms, chain u (E[d^2] + E[d]^2) in shape -- exactly u ((chain + 4) E[d^2] + 2 (chain + 2) |E d| E|d| + E[d]^2) -- does
               NOT shrink with the variance: it is the named component `cancel` of gn_stats_bounds, so that a test can ask how large it
               is (test_host_norm_ref.py::test_x0_cancellation_against_the_bf16_rounding).  GELU forms 1 + erff(x / sqrt 2), which
               cancels for x < -3: the named term u |0.5 x| (1 + |erf|).
  exact        zero rows of padding tokens and of the compact order's tail, sentinels, GroupNorm outputs whose ReLU gate is closed for
               certain, and GELU's signed zeros (compared by value) have bound 0.
  either way   a GroupNorm element whose float64 pre-activation x^ gamma + beta is closer to 0 than its evaluation error may pass the
               backward's gate either way; its bound, and the bound of every sum it enters, additionally holds the switched term.
               EITHER_WAY_CAP: at most ceil(numel / 10000) such elements per case (counted from the float64 reference alone).

`worst_ratio(got, ref, bound)` (tests/_loss_ref64.py): max |got - ref| / bound, inf for a non-finite result, bound 0 demands equality."""
import math

import numpy as np
import torch

from _gemm_ref64 import all_finite_bf16, gelu64, gelu_grad64, win_rows, window_rows
from _loss_ref64 import BF16, F32, F64, U32, ULP_FN, f32v, half_ulp_bf16, round_t, storage, worst_ratio  # noqa: F401

ULP = 2.0 * U32                     # one fp32 ulp relative to the value, at most
MIN_NORMAL32 = 2.0 ** -126
HALF_MIN_BF16 = 2.0 ** -134         # half the spacing of the bf16 subnormals (2^-133)
LN_MUTANTS = ("eps_dropped", "div_Cm1", "uncentred_var", "rstd_as_std", "dx_no_a2", "a1_no_gamma", "dgamma_dy_x", "pad_nonzero",
              "dres_twice", "dgamma_overwrite")
GN_MUTANTS = ("m_HW", "gate_x", "gate_ignored", "gate_no_beta")
GELU_MUTANTS = ("tanh", "bwd_no_xpdf", "bias_unrounded")


def either_way_cap(numel):
    return -(-numel // 10000)


def ulp32(x):
    """the spacing of fp32 at |x|"""
    x = x.double().abs()
    _, e = torch.frexp(x)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 24))


def stor(ref, e, dtype):
    """storage rounding of a value within e of ref"""
    a = ref.double().abs() + e
    if dtype == BF16:
        return half_ulp_bf16(a).clamp_min(HALF_MIN_BF16)
    return U32 * a


def as_read(x, dtype):
    """the fp32 master values as the kernel reads them from a buffer of `dtype`"""
    return x.to(dtype).to(F32)


# ============================================================================================ LayerNorm
def ln_layout(win, T):
    """token index per output row of dgx_layernorm_fwd (-1: a zero row).  win = (B, H, W, ws, shift) or None; ws > 0 classic window
    order, ws < 0 compact order: the T real rows first, then zero rows up to the classic row count."""
    if win is None or win[3] == 0:
        return torch.arange(T)
    tok, _ = window_rows(win)
    if win[3] < 0:
        total = win_rows((win[0], win[1], win[2], -win[3], win[4]))
        tok = torch.cat([tok, torch.full((total - T,), -1, dtype=torch.int64)])
    return tok


def ln_place(v, tok, mutant=None):
    """token-order rows v (T, C) in the order `tok`, zero rows where tok < 0"""
    out = torch.zeros(tok.numel(), v.shape[1], dtype=v.dtype)
    out[tok >= 0] = v[tok[tok >= 0]]
    if mutant == "pad_nonzero" and bool((tok < 0).any()):
        out[int(torch.nonzero(tok < 0)[0]), 0] = 1.0
    return out


def ln_fwd_ref64(x, gamma, beta, eps, win=None, dt=F64, mutant=None):
    """x (T, C) as read.  Returns mean, rstd (T), y (T, C) in token order and y_rows in the order of `win`."""
    v, g, b = x.to(dt), gamma.to(dt), beta.to(dt)
    C = v.shape[1]
    e = 0.0 if mutant == "eps_dropped" else f32v(eps)
    mu = v.sum(1, keepdim=True) / C
    d = v - mu
    q = (v * v).sum(1, keepdim=True) if mutant == "uncentred_var" else (d * d).sum(1, keepdim=True)
    var = q / (C - 1 if mutant == "div_Cm1" else C)
    rs = torch.sqrt(var + e) if mutant == "rstd_as_std" else 1.0 / torch.sqrt(var + e)
    y = d * rs * g + b
    return {"mean": mu[:, 0], "rstd": rs[:, 0], "y": y, "y_rows": ln_place(y, ln_layout(win, v.shape[0]), mutant)}


def ln_stat_err(x, eps):
    """(d_mu, d_rs / rs) of the forward kernels' statistics, per row, from the float64 values"""
    v, u = x.double(), U32
    C = v.shape[1]
    nj = -(-C // 256)
    # s: nj quads per lane, each (a + b) + (c + d) -> 2, added into s -> nj; 6 shuffle steps; the division
    chain = nj + 2 + 6
    mu = v.mean(1)
    dmu = (chain + 1) * u * v.abs().sum(1) / C
    var = ((v - mu[:, None]) ** 2).mean(1)
    # q: d = x - mu^ one rounding, twice in d * d, and the product: 3; the same chain; the division: 1.  The mean's error adds d_mu^2 exactly.
    n_var = 3 + chain + 1
    vh = var + dmu ** 2
    dvar = dmu ** 2 + n_var * u * vh + u * (vh + f32v(eps))                  # ... and the addition of eps
    drs = 0.5 * dvar / (var + f32v(eps)) + ULP_FN * ULP                      # d rs / rs = d(var + eps) / (2 (var + eps)); rsqrtf
    return dmu, drs


def ln_fwd_bounds(x, gamma, beta, eps, ref, ydtype, tok=None):
    v, g, b = x.double(), gamma.double(), beta.double()
    dmu, drs = ln_stat_err(x, eps)
    rs = ref["rstd"].double()
    t = ((v - ref["mean"].double()[:, None]) * rs[:, None] * g).abs()
    # y = (x - mu^) rs^ gamma + beta: the subtraction, two products, the addition: 4 roundings on |x^ gamma| + |beta|; the statistics
    # through the derivative (the mean's share with the kernel's own rstd: (1 + d_rs / rs))
    e = (dmu * rs * (1.0 + drs))[:, None] * g.abs() + t * drs[:, None] + 4 * U32 * (t + b.abs())
    by = e + stor(ref["y"], e, ydtype)
    out = {"mean": dmu, "rstd": drs * rs, "y": by}
    if tok is not None:
        out["y_rows"] = ln_place(by, tok)                                    # zero rows: bound 0
    return out


def ln_bwd_ref64(x, dy, mean, rstd, gamma, dres=None, dg0=None, db0=None, dt=F64, mutant=None):
    """x, dy (T, C) as read, dy in TOKEN order (the kernel gathers it from window order); mean, rstd (T) as read.  dx, and dgamma /
    dbeta on top of their initial values dg0 / db0 (the kernels accumulate)."""
    v, d, g = x.to(dt), dy.to(dt), gamma.to(dt)
    C = v.shape[1]
    mu, rs = mean.to(dt)[:, None], rstd.to(dt)[:, None]
    xh, gv = (v - mu) * rs, d * g
    a1 = (d if mutant == "a1_no_gamma" else gv).sum(1, keepdim=True) / C
    a2 = (gv * xh).sum(1, keepdim=True) / C
    dx = rs * (gv - a1 - (0.0 if mutant == "dx_no_a2" else xh * a2))
    if dres is not None:
        dx = dx + dres.to(dt) * (2.0 if mutant == "dres_twice" else 1.0)
    dgs, dbs = (d * (v if mutant == "dgamma_dy_x" else xh)).sum(0), d.sum(0)
    dg0 = torch.zeros(C, dtype=dt) if dg0 is None else dg0.to(dt)
    db0 = torch.zeros(C, dtype=dt) if db0 is None else db0.to(dt)
    return {"dx": dx, "dgamma": dgs + (0.0 if mutant == "dgamma_overwrite" else dg0), "dbeta": dbs + db0}


def ln_bwd_blocks(T):
    return min(max(-(-T // 8), 1), 512)                                      # dgx_layernorm_bwd_blocks


def ln_bwd_bounds(x, dy, mean, rstd, gamma, dres, dg0, db0, ref, xdtype, stat_err=None, waves=8):
    """stat_err = (d_mu, d_rs / rs) per row when mean / rstd are the KERNEL's (the product path) and the reference used its own."""
    v, d, g, u = x.double(), dy.double(), gamma.double(), U32
    T, C = v.shape
    nj = -(-C // 256)
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh, gv = (v - mu) * rs, d * g
    a1, a2 = gv.mean(1, keepdim=True), (gv * xh).mean(1, keepdim=True)
    # a1: gv one rounding; 4 nj sequential additions per lane, 6 shuffle steps, the division.  a2: gv x^ four roundings (x^ two, gv, the product)
    e_a1 = (1 + 4 * nj + 6 + 1) * u * gv.abs().mean(1, keepdim=True)
    e_a2 = (4 + 4 * nj + 6 + 1) * u * (gv * xh).abs().mean(1, keepdim=True)
    # dx = rs (gv - a1 - x^ a2): the x^ a2 term sees 5 roundings (x^ two, the product, the subtraction, rs), the others fewer
    core = rs * (gv - a1 - xh * a2)
    e = rs * (e_a1 + xh.abs() * e_a2) + 5 * u * rs * (gv.abs() + a1.abs() + (xh * a2).abs())
    if stat_err is not None:
        dmu, drs = (s.double()[:, None] for s in stat_err)
        e = e + rs * rs * dmu * (a2.abs() + xh.abs() * a1.abs()) + drs * rs * ((gv - a1).abs() + 3 * (xh * a2).abs())
    if dres is not None:
        e = e + u * (core.abs() + dres.double().abs())                       # the addition
    bdx = e + stor(ref["dx"], e, xdtype)
    # dgamma / dbeta: dy x^ three roundings.  chain: a wave's rows, the (waves - 1) additions of ln_fold_part, ln_param_reduce_kernel's
    # nblk / 64 rows per group + 7 + 7, and the addition into the gradient
    nblk = ln_bwd_blocks(T)
    chain = -(-T // (nblk * waves)) + (waves - 1) + -(-nblk // 64) + 7 + 7 + 1
    tg = (d * xh).abs()
    dg0 = torch.zeros(C, dtype=F64) if dg0 is None else dg0.double()
    db0 = torch.zeros(C, dtype=F64) if db0 is None else db0.double()
    bdg = 3 * u * tg.sum(0) + chain * u * (tg.sum(0) + dg0.abs())
    if stat_err is not None:
        bdg = bdg + (d.abs() * (rs * dmu + xh.abs() * drs)).sum(0)
    bdb = chain * u * (d.abs().sum(0) + db0.abs())
    return {"dx": bdx, "dgamma": bdg, "dbeta": bdb}


def _hard_rows(x, dy, gamma, xdtype):
    """the hard rows of the issue, among ordinary ones (T >= 7)"""
    C = x.shape[1]
    g = torch.Generator().manual_seed(C)
    x[1] = 1e4 + 1e-2 * torch.randn(C, generator=g)          # mean 1e4, spread 1e-2 (fp32 x; bf16 rounds it to a near-constant row)
    x[2] = 0.5                                               # constant: var = 0, rstd = 1 / sqrt(eps)
    x[3] = 1e-3
    x[3, C // 2] = 1e6                                       # one outlier
    x[4] = 0.0                                               # all zero
    dy[5] = 0.0
    gamma[1 % C] = 0.0
    gamma[2 % C] = -1.25
    gamma[C - 1] = -0.5


def ln_case(C, T, xdtype, eps=1e-5, win=None, hard=True, seed=0):
    """fp32 masters of one case: x, gamma, beta, dy (token order), dres, dg0, db0"""
    g = torch.Generator().manual_seed(100003 * C + 17 * T + seed)
    x = torch.randn(T, C, generator=g) * 2.0 + 0.5
    gamma, beta = 1.0 + 0.5 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(T, C, generator=g)
    if hard and T >= 7:
        _hard_rows(x, dy, gamma, xdtype)
    return {"x": x, "gamma": gamma, "beta": beta, "dy": dy, "dres": torch.randn(T, C, generator=g), "dg0": torch.randn(C, generator=g),
            "db0": torch.randn(C, generator=g), "eps": eps, "win": win, "C": C, "T": T, "xdtype": xdtype}


def _ln_cases():
    cases, ts = {}, (1, 7, 9, 37)
    for i, C in enumerate((4, 96, 192, 260, 384, 768, 1000, 1536, 1540, 3072)):
        for xd, nm in ((F32, "f32"), (BF16, "bf16")):
            T, eps = ts[(i + (xd == BF16)) % 4], (1e-5, 1e-6)[i % 2]
            cases["C%d_T%d_%s" % (C, T, nm)] = (lambda C=C, T=T, xd=xd, eps=eps: ln_case(C, T, xd, eps))
    cases["sweep_fwd_C96_T65549_f32"] = lambda: ln_case(96, 65536 + 13, F32, 1e-5)          # past the 8192 x 8 rows of one trip
    cases["sweep_bwd_C192_T16389_bf16"] = lambda: ln_case(192, 2 * 8192 + 5, BF16, 1e-5)     # past 512 workgroups x 8 waves x 2 rows
    for win in ((2, 10, 13, 7, 3), (1, 14, 25, 12, 6), (2, 17, 13, -7, 2)):
        T = win[0] * win[1] * win[2]
        cases["win_%d_%d_%d_ws%d_s%d_f32" % win] = (lambda win=win, T=T: ln_case(96, T, F32, 1e-5, win))
    return cases


LN_CASES = _ln_cases()
LN_BWD_MAX_C, LN_F32OUT_BWD_MAX_C = 1536, 768             # wider rows: forward only, the backward returns BAD_ARG
LN_SLOW_BWD = ("sweep_fwd_C96_T65549_f32",)                # the forward's sweep case; the backward has its own
LN_F32OUT_CASES = {k: v for k, v in LN_CASES.items() if k.split("_")[0] in ("C4", "C96", "C260", "C768", "C1000")}


def ln_inputs(c, dy_dtype=BF16):
    """the values the kernels read"""
    xd = c["xdtype"]
    return {"x": as_read(c["x"], xd), "dy": as_read(c["dy"], dy_dtype), "dres": as_read(c["dres"], xd)}


# ============================================================================================ patch merge + LayerNorm
PM_SHAPES = ((2, 7, 9, 48), (1, 5, 5, 96), (2, 6, 8, 192), (1, 3, 3, 384), (1, 4, 3, 768))      # NJ 2, 2, 3, 6, 12 (the 4-wave form)


def pm_index(B, H, W):
    """(T2, 4) pixel index b * H * W + y * W + x of the 2x2 neighbourhood [(2i, 2j) | (2i+1, 2j) | (2i, 2j+1) | (2i+1, 2j+1)] of every
    merged row, -1 in the zero padding of an odd H / W"""
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    b, i, j = torch.meshgrid(torch.arange(B), torch.arange(H2), torch.arange(W2), indexing="ij")
    idx = []
    for dy_, dx_ in ((0, 0), (1, 0), (0, 1), (1, 1)):
        y, x = 2 * i + dy_, 2 * j + dx_
        idx.append(torch.where((y < H) & (x < W), (b * H + y) * W + x, torch.full_like(y, -1)).reshape(-1))
    return torch.stack(idx, 1)


def pm_gather(x, B, H, W):
    """x (B * H * W, C0) -> merged rows (T2, 4 C0): the zero padding enters the statistics"""
    idx = pm_index(B, H, W)
    C0 = x.shape[1]
    src = torch.cat([x, torch.zeros(1, C0, dtype=x.dtype)])[idx]             # index -1 -> the zero row
    return src.reshape(idx.shape[0], 4 * C0)


def pm_scatter(dm, B, H, W):
    """merged-row gradients (T2, 4 C0) -> (B * H * W, C0): every real pixel once, the padding's share dropped"""
    idx = pm_index(B, H, W).reshape(-1)
    C0 = dm.shape[1] // 4
    out = torch.zeros(B * H * W, C0, dtype=dm.dtype)
    out[idx[idx >= 0]] = dm.reshape(-1, C0)[idx >= 0]
    return out


def pm_case(B, H, W, C0, xdtype, seed=0):
    g = torch.Generator().manual_seed(7919 * C0 + 31 * H + W + seed)
    T2, C = B * ((H + 1) // 2) * ((W + 1) // 2), 4 * C0
    c = {"x": torch.randn(B * H * W, C0, generator=g) * 2.0 + 0.5, "gamma": 1.0 + 0.5 * torch.randn(C, generator=g),
         "beta": 0.3 * torch.randn(C, generator=g), "dy": torch.randn(T2, C, generator=g), "dg0": torch.randn(C, generator=g),
         "db0": torch.randn(C, generator=g), "eps": 1e-5, "geom": (B, H, W, C0), "xdtype": xdtype}
    c["gamma"][1], c["gamma"][2] = 0.0, -1.25
    return c


PM_CASES = {"B%d_H%d_W%d_C%d_%s" % (s + (nm,)): (lambda s=s, xd=xd: pm_case(*s, xd)) for s in PM_SHAPES for xd, nm in ((F32, "f32"), (BF16, "bf16"))}


def pm_waves(C0):
    return 4 if -(-4 * C0 // 256) > 6 else 8


# ============================================================================================ GroupNorm
def gn_slabs(N, HW, G):
    """gn_slabs of csrc/groupnorm.hip"""
    if G == 32:
        return min(max(-(-HW // 128), 1), 64)
    S = min(-(-1024 // (N * G)), -(-HW // 256))
    return min(max(S, 1), 64)


def gn_chains(N, HW, G):
    """(pixels of one thread, additions of the workgroup fold, additions of the slab fold) of the reduction passes"""
    S = gn_slabs(N, HW, G)
    per = -(-HW // S)
    if G == 32:
        return -(-per // 8), 1 + 2, -(-S // 8) + 3          # 8-pixel stride; gn_fold32: one shuffle, (w0 + w1) + (w2 + w3); 8 lanes: s/8 + 3 shuffles
    return -(-per // 256), 6 + 3, -(-S // 8) + 3            # 256-pixel stride; block_sum: 6 shuffle steps + 3


def gn_fwd_ref64(x, gamma, beta, G, eps, relu, dt=F64, mutant=None):
    """x (N, HW, 8 G) as read.  The statistics in the kernel's shifted form (d = x - x0): in float64 equal to the plain ones, in fp32
    the kernel's own cancellation."""
    N, HW, C = x.shape
    v = x.to(dt).reshape(N, HW, G, 8)
    g, b = gamma.to(dt).reshape(G, 8), beta.to(dt).reshape(G, 8)
    x0 = v[:, :1, :, :1]
    d = v - x0
    m = float(HW if mutant == "m_HW" else 8 * HW)
    md = d.sum((1, 3), keepdim=True) / m
    var = torch.clamp((d * d).sum((1, 3), keepdim=True) / m - md * md, min=0.0)
    mu, rs = x0 + md, 1.0 / torch.sqrt(var + f32v(eps))
    pre = (v - mu) * rs * g + b
    y = torch.clamp(pre, min=0.0) if relu else pre
    return {"mean": mu.reshape(N, G), "rstd": rs.reshape(N, G), "y": y.reshape(N, HW, C), "pre": pre.reshape(N, HW, C)}


def gn_stats_bounds(x, G, eps):
    """per (n, g): d_mu, d_rs / rs, and `cancel`: the share of the rstd bound (absolute, on rstd) that comes from the summation error of
    E[d^2] - E[d]^2"""
    N, HW, C = x.shape
    u, e = U32, f32v(eps)
    v = x.double().reshape(N, HW, G, 8)
    d = v - v[:, :1, :, :1]
    m = 8.0 * HW
    npix, fold, sfold = gn_chains(N, HW, G)
    chain = 8 * npix + fold + sfold                          # 8 channels of every pixel of the thread, then the two folds
    Ed, Ead, Ed2 = d.sum((1, 3)) / m, d.abs().sum((1, 3)) / m, (d * d).sum((1, 3)) / m
    var = (Ed2 - Ed * Ed).clamp_min(0.0)
    e_md = (chain + 2) * u * Ead                             # d = x - x0 one rounding, the chain, the division
    # E[d^2]: d * d three roundings, the chain, the division: (chain + 4) u E[d^2];  md * md: 2 |md| e_md + u md^2
    cancel = u * ((chain + 4) * Ed2 + 2 * (chain + 2) * Ed.abs() * Ead + Ed * Ed)
    dvar = cancel + u * var + u * (var + e)                  # the subtraction, + eps
    r = dvar / (var + e)
    rs = 1.0 / torch.sqrt(var + e)
    cap = (1.0 / math.sqrt(e) / rs - 1.0).clamp_min(0.0)                      # fmaxf(var, 0): rstd never exceeds 1 / sqrt(eps)
    rel = lambda q: torch.minimum(torch.where(q < 1.0, 1.0 / torch.sqrt((1.0 - q).clamp_min(1e-300)) - 1.0, torch.full_like(q, float("inf"))), cap)
    drs = rel(r) + ULP_FN * ULP
    mu = v[:, 0, :, 0] + Ed
    dmu = e_md + u * mu.abs()
    return {"dmu": dmu, "drs": drs, "cancel": rel(cancel / (var + e)) * rs, "rstd": rs}


def gn_fwd_bounds(x, gamma, beta, G, eps, relu, ref):
    N, HW, C = x.shape
    sb = gn_stats_bounds(x, G, eps)
    v = x.double().reshape(N, HW, G, 8)
    g, b = gamma.double().reshape(G, 8), beta.double().reshape(G, 8)
    mu, rs = ref["mean"].double()[:, None, :, None], ref["rstd"].double()[:, None, :, None]
    dmu, drs = sb["dmu"][:, None, :, None], sb["drs"][:, None, :, None]
    t = ((v - mu) * rs * g).abs()
    e = dmu * rs * (1.0 + drs) * g.abs() + t * drs + 4 * U32 * (t + b.abs())        # as ln_fwd_bounds
    e = e.reshape(N, HW, C)
    by = e + stor(ref["y"], e, BF16)
    if relu:
        by = torch.where(ref["pre"].double() < -e, torch.zeros_like(by), by)       # closed for certain: exactly zero
    return {"mean": sb["dmu"], "rstd": sb["drs"] * sb["rstd"], "y": by}


def gn_bwd_ref64(x, dy, mean, rstd, gamma, beta, G, relu, dg0=None, db0=None, dt=F64, mutant=None):
    """one tensor.  The ReLU gate is the recomputed x^ gamma + beta > 0, as in the kernel.  Returns dx and the tensor's own parameter
    sums dgs / dbs; dgamma / dbeta = dg0 + dgs (gn_multi adds the tensors)."""
    N, HW, C = x.shape
    v, d = x.to(dt).reshape(N, HW, G, 8), dy.to(dt).reshape(N, HW, G, 8)
    g, b = gamma.to(dt).reshape(G, 8), beta.to(dt).reshape(G, 8)
    mu, rs = mean.to(dt)[:, None, :, None], rstd.to(dt)[:, None, :, None]
    xh = (v - mu) * rs
    if relu and mutant != "gate_ignored":
        gate = (v > 0) if mutant == "gate_x" else ((xh * g > 0) if mutant == "gate_no_beta" else (xh * g + b > 0))
        dh = torch.where(gate, d, torch.zeros_like(d))
    else:
        dh = d
    m = 8.0 * HW
    s1, s2 = (dh * g).sum((1, 3), keepdim=True), (dh * g * xh).sum((1, 3), keepdim=True)
    dx = rs * (dh * g - (s1 + xh * s2) / m)
    dgs, dbs = (dh * xh).sum((0, 1)).reshape(C), dh.sum((0, 1)).reshape(C)
    z = torch.zeros(C, dtype=dt)
    return {"dx": dx.reshape(N, HW, C), "dgs": dgs, "dbs": dbs, "dgamma": dgs + (z if dg0 is None else dg0.to(dt)),
            "dbeta": dbs + (z if db0 is None else db0.to(dt))}


def gn_bwd_terms(x, dy, mean, rstd, gamma, beta, G, relu, stat_err=None):
    """everything the backward's bounds need, from float64 alone: the per-element bound of dx, the bound and the magnitude of the
    tensor's dgamma / dbeta sums, and the number of either-way elements"""
    N, HW, C = x.shape
    u, m = U32, 8.0 * HW
    v, d = x.double().reshape(N, HW, G, 8), dy.double().reshape(N, HW, G, 8)
    g, b = gamma.double().reshape(G, 8), beta.double().reshape(G, 8)
    mu, rs = mean.double()[:, None, :, None], rstd.double()[:, None, :, None]
    xh = (v - mu) * rs
    t = (xh * g).abs()
    pre = xh * g + b
    e_pre = 3 * u * t + u * pre.abs()                         # x^ two roundings, * gamma, + beta
    if stat_err is not None:
        dmu, drs = (s.double()[:, None, :, None] for s in stat_err)
        e_pre = e_pre + dmu * rs * (1.0 + drs) * g.abs() + t * drs
    amb = (pre.abs() <= e_pre) & (e_pre > 0) if relu else torch.zeros_like(pre, dtype=torch.bool)
    open_ = (pre > 0) if relu else torch.ones_like(pre, dtype=torch.bool)
    dh = torch.where(open_, d, torch.zeros_like(d))
    sw = torch.where(amb, d.abs(), torch.zeros_like(d))      # the switched term of an either-way element
    npix, fold, sfold = gn_chains(N, HW, G)
    chain = 8 * npix + fold + sfold                          # s1 / s2 run over the 8 channels of every pixel of the thread
    gs = (1, 3)
    S1, S2 = (dh * g).sum(gs, keepdim=True), (dh * g * xh).sum(gs, keepdim=True)
    # s1: dh gamma one rounding + the chain; s2: x^ two, dh gamma, the product: four + the chain; + the switched terms
    e_s1 = (1 + chain) * u * (dh * g).abs().sum(gs, keepdim=True) + (sw * g.abs()).sum(gs, keepdim=True)
    e_s2 = (4 + chain) * u * (dh * g * xh).abs().sum(gs, keepdim=True) + (sw * t).sum(gs, keepdim=True)
    # dx = rs (dh gamma - (s1 + x^ s2) inv_m): the x^ s2 term sees 8 roundings (x^ two, the product, the sum, inv_m's own division and
    # the product with it, the subtraction, rs), dh gamma three
    e = rs * (3 * u * (dh * g).abs() + 8 * u * (S1.abs() + (xh * S2).abs()) / m + (e_s1 + xh.abs() * e_s2) / m + sw * g.abs())
    if stat_err is not None:
        a1, a2 = S1 / m, S2 / m
        e = e + rs * rs * dmu * (a2.abs() + xh.abs() * a1.abs()) + drs * rs * ((dh * g - a1).abs() + 3 * (xh * a2).abs())
    dxr = rs * (dh * g - (S1 + xh * S2) / m)
    bdx = e + stor(dxr, e, BF16)
    # dgamma / dbeta of this tensor up to its slab partials: dh x^ three roundings; the thread's pixels, the workgroup fold
    c1 = npix + fold
    tg = (dh * xh).abs()
    e_dg = (3 + c1) * u * tg.sum((0, 1)) + (sw * xh.abs()).sum((0, 1))
    e_db = c1 * u * dh.abs().sum((0, 1)) + sw.sum((0, 1))
    if stat_err is not None:
        e_dg = e_dg + (dh.abs() * (rs * dmu + xh.abs() * drs)).sum((0, 1))
    return {"dx": bdx.reshape(N, HW, C), "e_dg": e_dg.reshape(C), "e_db": e_db.reshape(C), "mag_dg": tg.sum((0, 1)).reshape(C),
            "mag_db": dh.abs().sum((0, 1)).reshape(C), "either_way": int(amb.sum()), "entries": N * gn_slabs(N, HW, G)}


def gn_param_bounds(terms, dg0, db0):
    """dgamma / dbeta over one or several tensors: gn_bwd_param(_multi)_kernel walks every (tensor, sample, slab) entry with 64 lanes,
    then 6 shuffle steps and the addition into the gradient"""
    chain = sum(-(-t["entries"] // 64) for t in terms) + 6 + 1
    bdg = sum(t["e_dg"] for t in terms) + chain * U32 * (sum(t["mag_dg"] for t in terms) + dg0.double().abs())
    bdb = sum(t["e_db"] for t in terms) + chain * U32 * (sum(t["mag_db"] for t in terms) + db0.double().abs())
    return {"dgamma": bdg, "dbeta": bdb}


GN_SHAPES = ((2, 35, 32), (1, 129, 32), (2, 16400, 32), (1, 35, 4), (3, 700, 8), (2, 300, 64), (1, 40, 40))
GN_MULTI_HW = (1600, 400, 100, 25, 9)
GN_X0_SIGMAS = (8.0, 32.0, 300.0)
GN_REFUSED_G = 257
X0_INSIDE = 0.97            # keeps the nominal 8-sigma outlier inside 8 sigma after the bf16 rounding of x0 and the group's own sampling of its mean


def gn_hard_groups(G):
    """{kind: group} of sample 0 (as many as the case has groups for)"""
    kinds = ("const", "x0_8", "x0_32", "x0_300", "mean200")
    return {k: i + 1 for i, k in enumerate(kinds) if i + 1 < G}


def gn_case(N, HW, G, seed=0, hard=True):
    """fp32 masters (x, dy are read as bf16)"""
    C = 8 * G
    g = torch.Generator().manual_seed(6007 * HW + 13 * G + N + seed)
    x = torch.randn(N, HW, C, generator=g) + 0.3
    gamma, beta = 1.0 + 0.5 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(N, HW, C, generator=g)
    if hard:
        hg = gn_hard_groups(G)
        for k, gi in hg.items():
            sl = slice(8 * gi, 8 * gi + 8)
            if k == "const":
                x[0, :, sl] = 0.75
            elif k.startswith("x0_"):
                x[0, 0, 8 * gi] = 0.3 + X0_INSIDE * float(k[3:])  # the group's FIRST element: an outlier of (just under) that many sigma
            else:
                x[0, :, sl] = 200.0 + 0.5 * torch.randn(HW, 8, generator=g)
        gamma[3], beta[3] = 0.0, -0.25                            # gamma = 0, beta < 0: the gate is closed for certain
        gamma[5] = -0.75
    return {"x": x, "gamma": gamma, "beta": beta, "dy": dy, "dg0": torch.randn(C, generator=g), "db0": torch.randn(C, generator=g),
            "eps": 1e-5, "N": N, "HW": HW, "G": G}


GN_CASES = {"N%d_HW%d_G%d" % s: (lambda s=s: gn_case(*s)) for s in GN_SHAPES}


def gn_multi_case():
    cs = [gn_case(2, hw, 32, seed=i, hard=(i == 1)) for i, hw in enumerate(GN_MULTI_HW)]
    for c in cs[1:]:
        for k in ("gamma", "beta", "dg0", "db0"):
            c[k] = cs[0][k]
    return cs


def gn_inputs(c):
    return as_read(c["x"], BF16), as_read(c["dy"], BF16)


# ============================================================================================ GELU
K_INV_SQRT2 = float(np.float32(0.70710678118654752440))
K_INV_SQRT2PI = float(np.float32(0.39894228040143267794))


def gelu_fwd_ref64(x, dt=F64, mutant=None):
    v = x.to(dt)
    if mutant == "tanh":
        return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    if dt == F64:
        return gelu64(v)                                          # 0.5 x erfc(-x / sqrt 2): no cancellation in the reference
    return 0.5 * v * (1.0 + torch.erf(v * K_INV_SQRT2))           # the kernel's form


def _erf_err(v):
    """absolute error of the kernel's 1 + erff(x * kInvSqrt2), and |erf|"""
    u = U32
    t = v / math.sqrt(2.0)
    erf = torch.erf(t)
    # the argument: the rounded constant and the product, 2 u relative, through erf' = 2 / sqrt(pi) exp(-t^2); erff itself ULP_FN ulp;
    # the addition of 1 (the cancelling step) u (1 + |erf|)
    return ULP_FN * ulp32(erf) + 2.0 / math.sqrt(math.pi) * torch.exp(-t * t) * 2 * u * t.abs() + u * (1.0 + erf.abs()), erf


def gelu_fwd_bounds(x, ref):
    v, u = x.double(), U32
    e_1perf, _ = _erf_err(v)
    e = (0.5 * v).abs() * e_1perf + u * ref.abs()                # 0.5 x is exact; the last product
    return e + stor(ref, e, BF16)


def gelu_bwd_ref64(x, dy, dt=F64, mutant=None):
    v, d = x.to(dt), dy.to(dt)
    if mutant == "bwd_no_xpdf":
        return d * (0.5 * torch.special.erfc(-v / math.sqrt(2.0)))
    if dt == F64:
        return d * gelu_grad64(v)
    return d * (0.5 * (1.0 + torch.erf(v * K_INV_SQRT2)) + v * (torch.exp(-0.5 * v * v) * K_INV_SQRT2PI))


def gelu_bwd_bounds(x, dy, ref):
    v, d, u = x.double(), dy.double(), U32
    e_1perf, _ = _erf_err(v)
    cdf = 0.5 * torch.special.erfc(-v / math.sqrt(2.0))
    a = -0.5 * v * v                                             # -0.5 x exact, one product: u relative on a -> u |a| relative on exp(a)
    ea = torch.exp(a)
    e_exp = ea * ((2.0 + a.abs()) * ULP + u * a.abs())           # __expf: 2 + |a| ulp (module docstring)
    e_exp = e_exp + torch.where(ea < MIN_NORMAL32, ea + 2.0 ** -149, torch.zeros_like(ea))        # a subnormal result may be flushed
    pdf = ea * K_INV_SQRT2PI
    e_pdf = K_INV_SQRT2PI * e_exp + 2 * u * pdf                  # the rounded constant, the product
    xp = (v * pdf).abs()
    # dy (cdf + x pdf): 0.5 (1 + erf) exact halving; x pdf one product; the sum; the product with dy
    e = d.abs() * (0.5 * e_1perf + v.abs() * e_pdf + u * xp + u * (cdf + xp)) + u * ref.abs()
    return e + stor(ref, e, BF16)


def gelu_slabs(M, N):
    panels = -(-N // 512)
    return max(min(-(-1024 // panels), 256, -(-M // 16)), 1)


def gelu_bias_ref64(dx_stored, bias0, beta, mutant_dx=None):
    """the bias gradient is DEFINED on the stored bf16 dx (csrc/gelu.hip): beta * bias0 + float64 column sums of the kernel's own dx output.
    mutant 'bias_unrounded': the sums of the unrounded dx (mutant_dx) instead."""
    s = (dx_stored if mutant_dx is None else mutant_dx).double().sum(0)
    return s if beta == 0.0 else f32v(beta) * bias0.double() + s


def gelu_bias_bounds(dx_stored, bias0, beta, ref):
    M, N = dx_stored.shape
    slabs = gelu_slabs(M, N)
    rows = -(-M // slabs)
    # a wave's rows of the slab (stride 4), the four waves: 3; gelu_colsum_final_kernel: slabs / 16 per row group, 15 to fold the groups;
    # beta * out + a: the product and the sum
    chain = -(-rows // 4) + 3 + -(-slabs // 16) + 15
    b = chain * U32 * dx_stored.double().abs().sum(0)
    if beta != 0.0:
        b = b + U32 * (f32v(beta) * bias0.double()).abs() + U32 * ref.abs()
    return b


GELU_DY_VALUES = (1.0, -1.0, 0.37, -0.37, 0.0, 300.0)
GELU_BETAS = (0.0, 1.0, 0.5)
GELU_SWEEP_N = 8 * (8192 * 256) + 8                              # one element group past the 8192-workgroup grid: the grid-stride path


def gelu_all_values_case():
    """every finite bf16 value as (48, 1360): the last 512-column panel is partial; dy from GELU_DY_VALUES"""
    x = all_finite_bf16().to(F32).reshape(48, 1360)
    g = torch.Generator().manual_seed(5)
    dy = torch.tensor(GELU_DY_VALUES)[torch.randint(0, len(GELU_DY_VALUES), (48, 1360), generator=g)]
    return {"x": x, "dy": dy}


def gelu_slab_case():
    """(4099, 520): 256 slabs of 17 rows, the last 14 of them empty"""
    g = torch.Generator().manual_seed(6)
    return {"x": torch.randn(4099, 520, generator=g) * 2.0, "dy": torch.randn(4099, 520, generator=g)}


GELU_CASES = {"all_bf16_M48_N1360": gelu_all_values_case, "slabs_M4099_N520": gelu_slab_case}
