"""float64 restatements of the optimizer kernels (csrc/optim.hip: dgx_adamw_ema_step[_scaled], dgx_sgd_ema_step, dgx_clip_coef_f32),
written from the contract in include/divergen_hip.h and the kernels' comments, the per-element a-priori error bounds the GPU tests
hold the kernels to (tests/test_gpu_optim_numerics.py), the case builders both test files use, and the mutants.  Plain torch / numpy,
elementwise, device agnostic (the GPU test evaluates the same functions densely in float64 on the device and again on the CPU at
chosen indices); no project kernel is called from here.  tests/test_host_optim_ref.py pins the restatements on torch.optim and on
oracle/solver.py, shows that a float32 CPU evaluation of the kernel's operation sequence stays inside every bound on every case, and
that every listed mutant lands outside one.

Every restatement takes `dt` (float64 = the reference; float32 = "the kernel's operation sequence in fp32", the host-side stand-in
for a correct kernel: every operation is a separate torch call, so each is rounded once, as under -ffp-contract=off) and `mutant`.

Scalars (`adamw_scalars` / `sgd_scalars`) are the values the kernel receives and forms: lr, betas, eps, weight decay, clip value,
grad_scale and ema decay rounded to float32; grad_scale * *scale_dev, 1 - decay, 1 - b1, 1 - b2 formed in float32; bc1 = (float)(1 -
pow(b1, step)) and bc2s = (float)sqrt(1 - pow(b2, step)) formed in double and rounded, as the host code does; per element lre = lr *
lr_scale[segment] and 1 - lre * wd formed in float32.  The reference then computes with these values in float64.

Bounds, u = 2^-24 (first order; every bound carries the factor 1 + 2^-20, which covers the neglected products of two rounding errors:
no count below exceeds 16, and 16 u = 2^-20).  Each is k u (sum of the magnitudes of the terms of that output in the float64
recurrence) + k TINY, k counted from the kernel's own operation sequence and written next to the bound; where an error passes through
a division or a square root it is carried through the derivative explicitly (|sqrt(x + e) - sqrt(x)| <= min(|e| / sqrt(x), sqrt|e|)).
  TINY     2^-126, the smallest normal float32, per operation: what an operation may lose to underflow whether or not the device
           flushes subnormals (g = 1e-30: the square is subnormal or zero).
  sqrtf    HIP's math-function table gives sqrtf a maximum error of 1 ulp: 2 u relative.
  a / b    the float32 division operator is IEEE correctly rounded in HIP device code unless the build asks otherwise
           (-fhip-fp32-correctly-rounded-divide-sqrt is the default and csrc/build.py does not switch it off): u relative.
  domain   no float32 intermediate overflows: with clipping off |g * scale| < 1e18; with clipping on any gradient, +-inf included.
  exact    the bf16 shadow is the round-to-nearest-even of the kernel's OWN float32 p; an element whose lr multiplier is 0 keeps its
           p bit for bit; found_inf leaves every array as it was; sentinels stay.  NaN rule: a NaN gradient element gives NaN in m, v,
           p and the shadow (buf and p for SGD) -- where the reference is NaN the result must be NaN, elsewhere it must be finite.

`worst_ratio(got, ref, bound)`: max |got - ref| / bound (inf for a non-finite result where the reference is finite, or a finite one
where it is NaN; an element with bound 0 must be equal)."""
import math
import types

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
SECOND = 1.0 + 2.0 ** -20
ULP_SQRT = 2.0             # sqrtf: 1 ulp (HIP math table) = 2 u relative
ULP_DIV = 1.0              # operator /: correctly rounded = u relative
F32, BF16, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
CLIP_BLOCKS = 1024         # sumsq_partial_kernel's grid cap = dgx_clip_coef_workspace_floats() (the GPU test asserts it)

ADAMW_MUTANTS = ("ema_post", "wd_from_lr", "seg_trip", "seg_ge", "clip_before_scale", "bc2_for_sqrt", "nan_to_minus_clip", "shadow_pre")
SGD_MUTANTS = ("ema_post", "seg_trip", "seg_ge", "clip_before_scale", "buf_step1", "nesterov_dropped", "nan_to_minus_clip", "shadow_pre")


def f32(x):
    return np.float32(x)


def f32v(x):
    """the value a C float argument holds"""
    return float(np.float32(x))


def worst_ratio(got, ref, bnd):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    bnd = torch.as_tensor(bnd, device=ref.device).double()
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    nan_ref = torch.isnan(ref)
    inf = torch.full_like(err, float("inf"))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.expand_as(err).clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(err) & torch.isfinite(ratio), ratio, inf)
    ratio = torch.where(nan_ref, torch.where(torch.isnan(got), torch.zeros_like(err), inf), ratio)     # NaN rule
    return float(ratio.max())


# ============================================================================================ segments
def segment_of(e, seg_end):
    """The segment of ELEMENT e: the first index whose exclusive end lies behind e; elements behind the last end belong to the last
    segment (the kernel's search never leaves [0, n_seg - 1])."""
    return torch.searchsorted(seg_end, e, right=True).clamp_max(seg_end.numel() - 1)


def segment_of_scalar(e, ends):
    """the kernel's loop, literally"""
    lo, hi = 0, len(ends) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if ends[mid] > e:
            hi = mid
        else:
            lo = mid + 1
    return lo


def quad_segment(i, seg_end, S=None, mutant=None):
    """The segment the KERNEL uses for all four elements of quad i: that of element 4 i.  Mutants: 'seg_trip' looks the second quad
    of a trip (S = quads per grid sweep) up by the first, 'seg_ge' compares with >= instead of >."""
    if mutant == "seg_trip":
        i = i - ((i // S) % 2) * S
    return torch.searchsorted(seg_end, 4 * i, right=mutant != "seg_ge").clamp_max(seg_end.numel() - 1)


def element_multipliers(e, seg):
    """float32 lr multiplier of every element index in e (None without segments)"""
    if seg is None:
        return None
    seg_end, lr_scale = seg
    return lr_scale.to(e.device)[segment_of(e, seg_end.to(e.device))]


def make_segments(gen, n4, S, variant, n_seg=400):
    """-> (seg_end i64, lr_scale f32) on the CPU for an arena of n4 quads.  'full': up to 400 segments with random 4-aligned ends, among
    them a run of 4-element segments at the front and around every multiple of S, an end exactly at 4 S and at 8 S, multipliers that
    include 0 and 1, the last end = n.  'short_last': the same with the last end smaller than n.  'one': n_seg = 1."""
    n = 4 * n4
    if variant == "one":
        return torch.tensor([n], dtype=I64), torch.tensor([0.25], dtype=F32)
    must = set(q for q in range(1, 9) if q < n4)
    for r in (1, 2, 3):
        must.update(q for q in range(r * S - 2, r * S + 3) if 0 < q < n4)
    want = max(min(n_seg, n4) - 1, 0)
    must = sorted(must)[:want]
    pool = torch.randperm(max(n4 - 1, 0), generator=gen)[:4 * n_seg].tolist()
    ends = set(must)
    for q in pool:
        if len(ends) >= want:
            break
        ends.add(q + 1)
    last = n4 if variant == "full" or n4 < 8 else n4 - min(5, n4 // 3)
    ends = sorted(q for q in ends if q < last) + [last]
    seg_end = 4 * torch.tensor(ends, dtype=I64)
    vals = torch.tensor([0.0, 1.0, 0.1, 0.25, 0.5, 2.0], dtype=F32)
    lr_scale = vals[torch.randint(0, vals.numel(), (len(ends),), generator=gen)]
    lr_scale[:min(6, len(ends))] = vals[:min(6, len(ends))]
    lr_scale = lr_scale[torch.randperm(len(ends), generator=gen)] if len(ends) > 1 else lr_scale
    return seg_end, lr_scale


# ============================================================================================ scalars
def _gscale(hp):
    gs = f32(hp["grad_scale"])
    return gs * f32(hp["scale_dev"]) if hp.get("scale_dev") is not None else gs            # float32 product: gscale *= *scale_dev


def adamw_scalars(hp):
    b1, b2, step, decay = f32(hp["beta1"]), f32(hp["beta2"]), int(hp["step"]), f32(hp.get("ema_decay", 0.0))
    clip = f32(hp["clip_value"])
    return types.SimpleNamespace(
        lr=float(f32(hp["lr"])), b1=float(b1), b2=float(b2), eps=float(f32(hp["eps"])), wd=float(f32(hp["weight_decay"])),
        clip=float(clip) if clip > 0 else float("inf"), gscale=float(_gscale(hp)), decay=float(decay),
        omd=float(f32(1.0) - decay), omb1=float(f32(1.0) - b1), omb2=float(f32(1.0) - b2),
        bc1=float(f32(1.0 - math.pow(float(b1), float(step)))), bc2s=float(f32(math.sqrt(1.0 - math.pow(float(b2), float(step))))),
        bc2=float(f32(1.0 - math.pow(float(b2), float(step)))), step=step)


def sgd_scalars(hp):
    clip, decay = f32(hp["clip_value"]), f32(hp.get("ema_decay", 0.0))
    return types.SimpleNamespace(
        lr=float(f32(hp["lr"])), mom=float(f32(hp["momentum"])), nesterov=bool(hp["nesterov"]), wd=float(f32(hp["weight_decay"])),
        clip=float(clip) if clip > 0 else float("inf"), gscale=float(_gscale(hp)), decay=float(decay), omd=float(f32(1.0) - decay),
        first=int(hp["step"]) == 1, step=int(hp["step"]))


def _clamp(x, clip, mutant):
    """fminf(fmaxf(x, -clip), clip) with a NaN kept (torch.clamp propagates it); the mutant absorbs it as fmaxf / fminf alone would"""
    y = x if math.isinf(clip) else x.clamp(-clip, clip)
    if mutant == "nan_to_minus_clip":
        y = torch.where(torch.isnan(x), torch.full_like(x, -clip), y)
    return y


def _lre(p, mult, lr):
    """float32 lr * lr_scale[segment] per element (a 0-dim tensor without segments)"""
    one = torch.ones((), dtype=F32, device=p.device)
    return (one if mult is None else mult.to(F32)) * lr


# ============================================================================================ AdamW + EMA
def adamw_ref64(p, g, m, v, ema, mult, sc, dt=F64, mutant=None):
    """One step from the float32 state (p, g, m, v, ema | None), mult = float32 lr multiplier per element | None.  -> (out, bounds):
    out = {p, m, v[, ema]} in dt; bounds (dt = float64 only) per element.  The operation sequence is adamw_ema_kernel's:
        gr = clamp(g * gscale);  p *= 1 - lre * wd;  m += (gr - m) * (1 - b1);  v = v * b2 + ((1 - b2) * gr) * gr
        p -= (lre / bc1) * (m / (sqrt(v) / bc2s + eps));  ema = ema * decay + (1 - decay) * p_before"""
    lre32 = _lre(p, mult, sc.lr)
    dfac32 = 1.0 - (torch.ones((), dtype=F32, device=p.device) * sc.lr if mutant == "wd_from_lr" else lre32) * sc.wd
    lre, dfac = lre32.to(dt), dfac32.to(dt)
    P, G, M, V = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    gr = _clamp(G, sc.clip, mutant) * sc.gscale if mutant == "clip_before_scale" else _clamp(G * sc.gscale, sc.clip, mutant)
    pd = P * dfac
    m2 = M + (gr - M) * sc.omb1
    v2 = V * sc.b2 + (sc.omb2 * gr) * gr
    s = torch.sqrt(v2)
    sb = s / (sc.bc2 if mutant == "bc2_for_sqrt" else sc.bc2s)
    den = sb + sc.eps
    q = m2 / den
    ss = lre / sc.bc1
    upd = ss * q
    p2 = pd - upd
    out = {"p": p2, "m": m2, "v": v2}
    if ema is not None:
        E = ema.to(dt)
        out["ema"] = E * sc.decay + sc.omd * (p2 if mutant == "ema_post" else P)
    if dt != F64:
        return out, None
    A = torch.abs
    agr = A(gr)
    # m: 4 roundings (scale, subtract, multiply, add), each at most u (|m| + (1-b1)(|gr| + |m|))                                k = 4
    b_m = 4 * U * (A(M) + sc.omb1 * (agr + A(M))) + 4 * TINY
    # v: the scale enters twice (2), (1-b2)*gr (1), *gr (1), v*b2 (1), add (1): the gr^2 term sees 5, the v term 2            k = 5
    b_v = 5 * U * (V * sc.b2 + sc.omb2 * gr * gr) + 5 * TINY
    # sqrt (1 ulp), / bc2s (u), + eps (u)
    d_s = torch.minimum(b_v / s.clamp_min(1e-300), torch.sqrt(b_v)) + ULP_SQRT * U * s
    d_den = d_s / sc.bc2s + ULP_DIV * U * sb + U * den + 2 * TINY
    # q = m / den (u), ss = lre / bc1 (u), upd = ss * q (u), p = p * dfac (u) - upd (u): k = 2 on |p dfac| + |p'|, 3 on |upd|, plus
    # the errors of m and den carried through the quotient
    d_q = b_m / den + A(m2) * d_den / (den * den) + ULP_DIV * U * A(q) + TINY
    d_upd = ss * d_q + ULP_DIV * U * ss * A(q) + U * A(upd) + TINY
    b_p = U * A(pd) + d_upd + U * A(p2) + 2 * TINY
    bnd = {"p": b_p * SECOND, "m": b_m * SECOND, "v": b_v * SECOND}
    if ema is not None:
        # ema: multiply, multiply, add: u (|ema| decay + (1-decay)|p| + |ema'|) <= 2 u (|ema| decay + (1-decay)|p|)               k = 2
        bnd["ema"] = (2 * U * (A(E) * sc.decay + sc.omd * A(P)) + 3 * TINY) * SECOND
    return out, bnd


# ============================================================================================ SGD + EMA
def sgd_ref64(p, g, buf, ema, mult, sc, dt=F64, mutant=None):
    """sgd_ema_kernel: d = clamp(g * gscale) + wd * p;  buf = first ? d : mom * buf + d (the old buffer is not read at step 1);
    d = nesterov ? d + mom * buf : buf;  p -= lre * d;  momentum == 0: no buffer.  -> (out {p[, buf][, ema]}, bounds)."""
    lre = _lre(p, mult, sc.lr).to(dt)
    P, G = p.to(dt), g.to(dt)
    gr = _clamp(G, sc.clip, mutant) * sc.gscale if mutant == "clip_before_scale" else _clamp(G * sc.gscale, sc.clip, mutant)
    wp = sc.wd * P
    d = gr + wp
    A = torch.abs
    # d: scale, wd * p, add: u (|gr| + wd |p| + |d|) <= 2 u (|gr| + wd |p|)                                                    k = 2
    b_d = U * (A(gr) + A(wp) + A(d)) + 3 * TINY
    out = {}
    if sc.mom != 0.0:
        first = sc.first and mutant != "buf_step1"
        if first:
            b2 = d
            b_b = b_d                                                                                                        # k = 2
        else:
            B = buf.to(dt)
            b2 = sc.mom * B + d
            # buf: mom * buf (1), add (1), on top of d's 2: <= 3 u (mom |buf| + |gr| + wd |p|)                                 k = 3
            b_b = U * sc.mom * A(B) + b_d + U * A(b2) + 2 * TINY
        if sc.nesterov and mutant != "nesterov_dropped":
            dd = d + sc.mom * b2
            # d + mom * buf': mom * buf' (1), add (1) on top of d (2) and mom buf' (3): <= 5 u (sum of the magnitudes)         k = 5
            b_dd = b_d + sc.mom * b_b + U * sc.mom * A(b2) + U * A(dd) + 2 * TINY
        else:
            dd, b_dd = b2, b_b
        out["buf"] = b2
    else:
        dd, b_dd, b_b = d, b_d, None
    step = lre * dd
    p2 = P - step
    out["p"] = p2
    # p: lre * d (1), subtract (1) on top of d's k: <= (k_d + 2) u (|p| + lre (sum of d's magnitudes))                  k = 4 .. 7
    b_p = lre * b_dd + U * A(step) + U * A(p2) + 2 * TINY
    if ema is not None:
        E = ema.to(dt)
        out["ema"] = E * sc.decay + sc.omd * (p2 if mutant == "ema_post" else P)
    if dt != F64:
        return out, None
    bnd = {"p": b_p * SECOND}
    if b_b is not None:
        bnd["buf"] = b_b * SECOND
    if ema is not None:
        bnd["ema"] = (2 * U * (A(E) * sc.decay + sc.omd * A(P)) + 3 * TINY) * SECOND                                         # k = 2
    return out, bnd


# ============================================================================================ the float32 stand-in and the checks
def quad_multipliers(n4, seg, S, mutant=None, device="cpu"):
    """float32 multiplier of every element as the KERNEL finds it: per quad, by its first element"""
    if seg is None:
        return None
    seg_end, lr_scale = seg[0].to(device), seg[1].to(device)
    i = torch.arange(n4, dtype=I64, device=device)
    return lr_scale[quad_segment(i, seg_end, S, mutant)].repeat_interleave(4)


def step_f32(kind, case, S, mutant=None):
    """The kernel's operation sequence in float32 on the CPU: the stand-in for a correct kernel (mutant None) or for one with one
    deliberate error.  -> got dict as the GPU test builds it from the device arrays."""
    inp, sc, seg = case["inp"], case["sc"], case["seg"]
    mult = quad_multipliers(inp["p"].numel() // 4, seg, S, mutant)
    if kind == "adamw":
        out, _ = adamw_ref64(inp["p"], inp["g"], inp["m"], inp["v"], inp.get("ema"), mult, sc, dt=F32, mutant=mutant)
    else:
        out, _ = sgd_ref64(inp["p"], inp["g"], inp.get("buf"), inp.get("ema"), mult, sc, dt=F32, mutant=mutant)
    if case["shadow"]:
        out["shadow"] = (inp["p"] if mutant == "shadow_pre" else out["p"]).to(BF16)
    return out


def step_check(kind, case, got, idx=None, device=None, chunk=1 << 22):
    """Every element (idx None) or the elements idx of `got` against the float64 restatement evaluated on `device` in chunks.
    -> (worst ratio per output, list of broken exact contracts)."""
    inp, sc, seg = case["inp"], case["sc"], case["seg"]
    device = device or inp["p"].device
    total = inp["p"].numel() if idx is None else idx.numel()
    worst, broken = {}, []
    for a in range(0, total, chunk):
        b = min(a + chunk, total)
        sel = slice(a, b) if idx is None else idx[a:b]
        e = torch.arange(a, b, dtype=I64, device=device) if idx is None else sel.to(device)

        def take(t):
            return None if t is None else t[sel].to(device)
        mult = element_multipliers(e, seg)
        if kind == "adamw":
            ref, bnd = adamw_ref64(take(inp["p"]), take(inp["g"]), take(inp["m"]), take(inp["v"]), take(inp.get("ema")), mult, sc)
        else:
            ref, bnd = sgd_ref64(take(inp["p"]), take(inp["g"]), take(inp.get("buf")), take(inp.get("ema")), mult, sc)
        for k in ref:
            worst[k] = max(worst.get(k, 0.0), worst_ratio(take(got[k]), ref[k], bnd[k]))
        gp = take(got["p"])
        if got.get("shadow") is not None:
            sh, want = take(got["shadow"]), gp.to(BF16)
            nan = torch.isnan(gp)
            if not bool(((sh.view(torch.int16) == want.view(torch.int16)) | (nan & torch.isnan(sh))).all()):
                broken.append("shadow != round-to-nearest-even of the kernel's own p")
        if mult is not None:
            still = (mult == 0) & torch.isfinite(ref["p"])
            if not bool((gp.view(torch.int32)[still] == take(inp["p"]).view(torch.int32)[still]).all()):
                broken.append("p changed in a segment with lr multiplier 0")
    return worst, sorted(set(broken))


# ============================================================================================ cases
def hard_targets(clip_on, c):
    """(name, target of g * gscale | None, state override).  c = the clip value (1.0 stands in when clipping is off)."""
    big = float("inf") if clip_on else 1e15
    return [("zero", 0.0, None), ("+clip", c, None), ("-clip", -c, None), ("+clip(1+2^-23)", c * (1 + 2.0 ** -23), None),
            ("+clip(1-2^-23)", c * (1 - 2.0 ** -23), None), ("-clip(1+2^-23)", -c * (1 + 2.0 ** -23), None),
            ("-clip(1-2^-23)", -c * (1 - 2.0 ** -23), None), ("+inf|1e15", big, None), ("-inf|-1e15", -big, None), ("1e-30", 1e-30, None),
            ("1e15", 1e15, None), ("nan", float("nan"), None), ("v0_g0", 0.0, "v0"), ("v0", None, "v0"), ("p+1e6", None, "p+"),
            ("p-1e6", None, "p-")]


def anchors_for(n4, S):
    """element offsets of the blocks of hard inputs: the start of every (trip, u) region of the step kernels' loops and the tail"""
    n = 4 * n4
    a = [4 * r * S for r in range((n4 + S - 1) // S)]
    if n >= 32:
        a.append(n - 16)
    return a


def _state(gen, n, scale_g):
    dev = gen.device
    r = lambda: torch.randn(n, generator=gen, device=dev, dtype=F32)            # noqa: E731
    p = r()
    p = torch.where(p == 0, torch.full_like(p, 0.5), p)
    m = 0.1 * r()
    m = torch.where(m == 0, torch.full_like(m, 0.05), m)
    v = (0.1 * r()) ** 2 + 1e-6
    return {"p": p, "g": r() * scale_g, "m": m, "v": v, "ema": r() + 0.25, "buf": r() + 0.125}


def _place_hard(inp, hp, n4, S, with_v):
    n = 4 * n4
    gscale = float(_gscale(hp))
    clip_on = hp["clip_value"] > 0
    hard = {}
    for a in anchors_for(n4, S):
        for k, (name, target, state) in enumerate(hard_targets(clip_on, float(f32(hp["clip_value"])) if clip_on else 1.0)):
            e = a + k
            if e >= n:
                break
            if target is not None:
                inp["g"][e] = float(np.float32(target / gscale))
            if state == "v0" and with_v:
                inp["v"][e] = 0.0
            if state in ("p+", "p-"):
                inp["p"][e] = 1e6 if state == "p+" else -1e6
            hard[e] = name
    return hard


ADAMW_OPTION_SETS = {
    # everything on: ema + shadow + clip + scale_dev + segments + found_inf present and zero; step 5
    "on": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, clip_value=1.0, grad_scale=1.0 / 65536, scale_dev=0.5, step=5,
               ema_decay=0.999, ema=True, shadow=True, segments="full", found_inf=True),
    # everything off: what engine/bsgal.py's trial step asks for -- betas (0, 0) at step 1, no decay, no clip
    "off": dict(lr=1e-4, beta1=0.0, beta2=0.0, eps=1e-8, weight_decay=0.0, clip_value=0.0, grad_scale=1.0, scale_dev=None, step=1,
                ema_decay=0.0, ema=False, shadow=False, segments=None, found_inf=False),
    # step 90 000 (bias corrections ~ 1), a scale that is no power of two, n_seg = 1
    "mixA": dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4, clip_value=0.5, grad_scale=0.37, scale_dev=None, step=90000,
                 ema_decay=0.9998, ema=True, shadow=False, segments="one", found_inf=False),
    # step 1 with the usual betas, clipping off, a last seg_end smaller than n
    "mixB": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, clip_value=0.0, grad_scale=1.0, scale_dev=0.731, step=1,
                 ema_decay=0.0, ema=False, shadow=True, segments="short_last", found_inf=True),
}


def _cpu_gen(gen):
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen, device=gen.device))
    return torch.Generator().manual_seed(seed)


def adamw_case(gen, n4, S, optset):
    """A one-step AdamW case of n4 quads on gen's device; S = quads per grid sweep (dgx_optim_grid_quads on the GPU, small on the
    host).  -> {inp, sc, hp, seg, shadow, found_inf, hard {element: name}}"""
    hp = dict(ADAMW_OPTION_SETS[optset])
    inp = _state(gen, 4 * n4, 3.0 / abs(float(_gscale(hp))))
    del inp["buf"]
    if not hp["ema"]:
        inp["ema"] = None
    hard = _place_hard(inp, hp, n4, S, True)
    seg = make_segments(_cpu_gen(gen), n4, S, hp["segments"]) if hp["segments"] else None
    return {"inp": inp, "sc": adamw_scalars(hp), "hp": hp, "seg": seg, "shadow": hp["shadow"], "found_inf": hp["found_inf"], "hard": hard,
            "n4": n4}


SGD_OPTION_SETS = {
    # the four (momentum, nesterov, clip) sets of test_sgd_ema_step_vs_torch_sgd; the last one's norm clip arrives as scale_dev
    "mom": dict(lr=0.02, momentum=0.9, nesterov=False, weight_decay=1e-3, clip_value=1.0, grad_scale=1.0, scale_dev=None, ema_decay=0.999,
                ema=True, shadow=True, segments="full", found_inf=True),
    "nesterov": dict(lr=0.02, momentum=0.9, nesterov=True, weight_decay=1e-3, clip_value=1.0, grad_scale=1.0 / 65536, scale_dev=None,
                     ema_decay=0.999, ema=True, shadow=False, segments="short_last", found_inf=False),
    "plain": dict(lr=0.02, momentum=0.0, nesterov=False, weight_decay=1e-3, clip_value=1.0, grad_scale=0.37, scale_dev=None, ema_decay=0.0,
                  ema=False, shadow=True, segments="one", found_inf=False),
    "normclip": dict(lr=0.02, momentum=0.9, nesterov=False, weight_decay=1e-3, clip_value=0.0, grad_scale=1.0, scale_dev=0.3172,
                     ema_decay=0.999, ema=True, shadow=True, segments="full", found_inf=False),
}


def sgd_case(gen, n4, S, optset, step):
    hp = dict(SGD_OPTION_SETS[optset], step=step)
    inp = _state(gen, 4 * n4, 3.0 / abs(float(_gscale(hp))))
    del inp["m"], inp["v"]
    if not hp["ema"]:
        inp["ema"] = None
    if hp["momentum"] == 0.0:
        inp["buf"] = None
    hard = _place_hard(inp, hp, n4, S, False)
    seg = make_segments(_cpu_gen(gen), n4, S, hp["segments"]) if hp["segments"] else None
    return {"inp": inp, "sc": sgd_scalars(hp), "hp": hp, "seg": seg, "shadow": hp["shadow"], "found_inf": hp["found_inf"], "hard": hard,
            "n4": n4}


def sample_indices(case, S, gen=None, n_random=65536, edge=1024):
    """The elements the GPU test evaluates a second time on the CPU: the first and last `edge` quads of every (trip, u) region, every
    hard input, every segment boundary +- 1 quad, n_random random ones.  -> sorted unique int64 (CPU)."""
    n4 = case["n4"]
    quads = []
    for r in range((n4 + S - 1) // S):
        lo, hi = r * S, min((r + 1) * S, n4)
        quads += [torch.arange(lo, min(lo + edge, hi)), torch.arange(max(hi - edge, lo), hi)]
    if case["seg"] is not None:
        b = case["seg"][0] // 4
        quads += [(b + d).clamp(0, n4 - 1) for d in (-1, 0, 1)]
    q = torch.cat(quads).to(I64)
    el = [(4 * q[:, None] + torch.arange(4)[None]).reshape(-1), torch.tensor(sorted(case["hard"]), dtype=I64)]
    if n_random:
        el.append(torch.randint(0, 4 * n4, (n_random,), generator=gen or torch.Generator().manual_seed(n4)))
    return torch.unique(torch.cat(el))


# ============================================================================================ full-model norm clip
def clip_trips(n4, blocks=CLIP_BLOCKS):
    grid = min((n4 + 255) // 256, blocks)
    return grid, (n4 + grid * 256 - 1) // (grid * 256)


def clip_coef_ref64(g, grad_scale, max_norm, blocks=CLIP_BLOCKS):
    """dgx_clip_coef_f32: norm = ||g||_2 |grad_scale|, coef = min(1, max_norm / (norm + 1e-6f)); a NaN norm gives a NaN coefficient.
    -> ({coef, norm} float64 0-dim, bounds).  The kernel: per lane the squares of a quad summed as (x^2 + y^2) + (z^2 + w^2) and added
    to the lane's running sum, once per trip; 6 wave-shuffle additions; 2 levels of the four-wave fold; the block partials folded and
    rooted in double; rounded to float, times |gscale|.  All addends are >= 0, so the sum's relative error is at most
    chain u with chain = 1 (square) + 2 (quad) + trips + 6 + 2; the root halves it; the rounding to float and the product add 2 u:
        norm: k = chain / 2 + 2        coef: + 1e-6f (u), / (u), carried through max_norm / t."""
    gs, mx = f32v(grad_scale), f32v(max_norm)
    n4 = g.numel() // 4
    _, trips = clip_trips(n4, blocks)
    chain = 1 + 2 + trips + 6 + 2
    G = g.double()
    norm = torch.sqrt((G * G).sum()) * abs(gs)
    t = norm + f32v(1e-6)
    r = mx / t
    coef = torch.where(torch.isnan(norm), norm, r.clamp_max(1.0))
    b_norm = ((chain / 2.0 + 2.0) * U + 2.0 ** -48) * norm + TINY
    b_coef = r * (b_norm / t + U) + ULP_DIV * U * r + TINY
    return {"coef": coef, "norm": norm}, {"coef": b_coef * SECOND, "norm": b_norm * SECOND}


def clip_coef_f32(g, grad_scale, max_norm, blocks=CLIP_BLOCKS, mutant=None):
    """the kernels' operation sequence and summation order in float32 on the CPU"""
    gs, mx = f32(grad_scale), f32(max_norm)
    n4 = g.numel() // 4
    grid, trips = clip_trips(n4, blocks)
    q = torch.zeros(trips * grid * 256, 4, dtype=F32)
    q[:n4] = g.float().view(n4, 4)
    q = q.view(trips, grid * 256, 4)
    s = torch.zeros(grid * 256, dtype=F32)
    for t in range(trips):
        x = q[t]
        s = s + ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + (x[:, 2] * x[:, 2] + x[:, 3] * x[:, 3]))
    s = s.view(grid, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ o]
    red = s[:, :, 0]
    part = (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])
    norm = np.float32(math.sqrt(float(part.double().sum()))) * np.float32(abs(gs))
    with np.errstate(all="ignore"):
        coef = np.float32(1.0) if mutant == "nan_to_one" and np.isnan(norm) else \
            (norm if np.isnan(norm) else min(np.float32(1.0), mx / (norm + np.float32(1e-6))))
    return {"coef": torch.tensor(float(coef), dtype=F64), "norm": torch.tensor(float(norm), dtype=F64)}


def clip_case(gen, n4):
    """lognormal gradients, sigma = 4, random signs"""
    dev = gen.device
    z = torch.randn(4 * n4, generator=gen, device=dev, dtype=F32)
    sgn = torch.where(torch.rand(4 * n4, generator=gen, device=dev) < 0.5, -1.0, 1.0)
    return (torch.exp(4.0 * z) * sgn).to(F32)
