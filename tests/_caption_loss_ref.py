"""numpy restatement, in float64, of what include/divergen_hip.h states for dgx_caption_prepare + dgx_caption_loss: the prepared caption
rows, the chosen row per image, the loss, stats_l_caption, the whole gradient of the projected rows u, d cls_bias and, per gradient
element, the condition floor the tests' bounds are relative to.  Everything is float64 on the values as stored (fp32 or bf16 inputs
are used as given).

The floor of a value is the sum of the absolute values of its addends, carried through the chain: a logit s_j = h . c_j + bias has the
floor A_j = sum_d |h_d c_jd| + |bias|; a logit gradient g_j = K w_j (sigmoid(s_j) - t_j) has K w_j (sigmoid(s_j) + t_j) + K w_j
sigmoid'(s_j) A_j (its two addends -- torch's backward forms sigmoid(s) - t, which at a saturated positive is 1.0f - 1 -- plus what an
error of the logit at the size of ITS floor moves it by: at NORM_TEMP 50 the logits reach +-50, where an fp32 rounding of the logit is
worth more than an fp32 rounding of g); dh = sum_j g_j c_j and the projection dh - uhat (uhat . dh) sum the
absolute addends with those floors in place of |g_j|.

`inputs()` / `gpu_cases()` are frozen input builders: the golden generator and the tests build the same bytes."""
import numpy as np

EPS = 1e-12
MUTANTS = ("first_row", "no_neg_weight", "no_projection", "target_unsynced", "mean_over_valid")


def f64(a):
    return np.asarray(a, np.float64)


def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def prepare(cap, D, norm_weight=True):
    """cap (N, >= D): the first D columns, each row divided by max(|row|, 1e-12) when norm_weight."""
    c = f64(cap)[:, :D]
    if not norm_weight:
        return c.copy()
    return c / np.maximum(np.sqrt((c * c).sum(1, keepdims=True)), EPS)


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def caption_loss(u, valid, counts, cap, D, target0, temp, norm_weight, bias, neg_weight, scale, stat_scale, upstream=1.0, ld_du=None,
                 mutant=None):
    """u (R_alloc, ld_u), valid (R,) or None, counts per image, cap (N, >= D) RAW caption rows (prepare() is applied here), bias a float
    or None.  -> dict(loss, l_caption, sel, du (R_alloc, ld_du), floor_du, dbias, floor_dbias, floor_loss, logits [per image or None])."""
    u = f64(u)
    R_alloc = u.shape[0]
    ld_du = u.shape[1] if ld_du is None else ld_du
    B = len(counts)
    c = prepare(cap, D, norm_weight)
    N = c.shape[0]
    b0 = 0.0 if bias is None else float(bias)
    nw = 1.0 if mutant == "no_neg_weight" else float(neg_weight)
    R = sum(counts)
    valid = np.ones(R, bool) if valid is None else np.asarray(valid).astype(bool)
    du, fdu = np.zeros((R_alloc, ld_du)), np.zeros((R_alloc, ld_du))
    sel, logits = [], []
    total, ftotal, gsum, fgsum = 0.0, 0.0, 0.0, 0.0
    r0 = 0
    counted = 0
    for b, n in enumerate(counts):
        rows = [r for r in range(n) if valid[r0 + r]]
        if not rows:
            sel.append(-1)
            logits.append(None)
            r0 += n
            continue
        counted += 1
        pick = rows[0] if mutant == "first_row" else rows[-1]
        sel.append(pick)
        x = u[r0 + pick, :D]
        nrm = np.sqrt((x * x).sum())
        h = temp * x / max(nrm, EPS) if norm_weight else x
        s = c @ h + b0
        A = np.abs(c * h).sum(1) + abs(b0)
        logits.append(s)
        t = np.zeros(N)
        t[(b if mutant == "target_unsynced" else target0 + b)] = 1.0
        w = np.where(t > 0.5, 1.0, nw)
        sg = sigmoid(s)
        l_el = np.maximum(s, 0.0) - s * t + np.log1p(np.exp(-np.abs(s)))
        dg = np.where(t > 0.5, -sigmoid(-s), sg)              # sigmoid(s) - t without cancellation
        total += (w * l_el).sum()
        ftotal += (w * (np.maximum(s, 0.0) + np.abs(s * t) + np.log1p(np.exp(-np.abs(s))))).sum() + (w * np.abs(dg) * A).sum()
        K = scale * upstream
        g = K * w * dg
        fg = np.abs(K) * w * (sg + t) + np.abs(K) * w * sg * (1.0 - sg) * A      # the two addends of sigmoid(s) - t, as torch forms it
        gsum += g.sum()
        fgsum += fg.sum()
        dh = g @ c
        fdh = fg @ np.abs(c)
        if not norm_weight:
            row, frow = dh, fdh
        elif nrm > EPS and mutant != "no_projection":
            uh = x / nrm
            row = temp * (dh - uh * (uh @ dh)) / nrm
            frow = temp * (fdh + np.abs(uh) * (np.abs(uh) @ fdh)) / nrm
        else:
            den = nrm if (mutant == "no_projection" and nrm > EPS) else EPS
            row, frow = temp * dh / den, temp * fdh / den
        du[r0 + pick, :D] = row
        fdu[r0 + pick, :D] = frow
        r0 += n
    if mutant == "mean_over_valid" and counted:
        total *= B / counted
    return dict(loss=scale * total, l_caption=stat_scale * total, floor_loss=abs(scale) * ftotal, sel=sel, du=du, floor_du=fdu,
                dbias=gsum, floor_dbias=fgsum, logits=logits)


def worst_ratio(got, ref, floor, rel):
    """max over elements of |got - ref| / (rel * max(|ref|, floor)); elements whose bound is zero must be equal (ratio inf otherwise)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = rel * np.maximum(np.abs(ref), floor)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------------------------------- frozen inputs
TEMP, CAPTION_WEIGHT, IMAGE_LOSS_WEIGHT, NEG_CAP_WEIGHT = 50.0, 0.5, 0.1, 0.125


def unit_rows(rng, n, D):
    c = rng.standard_normal((n, D))
    return (c / np.sqrt((c * c).sum(1, keepdims=True))).astype(np.float32)


def row_counts(B):
    """Per-image row counts: 1, 3, 129, 0, then 5 ...; the images named in `invalidate` lose rows through validity bytes."""
    base = [1, 3, 129, 0, 5, 2, 7, 4]
    return [base[i % len(base)] for i in range(B)]


def gpu_case(B, N, D, target0, seed, hard=True):
    """One call: u (R + 3 pad rows, D) fp32, valid, counts, cap (N, D) raw (not normalised) caption rows.
    Rows: image 1 (3 rows) has its last two rows invalid, image 2 (129 rows) keeps them all, image 4 (5 rows) is all invalid, image 3
    has no rows.  Hard inputs (when the shapes have room): the chosen row of image 0 is parallel to its own caption and anti-parallel to
    the next (logits +-TEMP: the saturated BCE branches), caption N - 1 is all zeros unless it is a positive, captions of columns
    target0 + 1 (a positive when B > 1) and the last negative are identical, the chosen row of image 1 has magnitude 1e-3 and the
    chosen row of image 2 magnitude 1e3."""
    rng = np.random.default_rng(seed)
    counts = row_counts(B)
    R = sum(counts)
    u = rng.standard_normal((R + 3, D)).astype(np.float32)
    valid = np.ones(R, np.uint8)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    if B > 1:
        valid[off[1] + 1:off[1] + 3] = 0
    if B > 4:
        valid[off[4]:off[5]] = 0
    cap = (unit_rows(rng, N, D) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    if hard:
        neg = [j for j in range(N) if not (target0 <= j < target0 + B)]
        u[off[0] + 0] = 3.0 * cap[target0]                       # parallel to its own caption: logit +TEMP
        if neg:
            cap[neg[0]] = -0.5 * cap[target0]                    # anti-parallel: logit -TEMP
        elif B > 1:
            cap[target0 + B - 1] = -0.5 * cap[target0]           # (N == B: another image's caption)
        if len(neg) > 1:
            cap[neg[-1]] = 0.0                                   # an all-zero caption row (a rank on a box step)
        if B > 1 and len(neg) > 2:
            cap[neg[-2]] = cap[target0 + 1]                      # image 1's positive and a negative with the same logit
        if B > 1:
            u[off[1] + 0] *= np.float32(1e-3)
        if B > 2:
            u[off[2] + 128] *= np.float32(1e3)
    return dict(u=u, valid=valid, counts=counts, cap=cap, B=B, N=N, D=D, target0=target0)


# (B, N, D, target0, ld_cap - D, ld_u - D, cls_bias or None, negative weight, NORM_WEIGHT).  Every target0 is a multiple of B: a column the
# reference can name (B * rank + idx), so that its own fp32 evaluation can be measured on every case; N == B with target0 0 and weight 1
# is the unsynced form.  N = 256 takes four column blocks of the forward grid, N <= 64 one.
GPU_CASES = (
    (1, 1, 8, 0, 0, 0, None, 1.0, True),
    (1, 3, 8, 2, 1, 8, -2.0, 0.125, True),
    (1, 256, 512, 1, 0, 0, -4.6, 0.125, True),
    (2, 2, 512, 0, 0, 0, -4.6, 1.0, True),
    (2, 6, 512, 2, 1, 8, -4.6, 0.125, True),
    (2, 256, 1024, 254, 0, 0, -2.0, 1.0, True),
    (5, 5, 512, 0, 1, 0, None, 1.0, True),
    (5, 15, 1024, 10, 0, 8, -2.0, 0.125, True),
    (5, 256, 512, 5, 1, 0, -4.6, 0.125, True),
    (5, 256, 8, 0, 0, 8, None, 1.0, False),
    (32, 32, 512, 0, 0, 0, -4.6, 1.0, True),
    (32, 96, 512, 64, 1, 8, -4.6, 0.125, True),
    (32, 256, 1024, 32, 1, 0, -2.0, 0.125, True),
    (32, 256, 512, 224, 0, 8, None, 0.125, False),
)


def case_id(c):
    return "B%d-N%d-D%d-t%d-lc%d-lu%d-%s-w%g-%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "nobias" if c[6] is None else "bias", c[7],
                                                    "norm" if c[8] else "raw")


def scales(B):
    """(scale, stat_scale) of a batch of B images: CAPTION_WEIGHT * IMAGE_LOSS_WEIGHT / B and CAPTION_WEIGHT / B."""
    return CAPTION_WEIGHT * IMAGE_LOSS_WEIGHT / B, CAPTION_WEIGHT / B


def case_inputs(c, k):
    return gpu_case(c[0], c[1], c[2], c[3], seed=9000 + k)


def golden_inputs():
    """The frozen inputs of tests/golden/caption_loss.npz: B = 4 images of 5, 3, 0, 6 proposals (the reference has no validity bytes: it
    is given the surviving rows), input width 24, embedding width 16, C = 11 classes."""
    rng = np.random.default_rng(20261021)
    B, Cin, D, C = 4, 24, 16, 11
    counts = [5, 3, 0, 6]
    R = sum(counts)
    return dict(B=B, Cin=Cin, D=D, C=C, counts=counts,
                x=rng.standard_normal((R, Cin)).astype(np.float32),
                lin_w=(rng.standard_normal((D, Cin)) * 0.3).astype(np.float32), lin_b=(rng.standard_normal(D) * 0.1).astype(np.float32),
                zs=unit_rows(rng, C, D),
                cap=(unit_rows(rng, B, D) * rng.uniform(0.5, 2.0, (B, 1))).astype(np.float32),
                cap_other=(unit_rows(rng, 2 * B, D) * rng.uniform(0.5, 2.0, (2 * B, 1))).astype(np.float32),
                labels=[[1, 7], [3], [2], [0, 10, 4]], use_bias=-2.0, rank=1, world=3)
