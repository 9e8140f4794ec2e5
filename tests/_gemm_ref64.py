"""float64 restatements of the forward / input-gradient GEMM family (dgx_gemm_bf16_nt: csrc/gemm_nt.hip with its two-workgroup form,
gemm_lw.hip, gemm_k192.hip, the split-K fold) and of its six fused tails (csrc/gemm_common.h g_epi_finish), the per-element a-priori
bounds the GPU test holds the kernels to (tests/test_gpu_gemm_numerics.py), the case table both test files use, the input kinds and the
mutants.  Plain torch on the CPU; no project kernel is called from here.  tests/test_host_gemm_ref.py pins the restatements on torch's
float64 matmul / gelu / autograd and the window map on oracle.swin, shows that fp32 CPU evaluations of the contract stay inside every
bound, that every mutant leaves one, measures G / G' and confirms the plan column with gemm_plan.h (tests/native/gemm_plan_check.cpp).

The contract, restated:  y = bf16(acc + bias) is rounded FIRST (acc: fp32 sum of the exact bf16 x bf16 products, any order, any split),
the tail acts on the rounded y:
  mode 0 / 1   C = y; with relu every negative value and -0 become +0
  mode 2       C = y, C2 = bf16(GELU_erf(y)), both at stride ldc
  mode 4       C = bf16(y * GELU'(aux)), aux bf16 (M, ldaux), no bias
  mode 5       C = y where the saved bf16 aux > 0 (+0, -0 and negatives are not), else +0; no bias
  mode 3       out[tok] = res[tok] + scale[b] * y, tok from the window map: identity (ws = 0), classic (ws > 0: the rows of the padded,
               rolled, partitioned grid; padding rows are not stored) or compact (ws < 0: the classic rows without the padding ones);
               res / out fp32 or bf16, contiguous (tokens, N)
`gemm64` returns (ref, A, n): the float64 value of the case's main output, the SAME contraction over absolute values (+ |bias|; in
token order for mode 3) and the addend count K (+ 1 with a bias).

Bounds, per element, u = 2^-24, EB = 2^-8, no global term:
  e_y (modes 0, 1, C of mode 2, unmasked mode 5)   EB |ref| + ACC_FACTOR n u A (1 + EB)
  mode 2 C2, against float64 GELU of the kernel's OWN C    EB |ref| + G max(1, |y|) (1 + EB)
  mode 4       EB |ref| + (e_y |g'| + (|y| + e_y) (G' max(1, |aux|) + u |g'|)) (1 + EB)
  mode 5       masked positions are +0 bit for bit
  mode 3       fp32 stream: |sc| e_y + 2u (|res| + |sc y|);  bf16 stream: EB |ref| + that (1 + EB)
G, G': the absolute errors of the A&S 7.1.26 cdf and of cdf + x pdf as g_gelu_terms evaluates them in fp32.  The host test restates
g_gelu_terms and measures both over all 65 280 finite bf16 inputs against float64 erfc: G = 2.32e-7, G' = 2.38e-7 (MEASURED_G below); the
constants are twice that, the margin being for the device's __expf and v_rcp_f32.  A GELU result whose reference lies below 2^-126
gets an absolute 2^-126 more (the device may flush it): in the exhaustive sweep, and for GELU of a y below -13 (the host test asserts
that nothing else gets there).
Everywhere else the host test asserts that every compared reference is 0 or a normal bf16 magnitude.

ACC_FACTOR = 1: the MI355X run of tests/test_gpu_gemm_numerics.py needed no factor on the accumulation term, and G / G' stayed at twice
the host figures.  Worst measured |err| / bound per form and output of that run (every row of the table, every input kind, contiguous
and strided; 783 tests, every launch reported the plan of its row, no sentinel or stride gap was disturbed, the one-hot launches and
the repeated split-K / walked-item launches were bit-exact):
  form          y (modes 0, 1, C of 2)   C2      mode 4   mode 5   mode 3 out   where the worst y is
  gemm_nt       0.990                    0.968   0.951    0.987    0.985        (8, 8, 8) scaled, mode 0
  gemm_lw       0.992                    0.968   0.951    0.975    0.992        I' (1160, 1672, 72) ordinary, bias
  gemm_nt.2wg   0.990                    0.968   0.924    0.989    0.993        W'' (4104, 192, 136) ordinary, mode 0
  gemm_k192     0.988                    0.968   0.981    -        0.993        P (32776, 192, 192) ordinary, mode 0
  exhaustive GELU sweep, forms 0 / 1 / 2 alike: C bit-exact (subnormal inputs included), C2 0.968, mode 4 0.993
Every figure is the one bf16 rounding itself (half an ulp at the bottom of a binade is 2^-8 |ref| to within 2^-8 of it; the host-side
fp32 evaluations reach the same 0.95 - 0.99).  Of the G and G' terms the sweep needed 1e-4 and less than 5e-5 of the constant beyond
2^-8 |ref| (`share_used`), on the device as in the host restatement: the margin for __expf and v_rcp_f32 was not drawn on.

Input kinds (make_inputs): `ordinary` randn, weights x 0.1; `cancelling` a + 64 against mixed-sign b (A >> |ref|); `scaled` row m of a
times 2^((7m) % 41 - 20), column n of b times 2^((5n) % 31 - 15) (the bias follows its column, 2^-20 below it, so that it shows in the
small rows only); `signed_zero` post-ReLU a with planted -0 and a zero row, for the relu tails and mode 5.  The saved activation of
mode 5 carries planted +0 and -0 in every kind; the residual stream of mode 3 has every seventh token 256 times larger, the DropPath
factors are 1 / 0.7 and, for the second sample, 0.

Case table (CASES): Case(row, M, N, K, mode, relu, res_bf16, win, knobs, reserved, plan).  knobs are dgx_dev_set pairs, reserved is what
dgx_set_reserved_cus gets (CUs of the chip: 16 leaves 30 workgroups per XCD to gemm_lw, 128 leaves 16), plan is what
dgx_gemm_last_form must report, (form, bm, bn, splits); every launch has the WS_BYTES workspace.  Every case runs contiguous and at
lda = K + 8, ldb = K + 24, ldc = N + 16, ldaux = N + 40.
  T    all 7 tiles x gemm_lw 0 / 1, M = bm + 40, N = bn + 8, K = 200: a full and a partial row tile, a full and an 8-wide column tile,
       three K-tiles and an 8-element tail.  Every tail on 128x128 and 256x192, modes 1 and 4 on the others.
  W    (168, 384, 200), gemm_lw 0, gemm_2wg 2: the two-workgroup form with every compiled tail (mc -1, 2, 3, 4, 6)
  W'   (168, 384, 520), same knobs, mode 2: form 2 through split-K (2 slabs of 5 K-tiles)
  W''  (4104, 192, 136), default knobs, modes 0 and 5: form 2 by the library's own plan
  P    (32776, 192 | 576, 192), default knobs, modes 0 - 4, reserved 0 and 16: gemm_k192 with a partial last 32-row tile, one and three
       panels; mode 5 must fall to form 2
  S    (136, 200, 1096), gemm_splitk 0 (plan: 4 slabs 5+5+5+3), 2, 3, 5 (4+4+4+4+2), 18 (one K-tile each, the last the 8-element tail
       alone) x gemm_lw 0 / 1, every tail.  Mode 3 there is classic with ws = 7 over a 7 x 20 grid, so M = 147 (136 is no multiple of
       49) with 7 padding rows; the plans are the same.
  I    (300, 200, 3080), 128x128, gemm_splitk 49, gemm_lw 1: 294 items, 37 per XCD: two items per workgroup at reserved 0, three at 128
  I'   (1160, 1672, 72), 128x128, gemm_lw 1: 140 tiles, 18 per XCD: a second item at reserved 128, the one-item control at 0
  E    (1, 8, 8), (40, 192, 72), (8, 8, 8), default knobs: M = 1, K < 64, N = 8

Mutants (MUTANTS, the text next to each): wrong restatements of the kind the kernels could produce.  A mutant is DEFINED on a case
when its float64 value differs from the restatement's at all; it must then leave the bound somewhere."""
import collections
import functools
import itertools
import math

import torch

from _conv_ref64 import BF16_MAX, BF16_MIN_NORMAL, EB, U, in_bf16_normal_range, ratios, worst_ratio  # noqa: F401

ACC_FACTOR = 1.0
MEASURED_G, MEASURED_GP = 2.32e-7, 2.38e-7      # host fp32 restatement of g_gelu_terms, all finite bf16 inputs (test_host_gemm_ref.py)
G_CDF, G_GRAD = 2 * MEASURED_G, 2 * MEASURED_GP
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
WS_BYTES = 16 << 20
SENT = -7.5
BK = 64
TILES = [(256, 192), (192, 192), (128, 192), (192, 256), (128, 256), (256, 128), (128, 128)]      # gemm_plan.h nt_stages
INPUT_KINDS = ("ordinary", "cancelling", "scaled", "signed_zero")
FORM_NAMES = {0: "gemm_nt", 1: "gemm_lw", 2: "gemm_nt.2wg", 3: "gemm_k192"}

MUTANTS = {
    "chunk8": "the last 8 of K dropped",
    "k_tail_tile": "the partial last K-tile dropped",
    "tail_unmasked": "the last K-tile read 64 wide into the stride gap (which holds NaN)",
    "split_tail": "the last K-tile of every split dropped",
    "split_overlap": "the first K-tile of every split but the first counted twice",
    "bias_per_split": "the bias added once per split",
    "row_tail": "rows behind the last full row tile zero",
    "col_tail": "columns behind the last full column tile zero",
    "second_item_stale": "items after a gemm_lw workgroup's first reuse the first item's A rows",
    "c2_stride_n": "C2 written at stride N",
    "aux_stride_ldc": "aux read at stride ldc",
    "relu_mask_from_y": "mode 5 masks on the sign of y",
    "neg_zero_positive": "a -0 saved activation passes",
    "pad_rows_stored": "classic padding rows written to token 0",
    "shift_sign": "the roll runs the other way",
    "scale_of_row0": "the DropPath factor of sample 0 used for every row",
    "res_as_bf16": "an fp32 residual stream rounded to bf16 on the way in",
    "gelu_unsigned": "cdf of |x| on the negative side",
}

Case = collections.namedtuple("Case", "row M N K mode relu res_bf16 win knobs reserved plan")


def strides(case, strided):
    M, N, K = case.M, case.N, case.K
    return dict(lda=K + 8, ldb=K + 24, ldc=N + 16, ldaux=N + 40) if strided else dict(lda=K, ldb=K, ldc=N, ldaux=N)


def case_id(c):
    s = "%s-%dx%dx%d-m%d%s" % (c.row, c.M, c.N, c.K, c.mode, "r" if c.relu else "")
    if c.win:
        s += "-%s-ws%d" % ("bf16" if c.res_bf16 else "f32", c.win[3])
    s += "".join("-%s%d" % (k.replace("gemm_", ""), v) for k, v in c.knobs)
    return s + ("-res%d" % c.reserved if c.reserved else "")


# ------------------------------------------------------------------ the window map, by pad / roll / partition of an index grid
def window_rows(win, roll=-1):
    """(tok, b) per GEMM row: the token index of the (B, H*W) stream the row is stored to (-1: a padding row, not stored), its sample.
    roll = +1: the `shift_sign` mutant."""
    B, H, W, ws, shift = win
    T = B * H * W
    if ws == 0:
        tok = torch.arange(T)
        return tok, tok // (H * W)
    a = abs(ws)
    Hp, Wp = -(-H // a) * a, -(-W // a) * a
    grid = torch.full((B, Hp, Wp), -1, dtype=torch.int64)
    grid[:, :H, :W] = torch.arange(T).reshape(B, H, W)                     # pad
    grid = torch.roll(grid, (roll * shift, roll * shift), (1, 2))                     # cyclic shift
    tok = grid.reshape(B, Hp // a, a, Wp // a, a).permute(0, 1, 3, 2, 4).reshape(-1)      # partition
    b = torch.arange(B).repeat_interleave(Hp * Wp)
    if ws < 0:                                                             # compact: the same order without the padding rows
        keep = tok >= 0
        tok, b = tok[keep], b[keep]
    return tok, b


def win_rows(win):
    return int(window_rows(win)[0].numel())


def _identity_win(M):
    B = 2 if (M % 2 == 0 and M >= 4) else 1
    hw = M // B
    H = max(d for d in range(1, int(math.isqrt(hw)) + 1) if hw % d == 0)
    return (B, H, hw // H, 0, 0)


def _compact_win(M):
    B, H, W, _, _ = _identity_win(M)
    return (B, H, W, -7, min(3, H, W))


def _classic_win(M):
    """ws = 2, shift 1 over odd H and W: one padding row and one padding column per image"""
    windows = M // 4
    B = 2 if windows % 2 == 0 else 1
    nw = windows // B
    nWh = 3 if nw % 3 == 0 else 1
    return (B, 2 * nWh - 1, 2 * (nw // nWh) - 1, 2, 1)


_WIN = {"identity": _identity_win, "classic": _classic_win, "compact": _compact_win}


# ------------------------------------------------------------------ the case table
def _build_cases():
    cases, m3 = [], itertools.count()

    def add(row, M, N, K, mode, plan, knobs=(), reserved=0, relu=False, win=None, res_bf16=None):
        if mode == 3:
            i = next(m3)
            if win is None:
                win = _WIN["identity" if M % 4 else ("identity", "classic", "compact")[i % 3]](M)
            res_bf16 = (i // 3) % 2 if res_bf16 is None else res_bf16
            M = win_rows(win)
        cases.append(Case(row, M, N, K, mode, bool(relu), int(bool(res_bf16)), win, tuple(knobs), reserved, tuple(plan)))

    def tails(full):
        return [(0, 0), (1, 0), (1, 1), (2, 0), (3, 0), (4, 0), (5, 0)] if full else [(1, 0), (4, 0)]

    for bm, bn in TILES:
        for lw in (0, 1):
            for mode, relu in tails((bm, bn) in ((128, 128), (256, 192))):
                add("T", bm + 40, bn + 8, 200, mode, (lw, bm, bn, 1), (("gemm_tile", bm * 1000 + bn), ("gemm_lw", lw)), relu=relu)
    two = (("gemm_lw", 0), ("gemm_2wg", 2))
    for mode, relu in tails(True):
        add("W", 168, 384, 200, mode, (2, 128, 192, 1), two, relu=relu)
    for order, bf in (("identity", 1), ("classic", 0), ("compact", 1), ("compact", 0)):      # both streams see a window order
        add("W", 168, 384, 200, 3, (2, 128, 192, 1), two, win=_WIN[order](168), res_bf16=bf)
    add("W'", 168, 384, 520, 2, (2, 128, 192, 2), two)
    for mode in (0, 5):
        add("W''", 4104, 192, 136, mode, (2, 128, 192, 1))
    for N in (192, 576):
        for reserved in (0, 16):
            for mode in (0, 1, 2, 3, 4):
                add("P", 32776, N, 192, mode, (3, 32, 192, 1), reserved=reserved)
        add("P", 32776, N, 192, 5, (2, 128, 192, 1))
    for sk, splits in ((0, 4), (2, 2), (3, 3), (5, 5), (18, 18)):
        for lw in (0, 1):
            for mode, relu in tails(True):
                add("S", 136, 200, 1096, mode, (lw, 128, 128, splits), (("gemm_splitk", sk), ("gemm_lw", lw)), relu=relu,
                    win=(1, 7, 20, 7, 3) if mode == 3 else None)
    walk = (("gemm_tile", 128128), ("gemm_splitk", 49), ("gemm_lw", 1))
    for reserved in (0, 128):
        for mode, relu in ((1, 1), (2, 0), (3, 0), (4, 0), (5, 0)):
            add("I", 300, 200, 3080, mode, (1, 128, 128, 49), walk, reserved, relu=relu)
        for mode in (1, 3):
            add("I'", 1160, 1672, 72, mode, (1, 128, 128, 1), (("gemm_tile", 128128), ("gemm_lw", 1)), reserved)
    for (M, N, K), plan in (((1, 8, 8), (0, 128, 128, 1)), ((40, 192, 72), (0, 128, 192, 1)), ((8, 8, 8), (0, 128, 128, 1))):
        for mode, relu in tails(True):
            add("E", M, N, K, mode, plan, relu=relu)
    return cases


CASES = _build_cases()


def kinds_of(case):
    return INPUT_KINDS if (case.relu or case.mode == 5) else INPUT_KINDS[:3]


# ------------------------------------------------------------------ inputs
def seed_of(case, kind):
    return case.M * 7 + case.N * 13 + case.K * 29 + INPUT_KINDS.index(kind) * 1000003


def plant_zeros(t, gen):
    """+0 at a twelfth of the positions, -0 at another twelfth"""
    r = torch.rand(t.shape, generator=gen)
    t = torch.where(r < 1.0 / 12, torch.zeros_like(t), t)
    return torch.where((r >= 1.0 / 12) & (r < 1.0 / 6), -torch.zeros_like(t), t)


def make_inputs(kind, case, seed):
    """bf16 operands of a case: a (M, K), b (N, K), bias (N), aux (M, N; the saved pre-activation of mode 4 or activation of mode 5), and for
    mode 3 res (tokens, N) fp32 | bf16 with outlier tokens and scale (B) f32 with a dropped sample (None for the one-token case).  a, b and bias depend on (M, N, K, kind) alone."""
    M, N, K = case.M, case.N, case.K
    g = torch.Generator().manual_seed(seed)
    a, b, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    if kind == "cancelling":
        a = a + 64.0
    elif kind == "signed_zero":
        a = plant_zeros(torch.relu(a), g)
        a[M // 2] = 0.0
    a, b, bias = a.to(BF16), b.to(BF16), bias.to(BF16)
    if kind == "scaled":
        rs = torch.exp2(((7 * torch.arange(M)) % 41 - 20).double())[:, None]
        cs = torch.exp2(((5 * torch.arange(N)) % 31 - 15).double())
        a, b = (a.double() * rs).to(BF16), (b.double() * cs[:, None]).to(BF16)         # powers of two: exact
        bias = (bias.double() * cs * 2.0 ** -20).to(BF16)
    inp = {"a": a, "b": b, "bias": bias, "aux": None, "res": None, "scale": None}
    g2 = torch.Generator().manual_seed(seed + 17 * case.mode + 1)
    if case.mode == 4:
        inp["aux"] = (torch.randn(M, N, generator=g2) * 2.0).to(BF16)
    elif case.mode == 5:
        inp["aux"] = plant_zeros(torch.relu(torch.randn(M, N, generator=g2)), g2).to(BF16)
    elif case.mode == 3:
        B, H, W = case.win[:3]
        res = torch.randn(B * H * W, N, generator=g2)
        res[::7] *= 256.0              # outlier tokens: the stream's own precision shows beside the rounding of y
        inp["res"] = res.to(BF16 if case.res_bf16 else F32)
        if not (B == 1 and case.win[3] == 0):           # one sample in token order: no DropPath factor at all (a null pointer)
            inp["scale"] = torch.tensor([1.0 / 0.7, 0.0, 1.0 / 0.7][:B], dtype=F32)
    return inp


@functools.lru_cache(maxsize=6)
def inputs(case, kind):
    return make_inputs(kind, case, seed_of(case, kind))


@functools.lru_cache(maxsize=2)
def _contraction(M, N, K, kind):
    inp = inputs(Case("-", M, N, K, 0, False, 0, None, (), 0, (0, 128, 128, 1)), kind)
    return contract64(inp["a"], inp["b"])


def contraction(case, kind):
    """contract64 of the case's a and b, shared by the cases of one shape (a and b depend on (M, N, K, kind) alone)"""
    return _contraction(case.M, case.N, case.K, kind)


def one_hot_a(M, K):
    a = torch.zeros(M, K, dtype=BF16)
    a[torch.arange(M), (37 * torch.arange(M) + 11) % K] = 1.0
    return a


# ------------------------------------------------------------------ float64 pieces
def gelu64(x):
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_cdf64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_grad64(x):
    return gelu_cdf64(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def k_tiles(K):
    return -(-K // BK)


def split_ranges(case):
    """[(first K-tile, K-tiles)] of every split of the case's plan"""
    nt, S = k_tiles(case.K), case.plan[3]
    kps = -(-nt // S)
    return [(s * kps, min(kps, nt - s * kps)) for s in range(S)]


def lw_stale_items(case):
    """gemm_lw's work lists (gemm_lw.hip: items of an XCD are consecutive; workgroup j of XCD x walks x per_xcd + j, + wgx, ...):
    [(tile row m0, tile column n0, first K-tile, K-tiles, m0 of the workgroup's FIRST item)] of every later item"""
    form, bm, bn, S = case.plan
    tiles_n = -(-case.N // bn)
    total = -(-case.M // bm) * tiles_n
    items, per_xcd = total * S, (total * S + 7) // 8
    wgx = min(per_xcd, 32 - min((case.reserved + 7) // 8, 24))
    rng, out = split_ranges(case), []
    for x in range(8):
        bound = min((x + 1) * per_xcd, items)
        for j in range(wgx):
            first = x * per_xcd + j
            for L0 in range(first + wgx, bound, wgx):
                L, s = divmod(L0, S)
                out.append(((L // tiles_n) * bm, (L % tiles_n) * bn, rng[s][0], rng[s][1], (first // S // tiles_n) * bm))
    return out


def contract64(a, b, case=None, mutant=None, A=None):
    """(acc, A) float64: a b^T and |a| |b|^T; with a contraction mutant, acc is the mutant's"""
    a64, b64 = a.double(), b.double()
    A = a64.abs() @ b64.abs().t() if A is None else A
    M, K = a64.shape
    w = torch.ones(K, dtype=F64)
    if mutant == "chunk8":
        w[K - 8:] = 0
    elif mutant == "k_tail_tile":
        if K % BK == 0:
            return None, A
        w[K // BK * BK:] = 0
    elif mutant == "split_tail":
        if case.plan[3] == 1:
            return None, A
        for t0, nt in split_ranges(case):
            w[(t0 + nt - 1) * BK:(t0 + nt) * BK] = 0
    elif mutant == "split_overlap":
        if case.plan[3] == 1:
            return None, A
        for t0, nt in split_ranges(case)[1:]:
            w[t0 * BK:(t0 + 1) * BK] = 2
    acc = (a64 * w) @ b64.t()
    if mutant in ("row_tail", "col_tail"):
        bm, bn = case.plan[1:3]
        if mutant == "row_tail":
            acc[M // bm * bm:] = 0
        else:
            acc[:, b64.shape[0] // bn * bn:] = 0
    elif mutant == "second_item_stale":
        if case.plan[0] != 1:
            return None, A
        bm, bn = case.plan[1:3]
        for m0, n0, t0, nt, mf in lw_stale_items(case):
            if mf == m0:
                continue
            ks = slice(t0 * BK, min((t0 + nt) * BK, K))
            rows = min(bm, M - m0)
            stale = torch.zeros(rows, ks.stop - ks.start, dtype=F64)            # rows beyond M load as zero
            have = max(0, min(rows, M - mf))
            stale[:have] = a64[mf:mf + have, ks]
            bb = b64[n0:n0 + bn, ks]
            acc[m0:m0 + rows, n0:n0 + bn] += (stale - a64[m0:m0 + rows, ks]) @ bb.t()
    return acc, A


def evaluate64(case, inp, mutant=None, strided=False, pre=None):
    """The case in float64: {"y", "A", "n", outputs "C" / "C2" / "out", and the tail's own operands in the outputs' geometry}.  With a mutant:
    the mutant's outputs, or None where the mutant does not apply to the case at all.  pre: a cached contract64(a, b)."""
    M, N, K, mode = case.M, case.N, case.K, case.mode
    st = strides(case, True)
    bias = inp["bias"] if mode in (1, 2, 3) else None
    if mutant in ("chunk8", "k_tail_tile", "split_tail", "split_overlap", "row_tail", "col_tail", "second_item_stale"):
        acc, A = contract64(inp["a"], inp["b"], case, mutant, A=None if pre is None else pre[1].clone())
        if acc is None:
            return None
    else:
        acc, A = pre if pre is not None else contract64(inp["a"], inp["b"])
        acc, A = acc.clone(), A.clone()
    if mutant == "tail_unmasked":
        if not strided or K % BK == 0:
            return None
        acc = torch.full_like(acc, float("nan"))
    n = K
    if bias is not None:
        if mutant == "bias_per_split" and case.plan[3] == 1:
            return None
        acc += bias.double() * (case.plan[3] if mutant == "bias_per_split" else 1)
        A += bias.double().abs()
        n += 1
    elif mutant == "bias_per_split":
        return None
    r = {"y": acc, "A": A, "n": n}
    aux = inp["aux"]
    if mutant == "aux_stride_ldc":
        if not strided or aux is None:
            return None
        flat = torch.full((M * st["ldaux"] + st["ldc"],), float("nan"), dtype=F64)
        flat[:M * st["ldaux"]].view(M, st["ldaux"])[:, :N] = aux.double()
        aux = torch.stack([flat[m * st["ldc"]:m * st["ldc"] + N] for m in range(M)])
    if mode <= 1:
        if mutant in ("relu_mask_from_y", "neg_zero_positive", "gelu_unsigned", "c2_stride_n", "pad_rows_stored", "shift_sign", "scale_of_row0",
                      "res_as_bf16"):
            return None
        r["C"] = torch.clamp_min(acc, 0.0) + 0.0 if case.relu else acc
    elif mode == 2:
        if mutant in ("relu_mask_from_y", "neg_zero_positive", "pad_rows_stored", "shift_sign", "scale_of_row0", "res_as_bf16"):
            return None
        r["C"] = acc
        c2 = gelu64(acc)
        if mutant == "gelu_unsigned":
            c2 = torch.where(acc < 0, acc * gelu_cdf64(acc.abs()), c2)
        if mutant == "c2_stride_n":
            if not strided:
                return None
            flat = torch.full((M * st["ldc"],), SENT, dtype=F64)
            flat[:M * N] = c2.reshape(-1)
            c2 = flat.view(M, st["ldc"])[:, :N].clone()
        r["C2"] = c2
    elif mode == 4:
        if mutant in ("relu_mask_from_y", "neg_zero_positive", "c2_stride_n", "pad_rows_stored", "shift_sign", "scale_of_row0", "res_as_bf16"):
            return None
        x = aux.double()
        gp = gelu_grad64(x)
        if mutant == "gelu_unsigned":
            gp = torch.where(x < 0, gelu_cdf64(x.abs()) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi), gp)
        r["gp"], r["aux"] = gp, x
        r["C"] = acc * gp
    elif mode == 5:
        if mutant in ("gelu_unsigned", "c2_stride_n", "pad_rows_stored", "shift_sign", "scale_of_row0", "res_as_bf16"):
            return None
        x = aux.double()
        keep = x > 0
        if mutant == "relu_mask_from_y":
            keep = acc > 0
        elif mutant == "neg_zero_positive":
            keep = keep | ((x == 0) & torch.signbit(x))
        r["keep"] = keep
        r["C"] = torch.where(keep, acc, torch.zeros_like(acc))
    else:
        if mutant in ("relu_mask_from_y", "neg_zero_positive", "gelu_unsigned", "c2_stride_n", "aux_stride_ldc"):
            return None
        B, H, W, ws, shift = case.win
        if mutant == "shift_sign" and (ws == 0 or shift == 0):
            return None
        tok, b = window_rows(case.win, roll=1 if mutant == "shift_sign" else -1)
        sc = inp["scale"].double()[b] if inp["scale"] is not None else torch.ones(M, dtype=F64)
        if mutant == "scale_of_row0":
            if B == 1:
                return None
            sc = torch.full_like(sc, float(inp["scale"][0]))
        res = inp["res"].double()
        if mutant == "res_as_bf16":
            if case.res_bf16:
                return None
            res = inp["res"].to(BF16).double()
        keep = tok >= 0
        T = B * H * W
        y_t, A_t, sc_t = torch.zeros(T, N, dtype=F64), torch.zeros(T, N, dtype=F64), torch.zeros(T, dtype=F64)
        y_t[tok[keep]], A_t[tok[keep]], sc_t[tok[keep]] = acc[keep], A[keep], sc[keep]
        out = res + sc_t[:, None] * y_t
        if mutant == "pad_rows_stored":
            if bool(keep.all()):
                return None
            last = int((~keep).nonzero()[-1])                  # the last padding row wins the race for token 0
            out[0] = res[0] + sc[last] * acc[last]
        r.update(y_t=y_t, A_t=A_t, sc_t=sc_t, res=inp["res"].double(), out=out, stored=int(keep.sum()))
    return r


def gemm64(a, b, bias, mode, relu=False, aux=None, res=None, scale=None, win=None, res_bf16=False):
    """(ref, A, n) of one problem: the float64 value of the main output (C; out of mode 3, in token order), the same contraction over
    absolute values with |bias| added, the addend count"""
    M, K = a.shape
    case = Case("-", M, b.shape[0], K, mode, relu, int(res_bf16), win, (), 0, (0, 128, 128, 1))
    r = evaluate64(case, {"a": a, "b": b, "bias": bias, "aux": aux, "res": res, "scale": scale})
    return (r["out"], r["A_t"], r["n"]) if mode == 3 else (r["C"], r["A"], r["n"])


# ------------------------------------------------------------------ bounds
def flushable(ref, bnd):
    return bnd + (ref.abs() < BF16_MIN_NORMAL).double() * BF16_MIN_NORMAL


def y_bound(ref, A, n):
    return EB * ref.abs() + ACC_FACTOR * n * U * A * (1.0 + EB)


def c2_reference(C_got):
    """mode 2: (ref, bound) of C2 from the kernel's own C"""
    y = C_got.double()
    ref = gelu64(y)
    return ref, flushable(ref, EB * ref.abs() + G_CDF * y.abs().clamp_min(1.0) * (1.0 + EB))


def gelu_grad_bound(ref, y, e_y, gp, aux):
    inner = e_y * gp.abs() + (y.abs() + e_y) * (G_GRAD * aux.abs().clamp_min(1.0) + U * gp.abs())
    return flushable(ref, EB * ref.abs() + inner * (1.0 + EB))


def share_used(got, ref, term):
    """the largest share of an absolute term of a bound that an error needs beyond the rounding 2^-8 |ref| (0: the rounding alone explains
    every element)"""
    err = (got.double() - ref).abs()
    ok = torch.isfinite(err) & (term > 0)
    return float(((err - EB * ref.abs()) / term.clamp_min(1e-300))[ok].clamp_min(0.0).max())


def residual_bound(ref, e_y, sc, res, y, bf16_stream):
    inner = sc.abs() * e_y + 2.0 * U * (res.abs() + (sc * y).abs())
    return EB * ref.abs() + inner * (1.0 + EB) if bf16_stream else inner


def references(case, r):
    """{output: (ref, bound)} of an evaluate64 result (C2 of mode 2 is not in it: `c2_reference`)"""
    e_y = y_bound(r["y"], r["A"], r["n"])
    if case.mode <= 1 or case.mode == 2:
        return {"C": (r["C"], y_bound(r["C"], r["A"], r["n"]))}
    if case.mode == 4:
        return {"C": (r["C"], gelu_grad_bound(r["C"], r["y"], e_y, r["gp"], r["aux"]))}
    if case.mode == 5:
        return {"C": (r["C"], torch.where(r["keep"], e_y, torch.zeros_like(e_y)))}
    e_t = y_bound(r["y_t"], r["A_t"], r["n"])
    return {"out": (r["out"], residual_bound(r["out"], e_t, r["sc_t"][:, None], r["res"], r["y_t"], bool(case.res_bf16)))}


def signed_zero_ok(case, r, got):
    """the relu tails write no -0, mode 5 writes +0 bit for bit at every masked position"""
    z = got.float()
    neg0 = (z == 0) & torch.signbit(z)
    if case.mode <= 1 and case.relu:
        return not bool(neg0.any())
    if case.mode == 5:
        return bool(((z == 0) & ~neg0)[~r["keep"]].all())
    return True


def check(case, r, outs):
    """{output: worst |err| / bound} of a result {"C" | "C2" | "out": tensor on the CPU} against an evaluate64 result"""
    res = {}
    for name, (ref, bnd) in references(case, r).items():
        res[name] = worst_ratio(outs[name], ref, bnd)
        if name == "C" and not signed_zero_ok(case, r, outs[name]):
            res[name] = float("inf")
    if case.mode == 2:
        res["C2"] = worst_ratio(outs["C2"], *c2_reference(outs["C"]))
    return res


def report(form, case, outputs):
    """outputs: name -> worst ratio.  Prints `RATIO gemm <form> <case> <output>=<worst |err| / bound> ...`, then asserts."""
    print("RATIO gemm %s %s %s" % (form, case, " ".join("%s=%.3f" % kv for kv in outputs.items())))
    assert all(v <= 1.0 for v in outputs.values()), (form, case, outputs)


def all_finite_bf16():
    """the 65 280 finite bf16 bit patterns"""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return (bits - (bits >= 32768) * 65536).to(torch.int16).view(BF16)
