"""CPU: tests/_gemm_ref64.py is held to what it claims before the GPU test leans on it.

* the restatements (a b^T, bias, GELU, GELU', ReLU', the residual store) equal torch's float64 matmul / gelu / autograd;
* the window map of mode 3 (pad, roll, partition by index arithmetic) equals oracle.swin's partition / roll / crop on every case;
* fp32 CPU evaluations of the contract -- bf16 operands, fp32 accumulation of the K-tiles forward, reversed, and per split then folded,
  ONE rounding, then the tail with g_gelu_terms restated in fp32 -- stay inside every bound on every case and input kind (elements
  that are exactly equal count as ratio 0); every compared reference is 0 or a normal bf16 magnitude;
* every mutant leaves its bound on every case where it is defined, and is defined somewhere;
* G and G' are measured over all 65 280 finite bf16 inputs against float64 erfc and the module's constants are twice the figures;
* the plan column of every table row is what gemm_plan.h decides (tests/native/gemm_plan_check.cpp, line kind `tab`).
The 32776 x 576 rows run here in the `ordinary` kind only (each is 19 M float64 elements per tensor); the GPU test runs every kind."""
import math
import os
import shutil
import subprocess

import pytest
import torch

import _gemm_ref64 as R
from oracle import swin as OSW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


def numeric_key(c):
    return (c.M, c.N, c.K, c.mode, c.relu, c.res_bf16, c.win, c.plan[3])


def unique(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


def host_kinds(case):
    return ("ordinary",) if (case.M > 30000 and case.N > 192) else R.kinds_of(case)


# ------------------------------------------------------------------ g_gelu_terms in fp32
def fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()          # the product is exact in float64


def c32(v):
    return torch.tensor(v, dtype=F32)


def gelu_terms32(x):
    """csrc/gemm_common.h g_gelu_terms, operation by operation in fp32 (the reciprocal and the exponential correctly rounded here)"""
    z = x.abs() * c32(0.70710678118654752440)
    t = 1.0 / fma32(c32(0.3275911), z, c32(1.0))
    e = torch.exp(-z * z)
    p = c32(1.061405429).expand_as(x)
    for coef in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        p = fma32(p, t, c32(coef))
    h = 0.5 * (p * t) * e
    return torch.where(x < 0, h, 1.0 - h), e * c32(0.39894228040143267794)


def test_gelu_constants_are_twice_the_measured_error_of_the_fp32_polynomial():
    x = R.all_finite_bf16()
    assert x.numel() == 65280 and bool(torch.isfinite(x.float()).all())
    xf, xd = x.float(), x.double()
    cdf, pdf = gelu_terms32(xf)
    g = float((cdf.double() - R.gelu_cdf64(xd)).abs().max())
    gp = float(((cdf + xf * pdf).double() - R.gelu_grad64(xd)).abs().max())
    print("MEASURED G=%.4g G'=%.4g" % (g, gp))
    assert abs(g / R.MEASURED_G - 1.0) < 0.01 and abs(gp / R.MEASURED_GP - 1.0) < 0.01, (g, gp)
    assert R.G_CDF == 2 * R.MEASURED_G and R.G_GRAD == 2 * R.MEASURED_GP
    # the fp32 polynomial itself inside the sweep's bounds: GELU through mode 2, GELU' through mode 4 with y = 1
    ref, bnd = R.c2_reference(x)
    assert R.worst_ratio((xf * cdf).to(BF16), ref, bnd) <= 1.0
    gref = R.gelu_grad64(xd)
    one, zero = torch.ones_like(xd), torch.zeros_like(xd)
    gb = R.gelu_grad_bound(gref, one, zero, gref, xd)
    assert R.worst_ratio((cdf + xf * pdf).to(BF16), gref, gb) <= 1.0
    print("USED host G=%.4f G'=%.4f" % (R.share_used((xf * cdf).to(BF16), ref, R.G_CDF * xd.abs().clamp_min(1.0)),
                                        R.share_used((cdf + xf * pdf).to(BF16), gref, R.G_GRAD * xd.abs().clamp_min(1.0))))


# ------------------------------------------------------------------ the restatements against torch
def test_restatements_equal_torch_float64():
    g = torch.Generator().manual_seed(3)
    M, N, K = 24, 16, 40
    a, b, bias = torch.randn(M, K, generator=g).to(BF16), torch.randn(N, K, generator=g).to(BF16), torch.randn(N, generator=g).to(BF16)
    lin = torch.nn.functional.linear(a.double(), b.double(), bias.double())
    ref, A, n = R.gemm64(a, b, bias, 1)
    assert torch.allclose(ref, lin, rtol=1e-13, atol=1e-13) and n == K + 1
    assert torch.allclose(A, a.double().abs() @ b.double().abs().t() + bias.double().abs(), rtol=1e-13)
    ref0, _, n0 = R.gemm64(a, b, None, 0)
    assert torch.allclose(ref0, a.double() @ b.double().t(), rtol=1e-13, atol=1e-13) and n0 == K
    assert torch.equal(R.gemm64(a, b, bias, 1, relu=True)[0], torch.relu(ref))
    x = torch.linspace(-12.0, 12.0, 4801, dtype=F64).requires_grad_(True)
    gel = torch.nn.functional.gelu(x)
    gel.sum().backward()
    # torch evaluates x (1 + erf) / 2, which cancels to zero down the negative tail: an absolute 2e-15 there; erfc keeps the tail
    assert torch.allclose(R.gelu64(x.detach()), gel.detach(), rtol=1e-12, atol=2e-15)
    assert torch.allclose(R.gelu_grad64(x.detach()), x.grad, rtol=1e-10, atol=2e-15)
    assert float(R.gelu64(torch.tensor(-12.0, dtype=F64))) < 0.0
    # mode 4 / 5: autograd through the activation of the product
    aux = (torch.randn(M, N, generator=g) * 2).to(BF16)
    pre = aux.double().requires_grad_(True)
    torch.nn.functional.gelu(pre).backward(ref0)
    assert torch.allclose(R.gemm64(a, b, None, 4, aux=aux)[0], pre.grad, rtol=1e-10, atol=1e-14)
    act = R.plant_zeros(torch.relu(torch.randn(M, N, generator=g)), g).to(BF16)
    assert torch.equal(R.gemm64(a, b, None, 5, aux=act)[0], ref0 * (act.double() > 0))
    res, scale = torch.randn(M, N, generator=g), torch.tensor([1.0 / 0.7, 0.0])
    out, At, _ = R.gemm64(a, b, bias, 3, res=res, scale=scale, win=(2, 3, 4, 0, 0))
    want = res.double() + scale.double().repeat_interleave(12)[:, None] * lin
    assert torch.allclose(out, want, rtol=1e-13, atol=1e-13) and torch.equal(At, A)


@pytest.mark.parametrize("win", sorted({c.win for c in R.CASES if c.win} | {(3, 10, 13, 7, 3), (2, 30, 26, -12, 6)}), ids=str)
def test_window_map_equals_the_oracles_partition_roll_crop(win):
    B, H, W, ws, shift = win
    tok, b = R.window_rows(win)
    T = B * H * W
    if ws == 0:
        assert torch.equal(tok, torch.arange(T)) and torch.equal(b, torch.arange(T) // (H * W))
        return
    a = abs(ws)
    Hp, Wp = -(-H // a) * a, -(-W // a) * a
    ids = torch.arange(T, dtype=F64).reshape(B, H, W, 1)
    x = torch.nn.functional.pad(ids, (0, 0, 0, Wp - W, 0, Hp - H), value=-1.0)
    rows = OSW.partition(torch.roll(x, (-shift, -shift), (1, 2)), a).reshape(-1).long()
    assert rows.numel() == B * Hp * Wp
    if ws < 0:
        rows = rows[rows >= 0]
    assert torch.equal(tok, rows)
    real = tok >= 0
    assert int(real.sum()) == T and torch.equal(tok[real].sort().values, torch.arange(T)) and torch.equal(b[real], tok[real] // (H * W))
    # the way back, as the Swin block does it: window_reverse, roll back, crop
    if ws > 0:
        y = torch.randn(tok.numel(), 3, dtype=F64)
        back = torch.roll(OSW.unpartition(y.reshape(-1, a * a, 3), a, Hp, Wp), (shift, shift), (1, 2))[:, :H, :W].reshape(T, 3)
        mine = torch.zeros(T, 3, dtype=F64)
        mine[tok[real]] = y[real]
        assert torch.equal(mine, back)


def test_gemm_lw_work_lists_reach_what_the_table_says():
    depth = {}
    for c in R.CASES:
        if c.row in ("I", "I'"):
            form, bm, bn, S = c.plan
            items = -(-c.M // bm) * -(-c.N // bn) * S
            wgx = min((items + 7) // 8, 32 - c.reserved // 8)
            later = R.lw_stale_items(c)
            assert len(later) == items - 8 * wgx or items % 8, (c, len(later))
            depth[(c.row, c.reserved)] = -(-((items + 7) // 8) // wgx)
    assert depth == {("I", 0): 2, ("I", 128): 3, ("I'", 0): 1, ("I'", 128): 2}, depth


# ------------------------------------------------------------------ fp32 evaluations of the contract
def accumulate32(case, inp, order):
    a, b = inp["a"].float(), inp["b"].float()
    nt = R.k_tiles(case.K)

    def part(t):
        return a[:, t * R.BK:(t + 1) * R.BK] @ b[:, t * R.BK:(t + 1) * R.BK].t()
    if order == "split":
        rng = R.split_ranges(case) if case.plan[3] > 1 else [(t, min(2, nt - t)) for t in range(0, nt, 2)]
        slabs = []
        for t0, n in rng:
            s = part(t0)
            for t in range(t0 + 1, t0 + n):
                s = s + part(t)
            slabs.append(s)
        acc = torch.zeros_like(slabs[0])
        for s in slabs:
            acc = acc + s
        return acc
    ts = range(nt) if order == "forward" else range(nt - 1, -1, -1)
    acc = torch.zeros(case.M, case.N, dtype=F32)
    for t in ts:
        acc = acc + part(t)
    return acc


def evaluate32(case, inp, order):
    """the contract in fp32: one rounding of acc + bias, then the tail of g_epi_finish on the rounded y"""
    acc = accumulate32(case, inp, order)
    if case.mode in (1, 2, 3):
        acc = acc + inp["bias"].float()
    y = acc.to(BF16)
    yf = y.float()
    if case.mode <= 1:
        return {"C": torch.where(yf > 0, y, torch.zeros_like(y)) if case.relu else y}
    if case.mode == 2:
        return {"C": y, "C2": (yf * gelu_terms32(yf)[0]).to(BF16)}
    if case.mode == 4:
        x = inp["aux"].float()
        cdf, pdf = gelu_terms32(x)
        return {"C": (yf * (cdf + x * pdf)).to(BF16)}
    if case.mode == 5:
        return {"C": torch.where(inp["aux"].float() > 0, y, torch.zeros_like(y))}
    tok, b = R.window_rows(case.win)
    keep = tok >= 0
    out = inp["res"].float().clone()
    sc = inp["scale"][b[keep]][:, None] if inp["scale"] is not None else torch.ones(1, 1)
    out[tok[keep]] = out[tok[keep]] + sc * yf[keep]
    return {"out": out.to(inp["res"].dtype)}


@pytest.mark.parametrize("case", unique(R.CASES, numeric_key), ids=R.case_id)
def test_fp32_contract_inside_every_bound(case):
    for kind in host_kinds(case):
        inp = R.inputs(case, kind)
        r = R.evaluate64(case, inp, pre=R.contraction(case, kind))
        for name, (ref, bnd) in R.references(case, r).items():
            assert R.in_bf16_normal_range(ref), (kind, name)
            assert bool((bnd >= 0).all())
        for order in ("forward", "reversed", "split"):
            outs = evaluate32(case, inp, order)
            got = R.check(case, r, outs)
            assert all(v <= 1.0 for v in got.values()), (R.case_id(case), kind, order, got)
            if case.mode == 2:             # GELU below the normal range: only where the pre-activation is far down the negative tail
                ref2 = R.gelu64(outs["C"].double())
                low = (ref2 != 0) & (ref2.abs() < R.BF16_MIN_NORMAL)
                assert bool((outs["C"].double()[low] < -13.0).all())


def test_scaled_kind_puts_every_row_and_column_at_its_own_scale():
    case = next(c for c in R.CASES if c.row == "S" and c.mode == 0)
    r = R.evaluate64(case, R.inputs(case, "scaled"))
    rows, cols = r["A"].amax(1), r["A"].amax(0)
    assert float(rows.max() / rows.min()) > 2.0 ** 35 and float(cols.max() / cols.min()) > 2.0 ** 25
    assert R.in_bf16_normal_range(r["C"])
    c = next(c for c in R.CASES if c.row == "W" and c.mode == 0)
    rc = R.evaluate64(c, R.inputs(c, "cancelling"))
    assert float((rc["A"] / rc["C"].abs().clamp_min(1e-300)).median()) > 10.0          # A >> |ref|


# ------------------------------------------------------------------ mutants
STRIDE_MUTANTS = ("tail_unmasked", "c2_stride_n", "aux_stride_ldc")
ZERO_MUTANTS = ("neg_zero_positive", "relu_mask_from_y")


def mutant_key(c):
    return numeric_key(c) + (c.plan, c.reserved if c.plan[0] == 1 else 0)


def differs(a, b):
    return not bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


MUTANT_CASES = [c for c in unique(R.CASES, mutant_key) if not (c.M > 30000 and c.N > 192)]


@pytest.mark.parametrize("case", MUTANT_CASES, ids=R.case_id)
def test_every_mutant_leaves_its_bound(case):
    defined = []
    for kind in (("ordinary", "signed_zero") if len(R.kinds_of(case)) == 4 else ("ordinary",)):
        inp, pre = R.inputs(case, kind), R.contraction(case, kind)
        r = R.evaluate64(case, inp, pre=pre)
        for name in R.MUTANTS:
            if kind == "signed_zero" and name not in ZERO_MUTANTS:
                continue
            rm = R.evaluate64(case, inp, mutant=name, strided=name in STRIDE_MUTANTS, pre=pre)
            if rm is None:
                continue
            outs = {k: rm[k] for k in ("C", "C2", "out") if k in rm}
            if not any(differs(outs[k], r[k]) for k in outs):
                continue
            got = R.check(case, r, outs)
            assert max(got.values()) > 1.0, (R.case_id(case), kind, name, got)
            defined.append(name)
    assert "chunk8" in defined, R.case_id(case)


def test_every_mutant_is_defined_on_some_row():
    """which rows of the table can see each mutant at all (the parametrised test above shows that they then do)"""
    rows = {name: set() for name in R.MUTANTS}
    for case in MUTANT_CASES:
        if case.M > 2000:
            continue
        inp = R.inputs(case, "ordinary")
        r = R.evaluate64(case, inp)
        for name in R.MUTANTS:
            rm = R.evaluate64(case, inp, mutant=name, strided=name in STRIDE_MUTANTS)
            if rm is not None and any(differs(rm[k], r[k]) for k in ("C", "C2", "out") if k in rm):
                rows[name].add(case.row)
    assert all(rows.values()), {k: v for k, v in rows.items() if not v}
    assert rows["second_item_stale"] == {"I", "I'"} and {"S", "I", "W'"} <= rows["split_tail"] and "S" in rows["pad_rows_stored"]
    assert {"T", "W", "S"} <= rows["tail_unmasked"] & rows["c2_stride_n"] and {"T", "W", "S", "E"} <= rows["aux_stride_ldc"]


# ------------------------------------------------------------------ the plan column
def plan_lines():
    lines = ["pin 1024 1024 12544 1 0 %d -1 0 0" % (64 << 20)]       # the checker insists on its own split-K pin in every case file
    for c in R.CASES:
        k = dict(c.knobs)
        lines.append("tab %d %d %d %d %d %d %d  %d %d %d %d %d  %d  %d %d %d %d" % (
            c.M, c.N, c.K, c.mode, c.res_bf16, int(c.relu), R.WS_BYTES, k.get("gemm_lw", -1), k.get("gemm_2wg", -1), k.get("gemm_tile", 0),
            k.get("gemm_splitk", 0), k.get("gemm_k192", -1), c.reserved, *c.plan))
    return lines


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_table_plans_are_what_gemm_plan_h_decides(tmp_path):
    exe, cases = str(tmp_path / "gemm_plan_check"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "gemm_plan_check.cpp")])
    lines = plan_lines()
    assert len(lines) == 1 + len(R.CASES)
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) == len(lines)


def test_table_reaches_every_form_tile_tail_and_split():
    plans = {c.plan for c in R.CASES}
    assert {p[0] for p in plans} == {0, 1, 2, 3}
    for lw in (0, 1):
        assert {p[1:3] for p in plans if p[0] == lw} >= set(R.TILES)
        assert {p[3] for p in plans if p[0] == lw} >= {1, 2, 3, 4, 5, 18}
    two = {(c.mode, c.res_bf16) for c in R.CASES if c.plan[0] == 2}
    assert two >= {(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (4, 0), (5, 0)}
    assert {c.mode for c in R.CASES if c.plan[0] == 3} == {0, 1, 2, 3, 4}
    for c in R.CASES:
        st = R.strides(c, True)
        assert all(v % 8 == 0 for v in st.values()) and c.M == (R.win_rows(c.win) if c.win else c.M)
        assert c.M * st["lda"] * 2 < 2 ** 31 and c.N * st["ldb"] * 2 < 2 ** 31
        assert c.plan[3] == 1 or c.plan[3] * c.M * c.N * 4 <= R.WS_BYTES
    orders = {(c.win[3] > 0) - (c.win[3] < 0) for c in R.CASES if c.win}
    assert orders == {-1, 0, 1} and math.prod(R.TILES[0]) == 256 * 192
