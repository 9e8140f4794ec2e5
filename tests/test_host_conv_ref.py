"""CPU: the float64 restatements, bounds, case tables and mutants of tests/_conv_ref64.py, which tests/test_gpu_conv_numerics.py holds the
convolution kernels to.

* the restatements equal torch.nn.functional.conv2d / conv_transpose2d and their autograd in float64 to 1e-12 of the tensor's scale, on
  every case; pad_layout has the row count of dgx_conv3x3_pad_rows and im2col / col2im are the adjoint pair of the stride;
* an fp32 CPU evaluation of the contract (bf16 operands, fp32 accumulation, one rounding) is inside every bound on every case, in three
  orders: torch's own, tap by tap, and slab by slab with the case's K-tiles per split (bias in the fold) / rows per M-slab;
* every mutant puts at least one element outside its bound on every case on which it is defined (= differs from the restatement at all),
  judged through its worst element;
* the implicit-GEMM plans of the table are what gemm_plan.h decides (tests/native/gemm_plan_check.cpp, with the 64 MB workspace and with
  none, default form and gemm_lw = 0), and the restated weight-gradient plan (csrc/wgrad_plan.h) reproduces every weight-gradient row."""
import functools
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import _conv_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


@functools.lru_cache(maxsize=None)
def inputs(geom, kind):
    return R.make_inputs(kind, geom, R.seed_of(geom, kind))


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def rel(got, ref):
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def fwd_plan(geom, direction="fwd", ws=R.WS_BYTES):
    N, H, W, Cin, Cout = geom
    K, Ncol = (9 * Cin, Cout) if direction == "fwd" else (9 * Cout, Cin)
    return R.gemm_plan(N * H * W, Ncol, K, ws)


ALL_WGRAD_GEOMS = list(R.WGRAD_ROWS)


# ------------------------------------------------------------------ restatements = torch float64
@pytest.mark.parametrize("geom", R.GEOMS, ids=str)
def test_forward_and_input_gradient_equal_torch_float64(geom):
    for kind in R.INPUT_KINDS:
        inp = inputs(geom, kind)
        for relu in (False, True):
            x = nchw(inp["x"].double()).requires_grad_(True)
            w = nchw(inp["w"].double())
            t = F.conv2d(x, w, inp["bias"].double(), padding=1)
            t = torch.relu(t) if relu else t
            ref, A, n = R.conv_fwd64(inp["x"], inp["w"], inp["bias"], relu)
            assert n == 9 * geom[3] + 1 and bool((A >= ref.abs() * (1 - 1e-12)).all())
            assert rel(ref, nhwc(t.detach())) <= 1e-12, (geom, kind, relu)
            ysave = ref.to(BF16)            # any saved activation does: the mask is y > 0 of what the backward is handed
            t.backward(nchw(inp["dy"].double() * (ysave.float() > 0) if relu else inp["dy"].double()))
            dx, Ad, nd = R.conv_dgrad64(inp["dy"], inp["w"], ysave, relu)
            assert nd == 9 * (-(-geom[4] // 64) * 64)
            assert rel(dx, nhwc(x.grad)) <= 1e-12, (geom, kind, relu)


@pytest.mark.parametrize("geom", ALL_WGRAD_GEOMS, ids=str)
def test_weight_and_bias_gradient_equal_torch_float64(geom):
    N, H, W, Cin, Cout = geom
    for kind in R.INPUT_KINDS:
        inp = inputs(geom, kind)
        w = nchw(inp["w"].double()).contiguous().requires_grad_(True)
        b = inp["bias"].double().requires_grad_(True)
        g = R.relu_mask(inp["dy"], inp["ysave"] if kind == "postrelu" else None)
        F.conv2d(nchw(inp["x"].double()), w, b, padding=1).backward(nchw(g.double()))
        for beta in (0.0, 1.0):
            (dW, db), (Aw, Ab), n = R.conv_wgrad64(g, inp["x"], inp["g0"], beta)
            assert n == N * (H + 2) * (W + 2) + (beta != 0)
            assert rel(dW, nhwc(w.grad) + beta * inp["g0"][0].double()) <= 1e-12, (geom, kind, beta)
            assert rel(db, b.grad + beta * inp["g0"][1].double()) <= 1e-12, (geom, kind, beta)


@pytest.mark.parametrize("shape", R.COL_SHAPES + [(2, 16, 13, 18), (1, 7, 5, 64)], ids=str)
@pytest.mark.parametrize("stride", [1, 2])
def test_stride_forms_equal_torch_float64(shape, stride):
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, H, W, C, generator=gen).to(BF16)
    Co = 8
    w = (torch.randn(Co, 3, 3, C, generator=gen) * 0.05).to(BF16)
    b = torch.randn(Co, generator=gen).to(BF16)
    xt = nchw(x.double()).requires_grad_(True)
    wt, bt = nchw(w.double()).contiguous().requires_grad_(True), b.double().requires_grad_(True)
    t = F.conv2d(xt, wt, bt, padding=1, stride=stride)
    ref, A, n = R.conv_fwd64(x, w, b, False, stride=stride)
    Ho, Wo = R.out_hw(H, W, stride)
    assert ref.shape == (N, Ho, Wo, Co) == tuple(nhwc(t).shape) and rel(ref, nhwc(t.detach())) <= 1e-12
    # im2col is the matrix whose product with the (Cout, 9 C) weight is the convolution, exactly the unfold of the zero-padded image
    col = R.im2col64(x, stride)
    assert col.dtype == BF16 and col.shape == (N * Ho * Wo, 9 * C)
    unf = F.unfold(nchw(x.double()), 3, padding=1, stride=stride).view(N, C, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(N * Ho * Wo, 9 * C)
    assert torch.equal(col.double(), unf)
    # col2im is its adjoint: the input gradient of the convolution from dcol = dy w
    dy = torch.randn(N, Ho, Wo, Co, generator=gen).to(BF16)
    t.backward(nchw(dy.double()))
    dx, A1, S1, n1, cnt = R.conv_dgrad_cols64(dy, w, N, H, W, stride)
    assert rel(dx, nhwc(xt.grad)) <= 1e-12 and n1 == Co and float(cnt.max()) <= 9 and bool((S1 >= dx.abs() * (1 - 1e-12)).all())
    (dW, db), _, nw = R.conv_wgrad_cols64(dy, x, stride)
    assert rel(dW, nhwc(wt.grad)) <= 1e-12 and rel(db, bt.grad) <= 1e-12 and nw == N * Ho * Wo
    dcol = torch.randn(N * Ho * Wo, 9 * C, generator=gen)
    got, _, _ = R.col2im64(dcol, N, H, W, C, stride)
    fold = F.fold(dcol.double().view(N, Ho * Wo, 9, C).permute(0, 3, 2, 1).reshape(N, C * 9, Ho * Wo), (H, W), 3, padding=1, stride=stride)
    assert rel(got, nhwc(fold)) <= 1e-12


def test_pad_layout_rows_and_content():
    for N, H, W, C in R.PAD_SHAPES + [g[:3] + (8,) for g in R.GEOMS]:
        x = torch.arange(1, N * H * W * C + 1, dtype=F32).view(N, H, W, C)
        xp = R.pad_layout(x)
        assert xp.shape == (R.pad_rows(N, H, W), C) == (N * (H + 2) * (W + 2) + 2 * (W + 3), C)
        assert float(xp.sum()) == float(x.sum()) and int((xp != 0).sum()) == x.numel()
        grid = xp[W + 3:W + 3 + N * (H + 2) * (W + 2)].view(N, H + 2, W + 2, C)
        assert torch.equal(grid[:, 1:H + 1, 1:W + 1], x)
        # every tap of every output pixel is a constant row shift inside the allocation (gemm_common.h g_a_voff / g_a_soff)
        wp = W + 2
        n, y, xx = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), indexing="ij")
        arow = ((n * (H + 2) + y + 1) * wp + xx + 1).reshape(-1)
        col = R.im2col64(x, 1)
        for t in range(9):
            assert torch.equal(xp[arow + (t // 3) * wp + t % 3], col[:, t * C:(t + 1) * C])


@pytest.mark.parametrize("case", [(3, 64, 7, 9, 32), (1, 8, 1, 1, 8)], ids=str)
@pytest.mark.parametrize("relu", [False, True])
def test_deconv2x2_equals_torch_float64(case, relu):
    N, Cin, H, W, Cout = case
    gen = torch.Generator().manual_seed(8 + Cin)
    x = torch.randn(N, H, W, Cin, generator=gen).to(BF16)
    w = (torch.randn(Cin, Cout, 2, 2, generator=gen) * 0.1).to(BF16)
    b = torch.randn(Cout, generator=gen).to(BF16)
    dy = torch.randn(N, 2 * H, 2 * W, Cout, generator=gen).to(BF16)
    xt, wt, bt = nchw(x.double()).requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    t = F.conv_transpose2d(xt, wt, bt, stride=2)
    t = torch.relu(t) if relu else t
    y0 = R.deconv2x2_64(x, w, b, relu)["y"][0]
    assert rel(y0, nhwc(t.detach())) <= 1e-12
    ysave = y0.to(BF16)
    out = R.deconv2x2_64(x, w, b, relu, dy=dy, y_kernel=ysave)
    t.backward(nchw(R.relu_mask(dy.double(), ysave if relu else None)))
    assert rel(out["dx"][0], nhwc(xt.grad)) <= 1e-12 and rel(out["dw"][0], wt.grad) <= 1e-12 and rel(out["db"][0], bt.grad) <= 1e-12
    assert (out["y"][2], out["dx"][2], out["dw"][2], out["db"][2]) == (Cin + 1, 4 * Cout, N * H * W, 4 * N * H * W)
    # the shuffles are inverse index maps
    y2 = torch.arange(N * H * W * 4 * Cout, dtype=F64).view(N * H * W, 4 * Cout)
    assert torch.equal(R.deconv_unshuffle(R.deconv_shuffle(y2, N, H, W, Cout).contiguous(), N, H, W, Cout), y2)


# ------------------------------------------------------------------ the contract in fp32, three orders
def fwd_f32(x, w, bias, relu, order, plan):
    """bf16 operands, fp32 accumulation, one rounding to bf16"""
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    xf, wf = x.float(), w.float()
    b = bias.float() if bias is not None else None
    if order == "torch":
        acc = nhwc(F.conv2d(nchw(xf), nchw(wf), b, padding=1)).reshape(-1, Cout)
    else:
        def tile(kt):
            tap, blk = divmod(kt, Cin // 64)
            rows = R._tap_rows(xf.reshape(-1, Cin), N, H, W, 1, tap // 3, tap % 3, None, H, W)
            return rows[:, 64 * blk:64 * blk + 64] @ wf[:, tap // 3, tap % 3, 64 * blk:64 * blk + 64].t()
        nt = 9 * Cin // 64
        kps = Cin // 64 if order == "tap" else plan[3]
        acc = torch.zeros(N * H * W, Cout)
        for k0 in range(0, nt, kps):                # one tap / one split-K slab at a time, then the fold in slab order
            slab = torch.zeros(N * H * W, Cout)
            for kt in range(k0, min(k0 + kps, nt)):
                slab += tile(kt)
            acc += slab
        if b is not None:
            acc = acc + b
    if relu:
        acc = acc.clamp_min(0)
    return acc.to(BF16).view(N, H, W, Cout)


@pytest.mark.parametrize("geom", R.GEOMS, ids=str)
def test_fp32_contract_inside_every_bound_forward_and_input_gradient(geom):
    worst = 0.0
    for kind in R.INPUT_KINDS:
        inp = inputs(geom, kind)
        for bias, relu in ((inp["bias"], True), (None, False), (inp["bias"], False)):
            ref, A, n = R.conv_fwd64(inp["x"], inp["w"], bias, relu)
            assert R.in_bf16_normal_range(ref), (geom, kind)
            bnd = R.bf16_bound(ref, A, n)
            for order in ("torch", "tap", "slab"):
                r = R.worst_ratio(fwd_f32(inp["x"], inp["w"], bias, relu, order, fwd_plan(geom)), ref, bnd)
                assert r <= 1.0, (geom, kind, relu, order, r)
                worst = max(worst, r)
        if "dgrad" in R.GEMM_ROWS[geom]:
            for relu in (False, True):
                ref, A, n = R.conv_dgrad64(inp["dy"], inp["w"], inp["ysave"], relu)
                assert R.in_bf16_normal_range(ref), (geom, kind)
                g = R.relu_mask(inp["dy"], inp["ysave"] if relu else None)
                for order in ("torch", "tap", "slab"):
                    r = R.worst_ratio(fwd_f32(g, R.flip_twin(inp["w"]), None, False, order, fwd_plan(geom, "dgrad")), ref, R.bf16_bound(ref, A, n))
                    assert r <= 1.0, (geom, kind, relu, order, r)
                    worst = max(worst, r)
    print("RATIO host fp32 forward/dgrad %s worst=%.3f" % (geom, worst))


def wgrad_f32(dy, x, g0, beta, order, plan):
    N, H, W, Cout = dy.shape
    Cin, wp, Mp = x.shape[3], W + 2, N * (H + 2) * (W + 2)
    if order == "torch":
        dW = nhwc(torch.nn.grad.conv2d_weight(nchw(x.float()), (Cout, Cin, 3, 3), nchw(dy.float()), padding=1)).contiguous()
        db = dy.float().sum((0, 1, 2))
    else:
        dyp, xp = R.pad_grid(dy.float()).reshape(Mp, Cout), R.pad_layout(x.float())
        slab = Mp if order == "tap" else plan[1]
        dW, db = torch.zeros(Cout, 3, 3, Cin), torch.zeros(Cout)
        for m0 in range(0, Mp, slab):               # the partial sums of the M-slabs, folded in slab order
            m1 = min(Mp, m0 + slab)
            for t in range(9):
                s = (t // 3) * wp + t % 3
                dW[:, t // 3, t % 3] += dyp[m0:m1].t() @ xp[s + m0:s + m1]
            db += dyp[m0:m1].sum(0)
    if beta != 0.0:
        dW, db = dW + beta * g0[0], db + beta * g0[1]
    return dW, db


@pytest.mark.parametrize("geom", ALL_WGRAD_GEOMS, ids=str)
def test_fp32_contract_inside_every_bound_weight_gradient(geom):
    S, slab, _, _ = R.wgrad_plan(*geom)
    worst = 0.0
    for kind in R.INPUT_KINDS:
        inp = inputs(geom, kind)
        g = R.relu_mask(inp["dy"], inp["ysave"] if kind == "postrelu" else None)
        for beta in (0.0, 1.0):
            (dW, db), (Aw, Ab), n = R.conv_wgrad64(g, inp["x"], inp["g0"], beta)
            assert R.in_bf16_normal_range(dW) and R.in_bf16_normal_range(db), (geom, kind)
            for order in ("torch", "tap", "slab"):
                gw, gb = wgrad_f32(g, inp["x"], inp["g0"], beta, order, (S, slab))
                r = max(R.worst_ratio(gw, dW, R.f32_bound(dW, Aw, n)), R.worst_ratio(gb, db, R.f32_bound(db, Ab, n)))
                assert r <= 1.0, (geom, kind, beta, order, r)
                worst = max(worst, r)
    print("RATIO host fp32 wgrad %s worst=%.3f" % (geom, worst))


def test_fp32_contract_inside_every_bound_column_form_and_deconv():
    for N, H, W, C in R.COL_SHAPES:
        gen = torch.Generator().manual_seed(N + H + W + C)
        for stride in (1, 2):
            Ho, Wo = R.out_hw(H, W, stride)
            dcol = torch.randn(N * Ho * Wo, 9 * C, generator=gen)
            for dt in (BF16, F32):
                d = dcol.to(dt)
                ref, A, cnt = R.col2im64(d, N, H, W, C, stride)
                got = nhwc(F.fold(d.float().view(N, Ho * Wo, 9, C).permute(0, 3, 2, 1).reshape(N, C * 9, Ho * Wo), (H, W), 3, padding=1, stride=stride))
                bnd = R.bf16_bound(ref, A, cnt) if dt == BF16 else R.f32_bound(ref, A, cnt)
                assert R.worst_ratio(got.to(dt), ref, bnd) <= 1.0, (N, H, W, C, stride, dt)
    # the two-rounding input gradient of the stride-2 Python path
    for N, C, H, W in ((2, 16, 13, 18), (1, 256, 7, 5)):
        gen = torch.Generator().manual_seed(C)
        Ho, Wo = R.out_hw(H, W, 2)
        w = (torch.randn(24, 3, 3, C, generator=gen) * 0.05).to(BF16)
        dy = torch.randn(N, Ho, Wo, 24, generator=gen).to(BF16)
        ref, A1, S1, n1, cnt = R.conv_dgrad_cols64(dy, w, N, H, W, 2)
        dcol = (dy.float().reshape(-1, 24) @ w.float().reshape(24, -1)).to(BF16)
        got = nhwc(F.fold(dcol.float().view(N, Ho * Wo, 9, C).permute(0, 3, 2, 1).reshape(N, C * 9, Ho * Wo), (H, W), 3, padding=1, stride=2)).to(BF16)
        assert R.worst_ratio(got, ref, R.two_rounding_bound(ref, A1, n1, S1, cnt)) <= 1.0
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3, 7, 9, 64, generator=gen).to(BF16)
    w = (torch.randn(64, 32, 2, 2, generator=gen) * 0.1).to(BF16)
    b = torch.randn(32, generator=gen).to(BF16)
    ref, A, n = R.deconv2x2_64(x, w, b, True)["y"]
    got = torch.relu(F.conv_transpose2d(nchw(x.float()), w.float(), b.float(), stride=2)).to(BF16)
    assert R.worst_ratio(nhwc(got), ref, R.bf16_bound(ref, A, n)) <= 1.0


# ------------------------------------------------------------------ mutants
def defined(mut, ref):
    return not torch.equal(mut, ref)


@pytest.mark.parametrize("geom", R.GEOMS, ids=str)
def test_every_forward_mutant_leaves_its_bound(geom):
    plan = fwd_plan(geom)
    seen = {}
    for kind in R.INPUT_KINDS:
        inp = inputs(geom, kind)
        for relu in ((True, False) if kind == "ordinary" else (True,)):
            ref, A, n = R.conv_fwd64(inp["x"], inp["w"], inp["bias"], relu)
            bnd = R.bf16_bound(ref, A, n)
            for m in R.FWD_MUTANTS:
                mut = R.conv_fwd64(inp["x"], inp["w"], inp["bias"], relu, mutant=m, plan=plan)[0]
                if defined(mut, ref):
                    r = R.worst_ratio(mut, ref, bnd)
                    assert r > 1.0, (geom, kind, relu, m, r)
                    seen[m] = min(seen.get(m, float("inf")), r)
        if "dgrad" in R.GEMM_ROWS[geom] and kind != "cancelling":
            dplan = fwd_plan(geom, "dgrad")
            ref, A, n = R.conv_dgrad64(inp["dy"], inp["w"], inp["ysave"], True)
            for m in R.FWD_MUTANTS:
                mut = R.conv_dgrad64(inp["dy"], inp["w"], inp["ysave"], True, mutant=m, plan=dplan)[0]
                if defined(mut, ref):
                    r = R.worst_ratio(mut, ref, R.bf16_bound(ref, A, n))
                    assert r > 1.0, (geom, kind, "dgrad", m, r)
                    seen["dgrad." + m] = min(seen.get("dgrad." + m, float("inf")), r)
    print("RATIO host mutants %s %s" % (geom, " ".join("%s=%.3g" % kv for kv in seen.items())))
    N, H, W, Cin, Cout = geom
    M = N * H * W
    want = {"row_wrap": N * H > 1, "image_wrap": N > 1, "taps_transposed": H * W > 1, "taps_flipped": H * W > 1, "corner_tap": True,
            "chunk8": H > 1 and W > 1, "bias_per_split": plan[2] > 1, "relu_first": True, "row_tail": M % plan[0] != 0, "col_tail": Cout % 256 != 0}
    assert {m for m, v in want.items() if v} <= set(seen) and not {m for m, v in want.items() if not v} & set(seen), (geom, sorted(seen))
    if geom == R.FORCED_GEOM:
        assert set(R.FWD_MUTANTS) <= set(seen)


@pytest.mark.parametrize("geom", ALL_WGRAD_GEOMS, ids=str)
def test_every_weight_gradient_mutant_leaves_its_bound(geom):
    S, slab, _, _ = R.wgrad_plan(*geom)
    seen = {}
    for kind in (R.INPUT_KINDS if geom[1] <= 20 else ("ordinary",)):
        inp = inputs(geom, kind)
        g = R.relu_mask(inp["dy"], inp["ysave"] if kind == "postrelu" else None)
        for beta in (0.0, 1.0):
            (dW, db), (Aw, Ab), n = R.conv_wgrad64(g, inp["x"], inp["g0"], beta)
            bw, bb = R.f32_bound(dW, Aw, n), R.f32_bound(db, Ab, n)
            for m in R.WGRAD_MUTANTS:
                (mW, mb), _, _ = R.conv_wgrad64(g, inp["x"], inp["g0"], beta, mutant=m, plan=(S, slab))
                if defined(mW, dW) or defined(mb, db):
                    r = max(R.worst_ratio(mW, dW, bw), R.worst_ratio(mb, db, bb))
                    assert r > 1.0, (geom, kind, beta, m, r)
                    seen[m] = min(seen.get(m, float("inf")), r)
    print("RATIO host mutants wgrad %s %s" % (geom, " ".join("%s=%.3g" % kv for kv in seen.items())))
    N, H, W, Cin, Cout = geom
    # the grid ends with W + 3 border positions: a dropped tail of rows is a different function only when it is longer than that
    Mp = N * (H + 2) * (W + 2)
    want = {"border_counted": True, "last_slab": Mp - (S - 1) * slab > W + 3, "step_tail": Mp % 32 > W + 3, "beta_ignored": True,
            "beta_per_slab": S > 1, "taps_transposed": H * W > 1, "db_tap4_shift": Cin != Cout}
    assert {m for m, v in want.items() if v} <= set(seen) and not {m for m, v in want.items() if not v} & set(seen), (geom, sorted(seen))


def test_every_weight_gradient_mutant_is_defined_on_several_rows():
    rows = [(g, R.wgrad_plan(*g)) for g in R.WGRAD_ROWS]
    tail = [g for g, p in rows if (g[0] * (g[1] + 2) * (g[2] + 2)) % 32 > g[2] + 3]
    last = [g for g, p in rows if g[0] * (g[1] + 2) * (g[2] + 2) - (p[0] - 1) * p[1] > g[2] + 3]
    assert len(tail) >= 4 and len(last) >= 4 and sum(g[3] != g[4] for g, p in rows) >= 3, (tail, last)


def test_stride2_mutants_leave_their_bound():
    for N, H, W, C in R.COL_SHAPES:
        gen = torch.Generator().manual_seed(N + H + W + C)
        x = torch.randn(N, H, W, C, generator=gen).to(BF16)
        w = (torch.randn(8, 3, 3, C, generator=gen) * 0.05).to(BF16)
        b = torch.randn(8, generator=gen).to(BF16)
        ref, A, n = R.conv_fwd64(x, w, b, False, stride=2)
        mut = R.conv_fwd64(x, w, b, False, stride=2, mutant="half_out")[0]
        assert defined(mut, ref) == (H % 2 == 1 or W % 2 == 1), (N, H, W, C)
        if defined(mut, ref):
            assert R.worst_ratio(mut, ref, R.bf16_bound(ref, A, n)) > 1.0, (N, H, W, C)
        Ho, Wo = R.out_hw(H, W, 2)
        for dt in (BF16, F32):
            dcol = torch.randn(N * Ho * Wo, 9 * C, generator=gen).to(dt)
            ref, A, cnt = R.col2im64(dcol, N, H, W, C, 2)
            bnd = R.bf16_bound(ref, A, cnt) if dt == BF16 else R.f32_bound(ref, A, cnt)
            for m in R.STRIDE2_MUTANTS:
                mut = R.col2im64(dcol, N, H, W, C, 2, mutant=m)[0]
                if m == "parity":
                    assert defined(mut, ref)
                if defined(mut, ref):
                    assert R.worst_ratio(mut, ref, bnd) > 1.0, (N, H, W, C, dt, m)


# ------------------------------------------------------------------ plans
def test_weight_gradient_rows_are_what_plan256_decides():
    for geom, (S, stages, form) in R.WGRAD_ROWS.items():
        s, slab, st, f = R.wgrad_plan(*geom)
        assert (s, st, f) == (S, stages, form), (geom, (s, st, f))
        Mp = geom[0] * (geom[1] + 2) * (geom[2] + 2)
        assert slab % 32 == 0 and (S - 1) * slab < Mp <= S * slab
    stages = sorted({v[1] for g, v in R.WGRAD_ROWS.items() if g[3:] == (64, 64)})
    assert stages == [1, 2, 3, 4, 5, 6, 7, 8] and {v[2] for v in R.WGRAD_ROWS.values()} == {"direct", "lpq1", "lpq16"}


def plan_lines():
    lines = ["pin 1024 1024 12544 1 0 %d -1 0 0" % R.WS_BYTES]      # the checker insists on its own split-K pin in every case file
    for geom, row in R.GEMM_ROWS.items():
        N, H, W, Cin, Cout = geom
        for direction, (bm, bn, splits) in row.items():
            Ncol, K, mode = (Cout, 9 * Cin, 1) if direction == "fwd" else (Cin, 9 * Cout, 0)
            assert (bm, bn, splits) == R.gemm_plan(N * H * W, Ncol, K, R.WS_BYTES)[:3], (geom, direction)
            for ws in (R.WS_BYTES, 0):
                for lw in (-1, 0):
                    lines.append("row 0 %d %d %d %d 0 1 %d %d 0 %d %d %d %d" % (N * H * W, Ncol, K, mode, ws, lw, 1 if lw else 0, bm, bn, splits if ws else 1))
    Ms = [n * h * w for n, h, w in R.MULTI_LEVELS]
    for Cin, Cout in R.MULTI_WIDTHS:
        for mode in (0, 1):
            for lw in (-1, 0):
                lines.append("row %d %s 0 %d %d %d 0 1 0 %d 0 %d %d %d %d" % ((len(Ms), " ".join(map(str, Ms)), Cout, 9 * Cin, mode, lw, 1 if lw else 0) + R.MULTI_PLAN))
    return lines


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_implicit_gemm_rows_are_what_gemm_plan_h_decides(tmp_path):
    exe, cases = str(tmp_path / "gemm_plan_check"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "gemm_plan_check.cpp")])
    lines = plan_lines()
    assert len(lines) == 1 + 4 * sum(len(r) for r in R.GEMM_ROWS.values()) + 8
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) == len(lines)
    # the forced plans of the GPU test, from the same restatement: every instantiated tile, split-K 3 and one K-tile per slab
    N, H, W, Cin, Cout = R.FORCED_GEOM
    for t in R.TILES:
        assert R.gemm_plan(N * H * W, Cout, 9 * Cin, R.WS_BYTES, tile=t)[:3] == t + (4,) and -(-N * H * W // t[0]) >= 2 and (N * H * W) % t[0]
    assert R.gemm_plan(N * H * W, Cout, 9 * Cin, R.WS_BYTES, splitk=3)[2:] == (3, 6)
    assert R.gemm_plan(N * H * W, Cout, 9 * Cin, R.WS_BYTES, splitk=18)[2:] == (18, 1)
