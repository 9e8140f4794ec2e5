"""The convolution kernels through the C ABI (and, at the end, through layers/conv_ops.py) against the float64 restatements of
tests/_conv_ref64.py: every element of every output inside its a-priori bound, or bit-exact where the contract is exact (the
zero-bordered copies, im2col, one-hot inputs), at the geometries where each code path first exists -- M = 1, one partial row tile, image
boundaries inside a tile, one row / one column, every column-tile width, conv_kc 1 / 2 / 3 / 5, every instantiated tile, the split-K
plans that do not align with taps, every stage count of the weight gradient's pipeline, both reduce forms.  The operands' padded
copies are built on the host by the restated layout, the references are computed on the CPU.  Output-only buffers are pre-filled with NaN,
64 sentinels stand behind every output and every workspace, and every implicit-GEMM launch must report the plan its table row names
(dgx_gemm_last_form), every weight gradient the slab count of its row (through the library's own workspace size).  Each test prints
`RATIO conv <kernel> <case> <output>=<worst |err| / bound> ...` before it asserts (pytest -s shows them)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _conv_ref64 as R  # noqa: E402

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SENT = -7.5
PAD = 64
NAN = float("nan")
FORMS = (("lw", -1, 1), ("nt", 0, 0))            # (tag, dgx_dev gemm_lw, the form dgx_gemm_last_form must report)


def guarded(n, dtype, src=None):
    """n elements (src, or NaN for an output-only buffer) with PAD sentinels behind them"""
    buf = torch.full((n + PAD,), SENT, dtype=dtype, device=DEV)
    buf[:n] = NAN if src is None else src.reshape(-1).to(DEV)
    return buf


def tail_ok(buf, n):
    return bool((buf[n:].float() == SENT).all())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


@functools.lru_cache(maxsize=None)
def gemm_workspace():
    return torch.full((R.WS_BYTES // 4 + PAD,), SENT, dtype=F32, device=DEV)


def last_form():
    from divergen_amd import _lib as L
    bm, bn, sp = L.c_i(), L.c_i(), L.c_i()
    form = L.lib().dgx_gemm_last_form(bm, bn, sp)
    return form, bm.value, bn.value, sp.value


def run_conv_gemm(xpad, w, bias, N, H, W, Cin, Cout, relu, use_ws):
    """one dgx_conv3x3_gemm launch into a NaN-filled, guarded output -> (y (N, H, W, Cout) on the CPU, the plan it reports)"""
    from divergen_amd import _lib as L
    y = guarded(N * H * W * Cout, BF16)
    ws = gemm_workspace() if use_ws else None
    rc = L.lib().dgx_conv3x3_gemm(L.ptr(xpad), L.ptr(w), L.ptr(bias), L.ptr(y), N, H, W, Cin, Cout, int(relu), L.ptr(ws), R.WS_BYTES if use_ws else 0,
                                  L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert tail_ok(y, N * H * W * Cout) and (ws is None or tail_ok(ws, R.WS_BYTES // 4)), "dgx_conv3x3_gemm wrote behind a buffer"
    return y[:N * H * W * Cout].view(N, H, W, Cout).cpu(), last_form()


@functools.lru_cache(maxsize=None)
def inputs(geom, kind):
    return R.make_inputs(kind, geom, R.seed_of(geom, kind))


# ------------------------------------------------------------------ exact: the zero-bordered copies
@pytest.mark.parametrize("shape", R.PAD_SHAPES, ids=str)
def test_pad_copies_bit_equal_the_documented_layout(shape):
    from divergen_amd import _lib as L
    lib = L.lib()
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = R.plant_zeros(torch.randn(N, H, W, C, generator=gen), gen).to(BF16)
    rows = int(lib.dgx_conv3x3_pad_rows(N, H, W))
    assert rows == R.pad_rows(N, H, W)
    want = R.pad_layout(x)
    xd = dev(x)
    out = guarded(rows * C, BF16)
    assert lib.dgx_conv3x3_pad(L.ptr(xd), L.ptr(out), N, H, W, C, L.stream()) == 0
    torch.cuda.synchronize()
    assert tail_ok(out, rows * C) and torch.equal(bits(out[:rows * C].cpu()), bits(want.reshape(-1))), "dgx_conv3x3_pad"
    # the grouped copy: this image between two others of the same width
    others = [(2, 3, 2), (1, 1, 1)]
    xs = [R.plant_zeros(torch.randn(n, h, w, C, generator=gen), gen).to(BF16) for n, h, w in others]
    xs.insert(1, x)
    xds = [dev(t) for t in xs]
    outs = [guarded(R.pad_rows(*t.shape[:3]) * C, BF16) for t in xs]
    items = (L.PadItem * 3)()
    for i, (t, o) in enumerate(zip(xds, outs)):
        items[i].x, items[i].xpad, items[i].N, items[i].H, items[i].W = L.ptr(t), L.ptr(o), t.shape[0], t.shape[1], t.shape[2]
    assert lib.dgx_conv3x3_pad_multi(items, 3, C, L.stream()) == 0
    torch.cuda.synchronize()
    for t, o in zip(xs, outs):
        n = R.pad_rows(*t.shape[:3]) * C
        assert tail_ok(o, n) and torch.equal(bits(o[:n].cpu()), bits(R.pad_layout(t).reshape(-1))), "dgx_conv3x3_pad_multi"
    # the copy with ReLU' folded in: kept where the saved bf16 activation is > 0 (+0 and -0 are not)
    ysave = R.plant_zeros(torch.randn(N, H, W, C, generator=gen), gen).to(BF16)
    out, yd = guarded(rows * C, BF16), dev(ysave)
    assert lib.dgx_conv3x3_pad_relu_grad(L.ptr(xd), L.ptr(yd), L.ptr(out), N, H, W, C, L.stream()) == 0
    torch.cuda.synchronize()
    masked = torch.where(ysave.float() > 0, x, torch.zeros_like(x))        # the kernel ANDs the bits away: +0 where masked
    assert tail_ok(out, rows * C) and torch.equal(bits(out[:rows * C].cpu()), bits(R.pad_layout(masked).reshape(-1))), "dgx_conv3x3_pad_relu_grad"


# ------------------------------------------------------------------ exact: one-hot inputs
HOT_GEOM = (2, 5, 6, 64, 64)


def hot_positions(H, W):
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (2, W - 1), (3, 0)]      # the corners; the last pixel of a row, the first of the next


@pytest.mark.parametrize("direction", ["forward", "input_gradient"])
def test_one_hot_pixel_gives_the_weights_bit_for_bit(direction, dgx_dev):
    """x = 1 in one channel of one pixel per image, no bias: y[n][py+1-ky][px+1-kx][:] = w[:][ky][kx][c_n] where that pixel exists, 0
    elsewhere -- a tap that wraps into the previous row or image, or is dropped at a corner, moves or loses a weight vector.  The input
    gradient is the same launch over a one-hot dy and the tap-flipped twin."""
    N, H, W, Cin, Cout = HOT_GEOM
    gen = torch.Generator().manual_seed(77)
    w = (torch.randn(Cout, 3, 3, Cin, generator=gen) * 0.05).to(BF16)
    wk = R.flip_twin(w) if direction == "input_gradient" else w          # (rows, 3, 3, cols): the operand as the launch reads it
    wd = dev(wk.reshape(wk.shape[0], -1))
    for tag, lw, form in FORMS:
        dgx_dev("gemm_lw", lw)
        for use_ws in (True, False):
            for py, px in hot_positions(H, W):
                x = torch.zeros(N, H, W, Cin, dtype=BF16)
                want = torch.zeros(N, H, W, Cout, dtype=BF16)
                for n in range(N):
                    c = (17 + 29 * n + 7 * py + px) % Cin
                    x[n, py, px, c] = 1.0
                    for ky in range(3):
                        for kx in range(3):
                            oy, ox = py + 1 - ky, px + 1 - kx
                            if 0 <= oy < H and 0 <= ox < W:
                                want[n, oy, ox] = wk[:, ky, kx, c]
                got, plan = run_conv_gemm(dev(R.pad_layout(x)), wd, None, N, H, W, Cin, Cout, 0, use_ws)
                assert plan == (form, 128, 128, 2 if use_ws else 1), plan
                assert torch.equal(bits(got), bits(want)), (direction, tag, use_ws, (py, px), (got.float() - want.float()).abs().nonzero()[:4])


# ------------------------------------------------------------------ implicit GEMM, every element
@functools.lru_cache(maxsize=None)
def fwd_reference(geom, kind, with_bias, relu):
    inp = inputs(geom, kind)
    ref, A, n = R.conv_fwd64(inp["x"], inp["w"], inp["bias"] if with_bias else None, relu)
    return ref, R.bf16_bound(ref, A, n)


@functools.lru_cache(maxsize=None)
def dgrad_reference(geom, kind, relu):
    inp = inputs(geom, kind)
    ref, A, n = R.conv_dgrad64(inp["dy"], inp["w"], inp["ysave"], relu)
    return ref, R.bf16_bound(ref, A, n)


def run_all_plans(dgx_dev, xpad, w, bias, shape, relu, ref, bnd, row, tiles=(None,), splitk=(0,)):
    """the launch under every (form, workspace[, forced tile, forced split]) -> {tag: worst ratio}; asserts the reported plan"""
    N, H, W, Cin, Cout = shape
    out = {}
    for tag, lw, form in FORMS:
        for use_ws in (True, False):
            for tile in tiles:
                for sk in splitk:
                    dgx_dev("reset", 0)
                    dgx_dev("gemm_lw", lw)
                    if tile is not None:
                        dgx_dev("gemm_tile", tile[0] * 1000 + tile[1])
                    if sk:
                        dgx_dev("gemm_splitk", sk)
                    got, plan = run_conv_gemm(xpad, w, bias, N, H, W, Cin, Cout, relu, use_ws)
                    want = R.gemm_plan(N * H * W, Cout, 9 * Cin, R.WS_BYTES if use_ws else 0, tile=tile, splitk=sk)[:3]
                    if tile is None and not sk:
                        assert want == (row if use_ws else row[:2] + (1,)), (shape, want, row)
                    assert plan == (form,) + want, (shape, tag, use_ws, tile, sk, plan, want)
                    name = tag + (".ws" if use_ws else ".nows") + ("" if tile is None else ".%dx%d" % tile) + (".k%d" % sk if sk else "")
                    out[name] = R.worst_ratio(got, ref, bnd)
    return out


@pytest.mark.parametrize("geom", R.GEOMS, ids=str)
def test_conv3x3_gemm_every_element_every_plan(geom, dgx_dev):
    N, H, W, Cin, Cout = geom
    row = R.GEMM_ROWS[geom]
    for kind in R.INPUT_KINDS:
        inp = inputs(geom, kind)
        xpad, wd, bd = dev(R.pad_layout(inp["x"])), dev(inp["w"].reshape(Cout, -1)), dev(inp["bias"])
        for with_bias, relu in (((True, True), (True, False), (False, False)) if kind == "ordinary" else ((True, True),)):
            ref, bnd = fwd_reference(geom, kind, with_bias, relu)
            out = run_all_plans(dgx_dev, xpad, wd, bd if with_bias else None, geom, relu, ref, bnd, row["fwd"])
            R.report("conv3x3_gemm", "%s %s bias%d relu%d" % (geom, kind, with_bias, relu), {"y." + k: v for k, v in out.items()})
        if "dgrad" in row:
            for relu in (False, True):
                ref, bnd = dgrad_reference(geom, kind, relu)
                g = R.relu_mask(inp["dy"], inp["ysave"] if relu else None)
                out = run_all_plans(dgx_dev, dev(R.pad_layout(g)), dev(R.flip_twin(inp["w"]).reshape(Cin, -1)), None, (N, H, W, Cout, Cin), 0, ref, bnd,
                                    row["dgrad"])
                R.report("conv3x3_gemm", "%s %s dgrad relu%d" % (geom, kind, relu), {"dx." + k: v for k, v in out.items()})


def test_conv3x3_gemm_every_tile_and_forced_splits(dgx_dev):
    """(2, 13, 18, 128, 264), M = 468: all seven instantiated tiles leave ragged row tiles; split-K forced to 3 slabs of 6 K-tiles and to 18
    of one"""
    geom = R.FORCED_GEOM
    N, H, W, Cin, Cout = geom
    for kind in R.INPUT_KINDS:
        inp = inputs(geom, kind)
        xpad, wd, bd = dev(R.pad_layout(inp["x"])), dev(inp["w"].reshape(Cout, -1)), dev(inp["bias"])
        ref, bnd = fwd_reference(geom, kind, True, True)
        out = run_all_plans(dgx_dev, xpad, wd, bd, geom, 1, ref, bnd, None, tiles=R.TILES)
        R.report("conv3x3_gemm", "%s %s tiles" % (geom, kind), {"y." + k: v for k, v in out.items()})
        out = run_all_plans(dgx_dev, xpad, wd, bd, geom, 1, ref, bnd, None, splitk=(3, 18))
        R.report("conv3x3_gemm", "%s %s splitk" % (geom, kind), {"y." + k: v for k, v in out.items()})


# ------------------------------------------------------------------ grouped forward
@functools.lru_cache(maxsize=None)
def multi_reference(level, width, kind, with_bias, relu):
    inp = inputs(level + width, kind)
    base = inputs(R.MULTI_LEVELS[0] + width, kind)          # the levels share the first level's weights and bias
    ref, A, n = R.conv_fwd64(inp["x"], base["w"], base["bias"] if with_bias else None, relu)
    return ref, R.bf16_bound(ref, A, n)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("relu", [0, 1], ids=["relu0", "relu1"])
@pytest.mark.parametrize("width", R.MULTI_WIDTHS, ids=str)
def test_conv3x3_gemm_multi_every_element(width, relu, with_bias, dgx_dev):
    from divergen_amd import _lib as L
    lib = L.lib()
    Cin, Cout = width
    for kind in R.INPUT_KINDS:
        base = inputs(R.MULTI_LEVELS[0] + width, kind)
        wd, bd = dev(base["w"].reshape(Cout, -1)), dev(base["bias"]) if with_bias else None
        xps = [dev(R.pad_layout(inputs(lv + width, kind)["x"])) for lv in R.MULTI_LEVELS]
        out = {}
        for tag, lw, form in FORMS:
            dgx_dev("gemm_lw", lw)
            ys = [guarded(n * h * w * Cout, BF16) for n, h, w in R.MULTI_LEVELS]
            items = (L.ConvItem * len(ys))()
            for i, ((n, h, w), xp, y) in enumerate(zip(R.MULTI_LEVELS, xps, ys)):
                items[i].xpad, items[i].y, items[i].N, items[i].H, items[i].W = L.ptr(xp), L.ptr(y), n, h, w
            assert lib.dgx_conv3x3_gemm_multi(items, len(ys), L.ptr(wd), L.ptr(bd), Cin, Cout, relu, L.stream()) == 0
            torch.cuda.synchronize()
            assert last_form() == (form,) + R.MULTI_PLAN, last_form()
            for lv, y in zip(R.MULTI_LEVELS, ys):
                n = lv[0] * lv[1] * lv[2] * Cout
                assert tail_ok(y, n), ("dgx_conv3x3_gemm_multi wrote behind level", lv)
                ref, bnd = multi_reference(lv, width, kind, with_bias, bool(relu))
                out["y%dx%d.%s" % (lv[1], lv[2], tag)] = R.worst_ratio(y[:n].view(ref.shape).cpu(), ref, bnd)
        R.report("conv3x3_gemm_multi", "%s %s bias%d relu%d" % (width, kind, with_bias, relu), out)


# ------------------------------------------------------------------ weight and bias gradient
def slabs_from_workspace(nbytes, Cin, Cout):
    assert nbytes % 4 == 0
    hit = [S for S in range(1, 4097) if R.wgrad_workspace_floats(S, Cin, Cout) * 4 == nbytes]
    assert len(hit) == 1, (nbytes, hit)
    return hit[0]


@pytest.mark.parametrize("geom", list(R.WGRAD_ROWS), ids=str)
def test_conv3x3_wgrad_bias_every_element(geom):
    from divergen_amd import _lib as L
    lib = L.lib()
    N, H, W, Cin, Cout = geom
    S, stages, form = R.WGRAD_ROWS[geom]
    assert (S, stages, form) == R.wgrad_plan(*geom)[:1] + R.wgrad_plan(*geom)[2:]
    nbytes = int(lib.dgx_conv3x3_wgrad_bias_workspace_bytes(N, H, W, Cin, Cout))
    assert slabs_from_workspace(nbytes, Cin, Cout) == S, (geom, nbytes)
    nws = max(nbytes // 4, 4)
    for kind in R.INPUT_KINDS:
        inp = inputs(geom, kind)
        g = R.relu_mask(inp["dy"], inp["ysave"] if kind == "postrelu" else None)
        gp, xp = dev(R.pad_layout(g)), dev(R.pad_layout(inp["x"]))
        out = {}
        for beta in (0.0, 1.0):
            (dW, db), (Aw, Ab), n = R.conv_wgrad64(g, inp["x"], inp["g0"], beta)
            for with_gb in (True, False):
                gw = guarded(dW.numel(), F32, inp["g0"][0] if beta else None)
                gb = guarded(Cout, F32, inp["g0"][1] if beta else None) if with_gb else None
                ws = guarded(nws, F32)
                assert lib.dgx_conv3x3_wgrad_bias(L.ptr(gp), L.ptr(xp), L.ptr(gw), L.ptr(gb), N, H, W, Cin, Cout, beta, L.ptr(ws), L.stream()) == 0
                torch.cuda.synchronize()
                assert tail_ok(gw, dW.numel()) and tail_ok(ws, nws) and (gb is None or tail_ok(gb, Cout)), "dgx_conv3x3_wgrad_bias wrote behind a buffer"
                tag = "beta%d%s" % (beta, "" if with_gb else ".nogb")
                out["dW." + tag] = R.worst_ratio(gw[:dW.numel()].view(dW.shape).cpu(), dW, R.f32_bound(dW, Aw, n))
                if with_gb:
                    out["db." + tag] = R.worst_ratio(gb[:Cout].cpu(), db, R.f32_bound(db, Ab, n))
        R.report("conv3x3_wgrad_bias", "%s %s S%d stages%d %s" % (geom, kind, S, stages, form), out)


@pytest.mark.parametrize("width", R.WGRAD_MULTI_WIDTHS, ids=str)
def test_conv3x3_wgrad_bias_multi_every_element(width):
    from divergen_amd import _lib as L
    lib = L.lib()
    Cin, Cout = width
    levels = R.WGRAD_MULTI_LEVELS
    Rrows, nsl = R.wgrad_multi_plan(levels, Cin, Cout)
    Stot = sum(nsl)
    for kind in R.INPUT_KINDS:
        inps = [inputs(lv + width, kind) for lv in levels]
        gs = [R.relu_mask(i["dy"], i["ysave"] if kind == "postrelu" else None) for i in inps]
        gps, xps = [dev(R.pad_layout(g)) for g in gs], [dev(R.pad_layout(i["x"])) for i in inps]
        items = (L.ConvWgradItem * len(levels))()
        for i, ((n, h, w), gp, xp) in enumerate(zip(levels, gps, xps)):
            items[i].dypad, items[i].xpad, items[i].N, items[i].H, items[i].W = L.ptr(gp), L.ptr(xp), n, h, w
        nbytes = int(lib.dgx_conv3x3_wgrad_bias_multi_workspace_bytes(items, len(levels), Cin, Cout))
        assert nbytes == (9 * Stot * Cout * Cin + (Stot * Cout + 3) // 4 * 4) * 4, (width, nbytes, Rrows, nsl)
        g0 = inps[0]["g0"]
        out = {}
        for beta in (0.0, 1.0):
            dW, db = (beta * g0[0].double(), beta * g0[1].double())
            Aw, Ab, n = dW.abs(), db.abs(), int(beta != 0)
            for g, i in zip(gs, inps):
                (w1, b1), (a1, a2), n1 = R.conv_wgrad64(g, i["x"], None, 0.0)
                dW, db, Aw, Ab, n = dW + w1, db + b1, Aw + a1, Ab + a2, n + n1
            for with_gb in (True, False):
                gw = guarded(dW.numel(), F32, g0[0] if beta else None)
                gb = guarded(Cout, F32, g0[1] if beta else None) if with_gb else None
                ws = guarded(nbytes // 4, F32)
                assert lib.dgx_conv3x3_wgrad_bias_multi(items, len(levels), L.ptr(gw), L.ptr(gb), Cin, Cout, beta, L.ptr(ws), L.stream()) == 0
                torch.cuda.synchronize()
                assert tail_ok(gw, dW.numel()) and tail_ok(ws, nbytes // 4) and (gb is None or tail_ok(gb, Cout)), "wgrad_bias_multi wrote behind a buffer"
                tag = "beta%d%s" % (beta, "" if with_gb else ".nogb")
                out["dW." + tag] = R.worst_ratio(gw[:dW.numel()].view(dW.shape).cpu(), dW, R.f32_bound(dW, Aw, n))
                if with_gb:
                    out["db." + tag] = R.worst_ratio(gb[:Cout].cpu(), db, R.f32_bound(db, Ab, n))
        R.report("conv3x3_wgrad_bias_multi", "%s %s R%d S%d" % (width, kind, Rrows, Stot), out)


# ------------------------------------------------------------------ column-matrix form
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", R.COL_SHAPES, ids=str)
def test_im2col_exact_and_col2im_every_element(shape, stride):
    from divergen_amd import _lib as L
    lib = L.lib()
    N, H, W, C0 = shape
    out = {}
    for dt, code in ((BF16, L.DGX_BF16), (F32, L.DGX_F32)):
        C = 4 if (dt == F32 and shape == R.COL_SHAPES[0]) else C0
        gen = torch.Generator().manual_seed(sum(shape) + stride)
        Ho, Wo = R.out_hw(H, W, stride)
        x = R.plant_zeros(torch.randn(N, H, W, C, generator=gen), gen).to(dt)
        col, xd = guarded(N * Ho * Wo * 9 * C, dt), dev(x)
        assert lib.dgx_im2col3x3(L.ptr(xd), L.ptr(col), N, H, W, C, stride, code, L.stream()) == 0
        torch.cuda.synchronize()
        want = R.im2col64(x, stride)
        assert tail_ok(col, want.numel()) and torch.equal(bits(col[:want.numel()].cpu()), bits(want.reshape(-1))), ("im2col", shape, stride, dt)
        for kind in ("ordinary", "cancelling"):
            dcol = torch.randn(N * Ho * Wo, 9 * C, generator=gen)
            dcol = ((dcol + 64.0) * torch.where(torch.rand(dcol.shape, generator=gen) < 0.5, -1.0, 1.0) if kind == "cancelling" else dcol).to(dt)
            dx, dcd = guarded(N * H * W * C, dt), dev(dcol)
            assert lib.dgx_col2im3x3(L.ptr(dcd), L.ptr(dx), N, H, W, C, stride, code, L.stream()) == 0
            torch.cuda.synchronize()
            ref, A, cnt = R.col2im64(dcol, N, H, W, C, stride)
            assert tail_ok(dx, ref.numel())
            bnd = R.bf16_bound(ref, A, cnt) if dt == BF16 else R.f32_bound(ref, A, cnt)
            out["dx.%s.%s" % ("bf16" if dt == BF16 else "f32", kind)] = R.worst_ratio(dx[:ref.numel()].view(ref.shape).cpu(), ref, bnd)
    R.report("col2im3x3", "%s stride%d" % (shape, stride), out)


# ------------------------------------------------------------------ through the Python layer
def nchw_leaf(x_nhwc, dtype=None):
    t = x_nhwc.to(DEV)
    t = t if dtype is None else t.to(dtype)
    return t.permute(0, 3, 1, 2).detach().requires_grad_(True)


def nhwc_cpu(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().cpu()


@pytest.mark.parametrize("relu", [False, True], ids=["relu0", "relu1"])
@pytest.mark.parametrize("Cout", [1, 4, 24, 64, 72])
def test_python_conv3x3_autograd_every_element(Cout, relu):
    """layers.conv_ops.conv3x3 at Cin = 64: the zero-padded output channels of the 1- and 4-channel predictors, the Cout % 64 channel
    padding of the input gradient, and both places where ReLU' is applied (in the padded copy at Cout % 64 == 0, as a product elsewhere)"""
    from divergen_amd.layers import conv_ops
    assert conv_ops._IMPLICIT and conv_ops._SPLITK
    geom = (2, 7, 9, 64, Cout)
    for kind in R.INPUT_KINDS:
        inp = R.make_inputs(kind, (2, 7, 9, 64, max(Cout, 8)), R.seed_of(geom, kind))
        w, b, dy = inp["w"][:Cout], inp["bias"][:Cout], inp["dy"][..., :Cout].contiguous()
        xd = nchw_leaf(inp["x"])
        wd, bd = w.float().permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True)
        y = conv_ops.conv3x3(xd, wd, bd, 1, relu=relu)
        assert y.dtype == BF16 and y.shape == (2, Cout, 7, 9)
        y.backward(dy.to(DEV).permute(0, 3, 1, 2))
        torch.cuda.synchronize()
        yk = nhwc_cpu(y)
        ref, A, n = R.conv_fwd64(inp["x"], w, b, relu)
        out = {"y": R.worst_ratio(yk, ref, R.bf16_bound(ref, A, n))}
        ref, A, n = R.conv_dgrad64(dy, w, yk, relu)
        out["dx"] = R.worst_ratio(nhwc_cpu(xd.grad), ref, R.bf16_bound(ref, A, n))
        (dW, db), (Aw, Ab), n = R.conv_wgrad64(R.relu_mask(dy, yk if relu else None), inp["x"], None, 0.0)
        assert wd.grad.dtype == F32 and bd.grad.dtype == F32
        out["dW"] = R.worst_ratio(nhwc_cpu(wd.grad), dW, R.f32_bound(dW, Aw, n))
        out["db"] = R.worst_ratio(bd.grad.cpu(), db, R.f32_bound(db, Ab, n))
        R.report("conv_ops.conv3x3", "%s %s relu%d" % (geom, kind, relu), out)


@pytest.mark.parametrize("case", [(2, 16, 13, 18), (1, 256, 7, 5)], ids=str)
def test_python_conv3x3_stride2_every_element(case):
    """im2col + GEMM forward; backward = GEMM to a bf16 column matrix + col2im (two roundings: _conv_ref64.two_rounding_bound), the weight
    gradient over the column matrix"""
    from divergen_amd.layers import conv_ops
    N, C, H, W = case
    Cout = 24
    for kind in R.INPUT_KINDS:
        inp = R.make_inputs(kind, (N, H, W, C, Cout), R.seed_of((N, H, W, C, Cout), kind))
        Ho, Wo = R.out_hw(H, W, 2)
        dy = inp["dy"][:, :Ho, :Wo].contiguous()
        xd = nchw_leaf(inp["x"])
        wd, bd = inp["w"].float().permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True), inp["bias"].float().to(DEV).requires_grad_(True)
        y = conv_ops.conv3x3(xd, wd, bd, 2)
        assert y.dtype == BF16 and y.shape == (N, Cout, Ho, Wo)
        y.backward(dy.to(DEV).permute(0, 3, 1, 2))
        torch.cuda.synchronize()
        ref, A, n = R.conv_fwd64(inp["x"], inp["w"], inp["bias"], False, stride=2)
        out = {"y": R.worst_ratio(nhwc_cpu(y), ref, R.bf16_bound(ref, A, n))}
        ref, A1, S1, n1, cnt = R.conv_dgrad_cols64(dy, inp["w"], N, H, W, 2)
        out["dx"] = R.worst_ratio(nhwc_cpu(xd.grad), ref, R.two_rounding_bound(ref, A1, n1, S1, cnt))
        (dW, db), (Aw, Ab), n = R.conv_wgrad_cols64(dy, inp["x"], 2)
        out["dW"] = R.worst_ratio(nhwc_cpu(wd.grad), dW, R.f32_bound(dW, Aw, n))
        out["db"] = R.worst_ratio(bd.grad.cpu(), db, R.f32_bound(db, Ab, n))
        R.report("conv_ops.conv3x3", "%s stride2 %s" % (case, kind), out)


@pytest.mark.parametrize("relu", [False, True], ids=["relu0", "relu1"])
@pytest.mark.parametrize("case", [(3, 64, 7, 9, 32), (1, 8, 1, 1, 8)], ids=str)
def test_python_deconv2x2_every_element(case, relu):
    from divergen_amd.layers.conv_ops import deconv2x2
    N, Cin, H, W, Cout = case
    gen = torch.Generator().manual_seed(8 + Cin + Cout)
    x = R.plant_zeros(torch.randn(N, H, W, Cin, generator=gen), gen).to(BF16)
    w = (torch.randn(Cin, Cout, 2, 2, generator=gen) * 0.1).to(BF16)
    b = torch.randn(Cout, generator=gen).to(BF16)
    dy = torch.randn(N, 2 * H, 2 * W, Cout, generator=gen).to(BF16)
    xd = nchw_leaf(x, F32)
    wd, bd = w.float().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16):
        y = deconv2x2(xd, wd, bd, relu=relu)
    assert y.dtype == BF16 and y.shape == (N, Cout, 2 * H, 2 * W)
    y.backward(dy.to(DEV).permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    yk = nhwc_cpu(y)
    ref = R.deconv2x2_64(x, w, b, relu, dy=dy, y_kernel=yk)
    got = {"y": yk, "dx": nhwc_cpu(xd.grad), "dw": wd.grad.cpu(), "db": bd.grad.cpu()}
    out = {k: R.worst_ratio(got[k], r, (R.bf16_bound if k in ("y", "dx") else R.f32_bound)(r, A, n)) for k, (r, A, n) in ref.items()}
    R.report("conv_ops.deconv2x2", "%s relu%d" % (case, relu), out)


def test_python_arena_conv_accumulates_two_steps():
    """A Conv2d(64, 64) in a FlatArena stepped twice: the second backward accumulates onto the first (beta = 1 onto the kernel's own
    first result), so the gradients are twice the reference, each step inside the beta = 1 bound."""
    from divergen_amd.layers.conv_ops import Conv2d
    from divergen_amd.solver import FlatArena
    torch.manual_seed(4)
    conv = Conv2d(64, 64, 3, 1, 1).to(DEV)
    w0, b0 = conv.weight.detach().clone(), conv.bias.detach().clone()
    arena = FlatArena(conv)
    assert float(arena.g.abs().sum()) == 0.0
    geom = (2, 12, 10, 64, 64)
    inp = R.make_inputs("ordinary", geom, R.seed_of(geom, "ordinary"))
    w = w0.to(BF16).permute(0, 2, 3, 1).contiguous().cpu()          # (Cout, 3, 3, Cin), the arena's bf16 shadow
    b = b0.to(BF16).cpu()
    x = nchw_leaf(inp["x"], F32)
    dy = inp["dy"]
    prev = (torch.zeros(64, 3, 3, 64), torch.zeros(64))
    total = [0.0, 0.0]
    for step in (1, 2):
        with torch.autocast("cuda", dtype=BF16):
            y = conv(x)
        y.backward(dy.to(DEV).permute(0, 3, 1, 2))
        torch.cuda.synchronize()
        ref, A, n = R.conv_fwd64(inp["x"], w, b, False)
        out = {"y": R.worst_ratio(nhwc_cpu(y), ref, R.bf16_bound(ref, A, n))}
        (dW, db), (Aw, Ab), n = R.conv_wgrad64(dy, inp["x"], prev, 1.0)
        gw, gb = nhwc_cpu(conv.weight.grad), conv.bias.grad.detach().cpu().clone()
        out["dW"] = R.worst_ratio(gw, dW, R.f32_bound(dW, Aw, n))
        out["db"] = R.worst_ratio(gb, db, R.f32_bound(db, Ab, n))
        R.report("conv_ops.Conv2d(arena)", "%s step%d" % (geom, step), out)
        prev = (gw, gb)
        total = [total[0] + R.f32_bound(dW, Aw, n), total[1] + R.f32_bound(db, Ab, n)]
    # |g2 - 2 dW| <= |g2 - (g1 + dW)| + |g1 - dW|: the two steps' bounds added
    (dW, db), _, _ = R.conv_wgrad64(dy, inp["x"], None, 0.0)
    two = {"dW": R.worst_ratio(prev[0], 2 * dW, total[0]), "db": R.worst_ratio(prev[1], 2 * db, total[1])}
    R.report("conv_ops.Conv2d(arena)", "%s twice-the-reference" % (geom,), two)


# ------------------------------------------------------------------ Linear weight gradients (the same kernels, through dgx_linear_wgrad_grouped)
@functools.lru_cache(maxsize=None)
def linear_case(shapes):
    """operands, first gradients and the float64 references of a group, computed once: [(dy, x, gw0, gb0, dW, Aw, db, Ab)]"""
    gen = torch.Generator().manual_seed(7000 + sum(M + Nn + Kk for M, Nn, Kk in shapes))
    out = []
    for M, Nn, Kk in shapes:
        dy, x = R.bf(torch.randn(M, Nn, generator=gen)), R.bf(torch.randn(M, Kk, generator=gen))
        gw0, gb0 = torch.randn(Nn, Kk, generator=gen), torch.randn(Nn, generator=gen)
        d, xx = dy.double(), x.double()
        out.append((dy, x, gw0, gb0, d.t() @ xx, d.abs().t() @ xx.abs(), d.sum(0), d.abs().sum(0)))
    return out


def run_linear_group(shapes, expect_form, out):
    from divergen_amd import _lib as L
    lib = L.lib()
    case = linear_case(shapes)
    ops = [(dev(c[0]), dev(c[1])) for c in case]
    for beta in (0.0, 1.0):
        for with_gb in (True, False):
            n = len(shapes)
            arr = (L.WgradProblem * n)()
            gws, gbs = [], []
            for i, ((M, Nn, Kk), c, (dyd, xd)) in enumerate(zip(shapes, case, ops)):
                gws.append(guarded(Nn * Kk, F32, c[2] if beta else None))
                gbs.append(guarded(Nn, F32, c[3] if beta else None) if with_gb else None)
                arr[i].dy, arr[i].x, arr[i].gw, arr[i].gb = L.ptr(dyd), L.ptr(xd), L.ptr(gws[i]), L.ptr(gbs[i])
                arr[i].M, arr[i].Nn, arr[i].Kk = M, Nn, Kk
            assert int(lib.dgx_wgrad_grouped_form(arr, n)) == expect_form
            nws = max(int(lib.dgx_wgrad_grouped_workspace_bytes(arr, n)) // 4, 4)
            ws = guarded(nws, F32)
            assert lib.dgx_linear_wgrad_grouped(arr, n, beta, L.ptr(ws), L.stream()) == 0
            torch.cuda.synchronize()
            assert tail_ok(ws, nws), "dgx_linear_wgrad_grouped wrote behind its workspace"
            for i, ((M, Nn, Kk), c) in enumerate(zip(shapes, case)):
                assert tail_ok(gws[i], Nn * Kk) and (gbs[i] is None or tail_ok(gbs[i], Nn)), "dgx_linear_wgrad_grouped wrote behind a buffer"
                dW, Aw, db, Ab, cnt = c[4], c[5], c[6], c[7], M
                if beta:
                    dW, Aw, db, Ab, cnt = dW + beta * c[2].double(), Aw + c[2].double().abs(), db + beta * c[3].double(), Ab + c[3].double().abs(), M + 1
                key = "%sbeta%d%s" % ("p%d." % i if n > 1 else "", beta, "" if with_gb else ".nogb")
                rw = R.worst_ratio(gws[i][:Nn * Kk].view(Nn, Kk).cpu(), dW, R.f32_bound(dW, Aw, cnt))
                rb = R.worst_ratio(gbs[i][:Nn].cpu(), db, R.f32_bound(db, Ab, cnt)) if with_gb else 0.0
                if i in (0, n - 1):
                    out["dW." + key] = rw
                    if with_gb:
                        out["db." + key] = rb
                else:                               # the inner problems of a long group: asserted, not printed one by one
                    assert rw <= 1.0 and rb <= 1.0, (shapes, i, rw, rb)


LINEAR_CASES = [("split", sh, 0) for sh in R.LINEAR_WGRAD_ROWS] + [("lw", sh, r) for sh in R.LINEAR_WGRAD_LW for r in (0, 16)]


@pytest.mark.parametrize("form,shapes,reserved_cus", LINEAR_CASES, ids=lambda v: "%dx%s" % (len(v), v[0]) if isinstance(v, tuple) else str(v))
def test_linear_wgrad_grouped_every_element(form, shapes, reserved_cus, dgx_dev):
    """gw and gb of every problem of dgx_linear_wgrad_grouped against float64 under the fp32-accumulation bound, beta 0 / 1, with and
    without bias gradients.  Split form: every branch of its plan (LINEAR_WGRAD_ROWS: unsplit, both reduce forms, 1-5 stages per slab with
    ragged last slabs, a mixed group).  Loader-wave form, forced: 13 problems of 4 ragged items each (n > 12: no fall-back, no workspace)
    and one problem of one exact item, with all CUs and with 16 reserved."""
    from divergen_amd import _lib as L
    out = {}
    if form == "split":
        S, stages, red = R.LINEAR_WGRAD_ROWS[shapes]
        plan = R.wgrad_group_plan(shapes)
        assert (plan[0], plan[1][-1] // 32, plan[2]) == (S, stages, red)
        dgx_dev("wgrad_lw", 0)
        run_linear_group(shapes, 0, out)
        R.report("linear_wgrad_grouped", "%s S%s stages%d %s" % (shapes if len(shapes) > 1 else shapes[0], S, stages, red), out)
    else:
        dgx_dev("wgrad_lw", 2)
        L.lib().dgx_set_reserved_cus(reserved_cus)
        try:
            run_linear_group(shapes, 1, out)
        finally:
            L.lib().dgx_set_reserved_cus(0)
        R.report("linear_wgrad_grouped", "lw %d x %s reserved%d" % (len(shapes), shapes[0], reserved_cus), out)
