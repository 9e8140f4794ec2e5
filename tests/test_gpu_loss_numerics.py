"""The fused loss kernels (csrc/detic_loss.hip, csrc/centernet_loss.hip, csrc/mask_loss.hip) through the C ABI against the float64
restatements of tests/_loss_ref64.py: every output element finite and inside its a-priori bound, or exact where the contract is exact
(counts, statistics, box-delta signs, zero columns, ignore rows, untouched sentinels) -- at the product's LVIS width C = 1203, around
the 256-thread column stride, on hard logits and on the strided joint layout layers/box_stage.py uses, with dgx_detic_grad_scale.
Every output buffer is pre-filled with NaN, every region the kernel must leave alone with a sentinel.  Each test prints
`RATIO <group> <case> <output>=<worst error / bound> ...` before it asserts (pytest -s shows them)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _loss_ref64 as R  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
SENT = -7.5                  # exact in bf16; no output of these kernels takes this value by accident in a whole region
PAD_ROWS = 3
SCALES = ((1.0, 1.0), (0.37, 2.5), (1.0, 0.0))


def _dev(t, dtype=None):
    return None if t is None else (t.to(dtype) if dtype is not None else t).contiguous().to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def report(group, what, ratios):
    print("RATIO %s %s %s" % (group, what, " ".join("%s=%.3f" % kv for kv in ratios.items())))
    assert all(v <= 1.0 for v in ratios.values()), (group, what, ratios)


# ------------------------------------------------------------------ Detic
def run_detic(c, dtype, joint, product_ld=False):
    """c: a case already cast (R.detic_cast).  Returns CPU tensors: out16, dlogits (R, C + 1), dsign, part, `raw` = the whole gradient
    buffer with its sentinel rows / columns, and for the joint entry `dev` = what dgx_detic_grad_scale needs."""
    from divergen_amd import _lib as L
    lib, st = L.lib(), L.stream()
    x, d = c["logits"], c["deltas"]
    Rr, C1 = x.shape
    C = C1 - 1
    gt, cw, prop, gtb, src = _dev(c["gt"]), _dev(c["class_w"], F32), _dev(c["prop"], F32), _dev(c["gtb"], F32), _dev(c["src"])
    wts = [float(w) for w in c["weights"]]
    rows = Rr + PAD_ROWS
    dsign = torch.full((rows, 4), SENT, dtype=F32, device=DEV)
    part = torch.full((rows, 8), SENT, dtype=F32, device=DEV)
    dsign[:Rr], part[:Rr] = float("nan"), float("nan")
    out16 = torch.full((16,), float("nan"), dtype=F32, device=DEV)
    code = L.DGX_BF16 if dtype == BF16 else L.DGX_F32
    if joint:
        ld, gcols = R.joint_ld(C, product_ld)
        y = torch.full((rows, ld), 0.25, dtype=dtype, device=DEV)             # logits | deltas | whatever the GEMM left behind them
        y[:Rr, :C1], y[:Rr, C1:C1 + 4] = x.to(DEV), d.to(DEV)
        dy = torch.full((rows, ld), SENT, dtype=dtype, device=DEV)
        dy[:Rr, :gcols] = float("nan")
        L.check(lib.dgx_detic_losses_strided(y.data_ptr(), ld, y.data_ptr() + y.element_size() * C1, ld, L.ptr(gt), L.ptr(cw), L.ptr(prop),
                                             L.ptr(gtb), L.ptr(src), Rr, C, wts[0], wts[1], wts[2], wts[3], dy.data_ptr(), ld, gcols,
                                             L.ptr(dsign), L.ptr(out16), L.ptr(part), code, st), "dgx_detic_losses_strided")
    else:
        gcols = C1
        xd, dd = _dev(x), _dev(d)
        dy = torch.full((rows, C1), SENT, dtype=dtype, device=DEV)
        dy[:Rr] = float("nan")
        L.check(lib.dgx_detic_losses(L.ptr(xd), L.ptr(dd), L.ptr(gt), L.ptr(cw), L.ptr(prop), L.ptr(gtb), L.ptr(src), Rr, C, wts[0], wts[1],
                                     wts[2], wts[3], L.ptr(dy), L.ptr(dsign), L.ptr(out16), L.ptr(part), code, st), "dgx_detic_losses")
    torch.cuda.synchronize()
    return {"out16": out16.cpu(), "dlogits": dy[:Rr, :C1].cpu(), "dsign": dsign[:Rr].cpu(), "part": part[:Rr].cpu(), "raw": dy.cpu(),
            "raw_dsign": dsign.cpu(), "raw_part": part.cpu(), "gcols": gcols, "dev": (dy, out16)}


def check_detic(group, what, got, ref, dtype):
    Rr, C1 = ref["dlogits"].shape
    for k in ("dlogits", "dsign", "part"):
        assert bool(torch.isfinite(got[k].float()).all()), (what, k, "not finite")
    assert bool(torch.isfinite(got["out16"][:15]).all()), (what, "out16", got["out16"])
    ratios = R.detic_check({k: got[k].double() for k in ("out16", "dlogits", "dsign", "part")}, ref, dtype)
    # sentinels: rows >= R of every buffer, columns >= grad_cols of the gradient buffer
    raw, gc = got["raw"].float(), got["gcols"]
    assert bool((raw[Rr:] == SENT).all()) and bool((raw[:, gc:] == SENT).all()), (what, "gradient buffer written outside (R, grad_cols)")
    assert bool((got["raw_dsign"][Rr:] == SENT).all()) and bool((got["raw_part"][Rr:] == SENT).all()), (what, "dsign / part rows >= R written")
    # column C and ignore rows: exactly zero (their bound is zero); restated here by name
    assert float(got["dlogits"][:, C1 - 1].float().abs().max()) == 0.0, (what, "background column")
    report(group, what, ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(R.DETIC_CASES))
def test_detic_contiguous_entry(name, dtype):
    c = R.detic_cast(R.DETIC_CASES[name](), dtype)
    ref = R.detic_ref64(*R.detic_args(c))
    got = run_detic(c, dtype, joint=False)
    what = "%s %s" % (name, "bf16" if dtype == BF16 else "f32")
    check_detic("detic-contiguous", what, got, ref, dtype)
    if name.startswith("all_ignore"):
        assert float(got["out16"][8]) == 0.0 and float(got["out16"][14]) == 1.0 and float(got["out16"][7]) == 0.0
    if name.startswith("all_background"):
        assert float(got["out16"][9]) == 0.0 and float(got["out16"][10]) == 1.0
    # the fold runs in a fixed order: a second run on the same inputs is bit-identical
    again = run_detic(c, dtype, joint=False)
    for k in ("out16", "dlogits", "dsign", "part"):
        assert torch.equal(_bits(got[k]), _bits(again[k])), (what, k, "two runs differ")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(R.DETIC_CASES))
def test_detic_joint_entry_and_grad_scale(name, dtype):
    """dgx_detic_losses_strided on the joint layout (logits and deltas read out of one (R, ld) buffer, the gradient row = logit
    gradients | signs | zeros up to grad_cols), then dgx_detic_grad_scale in place.  The widths 1204 and 41 use the product's
    ld = grad_cols = pad8(C + 5) (_loss_ref64.joint_ld); the others keep 8 sentinel columns behind grad_cols."""
    from divergen_amd import _lib as L
    c = R.detic_cast(R.DETIC_CASES[name](), dtype)
    ref = R.detic_ref64(*R.detic_args(c))
    Rr, C1 = c["logits"].shape
    C = C1 - 1
    got = run_detic(c, dtype, joint=True, product_ld=C1 in R.PRODUCT_WIDTHS)
    what = "%s %s" % (name, "bf16" if dtype == BF16 else "f32")
    check_detic("detic-joint", what, got, ref, dtype)
    gc = got["gcols"]
    raw = got["raw"]
    assert torch.equal(raw[:Rr, C1:C1 + 4].float(), got["dsign"]), (what, "joint columns [C+1, C+5) != dsign")
    assert float(raw[:Rr, C1 + 4:gc].float().abs().max() if gc > C1 + 4 else 0.0) == 0.0, (what, "pad columns [C+5, grad_cols) not zero")
    buf, bb, _, _ = R.detic_joint_ref64(ref, gc, dtype)
    assert R.worst_ratio(raw[:Rr, :gc].double(), buf, bb) <= 1.0
    dy, out16 = got["dev"]
    ld = dy.shape[1]
    code = L.DGX_BF16 if dtype == BF16 else L.DGX_F32
    ratios = {}
    for g_cls, g_box in SCALES:
        z = dy.clone()
        gc_t, gb_t = torch.tensor([g_cls], dtype=F32, device=DEV), torch.tensor([g_box], dtype=F32, device=DEV)
        L.check(L.lib().dgx_detic_grad_scale(z.data_ptr(), ld, Rr, C, L.ptr(out16), L.ptr(gc_t), L.ptr(gb_t), code, L.stream()), "dgx_detic_grad_scale")
        torch.cuda.synchronize()
        z = z.cpu()
        assert bool(torch.isfinite(z.float()).all()), (what, "grad_scale: not finite")
        # the kernel rounded to the storage type before the scale: expected = round_T(stored * scale), formed from the buffer as stored
        want = R.grad_scale_ref64(raw.double(), Rr, C, got["out16"], g_cls, g_box)
        ratios["g%g_%g" % (g_cls, g_box)] = R.worst_ratio(z[:Rr, :C + 5].double(), want[:Rr, :C + 5], R.grad_scale_bound(want[:Rr, :C + 5], dtype))
        assert torch.equal(_bits(z[:, C + 5:]), _bits(raw[:, C + 5:])), (what, "grad_scale touched columns >= C + 5")
        assert torch.equal(_bits(z[Rr:]), _bits(raw[Rr:])), (what, "grad_scale touched rows >= rows")
        if g_box == 0.0:
            assert float(z[:Rr, C1:C1 + 4].float().abs().max()) == 0.0
    report("grad-scale", what, ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_detic_no_rows_returns_sixteen_zeros(dtype):
    from divergen_amd import _lib as L
    out16 = torch.full((16,), float("nan"), dtype=F32, device=DEV)
    code = L.DGX_BF16 if dtype == BF16 else L.DGX_F32
    rc = L.lib().dgx_detic_losses(None, None, None, None, None, None, None, 0, 1203, 10.0, 10.0, 5.0, 5.0, None, None, L.ptr(out16), None, code, L.stream())
    assert rc == 0
    rc = L.lib().dgx_detic_grad_scale(None, 1208, 0, 1203, L.ptr(out16), None, None, code, L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert out16.cpu().tolist() == [0.0] * 16


# ------------------------------------------------------------------ CenterNet
def run_centernet(c):
    from divergen_amd import _lib as L
    lib = L.lib()
    cfg = c["cfg"]
    M, P = c["logit"].numel(), c["pos_idx"].numel()
    C = c["hms"].shape[1]
    g_reg = torch.full((M + PAD_ROWS, 4), SENT, dtype=F32, device=DEV)
    g_neg = torch.full((M + PAD_ROWS,), SENT, dtype=F32, device=DEV)
    g_pos = torch.full((M + PAD_ROWS,), SENT, dtype=F32, device=DEV)
    g_reg[:M], g_neg[:M], g_pos[:M] = float("nan"), float("nan"), float("nan")
    out = torch.full((8,), float("nan"), dtype=F32, device=DEV)
    part = torch.full((3 * lib.dgx_centernet_losses_blocks(M),), float("nan"), dtype=F32, device=DEV)
    rp, rt, hm, lg = _dev(c["reg_pred"], F32), _dev(c["reg_tgt"], F32), _dev(c["hms"], F32), _dev(c["logit"], F32)
    idx = _dev(c["pos_idx"]) if P else None
    car = _dev(c["cared"].to(torch.uint8)) if c["cared"] is not None and P else None
    L.check(lib.dgx_centernet_losses(L.ptr(rp), L.ptr(rt), L.ptr(hm), L.ptr(lg), L.ptr(idx), L.ptr(car), M, C, P, int(cfg["not_norm_reg"]),
                                     cfg["beta"], cfg["gamma"], cfg["clamp"], cfg["ignore_high_fp"], cfg["pos_mul"], cfg["neg_mul"],
                                     L.ptr(g_reg), L.ptr(g_neg), L.ptr(g_pos), L.ptr(out), L.ptr(part), L.stream()), "dgx_centernet_losses")
    torch.cuda.synchronize()
    for t in (g_reg, g_neg, g_pos):
        assert bool((t[M:] == SENT).all()), "rows >= M written"
    return {"out": out[:5].cpu(), "g_reg": g_reg[:M].cpu(), "g_neg": g_neg[:M].cpu(), "g_pos": g_pos[:M].cpu()}


@pytest.mark.parametrize("name", list(R.CENTERNET_CASES))
def test_centernet_losses(name):
    c = R.CENTERNET_CASES[name]()
    ref = R.centernet_ref64(*R.centernet_args(c))
    got = run_centernet(c)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (name, k, "not finite")
    ratios = R.centernet_check({k: v.double() for k, v in got.items()}, ref)
    assert float(got["out"][4]) == float(ref["out"][4]), (name, "number of cared positives")
    report("centernet", name, ratios)


# ------------------------------------------------------------------ mask BCE
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_mask_bce_grid_stride_on_a_strided_view(dtype):
    """n = 1400 * 28 * 28 > 1024 * 1024: the block count is capped at 1024 and every thread's grid-stride loop runs four or five times, on the
    class-1 slice of a (R, 2, S, S) buffer (row_stride = 2 S S)."""
    from divergen_amd import _lib as L
    lib = L.lib()
    c = R.mask_case()
    full = c["full"].to(dtype)
    Rr, K, S, _ = full.shape
    inner, n = S * S, Rr * S * S
    x = full[:, c["cls"]].reshape(Rr, inner)
    ref = R.mask_bce_ref64(x, c["gt"])
    fd = full.to(DEV)
    gt = c["gt"].to(torch.uint8).reshape(-1).to(DEV)
    grad = torch.full((n + 256,), SENT, dtype=dtype, device=DEV)
    grad[:n] = float("nan")
    out = torch.full((5,), float("nan"), dtype=F32, device=DEV)
    nws = int(lib.dgx_mask_bce_workspace_floats(n))
    assert nws == 1024 * 5 and n > 1024 * 1024
    ws = torch.full((nws,), float("nan"), dtype=F32, device=DEV)
    view = fd[:, c["cls"]]
    code = L.DGX_BF16 if dtype == BF16 else L.DGX_F32
    L.check(lib.dgx_mask_bce(view.data_ptr(), K * inner, inner, L.ptr(gt), n, L.ptr(grad), L.ptr(out), L.ptr(ws), code, L.stream()), "dgx_mask_bce")
    torch.cuda.synchronize()
    o, gr = out.cpu(), grad.cpu()
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(gr.float()).all())
    assert bool((gr[n:].float() == SENT).all()), "gradient written behind n"
    b = R.mask_bounds(ref, dtype)
    ratios = {"loss": R.worst_ratio(o[:1].double(), ref["out"][:1], b["out"][:1]), "grad": R.worst_ratio(gr[:n].double(), ref["grad"], b["grad"])}
    assert o[1:].double().tolist() == ref["out"][1:].tolist(), ("counts", o.tolist(), ref["out"].tolist())
    report("mask", "R1400_S28_strided %s" % ("bf16" if dtype == BF16 else "f32"), ratios)
