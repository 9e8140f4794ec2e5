"""GPU tests of the caption loss kernels (csrc/caption_loss.hip): dgx_caption_prepare + dgx_caption_loss through the C ABI against the
float64 restatement (tests/_caption_loss_ref.py), and the golden inputs against the reference's own fp32 outputs
(tests/golden/caption_loss.npz).

Tolerance.  |got - ref| <= rtol * max(|ref|, floor), floor = the restatement's sum of absolute addends per value (its docstring says how
the floor is carried through the chain).  tests/golden/make_golden_caption_loss.py measured the reference's OWN fp32 evaluation against
the restatement in that form at rtol = 1e-5, on the golden inputs and on the inputs of this file (_caption_loss_ref.GPU_CASES, values as
stored in fp32 and in bf16): worst ratio 0.0023 (loss), 0.0065 (du), 0.0020 (d cls_bias) on the golden inputs, 0.0034 / 0.025 / 0.0018 on
the inputs here (`measured.*` of the golden file).  The reference stays inside the bound, so rtol is 1e-5, the project's bound for fp32.
A bf16 gradient adds one bf16 rounding of the value, 2^-8 |ref|.  The loss, stats_l_caption and d cls_bias are fp32 in either dtype.
The chosen rows are compared exactly; the gradient outside the chosen rows, in pad rows and in pad columns is exactly zero in buffers
that were NaN-filled before the launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _caption_loss_ref as C  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
RTOL = 1e-5
GOLD = os.path.join(HERE, "golden", "caption_loss.npz")


def test_rtol_is_the_measured_one():
    """The bound of this file is the one the golden generator's measurement gives: the reference's fp32 evaluation inside 1e-5."""
    g = np.load(GOLD)
    assert max(g["measured.golden"].max(), g["measured.cases"].max()) <= 1.0 and RTOL == 1e-5


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def padded(a, ld, dtype):
    """(R, D) float32 numpy -> (R, ld) device tensor of `dtype`, pad columns NaN; and the values as stored, in float64."""
    R, D = a.shape
    t = torch.full((R, ld), float("nan"), dtype=dtype)
    t[:, :D] = T(a).to(dtype)
    return t.to(DEV), t[:, :D].double().numpy()


def run_kernel(u, valid, counts, cap, D, target0, temp, norm_weight, bias, neg_weight, scale, stat_scale, ld_du, upstream=None):
    """prepare + forward + gradient through the C ABI.  u (R_alloc, ld_u) and cap (N, ld_cap) device tensors.  Every output buffer is
    NaN-filled (sel: -7) before the launch.  -> out4, sel, du (R_alloc, ld_du), dbias, prepared rows, ws."""
    from divergen_amd import _lib as L
    lib = L.lib()
    R_alloc, ld_u = u.shape
    N, ld_cap = cap.shape
    B = len(counts)
    row0 = (ctypes.c_int * (B + 1))(*np.concatenate([[0], np.cumsum(counts)]).astype(int).tolist())
    prep = torch.full((N, D), float("nan"), device=DEV)
    L.check(lib.dgx_caption_prepare(L.ptr(cap), ld_cap, N, D, int(norm_weight), L.ptr(prep), L.stream()), "dgx_caption_prepare")
    out = torch.full((4,), float("nan"), device=DEV)
    sel = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((int(lib.dgx_caption_workspace_floats(B, N)),), float("nan"), device=DEV)
    du = torch.full((R_alloc, ld_du), float("nan"), dtype=u.dtype, device=DEV)
    db = torch.full((1,), float("nan"), device=DEV) if bias is not None else None
    head = (L.ptr(u), ld_u, R_alloc, L.ptr(valid), B, row0, L.ptr(prep), N, D, target0, float(temp), int(norm_weight), L.ptr(bias),
            float(neg_weight), float(scale), float(stat_scale))
    L.check(lib.dgx_caption_loss(*head, None, L.ptr(sel), L.ptr(out), L.ptr(ws), None, 0, None, L.dtype_code(u), L.stream()), "forward")
    L.check(lib.dgx_caption_loss(*head, L.ptr(upstream), L.ptr(sel), None, L.ptr(ws), L.ptr(du), ld_du, L.ptr(db), L.dtype_code(u),
                                 L.stream()), "gradient")
    torch.cuda.synchronize()
    return out, sel, du, db, prep, ws


def within(got, ref, floor, extra=0.0):
    return abs(got - ref) <= RTOL * max(abs(ref), floor) + extra


def check_against(res, r64, counts, D, dtype, what):
    out, sel, du, db, prep, ws = res
    assert sel.cpu().tolist() == r64["sel"], what + ": chosen rows"
    loss, stat = float(out[0]), float(out[1])
    print("%s: loss %.9g (float64 %.9g), stats_l_caption %.9g" % (what, loss, r64["loss"], stat))
    assert within(loss, r64["loss"], r64["floor_loss"]), what + ": loss"
    assert within(stat, r64["l_caption"], r64["floor_loss"] * abs(r64["l_caption"] / r64["loss"]) if r64["loss"] else 0.0), what + ": stats"
    assert out[2:].cpu().tolist() == [0.0, 0.0]
    d = du.float().cpu().numpy().astype(np.float64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    chosen = np.zeros(d.shape[0], bool)
    for b, s in enumerate(r64["sel"]):
        if s >= 0:
            chosen[off[b] + s] = True
    assert np.all(d[~chosen] == 0), what + ": rows that were not chosen (pad rows included)"
    assert np.all(d[:, D:] == 0), what + ": pad columns"
    ref, floor = r64["du"][:, :D], r64["floor_du"][:, :D]
    tol = RTOL * np.maximum(np.abs(ref), floor) + (2.0 ** -8 * np.abs(ref) if dtype == BF16 else 0.0)
    err = np.abs(d[:, :D] - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    print("%s: du worst ratio %.3g" % (what, float(ratio.max())))
    assert np.all(err <= tol), "%s: du worst ratio %.3g at %s" % (what, float(ratio.max()), np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    if db is not None:
        print("%s: dbias %.9g (float64 %.9g)" % (what, float(db), r64["dbias"]))
        assert within(float(db), r64["dbias"], r64["floor_dbias"]), what + ": d cls_bias"


_REF = {}


def _case(k, dtype):
    """Inputs as stored and the restatement on them, computed once per (case, dtype)."""
    key = (k, dtype)
    if key not in _REF:
        c = C.GPU_CASES[k]
        B, N, D, target0, lc, lu, bias, negw, norm_weight = c
        d = C.case_inputs(c, k)
        u_dev, u64 = padded(d["u"], D + lu, dtype)
        cap_dev, cap64 = padded(d["cap"], D + lc, torch.float32)
        if lc:
            cap_dev[:, D:] = float(target0 // B)            # the rank column: cut off by the prepare kernel
        scale, stat = C.scales(B)
        r64 = C.caption_loss(u64, d["valid"], d["counts"], cap64, D, target0, C.TEMP, norm_weight, bias, negw, scale, stat, ld_du=D + lu)
        _REF[key] = (d, u_dev, cap_dev, cap64, r64)
    return _REF[key]


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("k", range(len(C.GPU_CASES)), ids=[C.case_id(c) for c in C.GPU_CASES])
def test_caption_loss_against_float64(k, dtype):
    """Every case of _caption_loss_ref.GPU_CASES (an image without rows, one whose last two rows are invalid, one with every row invalid;
    the hard inputs: logits +-50 from a parallel / anti-parallel caption, an all-zero caption row, a positive and a negative with the
    same logit, rows of magnitude 1e-3 and 1e3): prepared rows, chosen rows, loss, stats_l_caption, the whole gradient buffer, d cls_bias;
    two runs bit-equal."""
    B, N, D, target0, lc, lu, bias, negw, norm_weight = C.GPU_CASES[k]
    d, u_dev, cap_dev, cap64, r64 = _case(k, dtype)
    valid = T(d["valid"]).to(DEV)
    bias_t = torch.tensor([bias], dtype=torch.float32, device=DEV) if bias is not None else None
    scale, stat = C.scales(B)
    args = (u_dev, valid, d["counts"], cap_dev, D, target0, C.TEMP, norm_weight, bias_t, negw, scale, stat, D + lu)
    res = run_kernel(*args)
    p64 = C.prepare(cap64, D, norm_weight)
    perr = np.abs(res[4].double().cpu().numpy() - p64)
    assert np.all(perr <= RTOL * np.abs(p64)), "prepared caption rows"
    check_against(res, r64, d["counts"], D, dtype, C.case_id(C.GPU_CASES[k]))
    again = run_kernel(*args)
    for a, b, name in zip(res, again, ("out4", "sel", "du", "dbias", "prepared", "ws")):
        if a is not None:
            assert torch.equal(a.view(torch.uint8) if a.dtype != torch.int32 else a, b.view(torch.uint8) if b.dtype != torch.int32 else b), \
                "two runs differ in " + name


def test_upstream_scalar_and_no_validity_bytes():
    """An upstream scalar on the device scales the gradient and d cls_bias; valid = NULL takes the last row of every image."""
    k = 4
    B, N, D, target0, lc, lu, bias, negw, norm_weight = C.GPU_CASES[k]
    d, u_dev, cap_dev, cap64, _ = _case(k, torch.float32)
    scale, stat = C.scales(B)
    u64 = u_dev[:, :D].double().cpu().numpy()
    r64 = C.caption_loss(u64, None, d["counts"], cap64, D, target0, C.TEMP, norm_weight, bias, negw, scale, stat, upstream=-2.5, ld_du=D + lu)
    assert r64["sel"] == [n - 1 for n in d["counts"]]
    up = torch.tensor([-2.5], device=DEV)
    bias_t = torch.tensor([bias], dtype=torch.float32, device=DEV)
    res = run_kernel(u_dev, None, d["counts"], cap_dev, D, target0, C.TEMP, norm_weight, bias_t, negw, scale, stat, D + lu, upstream=up)
    check_against(res, r64, d["counts"], D, torch.float32, "upstream -2.5, valid NULL")


def test_refused_calls_launch_nothing():
    """B > 32, D not a multiple of 8 or outside 8..4096, target0 + B > N, a NULL pointer: -1, the NaN-filled outputs untouched."""
    from divergen_amd import _lib as L
    lib = L.lib()
    D, N = 16, 4
    u = torch.zeros(40, D, device=DEV)
    cap = torch.zeros(N, D, device=DEV)
    out = torch.full((4,), float("nan"), device=DEV)
    sel = torch.full((40,), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((4096,), float("nan"), device=DEV)

    def call(B=2, D=D, N=N, target0=0, u_=u, cap_=cap, sel_=sel, ws_=ws):
        row0 = (ctypes.c_int * (B + 1))(*range(B + 1))
        return lib.dgx_caption_loss(L.ptr(u_), 16, 40, None, B, row0, L.ptr(cap_), N, D, target0, 50.0, 1, None, 1.0, 1.0, 1.0, None,
                                    L.ptr(sel_), L.ptr(out), L.ptr(ws_), None, 0, None, 0, L.stream())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    out.fill_(float("nan"))
    sel.fill_(-7)
    for kw in (dict(B=33), dict(D=12), dict(D=0), dict(D=4104), dict(target0=3), dict(target0=-1), dict(u_=None), dict(cap_=None),
               dict(sel_=None), dict(ws_=None), dict(N=0)):
        assert call(**kw) == -1, kw
    assert lib.dgx_caption_prepare(None, D, N, D, 1, L.ptr(cap), L.stream()) == -1
    assert lib.dgx_caption_prepare(L.ptr(cap), D, N, 12, 1, L.ptr(cap), L.stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and bool((sel == -7).all())


def test_golden_inputs_against_the_reference():
    """The golden inputs (tests/golden/caption_loss.npz) through the kernel: the reference's own projected rows u, its captions (plain and
    the gathered matrix of three ranks with the rank column, one rank all zeros) -> image_loss, stats_l_caption, the gradient of u and of
    cls_bias against the reference's fp32 outputs at the same rtol."""
    g = np.load(GOLD)
    d = C.golden_inputs()
    B, D = d["B"], d["D"]
    scale, stat = C.scales(B)
    bias_t = torch.tensor([d["use_bias"]], dtype=torch.float32, device=DEV)
    for name, cap, target0, negw in (("caption", d["cap"], 0, 1.0), ("synced", g["in.gathered"], B * d["rank"], C.NEG_CAP_WEIGHT)):
        u = g[name + ".u"]
        r64 = C.caption_loss(u, None, d["counts"], cap, D, target0, C.TEMP, True, d["use_bias"], negw, scale, stat)
        res = run_kernel(T(u).to(DEV), None, d["counts"], T(cap).to(DEV).contiguous(), D, target0, C.TEMP, True, bias_t, negw, scale, stat, D)
        out, sel, du, db = res[:4]
        assert within(float(out[0]), float(g[name + ".image_loss"]), r64["floor_loss"]), name
        assert within(float(out[1]), float(g[name + ".l_caption"]), r64["floor_loss"] / C.IMAGE_LOSS_WEIGHT), name
        assert sel.cpu().tolist() == [n - 1 for n in d["counts"]]
        ref = g[name + ".du"].astype(np.float64)
        err = np.abs(du.double().cpu().numpy() - ref)
        assert np.all(err <= RTOL * np.maximum(np.abs(ref), r64["floor_du"])), name + ": du against the reference"
        assert within(float(db), float(g[name + ".dbias"].reshape(-1)[0]), r64["floor_dbias"]), name + ": d cls_bias"
