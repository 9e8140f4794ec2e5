"""The norm and GELU kernels (csrc/layernorm.hip, csrc/groupnorm.hip, csrc/gelu.hip) through the C ABI against the float64 restatements
of tests/_norm_ref64.py: every output element finite and inside its a-priori bound, or exact where the contract is exact (zero rows of
padding tokens, gates closed for certain, signed zeros, untouched sentinels, refused calls) -- at every step of the NJ ladder, at
widths that leave tail lanes, past one grid sweep, in both window orders, on hard rows and groups, and once per family through the
Python wrappers of layers/norm_ops.py.  Every output buffer is pre-filled with NaN, every region the kernel must leave alone with
a sentinel.  Each test prints `RATIO <group> <case> <output>=<worst error / bound> ...` before it asserts (pytest -s shows them)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _norm_ref64 as R  # noqa: E402

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SENT = -7.5                  # exact in bf16; no output of these kernels takes this value over a whole region by accident
PAD = 3                      # sentinel rows behind every row buffer
TAIL = 64                    # sentinel floats behind every scratch buffer
NAN = float("nan")
DGX_ERR_BAD_ARG, DGX_ERR_UNSUPPORTED = -1, -2


def _dev(t, dtype=None):
    return None if t is None else (t.to(dtype) if dtype is not None else t).contiguous().to(DEV)


def _buf(rows, cols, dtype, live):
    """(rows + PAD, cols) buffer: NaN in the `live` first rows, the sentinel behind them"""
    b = torch.full((rows + PAD, cols) if cols else (rows + PAD,), SENT, dtype=dtype, device=DEV)
    b[:live] = NAN
    return b


def _scratch(n):
    b = torch.full((n + TAIL,), SENT, dtype=F32, device=DEV)
    b[:n] = NAN
    return b


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def report(group, what, ratios):
    print("RATIO %s %s %s" % (group, what, " ".join("%s=%.3f" % kv for kv in ratios.items())))
    assert all(v <= 1.0 for v in ratios.values()), (group, what, ratios)


def finite(what, **outs):
    for k, v in outs.items():
        assert bool(torch.isfinite(v.float()).all()), (what, k, "not finite")


def L_():
    from divergen_amd import _lib as L
    return L


# ================================================================================================ LayerNorm
@functools.lru_cache(maxsize=None)
def ln_setup(name, f32out=False):
    c = R.LN_CASES[name]()
    i = R.ln_inputs(c, F32 if f32out else BF16)
    fwd = R.ln_fwd_ref64(i["x"], c["gamma"], c["beta"], c["eps"], None if f32out else c["win"])
    return c, i, fwd


def _win_args(win):
    return tuple(win) if win is not None else (0, 0, 0, 0, 0)


def run_ln_fwd(c, i, f32out=False):
    L = L_()
    T, C, xd = c["T"], c["C"], c["xdtype"]
    tok = R.ln_layout(None if f32out else c["win"], T)
    rows = tok.numel()
    x, g, b = _dev(i["x"], xd), _dev(c["gamma"]), _dev(c["beta"])
    y = _buf(rows, C, F32 if f32out else BF16, rows)
    mean, rstd = _buf(T, 0, F32, T), _buf(T, 0, F32, T)
    if f32out:
        L.check(L.lib().dgx_layernorm_f32out_fwd(L.ptr(x), L.ptr(g), L.ptr(b), L.ptr(y), L.ptr(mean), L.ptr(rstd), T, C, c["eps"], L.dtype_code(x),
                                                 L.stream()), "dgx_layernorm_f32out_fwd")
    else:
        L.check(L.lib().dgx_layernorm_fwd(L.ptr(x), L.ptr(g), L.ptr(b), L.ptr(y), L.ptr(mean), L.ptr(rstd), T, C, c["eps"], *_win_args(c["win"]),
                                          L.dtype_code(x), L.stream()), "dgx_layernorm_fwd")
    torch.cuda.synchronize()
    return {"y_rows": y.cpu(), "mean": mean.cpu(), "rstd": rstd.cpu(), "tok": tok, "dev": (x, g, mean, rstd)}


def check_ln_fwd(group, what, c, i, fwd, got, ydtype):
    T, rows = c["T"], got["tok"].numel()
    bnd = R.ln_fwd_bounds(i["x"], c["gamma"], c["beta"], c["eps"], fwd, ydtype, got["tok"])
    for k, n in (("y_rows", rows), ("mean", T), ("rstd", T)):
        assert bool((got[k][n:].float() == SENT).all()), (what, k, "written past its rows")
    out = {"y_rows": got["y_rows"][:rows], "mean": got["mean"][:T], "rstd": got["rstd"][:T]}
    finite(what, **out)
    pad = got["tok"] < 0
    assert bool((out["y_rows"][pad].float() == 0).all()), (what, "rows of padding tokens must be zero")
    report(group, what, {k: R.worst_ratio(out[k], fwd[k], bnd[k]) for k in ("mean", "rstd", "y_rows")})


@pytest.mark.parametrize("name", list(R.LN_CASES))
def test_layernorm_forward(name):
    c, i, fwd = ln_setup(name)
    got = run_ln_fwd(c, i)
    check_ln_fwd("ln-fwd", name, c, i, fwd, got, BF16)


@pytest.mark.parametrize("name", list(R.LN_F32OUT_CASES))
def test_layernorm_f32out_forward(name):
    c, i, fwd = ln_setup(name, True)
    got = run_ln_fwd(c, i, f32out=True)
    check_ln_fwd("ln-f32out-fwd", name, c, i, fwd, got, F32)


def run_ln_bwd(c, i, mean, rstd, dres_mode, null_params=False, emit=None, f32out=False):
    """dres_mode: None, 'out' (its own buffer) or 'inplace' (dres aliases dx).  mean / rstd: CPU fp32.  emit = (ews, escale tensor or
    None): dgx_layernorm_bwd_emit with the case's geometry.  Returns CPU tensors and the return code."""
    L = L_()
    T, C, xd = c["T"], c["C"], c["xdtype"]
    win = None if f32out else c["win"]
    x, g = _dev(i["x"], xd), _dev(c["gamma"])
    if win is not None and win[3] > 0:                       # classic order: the padding tokens' rows hold NaN and must not be read
        tok = R.ln_layout(win, T)
        dyb = torch.full((tok.numel(), C), NAN)
        dyb[tok >= 0] = i["dy"][tok[tok >= 0]]
    elif win is not None:                                    # compact order: the T real rows only
        dyb = i["dy"][R.ln_layout(win, T)[:T]]
    else:
        dyb = i["dy"]
    dy = _dev(dyb, F32 if f32out else BF16)
    dx = _buf(T, C, xd, T)
    dres = None
    if dres_mode == "out":
        dres = _dev(i["dres"], xd)
    elif dres_mode == "inplace":
        dx[:T] = _dev(i["dres"], xd)
        dres = dx
    dg, db = _dev(c["dg0"]).clone(), _dev(c["db0"]).clone()
    nblk = L.lib().dgx_layernorm_bwd_blocks(T)
    assert nblk == R.ln_bwd_blocks(T)
    part = _scratch(nblk * 2 * C)
    m, r = _dev(mean.float()), _dev(rstd.float())
    pg, pb = (None, None) if null_params else (L.ptr(dg), L.ptr(db))
    em = None
    if f32out:
        rc = L.lib().dgx_layernorm_f32out_bwd(L.ptr(dy), L.ptr(x), L.ptr(m), L.ptr(r), L.ptr(g), L.ptr(dx), pg, pb, L.ptr(part), T, C,
                                              L.dtype_code(x), L.stream())
    elif emit is None:
        rc = L.lib().dgx_layernorm_bwd(L.ptr(dy), L.ptr(x), L.ptr(m), L.ptr(r), L.ptr(g), L.ptr(dres), L.ptr(dx), pg, pb, L.ptr(part), T, C,
                                       *_win_args(win), L.dtype_code(x), L.stream())
    else:
        ewin, esc = emit
        erows = R.ln_layout(ewin, T).numel() if ewin[3] > 0 else T
        em = _buf(erows, C, BF16, erows)
        rc = L.lib().dgx_layernorm_bwd_emit(L.ptr(dy), L.ptr(x), L.ptr(m), L.ptr(r), L.ptr(g), L.ptr(dres), L.ptr(dx), pg, pb, L.ptr(part), T, C,
                                            *_win_args(win), L.dtype_code(x), L.ptr(em), L.ptr(esc), *ewin, L.stream())
    torch.cuda.synchronize()
    return {"rc": rc, "dx": dx.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu(), "part": part, "emit": None if em is None else em.cpu(), "nblk": nblk}


def check_ln_bwd(group, what, c, got, ref, bnd):
    T, C = c["T"], c["C"]
    assert got["rc"] == 0, (what, got["rc"])
    assert bool((got["dx"][T:].float() == SENT).all()), (what, "dx written past T rows")
    assert bool((got["part"][got["nblk"] * 2 * C:] == SENT).all()), (what, "part written past nblk * 2 * C")
    out = {"dx": got["dx"][:T], "dgamma": got["dgamma"], "dbeta": got["dbeta"]}
    finite(what, **out)
    report(group, what, {k: R.worst_ratio(out[k], ref[k], bnd[k]) for k in ("dx", "dgamma", "dbeta")})


def ln_bwd_ref(c, i, fwd, dres_mode, own=False):
    dr = i["dres"] if dres_mode else None
    if own:                                                  # the product path: the reference's own float64 statistics, their error in the bound
        mean, rstd, se = fwd["mean"], fwd["rstd"], R.ln_stat_err(i["x"], c["eps"])
    else:
        mean, rstd, se = fwd["mean"].float(), fwd["rstd"].float(), None
    ref = R.ln_bwd_ref64(i["x"], i["dy"], mean, rstd, c["gamma"], dr, c["dg0"], c["db0"])
    return ref, R.ln_bwd_bounds(i["x"], i["dy"], mean, rstd, c["gamma"], dr, c["dg0"], c["db0"], ref, c["xdtype"], stat_err=se)


@pytest.mark.parametrize("name", [k for k in R.LN_CASES if k not in R.LN_SLOW_BWD])
def test_layernorm_backward(name):
    """twice: given the reference's mean / rstd rounded to fp32 (the backward alone), then given the kernel's own forward outputs (the
    product path); dres absent, out of place and in place (bit-identical)"""
    c, i, fwd = ln_setup(name)
    T, C = c["T"], c["C"]
    if C > R.LN_BWD_MAX_C:
        got = run_ln_bwd(c, i, fwd["mean"], fwd["rstd"], None)
        assert got["rc"] == DGX_ERR_BAD_ARG, (name, got["rc"])
        assert bool(torch.isnan(got["dx"][:T].float()).all()) and torch.equal(got["dgamma"], c["dg0"]) and bool(torch.isnan(got["part"][:-TAIL]).all())
        return
    modes = (None, "out", "inplace") if T < 1000 else ("out",)
    outs = {}
    for mode in modes:
        ref, bnd = ln_bwd_ref(c, i, fwd, mode)
        outs[mode] = run_ln_bwd(c, i, fwd["mean"], fwd["rstd"], mode)
        check_ln_bwd("ln-bwd", "%s dres=%s" % (name, mode), c, outs[mode], ref, bnd)
    if "inplace" in outs:
        assert torch.equal(_bits(outs["out"]["dx"]), _bits(outs["inplace"]["dx"])), (name, "dres in place differs from out of place")
    k = run_ln_fwd(c, i)
    ref, bnd = ln_bwd_ref(c, i, fwd, "out", own=True)
    check_ln_bwd("ln-bwd-own-stats", name, c, run_ln_bwd(c, i, k["mean"][:T], k["rstd"][:T], "out"), ref, bnd)


@pytest.mark.parametrize("name", list(R.LN_F32OUT_CASES))
def test_layernorm_f32out_backward(name):
    c, i, fwd = ln_setup(name, True)
    T, C = c["T"], c["C"]
    got = run_ln_bwd(c, i, fwd["mean"], fwd["rstd"], None, f32out=True)
    if C > R.LN_F32OUT_BWD_MAX_C:
        assert got["rc"] == DGX_ERR_BAD_ARG, (name, got["rc"])
        assert bool(torch.isnan(got["dx"][:T].float()).all()) and torch.equal(got["dgamma"], c["dg0"]) and bool(torch.isnan(got["part"][:-TAIL]).all())
        return
    ref, bnd = ln_bwd_ref(c, i, fwd, None)
    check_ln_bwd("ln-f32out-bwd", name, c, got, ref, bnd)


@pytest.mark.parametrize("name", ["win_2_10_13_ws7_s3_f32", "win_2_17_13_ws-7_s2_f32", "C260_T37_f32", "C384_T7_bf16"])
def test_layernorm_backward_emit_and_deferred_parameter_fold(name):
    """dgx_layernorm_bwd_emit: dx and the parameter gradients bit-identical to the plain entry; emit = bf16(scale[b] * dx AS STORED) in
    token and in classic window order (zero rows for the padding tokens).  dgamma = dbeta = NULL + dgx_layernorm_param_reduce_n /
    _reduce2: bit-identical to the single call's second stage."""
    L = L_()
    c, i, fwd = ln_setup(name)
    T, C = c["T"], c["C"]
    B, H, W = (c["win"][0], c["win"][1], c["win"][2]) if c["win"] else (1, 1, T)
    plain = run_ln_bwd(c, i, fwd["mean"], fwd["rstd"], "out")
    esc = torch.linspace(0.5, 1.75, B)
    for ewin in ((B, H, W, 0, 0), (B, H, W, 3, 1)):
        for scale in (None, esc):
            got = run_ln_bwd(c, i, fwd["mean"], fwd["rstd"], "out", emit=(ewin, _dev(scale)))
            what = "%s emit ws=%d scale=%s" % (name, ewin[3], scale is not None)
            assert got["rc"] == 0
            for k in ("dx", "dgamma", "dbeta"):
                assert torch.equal(_bits(got[k]), _bits(plain[k])), (what, k, "differs from dgx_layernorm_bwd")
            tok = R.ln_layout(ewin, T)
            stored = got["dx"][:T].double()
            s = torch.ones(T, dtype=F64) if scale is None else scale.double().repeat_interleave(H * W)
            want = R.ln_place(stored * s[:, None], tok)
            # one fp32 product and the bf16 rounding of it
            e = R.U32 * want.abs()
            bnd = R.ln_place(torch.ones(T, C, dtype=F64), tok) * (e + R.stor(want, e, BF16))
            em = got["emit"]
            assert bool((em[tok.numel():].float() == SENT).all()), (what, "emit written past its rows")
            finite(what, emit=em[:tok.numel()])
            report("ln-bwd-emit", what, {"emit": R.worst_ratio(em[:tok.numel()], want, bnd)})
    # the deferred second stage
    a = run_ln_bwd(c, i, fwd["mean"], fwd["rstd"], "out", null_params=True)
    assert a["rc"] == 0 and torch.equal(a["dgamma"], c["dg0"]) and torch.equal(_bits(a["dx"]), _bits(plain["dx"]))
    dgs = [_dev(c["dg0"]).clone() for _ in range(5)]
    dbs = [_dev(c["db0"]).clone() for _ in range(5)]
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    L.check(L.lib().dgx_layernorm_param_reduce_n(arr([a["part"]] * 2), arr(dgs[:2]), arr(dbs[:2]), 2, T, C, L.stream()), "dgx_layernorm_param_reduce_n")
    L.check(L.lib().dgx_layernorm_param_reduce2(L.ptr(a["part"]), L.ptr(dgs[2]), L.ptr(dbs[2]), L.ptr(a["part"]), L.ptr(dgs[3]), L.ptr(dbs[3]), T, C,
                                                L.stream()), "dgx_layernorm_param_reduce2")
    L.check(L.lib().dgx_layernorm_param_reduce2(L.ptr(a["part"]), L.ptr(dgs[4]), L.ptr(dbs[4]), L.ptr(a["part"]), L.ptr(dgs[4]), L.ptr(dbs[4]), 0, C,
                                                L.stream()), "dgx_layernorm_param_reduce2 (T = 0: nothing to do)")
    torch.cuda.synchronize()
    for k in range(4):
        assert torch.equal(_bits(dgs[k].cpu()), _bits(plain["dgamma"])) and torch.equal(_bits(dbs[k].cpu()), _bits(plain["dbeta"])), (name, k)
    assert torch.equal(dgs[4].cpu(), c["dg0"]) and torch.equal(dbs[4].cpu(), c["db0"])


# ================================================================================================ patch merge + LayerNorm
@functools.lru_cache(maxsize=None)
def pm_setup(name):
    c = R.PM_CASES[name]()
    B, H, W, C0 = c["geom"]
    x, dy = R.as_read(c["x"], c["xdtype"]), R.as_read(c["dy"], BF16)
    xm = R.pm_gather(x, B, H, W)
    return c, x, dy, xm, R.ln_fwd_ref64(xm, c["gamma"], c["beta"], c["eps"])


def pm_bwd_ref(c, dy, xm, fwd, own=False):
    B, H, W, C0 = c["geom"]
    if own:
        mean, rstd, se = fwd["mean"], fwd["rstd"], R.ln_stat_err(xm, c["eps"])
    else:
        mean, rstd, se = fwd["mean"].float(), fwd["rstd"].float(), None
    ref = R.ln_bwd_ref64(xm, dy, mean, rstd, c["gamma"], None, c["dg0"], c["db0"])
    bnd = R.ln_bwd_bounds(xm, dy, mean, rstd, c["gamma"], None, c["dg0"], c["db0"], ref, c["xdtype"], stat_err=se, waves=R.pm_waves(C0))
    return dict(ref, dx=R.pm_scatter(ref["dx"], B, H, W)), dict(bnd, dx=R.pm_scatter(bnd["dx"], B, H, W))


@pytest.mark.parametrize("name", list(R.PM_CASES))
def test_patch_merge_layernorm(name):
    L = L_()
    c, x, dy, xm, fwd = pm_setup(name)
    B, H, W, C0 = c["geom"]
    T2, C, xd = xm.shape[0], 4 * C0, c["xdtype"]
    xg, g, b = _dev(x, xd), _dev(c["gamma"]), _dev(c["beta"])
    y, mean, rstd = _buf(T2, C, BF16, T2), _buf(T2, 0, F32, T2), _buf(T2, 0, F32, T2)
    L.check(L.lib().dgx_patch_merge_ln_fwd(L.ptr(xg), L.ptr(g), L.ptr(b), L.ptr(y), L.ptr(mean), L.ptr(rstd), B, H, W, C0, c["eps"], L.dtype_code(xg),
                                           L.stream()), "dgx_patch_merge_ln_fwd")
    torch.cuda.synchronize()
    for k, t in (("y", y), ("mean", mean), ("rstd", rstd)):
        assert bool((t[T2:].float() == SENT).all()), (name, k, "written past its rows")
    out = {"y": y[:T2].cpu(), "mean": mean[:T2].cpu(), "rstd": rstd[:T2].cpu()}
    finite(name, **out)
    bnd = R.ln_fwd_bounds(xm, c["gamma"], c["beta"], c["eps"], fwd, BF16)
    report("pm-fwd", name, {k: R.worst_ratio(out[k], fwd[k], bnd[k]) for k in ("mean", "rstd", "y")})
    nblk = L.lib().dgx_layernorm_bwd_blocks(T2)
    dyg = _dev(dy, BF16)
    for own in (False, True):
        m, r = (mean[:T2].clone(), rstd[:T2].clone()) if own else (_dev(fwd["mean"].float()), _dev(fwd["rstd"].float()))
        dx = _buf(B * H * W, C0, xd, B * H * W)             # (there is no padding in dx: the end of the buffer is what can be overrun)
        dg, db, part = _dev(c["dg0"]).clone(), _dev(c["db0"]).clone(), _scratch(nblk * 2 * C)
        L.check(L.lib().dgx_patch_merge_ln_bwd(L.ptr(dyg), L.ptr(xg), L.ptr(m), L.ptr(r), L.ptr(g), L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(part), B, H, W,
                                               C0, L.dtype_code(xg), L.stream()), "dgx_patch_merge_ln_bwd")
        torch.cuda.synchronize()
        assert bool((dx[B * H * W:].float() == SENT).all()) and bool((part[nblk * 2 * C:] == SENT).all()), (name, "written past the end")
        o = {"dx": dx[:B * H * W].cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()}
        finite(name, **o)
        ref, bb = pm_bwd_ref(c, dy, xm, fwd, own)
        report("pm-bwd-own-stats" if own else "pm-bwd", name, {k: R.worst_ratio(o[k], ref[k], bb[k]) for k in ("dx", "dgamma", "dbeta")})


# ================================================================================================ GroupNorm
@functools.lru_cache(maxsize=None)
def gn_setup(name, relu):
    c = R.GN_CASES[name]()
    x, dy = R.gn_inputs(c)
    return c, x, dy, R.gn_fwd_ref64(x, c["gamma"], c["beta"], c["G"], c["eps"], relu)


def run_gn_fwd(x, gamma, beta, G, eps, relu):
    L = L_()
    N, HW, C = x.shape
    xg, g, b = _dev(x, BF16), _dev(gamma), _dev(beta)
    y = _buf(N * HW, C, BF16, N * HW)
    mean, rstd = _buf(N * G, 0, F32, N * G), _buf(N * G, 0, F32, N * G)
    ns = int(L.lib().dgx_groupnorm_scratch_floats(N, HW, G))
    assert ns == N * G * (R.gn_slabs(N, HW, G) * 18 + 18)
    scratch = _scratch(ns)
    rc = L.lib().dgx_groupnorm_fwd(L.ptr(xg), L.ptr(g), L.ptr(b), L.ptr(y), L.ptr(mean), L.ptr(rstd), L.ptr(scratch), N, HW, C, G, eps, relu, L.stream())
    torch.cuda.synchronize()
    return {"rc": rc, "y": y, "mean": mean, "rstd": rstd, "scratch": scratch, "ns": ns}


def run_gn_bwd(x, dy, mean, rstd, gamma, beta, G, relu, dg0, db0):
    L = L_()
    N, HW, C = x.shape
    xg, dyg, g, b = _dev(x, BF16), _dev(dy, BF16), _dev(gamma), _dev(beta)
    dx = _buf(N * HW, C, BF16, N * HW)
    dg, db = _dev(dg0).clone(), _dev(db0).clone()
    ns = int(L.lib().dgx_groupnorm_scratch_floats(N, HW, G))
    part = _scratch(ns)
    m, r = _dev(mean.float()), _dev(rstd.float())
    rc = L.lib().dgx_groupnorm_bwd(L.ptr(xg), L.ptr(dyg), L.ptr(m), L.ptr(r), L.ptr(g), L.ptr(b), L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(part), N, HW, C,
                                   G, relu, L.stream())
    torch.cuda.synchronize()
    return {"rc": rc, "dx": dx, "dgamma": dg, "dbeta": db, "part": part, "ns": ns}


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("name", list(R.GN_CASES))
def test_groupnorm_forward_and_backward(name, relu):
    c, x, dy, fwd = gn_setup(name, relu)
    N, HW, C = x.shape
    G, what = c["G"], "%s relu%d" % (name, relu)
    k = run_gn_fwd(x, c["gamma"], c["beta"], G, c["eps"], relu)
    assert k["rc"] == 0
    assert bool((k["y"][N * HW:].float() == SENT).all()) and bool((k["mean"][N * G:] == SENT).all()) and bool((k["rstd"][N * G:] == SENT).all())
    assert bool((k["scratch"][k["ns"]:] == SENT).all()), (what, "scratch written past dgx_groupnorm_scratch_floats")
    out = {"y": k["y"][:N * HW].cpu().reshape(N, HW, C), "mean": k["mean"][:N * G].cpu().reshape(N, G), "rstd": k["rstd"][:N * G].cpu().reshape(N, G)}
    finite(what, **out)
    bnd = R.gn_fwd_bounds(x, c["gamma"], c["beta"], G, c["eps"], relu, fwd)
    if relu:
        assert float(out["y"][:, :, 3].float().abs().max()) == 0.0, (what, "gamma = 0, beta < 0: closed for certain")
    report("gn-fwd", what, {key: R.worst_ratio(out[key], fwd[key], bnd[key]) for key in ("mean", "rstd", "y")})
    # backward, given the reference's statistics rounded to fp32
    mean, rstd = fwd["mean"].float(), fwd["rstd"].float()
    ref = R.gn_bwd_ref64(x, dy, mean, rstd, c["gamma"], c["beta"], G, relu, c["dg0"], c["db0"])
    t = R.gn_bwd_terms(x, dy, mean, rstd, c["gamma"], c["beta"], G, relu)
    assert t["either_way"] <= R.either_way_cap(x.numel())
    pb = R.gn_param_bounds([t], c["dg0"], c["db0"])
    g = run_gn_bwd(x, dy, mean, rstd, c["gamma"], c["beta"], G, relu, c["dg0"], c["db0"])
    assert g["rc"] == 0
    assert bool((g["dx"][N * HW:].float() == SENT).all()) and bool((g["part"][g["ns"]:] == SENT).all()), (what, "written past the end")
    o = {"dx": g["dx"][:N * HW].cpu().reshape(N, HW, C), "dgamma": g["dgamma"].cpu(), "dbeta": g["dbeta"].cpu()}
    finite(what, **o)
    report("gn-bwd", what, {"dx": R.worst_ratio(o["dx"], ref["dx"], t["dx"]), "dgamma": R.worst_ratio(o["dgamma"], ref["dgamma"], pb["dgamma"]),
                            "dbeta": R.worst_ratio(o["dbeta"], ref["dbeta"], pb["dbeta"])})


def test_groupnorm_refuses_more_than_256_groups_before_any_launch():
    """G = 257: DGX_ERR_UNSUPPORTED with every output and scratch buffer still holding its sentinel"""
    L = L_()
    G, N, HW = R.GN_REFUSED_G, 1, 9
    C = 8 * G
    x = torch.zeros(N, HW, C, dtype=BF16, device=DEV)
    g, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    ns = int(L.lib().dgx_groupnorm_scratch_floats(N, HW, G))
    mk = lambda n, dt=F32: torch.full((n,), SENT, dtype=dt, device=DEV)
    y, mean, rstd, scratch = mk(N * HW * C, BF16), mk(N * G), mk(N * G), mk(ns + TAIL)
    rc = L.lib().dgx_groupnorm_fwd(L.ptr(x), L.ptr(g), L.ptr(b), L.ptr(y), L.ptr(mean), L.ptr(rstd), L.ptr(scratch), N, HW, C, G, 1e-5, 1, L.stream())
    torch.cuda.synchronize()
    assert rc == DGX_ERR_UNSUPPORTED
    for k, t in (("y", y), ("mean", mean), ("rstd", rstd), ("scratch", scratch)):
        assert bool((t.float() == SENT).all()), ("forward", k, "written by a refused call")
    dx, dg, db, part = mk(N * HW * C, BF16), mk(C), mk(C), mk(ns + TAIL)
    m1, r1 = torch.zeros(N * G, device=DEV), torch.ones(N * G, device=DEV)
    rc = L.lib().dgx_groupnorm_bwd(L.ptr(x), L.ptr(x), L.ptr(m1), L.ptr(r1), L.ptr(g), L.ptr(b), L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(part), N, HW, C, G, 1,
                                   L.stream())
    torch.cuda.synchronize()
    assert rc == DGX_ERR_UNSUPPORTED
    for k, t in (("dx", dx), ("dgamma", dg), ("dbeta", db), ("part", part)):
        assert bool((t.float() == SENT).all()), ("backward", k, "written by a refused call")


@pytest.mark.parametrize("relu", [0, 1])
def test_groupnorm_multi(relu):
    """five tensors (the FPN levels of one tower layer) in one launch per pass; dgamma / dbeta summed over them"""
    L = L_()
    cs = R.gn_multi_case()
    n, G, C = len(cs), 32, 256
    g, b = _dev(cs[0]["gamma"]), _dev(cs[0]["beta"])
    items, keep, refs = (L.GnItem * n)(), [], []
    for j, c in enumerate(cs):
        x, dy = R.gn_inputs(c)
        N, HW, _ = x.shape
        ns = int(L.lib().dgx_groupnorm_scratch_floats(N, HW, G))
        d = {"x": _dev(x, BF16), "dy": _dev(dy, BF16), "y": _buf(N * HW, C, BF16, N * HW), "mean": _buf(N * G, 0, F32, N * G),
             "rstd": _buf(N * G, 0, F32, N * G), "scratch": _scratch(ns), "ns": ns}
        it = items[j]
        it.x, it.dy, it.out, it.mean, it.rstd, it.scratch = L.ptr(d["x"]), None, L.ptr(d["y"]), L.ptr(d["mean"]), L.ptr(d["rstd"]), L.ptr(d["scratch"])
        it.N, it.HW = N, HW
        keep.append(d)
        refs.append((c, x, dy, R.gn_fwd_ref64(x, c["gamma"], c["beta"], G, c["eps"], relu)))
    L.check(L.lib().dgx_groupnorm_fwd_multi(items, n, L.ptr(g), L.ptr(b), C, G, cs[0]["eps"], relu, L.stream()), "dgx_groupnorm_fwd_multi")
    torch.cuda.synchronize()
    worst = {"mean": 0.0, "rstd": 0.0, "y": 0.0}
    for d, (c, x, dy, fwd) in zip(keep, refs):
        N, HW, _ = x.shape
        assert bool((d["y"][N * HW:].float() == SENT).all()) and bool((d["mean"][N * G:] == SENT).all()) and bool((d["scratch"][d["ns"]:] == SENT).all())
        out = {"y": d["y"][:N * HW].cpu().reshape(N, HW, C), "mean": d["mean"][:N * G].cpu().reshape(N, G), "rstd": d["rstd"][:N * G].cpu().reshape(N, G)}
        finite("multi HW%d" % HW, **out)
        bnd = R.gn_fwd_bounds(x, c["gamma"], c["beta"], G, c["eps"], relu, fwd)
        for k in worst:
            worst[k] = max(worst[k], R.worst_ratio(out[k], fwd[k], bnd[k]))
    report("gn-multi-fwd", "relu%d" % relu, worst)
    # backward on the kernel's own statistics (the product path): the reference keeps its float64 ones, the bound carries their error
    dg, db = _dev(cs[0]["dg0"]).clone(), _dev(cs[0]["db0"]).clone()
    terms, want = [], []
    dgr, dbr = cs[0]["dg0"].double(), cs[0]["db0"].double()
    for j, (d, (c, x, dy, fwd)) in enumerate(zip(keep, refs)):
        N, HW, _ = x.shape
        d["dx"], d["part"] = _buf(N * HW, C, BF16, N * HW), _scratch(d["ns"])
        it = items[j]
        it.dy, it.out, it.scratch = L.ptr(d["dy"]), L.ptr(d["dx"]), L.ptr(d["part"])
        sb = R.gn_stats_bounds(x, G, c["eps"])
        o = R.gn_bwd_ref64(x, dy, fwd["mean"], fwd["rstd"], c["gamma"], c["beta"], G, relu)
        terms.append(R.gn_bwd_terms(x, dy, fwd["mean"], fwd["rstd"], c["gamma"], c["beta"], G, relu, stat_err=(sb["dmu"], sb["drs"])))
        dgr, dbr = dgr + o["dgs"], dbr + o["dbs"]
        want.append(o)
    L.check(L.lib().dgx_groupnorm_bwd_multi(items, n, L.ptr(g), L.ptr(b), L.ptr(dg), L.ptr(db), C, G, relu, L.stream()), "dgx_groupnorm_bwd_multi")
    torch.cuda.synchronize()
    assert sum(t["either_way"] for t in terms) <= R.either_way_cap(sum(o["dx"].numel() for o in want))
    wdx = 0.0
    for d, o, t in zip(keep, want, terms):
        rows = o["dx"].shape[0] * o["dx"].shape[1]
        assert bool((d["dx"][rows:].float() == SENT).all()) and bool((d["part"][d["ns"]:] == SENT).all())
        got = d["dx"][:rows].cpu().reshape(o["dx"].shape)
        finite("multi dx", dx=got)
        wdx = max(wdx, R.worst_ratio(got, o["dx"], t["dx"]))
    pb = R.gn_param_bounds(terms, cs[0]["dg0"], cs[0]["db0"])
    finite("multi", dgamma=dg, dbeta=db)
    report("gn-multi-bwd", "relu%d" % relu, {"dx": wdx, "dgamma": R.worst_ratio(dg.cpu(), dgr, pb["dgamma"]), "dbeta": R.worst_ratio(db.cpu(), dbr, pb["dbeta"])})


# ================================================================================================ GELU
def test_gelu_forward_every_finite_bf16_value():
    L = L_()
    x = R.gelu_all_values_case()["x"].reshape(-1)
    n = x.numel()
    assert n == 65280 and n % 8 == 0
    xg = _dev(x, BF16)
    y = torch.full((n + 8,), SENT, dtype=BF16, device=DEV)
    y[:n] = NAN
    L.check(L.lib().dgx_gelu_fwd(L.ptr(xg), L.ptr(y), n, L.stream()), "dgx_gelu_fwd")
    torch.cuda.synchronize()
    assert bool((y[n:].float() == SENT).all())
    got = y[:n].cpu()
    finite("gelu-fwd", y=got)
    ref = R.gelu_fwd_ref64(x)
    # (signed zeros compare by value: worst_ratio takes the difference)
    report("gelu-fwd", "all_bf16", {"y": R.worst_ratio(got, ref, R.gelu_fwd_bounds(x, ref))})


def test_gelu_forward_past_one_grid_sweep():
    """n = 8 (8192 * 256) + 8 zeros and ones: the last eight elements belong to the second trip of workgroup 0"""
    L = L_()
    n = R.GELU_SWEEP_N
    xg = (torch.arange(n, device=DEV) % 3 == 1).to(BF16)
    y = torch.full((n + 8,), SENT, dtype=BF16, device=DEV)
    y[:n] = NAN
    L.check(L.lib().dgx_gelu_fwd(L.ptr(xg), L.ptr(y), n, L.stream()), "dgx_gelu_fwd")
    torch.cuda.synchronize()
    assert bool((y[n:].float() == SENT).all())
    one = torch.ones(1)
    ref1 = R.gelu_fwd_ref64(one)
    b1 = R.gelu_fwd_bounds(one, ref1)
    yo, yz = y[:n][xg == 1].float(), y[:n][xg == 0].float()
    assert bool((yz == 0).all()), "gelu(0) must be 0"
    vals = torch.unique(yo).cpu()
    assert vals.numel() == 1, vals
    report("gelu-fwd", "sweep_n%d" % n, {"y": R.worst_ratio(vals, ref1, b1)})


@pytest.mark.parametrize("beta", R.GELU_BETAS)
@pytest.mark.parametrize("name", list(R.GELU_CASES))
def test_gelu_backward_and_bias_gradient(name, beta):
    L = L_()
    c = R.GELU_CASES[name]()
    x, dy = R.as_read(c["x"], BF16), R.as_read(c["dy"], BF16)
    M, N = x.shape
    xg, dyg = _dev(x, BF16), _dev(dy, BF16)
    slabs = R.gelu_slabs(M, N)
    nws = int(L.lib().dgx_gelu_bwd_workspace_bytes(M, N)) // 4
    assert nws == slabs * N
    bias0 = torch.linspace(-1.0, 1.0, N)
    outs = {}
    for with_bias in (True, False):
        dx = _buf(M, N, BF16, M)
        ws = _scratch(nws)
        bias = _dev(bias0).clone() if beta != 0.0 else torch.full((N,), NAN, device=DEV)
        untouched = torch.full((N,), SENT, device=DEV)
        L.check(L.lib().dgx_gelu_bwd_colsum(L.ptr(dyg), L.ptr(xg), L.ptr(dx), L.ptr(bias) if with_bias else None, M, N, beta, L.ptr(ws), L.stream()),
                "dgx_gelu_bwd_colsum")
        torch.cuda.synchronize()
        assert bool((dx[M:].float() == SENT).all()) and bool((ws[nws:] == SENT).all()) and bool((untouched == SENT).all())
        outs[with_bias] = (dx[:M].cpu(), bias.cpu(), ws[:nws].cpu().reshape(slabs, N))
    dxk, bias, wsk = outs[True]
    assert torch.equal(_bits(dxk), _bits(outs[False][0])), "dx depends on bias_grad being passed"
    finite(name, dx=dxk, bias=bias, workspace=wsk)
    rows = -(-M // slabs)
    empty = [s for s in range(slabs) if s * rows >= M]
    if name.startswith("slabs"):
        assert (slabs, rows, len(empty)) == (256, 17, 14)
    assert bool((wsk[empty] == 0).all()), "partial rows of empty slabs must be zero"
    ref = R.gelu_bwd_ref64(x, dy)
    want = R.gelu_bias_ref64(dxk, bias0, beta)              # defined on the kernel's own stored dx: only the summation chain is granted
    report("gelu-bwd", "%s beta%g" % (name, beta), {"dx": R.worst_ratio(dxk, ref, R.gelu_bwd_bounds(x, dy, ref)),
                                                    "bias": R.worst_ratio(bias, want, R.gelu_bias_bounds(dxk, bias0, beta, want))})


# ================================================================================================ the Python wrappers (autograd plumbing)
def _leaf(t, dtype=F32):
    return t.to(dtype).to(DEV).requires_grad_(True)


@pytest.mark.parametrize("which", ["layernorm_bf16", "layernorm_window_gather", "layernorm_f32out"])
def test_layernorm_wrappers_sit_under_the_same_bounds(which):
    from divergen_amd.layers import norm_ops as NO
    name = {"layernorm_bf16": "C260_T37_f32", "layernorm_window_gather": "win_2_10_13_ws7_s3_f32", "layernorm_f32out": "C96_T7_f32"}[which]
    f32out = which == "layernorm_f32out"
    c, i, fwd = ln_setup(name, f32out)
    T, C = c["T"], c["C"]
    x, w, b = _leaf(i["x"]), _leaf(c["gamma"]), _leaf(c["beta"])
    if which == "layernorm_window_gather":
        B, H, W, ws, shift = c["win"]
        y = NO.layernorm_window_gather(x.reshape(B, H * W, C), w, b, c["eps"], B, H, W, ws, shift)
        tok = R.ln_layout(c["win"], T)
        dyb = torch.randn(tok.numel(), C)                   # the padding rows' gradient is whatever the consumer left there: not read
        dyb[tok >= 0] = i["dy"][tok[tok >= 0]]
        dyg = _dev(dyb, BF16).reshape(y.shape)
    else:
        tok = torch.arange(T)
        y = (NO.layernorm_f32out if f32out else NO.layernorm_bf16)(x, w, b, c["eps"])
        dyg = _dev(i["dy"], F32 if f32out else BF16)
    y.backward(dyg)
    torch.cuda.synchronize()
    ydt = F32 if f32out else BF16
    assert y.dtype == ydt
    bnd = R.ln_fwd_bounds(i["x"], c["gamma"], c["beta"], c["eps"], fwd, ydt, tok)
    got = y.detach().reshape(-1, C).cpu()
    finite(which, y=got, dx=x.grad, dgamma=w.grad, dbeta=b.grad)
    z = torch.zeros(C)
    ref = R.ln_bwd_ref64(i["x"], i["dy"], fwd["mean"], fwd["rstd"], c["gamma"], None, z, z)
    bb = R.ln_bwd_bounds(i["x"], i["dy"], fwd["mean"], fwd["rstd"], c["gamma"], None, z, z, ref, F32, stat_err=R.ln_stat_err(i["x"], c["eps"]))
    report("wrapper", which, {"y": R.worst_ratio(got, R.ln_place(fwd["y"], tok), bnd["y_rows"]), "dx": R.worst_ratio(x.grad.cpu(), ref["dx"], bb["dx"]),
                              "dgamma": R.worst_ratio(w.grad.cpu(), ref["dgamma"], bb["dgamma"]),
                              "dbeta": R.worst_ratio(b.grad.cpu(), ref["dbeta"], bb["dbeta"])})


def test_patch_merge_wrapper_sits_under_the_same_bounds():
    from divergen_amd.layers import norm_ops as NO
    name = "B2_H7_W9_C48_f32"
    c, x0, dy, xm, fwd = pm_setup(name)
    B, H, W, C0 = c["geom"]
    x, w, b = _leaf(x0.reshape(B, H * W, C0)), _leaf(c["gamma"]), _leaf(c["beta"])
    y = NO.patch_merge_layernorm(x, w, b, c["eps"], B, H, W)
    y.backward(_dev(dy, BF16).reshape(y.shape))
    torch.cuda.synchronize()
    z = dict(c, dg0=torch.zeros(4 * C0), db0=torch.zeros(4 * C0))
    ref, bb = pm_bwd_ref(z, dy, xm, fwd, own=True)
    bnd = R.ln_fwd_bounds(xm, c["gamma"], c["beta"], c["eps"], fwd, BF16)
    finite(name, y=y, dx=x.grad, dgamma=w.grad, dbeta=b.grad)
    report("wrapper", "patch_merge_layernorm", {"y": R.worst_ratio(y.detach().reshape(-1, 4 * C0).cpu(), fwd["y"], bnd["y"]),
                                                "dx": R.worst_ratio(x.grad.reshape(-1, C0).cpu(), ref["dx"], bb["dx"]),
                                                "dgamma": R.worst_ratio(w.grad.cpu(), ref["dgamma"], bb["dgamma"]),
                                                "dbeta": R.worst_ratio(b.grad.cpu(), ref["dbeta"], bb["dbeta"])})


def _gn_wrapper_case(c, x, dy, relu, stats):
    G = c["G"]
    sb = R.gn_stats_bounds(x, G, c["eps"])
    o = R.gn_bwd_ref64(x, dy, stats["mean"], stats["rstd"], c["gamma"], c["beta"], G, relu)
    return o, R.gn_bwd_terms(x, dy, stats["mean"], stats["rstd"], c["gamma"], c["beta"], G, relu, stat_err=(sb["dmu"], sb["drs"]))


def test_groupnorm_wrappers_sit_under_the_same_bounds():
    from divergen_amd.layers import norm_ops as NO
    # one tensor: (2, 35, 32) as a 5 x 7 map
    c, x, dy, fwd = gn_setup("N2_HW35_G32", 1)
    N, HW, C = x.shape
    xl, w, b = _leaf(x.reshape(N, 5, 7, C), BF16), _leaf(c["gamma"]), _leaf(c["beta"])
    y = NO.groupnorm_relu(xl.permute(0, 3, 1, 2), w, b, c["G"], c["eps"], relu=True)
    y.backward(_dev(dy, BF16).reshape(N, 5, 7, C).permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    o, t = _gn_wrapper_case(c, x, dy, 1, fwd)
    z = torch.zeros(C)
    pb = R.gn_param_bounds([t], z, z)
    bnd = R.gn_fwd_bounds(x, c["gamma"], c["beta"], c["G"], c["eps"], 1, fwd)
    finite("groupnorm_relu", y=y, dx=xl.grad, dgamma=w.grad, dbeta=b.grad)
    report("wrapper", "groupnorm_relu", {"y": R.worst_ratio(y.detach().permute(0, 2, 3, 1).reshape(N, HW, C).cpu(), fwd["y"], bnd["y"]),
                                         "dx": R.worst_ratio(xl.grad.reshape(N, HW, C).cpu(), o["dx"], t["dx"]),
                                         "dgamma": R.worst_ratio(w.grad.cpu(), o["dgs"], pb["dgamma"]),
                                         "dbeta": R.worst_ratio(b.grad.cpu(), o["dbs"], pb["dbeta"])})
    # the five levels of one tower layer
    cs = R.gn_multi_case()
    w, b = _leaf(cs[0]["gamma"]), _leaf(cs[0]["beta"])
    leaves, ins, refs = [], [], []
    for cc in cs:
        x, dy = R.gn_inputs(cc)
        N, HW, C = x.shape
        side = int(round(HW ** 0.5))
        leaf = _leaf(x.reshape(N, side, side, C), BF16)
        leaves.append(leaf)
        ins.append(leaf.permute(0, 3, 1, 2))
        refs.append((cc, x, dy, side))
    ys = NO.groupnorm_relu_multi(ins, w, b, 32, cs[0]["eps"], relu=True)
    torch.autograd.backward(ys, [_dev(dy, BF16).reshape(x.shape[0], s, s, 256).permute(0, 3, 1, 2) for _, x, dy, s in refs])
    torch.cuda.synchronize()
    terms, dgr, dbr, wy, wdx = [], torch.zeros(256, dtype=F64), torch.zeros(256, dtype=F64), 0.0, 0.0
    for (cc, x, dy, s), y, leaf in zip(refs, ys, leaves):
        N, HW, C = x.shape
        fwd = R.gn_fwd_ref64(x, cc["gamma"], cc["beta"], 32, cc["eps"], 1)
        o, t = _gn_wrapper_case(cc, x, dy, 1, fwd)
        bnd = R.gn_fwd_bounds(x, cc["gamma"], cc["beta"], 32, cc["eps"], 1, fwd)
        finite("groupnorm_relu_multi", y=y, dx=leaf.grad)
        wy = max(wy, R.worst_ratio(y.detach().permute(0, 2, 3, 1).reshape(N, HW, C).cpu(), fwd["y"], bnd["y"]))
        wdx = max(wdx, R.worst_ratio(leaf.grad.reshape(N, HW, C).cpu(), o["dx"], t["dx"]))
        terms.append(t)
        dgr, dbr = dgr + o["dgs"], dbr + o["dbs"]
    z = torch.zeros(256)
    pb = R.gn_param_bounds(terms, z, z)
    report("wrapper", "groupnorm_relu_multi", {"y": wy, "dx": wdx, "dgamma": R.worst_ratio(w.grad.cpu(), dgr, pb["dgamma"]),
                                               "dbeta": R.worst_ratio(b.grad.cpu(), dbr, pb["dbeta"])})
