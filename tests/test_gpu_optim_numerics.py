"""The optimizer kernels (csrc/optim.hip) through the C ABI against the float64 restatements of tests/_optim_ref64.py: every element
of every output inside its a-priori bound, or exact where the contract is exact (bf16 shadow = round-to-nearest-even of the kernel's
own p, lr multiplier 0, found_inf, sentinels, the NaN rule) -- at the sizes at which each path of the kernels' loops first exists.
S = dgx_optim_grid_quads() is the number of quads one sweep of the capped grid covers; the AdamW kernel handles two quads per trip, so
  n4 <= S            one trip, the second quad's load clamped for every lane
  n4 = S + 37        the second quad live for 37 lanes
  n4 = 3 S + 37      a second trip with a partial second quad
and the SGD / sum-of-squares kernels enter their grid-stride loops again behind S / 1024 * 256 quads.  The dense reference is the
restatement in torch float64 ON THE DEVICE in chunks; the same restatement runs again on the CPU for the edges of every (trip, u)
region, every hard input, every segment boundary and 65 536 random elements, so no verdict rests on one library.  Output-only buffers
are pre-filled with NaN, 64 sentinels stand behind every array.  Each test prints `RATIO <kernel> <case> <output>=<worst error /
bound> ...` before it asserts (pytest -s shows them)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _optim_ref64 as R  # noqa: E402

DEV = "cuda"
F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64
SENT = -7.5
PAD = 64
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def grid_quads():
    from divergen_amd import _lib as L
    S = int(L.lib().dgx_optim_grid_quads())
    assert S >= 256 and S % 256 == 0
    return S


SIZES = {"1": lambda S: 1, "255": lambda S: 255, "256": lambda S: 256, "257": lambda S: 257, "S-1": lambda S: S - 1, "S": lambda S: S,
         "S+37": lambda S: S + 37, "2S+37": lambda S: 2 * S + 37, "3S+37": lambda S: 3 * S + 37}


def report(group, what, ratios, broken=()):
    print("RATIO %s %s %s" % (group, what, " ".join("%s=%.3f" % kv for kv in ratios.items())))
    assert not broken, (group, what, broken)
    assert all(v <= 1.0 for v in ratios.values()), (group, what, ratios)


def padded(t, n, dtype=F32, fill=None):
    """n elements (t, or `fill` for an output-only buffer) with PAD sentinels behind them"""
    buf = torch.full((n + PAD,), SENT, dtype=dtype, device=DEV)
    if t is not None:
        buf[:n] = t
    else:
        buf[:n] = fill
    return buf


def broken_tails(bufs, n):
    return [k for k, b in bufs.items() if b is not None and not bool((b[n:].float() == SENT).all())]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def device_args(case):
    seg = case["seg"]
    lr_scale = seg[1].to(DEV) if seg is not None else None
    seg_end = seg[0].to(DEV) if seg is not None else None
    flag = torch.zeros(1, dtype=torch.int32, device=DEV) if case["found_inf"] else None
    sd = case["hp"].get("scale_dev")
    sdev = torch.tensor([sd], dtype=F32, device=DEV) if sd is not None else None
    return lr_scale, seg_end, flag, sdev


def launch_adamw(case, bufs, flag_override=None):
    from divergen_amd import _lib as L
    hp = case["hp"]
    lr_scale, seg_end, flag, sdev = device_args(case)
    flag = flag_override if flag_override is not None else flag
    n = 4 * case["n4"]
    rc = L.lib().dgx_adamw_ema_step_scaled(L.ptr(bufs["p"]), L.ptr(bufs["g"]), L.ptr(bufs["m"]), L.ptr(bufs["v"]), L.ptr(bufs["ema"]),
                                           L.ptr(bufs["shadow"]), n, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"],
                                           hp["clip_value"], hp["grad_scale"], L.ptr(sdev), hp["step"], hp["ema_decay"], L.ptr(lr_scale),
                                           L.ptr(seg_end), 0 if lr_scale is None else lr_scale.numel(), L.ptr(flag), L.stream())
    torch.cuda.synchronize()
    return rc


def launch_sgd(case, bufs, flag_override=None):
    from divergen_amd import _lib as L
    hp = case["hp"]
    lr_scale, seg_end, flag, sdev = device_args(case)
    flag = flag_override if flag_override is not None else flag
    n = 4 * case["n4"]
    rc = L.lib().dgx_sgd_ema_step(L.ptr(bufs["p"]), L.ptr(bufs["g"]), L.ptr(bufs["buf"]), L.ptr(bufs["ema"]), L.ptr(bufs["shadow"]), n, hp["lr"],
                                  hp["momentum"], int(hp["nesterov"]), hp["weight_decay"], hp["clip_value"], hp["grad_scale"], L.ptr(sdev),
                                  hp["step"], hp["ema_decay"], L.ptr(lr_scale), L.ptr(seg_end), 0 if lr_scale is None else lr_scale.numel(),
                                  L.ptr(flag), L.stream())
    torch.cuda.synchronize()
    return rc


def make_bufs(kind, case):
    inp, n = case["inp"], 4 * case["n4"]
    bufs = {"p": padded(inp["p"], n), "g": padded(inp["g"], n), "ema": padded(inp["ema"], n) if inp.get("ema") is not None else None,
            "shadow": padded(None, n, BF16, NAN) if case["shadow"] else None}
    if kind == "adamw":
        bufs["m"], bufs["v"] = padded(inp["m"], n), padded(inp["v"], n)
    elif inp.get("buf") is not None:
        # step 1 writes the buffer without reading it: output-only there
        bufs["buf"] = padded(None, n, F32, NAN) if case["sc"].first else padded(inp["buf"], n)
    else:
        bufs["buf"] = None
    return bufs


def verdict(kind, what, case, bufs, sample=True, group=None):
    n, S = 4 * case["n4"], grid_quads()
    assert not broken_tails(bufs, n), (what, "sentinels overwritten", broken_tails(bufs, n))
    assert torch.equal(bits(bufs["g"][:n]), bits(case["inp"]["g"])), (what, "the gradient was written")
    got = {k: b[:n] for k, b in bufs.items() if b is not None and k != "g"}
    worst, broken = R.step_check(kind, case, got)
    ratios = dict(worst)
    if sample:
        idx = R.sample_indices(case, S).to(DEV)
        w2, b2 = R.step_check(kind, case, got, idx=idx, device="cpu")
        ratios.update({"cpu." + k: v for k, v in w2.items()})
        broken = broken + b2
    report(group or kind, what, ratios, broken)


# ------------------------------------------------------------------ AdamW
ADAMW_GRID = [(s, o) for s in ("1", "255", "256", "257", "S-1", "S", "S+37") for o in R.ADAMW_OPTION_SETS] + [("3S+37", "on")]


@pytest.mark.parametrize("size,optset", ADAMW_GRID, ids=["%s-%s" % so for so in ADAMW_GRID])
def test_adamw_one_step_every_element(size, optset):
    S = grid_quads()
    n4 = SIZES[size](S)
    case = R.adamw_case(torch.Generator(device=DEV).manual_seed(7000 + len(size) * 131 + n4 % 1000), n4, S, optset)
    bufs = make_bufs("adamw", case)
    assert launch_adamw(case, bufs) == 0
    verdict("adamw", "n4=%s %s" % (size, optset), case, bufs)


def test_adamw_five_steps_each_from_the_kernels_own_state():
    """n4 = S + 37, everything on: the reference restarts every step from the float32 state the kernel left, so the one-step bound
    holds at every step (and an error in the second quad's stores would carry into the next step's inputs and be seen there too)."""
    S = grid_quads()
    n4 = S + 37
    gen = torch.Generator(device=DEV).manual_seed(7700)
    case = R.adamw_case(gen, n4, S, "on")
    bufs = make_bufs("adamw", case)
    for step in range(1, 6):
        case["hp"]["step"] = step
        case["sc"] = R.adamw_scalars(case["hp"])
        if step > 1:
            g = torch.randn(4 * n4, generator=gen, device=DEV) * (3.0 / abs(case["sc"].gscale))
            for e, name in case["hard"].items():
                g[e] = case["inp"]["g"][e]
            case["inp"] = {"p": bufs["p"][:4 * n4].clone(), "g": g, "m": bufs["m"][:4 * n4].clone(), "v": bufs["v"][:4 * n4].clone(),
                           "ema": bufs["ema"][:4 * n4].clone()}
            bufs["g"][:4 * n4] = g
        assert launch_adamw(case, bufs) == 0
        verdict("adamw", "n4=S+37 on step%d" % step, case, bufs, sample=step == 5, group="adamw-trajectory")


# ------------------------------------------------------------------ SGD
SGD_GRID = [(s, o, st) for s in ("1", "257", "S+37", "2S+37") for o in R.SGD_OPTION_SETS for st in (1, 5)]


@pytest.mark.parametrize("size,optset,step", SGD_GRID, ids=["%s-%s-step%d" % t for t in SGD_GRID])
def test_sgd_one_step_every_element(size, optset, step):
    """step 1: the momentum buffer handed in is all NaN (the kernel must not read it) and every result is finite where the reference
    is; 'plain' = zero momentum with buf = NULL."""
    S = grid_quads()
    n4 = SIZES[size](S)
    case = R.sgd_case(torch.Generator(device=DEV).manual_seed(8000 + len(size) * 131 + n4 % 1000 + step), n4, S, optset, step)
    bufs = make_bufs("sgd", case)
    assert (bufs["buf"] is None) == (case["hp"]["momentum"] == 0.0)
    if step == 1 and bufs["buf"] is not None:
        assert bool(torch.isnan(bufs["buf"][:4 * n4]).all())
    assert launch_sgd(case, bufs) == 0
    verdict("sgd", "n4=%s %s step%d" % (size, optset, step), case, bufs)


# ------------------------------------------------------------------ found_inf
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_found_inf_set_leaves_every_array_bit_for_bit(kind):
    S = grid_quads()
    n4 = S + 37
    gen = torch.Generator(device=DEV).manual_seed(7800)
    case = R.adamw_case(gen, n4, S, "on") if kind == "adamw" else R.sgd_case(gen, n4, S, "mom", 5)
    bufs = make_bufs(kind, case)
    bufs["shadow"][:4 * n4] = case["inp"]["p"].to(BF16)
    keep = {k: b.clone() for k, b in bufs.items() if b is not None}
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    assert (launch_adamw if kind == "adamw" else launch_sgd)(case, bufs, flag_override=flag) == 0
    for k, b in keep.items():
        assert torch.equal(bits(bufs[k]), bits(b)), (kind, k, "written although found_inf is set")


# ------------------------------------------------------------------ full-model norm clip
def run_clip(g, gs, max_norm):
    from divergen_amd import _lib as L
    nws = int(L.lib().dgx_clip_coef_workspace_floats())
    ws = padded(None, nws, F32, NAN)
    out = padded(None, 2, F32, NAN)
    rc = L.lib().dgx_clip_coef_f32(L.ptr(g), g.numel(), gs, max_norm, L.ptr(ws), L.ptr(out), L.stream())
    torch.cuda.synchronize()
    assert bool((ws[nws:] == SENT).all()) and bool((out[2:] == SENT).all()), "clip_coef wrote behind its buffers"
    return rc, out[:2].clone()


CLIP_SIZES = {"1": 1, "255": 255, "1024*256-1": R.CLIP_BLOCKS * 256 - 1, "2*1024*256+37": 2 * R.CLIP_BLOCKS * 256 + 37}


@pytest.mark.parametrize("size", list(CLIP_SIZES))
def test_clip_coef_norm_and_coefficient(size):
    from divergen_amd import _lib as L
    assert int(L.lib().dgx_clip_coef_workspace_floats()) == R.CLIP_BLOCKS
    n4 = CLIP_SIZES[size]
    g = R.clip_case(torch.Generator(device=DEV).manual_seed(9000 + n4 % 1000), n4)
    g_cpu = g.cpu()
    ratios = {}
    for gs in (1.0, 1.0 / 65536, -0.5):
        # a max_norm on either side of the norm: the coefficient is below 1 for one of them
        for mx in (1.5, 1e12):
            rc, out = run_clip(g, gs, mx)
            assert rc == 0
            rc2, again = run_clip(g, gs, mx)
            assert torch.equal(bits(out), bits(again)), (size, gs, "two calls differ")
            assert bool(torch.isfinite(out).all()), (size, gs, out)
            for where, gg in (("", g), ("cpu.", g_cpu)):
                ref, bnd = R.clip_coef_ref64(gg, gs, mx)
                tag = "%sgs%g_mx%g" % (where, gs, mx)
                ratios["coef_" + tag] = R.worst_ratio(out[0].cpu(), ref["coef"].cpu(), bnd["coef"].cpu())
                ratios["norm_" + tag] = R.worst_ratio(out[1].cpu(), ref["norm"].cpu(), bnd["norm"].cpu())
    # a lognormal sum is carried by a handful of elements: put the weight on the very last quad (the partial last trip of the
    # grid-stride loop) and on the very first, so that a quad the loop misses cannot hide behind the rest
    for name, sl in (("last", slice(4 * n4 - 4, 4 * n4)), ("first", slice(0, 4))):
        heavy = g.clone()
        heavy[sl] = torch.tensor([3e11, -1e11, 2e11, 5e10], device=DEV)
        rc, out = run_clip(heavy, 1.0, 1.5)
        ref, bnd = R.clip_coef_ref64(heavy.cpu(), 1.0, 1.5)
        assert rc == 0
        ratios["coef_heavy_" + name] = R.worst_ratio(out[0].cpu(), ref["coef"], bnd["coef"])
        ratios["norm_heavy_" + name] = R.worst_ratio(out[1].cpu(), ref["norm"], bnd["norm"])
    report("clip_coef", "n4=%s" % size, ratios)
    bad = g.clone()
    bad[(4 * n4) // 2] = NAN
    rc, out = run_clip(bad, 1.0, 1.5)
    assert rc == 0 and bool(torch.isnan(out).all()), (size, "a NaN gradient element must give a NaN norm and a NaN coefficient", out)


# ------------------------------------------------------------------ dgx_zero_ranges_f32
def test_zero_ranges_exactly_the_ranges():
    from divergen_amd import _lib as L
    n = 4 * 65536
    gen = torch.Generator(device=DEV).manual_seed(9100)
    base = torch.randn(n, generator=gen, device=DEV) + 3.0
    base[8 + 65536 + 4:8 + 65536 + 8] = SENT                    # the 4-element gap between two ranges of 'mixed' holds the sentinel
    tables = {
        "mixed": [(0, 4), (4, 4), (8, 65536), (8 + 65536, 4), (8 + 65536 + 8, 4), (100000, 65536), (n - 4, 4)],      # adjacent ranges and gaps
        "one": [(1024, 65536)],
    }
    for name, table in tables.items():
        g = padded(base, n)
        tab = torch.tensor(table, dtype=I64, device=DEV)
        assert L.lib().dgx_zero_ranges_f32(L.ptr(g), L.ptr(tab), tab.shape[0], L.stream()) == 0
        torch.cuda.synchronize()
        want = padded(base, n)
        for a, c in table:
            want[a:a + c] = 0.0
        assert torch.equal(bits(g), bits(want)), name
    g = padded(base, n)
    assert L.lib().dgx_zero_ranges_f32(L.ptr(g), None, 0, L.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(g), bits(padded(base, n)))


# ------------------------------------------------------------------ argument checks
def test_bad_arguments_return_an_error_and_write_nothing():
    from divergen_amd import _lib as L
    lib, st = L.lib(), L.stream()
    n = 4 * 64
    gen = torch.Generator(device=DEV).manual_seed(9200)
    t = {k: torch.randn(n + PAD, generator=gen, device=DEV) for k in ("p", "g", "m", "v", "ema", "buf")}
    t["shadow"] = torch.randn(n + PAD, generator=gen, device=DEV).to(BF16)
    keep = {k: v.clone() for k, v in t.items()}
    lr_scale = torch.tensor([0.5, 1.0], dtype=F32, device=DEV)
    seg_end = torch.tensor([n // 2, n], dtype=I64, device=DEV)
    ws = torch.full((int(lib.dgx_clip_coef_workspace_floats()),), SENT, dtype=F32, device=DEV)
    out = torch.full((2,), SENT, dtype=F32, device=DEV)

    def adamw(n_, step, ls, se):
        return lib.dgx_adamw_ema_step_scaled(L.ptr(t["p"]), L.ptr(t["g"]), L.ptr(t["m"]), L.ptr(t["v"]), L.ptr(t["ema"]), L.ptr(t["shadow"]), n_,
                                             1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1.0, None, step, 0.999, L.ptr(ls), L.ptr(se), 2 if ls is not None else 0,
                                             None, st)

    def sgd(n_, step, ls, se, mom=0.9, nesterov=0):
        return lib.dgx_sgd_ema_step(L.ptr(t["p"]), L.ptr(t["g"]), L.ptr(t["buf"]), L.ptr(t["ema"]), L.ptr(t["shadow"]), n_, 0.02, mom, nesterov, 1e-3,
                                    1.0, 1.0, None, step, 0.999, L.ptr(ls), L.ptr(se), 2 if ls is not None else 0, None, st)

    bad = {"adamw n%4": adamw(n - 2, 3, None, None), "adamw step0": adamw(n, 0, None, None), "adamw lr_scale alone": adamw(n, 3, lr_scale, None),
           "adamw seg_end alone": adamw(n, 3, None, seg_end), "sgd n%4": sgd(n - 2, 3, None, None), "sgd step0": sgd(n, 0, None, None),
           "sgd lr_scale alone": sgd(n, 3, lr_scale, None), "sgd seg_end alone": sgd(n, 3, None, seg_end),
           "sgd nesterov without momentum": sgd(n, 3, None, None, mom=0.0, nesterov=1),
           "clip n%4": lib.dgx_clip_coef_f32(L.ptr(t["g"]), n - 2, 1.0, 1.5, L.ptr(ws), L.ptr(out), st),
           "clip max_norm 0": lib.dgx_clip_coef_f32(L.ptr(t["g"]), n, 1.0, 0.0, L.ptr(ws), L.ptr(out), st),
           "clip max_norm < 0": lib.dgx_clip_coef_f32(L.ptr(t["g"]), n, 1.0, -1.0, L.ptr(ws), L.ptr(out), st),
           "clip max_norm NaN": lib.dgx_clip_coef_f32(L.ptr(t["g"]), n, 1.0, NAN, L.ptr(ws), L.ptr(out), st)}
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad.values()), bad
    for k, v in keep.items():
        assert torch.equal(bits(t[k]), bits(v)), (k, "written by a refused call")
    assert bool((ws == SENT).all()) and bool((out == SENT).all())
