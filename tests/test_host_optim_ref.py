"""tests/_optim_ref64.py (the float64 restatements of the optimizer kernels of csrc/optim.hip, their a-priori bounds, the shared cases and
the mutants that tests/test_gpu_optim_numerics.py holds the kernels to) checked on the host: the restatements against torch.optim and
oracle/solver.py in float64, a float32 CPU evaluation of the kernel's operation sequence inside every bound on every case, every
mutant outside one, the quad-wise segment lookup equal to the per-element one, and the arena invariant that makes the quad-wise lookup
right (solver.check_quad_multipliers)."""
import functools

import pytest
import torch

import _optim_ref64 as R

F32, F64, I64 = torch.float32, torch.float64, torch.int64
S_HOST = 64                                                       # quads per "grid sweep" of the host-sized cases
ADAMW_N4 = (1, 63, 64, 65, S_HOST + 37, 3 * S_HOST + 37)
SGD_N4 = (1, 65, S_HOST + 37, 2 * S_HOST + 37)
CLIP_BLOCKS_HOST = 2
CLIP_N4 = (1, 255, CLIP_BLOCKS_HOST * 256 - 1, 2 * CLIP_BLOCKS_HOST * 256 + 37)
CLIP_SCALES = (1.0, 1.0 / 65536, -0.5)
K_HYPER = 64            # the torch comparisons: 64 u of the tensor's largest magnitude -- torch forms lr * 0.1, 1 - lr * wd, the bias
#                         corrections and the clip coefficient in double, the restatement in float32 as the kernel does (a handful of
#                         relative errors of u each, carried over five steps)


def close(a, b, k=K_HYPER):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= k * R.U * float(b.abs().max())


@functools.lru_cache(maxsize=None)
def adamw_case(n4, optset):
    return R.adamw_case(torch.Generator().manual_seed(1000 + n4), n4, S_HOST, optset)


@functools.lru_cache(maxsize=None)
def sgd_case(n4, optset, step):
    return R.sgd_case(torch.Generator().manual_seed(2000 + n4 + step), n4, S_HOST, optset, step)


def all_cases():
    for n4 in ADAMW_N4:
        for o in R.ADAMW_OPTION_SETS:
            yield "adamw", "n4=%d %s" % (n4, o), adamw_case(n4, o)
    for n4 in SGD_N4:
        for o in R.SGD_OPTION_SETS:
            for step in (1, 5):
                yield "sgd", "n4=%d %s step%d" % (n4, o, step), sgd_case(n4, o, step)


# ------------------------------------------------------------------ the restatements are right
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, clip_value=1.0, grad_scale=1.0, scale_dev=None, ema_decay=0.999)


def _f32d(x):
    return R.f32v(x)


@pytest.mark.parametrize("clip", ["value", "norm"])
def test_adamw_ref64_equals_torch_adamw_in_float64(clip):
    """torch.optim.AdamW behind clip_grad_value_ (maybe_add_gradient_clipping) or clip_grad_norm_ (FullModelGradientClippingOptimizer,
    its coefficient from clip_coef_ref64), five steps in float64 with the float32-rounded hyper-parameters."""
    g = torch.Generator().manual_seed(11)
    n = 4 * 300
    a = torch.nn.Parameter(torch.randn(n, generator=g, dtype=F64))
    opt = torch.optim.AdamW([a], lr=_f32d(HP["lr"]), betas=(_f32d(0.9), _f32d(0.999)), eps=_f32d(1e-8), weight_decay=_f32d(1e-2), foreach=False)
    p, m, v = a.detach().clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in range(1, 6):
        gr = torch.randn(n, generator=g, dtype=F64) * (0.01 if step == 3 else 3.0)
        a.grad = gr.clone()
        hp = dict(HP, step=step)
        if clip == "value":
            torch.nn.utils.clip_grad_value_([a], 1.0)
        else:
            total = torch.nn.utils.clip_grad_norm_([a], 1.5)
            c, _ = R.clip_coef_ref64(gr, 1.0, 1.5)
            assert close(c["norm"], total, 4) and close(c["coef"], min(1.0, 1.5 / (float(total) + 1e-6)), 4)
            hp.update(clip_value=0.0, scale_dev=float(c["coef"]))
        opt.step()
        out, _ = R.adamw_ref64(p, gr, m, v, None, None, R.adamw_scalars(hp))
        p, m, v = out["p"], out["m"], out["v"]
    assert close(p, a.detach()) and close(m, opt.state[a]["exp_avg"]) and close(v, opt.state[a]["exp_avg_sq"])


@pytest.mark.parametrize("momentum,nesterov", [(0.9, False), (0.9, True), (0.0, False)])
def test_sgd_ref64_equals_torch_sgd_two_groups_in_float64(momentum, nesterov):
    g = torch.Generator().manual_seed(13)
    n0, n1 = 4 * 30, 4 * 70
    a0 = torch.nn.Parameter(torch.randn(n0, generator=g, dtype=F64))
    a1 = torch.nn.Parameter(torch.randn(n1, generator=g, dtype=F64))
    lr, wd = _f32d(0.02), _f32d(1e-3)
    opt = torch.optim.SGD([{"params": [a0], "lr": lr * 0.1}, {"params": [a1], "lr": lr}], lr, momentum=_f32d(momentum), nesterov=nesterov,
                          weight_decay=wd, foreach=False)
    seg = (torch.tensor([n0, n0 + n1], dtype=I64), torch.tensor([0.1, 1.0], dtype=F32))
    mult = R.element_multipliers(torch.arange(n0 + n1), seg)
    p = torch.cat([a0.detach(), a1.detach()]).clone()
    buf = torch.full_like(p, float("nan")) if momentum else None            # step 1 must not read it
    ema, ema_t = p.clone() + 0.5, p.clone() + 0.5
    for step in range(1, 6):
        gr = torch.randn(n0 + n1, generator=g, dtype=F64) * 3
        ema_t = ema_t * _f32d(0.999) + (1.0 - _f32d(0.999)) * torch.cat([a0.detach(), a1.detach()])
        a0.grad, a1.grad = gr[:n0].clone(), gr[n0:].clone()
        torch.nn.utils.clip_grad_value_([a0, a1], 1.0)
        opt.step()
        sc = R.sgd_scalars(dict(lr=0.02, momentum=momentum, nesterov=nesterov, weight_decay=1e-3, clip_value=1.0, grad_scale=1.0, scale_dev=None,
                                ema_decay=0.999, step=step))
        out, _ = R.sgd_ref64(p, gr, buf, ema, mult, sc)
        p, ema, buf = out["p"], out["ema"], out.get("buf")
    assert close(p, torch.cat([a0.detach(), a1.detach()])) and close(ema, ema_t)
    if momentum:
        assert close(buf, torch.cat([opt.state[a0]["momentum_buffer"], opt.state[a1]["momentum_buffer"]]))


def test_adamw_ref64_equals_the_oracle_solver_in_float64():
    from oracle import solver as OS
    g = torch.Generator().manual_seed(17)
    n = 4 * 250
    p0 = torch.randn(n, generator=g, dtype=F64)
    p, m, v, ema = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), p0.clone()
    q, qm, qv, qe = p0.clone(), m.clone(), v.clone(), p0.clone()
    for step in range(1, 6):
        gr = torch.randn(n, generator=g, dtype=F64) * 3
        OS.ema_update(ema, p, _f32d(0.999))
        OS.adamw_clip_step(p, gr, m, v, step, _f32d(1e-3), _f32d(0.9), _f32d(0.999), _f32d(1e-8), _f32d(1e-4), 1.0)
        out, _ = R.adamw_ref64(q, gr, qm, qv, qe, None, R.adamw_scalars(dict(HP, weight_decay=1e-4, step=step)))
        q, qm, qv, qe = out["p"], out["m"], out["v"], out["ema"]
    assert close(q, p) and close(qm, m) and close(qv, v) and close(qe, ema)


# ------------------------------------------------------------------ the bounds hold for a correct float32 evaluation, and only for one
def _verdict(kind, case, mutant=None):
    got = R.step_f32(kind, case, S_HOST, mutant)
    worst, broken = R.step_check(kind, case, got)
    return worst, broken


def test_float32_evaluation_stays_inside_every_bound_on_every_case():
    top = {}
    for kind, what, case in all_cases():
        worst, broken = _verdict(kind, case)
        assert not broken, (kind, what, broken)
        assert all(v <= 1.0 for v in worst.values()), (kind, what, worst)
        for k, v in worst.items():
            top[(kind, k)] = max(top.get((kind, k), 0.0), v)
    for (kind, k), v in sorted(top.items()):
        print("RATIO host-f32 %s %s=%.3f" % (kind, k, v))
    assert min(top.values()) > 0.02, ("a bound nobody comes near checks nothing", top)


def test_nan_rule_and_hard_inputs_are_in_the_cases():
    c = adamw_case(3 * S_HOST + 37, "on")
    names = set(c["hard"].values())
    assert {"nan", "+inf|1e15", "1e-30", "v0_g0", "p+1e6", "+clip(1+2^-23)"} <= names
    assert sorted(e for e in c["hard"] if e % (4 * S_HOST) == 0) == [0, 4 * S_HOST, 8 * S_HOST, 12 * S_HOST]      # one block per (trip, u) region
    nan_at = [e for e, k in c["hard"].items() if k == "nan"]
    ref, _ = R.adamw_ref64(c["inp"]["p"], c["inp"]["g"], c["inp"]["m"], c["inp"]["v"], c["inp"]["ema"], None, c["sc"])
    for k in ("p", "m", "v"):
        assert bool(torch.isnan(ref[k][nan_at]).all()) and int(torch.isnan(ref[k]).sum()) == len(nan_at)
    assert bool(torch.isfinite(ref["ema"]).all())
    inf_at = [e for e, k in c["hard"].items() if k == "+inf|1e15"]
    assert bool(torch.isinf(c["inp"]["g"][inf_at]).all()) and bool(torch.isfinite(ref["p"][inf_at]).all())
    seg_end, lr_scale = c["seg"]
    assert seg_end.numel() == min(400, 3 * S_HOST + 37)
    big = R.make_segments(torch.Generator().manual_seed(5), 5000, 1024, "full")[0]
    assert big.numel() == 400 and 4 * 1024 in big.tolist() and 8 * 1024 in big.tolist() and int(big[-1]) == 4 * 5000
    assert 4 * S_HOST in seg_end.tolist() and 8 * S_HOST in seg_end.tolist() and 0.0 in lr_scale.tolist() and 1.0 in lr_scale.tolist()
    assert bool((seg_end % 4 == 0).all()) and bool((seg_end[1:] > seg_end[:-1]).all())
    short = adamw_case(3 * S_HOST + 37, "mixB")["seg"][0]
    assert int(short[-1]) < 4 * (3 * S_HOST + 37)
    assert adamw_case(257 if 257 in ADAMW_N4 else 65, "mixA")["seg"][0].numel() == 1


@pytest.mark.parametrize("kind,mutant", [("adamw", m) for m in R.ADAMW_MUTANTS] + [("sgd", m) for m in R.SGD_MUTANTS])
def test_every_mutant_breaks_a_bound_or_an_exact_check(kind, mutant):
    caught = []
    for k, what, case in all_cases():
        if k != kind:
            continue
        worst, broken = _verdict(kind, case, mutant)
        if broken or any(v > 1.0 for v in worst.values()):
            caught.append(what)
    print("MUTANT %s %s caught on %d cases, first: %s" % (kind, mutant, len(caught), caught[:1]))
    assert caught, (kind, mutant)


def test_clip_coef_float32_evaluation_inside_bounds_and_nan():
    top = {}
    for n4 in CLIP_N4:
        g = R.clip_case(torch.Generator().manual_seed(3000 + n4), n4)
        for gs in CLIP_SCALES:
            ref, bnd = R.clip_coef_ref64(g, gs, 1.5, CLIP_BLOCKS_HOST)
            got = R.clip_coef_f32(g, gs, 1.5, CLIP_BLOCKS_HOST)
            for k in ("coef", "norm"):
                r = R.worst_ratio(got[k], ref[k], bnd[k])
                assert r <= 1.0, (n4, gs, k, r, float(got[k]), float(ref[k]))
                top[k] = max(top.get(k, 0.0), r)
        bad = g.clone()
        bad[bad.numel() // 2] = float("nan")
        ref, bnd = R.clip_coef_ref64(bad, 1.0, 1.5, CLIP_BLOCKS_HOST)
        assert bool(torch.isnan(ref["coef"])) and bool(torch.isnan(ref["norm"]))
        assert R.worst_ratio(R.clip_coef_f32(bad, 1.0, 1.5, CLIP_BLOCKS_HOST)["coef"], ref["coef"], bnd["coef"]) == 0.0
        assert R.worst_ratio(R.clip_coef_f32(bad, 1.0, 1.5, CLIP_BLOCKS_HOST, mutant="nan_to_one")["coef"], ref["coef"], bnd["coef"]) > 1.0
    print("RATIO host-f32 clip coef=%.3f norm=%.3f" % (top["coef"], top["norm"]))
    assert R.clip_trips(2 * CLIP_BLOCKS_HOST * 256 + 37, CLIP_BLOCKS_HOST) == (CLIP_BLOCKS_HOST, 3)
    assert R.clip_trips(R.CLIP_BLOCKS * 256 - 1) == (R.CLIP_BLOCKS, 1) and R.clip_trips(2 * R.CLIP_BLOCKS * 256 + 37) == (R.CLIP_BLOCKS, 3)


# ------------------------------------------------------------------ segment lookup
def test_quad_wise_lookup_equals_the_per_element_one_on_every_case():
    seen = 0
    for kind, what, case in all_cases():
        if case["seg"] is None:
            continue
        seg_end, _ = case["seg"]
        n4 = case["n4"]
        per_el = R.segment_of(torch.arange(4 * n4), seg_end)
        per_quad = R.quad_segment(torch.arange(n4), seg_end).repeat_interleave(4)
        assert torch.equal(per_el, per_quad), (kind, what)
        ends = seg_end.tolist()
        probe = sorted({e for b in ends for e in (b - 4, b - 1, b, b + 3) if 0 <= e < 4 * n4} | {0, 4 * n4 - 1})
        assert [R.segment_of_scalar(e, ends) for e in probe] == per_el[probe].tolist(), (kind, what)      # the kernel's loop, literally
        seen += 1
    assert seen > 20
    # ends that are NOT 4-aligned: the two disagree -- which is why the optimizers refuse such an arena when the multipliers differ
    odd = torch.tensor([6, 16], dtype=I64)
    assert not torch.equal(R.segment_of(torch.arange(16), odd), R.quad_segment(torch.arange(4), odd).repeat_interleave(4))


# ------------------------------------------------------------------ the arena keeps what the lookup relies on
def _quads_share_a_multiplier(opt):
    ar = opt.arena
    if opt.lr_scale is None:
        return True
    mult = torch.full((ar.numel,), float("nan"))
    for o, z, s in zip(ar.offsets, ar.sizes, opt.lr_scale.tolist()):
        mult[o:o + z] = s
    assert not bool(torch.isnan(mult).any())
    q = mult.view(-1, 4)
    return bool((q == q[:, :1]).all())


class _Pair(torch.nn.Module):
    """a grouped 1-row and 4-row pair, as the CenterNet predictors are laid out (weights of 6 and 24 elements, biases of 1 and 4)"""

    def __init__(self):
        super().__init__()
        from divergen_amd.layers.linear_ops import group_parameters
        self.backbone = torch.nn.Linear(10, 7)
        self.agn_hm, self.bbox_pred = torch.nn.Linear(6, 1), torch.nn.Linear(6, 4)
        group_parameters(self.agn_hm.weight, self.bbox_pred.weight)
        group_parameters(self.agn_hm.bias, self.bbox_pred.bias)


class _Plain(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = torch.nn.Linear(4, 4)
        self.head = torch.nn.Sequential(torch.nn.Linear(10, 7), torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))


@pytest.mark.parametrize("optimizer", ["ADAMW", "SGD"])
def test_all_elements_of_a_quad_share_one_multiplier_or_the_config_is_refused(optimizer):
    from divergen_amd.config import get_cfg
    from divergen_amd.solver import build_optimizer
    cfg = get_cfg()
    cfg.SOLVER.USE_CUSTOM_SOLVER, cfg.SOLVER.OPTIMIZER = True, optimizer
    cfg.SOLVER.BACKBONE_MULTIPLIER, cfg.SOLVER.CUSTOM_MULTIPLIER = 0.1, 0.5
    for names in ([], ["head.1"], ["head.0.bias", "head.2.weight"]):
        cfg.SOLVER.CUSTOM_MULTIPLIER_NAME = names
        opt = build_optimizer(cfg, _Plain())
        assert opt.lr_scale is not None and _quads_share_a_multiplier(opt)
    for names in ([], ["agn_hm", "bbox_pred"]):
        cfg.SOLVER.CUSTOM_MULTIPLIER_NAME = names
        opt = build_optimizer(cfg, _Pair())
        assert _quads_share_a_multiplier(opt)
        offs = dict(zip(opt.arena.names, opt.arena.offsets))
        assert offs["bbox_pred.bias"] == offs["agn_hm.bias"] + 1 and offs["bbox_pred.weight"] == offs["agn_hm.weight"] + 6
    # a name that matches ONE member of the pair: up to 3 elements of its neighbour would be stepped with the wrong learning rate
    cfg.SOLVER.CUSTOM_MULTIPLIER_NAME = ["agn_hm"]
    with pytest.raises(ValueError) as ei:
        build_optimizer(cfg, _Pair())
    assert "agn_hm.weight" in str(ei.value) and "bbox_pred.weight" in str(ei.value)
    cfg.SOLVER.CUSTOM_MULTIPLIER_NAME = ["bbox_pred.bias"]
    with pytest.raises(ValueError) as ei:
        build_optimizer(cfg, _Pair())
    assert "agn_hm.bias" in str(ei.value) and "bbox_pred.bias" in str(ei.value)
    # all multipliers 1: no lookup, nothing to refuse
    cfg.SOLVER.BACKBONE_MULTIPLIER, cfg.SOLVER.CUSTOM_MULTIPLIER = 1.0, 1.0
    assert build_optimizer(cfg, _Pair()).lr_scale is None
