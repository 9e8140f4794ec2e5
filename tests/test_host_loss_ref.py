"""tests/_loss_ref64.py (the float64 restatements of the fused loss kernels, their a-priori bounds and the shared inputs that
tests/test_gpu_loss_numerics.py holds csrc/detic_loss.hip, csrc/centernet_loss.hip and csrc/mask_loss.hip to) checked on the host:
the restatements against the reference's goldens and the project's composed torch paths in float64, an fp32 CPU evaluation of the
same formulas inside every bound on every case, and every listed mutant of the restatement outside a bound (or breaking an exact
comparison) on at least one case."""
import functools
import types

import numpy as np
import pytest
import torch

import _loss_ref64 as R

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = [F32, BF16]


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, rel=1e-5):
    """the project's bound for float goldens: 1e-5 relative (tensors: relative to the tensor's largest magnitude)"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= rel * float(b.abs().max())


@functools.lru_cache(maxsize=None)
def detic_case(name, dtype):
    c = R.detic_cast(R.DETIC_CASES[name](), dtype)
    return c, R.detic_ref64(*R.detic_args(c))


@functools.lru_cache(maxsize=None)
def centernet_case(name):
    c = R.CENTERNET_CASES[name]()
    return c, R.centernet_ref64(*R.centernet_args(c))


# ------------------------------------------------------------------ the bounds' storage term
def test_bf16_storage_bound_is_the_half_ulp():
    """Round-to-nearest-even to bf16 commits up to 2^-8 |x| just above a power of two: a flat 2^-9 |x| would fail a correct rounding.
    half_ulp_bf16 holds for every value, is attained, and is never wider than 2^-8 |x| nor tighter than 2^-9 |x|."""
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -8 - 2.0 ** -20], dtype=F64)
    err = (R.round_t(x, BF16) - x).abs()
    assert bool((err > 2.0 ** -9 * x.abs()).all()) and bool((err <= R.half_ulp_bf16(x)).all())
    g = torch.Generator().manual_seed(1)
    y = (torch.randn(200000, generator=g, dtype=F64) * torch.exp(torch.randn(200000, generator=g, dtype=F64) * 8)).float().double()
    e = (R.round_t(y, BF16) - y).abs()
    h = R.half_ulp_bf16(y)
    assert bool((e <= h).all()) and float((e / h).max()) > 0.99
    assert bool((h <= 2.0 ** -8 * y.abs()).all()) and bool((h > 2.0 ** -9 * y.abs() * (1 - 1e-12)).all())
    assert R.worst_ratio(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 1.0]), torch.tensor([1.0, 1.0])) == float("inf")
    assert R.worst_ratio(torch.tensor([0.0, 1.0]), torch.tensor([0.0, 1.0]), torch.tensor([0.0, 0.0])) == 0.0
    assert R.worst_ratio(torch.tensor([1e-30]), torch.tensor([0.0]), torch.tensor([0.0])) > 1.0


def test_torch_semantics_the_restatement_relies_on():
    a = torch.tensor([2.0, 1.0], dtype=F64, requires_grad=True)
    b = torch.tensor([2.0, 3.0], dtype=F64, requires_grad=True)
    (torch.minimum(a, b).sum() + 3 * torch.maximum(a, b).sum()).backward()
    assert a.grad.tolist() == [2.0, 1.0] and b.grad.tolist() == [2.0, 3.0]                 # ties split evenly
    x = torch.tensor([0.1, 0.5, 0.9, 0.05, 0.95], dtype=F64, requires_grad=True)
    torch.clamp(x, min=0.1, max=0.9).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]                                      # clamp passes on the closed interval
    assert float(np.float32(1.0) - np.float32(R.CLAMP_AT_IHF)) == float(np.float32(0.85))   # the clamp end that equals ignore_high_fp
    assert torch.equal(torch.sign(torch.tensor([0.0, -0.0])), torch.tensor([0.0, -0.0]))


# ------------------------------------------------------------------ the reference is right
def _golden_roi(golden):
    g = golden("roi_losses")
    C = 40
    w = torch.zeros(C + 1)
    w[T(g["appeared"]).long()] = 1
    return g, (T(g["logits"]), T(g["pred_deltas"]), T(g["gt_classes"]), w[:C], T(g["prop_boxes"]), T(g["gt_boxes"]), None,
               tuple(g["weights"].tolist()))


def test_detic_ref64_reproduces_the_roi_losses_golden(golden):
    g, args = _golden_roi(golden)
    r = R.detic_ref64(*args)
    assert close(r["out16"][8], T(g["loss_cls"])) and close(r["out16"][9], T(g["loss_box"]))
    assert close(r["dlogits"] * r["out16"][14], T(g["d_logits"]))
    assert close(r["dsign"] * r["out16"][10], T(g["d_pred_deltas"]))
    gtc = args[2]
    assert float(r["out16"][11]) == float(np.float32(int((args[0].argmax(1) == gtc).sum())) / np.float32(gtc.numel()))      # divided in fp32
    assert r["aux"]["sign_safe"]


CN_GOLDEN_CFG = {"not_norm_reg": 1, "beta": 4.0, "gamma": 2.0, "clamp": 1e-4, "ignore_high_fp": 0.85, "pos_mul": 0.25, "neg_mul": 0.75}


def test_centernet_ref64_reproduces_the_centernet_targets_golden(golden):
    """the golden's net: reg_weight 1, pos_weight = neg_weight 0.5, not_norm_reg, alpha 0.25, one rank"""
    g = golden("centernet_targets")
    r = R.centernet_ref64(T(g["reg_pred"]), T(g["reg2"]), T(g["hm2"]), T(g["agn_logit"]), T(g["pos2"]), None, CN_GOLDEN_CFG)
    o = r["out"]
    reg_norm, npos = max(float(o[0]), 1.0), max(float(o[4]), 1.0)
    assert int(o[4]) == T(g["pos2"]).numel()
    assert close(o[1] / reg_norm, T(g["loss_loc"])) and close(0.5 * o[3] / npos, T(g["loss_pos"])) and close(0.5 * o[2] / npos, T(g["loss_neg"]))
    assert close(r["g_reg"] / reg_norm, T(g["d_reg_pred"]))
    assert close(0.5 * (r["g_pos"] + r["g_neg"]) / npos, T(g["d_agn_logit"]))


@pytest.mark.parametrize("name", ["R64_W257", "R37_W1204", "R37_W41"])
def test_detic_ref64_equals_the_composed_torch_path_in_float64(name):
    """DeticFastRCNNOutputLayers.sigmoid_cross_entropy_loss / box_reg_loss on CPU in float64 (they know no ignore rows: gt < 0 -> C)"""
    import divergen_amd.modeling.roi_heads.detic_fast_rcnn as M
    from divergen_amd.modeling.box_regression import Box2BoxTransform
    c = dict(R.DETIC_CASES[name]())
    C = c["logits"].shape[1] - 1
    c["gt"] = torch.where(c["gt"] < 0, torch.full_like(c["gt"], C), c["gt"])
    fake = types.SimpleNamespace(use_fed_loss=False, freq_weight=None, fed_loss_num_cat=10, ignore_zero_cats=False, num_classes=C,
                                 smooth_l1_beta=0.0, box2box_transform=Box2BoxTransform(c["weights"]))
    x, d = c["logits"].double().requires_grad_(True), c["deltas"].double().requires_grad_(True)
    w = c["class_w"].double() if c["class_w"] is not None else "none"
    lc = M.DeticFastRCNNOutputLayers.sigmoid_cross_entropy_loss(fake, x, c["gt"], w)
    lb = M.DeticFastRCNNOutputLayers.box_reg_loss(fake, c["prop"].double(), c["gtb"].double(), d, c["gt"], c["src"])
    (lc + lb).backward()
    r = R.detic_ref64(*R.detic_args(c))
    assert close(r["out16"][8], lc.detach(), 1e-12) and close(r["out16"][9], lb.detach(), 1e-12)
    assert close(r["dlogits"] * r["out16"][14], x.grad, 1e-12) and close(r["dsign"] * r["out16"][10], d.grad, 1e-12)


@pytest.mark.parametrize("name", ["M5000_P37_C1_g2_b4_nnr0_ihf0.85_mixed", "M257_P300_C3_g2_b2_nnr1_ihf0.85_all", "M5000_P300_C3_g1.5_b4_nnr1_ihf0_mixed",
                                  "M5000_P300_C1_g3_b2_nnr0_ihf0.85_none"])
def test_centernet_ref64_equals_the_composed_path_in_float64(name):
    """CenterNet.losses on CPU tensors takes the composed (_FUSED_CN_LOSSES = False) path; float64"""
    import divergen_amd.modeling.dense_heads.centernet as CM
    from divergen_amd.utils.events import EventStorage
    c, r = centernet_case(name)
    cfg = c["cfg"]
    net = CM.CenterNet(in_channels=16, num_classes=7, with_agn_hm=True, only_proposal=True, reg_weight=2.0, not_norm_reg=bool(cfg["not_norm_reg"]),
                       pos_weight=0.5, neg_weight=0.75, ignore_high_fp=cfg["ignore_high_fp"], hm_focal_alpha=0.25, hm_focal_beta=cfg["beta"],
                       loss_gamma=cfg["gamma"], sigmoid_clamp=cfg["clamp"], centernet_head=torch.nn.Identity()).train()
    rp, al = c["reg_pred"].double().requires_grad_(True), c["logit"].double().requires_grad_(True)
    pos = c["pos_idx"] if c["cared"] is None else (c["pos_idx"], c["cared"])
    with EventStorage(0):
        L = net.losses(pos, c["reg_tgt"].double(), c["hms"].double(), rp, al)
    (L["loss_centernet_loc"] * 1.3 + L["loss_centernet_agn_pos"] * 0.7 + L["loss_centernet_agn_neg"] * 1.9).backward()
    o = r["out"]
    reg_norm, npos = max(float(o[0]), 1.0), max(float(o[4]), 1.0)
    # (the composed path clamps at 1 - c in float64, the kernel at the fp32 value of 1.0f - c: 1e-6 covers the clamped elements)
    assert close(2.0 * o[1] / reg_norm, L["loss_centernet_loc"].detach(), 1e-6)
    assert close(0.5 * o[3] / npos, L["loss_centernet_agn_pos"].detach(), 1e-6)
    assert close(0.75 * o[2] / npos, L["loss_centernet_agn_neg"].detach(), 1e-6)
    assert close(1.3 * 2.0 * r["g_reg"] / reg_norm, rp.grad, 1e-6)
    # ... but not the few placed logits whose sigmoid lies between the two upper clamp ends: there the two pass / block differently
    sg = torch.sigmoid(c["logit"].double())
    between = (sg - (1.0 - cfg["clamp"])).abs() < 1e-7
    assert int(between.sum()) <= 3
    assert close(((0.7 * 0.5 * r["g_pos"] + 1.9 * 0.75 * r["g_neg"]) / npos)[~between], al.grad[~between], 1e-6)


def test_mask_ref64_equals_torch_bce():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(9, 50, generator=g, dtype=F64) * 5).requires_grad_(True)
    gt = torch.rand(9, 50, generator=g) > 0.5
    ref = torch.nn.functional.binary_cross_entropy_with_logits(x, gt.double(), reduction="mean")
    ref.backward()
    r = R.mask_bce_ref64(x.detach(), gt)
    assert close(r["out"][0], ref.detach(), 1e-12) and close(r["grad"].reshape(9, 50), x.grad, 1e-12)
    wrong = (x.detach() > 0) != gt
    assert r["out"][1:].tolist() == [float(wrong.sum()), float((wrong & ~gt).sum()), float((wrong & gt).sum()), float(gt.sum())]


# ------------------------------------------------------------------ the reference alone stays inside its own bounds
def eval32_detic(c, dtype):
    """the same formulas in torch float32, the gradient rounded to the storage type"""
    e = R.detic_ref64(*R.detic_args(c), dt=F32)
    e["dlogits"] = e["dlogits"].to(dtype).double()
    return e


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(R.DETIC_CASES))
def test_detic_fp32_cpu_evaluation_is_inside_the_bounds(name, dtype):
    c, ref = detic_case(name, dtype)
    assert ref["aux"]["sign_safe"], "a delta sits within the evaluation error of its target: the sign is not decidable"
    e = eval32_detic(c, dtype)
    ratios = R.detic_check(e, ref, dtype)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    C = c["logits"].shape[1] - 1
    # joint layout and the in-place scale
    _, gcols = R.joint_ld(C, c["logits"].shape[1] in R.PRODUCT_WIDTHS)
    for g_cls, g_box in ((1.0, 1.0), (0.37, 2.5), (1.0, 0.0)):
        buf, bb, scaled, bs = R.detic_joint_ref64(ref, gcols, dtype, g_cls, g_box)
        stored = torch.zeros_like(buf)
        stored[:, :C + 1], stored[:, C + 1:C + 5] = e["dlogits"], e["dsign"]
        assert R.worst_ratio(stored, buf, bb) <= 1.0
        want = R.grad_scale_ref64(stored, stored.shape[0], C, e["out16"], g_cls, g_box)
        got = (stored.float() * torch.where(torch.arange(gcols) < C + 1, torch.tensor(float(np.float32(g_cls) * np.float32(float(e["out16"][14])))),
                                            torch.tensor(float(np.float32(g_box) * np.float32(float(e["out16"][10])))))).to(dtype).double()
        got[:, C + 5:] = stored[:, C + 5:]
        assert R.worst_ratio(got, want, R.grad_scale_bound(want, dtype)) <= 1.0
        # against the reference's own chain: two storage roundings, the fp32 scale and the bound of the unscaled gradient
        sc = torch.where(torch.arange(gcols) < C + 1, ref["out16"][14] * g_cls, ref["out16"][10] * g_box).abs()
        chain = buf * torch.where(torch.arange(gcols) < C + 1, ref["out16"][14] * g_cls, ref["out16"][10] * g_box)
        assert R.worst_ratio(got, chain, 2 * R.storage(chain, dtype) + bb * sc + 4 * R.U32 * chain.abs()) <= 1.0
    if name.startswith("all_ignore"):
        assert float(ref["out16"][8]) == 0.0 and float(ref["out16"][14]) == 1.0 and float(ref["dlogits"].abs().max()) == 0.0
    if name.startswith("all_background"):
        assert float(ref["out16"][9]) == 0.0 and float(ref["out16"][10]) == 1.0


@pytest.mark.parametrize("name", list(R.CENTERNET_CASES))
def test_centernet_fp32_cpu_evaluation_is_inside_the_bounds(name):
    c, ref = centernet_case(name)
    e = R.centernet_ref64(*R.centernet_args(c), dt=F32)
    ratios = R.centernet_check(e, ref)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert float(e["out"][4]) == float(ref["out"][4])
    b = R.centernet_bounds(ref)
    # the either-way elements are placed ones, not the bulk: everywhere else the gradient is held to better than 1 %
    # (next to the upper clamp end 1 - p itself carries 4 u / 1e-4 = 2.4e-3 of relative error in fp32)
    loose = (b["g_neg"] > 1e-2 * ref["g_neg"].abs()) & (ref["g_neg"] != 0)
    assert int(loose.sum()) <= len(c["placed"]), int(loose.sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_mask_fp32_cpu_evaluation_is_inside_the_bounds(dtype):
    c = R.mask_case()
    x = c["full"].to(dtype)[:, c["cls"]].reshape(c["full"].shape[0], -1)
    ref = R.mask_bce_ref64(x, c["gt"])
    e = R.mask_bce_ref64(x, c["gt"], dt=F32)
    b = R.mask_bounds(ref, dtype)
    assert R.worst_ratio(e["out"], ref["out"], b["out"]) <= 1.0
    assert R.worst_ratio(e["grad"].to(dtype), ref["grad"], b["grad"]) <= 1.0
    assert x.numel() > 1024 * 1024 and float(b["out"][0]) < 1e-3 * float(ref["out"][0])


# ------------------------------------------------------------------ the bounds and inputs have teeth
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("mutant", R.DETIC_MUTANTS)
def test_detic_mutant_is_caught(mutant, dtype):
    caught = []
    for name in R.DETIC_CASES:
        c, ref = detic_case(name, dtype)
        m = R.detic_ref64(*R.detic_args(c), mutant=mutant)
        if max(R.detic_check(m, ref, dtype).values()) > 1.0:
            caught.append(name)
    assert caught, mutant


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("mutant", R.JOINT_MUTANTS)
def test_detic_joint_mutant_is_caught(mutant, dtype):
    caught = []
    for name in R.DETIC_CASES:
        c, ref = detic_case(name, dtype)
        C = c["logits"].shape[1] - 1
        _, gcols = R.joint_ld(C, c["logits"].shape[1] in R.PRODUCT_WIDTHS)
        for g_cls, g_box in ((1.0, 1.0), (0.37, 2.5), (1.0, 0.0)):
            buf, bb, scaled, bs = R.detic_joint_ref64(ref, gcols, dtype, g_cls, g_box)
            mbuf, _, mscaled, _ = R.detic_joint_ref64(ref, gcols, dtype, g_cls, g_box, mutant=mutant)
            if R.worst_ratio(mbuf, buf, bb) > 1.0 or R.worst_ratio(R.round_t(mscaled, dtype), scaled, bs) > 1.0:
                caught.append((name, g_cls, g_box))
    assert caught, mutant


@pytest.mark.parametrize("mutant", R.CENTERNET_MUTANTS)
def test_centernet_mutant_is_caught(mutant):
    caught = []
    for name in R.CENTERNET_CASES:
        c, ref = centernet_case(name)
        m = R.centernet_ref64(*R.centernet_args(c), mutant=mutant)
        if max(R.centernet_check(m, ref).values()) > 1.0:
            caught.append(name)
    assert caught, mutant
