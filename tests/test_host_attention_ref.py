"""tests/_attn_ref64.py (the float64 reference, the emulation of the kernel's rounding contract and the per-element bounds that
tests/test_gpu_attention_numerics.py holds the window-attention kernels to) checked on the host: the analytic backward against
autograd of the existing fp32 restatement test_gpu_kernels._attn_ref run in float64, the emulation inside its own bounds, and the
bounds far from "anything passes"."""
import pytest
import torch

import _attn_ref64 as R
from test_gpu_kernels import _attn_ref

SCALE = 32 ** -0.5


@pytest.mark.parametrize("ws,B_,nW,nH", [(7, 6, 3, 2), (12, 4, 2, 2)])
def test_attn_ref64_equals_autograd_of_the_existing_reference(ws, B_, nW, nH):
    qkv, table, region, dout = R.ordinary_inputs(ws, B_, nW, nH)
    r = R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout)
    q64 = qkv.double().requires_grad_(True)
    t64 = table.double().requires_grad_(True)
    out = _attn_ref(q64, t64, region, nH, ws, SCALE, dtype=torch.float64)
    assert out.dtype == torch.float64
    out.backward(dout.double())
    for name, a, b in (("out", r["out"], out.detach()), ("dqkv", r["dqkv"], q64.grad), ("dtable", r["dtable"], t64.grad)):
        assert float((a - b).abs().max()) <= 1e-11 * float(b.abs().max()), name
    # lse: the logsumexp of the logits that reproduce `out`
    s = R.logits64(qkv, table, region, nW, nH, ws, SCALE)
    assert torch.allclose(r["lse"], torch.logsumexp(s, -1), rtol=0, atol=1e-12)
    # the abs_* products bound their signed twins
    assert bool((r["abs_out"] >= r["out"].abs() - 1e-12).all()) and bool((r["abs_dqkv"] >= r["dqkv"].abs() - 1e-12).all())
    assert bool((r["abs_dtable"] >= r["dtable"].abs() - 1e-12).all())
    # handed the float64 out itself, the backward is the same function
    r2 = R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout, out=r["out"])
    assert float((r2["dqkv"] - r["dqkv"]).abs().max()) <= 1e-11 * float(r["dqkv"].abs().max())


def _emu_and_ref(qkv, table, region, nW, nH, ws, dout):
    e = R.attn_emu(qkv, table, region, nW, nH, ws, SCALE, dout)
    return e, R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout, out=e["out"].to(torch.bfloat16))


@pytest.mark.parametrize("ws,B_,nW,nH", R.PARITY_SHAPES)
def test_emulation_stays_inside_its_bounds_and_the_bounds_are_tight(ws, B_, nW, nH):
    qkv, table, region, dout = R.ordinary_inputs(ws, B_, nW, nH)
    e, r = _emu_and_ref(qkv, table, region, nW, nH, ws, dout)
    b = R.bounds(r)
    for k in ("out", "lse", "dqkv", "dtable"):
        assert R.worst_ratio(e[k], r[k], b[k]) <= 1.0, k
        frac = float((b[k] < 0.25 * r[k].abs().max()).double().mean())
        assert frac >= 0.99, (k, frac)
    # m was set from these ratios (module docstring): twice the measured one, rounded up, never below 1
    for k, v in R.emu_ratios(qkv, table, region, nW, nH, ws, SCALE, dout).items():
        assert 2 * v <= R.M[k], (k, v)
    # every table corner of every head is held to its own one-term scale: losing the entry altogether is outside the bound
    corners, _ = R.edge_entries(ws)
    assert bool((b["dtable"][corners] < r["dtable"][corners].abs()).all()), (b["dtable"][corners] / r["dtable"][corners].abs())


@pytest.mark.parametrize("level", [40, 300])
def test_peaked_rows_take_delta_from_the_out_the_backward_is_given(level):
    """Near one-hot rows: dS = P (dP - delta) cancels to the 2^-8 rounding of the out inside delta.  With the reference's delta formed
    from the same bf16 out the emulation is inside the bounds; against the plain float64 gradient (delta from the float64 out) the
    same results are far outside them -- that reference answers another question."""
    ws, B_, nW, nH = 7, 3, 1, 1
    qkv, table, region, dout = R.ordinary_inputs(ws, B_, nW, nH, seed=5)
    x = qkv.float()
    s = R.logits64(qkv, table * 0, None, 1, nH, ws, SCALE)
    x[..., :2 * nH * 32] *= (level / float(s.max(-1).values.mean())) ** 0.5
    qkv = x.to(torch.bfloat16)
    e, r = _emu_and_ref(qkv, table, region, nW, nH, ws, dout)
    b = R.bounds(r)
    for k in ("out", "lse", "dqkv", "dtable"):
        assert R.worst_ratio(e[k], r[k], b[k]) <= 1.0, k
    r0 = R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout)
    b0 = R.bounds(r0)
    assert R.worst_ratio(e["dqkv"], r0["dqkv"], b0["dqkv"]) > 50.0 and R.worst_ratio(e["dtable"], r0["dtable"], b0["dtable"]) > 50.0


def test_exclusion_mask_is_invisible_in_out_and_gradients_at_ordinary_logits():
    """Why the mask-semantics test needs constructed inputs: at logits of a few units an excluded key and a key at -100 give the same
    out to float64 rounding; only inputs whose own region scores ~100 lower tell them apart."""
    ws, B_, nW, nH = 7, 3, 3, 1
    qkv, table, region, dout = R.ordinary_inputs(ws, B_, nW, nH)
    r = R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout)
    x = R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout, mask_value=float("-inf"))
    assert float((r["out"] - x["out"]).abs().max()) < 1e-14 and float((r["dqkv"] - x["dqkv"]).abs().max()) < 1e-14
