"""float64 reference of the window-attention core (forward and backward), a CPU emulation of the kernel's rounding contract, and the
per-element a-priori error bounds the GPU tests hold csrc/window_attention.hip to.  Host only, plain torch; the math restates
test_gpu_kernels._attn_ref (pinned on it by test_host_attention_ref.py) with oracle.swin.relative_position_index for the bias.

Layouts: qkv (B_, N, 3 * nH * 32) bf16, window b uses mask row b % nW; table ((2 ws - 1)^2, nH); region (nW, N) integer ids or None;
dout (B_, N, nH * 32).  Per-head tensors below are (B_, nH, N, ...).

The kernel's contract (csrc/window_attention.hip): bf16 inputs and outputs; logits, softmax statistics and every accumulation in
fp32; the probabilities P (forward: the un-normalised exp(s - max), normalised after the MFMA; backward: exp(s - lse)) and dS are
rounded to bf16 where they feed an MFMA; one final bf16 rounding of out / dq / dk / dv; lse and the table gradient stay fp32 (the
table gradient sums the UNROUNDED dS).  The backward entry point takes the forward's bf16 `out` as an INPUT and forms
delta = rowsum(dO * out) from it, as every flash-style backward does.  The reference follows that interface: `attn_ref64(..., out=)`
is given the very tensor handed to the backward kernel and forms its delta from it in float64 (at a peaked softmax row dS, hence
dq and dk, is nothing but P times the 2^-8 rounding of out inside delta: a reference built on the float64 out would compare the
kernel with a function of inputs it never saw).  With out=None it is the plain float64 gradient, which
test_host_attention_ref.py pins on autograd.

Bound per element (`bounds`), the shape of test_gpu_gemm.close_bf16:

    |got - ref| <= 2^-9 |ref|                      final bf16 rounding (not for the fp32 outputs lse, dtable)
                 + m 2^-9 abs_X                    bf16 rounding of the operands P / dS (abs_X = the same product with absolute values)
                 + 1e-5 max|ref| + 1e-6            fp32 summation order (dq, dk, dv: each part's own max|ref|)

(bf16 keeps 8 significant bits: its unit roundoff is 2^-8.  The formula's factor is 2^-9; m, measured below, carries the other
factor of two -- abs_X >= |ref| everywhere.)

m per output.  `attn_emu` is the contract in float64 with `.to(torch.bfloat16)` at P, dS and the results; the reference's backward
gets the emulation's out.  Largest ratio (|emu - ref| - 2^-9 |ref| - (1e-5 max|ref| + 1e-6)) / (2^-9 abs_X) over PARITY_SHAPES
with `ordinary_inputs` (randn * 1.5, table randn); m = ceil(2 * ratio), at least 1:

    shape (ws, B_, nW, nH)   out     dq      dk      dv      dtable
    (7, 3, 3, 1)             1.15    1.78    1.64    2.06    <= 0
    (7, 8, 4, 3)             1.69    2.05    1.82    2.17    <= 0
    (12, 6, 3, 2)            1.35    2.08    2.38    1.86    <= 0
    (12, 19, 1, 6)           1.56    1.95    1.98    1.72    <= 0
    (7, 75, 25, 4)           2.01    2.41    2.28    2.21    <= 0
    (12, 27, 9, 10)          1.78    2.32    2.20    2.14    <= 0
    worst                    2.01    2.41    2.38    2.21    <= 0
    m                        5       5       5       5       1

(`python tests/_attn_ref64.py` prints the table; test_host_attention_ref.py asserts 2 * ratio <= m at all six.  dtable: the
emulation sums the same unrounded float64 dS as the reference; on the GPU its P and dS are fp32.)  lse has no rounded operand:
its bound is 1e-5 max|ref| + 1e-6.
"""
import torch

from oracle import swin as OSW

U = 2.0 ** -9          # the factor of the bound's formula (half the bf16 unit roundoff)
M = {"out": 5, "dq": 5, "dk": 5, "dv": 5, "dtable": 1}
MASK = -100.0
PARITY_SHAPES = [(7, 3, 3, 1), (7, 8, 4, 3), (12, 6, 3, 2), (12, 19, 1, 6), (7, 75, 25, 4), (12, 27, 9, 10)]     # (ws, B_, nW, nH)


def _bf(x):
    return x.to(torch.bfloat16).double()


def _heads(x, nH, parts):
    B_, N, _ = x.shape
    return x.double().reshape(B_, N, parts, nH, 32).permute(2, 0, 3, 1, 4)


def _unheads(x):            # (B_, nH, N, 32) -> (B_, N, nH * 32)
    B_, nH, N, _ = x.shape
    return x.transpose(1, 2).reshape(B_, N, nH * 32)


def logits64(qkv, table, region, nW, nH, ws, scale, mask_value=MASK):
    """float64 logits (B_, nH, N, N): q k^T * scale + bias (+ mask_value where the region ids differ; -inf = exclusion)."""
    q, k, _ = _heads(qkv, nH, 3)
    B_, N = q.shape[0], q.shape[2]
    idx = OSW.relative_position_index(ws).reshape(-1)
    s = (q * float(scale)) @ k.transpose(-2, -1) + table.double()[idx].reshape(N, N, nH).permute(2, 0, 1)[None]
    if region is not None:
        assert region.shape[0] == nW and B_ % nW == 0
        r = region.long()
        diff = (r[:, None, :] != r[:, :, None])                     # (nW, query, key), symmetric
        m = torch.zeros(nW, N, N, dtype=torch.float64).masked_fill(diff, mask_value)
        s = (s.reshape(B_ // nW, nW, nH, N, N) + m[None, :, None]).reshape(B_, nH, N, N)
    return s


def _index_add_table(x, ws):
    """(B_, nH, N, N) -> ((2 ws - 1)^2, nH): the sum over windows, added into the table by the relative-position index."""
    B_, nH, N, _ = x.shape
    idx = OSW.relative_position_index(ws).reshape(-1)
    return torch.zeros((2 * ws - 1) ** 2, nH, dtype=torch.float64).index_add_(0, idx, x.sum(0).reshape(nH, N * N).t().contiguous())


def _backward(P, dS, q, k, dO, scale, ws, Pv=None, dSm=None):
    """dq, dk, dv, dtable from P / dS; Pv, dSm = the (rounded) operands of the products, dS itself goes to the table."""
    Pv = P if Pv is None else Pv
    dSm = dS if dSm is None else dSm
    return scale * dSm @ k, scale * dSm.transpose(-2, -1) @ q, Pv.transpose(-2, -1) @ dO, _index_add_table(dS, ws)


def attn_ref64(qkv, table, region, nW, nH, ws, scale, dout, out=None, mask_value=MASK):
    """float64 forward and backward of the bf16-rounded inputs.  Returns a dict: out (B_, N, C), lse (B_, nH, N; natural log),
    dqkv (B_, N, 3 C), dtable (T, nH); abs_out, abs_dq / abs_dk / abs_dv (packed as abs_dqkv too), abs_dtable.
    out: the bf16 (B_, N, C) tensor handed to the backward entry point (the forward's result): delta = rowsum(dO * out) is then
    formed from it, as the kernel's interface has it; None: from the float64 out (plain autograd of the forward)."""
    scale = float(scale)
    q, k, v = _heads(qkv, nH, 3)
    dO = _heads(dout, nH, 1)[0]
    s = logits64(qkv, table, region, nW, nH, ws, scale, mask_value)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o64 = P @ v
    dP = dO @ v.transpose(-2, -1)
    delta = ((dO * o64) if out is None else (dO * _heads(out, nH, 1)[0])).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dq, dk, dv, dtable = _backward(P, dS, q, k, dO, scale, ws)
    aS = dS.abs()
    r = {"out": _unheads(o64), "lse": lse, "dqkv": torch.cat([_unheads(dq), _unheads(dk), _unheads(dv)], -1), "dtable": dtable,
         "abs_out": _unheads(P @ v.abs()), "abs_dv": _unheads(P.transpose(-2, -1) @ dO.abs()),
         "abs_dq": _unheads(scale * aS @ k.abs()), "abs_dk": _unheads(scale * aS.transpose(-2, -1) @ q.abs()),
         "abs_dtable": _index_add_table(aS, ws)}
    r["abs_dqkv"] = torch.cat([r["abs_dq"], r["abs_dk"], r["abs_dv"]], -1)
    return r


def attn_emu(qkv, table, region, nW, nH, ws, scale, dout):
    """The kernel's contract in float64 with the bf16 roundings at the places the module docstring names.  Same keys as attn_ref64
    (out, lse, dqkv, dtable)."""
    scale = float(scale)
    q, k, v = _heads(qkv, nH, 3)
    dO = _heads(dout, nH, 1)[0]
    s = logits64(qkv, table, region, nW, nH, ws, scale)
    mx = s.max(-1, keepdim=True).values
    e = torch.exp(s - mx)
    lse = mx[..., 0] + torch.log(e.sum(-1))
    out = _bf((_bf(e) @ v) / e.sum(-1, keepdim=True))                       # P rounded un-normalised, one final rounding
    P = torch.exp(s - lse[..., None])                                       # the backward recomputes P from lse
    dP = dO @ v.transpose(-2, -1)
    delta = (dO * out).sum(-1, keepdim=True)                                # ... and delta from the bf16 out
    dS = P * (dP - delta)
    dq, dk, dv, dtable = _backward(P, dS, q, k, dO, scale, ws, Pv=_bf(P), dSm=_bf(dS))
    return {"out": _unheads(out), "lse": lse, "dqkv": _bf(torch.cat([_unheads(dq), _unheads(dk), _unheads(dv)], -1)), "dtable": dtable}


def _floor(ref):
    return 1e-5 * float(ref.abs().max()) + 1e-6


def bounds(r):
    """Per-element bound of every compared tensor of an attn_ref64 result: dict out, lse, dqkv, dtable (the module docstring).
    The fp32-order floor of dq, dk and dv is taken from each part's own max|ref|."""
    C = r["out"].shape[-1]
    m = torch.cat([torch.full((C,), float(M[n])) for n in ("dq", "dk", "dv")]).double()
    fl = torch.cat([torch.full((C,), _floor(r["dqkv"][..., i * C:(i + 1) * C])) for i in range(3)]).double()
    return {"out": U * r["out"].abs() + M["out"] * U * r["abs_out"] + _floor(r["out"]),
            "lse": torch.full_like(r["lse"], _floor(r["lse"])),
            "dqkv": U * r["dqkv"].abs() + m * U * r["abs_dqkv"] + fl,
            "dtable": M["dtable"] * U * r["abs_dtable"] + _floor(r["dtable"])}


def worst_ratio(got, ref, bnd):
    """max over elements of |got - ref| / bound (inf for a non-finite result): <= 1 passes."""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bnd).max())


def edge_entries(ws):
    """indices into the (2 ws - 1)^2 table: the four corners and the 4 (2 ws - 3) other edge entries."""
    n = 2 * ws - 1
    corners = [0, n - 1, n * (n - 1), n * n - 1]
    edges = [y * n + x for y in range(n) for x in range(n) if (y in (0, n - 1) or x in (0, n - 1)) and y * n + x not in corners]
    assert len(edges) == 4 * (2 * ws - 3)
    return corners, edges


def ordinary_inputs(ws, B_, nW, nH, seed=None):
    """randn * 1.5 qkv, randn table, randn dO, random region ids (row 0 unmasked) when nW > 1: the inputs of the parity shapes.
    (The default seeds are drawn so that at every PARITY_SHAPE no table corner of any head has a gradient near zero -- a corner is one
    (query, key) pair per window, masked in some: the corner checks need a value that a lost entry would miss by more than the bound.)"""
    g = torch.Generator().manual_seed(500000 + ws * 1000 + B_ * 10 + nH if seed is None else seed)
    N = ws * ws
    qkv = (torch.randn(B_, N, 3 * nH * 32, generator=g) * 1.5).to(torch.bfloat16)
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g)
    region = None
    if nW > 1:
        region = torch.randint(0, 3, (nW, N), generator=g, dtype=torch.int8)
        region[0] = 0
    dout = torch.randn(B_, N, nH * 32, generator=g).to(torch.bfloat16)
    return qkv, table, region, dout


def emu_ratios(qkv, table, region, nW, nH, ws, scale, dout):
    """(|emu - ref| - 2^-9 |ref| - floor) / (2^-9 abs_X), the largest per output: what M is set from.  The reference's backward is
    given the emulation's bf16 out, as the GPU tests give it the kernel's."""
    e = attn_emu(qkv, table, region, nW, nH, ws, scale, dout)
    r = attn_ref64(qkv, table, region, nW, nH, ws, scale, dout, out=e["out"].to(torch.bfloat16))
    C = r["out"].shape[-1]

    def ratio(got, ref, absx, rounded):
        num = (got - ref).abs() - (U * ref.abs() if rounded else 0.0) - _floor(ref)
        return float((num / (U * absx).clamp_min(1e-300)).max())
    res = {"out": ratio(e["out"], r["out"], r["abs_out"], True)}
    for i, n in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        res[n] = ratio(e["dqkv"][..., sl], r["dqkv"][..., sl], r["abs_dqkv"][..., sl], True)
    res["dtable"] = ratio(e["dtable"], r["dtable"], r["abs_dtable"], False)
    return res


if __name__ == "__main__":
    worst = {}
    for ws, B_, nW, nH in PARITY_SHAPES:
        qkv, table, region, dout = ordinary_inputs(ws, B_, nW, nH)
        rr = emu_ratios(qkv, table, region, nW, nH, ws, 32 ** -0.5, dout)
        print((ws, B_, nW, nH), {k: round(v, 2) for k, v in rr.items()})
        for k, v in rr.items():
            worst[k] = max(worst.get(k, -1e9), v)
    print("worst", {k: round(v, 2) for k, v in worst.items()})
