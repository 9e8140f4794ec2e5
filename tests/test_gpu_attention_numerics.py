"""Window attention (csrc/window_attention.hip) through the C ABI against the float64 reference of tests/_attn_ref64.py:
per-element a-priori bounds instead of a fraction of the tensor's maximum, bit-exact routing with one-hot softmax rows, logits up to
several hundred, and the additive (-100, not exclusion) semantics of the shift mask -- forward, lse and backward, padded and compact
entry points.  Every test prints its worst error / bound ratio per output before it asserts (pytest -s shows them)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _attn_ref64 as R  # noqa: E402
import test_gpu_kernels as TK  # noqa: E402  (its _classic_rows and the compact == padded comparison are reused, not copied)
from divergen_amd.layers import shift_regions  # noqa: E402

DEV = "cuda"
SCALE = 32 ** -0.5
PARITY_SHAPES = R.PARITY_SHAPES          # (ws, B_, nW, nH)


# ------------------------------------------------------------------ drivers: CPU tensors in, CPU tensors out, padded layout
def run_padded(qkv, table, region, nW, nH, ws, dout, backward=True):
    from divergen_amd import _lib as L
    lib, st = L.lib(), L.stream()
    B_, N, C = qkv.shape[0], ws * ws, nH * 32
    qd, dd = qkv.to(DEV).contiguous(), dout.to(DEV).contiguous()
    td = table.float().t().contiguous().to(DEV)                       # (nH, T): stride_head T, stride_index 1
    rd = region.to(torch.int8).to(DEV) if region is not None else None
    out = torch.full((B_, N, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B_, nH, N), float("nan"), dtype=torch.float32, device=DEV)
    L.check(lib.dgx_window_attention_fwd(L.ptr(qd), L.ptr(td), td.shape[1], 1, L.ptr(rd), L.ptr(out), L.ptr(lse), B_, nW, nH, ws, SCALE, st), "fwd")
    res = {"out": out, "lse": lse}
    if backward:
        dq, dt = torch.full_like(qd, float("nan")), torch.zeros_like(td)
        L.check(lib.dgx_window_attention_bwd(L.ptr(qd), L.ptr(td), L.ptr(rd), L.ptr(out), L.ptr(lse), L.ptr(dd), L.ptr(dq), L.ptr(dt),
                                             td.shape[1], 1, B_, nW, nH, ws, SCALE, st), "bwd")
        res.update(dqkv=dq, dtable=dt.t())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def run_compact(qkv_p, bias, table, B, H, W, nH, ws, shift, dout_p, backward=True):
    """qkv_p / dout_p: the padded (classic) layout (B * nW, N, .), padding rows = bias / 0.  Runs the compact entry points on the rows of
    the real tokens and returns the results in the padded layout again, + `real` (B * nW, N): out is defined for real tokens only."""
    from divergen_amd import _lib as L
    lib, st = L.lib(), L.stream()
    N, C = ws * ws, nH * 32
    real = (TK._classic_rows(B, H, W, ws, shift) >= 0)
    T, Tw = int(real.sum()), real.numel()
    assert T == B * H * W and Tw == qkv_p.shape[0] * N
    assert torch.equal(qkv_p.reshape(Tw, 3 * C)[~real], bias[None].expand(Tw - T, 3 * C)) and not bool(dout_p.reshape(Tw, C)[~real].any())
    qc, dc = qkv_p.reshape(Tw, 3 * C)[real].contiguous().to(DEV), dout_p.reshape(Tw, C)[real].contiguous().to(DEV)
    bd = bias.to(DEV)
    td = table.float().t().contiguous().to(DEV)
    rd = shift_regions(H, W, ws).to(DEV) if shift else None
    B_ = Tw // N
    out_c = torch.full((T, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B_, nH, N), float("nan"), dtype=torch.float32, device=DEV)
    L.check(lib.dgx_window_attention_fwd_compact(L.ptr(qc), L.ptr(bd), L.ptr(td), td.shape[1], 1, L.ptr(rd), L.ptr(out_c), L.ptr(lse),
                                                 B, H, W, nH, ws, shift, SCALE, st), "fwd_compact")
    out = torch.zeros(Tw, C, dtype=torch.bfloat16)
    res = {"lse": lse}
    if backward:
        dq_c, dt = torch.full((Tw, 3 * C), float("nan"), dtype=torch.bfloat16, device=DEV), torch.zeros_like(td)
        L.check(lib.dgx_window_attention_bwd_compact(L.ptr(qc), L.ptr(bd), L.ptr(td), L.ptr(rd), L.ptr(out_c), L.ptr(lse), L.ptr(dc), L.ptr(dq_c),
                                                     L.ptr(dt), td.shape[1], 1, B, H, W, nH, ws, shift, SCALE, st), "bwd_compact")
        torch.cuda.synchronize()
        dq = torch.empty(Tw, 3 * C, dtype=torch.bfloat16)
        dq[real], dq[~real] = dq_c[:T].cpu(), dq_c[T:].cpu()          # the padding tokens' rows follow the real ones, in classic order
        res.update(dqkv=dq.reshape(B_, N, 3 * C), dtable=dt.t())
    torch.cuda.synchronize()
    out[real] = out_c.cpu()
    res["out"] = out.reshape(B_, N, C)
    return {k: v.cpu() for k, v in res.items()}, real.reshape(B_, N)


def check(group, what, got, r, keys=("out", "lse", "dqkv", "dtable"), real=None, lse_bound=None):
    """every element inside its bound (tests/_attn_ref64.py), every result finite; prints the worst error / bound per output first."""
    b = R.bounds(r)
    if lse_bound is not None:
        b["lse"] = lse_bound
    ratios = {}
    for k in keys:
        g, ref, bnd = got[k].double(), r[k], b[k]
        if k == "out" and real is not None:
            g, ref, bnd = g[real], ref[real], bnd[real]
        assert bool(torch.isfinite(g).all()), (what, k, "not finite")
        ratios[k] = R.worst_ratio(g, ref, bnd)
    print("RATIO %s %s %s" % (group, what, " ".join("%s=%.3f" % kv for kv in ratios.items())))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)
    return ratios


# ------------------------------------------------------------------ 5. per-element parity at ordinary inputs, table edges by name
def ref_for(got, qkv, table, region, nW, nH, ws, dout):
    """the float64 reference whose backward is handed what the backward kernel was handed: the forward kernel's bf16 out."""
    return R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout, out=got["out"])


def _check_table_edges(what, ws, got, r):
    bnd = R.bounds(r)["dtable"]
    n = 2 * ws - 1
    corners, edges = R.edge_entries(ws)
    for kind, ids in (("corner", corners), ("edge", edges)):
        for i in ids:
            err = (got["dtable"][i].double() - r["dtable"][i]).abs()
            assert bool((err <= bnd[i]).all()), "%s: table gradient, %s entry (dy, dx) = (%d, %d): got %s, expected %s, bound %s" % (
                what, kind, i // n - (ws - 1), i % n - (ws - 1), got["dtable"][i].tolist(), r["dtable"][i].tolist(), bnd[i].tolist())
    # a corner's bound is its own one-term scale, not the centre's: an entry that is missing altogether is outside it, in every head
    assert bool((bnd[corners] < r["dtable"][corners].abs()).all()), (what, "corner bounds degenerate", (bnd[corners] / r["dtable"][corners].abs()).tolist())


@pytest.mark.parametrize("ws,B_,nW,nH,reserved", [s + (0,) for s in PARITY_SHAPES] + [s + (16,) for s in PARITY_SHAPES[-2:]])
def test_parity_per_element_and_table_edges(ws, B_, nW, nH, reserved):
    """randn * 1.5 inputs: out, lse, dqkv and dtable inside the per-element bounds, the table's 4 corners and 4 (2 ws - 3) edge
    entries named one by one.  The last two shapes run `upw = 2` units per workgroup with one window left over per head (300 and 270
    units on 256 CUs), again on the 240 CUs the data-parallel reducer leaves."""
    from divergen_amd import _lib as L
    qkv, table, region, dout = R.ordinary_inputs(ws, B_, nW, nH)
    L.set_reserved_cus(reserved)
    try:
        got = run_padded(qkv, table, region, nW, nH, ws, dout)
    finally:
        L.set_reserved_cus(0)
    r = ref_for(got, qkv, table, region, nW, nH, ws, dout)
    what = "parity ws=%d B_=%d nW=%d nH=%d reserved=%d" % (ws, B_, nW, nH, reserved)
    check("parity", what, got, r)
    _check_table_edges(what, ws, got, r)


@pytest.mark.parametrize("B,H,W,ws,nH,shift", [(3, 33, 30, 7, 4, 3), (3, 30, 26, 12, 10, 6)])
def test_compact_equals_padded_multi_unit_runs(B, H, W, ws, nH, shift):
    """The comparison of test_window_attention_compact_equals_padded (same tensors, bit for bit) where B_ * nH > 256 and
    B_ % upw != 0: several units per workgroup, the register prefetch of the next window, multi-unit table-gradient sums."""
    TK.test_window_attention_compact_equals_padded(B, H, W, ws, nH, shift)


def _padded_layout_case(B, H, W, ws, nH, shift, seed):
    """randn * 1.5 tokens laid out in the classic padded order, padding rows = the qkv bias, their dO = 0."""
    g = torch.Generator().manual_seed(seed)
    N, C = ws * ws, nH * 32
    real = TK._classic_rows(B, H, W, ws, shift) >= 0
    Tw = real.numel()
    bias = (torch.randn(3 * C, generator=g)).to(torch.bfloat16)
    qkv = (torch.randn(Tw, 3 * C, generator=g) * 1.5).to(torch.bfloat16)
    qkv[~real] = bias
    dout = torch.randn(Tw, C, generator=g).to(torch.bfloat16)
    dout[~real] = 0
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g)
    return qkv.reshape(-1, N, 3 * C), bias, table, dout.reshape(-1, N, C)


def test_compact_against_float64_on_the_padded_layout():
    B, H, W, ws, nH, shift = 3, 33, 30, 7, 4, 3
    qkv, bias, table, dout = _padded_layout_case(B, H, W, ws, nH, shift, 11)
    region = shift_regions(H, W, ws)
    nW = region.shape[0]
    got, real = run_compact(qkv, bias, table, B, H, W, nH, ws, shift, dout)
    r = ref_for(got, qkv, table, region, nW, nH, ws, dout)
    check("parity", "compact 3x33x30 ws=7", got, r, real=real)
    _check_table_edges("compact 3x33x30 ws=7", ws, got, r)


# ------------------------------------------------------------------ 2. exact routing: one-hot softmax rows
def _codes(ids):
    """±1 codes over 32 dims: the 8-bit binary expansion of the id, written four times (distinct ids: dot <= 24)."""
    bits = ((ids[..., None] >> torch.arange(8)) & 1) * 2 - 1
    return torch.cat([bits] * 4, -1).float()


def _sparse_dout(shape_bhn, g):
    """one random bf16 entry per (row, head): dP and delta are then single exact products and cancel exactly at the winning key
    (with a dense dO the two fp32 sums differ in their last bit and dS = 0 holds to 1e-6 |dO| only, times |q| = 32 in dk).  The dv
    check of these cases therefore sees one head-dim column per row; test_routing_dv_with_dense_dout sees all 32."""
    B_, nH, N = shape_bhn
    d = torch.zeros(B_, nH, N, 32)
    d.scatter_(-1, torch.randint(0, 32, (B_, nH, N, 1), generator=g), torch.randn(B_, nH, N, 1, generator=g))
    return R._unheads(d.double()).to(torch.bfloat16)


def _routing_inputs(ws, B_, nH, pi, g, dup=None, below_zero=False):
    """k = a distinct code per key (another assignment per window and head), q_i = 32 k_pi(i), random bf16 v.  pi: (B_, nH, N) long.
    dup = (ja, jb) long (B_, nH): key jb gets key ja's code.  below_zero: the code written three times, the last 8 dims 1 in every
    key and -128 in every query: every logit 181 lower -- the winner at -45, the others 34 or more behind it."""
    N = ws * ws
    ids = torch.stack([torch.stack([torch.randperm(256, generator=g)[:N] for _ in range(nH)]) for _ in range(B_)])     # (B_, nH, N)
    if dup is not None:
        ids.scatter_(-1, dup[1][..., None], ids.gather(-1, dup[0][..., None]))
    k = _codes(ids)                                                   # (B_, nH, N, 32)
    if below_zero:
        k[..., 24:] = 1.0
    q = 32.0 * k.gather(2, pi[..., None].expand(-1, -1, -1, 32))
    if below_zero:
        q[..., 24:] = -128.0
    v = torch.randn(B_, nH, N, 32, generator=g) * 1.5
    qkv = torch.cat([R._unheads(q.double()), R._unheads(k.double()), R._unheads(v.double())], -1).to(torch.bfloat16)
    return qkv, _sparse_dout((B_, nH, N), g)


def _check_routing(what, got, qkv, table, region, nW, nH, ws, dout, pi, real=None, backward=True):
    B_, N, C = qkv.shape[0], ws * ws, nH * 32
    v = R._heads(qkv, nH, 3)[2].to(torch.bfloat16)                    # (B_, nH, N, 32)
    expect = R._unheads(v.gather(2, pi[..., None].expand(-1, -1, -1, 32)))
    o = got["out"]
    qmask = torch.ones(B_, N, dtype=torch.bool) if real is None else real
    assert torch.equal(o[qmask], expect[qmask]), (what, "out != v[pi]", int((o[qmask] != expect[qmask]).any(-1).sum()), "rows differ")
    win = R.logits64(qkv, table, region, nW, nH, ws, SCALE).gather(-1, pi[..., None])[..., 0]          # (B_, nH, N)
    lerr = ((got["lse"].double() - win).abs() / win.abs())[qmask[:, None, :].expand(-1, nH, -1)]
    print("RATIO routing %s lse_rel=%.2e" % (what, float(lerr.max())))
    assert float(lerr.max()) <= 1e-4, (what, "lse != winning logit", float(lerr.max()))
    if not backward:
        return
    dmax = float(dout.float().abs().max())
    dqkv, dt = got["dqkv"].double(), got["dtable"].double()
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(dt).all()), what
    zero = max(float(dqkv[..., :2 * C].abs().max()), float(dt.abs().max()))
    r = R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout)
    dv_ref = r["dqkv"][..., 2 * C:]
    dv_ratio = float(((dqkv[..., 2 * C:] - dv_ref).abs() / (2.0 ** -8 * dv_ref.abs() + 1e-6)).max())
    print("RATIO routing %s dq_dk_dtable_max/(1e-6 max|dO|)=%.3f dv=%.3f" % (what, zero / (1e-6 * dmax), dv_ratio))
    assert zero <= 1e-6 * dmax, (what, "dS must vanish", zero, dmax)
    assert dv_ratio <= 1.0, (what, "dv != sum of dO over pi(i) = j", dv_ratio)


def _pi(kind, B_, nH, N, g, region=None, nW=1, keep=None):
    """query -> key maps, another one per window and head.  region: pi stays inside the query's region.  keep (B_, N) bool: keys allowed."""
    if kind == "last":
        return torch.full((B_, nH, N), N - 1, dtype=torch.long)
    if kind == "first":
        return torch.zeros(B_, nH, N, dtype=torch.long)
    if kind == "reverse":
        return (N - 1 - torch.arange(N)).expand(B_, nH, N).contiguous()
    pi = torch.arange(N).repeat(B_, nH, 1)
    for b in range(B_):
        reg = region[b % nW].long() if region is not None else torch.zeros(N, dtype=torch.long)
        ok = keep[b] if keep is not None else torch.ones(N, dtype=torch.bool)
        for h in range(nH):
            for rid in reg.unique():
                idx = torch.nonzero((reg == rid) & ok)[:, 0]
                pi[b, h, idx] = idx[torch.randperm(idx.numel(), generator=g)]       # a permutation of the group onto itself
    return pi


@pytest.mark.parametrize("table_kind", ["zero", "ints"])
@pytest.mark.parametrize("kind", ["perm", "last", "first", "reverse", "masked"])
@pytest.mark.parametrize("ws", [7, 12])
def test_routing_one_hot_rows_are_bit_exact(ws, kind, table_kind):
    """out[i] == v[pi(i)] bit for bit, lse == the winning logit, dq = dk = dtable = 0, dv[j] = sum of dO[i] over pi(i) = j."""
    g = torch.Generator().manual_seed(ws * 10 + len(kind) + len(table_kind))
    N, nH, nW = ws * ws, 3, 4
    B_ = 8
    region = shift_regions(2 * ws, 2 * ws, ws) if kind == "masked" else None
    pi = _pi(kind, B_, nH, N, g, region, nW)
    table = torch.zeros((2 * ws - 1) ** 2, nH) if table_kind == "zero" else torch.randint(-8, 9, ((2 * ws - 1) ** 2, nH), generator=g).float()
    qkv, dout = _routing_inputs(ws, B_, nH, pi, g)
    got = run_padded(qkv, table, region, nW if region is not None else 1, nH, ws, dout)
    _check_routing("ws=%d %s table=%s" % (ws, kind, table_kind), got, qkv, table, region, nW, nH, ws, dout, pi)


@pytest.mark.parametrize("kind", ["perm", "last"])
@pytest.mark.parametrize("ws", [7, 12])
def test_routing_dv_with_dense_dout(ws, kind):
    """dv[j] = the fp32 sum of dO[i] over pi(i) = j, rounded once, with a dense random dO: all 32 head dims of every row (dq, dk and
    dtable are left to the sparse-dO cases, where they vanish exactly)."""
    g = torch.Generator().manual_seed(90 + ws + len(kind))
    N, nH, B_ = ws * ws, 3, 8
    C = nH * 32
    pi = _pi(kind, B_, nH, N, g)
    table = torch.zeros((2 * ws - 1) ** 2, nH)
    qkv, _ = _routing_inputs(ws, B_, nH, pi, g)
    dout = torch.randn(B_, N, C, generator=g).to(torch.bfloat16)
    got = run_padded(qkv, table, None, 1, nH, ws, dout)
    dv_ref = torch.zeros(B_, nH, N, 32, dtype=torch.float64).scatter_add_(2, pi[..., None].expand(-1, -1, -1, 32), R._heads(dout, nH, 1)[0])
    dv_ref = R._unheads(dv_ref)
    ratio = float(((got["dqkv"][..., 2 * C:].double() - dv_ref).abs() / (2.0 ** -8 * dv_ref.abs() + 1e-6)).max())
    print("RATIO routing ws=%d %s dense dO dv=%.3f" % (ws, kind, ratio))
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("ws", [7, 12])
def test_routing_winner_below_zero_keeps_padded_key_columns_out(ws):
    """Every real logit far below zero (winner -45): a key column of the MFMA padding (49 -> 64, 144 -> 160 keys; its k is zero, its
    logit the bare bias) would win the row if it were let in."""
    g = torch.Generator().manual_seed(70 + ws)
    N, nH, B_ = ws * ws, 3, 8
    pi = _pi("perm", B_, nH, N, g)
    table = torch.zeros((2 * ws - 1) ** 2, nH)
    qkv, dout = _routing_inputs(ws, B_, nH, pi, g, below_zero=True)
    win = R.logits64(qkv, table, None, 1, nH, ws, SCALE)
    top2 = win.topk(2, -1).values
    assert float(top2[..., 0].max()) < -40.0 and float((top2[..., 0] - top2[..., 1]).min()) > 30.0
    got = run_padded(qkv, table, None, 1, nH, ws, dout)
    _check_routing("ws=%d winner below zero" % ws, got, qkv, table, None, 1, nH, ws, dout, pi)


@pytest.mark.parametrize("ws", [7, 12])
def test_routing_bias_entry_decides_between_twin_keys(ws):
    """Two keys with the SAME code: only a table entry (a corner of the table: one (query, key) pair reads it) separates them, +20
    picks the far key, -20 its twin."""
    g = torch.Generator().manual_seed(ws)
    N, nH, B_ = ws * ws, 3, 8
    n = 2 * ws - 1
    pairs = [(0, N - 1, 0), (N - 1, 0, n * n - 1), (ws - 1, N - ws, n - 1), (N - ws, ws - 1, n * (n - 1))]       # (query, far key, table entry)
    idx = R.OSW.relative_position_index(ws)
    for i0, ja, e in pairs:
        assert int(idx[i0, ja]) == e and int((idx == e).sum()) == 1
    jb = N // 2
    sign = torch.randint(0, 2, (4, nH), generator=g) * 2 - 1
    sign[:, 0] = torch.tensor([1, -1, 1, -1])                          # both signs occur whatever the draw
    table = torch.zeros(n * n, nH)
    for c, (_, _, e) in enumerate(pairs):
        table[e] = 20.0 * sign[c]
    corner_keys = torch.tensor([p[1] for p in pairs] + [jb])
    keep = torch.ones(B_, N, dtype=torch.bool)
    keep[:, corner_keys] = False                                       # nobody else looks at the corner keys or the twin
    pi = _pi("perm", B_, nH, N, g, keep=keep)
    ja_t, jb_t = torch.zeros(B_, nH, dtype=torch.long), torch.full((B_, nH), jb, dtype=torch.long)
    for b in range(B_):
        for h in range(nH):
            c = (b + h) % 4
            i0, ja, _ = pairs[c]
            ja_t[b, h] = ja
            pi[b, h, i0] = ja
            for j in corner_keys.tolist():                             # the queries at the other excluded positions: an allowed key
                if j != i0:
                    pi[b, h, j] = 1
    qkv, dout = _routing_inputs(ws, B_, nH, pi, g, dup=(ja_t, jb_t))
    expect_pi = pi.clone()
    for b in range(B_):
        for h in range(nH):
            c = (b + h) % 4
            if sign[c, h] < 0:
                expect_pi[b, h, pairs[c][0]] = jb
    got = run_padded(qkv, table, None, 1, nH, ws, dout)
    _check_routing("ws=%d twin keys" % ws, got, qkv, table, None, 1, nH, ws, dout, expect_pi)


def _compact_routing_case(B, H, W, ws, nH, shift, g, pad_wins=False):
    N, C = ws * ws, nH * 32
    real = (TK._classic_rows(B, H, W, ws, shift) >= 0).reshape(-1, N)
    B_ = real.shape[0]
    region = shift_regions(H, W, ws) if shift else None
    nW = B_ // B
    pi = _pi("perm", B_, nH, N, g, region, nW, keep=real)              # real queries -> real keys of their region; padding: itself
    qkv, dout = _routing_inputs(ws, B_, nH, pi, g)
    # the qkv bias: its key code [c, c, -c, -c] is orthogonal to every code written four times, so a padding key scores 0
    c8 = (torch.randint(0, 2, (nH, 8), generator=g) * 2 - 1).float()
    kb = torch.cat([c8, c8, -c8, -c8], -1)
    bias = torch.cat([(32 * kb).reshape(-1), kb.reshape(-1), (torch.randn(C, generator=g) * 1.5)]).to(torch.bfloat16)
    chosen = torch.zeros(B_, N, dtype=torch.bool)
    if pad_wins:                                                       # every third real query of a window with padding asks for the bias key
        haspad = ~real.all(-1)
        chosen = real & haspad[:, None] & (torch.arange(N) % 3 == 0)[None]
        qkv[..., :C] = torch.where(chosen[..., None], bias[:C][None, None], qkv[..., :C])
    qkv[~real] = bias
    dout[~real] = 0
    return qkv, bias, dout, region, nW, pi, real, chosen


@pytest.mark.parametrize("B,H,W,ws,nH", [(2, 10, 13, 7, 2), (2, 13, 30, 12, 2)])
def test_routing_compact_padding_never_wins(B, H, W, ws, nH):
    """Compact entry points on a grid with padding, shift on: padding keys (k = the qkv bias) are orthogonal to every real key's code."""
    g = torch.Generator().manual_seed(H * W)
    shift = ws // 2
    qkv, bias, dout, region, nW, pi, real, _ = _compact_routing_case(B, H, W, ws, nH, shift, g)
    table = torch.randint(-8, 9, ((2 * ws - 1) ** 2, nH), generator=g).float()
    got, real2 = run_compact(qkv, bias, table, B, H, W, nH, ws, shift, dout)
    assert torch.equal(real, real2)
    _check_routing("compact %dx%d ws=%d" % (H, W, ws), got, qkv, table, region, nW, nH, ws, dout, pi, real=real)


@pytest.mark.parametrize("B,H,W,ws,nH", [(2, 10, 13, 7, 2), (2, 13, 30, 12, 2)])
def test_routing_compact_padding_wins_where_asked(B, H, W, ws, nH):
    """Unmasked windows (no shift): queries that ask for the bias key get the bias v (all padding keys of the window tie), lse = the
    winning logit + log(padding keys in the window); the other queries their own key."""
    g = torch.Generator().manual_seed(H * W + 1)
    N, C = ws * ws, nH * 32
    qkv, bias, dout, region, nW, pi, real, chosen = _compact_routing_case(B, H, W, ws, nH, 0, g, pad_wins=True)
    assert int(chosen.sum()) > 0
    table = torch.zeros((2 * ws - 1) ** 2, nH)
    got, _ = run_compact(qkv, bias, table, B, H, W, nH, ws, 0, dout, backward=False)
    v = qkv[..., 2 * C:]
    normal = real & ~chosen
    expect = R._unheads(R._heads(v, nH, 1)[0].gather(2, pi[..., None].expand(-1, -1, -1, 32))).to(torch.bfloat16)
    assert torch.equal(got["out"][normal], expect[normal])
    assert torch.equal(got["out"][chosen], bias[2 * C:][None].expand(int(chosen.sum()), C))
    npad = (~real).sum(-1).double()
    want = 32.0 * 32.0 * SCALE + torch.log(npad)[:, None].expand(-1, N)[chosen]
    for h in range(nH):
        rel = ((got["lse"][:, h][chosen].double() - want).abs() / want).max()
        assert float(rel) <= 1e-4, (h, float(rel))


# ------------------------------------------------------------------ 3. hard logits
def _hard_inputs(ws, B_, nW, nH, kind, g):
    N, C = ws * ws, nH * 32
    qkv = torch.randn(B_, N, 3 * C, generator=g) * 1.5
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g)
    region = None
    if nW > 1:
        region = torch.randint(0, 3, (nW, N), generator=g, dtype=torch.int8)
        region[0] = 0
    if isinstance(kind, int):                                          # q and k scaled so that the row maxima reach about `kind`
        s = R.logits64(qkv.to(torch.bfloat16), table * 0, None, 1, nH, ws, SCALE)
        qkv[..., :2 * C] *= (kind / float(s.max(-1).values.mean())) ** 0.5
    elif kind == "table30":                                            # large logits through the fp32 bias path
        table = (torch.rand((2 * ws - 1) ** 2, nH, generator=g) * 2 - 1) * 30
    elif kind == "offsets":                                            # row i of every head: + c_i, |c_i| in 50 .. 200, either sign
        c = (50 + 150 * torch.rand(B_, N, nH, generator=g)) * (torch.randint(0, 2, (B_, N, nH), generator=g) * 2 - 1)
        x = qkv.view(B_, N, 3, nH, 32)
        x[:, :, 0, :, 31] = c / SCALE
        x[:, :, 1, :, 31] = 1.0
    dout = torch.randn(B_, N, C, generator=g).to(torch.bfloat16)
    return qkv.to(torch.bfloat16), table, region, dout


@pytest.mark.parametrize("kind", [40, 90, 300, "table30", "offsets"])
@pytest.mark.parametrize("ws,B_,nW,nH", [(7, 6, 3, 2), (12, 3, 1, 2)])
def test_hard_logits_against_float64(ws, B_, nW, nH, kind):
    """Row maxima of 40 / 90 / 300 (exp overflows fp32 at 89 without the max subtraction), a table at +-30, a different offset of up to
    +-200 per row: everything finite and inside the per-element bounds, lse against the float64 logsumexp."""
    g = torch.Generator().manual_seed(ws + 7 * len(str(kind)) + (kind if isinstance(kind, int) else 0))
    qkv, table, region, dout = _hard_inputs(ws, B_, nW, nH, kind, g)
    top = float(R.logits64(qkv, table, region, nW, nH, ws, SCALE).max(-1).values.abs().mean())
    if isinstance(kind, int):
        assert 0.5 * kind <= top <= 1.5 * kind, (kind, top)
    got = run_padded(qkv, table, region, nW, nH, ws, dout)
    r = ref_for(got, qkv, table, region, nW, nH, ws, dout)
    check("hard", "ws=%d %s (mean |row max| %.0f)" % (ws, kind, top), got, r, lse_bound=1e-5 * r["lse"].abs() + 1e-4)


# ------------------------------------------------------------------ 4. the mask is an additive -100, not an exclusion
def _mask_inputs(ws, B_, nH, region, g):
    """A query's same-region keys score about -60 (dims 8..16, one per region id: -a in q, +a in k), the first two keys of every
    region score about +60 for the queries of the OTHER regions (dims 17..25: the key marks its region, the query every region but
    its own); after the -100 those still lead the query's own region by e^20.  Dims 0..7 carry a small random part."""
    nW, N = region.shape
    C = nH * 32
    a = 18.5                                                           # 18.5^2 * 32^-0.5 = 60.5
    assert int(region.max()) <= 8
    x = torch.zeros(B_, N, 3, nH, 32)
    x[..., :8] = torch.randn(B_, N, 3, nH, 8, generator=g) * 0.5
    x[:, :, 2] = torch.randn(B_, N, nH, 32, generator=g) * 1.5
    for b in range(B_):
        reg = region[b % nW].long()
        own = torch.nn.functional.one_hot(reg, 9).float()             # (N, 9)
        x[b, :, 0, :, 8:17] = (-a * own)[:, None]
        x[b, :, 1, :, 8:17] = (a * own)[:, None]
        x[b, :, 0, :, 17:26] = (a * (1 - own))[:, None]
        for rid in reg.unique():
            first = torch.nonzero(reg == rid)[:2, 0]
            x[b, first, 1, :, 17 + int(rid)] = a
    dout = torch.randn(B_, N, C, generator=g).to(torch.bfloat16)
    return x.reshape(B_, N, 3 * C).to(torch.bfloat16), dout


def _assert_exclusion_would_fail(what, r, r_inf, real=None):
    b = R.bounds(r)
    for k in ("out", "lse", "dqkv"):
        a, ref, bnd = r_inf[k], r[k], b[k]
        if k == "out" and real is not None:
            a, ref, bnd = a[real], ref[real], bnd[real]
        ratio = R.worst_ratio(a, ref, bnd)
        assert ratio > 100.0, (what, k, "an exclusion-style mask would pass", ratio)


@pytest.mark.parametrize("ws,nH", [(7, 2), (12, 2)])
def test_mask_is_additive_minus_100_padded(ws, nH):
    g = torch.Generator().manual_seed(40 + ws)
    region = shift_regions(2 * ws, 2 * ws, ws)
    nW, B_ = region.shape[0], 2 * region.shape[0]
    assert int(region[0].max()) == 0 and all(len(region[w].unique()) >= 2 for w in range(1, nW))
    qkv, dout = _mask_inputs(ws, B_, nH, region, g)
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g)
    r = R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout)
    _assert_exclusion_would_fail("ws=%d" % ws, r, R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout, mask_value=float("-inf")))
    got = run_padded(qkv, table, region, nW, nH, ws, dout)
    check("mask", "padded ws=%d" % ws, got, ref_for(got, qkv, table, region, nW, nH, ws, dout))


def test_mask_is_additive_minus_100_compact():
    B, H, W, ws, nH, shift = 2, 10, 13, 7, 2, 3
    g = torch.Generator().manual_seed(47)
    N, C = ws * ws, nH * 32
    region = shift_regions(H, W, ws)
    nW = region.shape[0]
    real = (TK._classic_rows(B, H, W, ws, shift) >= 0).reshape(-1, N)
    qkv, dout = _mask_inputs(ws, B * nW, nH, region, g)
    bias = (torch.randn(3 * C, generator=g) * 0.5).to(torch.bfloat16)
    qkv[~real] = bias
    dout[~real] = 0
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g)
    r = R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout)
    _assert_exclusion_would_fail("compact", r, R.attn_ref64(qkv, table, region, nW, nH, ws, SCALE, dout, mask_value=float("-inf")), real=real)
    got, _ = run_compact(qkv, bias, table, B, H, W, nH, ws, shift, dout)
    check("mask", "compact 10x13 ws=7", got, ref_for(got, qkv, table, region, nW, nH, ws, dout), real=real)
