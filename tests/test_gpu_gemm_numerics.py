"""dgx_gemm_bf16_nt through the C ABI against the float64 restatements of tests/_gemm_ref64.py: every element of every output of every
table row inside its a-priori bound -- all four kernel forms, all seven tiles, all six tails, the split-K fold with each tail, the
persistent loop of gemm_lw past a workgroup's first item, ragged M / N / K next to stride gaps -- or bit-exact where the contract is
exact (one-hot rows, masked positions, stride gaps, sentinels).  The test owns every buffer: output-only ones are pre-filled with NaN,
64 sentinels stand behind every output and behind a private NaN-filled split-K workspace, the stride gaps of C / C2 hold sentinels that
must survive, the gaps of A / B / aux hold NaN, and after every launch dgx_gemm_last_form must report the plan of the row.  Each test
prints `RATIO gemm <form> <case> <output>=<worst |err| / bound> ...` before it asserts (pytest -s shows them)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import _gemm_ref64 as R  # noqa: E402

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SENT, PAD, NAN = R.SENT, 64, float("nan")


@pytest.fixture
def reserved():
    """dgx_set_reserved_cus for one test; the whole chip again afterwards"""
    from divergen_amd import _lib as L
    yield L.lib().dgx_set_reserved_cus
    L.lib().dgx_set_reserved_cus(0)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def operand(t, ld):
    """a (rows, cols) operand at leading dimension ld on the device, NaN in the stride gaps"""
    rows, cols = t.shape
    buf = torch.full((rows * ld,), NAN, dtype=t.dtype, device=DEV)
    buf.view(rows, ld)[:, :cols] = t.to(DEV)
    return buf


class Output:
    """an output-only (rows, cols) tensor at leading dimension ld: NaN where the kernel must write, sentinels in the stride gaps and PAD
    of them behind the last row"""

    def __init__(self, rows, cols, ld, dtype):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.buf = torch.full((rows * ld + PAD,), SENT, dtype=dtype, device=DEV)
        self.buf[:rows * ld].view(rows, ld)[:, :cols] = NAN

    def untouched(self):
        body = self.buf[:self.rows * self.ld].view(self.rows, self.ld)
        return bool((body[:, self.cols:].float() == SENT).all()) and bool((self.buf[self.rows * self.ld:].float() == SENT).all())

    def value(self):
        return self.buf[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols].cpu()


_WS = []


def workspace():
    """the private split-K workspace: NaN, PAD sentinels behind it"""
    if not _WS:
        _WS.append(torch.empty(R.WS_BYTES // 4 + PAD, dtype=F32, device=DEV))
    _WS[0][:R.WS_BYTES // 4] = NAN
    _WS[0][R.WS_BYTES // 4:] = SENT
    return _WS[0]


def last_form():
    from divergen_amd import _lib as L
    bm, bn, sp = L.c_i(), L.c_i(), L.c_i()
    form = L.lib().dgx_gemm_last_form(bm, bn, sp)
    return form, bm.value, bn.value, sp.value


def launch(case, inp, strided, dgx_dev, reserved, plan=None):
    """one dgx_gemm_bf16_nt launch of a table row under its knobs -> {"C" | "C2" | "out": tensor on the CPU}; asserts the return code, the
    reported plan, every sentinel and every stride gap"""
    from divergen_amd import _lib as L
    M, N, K = case.M, case.N, case.K
    st = R.strides(case, strided)
    a, b = operand(inp["a"], st["lda"]), operand(inp["b"], st["ldb"])
    ep = L.GemmEpilogue()
    ep.mode, ep.relu = case.mode, int(case.relu)
    keep, outs = [], {}
    if case.mode in (1, 2, 3):
        keep.append(inp["bias"].to(DEV))
        ep.bias = L.ptr(keep[-1])
    if case.mode != 3:
        outs["C"] = Output(M, N, st["ldc"], BF16)
        ep.c, ep.ldc = L.ptr(outs["C"].buf), st["ldc"]
    if case.mode == 2:
        outs["C2"] = Output(M, N, st["ldc"], BF16)
        ep.c2 = L.ptr(outs["C2"].buf)
    if case.mode in (4, 5):
        keep.append(operand(inp["aux"], st["ldaux"]))
        ep.aux, ep.ldaux = L.ptr(keep[-1]), st["ldaux"]
    if case.mode == 3:
        B, H, W, ws, shift = case.win
        res = inp["res"].to(DEV)
        outs["out"] = Output(B * H * W, N, N, res.dtype)
        keep += [res, None if inp["scale"] is None else inp["scale"].to(DEV)]
        ep.residual, ep.out, ep.scale, ep.residual_dtype = L.ptr(res), L.ptr(outs["out"].buf), L.ptr(keep[-1]), L.dtype_code(res)
        ep.B, ep.H, ep.W, ep.ws, ep.shift = B, H, W, ws, shift
    wsb = workspace()
    ep.workspace, ep.workspace_bytes = L.ptr(wsb), R.WS_BYTES
    dgx_dev("reset", 0)
    for key, value in case.knobs:
        dgx_dev(key, value)
    reserved(case.reserved)
    rc = L.lib().dgx_gemm_bf16_nt(L.ptr(a), L.ptr(b), M, N, K, st["lda"], st["ldb"], ctypes.byref(ep), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, (R.case_id(case), rc)
    want = case.plan if plan is None else plan
    got = last_form()
    assert got[:len(want)] == tuple(want), (R.case_id(case), got, want)
    assert bool((wsb[R.WS_BYTES // 4:] == SENT).all()), "wrote behind the workspace"
    for name, o in outs.items():
        assert o.untouched(), (R.case_id(case), name, "a stride gap or the sentinels behind the output were written")
    return {name: o.value() for name, o in outs.items()}


def form_name(case):
    return R.FORM_NAMES[case.plan[0]]


# ------------------------------------------------------------------ every element of every row
def _parity_params():
    shape_first, numeric_first = {}, {}
    for i, c in enumerate(R.CASES):
        shape_first.setdefault((c.M, c.N, c.K), i)
        numeric_first.setdefault(numeric_key(c), i)
    params = [(c, kind) for c in R.CASES for kind in R.kinds_of(c)]
    # cases that share operands, then references, run next to each other (the caches below hold one or two entries)
    params.sort(key=lambda p: (shape_first[(p[0].M, p[0].N, p[0].K)], R.INPUT_KINDS.index(p[1]), numeric_first[numeric_key(p[0])]))
    return params


def numeric_key(c):
    return (c.M, c.N, c.K, c.mode, c.relu, c.res_bf16, c.win)


_REF = {}


def reference(case, kind):
    """evaluate64 of (case, kind), kept for the next case with the same arithmetic (another form, tile, split or reserved count)"""
    key = (numeric_key(case), kind)
    if key not in _REF:
        _REF.clear()
        _REF[key] = R.evaluate64(case, R.inputs(case, kind), pre=R.contraction(case, kind))
    return _REF[key]


@pytest.mark.parametrize("case,kind", _parity_params(), ids=lambda v: v if isinstance(v, str) else R.case_id(v))
def test_every_element_inside_its_bound(case, kind, dgx_dev, reserved):
    inp, r = R.inputs(case, kind), reference(case, kind)
    for strided in (False, True):
        outs = launch(case, inp, strided, dgx_dev, reserved)
        R.report(form_name(case), "%s %s %s" % (R.case_id(case), kind, "strided" if strided else "contiguous"), R.check(case, r, outs))


# ------------------------------------------------------------------ exact: one-hot rows
@pytest.mark.parametrize("case", [c for c in R.CASES if c.row in ("T", "S", "I", "P") and c.mode in (0, 1, 5)], ids=R.case_id)
def test_one_hot_rows_give_the_weights_bit_for_bit(case, dgx_dev, reserved):
    """a[m][(37 m + 11) % K] = 1: out[m][:] = b[:, k_m] (with a bias bf16(b + bias); ReLU, the ReLU' mask applied) -- a K chunk, split or
    walked item that is lost, doubled or read from another row moves a weight vector"""
    M, N, K = case.M, case.N, case.K
    inp = dict(R.inputs(case, "ordinary"))
    inp["a"] = R.one_hot_a(M, K)
    col = inp["b"].float().t()[(37 * torch.arange(M) + 11) % K]
    if case.mode == 1:
        col = col + inp["bias"].float()
    want = col.to(BF16)
    if case.relu:
        want = torch.where(want.float() > 0, want, torch.zeros_like(want))
    if case.mode == 5:
        want = torch.where(inp["aux"].float() > 0, want, torch.zeros_like(want))
    for strided in (False, True):
        got = launch(case, inp, strided, dgx_dev, reserved)["C"]
        assert torch.equal(bits(got), bits(want)), (R.case_id(case), strided, (got.float() != want.float()).nonzero()[:4])


# ------------------------------------------------------------------ non-finite operands stay where they belong
@pytest.mark.parametrize("case", [c for c in R.CASES if c.mode <= 1 and not c.relu and
                                  ((c.row == "T" and c.plan[1:3] == (128, 128)) or (c.row == "W") or (c.row == "S" and c.plan[3] == 18))], ids=R.case_id)
def test_one_nan_one_inf_poison_one_row_one_column(case, dgx_dev, reserved):
    M, N, K = case.M, case.N, case.K
    r = reference(case, "ordinary")
    inp = dict(R.inputs(case, "ordinary"))
    m0, n0 = M - 3, N - 5
    a, b = inp["a"].clone(), inp["b"].clone()
    a[m0, K - 1] = NAN
    b[n0, K // 2] = float("inf")
    inp["a"], inp["b"] = a, b
    for strided in (False, True):
        got = launch(case, inp, strided, dgx_dev, reserved)["C"].float()
        assert bool(torch.isnan(got[m0]).all()) and not bool(torch.isfinite(got[:, n0]).any())
        clean = torch.ones(M, N, dtype=torch.bool)
        clean[m0], clean[:, n0] = False, False
        assert bool(torch.isfinite(got[clean]).all())
        (ref, bnd), = R.references(case, r).values()
        worst = float(R.ratios(torch.where(clean, got.double(), ref), ref, bnd).max())
        R.report(form_name(case), "%s nonfinite %s" % (R.case_id(case), "strided" if strided else "contiguous"), {"C": worst})


# ------------------------------------------------------------------ GELU and GELU' at every finite bf16 input
SWEEP_FORMS = {0: (("gemm_lw", 0), ("gemm_2wg", 0)), 1: (("gemm_lw", 1),), 2: (("gemm_lw", 0), ("gemm_2wg", 2))}


@pytest.mark.parametrize("form", sorted(SWEEP_FORMS))
def test_gelu_tails_at_every_finite_bf16_input(form, dgx_dev, reserved):
    """all 65 280 finite bf16 bit patterns as a (340, 192) matrix: through mode 2 by an identity weight (C = x, C2 = GELU(C)), through mode
    4 as the saved pre-activation under y = 1"""
    x = R.all_finite_bf16().reshape(340, 192)
    eye = torch.eye(192).to(BF16)
    case = R.Case("G", 340, 192, 192, 2, False, 0, None, SWEEP_FORMS[form], 0, (form,))
    outs = launch(case, {"a": x, "b": eye, "bias": torch.zeros(192).to(BF16)}, True, dgx_dev, reserved)
    xd = x.double()
    res = {"C": R.worst_ratio(outs["C"], xd, R.flushable(xd, R.y_bound(xd, xd.abs(), 193))),
           "C2": R.worst_ratio(outs["C2"], *R.c2_reference(outs["C"]))}
    normal = x.float().abs() >= R.BF16_MIN_NORMAL
    assert torch.equal(bits(outs["C"])[normal], bits(x)[normal])
    ones = torch.zeros(340, 192)
    ones[:, 0] = 1.0
    w = torch.zeros(192, 192)
    w[:, 0] = 1.0
    case4 = case._replace(mode=4)
    got = launch(case4, {"a": ones.to(BF16), "b": w.to(BF16), "aux": x}, True, dgx_dev, reserved)["C"]
    gref = R.gelu_grad64(xd)
    one, zero = torch.ones_like(xd), torch.zeros_like(xd)                  # y = 1 exactly: one product, nothing to round
    res["C.mode4"] = R.worst_ratio(got, gref, R.gelu_grad_bound(gref, one, zero, gref, xd))
    ref2 = R.c2_reference(outs["C"])[0]
    print("USED gemm %s G=%.4f G'=%.4f" % (R.FORM_NAMES[form], R.share_used(outs["C2"], ref2, R.G_CDF * outs["C"].double().abs().clamp_min(1.0)),
                                          R.share_used(got, gref, R.G_GRAD * xd.abs().clamp_min(1.0))))
    R.report(R.FORM_NAMES[form], "sweep-340x192x192", res)


# ------------------------------------------------------------------ the same launch twice
@pytest.mark.parametrize("case", [c for c in R.CASES if c.row in ("S", "I")], ids=R.case_id)
def test_split_k_and_walked_items_are_deterministic(case, dgx_dev, reserved):
    inp = R.inputs(case, "ordinary")
    first = launch(case, inp, True, dgx_dev, reserved)
    second = launch(case, inp, True, dgx_dev, reserved)
    for name in first:
        assert torch.equal(bits(first[name]), bits(second[name])), (R.case_id(case), name)
