"""The RoI pooling kernels (csrc/roi_align.hip) through the C ABI -- so that the test, not layers/roi_ops.py, chooses the kernel form --
against the float64 restatements of tests/_roi_ref64.py: every element of every output inside its a-priori bound, exact where the bound
is zero (elements no sample reaches, pixels no box reaches), levels_out equal to the rule, the mask-crop bits equal.  Outputs and gather
maps start from NaN and every buffer lies between sentinel guards: every element must be written and nothing beside the buffer.  One
pass goes through la.roi_pooler / la.roi_align with autograd for the Python routing.  Each test prints
`RATIO roi <kernel> <case> <output>=<worst error / bound> ...` before it asserts (pytest -s shows them)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _roi_ref64 as R  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENT = -7.5                  # exact in bf16
GUARD = 64                   # sentinel elements either side of every buffer (a multiple of 16 bytes in both dtypes)
NAN = float("nan")
DGX_ERR_UNSUPPORTED = -2
NAMES = list(R.BOXES) + list(R.LEVEL_BOXES)
DT = {"f32": F32, "bf16": BF16}


def L_():
    from divergen_amd import _lib as L
    return L


class Buf:
    """a device buffer between two guards; `offset` bytes move the payload off 16-byte alignment"""

    def __init__(self, shape, dtype, fill=NAN, offset=0):
        n = int(np.prod(shape))
        sent = SENT if dtype.is_floating_point else 0x55
        off = offset // torch.empty(0, dtype=dtype).element_size()
        self.whole = torch.full((GUARD + off + n + GUARD,), sent, dtype=dtype, device=DEV)
        self.lo, self.hi, self.sent = GUARD + off, GUARD + off + n, sent
        self.t = self.whole[self.lo:self.hi].view(shape)
        if isinstance(fill, (float, int)):
            self.t.fill_(fill)
        else:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(fill)).to(dtype).view(shape))
        assert self.t.data_ptr() % 16 == offset % 16

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.whole[:self.lo] == self.sent).all()) and bool((self.whole[self.hi:] == self.sent).all())

    def np(self):
        return self.t.float().cpu().numpy().astype(np.float64) if self.t.dtype.is_floating_point else self.t.cpu().numpy()

    def bits(self):
        return self.t.contiguous().view(torch.int16 if self.t.dtype == BF16 else torch.int32).cpu()


def maps_of(c):
    return {"single": R.LEVELS[:1], "small": [R.SMALL]}.get(c.get("levels"), R.LEVELS)


def values(shape, seed, dt):
    v = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return R.to_bf16(v) if dt == "bf16" else v


def ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def ptrs(bufs):
    return (ctypes.c_void_p * len(bufs))(*[b.ptr() for b in bufs])


def scales_of(maps):
    return R.pooler_scales(len(maps)) if len(maps) > 1 else [R.SCALE0]


def min_level_of(maps):
    return R.MIN_LEVEL if len(maps) > 1 else 0


def run_fwd(feats, rois, maps, C, S, sr, aligned, nhwc, dt, offset=0):
    """feats: list of (N, H, W, C) fp32 arrays holding values of dtype dt -> (out (R, S, S, C) float64, levels or None)"""
    L, lib = L_(), L_().lib()
    Rn, nl = len(rois), len(maps)
    fb = [Buf(f.shape, DT[dt], f) for f in feats]
    rb = Buf(rois.shape, F32, rois)
    out = Buf((Rn, S, S, C) if nhwc else (Rn, C, S, S), DT[dt], NAN, offset)
    code = L.DGX_BF16 if dt == "bf16" else L.DGX_F32
    lv = None
    if nl == 1:
        H, W = maps[0]
        L.check(lib.dgx_roi_align_fwd(fb[0].ptr(), rb.ptr(), out.ptr(), R.N_IMG, H, W, C, Rn, R.SCALE0, S, S, sr, aligned, nhwc, code,
                                      L.stream()), "dgx_roi_align_fwd")
    else:
        lv = Buf((Rn,), torch.int32, -77)
        L.check(lib.dgx_roi_pooler_fwd(ptrs(fb), ints([h for h, _ in maps]), ints([w for _, w in maps]), nl, R.MIN_LEVEL, rb.ptr(), out.ptr(),
                                       lv.ptr(), R.N_IMG, C, Rn, S, S, sr, nhwc, code, L.stream()), "dgx_roi_pooler_fwd")
    torch.cuda.synchronize()
    assert out.guards_intact() and rb.guards_intact() and all(b.guards_intact() for b in fb) and (lv is None or lv.guards_intact())
    got = out.np()
    return (got if nhwc else got.transpose(0, 2, 3, 1)), (None if lv is None else lv.np()), out


def check_levels(lv, rois, maps):
    if lv is not None:
        want = [R.level_of(r, R.MIN_LEVEL, len(maps)) for r in rois]
        assert lv.tolist() == want, [(i, a, b) for i, (a, b) in enumerate(zip(lv.tolist(), want)) if a != b]


def run_scatter(go, rois, maps, C, S, sr, aligned, nhwc, dt, offset=0):
    """go (R, S, S, C) fp32 array of dtype-dt values -> list of (N, H, W, C) float64 gradients (the caller's zeroed fp32 maps)"""
    L, lib = L_(), L_().lib()
    Rn, nl = len(rois), len(maps)
    gb = Buf(go.shape if nhwc else (Rn, C, S, S), DT[dt], go if nhwc else go.transpose(0, 3, 1, 2), offset)
    rb = Buf(rois.shape, F32, rois)
    grads = [Buf((R.N_IMG, H, W, C), F32, 0.0) for H, W in maps]
    code = L.DGX_BF16 if dt == "bf16" else L.DGX_F32
    if nl == 1:
        H, W = maps[0]
        L.check(lib.dgx_roi_align_bwd(gb.ptr(), rb.ptr(), grads[0].ptr(), R.N_IMG, H, W, C, Rn, R.SCALE0, S, S, sr, aligned, nhwc, code,
                                      L.stream()), "dgx_roi_align_bwd")
    else:
        L.check(lib.dgx_roi_pooler_bwd(gb.ptr(), ptrs(grads), ints([h for h, _ in maps]), ints([w for _, w in maps]), nl, R.MIN_LEVEL,
                                       rb.ptr(), R.N_IMG, C, Rn, S, S, sr, nhwc, code, L.stream()), "dgx_roi_pooler_bwd")
    torch.cuda.synchronize()
    assert gb.guards_intact() and all(b.guards_intact() for b in grads)
    return [g.np() for g in grads]


def run_gather(go, rois, maps, n_img, C, S, sr, aligned, dt, prev=None, gscale=1.0, go_offset=0, map_offset=0, expect=0):
    """-> the maps as Buf (NaN before the launch when prev is None, else prev with accumulate = 1)"""
    L, lib = L_(), L_().lib()
    Rn, nl = len(rois), len(maps)
    gb = Buf(go.shape, DT[dt], go, go_offset)
    rb = Buf((max(Rn, 1), 5), F32, rois if Rn else 0.0)
    out = [Buf((n_img, H, W, C), DT[dt], NAN if prev is None else prev[l], map_offset) for l, (H, W) in enumerate(maps)]
    code = L.DGX_BF16 if dt == "bf16" else L.DGX_F32
    rc = lib.dgx_roi_pooler_bwd_gather_accum(gb.ptr(), ptrs(out), ints([h for h, _ in maps]), ints([w for _, w in maps]), nl, min_level_of(maps),
                                             R.SCALE0, aligned, rb.ptr(), n_img, C, Rn, S, S, sr, int(prev is not None), gscale, code, L.stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert gb.guards_intact() and all(b.guards_intact() for b in out)
    return out


# ================================================================================================ forward
@pytest.mark.parametrize("name", list(R.FORWARD_FORMS))
def test_forward_every_element(name):
    c = R.FORWARD_FORMS[name]
    maps, C, S = maps_of(c), c["C"], c["S"]
    rois = R.rois_of(NAMES)
    worst = {}
    for dt in ("f32", "bf16"):
        feats = [values((R.N_IMG, H, W, C), 100 + l, dt) for l, (H, W) in enumerate(maps)]
        for sr in (0, 2):
            got, lv, _ = run_fwd(feats, rois, maps, C, S, sr, c.get("aligned", 1), c["nhwc"], dt, c.get("offset", 0))
            ref, A, n, _ = R.forward64(feats, rois, scales_of(maps), min_level_of(maps), S, S, sr, c.get("aligned", 1))
            worst["%s_sr%d" % (dt, sr)] = R.worst_ratio(got, ref, R.bound_of(dt, ref, A, n))
            check_levels(lv, rois, maps)
            unreached = A == 0
            assert unreached.any() and np.array_equal(got[unreached], np.zeros(int(unreached.sum())))
    R.report("fwd_" + c["form"], name, worst)


@pytest.mark.parametrize("Rn", R.R_THRESHOLDS)
def test_forward_and_scatter_at_the_nsplit_thresholds(Rn):
    """C = 24 (separable, channels-last): R = 1, 511 | 512, 2047 | 2048 give 4, 4 | 2, 2 | 1 slices of the 49 bins (tests/test_host_roi_ref.py
    holds the figures to the header's function)"""
    maps, C, S = R.LEVELS, 24, 7
    rois = R.cycled_rois(Rn)
    feats = [values((R.N_IMG, H, W, C), 200 + l, "f32") for l, (H, W) in enumerate(maps)]
    got, lv, _ = run_fwd(feats, rois, maps, C, S, 0, 1, 1, "f32")
    ref, A, n, _ = R.forward64(feats, rois, scales_of(maps), R.MIN_LEVEL, S, S, 0, 1)
    check_levels(lv, rois, maps)
    go = values((Rn, S, S, C), 210, "f32")
    grads = run_scatter(go, rois, maps, C, S, 0, 1, 1, "f32")
    sref, _ = R.scatter64(go, rois, maps, R.N_IMG, scales_of(maps), R.MIN_LEVEL, 0, 1)
    worst = {"out": R.worst_ratio(got, ref, R.f32_bound(ref, A, n))}
    for l in range(len(maps)):
        worst["grad%d" % l] = R.worst_ratio(grads[l], sref[l][0], R.f32_bound(*sref[l]))
    R.report("sep_cl", "R%d" % Rn, worst)


def test_forward_vector_and_separable_forms_agree_bit_for_bit_and_one_hot_weights():
    """C = 64, channels-last: the vector form and the separable form (reached through an output pointer 4 bytes off alignment) share the
    tables and the summation order per channel (the vector form's padding taps add 0 * v), so their results are bit-equal.  One feature
    pixel = 1 makes the output the weight table itself: WY[i][y] WX[j][x] / count, n = the table additions + the product + the division."""
    maps, C, S = R.LEVELS, 64, 7
    rois = R.rois_of(NAMES)
    for dt in ("f32", "bf16"):
        feats = [values((R.N_IMG, H, W, C), 300 + l, dt) for l, (H, W) in enumerate(maps)]
        for sr in (0, 2):
            _, _, a = run_fwd(feats, rois, maps, C, S, sr, 1, 1, dt)
            _, _, b = run_fwd(feats, rois, maps, C, S, sr, 1, 1, dt, offset=4)
            assert torch.equal(a.bits(), b.bits()), (dt, sr)
    worst = {}
    for (l, n_, y, x) in ((0, 0, 10, 12), (0, 1, 0, 0), (0, 0, 20, 26), (1, 1, 5, 6), (2, 0, 5, 6)):
        feats = [np.zeros((R.N_IMG, H, W, C), np.float32) for H, W in maps]
        feats[l][n_, y, x] = 1.0
        for sr in (0, 2):
            got, _, _ = run_fwd(feats, rois, maps, C, S, sr, 1, 1, "f32")
            ref, A, n, tabs = R.forward64(feats, rois, scales_of(maps), R.MIN_LEVEL, S, S, sr, 1)
            nt = np.array([R.table_ops(t) + 2 for t in tabs], np.float64).reshape(-1, 1, 1, 1)
            worst["l%d_%d_%d_sr%d" % (l, y, x, sr)] = R.worst_ratio(got, ref, R.f32_bound(ref, A, nt))
    R.report("fwd_vec", "one_hot", worst)


# ================================================================================================ scatter backward
@pytest.mark.parametrize("name", list(R.FORWARD_FORMS))
def test_scatter_backward_every_element(name):
    c = R.FORWARD_FORMS[name]
    maps, C, S = maps_of(c), c["C"], c["S"]
    rois = R.rois_of(NAMES)
    worst = {}
    for dt in ("f32", "bf16"):
        go = values((len(rois), S, S, C), 400, dt)
        for sr in (0, 2):
            grads = run_scatter(go, rois, maps, C, S, sr, c.get("aligned", 1), c["nhwc"], dt, c.get("offset", 0))
            sref, _ = R.scatter64(go, rois, maps, R.N_IMG, scales_of(maps), min_level_of(maps), sr, c.get("aligned", 1))
            for l in range(len(maps)):
                worst["%s_sr%d_l%d" % (dt, sr, l)] = R.worst_ratio(grads[l], sref[l][0], R.f32_bound(*sref[l]))
    R.report("bwd_" + c["form"], name, worst)


# ================================================================================================ gather backward
def check_gather(out, ref, dt):
    return {"l%d" % l: R.worst_ratio(o.np(), ref[l][0], R.bound_of(dt, *ref[l])) for l, o in enumerate(out)}


@pytest.mark.parametrize("name", list(R.GATHER_FORMS))
def test_gather_backward_every_element(name):
    c = R.GATHER_FORMS[name]
    maps, C, S, aligned = maps_of(c), c["C"], c["S"], c.get("aligned", 1)
    rois = R.rois_of(NAMES)
    worst = {}
    for dt in ("f32", "bf16"):
        go = values((len(rois), S, S, C), 500, dt)
        for sr in (0, 2):
            combos = [(0, 1.0), (1, 1.0), (0, 1.0 / 3.0), (1, 1.0 / 3.0)] if name == "c256_s7" else [(0, 1.0), (1, 1.0 / 3.0)][(sr > 0) ^ (dt == "bf16")::2]
            for acc, gs in combos:
                prev = [values((R.N_IMG, H, W, C), 510 + l, dt) for l, (H, W) in enumerate(maps)] if acc else None
                out = run_gather(go, rois, maps, R.N_IMG, C, S, sr, aligned, dt, prev, gs)
                again = run_gather(go, rois, maps, R.N_IMG, C, S, sr, aligned, dt, prev, gs)
                assert all(torch.equal(a.bits(), b.bits()) for a, b in zip(out, again)), "not reproducible"
                ref, _ = R.gather64(go, rois, maps, R.N_IMG, scales_of(maps), min_level_of(maps), sr, aligned, prev, gs)
                for k, v in check_gather(out, ref, dt).items():
                    worst["%s_sr%d_a%d_g%d_%s" % (dt, sr, acc, int(gs == 1.0), k)] = v
    R.report("gather_th4", name, worst)


@functools.lru_cache(maxsize=None)
def _th8_case():
    g = R.GATHER_TH8
    rois = R.random_rois(8, g["R"], g["N"], g["W"] * 8.0, g["H"] * 8.0)
    rois[:4, 1:] = [[-20.0, -20.0, 300.0, 200.0], [1000.0, 1000.0, 1100.0, 1100.0], [512.0, 512.0, 576.0, 640.0], [700.0, 300.0, 500.0, 100.0]]
    go = values((g["R"], g["S"], g["S"], g["C"]), 600, "bf16")
    ref = {sr: R.gather64(go, rois, [(g["H"], g["W"])], g["N"], [R.SCALE0], 0, sr, 1)[0] for sr in (0, 2)}
    return rois, go, ref


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gather_backward_eight_row_tiles(dt):
    """4 x 128 x 128 x 256: 1024 tiles of 8 rows, the smallest geometry at which launch_gather picks TH = 8; a few dozen boxes"""
    g = R.GATHER_TH8
    rois, go, ref = _th8_case()
    worst = {}
    for sr in (0, 2):
        out = run_gather(go, rois, [(g["H"], g["W"])], g["N"], g["C"], g["S"], sr, 1, dt)
        worst["sr%d" % sr] = check_gather(out, ref[sr], dt)["l0"]
    R.report("gather_th8", dt, worst)


@pytest.mark.parametrize("Rn", [0, 256, 257])
def test_gather_backward_list_loop(Rn):
    """R = 0 writes zeros over every pixel (accumulate = 0) or leaves the maps bit-unchanged (accumulate = 1); 256 | 257 boxes are one |
    two trips of the 256-wide list loop"""
    maps, C, S, dt = R.LEVELS, 64, 7, "bf16"
    rois = R.cycled_rois(Rn) if Rn else np.zeros((0, 5), np.float32)
    go = values((max(Rn, 1), S, S, C), 700, dt)[:Rn]
    prev = [values((R.N_IMG, H, W, C), 710 + l, dt) for l, (H, W) in enumerate(maps)]
    worst = {}
    for p in (None, prev):
        out = run_gather(go if Rn else np.zeros((1, S, S, C), np.float32), rois, maps, R.N_IMG, C, S, 0, 1, dt, p)
        if Rn == 0:
            for l, o in enumerate(out):
                want = np.zeros_like(prev[l]) if p is None else prev[l]
                assert torch.equal(o.bits(), torch.as_tensor(want).to(BF16).view(torch.int16)), (l, p is None)
            continue
        ref, _ = R.gather64(go, rois, maps, R.N_IMG, scales_of(maps), R.MIN_LEVEL, 0, 1, p)
        for k, v in check_gather(out, ref, dt).items():
            worst["a%d_%s" % (int(p is not None), k)] = v
    R.report("gather_th4", "R%d" % Rn, worst)


@pytest.mark.parametrize("copies", [8, 9])
def test_gather_backward_resident_batch_and_empty_image_and_levels(copies):
    """exactly 8 | 9 boxes reach the same tiles (one | two batches of GT_QB resident tables); all of them on image 1 and level 0: image 0
    and levels 1, 2 get no box and must still be written -- zeros, or the earlier contents when accumulating"""
    maps, C, S, dt = R.LEVELS, 256, 7, "f32"
    rois = R.rois_of(["inside"] * copies, batch=[1] * copies)
    go = values((copies, S, S, C), 800, dt)
    prev = [values((R.N_IMG, H, W, C), 810 + l, dt) for l, (H, W) in enumerate(maps)]
    worst = {}
    for p in (None, prev):
        out = run_gather(go, rois, maps, R.N_IMG, C, S, 2, 1, dt, p, 1.0 / 3.0)
        ref, tabs = R.gather64(go, rois, maps, R.N_IMG, scales_of(maps), R.MIN_LEVEL, 2, 1, p, 1.0 / 3.0)
        assert all(t.lvl == 0 for t in tabs)
        for k, v in check_gather(out, ref, dt).items():
            worst["a%d_%s" % (int(p is not None), k)] = v
        for l, o in enumerate(out):
            want = np.zeros_like(prev[l]) if p is None else prev[l]
            if l > 0:
                assert np.array_equal(o.np(), want.astype(np.float64))
            else:
                assert np.array_equal(o.np()[0], want[0].astype(np.float64))
    R.report("gather_th4", "copies%d" % copies, worst)


def test_gather_backward_one_hot_is_the_weight_table():
    """one go element = 1: the gradient map is WY[i][y] WX[j][x] / count * grad_scale of that bin, n = the table additions + 3"""
    maps, C, S = R.LEVELS, 64, 7
    rois = R.rois_of(NAMES)
    worst = {}
    for sr in (0, 2):
        for (r, i, j) in ((0, 3, 3), (9, 0, 6), (12, 6, 0), (16, 2, 5)):
            go = np.zeros((len(rois), S, S, C), np.float32)
            go[r, i, j] = 1.0
            out = run_gather(go, rois, maps, R.N_IMG, C, S, sr, 1, "f32")
            ref, tabs = R.gather64(go, rois, maps, R.N_IMG, scales_of(maps), R.MIN_LEVEL, sr, 1)
            nt = float(R.table_ops(tabs[r]) + 3)
            worst["sr%d_r%d" % (sr, r)] = max(R.worst_ratio(o.np(), ref[l][0], R.f32_bound(ref[l][0], ref[l][1], nt)) for l, o in enumerate(out))
    R.report("gather_th4", "one_hot", worst)


def test_gather_backward_refuses_what_it_cannot_run_and_leaves_the_maps():
    maps, C, S = R.LEVELS, 64, 7
    rois = R.rois_of(NAMES)
    go = values((len(rois), S, S, C), 900, "f32")
    for kw in (dict(go_offset=4), dict(map_offset=4)):
        out = run_gather(go, rois, maps, R.N_IMG, C, S, 0, 1, "f32", expect=DGX_ERR_UNSUPPORTED, **kw)
        assert all(bool(torch.isnan(o.t).all()) for o in out)
    go17 = values((len(rois), 17, 17, C), 901, "f32")
    out = run_gather(go17, rois, maps, R.N_IMG, C, 17, 0, 1, "f32", expect=DGX_ERR_UNSUPPORTED)
    assert all(bool(torch.isnan(o.t).all()) for o in out)


# ================================================================================================ mask crop
@pytest.mark.parametrize("case", list(R.CROP_CASES))
def test_mask_crop_bits(case):
    L, lib = L_(), L_().lib()
    S = R.CROP_CASES[case]["S"]
    masks, boxes, idx = R.crop_inputs(case)
    want, avg = R.mask_crop32(masks, boxes, idx, S)
    assert (avg[6] == 0.5).any() and (avg[7] == 0.5).any()
    mb, bb, ib = Buf(masks.shape, torch.uint8, masks), Buf(boxes.shape, F32, boxes), Buf(idx.shape, torch.int32, idx)
    out = Buf((len(boxes), S, S), torch.uint8, 0xCC)
    L.check(lib.dgx_mask_crop(mb.ptr(), bb.ptr(), ib.ptr(), out.ptr(), masks.shape[0], masks.shape[1], masks.shape[2], len(boxes), S, L.stream()),
            "dgx_mask_crop")
    torch.cuda.synchronize()
    assert out.guards_intact() and mb.guards_intact()
    assert np.array_equal(out.np(), want), np.argwhere(out.np() != want)[:10]


# ================================================================================================ the Python routing
def test_python_layer_routes_to_the_same_bounds():
    """la.roi_pooler / la.roi_align with autograd: C = 64 bf16 (vector forward, gather backward with grad_scale), C = 24 fp32 (C % 8 != 0:
    the separable NCHW forward and the NCHW scatter backward behind it), and a single level, not aligned"""
    from divergen_amd import layers as la
    maps, S = R.LEVELS, 7
    rois = R.rois_of(NAMES)
    rd = torch.from_numpy(rois).to(DEV)
    worst = {}
    for C, dt, gs in ((64, "bf16", 0.5), (24, "f32", 1.0)):
        feats = [values((R.N_IMG, H, W, C), 950 + l, dt) for l, (H, W) in enumerate(maps)]
        go = values((len(rois), S, S, C), 960, dt)
        fd = [torch.from_numpy(f).permute(0, 3, 1, 2).to(DEV).to(DT[dt]).requires_grad_(True) for f in feats]
        out = la.roi_pooler(fd, rd, S, scales_of(maps), sampling_ratio=2, grad_scale=gs)
        out.backward(torch.from_numpy(go).permute(0, 3, 1, 2).to(DEV).to(DT[dt]))
        ref, A, n, _ = R.forward64(feats, rois, scales_of(maps), R.MIN_LEVEL, S, S, 2, 1)
        worst["C%d_out" % C] = R.worst_ratio(out.detach().float().cpu().numpy().transpose(0, 2, 3, 1), ref, R.bound_of(dt, ref, A, n))
        if C % 8 == 0:
            gref, _ = R.gather64(go, rois, maps, R.N_IMG, scales_of(maps), R.MIN_LEVEL, 2, 1, None, gs)
        else:
            gref, _ = R.scatter64(go, rois, maps, R.N_IMG, scales_of(maps), R.MIN_LEVEL, 2, 1)
        for l, f in enumerate(fd):
            worst["C%d_grad%d" % (C, l)] = R.worst_ratio(f.grad.float().cpu().numpy().transpose(0, 2, 3, 1), gref[l][0], R.bound_of(dt, *gref[l]))
    H, W = maps[0]
    feat, go = values((R.N_IMG, H, W, 24), 970, "f32"), values((len(rois), S, S, 24), 971, "f32")
    f1 = torch.from_numpy(feat).permute(0, 3, 1, 2).to(DEV).requires_grad_(True)
    o1 = la.roi_align(f1, rd, R.SCALE0, S, 0, False)
    o1.backward(torch.from_numpy(go).permute(0, 3, 1, 2).to(DEV))
    ref, A, n, _ = R.forward64([feat], rois, [R.SCALE0], 0, S, S, 0, 0)
    worst["align_out"] = R.worst_ratio(o1.detach().cpu().numpy().transpose(0, 2, 3, 1), ref, R.f32_bound(ref, A, n))
    (gr, gA, gn), = R.scatter64(go, rois, maps[:1], R.N_IMG, [R.SCALE0], 0, 0, 0)[0]
    worst["align_grad"] = R.worst_ratio(f1.grad.cpu().numpy().transpose(0, 2, 3, 1), gr, R.f32_bound(gr, gA, gn))
    R.report("layers", "roi_ops", worst)
