"""GPU: the 'possion' blend (dgx_poisson_blend, dgx_copy_paste_blend_ws; csrc/poisson_blend.hip) against the float64 restatement
tests/_poisson_ref.py (itself pinned on the reference's own poisson_edit by tests/test_host_poisson.py).

The band rule.  The kernel's contract is |x - x*| <= DELTA = 1e-3 grey levels before the clamp, x* the exact solution.  So where
frac(x*) lies in (DELTA, 1 - DELTA), or x* is beyond [0, 255] by more than DELTA, the device byte must equal trunc(clamp(x*)); in the
thin band around the integers it may be either adjacent value; bytes outside U = F + frame must equal the input.  A uniformly
spread frac puts 2 * DELTA = 0.2 % of the bytes into the band; every case asserts, on the restatement alone and before the device
is looked at, that its band holds at most 1 % of the bytes of U.

One exception, by construction and not by measurement: a footprint that covers the WHOLE image makes every row a Laplacian row with
right-hand side A S, so x* = S exactly -- integers, every byte in the band.  That case keeps the band rule (each byte S or S - 1)
and drops the 1 % precondition, which no solver and no seed could meet there.

Each case is one bounded call (the iteration count is fixed by the host); nothing is re-run on a failure."""
import os

import numpy as np
import pytest
import torch

import _blend_ref as BR
import _poisson_ref as PR

pytestmark = pytest.mark.gpu

from divergen_amd import _lib as L  # noqa: E402
from divergen_amd import layers as la  # noqa: E402
from divergen_amd.layers.copy_paste import check_poisson_report, pack_pastes, poisson_unknowns  # noqa: E402
from oracle import compositor as OK  # noqa: E402

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = torch.from_numpy
BAND_CAP = 0.01


def soft(rng, sh, sw, gain=700.0):
    rgba = rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8)
    y2, x2 = np.mgrid[0:sh, 0:sw]
    d = np.sqrt(((x2 + 0.5 - sw / 2) / (sw / 2)) ** 2 + ((y2 + 0.5 - sh / 2) / (sh / 2)) ** 2)
    rgba[..., 3] = np.clip((1.0 - d) * gain, 0, 255).astype(np.uint8)
    return rgba


def one_paste(img, rgba, x0, y0, what, band_cap=BAND_CAP, max_iter=-1):
    """Restatement first (and its band precondition), then ONE device call; returns (device image, report row, band bytes)."""
    H, W = img.shape[1:]
    placed, m = OK.place(rgba, x0, y0, H, W)
    _, x, U = PR.solve(img, placed[:3], m[0])
    nband = int(PR.band(x, U).sum())
    if band_cap is not None:
        assert nband <= band_cap * 3 * U.sum(), "%s: the restatement's band holds %d of %d bytes: pick another seed" % (what, nband, 3 * U.sum())
    got, rep = la.poisson_blend(T(img).to(DEV), rgba, x0, y0, max_iter=max_iter)
    got, rep = got.cpu().numpy(), rep.cpu().numpy()
    print("%s: |U| = %d, band %d, report %s" % (what, int(U.sum()), nband, rep.tolist()))
    if max_iter < 0:
        cap = L.lib().dgx_poisson_max_iter(H, W, poisson_unknowns([0, rgba.shape[0], rgba.shape[1], x0, y0], H, W))
        assert rep[2] == 1.0 and 0 <= rep[0] <= cap and rep[3] == U.sum() and 0 <= rep[1], "%s: report %s (cap %d)" % (what, rep.tolist(), cap)
        assert PR.check_band(got, img, x, U, what) == nband
    return got, rep, nband


def golden():
    z = np.load(os.path.join(GOLD, "poisson_blend.npz"))
    pastes = [(z["src%d_rgba" % k], int(z["src%d_xy" % k][0]), int(z["src%d_xy" % k][1]), int(z["src%d_label" % k][0]))
              for k in range(int(z["K"]))]
    return z, pastes


def test_golden_geometry_band_rule_and_reference():
    """The golden's six pastes, each applied to the REFERENCE's own previous image: the band rule against the restatement, and
    against the reference itself every byte within 1 with at most (the generator's reference-vs-restatement count + the band)
    differing bytes."""
    z, pastes = golden()
    steps = z["possion_steps"]
    differing = bands = 0
    for k, (rgba, x0, y0, _) in enumerate(pastes):
        before = z["dst_image"] if k == 0 else steps[k - 1]
        got, _, nband = one_paste(before, rgba, x0, y0, "golden paste %d" % k)
        d = np.abs(got.astype(np.int64) - steps[k].astype(np.int64))
        assert d.max() <= 1, k
        differing += int((d != 0).sum())
        bands += nband
    print("golden: %d bytes differ from the reference (restatement: %d, band %d)" % (differing, int(z["possion_ref_vs_restated_mismatches"]), bands))
    assert differing <= int(z["possion_ref_vs_restated_mismatches"]) + bands


RAGGED_SEEDS = {(77, 101): 0, (30, 24): 0, (3, 3): 1, (9, 33): 0}      # the first seeds whose restatement meets the band precondition


def ragged_pastes(H, W, seed):
    """Patches flush with and overhanging every image edge and corner (the placements of test_gpu_blend_modes.py)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    pastes = []
    for i, (fx, fy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1), (0.5, 0), (0.5, 1), (0, 0.5), (1, 0.5))):
        sh, sw = max(2, H // 3), max(2, W // 3)
        over = 2 * (i % 2)
        x0 = int(round(fx * (W - sw))) + (over if fx == 1 else -over if fx == 0 else 0)
        y0 = int(round(fy * (H - sh))) + (over if fy == 1 else -over if fy == 0 else 0)
        pastes.append((soft(rng, sh, sw, rng.uniform(300, 1500)), x0, y0))
    return img, pastes


@pytest.mark.parametrize("H,W", sorted(RAGGED_SEEDS))
def test_ragged_sizes_every_edge_and_corner(H, W):
    img, pastes = ragged_pastes(H, W, RAGGED_SEEDS[(H, W)])
    for i, (rgba, x0, y0) in enumerate(pastes):
        one_paste(img, rgba, x0, y0, "%dx%d paste %d at (%d, %d)" % (H, W, i, x0, y0))


def big_case():
    rng = np.random.default_rng(7)
    return rng.integers(0, 256, (3, 256, 320), dtype=np.uint8), soft(rng, 120, 150), 70, 60


def test_256x320_with_a_120x150_footprint():
    img, rgba, x0, y0 = big_case()
    one_paste(img, rgba, x0, y0, "256x320")


def test_empty_footprint_still_solves_the_frame():
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (3, 40, 56), dtype=np.uint8)
    rgba = rng.integers(0, 256, (10, 12, 4), dtype=np.uint8)
    rgba[..., 3] = 0
    got, rep, _ = one_paste(img, rgba, 9, 7, "alpha 0 everywhere")
    assert rep[3] == 2 * 40 + 2 * 56 - 4 and (got != img).sum() > 0.9 * 3 * rep[3]      # the frame quirk: nearly every frame byte moves
    assert np.array_equal(got[:, 1:-1, 1:-1], img[:, 1:-1, 1:-1])
    rgba[..., 3] = 255
    got2, _, _ = one_paste(img, rgba, 200, -50, "rectangle wholly outside the image")
    assert np.array_equal(got2, got)


def test_full_image_footprint():
    """x* = S exactly (see the module docstring): every byte is S or S - 1, nothing else; the 1 % precondition cannot apply."""
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (3, 33, 47), dtype=np.uint8)
    rgba = rng.integers(0, 256, (37, 51, 4), dtype=np.uint8)
    rgba[..., 3] = rng.integers(1, 256, (37, 51), dtype=np.uint8)
    got, rep, nband = one_paste(img, rgba, -2, -2, "full image", band_cap=None)
    S = rgba[2:35, 2:49, :3].transpose(2, 0, 1).astype(np.int64)
    assert nband == got.size and rep[3] == 33 * 47
    assert (((got == S) | (got == np.maximum(S - 1, 0)))).all()


def prefix_images(img, masks, boxes, labels, pastes, modes):
    """The device image after every paste: copy_paste over the first k pastes, k = 1..K (the kernels are deterministic)."""
    outs = []
    for k in range(1, len(pastes) + 1):
        outs.append(la.copy_paste(T(img).to(DEV), T(masks).to(DEV), T(boxes).to(DEV), T(labels).to(DEV), pastes[:k], modes=modes[:k],
                                  allow_poisson=True))
    return outs


def check_chain(img, masks, boxes, labels, pastes, modes, what):
    H, W = img.shape[1:]
    outs = prefix_images(img, masks, boxes, labels, pastes, modes)
    before = img
    for k, ((rgba, x0, y0, _), mode) in enumerate(zip(pastes, modes)):
        got = outs[k]["image"].cpu().numpy()
        placed, m = OK.place(np.asarray(rgba), x0, y0, H, W)
        if mode == 3:
            _, x, U = PR.solve(before, placed[:3], m[0])              # re-seeded from the device image of the previous step
            assert PR.band(x, U).sum() <= BAND_CAP * 3 * U.sum(), "%s: step %d band" % (what, k)
            PR.check_band(got, before, x, U, "%s step %d" % (what, k))
        else:
            assert np.array_equal(got, BR.blend(before, placed[:3], placed[3], mode)), "%s: step %d (mode %d)" % (what, k, mode)
        before = got
    out = outs[-1]
    rep = check_poisson_report(out["poisson_report"], modes)
    assert rep.shape == (len(pastes), 4)
    for k, mode in enumerate(modes):
        if mode == 3:
            assert rep[k, 2] == 1.0 and rep[k, 0] <= L.lib().dgx_poisson_max_iter(H, W, H * W)
        else:
            assert not rep[k].any()
    basic = la.copy_paste(T(img).to(DEV), T(masks).to(DEV), T(boxes).to(DEV), T(labels).to(DEV), pastes)
    lazy = la.copy_paste(T(img).to(DEV), T(masks).to(DEV), T(boxes).to(DEV), T(labels).to(DEV), pastes, modes=modes, allow_poisson=True,
                         lazy_masks=True)
    lazy_basic = la.copy_paste(T(img).to(DEV), T(masks).to(DEV), T(boxes).to(DEV), T(labels).to(DEV), pastes, lazy_masks=True)
    for key in ("masks", "boxes", "labels", "source"):
        assert torch.equal(out[key], basic[key]), key
    assert torch.equal(lazy["keep"], lazy_basic["keep"]) and torch.equal(lazy["image"], out["image"])
    ref = OK.composite(img, masks, boxes, labels, pastes)
    for key in ("masks", "boxes", "labels", "source"):
        assert np.array_equal(out[key].cpu().numpy(), ref[key]), key


def test_mixed_chain_golden():
    z, pastes = golden()
    check_chain(z["dst_image"], z["dst_masks"], z["dst_boxes"], z["dst_labels"], pastes, z["mixed4_modes"].tolist(), "mixed4")
    assert z["mixed4_modes"].tolist().count(3) >= 1 and set(z["mixed4_modes"].tolist()) == {0, 1, 2, 3}


def test_mixed_chain_poisson_first_and_between():
    """'possion' as the first paste (the cover words come from a launch that folds nothing), between other modes, and last."""
    from test_gpu_blend_modes import ragged
    img, masks, boxes, labels, pastes, _ = ragged(77, 101, 3, 7, 12)
    check_chain(img, masks, boxes, labels, pastes, [3, 1, 2, 3, 3, 0, 3], "77x101")


def _raw_ws(img, masks, boxes, pastes, modes, work_bytes, entry="ws"):
    H, W = img.shape[1:]
    n0, K = masks.shape[0], len(pastes)
    pk = pack_pastes(pastes, DEV)
    image = T(img).to(DEV)
    out_masks = torch.full((n0 + K, H, W), 7, dtype=torch.uint8, device=DEV)
    out_boxes = torch.full((n0 + K, 4), -1.0, device=DEV)
    out_valid = torch.full((n0 + K,), 9, dtype=torch.uint8, device=DEV)
    stats = torch.full(((n0 + K) * (K + 1) * 5 + 3 + H * W,), 5, dtype=torch.int32, device=DEV)
    m, b = T(masks).to(DEV), T(boxes).to(DEV)
    work = torch.zeros(max(1, (work_bytes + 7) // 8), dtype=torch.float64, device=DEV) if work_bytes is not None else None
    mh = np.ascontiguousarray(modes, dtype=np.uint8) if modes is not None else None
    args = [L.ptr(image), L.ptr(m) if n0 else None, L.ptr(b) if n0 else None, n0, H, W, L.ptr(pk.flat), L.ptr(pk.desc), K,
            L.ptr(out_masks), L.ptr(out_boxes), L.ptr(out_valid), L.ptr(stats), mh.ctypes.data if mh is not None else None]
    if entry == "ws":
        rc = L.lib().dgx_copy_paste_blend_ws(*args, L.ptr(work), work_bytes or 0, L.stream())
    else:
        rc = L.lib().dgx_copy_paste_blend(*args, L.stream())
    torch.cuda.synchronize()
    return rc, [t.cpu() for t in (image, out_masks, out_boxes, out_valid, stats)]


def test_modes_0_to_2_through_ws_equal_dgx_copy_paste_blend():
    from test_gpu_blend_modes import ragged
    img, masks, boxes, labels, pastes, _ = ragged(77, 101, 3, 7, 4)
    for modes in ([0, 1, 2, 0, 2, 1, 1], [0] * 7, None):
        rc0, base = _raw_ws(img, masks, boxes, pastes, modes, None, "blend")
        rc1, got = _raw_ws(img, masks, boxes, pastes, modes, None, "ws")               # no workspace needed without a mode-3 paste
        assert rc0 == rc1 == 0
        for a, b in zip(got, base):
            assert torch.equal(a, b)


def test_report_and_bounded_early_stop():
    """max_iter = 1 on the 120 x 150 footprint: the call returns normally, the flag is 0, the image holds the first iterate, and
    check_poisson_report raises.  A bounded early stop, nothing else."""
    img, rgba, x0, y0 = big_case()
    got, rep, _ = one_paste(img, rgba, x0, y0, "256x320, max_iter 1", max_iter=1)
    assert rep[0] == 1.0 and rep[2] == 0.0 and rep[1] > 1.0 and np.isfinite(rep[1])
    with pytest.raises(RuntimeError, match="paste 0"):
        check_poisson_report(rep[None])
    assert got.shape == img.shape


def test_refusals():
    from test_gpu_blend_modes import ragged
    img, masks, boxes, labels, pastes, _ = ragged(30, 24, 2, 5, 3)
    need = int(L.lib().dgx_poisson_work_bytes(30, 24, 30 * 24))
    before = T(img)
    rc, got = _raw_ws(img, masks, boxes, pastes, [0, 1, 3, 0, 0], 256)                 # short workspace: nothing launched
    assert rc == -1 and torch.equal(got[0], before) and (got[3] == 9).all()
    rc, got = _raw_ws(img, masks, boxes, pastes, [0, 1, 3, 0, 0], None)                # no workspace at all
    assert rc == -1 and torch.equal(got[0], before)
    rc, _ = _raw_ws(img, masks, boxes, pastes, [0, 1, 4, 0, 0], need)                  # mode byte 4
    assert rc == -1
    rc, _ = _raw_ws(img, masks, boxes, pastes, [0, 1, 3, 0, 0], need)
    assert rc == 0
    rc, _ = _raw_ws(img, masks, boxes, pastes, [0, 1, 3, 0, 0], None, "blend")         # dgx_copy_paste_blend itself: still BAD_ARG
    assert rc == -1
    rgba = np.full((2, 2, 4), 200, np.uint8)
    tiny = np.zeros((3, 2, 9), np.uint8)
    rc, _ = _raw_ws(tiny, np.zeros((0, 2, 9), np.uint8), np.zeros((0, 4), np.float32), [(rgba, 0, 0, 1)], [3], 1 << 20)
    assert rc == -2                                                                     # DGX_ERR_UNSUPPORTED: H < 3
    # the unit entry point
    d = np.array([0, 2, 2, 0, 0], np.int32)
    flat = T(rgba.reshape(-1)).to(DEV)
    work = torch.zeros(1 << 17, dtype=torch.float64, device=DEV)
    t = T(tiny).to(DEV)
    assert L.lib().dgx_poisson_blend(L.ptr(t), L.ptr(flat), d.ctypes.data, 2, 9, L.ptr(work), work.numel() * 8, -1, L.stream()) == -2
    ok = torch.zeros(3, 8, 9, dtype=torch.uint8, device=DEV)
    assert L.lib().dgx_poisson_blend(L.ptr(ok), L.ptr(flat), d.ctypes.data, 8, 9, L.ptr(work), 512, -1, L.stream()) == -1
    assert L.lib().dgx_poisson_blend(L.ptr(ok), L.ptr(flat), d.ctypes.data, 8, 9, None, 1 << 20, -1, L.stream()) == -1
    torch.cuda.synchronize()
    assert not ok.any()


def test_loader_chain_sample_with_cp_poisson(tmp_path, monkeypatch):
    """INPUT.CP_POISSON + CP_METHOD ['possion'] through CopyPasteMapper: worker half (prepare + pack_sample, mode bytes 3 and the host
    descriptors next to the blob), training half (finish -> InstPool.composite -> dgx_copy_paste_blend_ws).  The finished image equals
    the compositor called on the same pack, and every paste of it satisfies the band rule."""
    from test_gpu_loader import _mini_cfg
    from divergen_amd.data import build as B
    cfg, info = _mini_cfg(tmp_path, 128, 0, ["INPUT.CP_METHOD", ["possion"], "INPUT.CP_POISSON", True])
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
    mapper = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    mapper.set_dataset(dicts)
    assert mapper.inst_pool.cp_method == ["possion"] and mapper.inst_pool.allow_poisson
    B._worker_init(0, 77, in_worker=False, pool=mapper.inst_pool)
    prepared = None
    for d in dicts:                                    # a sample with a handful of pastes (host work only)
        cand = mapper(d)
        if 2 <= int(cand.get("blob_K", 0)) <= 5:
            prepared = cand
            break
    assert prepared is not None and prepared["blob_modes"].tolist() == [3] * prepared["blob_K"] and "blob_desc" in prepared
    host = B.unpack_sample(dict(prepared), "cpu")
    pk = host["paste_pack"]
    flat = pk["flat"].numpy()
    pastes = [(flat[o:o + h * w * 4].reshape(h, w, 4), x0, y0, int(lab)) for (o, h, w, x0, y0), lab in zip(pk["desc"].tolist(), pk["labels"].tolist())]
    have = mapper.finish(prepared, "cuda")
    inst = host["instances"]
    img, masks = host["image"].numpy(), inst.gt_masks.tensor.view(torch.uint8).numpy()
    boxes, labels = inst.gt_boxes.tensor.numpy(), inst.gt_classes.numpy()
    outs = prefix_images(img, masks, boxes, labels, pastes, [3] * len(pastes))
    assert torch.equal(have["image"], outs[-1]["image"])
    assert torch.equal(have["instances"].gt_boxes.tensor, outs[-1]["boxes"])
    H, W = img.shape[1:]
    before = img
    for k, (rgba, x0, y0, _) in enumerate(pastes):
        placed, m = OK.place(rgba, x0, y0, H, W)
        _, x, U = PR.solve(before, placed[:3], m[0])
        assert PR.band(x, U).sum() <= BAND_CAP * 3 * U.sum()
        got = outs[k]["image"].cpu().numpy()
        PR.check_band(got, before, x, U, "loader sample, paste %d" % k)
        before = got
    check_poisson_report(outs[-1]["poisson_report"])
