"""GPU: self copy-paste (INPUT.USE_COPY_METHOD 'self_copy' / 'both' / 'p:<f>').  dgx_self_copy_paste and layers.self_copy_paste
bit-exact (np.array_equal, no tolerance anywhere) against the reference's own CopyPaste.__call__ outputs (tests/golden/self_copy.npz)
and against the numpy restatement (tests/_selfcopy_ref.py) on ragged geometries; every output byte written; argument errors; the
'both' chain (pool compositor, then self copy); the real loader with worker processes and a short training run.
Reference: DG/divergen/data/transforms/custom_copypaste.py:242-506; DG/divergen/data/custom_build_copypaste_mapper.py:873-936."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _selfcopy_ref as SR  # noqa: E402


def _scene(rng, n, h, w, big=False):
    """image, n blob masks (0/1 bytes; some empty when n is large), their boxes and labels."""
    img = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    masks = np.zeros((n, h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        if n > 8 and i % 9 == 4:
            continue                                   # an empty mask
        ry, rx = (rng.integers(2, max(3, h // (2 if big else 4))), rng.integers(2, max(3, w // (2 if big else 4))))
        cy, cx = rng.integers(0, h), rng.integers(0, w)
        masks[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1
    boxes = SR.mask_boxes(masks)
    labels = rng.integers(0, 1203, n).astype(np.int64)
    return img, masks, boxes, labels


def _gpu(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _run_layer(dst, src, sel, lazy=False, canvas_hw=None):
    from divergen_amd.layers import self_copy_paste
    out = self_copy_paste(*_gpu(*dst), *_gpu(*src), sel, canvas_hw=canvas_hw, lazy_masks=lazy)
    torch.cuda.synchronize()
    return out


def _assert_equal(out, ref):
    masks = out["masks"].index_select(0, out["keep"]) if "keep" in out else out["masks"]
    assert np.array_equal(out["image"].cpu().numpy(), ref["image"])
    assert np.array_equal(masks.cpu().numpy(), ref["masks"])
    assert np.array_equal(out["boxes"].cpu().numpy(), ref["boxes"]) and out["boxes"].dtype == torch.float32
    assert np.array_equal(out["labels"].cpu().numpy(), ref["labels"])
    assert "source" not in out


def _golden_cases():
    z = np.load(os.path.join(GOLD, "self_copy.npz"))
    return z, [str(c) for c in z["cases"]]


def test_layer_equals_reference_golden():
    z, cases = _golden_cases()
    assert len(cases) == 10
    for ci, c in enumerate(cases):
        g = lambda k: z["%s_%s" % (c, k)]      # noqa: E731
        out = _run_layer((g("dst_image"), g("dst_masks"), g("dst_boxes"), g("dst_labels")),
                         (g("src_image"), g("src_masks"), g("src_boxes"), g("src_labels")), g("sel"), lazy=bool(ci % 2))
        _assert_equal(out, dict(image=g("out_image"), masks=g("out_masks"), boxes=g("out_boxes"), labels=g("out_labels")))


RAGGED = [((77, 101), (64, 80)), ((30, 24), (50, 37)), ((3, 3), (9, 33)), ((64, 80), (64, 80)), ((48, 64), (100, 131))]


@pytest.mark.parametrize("geom", RAGGED)
def test_kernel_equals_restatement_on_ragged_sizes(geom):
    (h1, w1), (hs, ws) = geom
    rng = np.random.default_rng(h1 * 1000 + ws)
    n_checked = 0
    for n0, m in itertools.product((0, 4, 70), (0, 1, 31, 99)):
        ns = max(m, 1) + 3
        dst = _scene(rng, n0, h1, w1, big=True)
        src = _scene(rng, ns, hs, ws)
        sel = rng.permutation(ns)[:m]
        ref = SR.self_copy(*dst, *src, sel)
        out = _run_layer(dst, src, sel, lazy=bool(n0 % 8))
        _assert_equal(out, ref)
        n_checked += 1
    assert n_checked == 12


def _raw_call(dst, src, sel, H, W, sentinel=0xA5):
    """dgx_self_copy_paste itself, outputs pre-filled with a sentinel; returns numpy outputs and the return code."""
    from divergen_amd import _lib as L
    di, dm, db, _ = dst
    si, sm, _, _ = src
    n0, m, ns = len(dm), len(sel), len(sm)
    t = _gpu(di, dm, db.astype(np.float32), si, sm, np.asarray(sel, dtype=np.int32))
    oi = torch.full((3, H, W), sentinel, dtype=torch.uint8, device="cuda")
    om = torch.full((n0 + m, H, W), sentinel, dtype=torch.uint8, device="cuda")
    ob = torch.full((n0, 4), -7.0, dtype=torch.float32, device="cuda")
    ov = torch.full((n0,), sentinel, dtype=torch.uint8, device="cuda")
    work = torch.empty(((n0 * 5 + 3) & ~3) + max(H, 1) * ((max(W, 1) + 15) // 16) * 4, dtype=torch.int32, device="cuda")
    p = lambda x: x.data_ptr() if x.numel() else None      # noqa: E731
    rc = L.lib().dgx_self_copy_paste(p(t[0]), p(t[1]), p(t[2]), n0, di.shape[1], di.shape[2], p(t[3]), p(t[4]), ns, si.shape[1], si.shape[2],
                                     p(t[5]), m, H, W, oi.data_ptr(), p(om), p(ob), p(ov), work.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return rc, oi.cpu().numpy(), om.cpu().numpy(), ob.cpu().numpy(), ov.cpu().numpy()


@pytest.mark.parametrize("geom", [((77, 101), (64, 80)), ((64, 80), (96, 112)), ((30, 24), (50, 37))])
def test_every_output_byte_is_written(geom):
    (h1, w1), (hs, ws) = geom
    rng = np.random.default_rng(11)
    dst, src = _scene(rng, 6, h1, w1, big=True), _scene(rng, 9, hs, ws)
    sel = np.array([7, 2, 5])
    H, W = SR.canvas_hw((h1, w1), src[2][sel])
    for sentinel in (0xA5, 0x01):          # two fills: a byte the kernel left alone cannot equal both
        rc, oi, om, ob, ov = _raw_call(dst, src, sel, H, W, sentinel)
        assert rc == 0
        ref = SR.self_copy(*dst, *src, sel)
        upd = np.where(SR.pad_to_hw(src[1][sel], H, W).any(0)[None], 0, SR.pad_to_hw(dst[1], H, W))
        assert np.array_equal(oi, ref["image"])
        assert np.array_equal(om, np.concatenate([upd, SR.pad_to_hw(src[1][sel], H, W)]))
        assert np.array_equal(ob, SR.mask_boxes(upd)) and np.array_equal(ov.astype(bool), ref["valid"])


def test_kernel_level_m0_ns0_n0_are_legal():
    """m == 0 / ns == 0 at the C entry: out_image is the padded destination, every destination object valid with its mask-derived
    box; n0 == 0: image and source planes only."""
    rng = np.random.default_rng(5)
    dst, src = _scene(rng, 5, 40, 56, big=True), _scene(rng, 4, 33, 47)
    empty_src = (np.zeros((3, 0, 0), np.uint8), np.zeros((0, 0, 0), np.uint8), np.zeros((0, 4), np.float32), np.zeros(0, np.int64))
    for s in (src, empty_src):
        rc, oi, om, ob, ov = _raw_call(dst, s, [], 52, 70)
        assert rc == 0
        assert np.array_equal(oi, SR.pad_to_hw(dst[0], 52, 70)) and np.array_equal(om, SR.pad_to_hw(dst[1], 52, 70))
        assert np.array_equal(ob, SR.mask_boxes(dst[1])) and ov.tolist() == [1] * 5
    none = _scene(rng, 0, 40, 56)
    rc, oi, om, ob, ov = _raw_call(none, src, [1, 3], 40, 56)
    assert rc == 0 and np.array_equal(om, SR.pad_to_hw(src[1][[1, 3]], 40, 56))
    assert np.array_equal(oi, SR.self_copy(*none, *src, [1, 3])["image"][:, :40, :56])


def test_bad_arguments():
    from divergen_amd import _lib as L
    assert L.DGX_ERR_BAD_ARG == -1 if hasattr(L, "DGX_ERR_BAD_ARG") else True
    rng = np.random.default_rng(6)
    dst, src = _scene(rng, 3, 32, 48), _scene(rng, 120, 32, 48)
    assert _raw_call(dst, src, list(range(100)), 32, 48)[0] == -1           # m > 99
    assert _raw_call(dst, src, [0], 31, 48)[0] == -1           # H < h1
    assert _raw_call(dst, src, [0], 32, 47)[0] == -1           # W < w1
    from divergen_amd.layers import self_copy_paste
    with pytest.raises(ValueError):                            # sel out of range: a host-side check
        self_copy_paste(*_gpu(*dst), *_gpu(*src), [0, 120])
    with pytest.raises(ValueError):
        self_copy_paste(*_gpu(*dst), *_gpu(*src), [-1])
    with pytest.raises(ValueError):
        self_copy_paste(*_gpu(*dst), *_gpu(*src), list(range(100)))
    with pytest.raises(L.DgxError):                            # no CPU fallback
        self_copy_paste(*[torch.from_numpy(a) for a in dst], *[torch.from_numpy(a) for a in src], [0])


def test_1024_square():
    rng = np.random.default_rng(1024)
    dst, src = _scene(rng, 20, 1024, 1024), _scene(rng, 40, 1024, 1024)
    sel = rng.permutation(40)[:25]
    _assert_equal(_run_layer(dst, src, sel, lazy=True), SR.self_copy(*dst, *src, sel))


def test_both_chain_pool_compositor_then_self_copy():
    """'both' on the GPU: dgx_copy_paste pastes the pool patches, dgx_self_copy_paste pastes the real instances on that result ==
    the reference's InstPool._copy_paste chain followed by its CopyPaste.__call__ (golden case 'both'), and == the restatement fed
    the compositor's own output."""
    from divergen_amd.layers import copy_paste, self_copy_paste
    z, _ = _golden_cases()
    g = lambda k: z["both_%s" % k]      # noqa: E731
    pastes = [(g("p%d_rgba" % k), int(g("p%d_xy" % k)[0]), int(g("p%d_xy" % k)[1]), int(g("p%d_label" % k)[0])) for k in range(int(g("K")))]
    mid = copy_paste(*_gpu(g("pre_image"), g("pre_masks"), g("pre_boxes"), g("pre_labels")), pastes)
    assert int(mid["source"].sum()) >= 3
    for k, name in (("image", "dst_image"), ("masks", "dst_masks"), ("boxes", "dst_boxes"), ("labels", "dst_labels")):
        assert np.array_equal(mid[k].cpu().numpy(), g(name)), name          # the pool half equals the reference's
    src = _gpu(g("src_image"), g("src_masks"), g("src_boxes"), g("src_labels"))
    out = self_copy_paste(mid["image"], mid["masks"], mid["boxes"], mid["labels"], *src, g("sel"), lazy_masks=True)
    _assert_equal(out, dict(image=g("out_image"), masks=g("out_masks"), boxes=g("out_boxes"), labels=g("out_labels")))
    ref = SR.self_copy(*[mid[k].cpu().numpy() for k in ("image", "masks", "boxes", "labels")], g("src_image"), g("src_masks"),
                       g("src_boxes"), g("src_labels"), g("sel"))
    _assert_equal(out, ref)


def _loader_cfg(tmp_path, extra=()):
    from tests.test_gpu_loader import _mini_cfg
    return _mini_cfg(tmp_path, 128, 4, ["INPUT.USE_COPY_METHOD", "both"] + list(extra))


def test_loader_with_workers_equals_one_process_with_both(tmp_path, monkeypatch):
    """The real loader, 4 worker processes, INPUT.USE_COPY_METHOD 'both': every batch equals the mapper run inline with the workers'
    seeds, the Instances carry gt_boxes / gt_classes / gt_masks only, and each sample equals the restatement applied to the
    pool-pasted sample and the worker's source."""
    from divergen_amd.data import build as B
    from divergen_amd.data.copypaste import InstPool
    from divergen_amd.data.samplers import RepeatFactorTrainingSampler
    cfg, info = _loader_cfg(tmp_path)
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    seed, per_gpu, nb = 3, 2, 6
    it = B.build_detection_train_loader(cfg, per_gpu, "cuda", seed)
    got = [next(it) for _ in range(nb)]
    torch.cuda.synchronize()
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
    mapper = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    mapper.set_dataset(dicts)
    plain = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    plain.set_dataset(dicts)
    plain.pack = False
    rf = RepeatFactorTrainingSampler.repeat_factors_from_category_frequency(dicts, cfg.DATALOADER.REPEAT_THRESHOLD)
    idx = list(itertools.islice(iter(RepeatFactorTrainingSampler(rf, seed=seed)), nb * per_gpu))
    pasted = grown = 0
    for w in range(4):
        wseed = (seed * 1009 + w) % (2 ** 31)
        np.random.seed(wseed)
        mapper.inst_pool.seed(wseed)
        for b in range(w, nb, 4):
            for j in range(per_gpu):
                want = mapper.finish(mapper(dicts[idx[b * per_gpu + j]]), "cuda")
                have = got[b][j]
                assert have["file_name"] == want["file_name"] and have["scp_file_name"] == want["scp_file_name"]
                assert torch.equal(have["image"], want["image"]), (b, j)
                hi, wi = have["instances"], want["instances"]
                assert sorted(hi.get_fields()) == ["gt_boxes", "gt_classes", "gt_masks"]
                assert torch.equal(hi.gt_boxes.tensor, wi.gt_boxes.tensor) and torch.equal(hi.gt_classes, wi.gt_classes)
                assert torch.equal(hi.gt_masks.tensor, wi.gt_masks.tensor)
                assert "paste_pack" not in have and "scp_src" not in have
                assert (have["height"], have["width"]) == tuple(have["image"].shape[-2:]) == tuple(hi.image_size)
        # the same samples once more, unpacked: pool compositor on the GPU, then the numpy restatement of the self copy
        np.random.seed(wseed)
        plain.inst_pool.seed(wseed)
        for b in range(w, nb, 4):
            for j in range(per_gpu):
                raw = plain(dicts[idx[b * per_gpu + j]])
                scp = raw.pop("scp_src")
                mid = InstPool.composite(raw, torch.device("cuda"))
                mi = mid["instances"]
                m = int(scp["labels"].shape[0])
                ref = SR.self_copy(mid["image"].cpu().numpy(), mi.gt_masks.tensor.cpu().numpy().astype(np.uint8), mi.gt_boxes.tensor.cpu().numpy(),
                                   mi.gt_classes.cpu().numpy(), scp["image"].numpy(), scp["masks"].numpy(), scp["boxes"].numpy(),
                                   scp["labels"].numpy(), np.arange(m))
                have = got[b][j]
                _assert_equal(dict(image=have["image"], masks=have["instances"].gt_masks.tensor.view(torch.uint8),
                                   boxes=have["instances"].gt_boxes.tensor, labels=have["instances"].gt_classes), ref)
                pasted += m
                grown += int(tuple(have["image"].shape[-2:]) != tuple(raw["image"].shape[-2:]))
    assert pasted > 0 and it.side is not None


def test_do_train_with_both_runs_with_finite_losses(tmp_path, monkeypatch):
    import json
    sys.path.insert(0, ROOT)
    import train_net
    from divergen_amd.modeling import build_model
    cfg, info = _loader_cfg(tmp_path, ["SOLVER.MAX_ITER", 8, "SOLVER.CHECKPOINT_PERIOD", 100, "SOLVER.WARMUP_ITERS", 2, "SEED", 7])
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    torch.manual_seed(7)
    train_net.do_train(cfg, build_model(cfg))
    rows = [json.loads(line) for line in open(os.path.join(cfg.OUTPUT_DIR, "metrics.json"))]
    losses = [r["total_loss"] for r in rows if "total_loss" in r]
    assert len(losses) >= 1 and all(np.isfinite(v) for v in losses), rows
    ck = torch.load(os.path.join(cfg.OUTPUT_DIR, "model_final.pth"), map_location="cpu", weights_only=False)
    assert ck["iteration"] == 8
