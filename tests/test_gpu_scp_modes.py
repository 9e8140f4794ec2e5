"""GPU: what INPUT.SCP_SRC_MODES adds on the device.  dgx_remove_background / layers.remove_background and dgx_self_copy_paste_all /
layers.self_copy_paste_all, integer-exact (torch.equal / np.array_equal, no tolerance anywhere) against the reference's own
CopyPaste.remove_background and CopyPaste(selected=False).__call__ outputs (tests/golden/scp_modes.npz) and against
image * masks.any(0) / the selected paste with sel = 0 .. ns - 1; argument errors at the C entry (rejected on the host side, nothing
launched); the real loader with worker processes, 'in_domain' sources, background removal and the pool paste.
Reference: DG/divergen/data/transforms/custom_copypaste.py:101-109, :242-341; DG/divergen/data/custom_build_copypaste_mapper.py:764-936."""
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
import _scp_modes_ref as MR  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2


def _gold():
    return np.load(os.path.join(GOLD, "scp_modes.npz"))


def _gpu(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _offset(t, by=1):
    """The same values in storage whose base is `by` bytes past an aligned address (a sliced tensor)."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[by:by + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == by and out.is_contiguous()
    return out


def test_remove_background_equals_reference_golden():
    from divergen_amd.layers import remove_background
    z = _gold()
    for c in [str(c) for c in z["rb_cases"]]:
        img, masks = _gpu(z["%s_image" % c], z["%s_masks" % c])
        want = torch.from_numpy(z["%s_out" % c]).cuda()
        keep = img.clone()
        assert torch.equal(remove_background(img, masks), want) and torch.equal(img, keep), c      # out of place: the input stays
        assert torch.equal(remove_background(img, masks.view(torch.bool)), want), c
        assert remove_background(img, masks, out=img) is img and torch.equal(img, want), c         # in place


@pytest.mark.parametrize("hw", [(3, 3), (9, 33), (30, 24), (64, 80), (77, 101)])
def test_remove_background_sizes_counts_in_place_and_misaligned(hw):
    from divergen_amd.layers import remove_background
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    for n in (0, 1, 5, 70):
        img = rng.integers(1, 256, (3, h, w), dtype=np.uint8)            # no zero byte: a pixel that wrongly survives shows
        masks = np.zeros((n, h, w), np.uint8)
        for i in range(n):
            cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, max(2, min(h, w) // 3))
            masks[i] = (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r) * (1, 255, 2, 128)[i % 4]      # any non-zero byte counts
        if n >= 5:
            masks[n // 2] = 0                                            # an empty plane
        union = masks.any(0)
        assert n == 0 or union.any()
        want = torch.from_numpy(MR.remove_background(img, masks)).cuda()
        assert np.array_equal(want.cpu().numpy(), img * union[None])
        ti, tm = _gpu(img, masks)
        for sentinel in (0xA5, 0x00):                                    # every output byte is written
            out = torch.full((3, h, w), sentinel, dtype=torch.uint8, device="cuda")
            assert remove_background(ti, tm, out=out) is out and torch.equal(out, want), (n, sentinel)
        # a base 1 byte off: the byte path, also on a width that is a multiple of 16 -- image, masks and output in turn, then all
        for oi, om, oo in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            a = _offset(ti) if oi else ti
            b = _offset(tm) if om and n else tm
            out = _offset(torch.full((3, h, w), 0xA5, dtype=torch.uint8, device="cuda")) if oo else torch.full((3, h, w), 0xA5, dtype=torch.uint8, device="cuda")
            assert torch.equal(remove_background(a, b, out=out), want), (n, oi, om, oo)
        for a in (ti.clone(), _offset(ti)):                              # in place, aligned and not
            assert remove_background(a, tm, out=a) is a and torch.equal(a, want), n
    torch.cuda.synchronize()


def test_remove_background_beyond_one_grid_sweep():
    """More 16-pixel chunks than 2048 x 256 lanes: the grid-stride loop, on a width that is no multiple of 16."""
    from divergen_amd.layers import remove_background
    h, w, n = 2304, 3700, 3
    assert h * ((w + 15) // 16) > 2048 * 256
    g = torch.Generator(device="cuda").manual_seed(7)
    img = torch.randint(1, 256, (3, h, w), dtype=torch.uint8, device="cuda", generator=g)
    masks = torch.zeros(n, h, w, dtype=torch.uint8, device="cuda")
    masks[0, 100:900, 50:3000], masks[1, 800:2304, 3500:3700], masks[2, 2000:2100, 0:17] = 1, 1, 7
    want = img * masks.any(0).to(torch.uint8)[None]
    assert torch.equal(remove_background(img, masks), want)
    assert remove_background(img, masks, out=img) is img and torch.equal(img, want)


def test_remove_background_argument_errors():
    from divergen_amd import _lib as L
    from divergen_amd.layers import remove_background
    f = L.lib().dgx_remove_background
    img, masks = torch.zeros(3, 8, 8, dtype=torch.uint8, device="cuda"), torch.ones(2, 8, 8, dtype=torch.uint8, device="cuda")
    out = torch.full((3, 8, 8), 0xA5, dtype=torch.uint8, device="cuda")
    i, m, o, s = img.data_ptr(), masks.data_ptr(), out.data_ptr(), L.stream()
    for args in ((None, m, 2, 8, 8, o), (i, m, 2, 8, 8, None), (i, m, 2, 0, 8, o), (i, m, 2, 8, 0, o), (i, m, 2, -1, 8, o), (i, m, -1, 8, 8, o),
                 (i, None, 2, 8, 8, o)):
        assert f(*args, s) == BAD_ARG, args
    assert f(i, m, 2, 65536, 32768, o, s) == UNSUPPORTED                 # h * w == 2^31
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                                     # nothing was launched
    assert f(i, None, 0, 8, 8, o, s) == 0                                # n == 0 with NULL masks is legal
    torch.cuda.synchronize()
    assert not bool(out.any())
    with pytest.raises(ValueError):
        remove_background(img, masks[:, :7])
    with pytest.raises(ValueError):
        remove_background(img.float(), masks)
    with pytest.raises(ValueError):
        remove_background(img, masks, out=torch.zeros(3, 8, 9, dtype=torch.uint8, device="cuda"))
    with pytest.raises(L.DgxError):                                      # no CPU fallback
        remove_background(img.cpu(), masks.cpu())


def _assert_equal(out, ref):
    masks = out["masks"].index_select(0, out["keep"]) if "keep" in out else out["masks"]
    assert np.array_equal(out["image"].cpu().numpy(), ref["image"])
    assert np.array_equal(masks.cpu().numpy(), ref["masks"])
    assert np.array_equal(out["boxes"].cpu().numpy(), ref["boxes"]) and out["boxes"].dtype == torch.float32
    assert np.array_equal(out["labels"].cpu().numpy(), ref["labels"])
    assert "source" not in out


def test_paste_all_equals_reference_golden():
    """Every paste-all golden: ragged sizes, ns = 130 on n0 = 0 and n0 = 70 (more source objects than the selected entry's 99, more
    destination objects than one group's 64), ns = 0, n0 = 0, the 'both' chain and background removal followed by the paste."""
    from divergen_amd.layers import copy_paste, remove_background, self_copy_paste_all
    z = _gold()
    cases = [str(c) for c in z["paste_all_cases"]]
    assert cases == ["ragged_a", "ragged_b", "ragged_c", "big130_n0", "big130_n70", "ns0", "n0_0", "both"]
    for ci, c in enumerate(cases + ["rb_then_paste"]):
        g = lambda k: z["%s_%s" % (c, k)]      # noqa: E731
        dst = _gpu(g("dst_image"), g("dst_masks"), g("dst_boxes"), g("dst_labels"))
        if c == "rb_then_paste":
            dst[0] = remove_background(dst[0], dst[1])
        out = self_copy_paste_all(*dst, *_gpu(g("src_image"), g("src_masks"), g("src_boxes"), g("src_labels")), lazy_masks=bool(ci % 2))
        _assert_equal(out, dict(image=g("out_image"), masks=g("out_masks"), boxes=g("out_boxes"), labels=g("out_labels")))
        assert tuple(out["image"].shape[-2:]) == tuple(g("out_hw"))
    assert len(z["big130_n70_src_masks"]) == 130 and len(z["big130_n70_dst_masks"]) == 70 and len(z["big130_n0_dst_masks"]) == 0
    # 'both' from the start: the pool compositor's output is the golden's destination
    g = lambda k: z["both_%s" % k]      # noqa: E731
    pastes = [(g("p%d_rgba" % k), int(g("p%d_xy" % k)[0]), int(g("p%d_xy" % k)[1]), int(g("p%d_label" % k)[0])) for k in range(int(g("K")))]
    mid = copy_paste(*_gpu(g("pre_image"), g("pre_masks"), g("pre_boxes"), g("pre_labels")), pastes)
    for k, name in (("image", "dst_image"), ("masks", "dst_masks"), ("boxes", "dst_boxes"), ("labels", "dst_labels")):
        assert np.array_equal(mid[k].cpu().numpy(), g(name)), name
    out = self_copy_paste_all(mid["image"], mid["masks"], mid["boxes"], mid["labels"], *_gpu(g("src_image"), g("src_masks"), g("src_boxes"), g("src_labels")))
    _assert_equal(out, dict(image=g("out_image"), masks=g("out_masks"), boxes=g("out_boxes"), labels=g("out_labels")))


def _scene(rng, n, h, w):
    from test_gpu_self_copy import _scene as scene
    return scene(rng, n, h, w, big=True)


@pytest.mark.parametrize("geom", [((77, 101), (64, 80)), ((48, 64), (100, 131))])
def test_paste_all_of_40_equals_the_selected_paste_of_all_40(geom):
    from divergen_amd.layers import self_copy_paste, self_copy_paste_all
    (h1, w1), (hs, ws) = geom
    rng = np.random.default_rng(40)
    dst, src = _gpu(*_scene(rng, 9, h1, w1)), _gpu(*_scene(rng, 40, hs, ws))
    for lazy in (False, True):
        a = self_copy_paste_all(*dst, *src, lazy_masks=lazy)
        b = self_copy_paste(*dst, *src, np.arange(40), lazy_masks=lazy)
        assert sorted(a) == sorted(b)
        for k in a:
            assert torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
    ref = MR.paste_all(*[t.cpu().numpy() for t in dst], *[t.cpu().numpy() for t in src])
    _assert_equal(a, ref)


def test_paste_all_of_130_on_70_at_a_frame_that_takes_full_groups():
    """At 2048 x 2048 the chunks alone fill the grid, so the planes go in full groups: 130 source planes are two groups of at most
    SC_MAX_M = 99, 70 destination objects two groups of at most SC_MAX_OPG = 64.  Compared with the merged entry (sel = 0 .. 129, bound
    4 x 99) and with the same step written in torch."""
    from divergen_amd.layers import self_copy_paste, self_copy_paste_all
    size, ns, n0 = 2048, 130, 70
    g = torch.Generator(device="cuda").manual_seed(130)
    dst_img = torch.randint(0, 256, (3, size, size), dtype=torch.uint8, device="cuda", generator=g)
    src_img = torch.randint(0, 256, (3, size, size), dtype=torch.uint8, device="cuda", generator=g)
    rects = [(100, 100, 500, 400), (1000, 0, 1100, 2048), (320, 1420, 332, 1432)]      # (x0, y0, x1, y1); the third lies under a source object
    rng = np.random.default_rng(70)
    for _ in range(n0 - 3):
        x0, y0 = int(rng.integers(0, size - 200)), int(rng.integers(0, size - 200))
        rects.append((x0, y0, x0 + int(rng.integers(5, 200)), y0 + int(rng.integers(5, 200))))
    dst_m = torch.zeros(n0, size, size, dtype=torch.uint8, device="cuda")
    for i, (x0, y0, x1, y1) in enumerate(rects):
        dst_m[i, y0:y1, x0:x1] = 1
    dst_b = torch.tensor(rects, dtype=torch.float32, device="cuda")
    src_m = torch.zeros(ns, size, size, dtype=torch.uint8, device="cuda")
    boxes = []
    for j in range(ns):
        x0, y0 = (j % 13) * 150 + 7, (j // 13) * 200 + 3
        src_m[j, y0:y0 + 90, x0:x0 + 120] = 1
        boxes.append([x0, y0, x0 + 120, y0 + 90])
    src_b = torch.tensor(boxes, dtype=torch.float32, device="cuda")
    labels = torch.arange(n0, dtype=torch.int64, device="cuda")
    src_l = torch.arange(ns, dtype=torch.int64, device="cuda") + 500
    a = self_copy_paste_all(dst_img, dst_m, dst_b, labels, src_img, src_m, src_b, src_l, lazy_masks=True)
    b = self_copy_paste(dst_img, dst_m, dst_b, labels, src_img, src_m, src_b, src_l, np.arange(ns), lazy_masks=True, merged=True)
    for k in b:
        assert torch.equal(a[k], b[k]), k
    union = src_m.bool().any(0)                        # (any() of a uint8 tensor is uint8: its ~ would not be a logical not)
    upd = dst_m * (~union).to(torch.uint8)[None]
    assert torch.equal(a["image"], torch.where(union[None], src_img, dst_img))
    assert torch.equal(a["masks"][n0:], src_m) and torch.equal(a["masks"][:n0], upd)
    nb = torch.zeros(n0, 4, device="cuda")
    for i in range(n0):
        ys, xs = upd[i].any(1).nonzero().flatten(), upd[i].any(0).nonzero().flatten()
        if len(ys):
            nb[i] = torch.stack([xs[0], ys[0], xs[-1] + 1, ys[-1] + 1]).float()
    valid = ((nb - dst_b).abs() <= 10).all(1) | (upd.flatten(1).sum(1, dtype=torch.int64) > 300)
    assert not bool(valid[2]) and bool(valid[0]) and bool(valid[1]) and 0 < int(valid.sum()) < n0
    assert torch.equal(a["keep"], torch.cat([valid.nonzero().flatten(), n0 + torch.arange(ns, device="cuda")]))
    assert torch.equal(a["boxes"], torch.cat([nb[valid], src_b])) and torch.equal(a["labels"], torch.cat([labels[valid], src_l]))


def _raw_paste_args(n0, ns, h, w):
    dst = [torch.zeros(3, h, w, dtype=torch.uint8, device="cuda"), torch.zeros(max(n0, 1), h, w, dtype=torch.uint8, device="cuda"),
           torch.zeros(max(n0, 1), 4, device="cuda")]
    src = [torch.zeros(3, h, w, dtype=torch.uint8, device="cuda"), torch.zeros(max(ns, 1), h, w, dtype=torch.uint8, device="cuda")]
    outs = [torch.full((3, h, w), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((n0 + ns, h, w), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((max(n0, 1), 4), -7.0, device="cuda"), torch.full((max(n0, 1),), 0xA5, dtype=torch.uint8, device="cuda")]
    work = torch.empty(((n0 * 5 + 3) & ~3) + h * ((w + 15) // 16) * 4, dtype=torch.int32, device="cuda")
    return dst, src, outs, work


def test_paste_all_argument_errors_and_the_bound_of_the_selected_entry():
    from divergen_amd import _lib as L
    from divergen_amd.layers import self_copy_paste, self_copy_paste_all
    lib, s = L.lib(), L.stream()
    h, w, n0, ns = 16, 32, 2, 120
    dst, src, outs, work = _raw_paste_args(n0, ns, h, w)
    p = lambda t: t.data_ptr()      # noqa: E731
    d, sc, o = [p(t) for t in dst], [p(t) for t in src], [p(t) for t in outs]

    def call_all(n0=n0, h1=h, w1=w, ns=ns, hs=h, ws=w, H=h, W=w, src_masks=sc[1], out_image=o[0], work_p=p(work)):
        return lib.dgx_self_copy_paste_all(d[0], d[1], d[2], n0, h1, w1, sc[0], src_masks, ns, hs, ws, H, W, out_image, o[1], o[2], o[3], work_p, s)
    assert call_all(H=h - 1) == BAD_ARG and call_all(W=w - 1) == BAD_ARG and call_all(ns=-1) == BAD_ARG and call_all(n0=-1) == BAD_ARG
    assert call_all(src_masks=None) == BAD_ARG and call_all(out_image=None) == BAD_ARG and call_all(hs=0) == BAD_ARG
    assert call_all(work_p=p(work) + 4) == BAD_ARG                       # a misaligned workspace
    assert call_all(H=65536, W=32768) == UNSUPPORTED                     # H * W == 2^31
    assert call_all(ns=99 * 65535 + 1) == UNSUPPORTED                    # more plane groups than grid.y holds
    assert call_all(n0=2 ** 31 - 1, ns=1) == UNSUPPORTED                 # n0 + ns == 2^31
    # dgx_self_copy_paste keeps its bound: m = 100 is refused there, and NULL sel stays an error
    sel = torch.arange(100, dtype=torch.int32, device="cuda")
    sel_args = lambda sp, m: (d[0], d[1], d[2], n0, h, w, sc[0], sc[1], ns, h, w, sp, m, h, w, o[0], o[1], o[2], o[3], p(work), s)      # noqa: E731
    assert lib.dgx_self_copy_paste(*sel_args(p(sel), 100)) == BAD_ARG
    assert lib.dgx_self_copy_paste(*sel_args(None, 5)) == BAD_ARG and lib.dgx_self_copy_paste_merged(*sel_args(None, 5)) == BAD_ARG
    torch.cuda.synchronize()
    assert all(bool((t == (0xA5 if t.dtype == torch.uint8 else -7.0)).all()) for t in outs)      # nothing was launched
    assert call_all() == 0                                               # and the same arguments, in range, run
    torch.cuda.synchronize()
    assert not bool(outs[0].any()) and not bool(outs[1].any())
    src5 = _gpu(np.zeros((3, h, w), np.uint8), np.zeros((5, h, w), np.uint8), np.zeros((5, 4), np.float32), np.zeros(5, np.int64))
    dst4 = [dst[0], dst[1][:n0], dst[2][:n0], torch.zeros(n0, dtype=torch.int64, device="cuda")]
    with pytest.raises(ValueError):                                      # the layer above it too
        self_copy_paste(*dst4, src[0], src[1], torch.zeros(ns, 4, device="cuda"), torch.zeros(ns, dtype=torch.int64, device="cuda"), list(range(100)))
    with pytest.raises(ValueError):
        self_copy_paste_all(*dst4, src5[0], src5[1], src5[2][:4], src5[3])
    with pytest.raises(L.DgxError):                                      # no CPU fallback
        self_copy_paste_all(*[t.cpu() for t in dst4], *[t.cpu() for t in src5])


def test_loader_with_workers_in_domain_rm_bg_both(tmp_path, monkeypatch):
    """The real loader, 2 worker processes, INPUT.SCP_SRC_MODES with SCP_TYPE 'in_domain' (a source of the destination's own classes,
    pasted whole), RM_BG_PROB 0.5 and USE_COPY_METHOD 'both': every sample equals the single-process recomputation -- the worker half
    inline with the workers' seeds, background removal by the numpy restatement, the pool compositor, then the restatement of the paste."""
    from divergen_amd.data import build as B
    from divergen_amd.data.copypaste import InstPool
    from divergen_amd.data.samplers import RepeatFactorTrainingSampler
    from tests.test_gpu_loader import _mini_cfg
    cfg, info = _mini_cfg(tmp_path, 128, 2, ["INPUT.USE_COPY_METHOD", "both", "INPUT.SCP_SRC_MODES", True, "INPUT.SCP_TYPE", "in_domain",
                                             "INPUT.RM_BG_PROB", 0.5])
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    seed, per_gpu, nb, nw = 3, 2, 4, 2
    it = B.build_detection_train_loader(cfg, per_gpu, "cuda", seed)
    got = [next(it) for _ in range(nb)]
    torch.cuda.synchronize()
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
    plain = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    plain.set_dataset(dicts)
    plain.pack = False
    assert plain.paste_all and plain.scp_type == "in_domain" and plain.rm_bg_prob == 0.5
    rf = RepeatFactorTrainingSampler.repeat_factors_from_category_frequency(dicts, cfg.DATALOADER.REPEAT_THRESHOLD)
    idx = list(itertools.islice(iter(RepeatFactorTrainingSampler(rf, seed=seed)), nb * per_gpu))
    n_rm = n_plain = pasted = 0
    for w in range(nw):
        wseed = (seed * 1009 + w) % (2 ** 31)
        np.random.seed(wseed)
        plain.inst_pool.seed(wseed)
        for b in range(w, nb, nw):
            for j in range(per_gpu):
                raw = plain(dicts[idx[b * per_gpu + j]])
                have = got[b][j]
                assert have["file_name"] == raw["file_name"] and have.get("scp_file_name") == raw.get("scp_file_name")
                assert "rm_bg" not in have and "scp_src" not in have and "paste_pack" not in have
                scp = raw.pop("scp_src", None)
                if raw.pop("rm_bg", False):
                    n_rm += 1
                    raw["image"] = torch.from_numpy(MR.remove_background(raw["image"].numpy(), raw["instances"].gt_masks.tensor.numpy()))
                else:
                    n_plain += 1
                mid = InstPool.composite(raw, torch.device("cuda"))
                mi = mid["instances"]
                hi = have["instances"]
                if scp is None:                                 # no source: the pool paste's Instances, instance_source included
                    assert sorted(hi.get_fields()) == ["gt_boxes", "gt_classes", "gt_masks", "instance_source"]
                    assert torch.equal(have["image"], mid["image"]) and torch.equal(hi.gt_masks.tensor, mi.gt_masks.tensor)
                    assert torch.equal(hi.gt_boxes.tensor, mi.gt_boxes.tensor) and torch.equal(hi.gt_classes, mi.gt_classes)
                    continue
                assert scp.get("all") is True and sorted(hi.get_fields()) == ["gt_boxes", "gt_classes", "gt_masks"]
                ref = MR.paste_all(mid["image"].cpu().numpy(), mi.gt_masks.tensor.cpu().numpy().astype(np.uint8), mi.gt_boxes.tensor.cpu().numpy(),
                                   mi.gt_classes.cpu().numpy(), scp["image"].numpy(), scp["masks"].numpy(), scp["boxes"].numpy(), scp["labels"].numpy())
                _assert_equal(dict(image=have["image"], masks=hi.gt_masks.tensor.view(torch.uint8), boxes=hi.gt_boxes.tensor, labels=hi.gt_classes), ref)
                assert (have["height"], have["width"]) == tuple(have["image"].shape[-2:]) == tuple(hi.image_size)
                pasted += int(scp["labels"].shape[0])
    assert n_rm > 0 and n_plain > 0 and n_rm + n_plain == nb * per_gpu          # the background is removed for some samples, not for all
    assert pasted > 0 and it.side is not None
