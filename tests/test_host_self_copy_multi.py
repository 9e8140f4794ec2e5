"""CPU: the host half of self copy-paste from several source images (INPUT.SCP_NUM_SRC > 1 with INPUT.SCP_MULTI_SRC).
(a) the numpy restatement of the fold (tests/_selfcopy_multi_ref.py) equals the reference's own CopyPaste.__call__ outputs
    (tests/golden/self_copy_multi.npz) for every array, the stage canvases and the validity of every plane included, and numpy draws the
    recorded m / sel from the recorded seed;
(b) INPUT.SCP_MULTI_SRC gates the refusal of INPUT.SCP_NUM_SRC != 1 both ways, up to the bound of the build;
(c) CopyPasteMapper with SCP_NUM_SRC 2 consumes np.random in the reference's order (mapper.py:873-936, custom_copypaste.py:275-297): all
    index draws, the sources through the same mapper in index order, [pool], then randint / choice per source; one blend-mode draw
    per _copy_paste that happens;
(d) pack_sample / unpack_sample with two source groups round-trip; a sample with one source packs to the bytes it always did.
All comparisons are exact equality."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _selfcopy_multi_ref as MR  # noqa: E402
import _selfcopy_ref as SR  # noqa: E402

CASES = ["s2_ragged", "s3_skip_mid", "tmp_crop", "drift", "drop_300_301", "dst_larger", "dst_smaller", "all_empty", "s4"]


def golden_case(z, c):
    """-> (getter, destination 4-tuple, the SELECTED objects of every source as 4-tuples, in order)"""
    g = lambda k: z["%s_%s" % (c, k)]      # noqa: E731
    sources = []
    for i in range(int(g("n_src"))):
        sel = g("src%d_sel" % i)
        sources.append((g("src%d_image" % i), g("src%d_masks" % i)[sel], g("src%d_boxes" % i)[sel], g("src%d_labels" % i)[sel]))
    return g, (g("dst_image"), g("dst_masks"), g("dst_boxes"), g("dst_labels")), sources


def test_restatement_equals_reference_golden():
    z = np.load(os.path.join(GOLD, "self_copy_multi.npz"))
    assert [str(c) for c in z["cases"]] == CASES
    n_stages = set()
    for c in CASES:
        g, dst, sources = golden_case(z, c)
        np.random.seed(int(g("seed")))                         # _select_object's draws, source after source
        for i in range(int(g("n_src"))):
            ns = len(g("src%d_masks" % i))
            m = np.random.randint(0, min(ns + 1, 100))
            sel = np.random.choice(ns, size=m, replace=False)
            assert m == int(g("src%d_m" % i)) and np.array_equal(sel, g("src%d_sel" % i)), (c, i)
        r = MR.self_copy_multi(*dst, sources)
        assert np.array_equal(r["image"], g("out_image")) and r["image"].dtype == np.uint8, c
        assert np.array_equal(r["masks"], g("out_masks")), c
        assert np.array_equal(r["boxes"], g("out_boxes")) and r["boxes"].dtype == np.float32, c
        assert np.array_equal(r["labels"], g("out_labels")), c
        assert tuple(r["image"].shape[-2:]) == tuple(g("out_hw")), c
        assert np.array_equal(r["valid"], g("dst_valid").astype(bool)), c
        acc = r["merge"]
        if acc is None:
            assert len(g("merge_valid")) == 0 and len(g("tmp_hw")) == 0
        else:
            assert np.array_equal(acc["valid"], g("merge_valid").astype(bool)), c
            assert [tuple(x) for x in acc["hw"]] == [tuple(x) for x in g("tmp_hw").tolist()], c
        n_stages.add(len(g("tmp_hw")))
    assert n_stages == {0, 1, 2, 3}
    # what the cases are there for, on the reference's numbers
    assert z["s3_skip_mid_src1_m"] == 0 and z["drift_merge_valid"].tolist() == [1, 1, 1]
    assert z["drop_300_301_merge_valid"].sum() == 3 and (z["tmp_crop_tmp_hw"][0] < z["tmp_crop_out_hw"]).all()


def test_one_source_left_is_the_single_paste():
    """Exactly one source selects something: no temporary stage, the result is _selfcopy_ref.self_copy with that source."""
    z = np.load(os.path.join(GOLD, "self_copy_multi.npz"))
    _, dst, sources = golden_case(z, "s2_ragged")
    empty = (sources[1][0], sources[1][1][:0], sources[1][2][:0], sources[1][3][:0])
    r = MR.self_copy_multi(*dst, [empty, sources[0], empty])
    one = SR.self_copy(*dst, *sources[0], np.arange(len(sources[0][2])))
    for k in ("image", "masks", "boxes", "labels", "valid"):
        assert np.array_equal(r[k], one[k]), k


def _cfg(tmp_path, method, extra=()):
    from tests.test_gpu_loader import _mini_cfg
    return _mini_cfg(tmp_path, 128, 0, ["INPUT.USE_COPY_METHOD", method] + list(extra))


def _mapper(cfg, info, monkeypatch, seed=None):
    from divergen_amd.data import build as B
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])
    dicts = B.get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
    mapper = B.CopyPasteMapper(B.DatasetMapper(cfg, True), cfg)
    mapper.set_dataset(dicts)
    mapper.pack = False
    if seed is not None and mapper.inst_pool is not None:
        mapper.inst_pool.seed(seed)
    return mapper, dicts


def test_key_gates_the_refusal_both_ways(tmp_path, monkeypatch):
    from divergen_amd.config import get_cfg
    from divergen_amd.data import build as B
    from divergen_amd.layers.copy_paste import SELF_COPY_MAX_SRC
    assert get_cfg().INPUT.SCP_MULTI_SRC is False and SELF_COPY_MAX_SRC == 4
    cfg, info = _cfg(tmp_path, "syn_copy")
    monkeypatch.setenv("DETECTRON2_DATASETS", info["root"])

    def build(method, *opts):
        c = cfg.clone()
        c.defrost()
        c.merge_from_list(["INPUT.USE_COPY_METHOD", method] + list(opts))
        return B.CopyPasteMapper(B.DatasetMapper(c, True), c)
    for method in ("self_copy", "both", "p:0.25"):
        for n in (0, 2, 3, 4, 5):                               # key off: refused as it always was, same words
            with pytest.raises(NotImplementedError, match="SCP_NUM_SRC .* only 1 \\(several sources are merged on a temporary canvas first\\)"):
                build(method, "INPUT.SCP_NUM_SRC", n)
        for n in (1, 2, 3, 4):                                  # key on: admitted up to the bound
            assert build(method, "INPUT.SCP_NUM_SRC", n, "INPUT.SCP_MULTI_SRC", True).num_src == n
        for n in (0, 5, 9):
            with pytest.raises(NotImplementedError, match="SCP_NUM_SRC"):
                build(method, "INPUT.SCP_NUM_SRC", n, "INPUT.SCP_MULTI_SRC", True)
        with pytest.raises(NotImplementedError, match="ROTATE_SRC"):      # every other refusal is unchanged by the key
            build(method, "INPUT.SCP_NUM_SRC", 2, "INPUT.SCP_MULTI_SRC", True, "INPUT.ROTATE_SRC", True)
        with pytest.raises(NotImplementedError, match="BLANK_RATIO"):
            build(method, "INPUT.SCP_MULTI_SRC", True, "INPUT.BLANK_RATIO", 0.3)
    assert build("syn_copy", "INPUT.SCP_NUM_SRC", 7, "INPUT.SCP_MULTI_SRC", True).self_prob is None      # not a self-copy method


class _CountingPool:
    """Stands in front of the mapper's InstPool: counts the blend-mode draws."""

    def __init__(self, pool):
        self.pool, self.drawn = pool, []

    def __getattr__(self, name):
        return getattr(self.pool, name)

    def draw_modes(self, K):
        self.drawn.append(K)
        return self.pool.draw_modes(K)


@pytest.mark.parametrize("method", ["self_copy", "both", "p:0.5"])
def test_mapper_consumes_np_random_in_reference_order_with_two_sources(tmp_path, monkeypatch, method):
    extra = ["INPUT.SCP_NUM_SRC", 2, "INPUT.SCP_MULTI_SRC", True]
    cfg, info = _cfg(tmp_path, method, extra)
    mapper, dicts = _mapper(cfg, info, monkeypatch, seed=1)
    hand, _ = _mapper(cfg, info, monkeypatch, seed=1)          # its DatasetMapper / InstPool, driven by hand below
    if mapper.inst_pool is not None:
        mapper.inst_pool = _CountingPool(mapper.inst_pool)
    groups = {0: 0, 1: 0, 2: 0}
    for k in range(14):
        d = dicts[k % len(dicts)]
        np.random.seed(300 + k)
        got = mapper(d)
        after_got = np.random.rand()
        # ---- the reference's order, by hand
        np.random.seed(300 + k)
        dst = hand.mapper(d)
        idxs = [np.random.randint(0, len(dicts)) for _ in range(2)]
        self_branch = True
        if method.startswith("p:"):
            self_branch = np.random.rand() < 0.5
        srcs = [hand.mapper(dicts[i]) for i in idxs] if self_branch else []
        if method == "both" or not self_branch:
            dst = hand.inst_pool.prepare(dst)
        picked = []
        for src in srcs:
            ns = len(src["instances"])
            m = np.random.randint(0, min(ns + 1, 100))
            sel = np.random.choice(ns, size=m, replace=False)
            if m:
                picked.append((src, torch.from_numpy(sel)))
        assert after_got == np.random.rand(), (method, k)
        # ---- and what the mapper hands over
        assert torch.equal(got["image"], dst["image"]) and ("paste_pack" in got) == ("paste_pack" in dst)
        assert ("scp_src" in got) == self_branch
        if not self_branch:
            continue
        assert got["scp_file_name"] == [s["file_name"] for s in srcs]
        groups[len(picked)] += 1
        if mapper.inst_pool is not None:                        # one draw per _copy_paste: the temporary stages and the final paste
            assert sum(mapper.inst_pool.drawn) == len(picked)
            mapper.inst_pool.drawn.clear()
        h1, w1 = dst["image"].shape[-2:]
        if len(picked) == 2:
            assert isinstance(got["scp_src"], list) and len(got["scp_src"]) == 2
            boxes = torch.cat([s["instances"].gt_boxes.tensor[st] for s, st in picked]).numpy()
            H, W = SR.canvas_hw((0, 0), boxes)                  # no canvas reaches beyond the largest box extent of all sources
            for grp, (src, st) in zip(got["scp_src"], picked):
                si = src["instances"]
                assert sorted(grp) == ["boxes", "image", "labels", "masks"]
                assert torch.equal(grp["boxes"], si.gt_boxes.tensor[st]) and torch.equal(grp["labels"], si.gt_classes[st])
                assert torch.equal(grp["masks"], si.gt_masks.tensor.view(torch.uint8)[st][:, :H, :W])
                assert torch.equal(grp["image"], src["image"][:, :H, :W])
        elif len(picked) == 1:                                  # one source left: the dict a single source always gave
            src, st = picked[0]
            s = got["scp_src"]
            H, W = SR.canvas_hw((h1, w1), src["instances"].gt_boxes.tensor[st].numpy())
            assert isinstance(s, dict) and tuple(s["hw"]) == (H, W) and torch.equal(s["boxes"], src["instances"].gt_boxes.tensor[st])
            assert torch.equal(s["image"], src["image"][:, :H, :W])
        else:
            assert isinstance(got["scp_src"], dict) and tuple(got["scp_src"]["hw"]) == (h1, w1) and got["scp_src"]["masks"].shape[0] == 0
    assert groups[2] > 0


def test_worker_draws_reproduce_the_golden_selections():
    """The worker's draw order for two sources, fed the golden's seed and object counts, selects what the reference's
    _select_object selected (the draws sit in CopyPasteMapper._call_self_copy: randint, choice per source, in order)."""
    from divergen_amd.data import build as B
    from divergen_amd.structures import BitMasks, Boxes, Instances
    z = np.load(os.path.join(GOLD, "self_copy_multi.npz"))
    for c in ("s2_ragged", "tmp_crop", "drop_300_301", "all_empty"):
        g = lambda k: z["%s_%s" % (c, k)]      # noqa: E731

        def inst(p):
            h, w = g(p + "_image").shape[-2:]
            return {"image": torch.from_numpy(g(p + "_image")), "file_name": p,
                    "instances": Instances((h, w), gt_boxes=Boxes(torch.from_numpy(g(p + "_boxes"))), gt_classes=torch.from_numpy(g(p + "_labels")),
                                           gt_masks=BitMasks(torch.from_numpy(g(p + "_masks").astype(bool))))}
        samples = {"src0": inst("src0"), "src1": inst("src1")}
        mapper = B.CopyPasteMapper.__new__(B.CopyPasteMapper)
        mapper.method, mapper.self_prob, mapper.inst_pool, mapper.pack = "self_copy", 1.0, None, False
        mapper.dataset, mapper.mapper = ["src0", "src1"], lambda name: samples[name]
        np.random.seed(int(g("seed")))
        got = mapper._call_self_copy(inst("dst"), [0, 1])["scp_src"]
        taken = [i for i in range(2) if int(g("src%d_m" % i))]
        if len(taken) == 2:
            for grp, i in zip(got, taken):
                sel = g("src%d_sel" % i)
                assert np.array_equal(grp["labels"].numpy(), g("src%d_labels" % i)[sel]) and np.array_equal(grp["boxes"].numpy(), g("src%d_boxes" % i)[sel])
        else:
            assert taken == [] and got["masks"].shape[0] == 0


def _two_group_sample(tmp_path, monkeypatch, method="both"):
    cfg, info = _cfg(tmp_path, method, ["INPUT.SCP_NUM_SRC", 2, "INPUT.SCP_MULTI_SRC", True])
    mapper, dicts = _mapper(cfg, info, monkeypatch, seed=3)
    for k in range(40):
        np.random.seed(500 + k)
        raw = mapper(dicts[k % len(dicts)])
        if isinstance(raw.get("scp_src"), list):
            return raw
    raise AssertionError("no sample with two source groups")


def test_blob_round_trip_with_two_source_groups(tmp_path, monkeypatch):
    from divergen_amd.data import build as B
    raw = _two_group_sample(tmp_path, monkeypatch)
    packed = B.pack_sample(dict(raw))
    names = [x[0] for x in packed["blob_layout"]]
    assert names == ["image", "gt_masks", "gt_boxes", "gt_classes", "flat", "desc", "labels",
                     "scp0_image", "scp0_masks", "scp0_boxes", "scp0_labels", "scp1_image", "scp1_masks", "scp1_boxes", "scp1_labels"]
    assert all(x[3] % 64 == 0 for x in packed["blob_layout"]) and "scp_src" not in packed and packed["blob_scp_n"] == 2
    assert "blob_scp_hw" not in packed
    back = B.unpack_sample(packed, torch.device("cpu"))
    assert torch.equal(back["image"], raw["image"]) and torch.equal(back["instances"].gt_masks.tensor, raw["instances"].gt_masks.tensor)
    assert isinstance(back["scp_src"], list) and len(back["scp_src"]) == 2 and back["scp_file_name"] == raw["scp_file_name"]
    for b, r in zip(back["scp_src"], raw["scp_src"]):
        for key in ("image", "masks", "boxes", "labels"):
            assert torch.equal(b[key], r[key]) and b[key].dtype == r[key].dtype


def test_one_source_blob_is_unchanged_by_the_key(tmp_path, monkeypatch):
    """SCP_NUM_SRC 1: the same sample, packed with and without INPUT.SCP_MULTI_SRC, is the same bytes, layout and keys -- and they
    are the eleven sections a self-copy sample always had."""
    from divergen_amd.data import build as B
    packed = []
    for sub, extra in (("off", []), ("on", ["INPUT.SCP_MULTI_SRC", True])):
        cfg, info = _cfg(tmp_path / sub, "both", extra)
        mapper, dicts = _mapper(cfg, info, monkeypatch, seed=3)
        np.random.seed(12)
        raws = [mapper(dicts[k]) for k in range(4)]
        assert all(isinstance(r["scp_src"], dict) and isinstance(r["scp_file_name"], str) for r in raws)
        packed.append([B.pack_sample(dict(r)) for r in raws])
    for a, b in zip(*packed):
        assert a["blob_layout"] == b["blob_layout"] and torch.equal(a["blob"], b["blob"]) and set(a) == set(b)
        assert [x[0] for x in a["blob_layout"]] == ["image", "gt_masks", "gt_boxes", "gt_classes", "flat", "desc", "labels",
                                                    "scp_image", "scp_masks", "scp_boxes", "scp_labels"]
        assert a["blob_scp_hw"] == b["blob_scp_hw"] and "blob_scp_n" not in a


def test_finish_refuses_several_sources_without_the_gpu(tmp_path, monkeypatch):
    """No quiet fall-back for the merge either."""
    from divergen_amd.data import build as B
    raw = _two_group_sample(tmp_path, monkeypatch, "self_copy")
    mapper = B.CopyPasteMapper.__new__(B.CopyPasteMapper)
    mapper.ring, mapper.active_select = None, False
    with pytest.raises(RuntimeError, match="dgx_self_copy_paste"):
        mapper.finish(raw, "cpu")
