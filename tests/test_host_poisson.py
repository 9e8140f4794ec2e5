"""CPU: the opt-in 'possion' blend of INPUT.CP_METHOD (INPUT.CP_POISSON).
(a) tests/_poisson_ref.py (the reduced system the GPU tests check the kernel against) follows the reference's own poisson_edit
    (tests/golden/poisson_blend.npz, make_golden_poisson.py) after every paste: every byte within 1, and exactly as many differing
    bytes as the generator counted -- the reference's sparse LU is not reproducible to the byte (T - eps on identity rows, then
    truncation), so the pin is on the count, not on the reference's rounding noise;
(b) without CP_POISSON 'possion' is refused as before; with it InstPool accepts it, draws the reference's mode sequence from its own
    generator, leaves np.random and the global `random` alone, and mode byte 3 survives the worker -> ring -> training hand-over;
(c) host_modes(..., allow_poisson=True).
The GPU twin is tests/test_gpu_poisson.py."""
import os
import random

import numpy as np
import pytest
import torch

import _blend_ref as BR
import _poisson_ref as PR
import test_host_blend_modes as HB

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASES = ("possion", "mixed4")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLD, "poisson_blend.npz"))


def golden_pastes(z):
    return [(z["src%d_rgba" % k], int(z["src%d_xy" % k][0]), int(z["src%d_xy" % k][1]), int(z["src%d_label" % k][0]))
            for k in range(int(z["K"]))]


@pytest.mark.parametrize("case", CASES)
def test_restatement_follows_reference_per_step(z, case):
    from oracle import compositor as OK
    pastes = golden_pastes(z)
    modes = z["%s_modes" % case].tolist()
    steps = z["%s_steps" % case]
    H, W = (int(v) for v in z["hw"])
    differing = 0
    for k, ((rgba, x0, y0, _), mode) in enumerate(zip(pastes, modes)):
        before = z["dst_image"] if k == 0 else steps[k - 1]          # the reference's own previous image: nothing compounds
        placed, m = OK.place(rgba, x0, y0, H, W)
        if mode == 3:
            mine, x, U = PR.solve(before, placed[:3], m[0])
            d = np.abs(mine.astype(np.int64) - steps[k].astype(np.int64))
            assert d.max() <= 1, "%s: step %d differs by %d" % (case, k, d.max())
            differing += int((d != 0).sum())
            assert np.array_equal(x[:, ~U], before[:, ~U].astype(np.float64))
        else:
            assert np.array_equal(BR.blend(before, placed[:3], placed[3], mode), steps[k]), "%s: step %d (mode %d)" % (case, k, mode)
    assert differing == int(z["%s_ref_vs_restated_mismatches" % case])
    ref = OK.composite(z["dst_image"], z["dst_masks"], z["dst_boxes"], z["dst_labels"], pastes)
    assert np.array_equal(ref["masks"], z["%s_out_masks" % case]) and np.array_equal(ref["boxes"], z["%s_out_boxes" % case])
    assert np.array_equal(ref["labels"], z["%s_out_labels" % case]) and np.array_equal(ref["source"], z["%s_out_source" % case])


def test_golden_draws_every_mode_and_shows_the_frame_quirk(z):
    from oracle import compositor as OK
    assert set(z["mixed4_modes"].tolist()) == {0, 1, 2, 3} and set(z["possion_modes"].tolist()) == {3}
    H, W = (int(v) for v in z["hw"])
    rgba, x0, y0, _ = golden_pastes(z)[0]                             # an interior paste: its footprint does not touch the frame
    _, m = OK.place(rgba, x0, y0, H, W)
    frame = PR.unknowns(np.zeros((H, W), bool))
    assert not (frame & (m[0] > 0)).any()
    changed = z["possion_steps"][0] != z["dst_image"]
    assert changed[:, frame].sum() > 0.9 * 3 * frame.sum()            # the reference rewrites nearly every frame byte
    inner = ~frame & (m[0] == 0)
    # interior pixels outside F: identity rows.  The reference's LU may return T - eps there (then truncates): at most 1 off
    assert np.abs(z["possion_steps"][0].astype(int) - z["dst_image"].astype(int))[:, inner].max() <= 1


def test_restatement_band_is_thin_on_the_golden(z):
    """The property the GPU test relies on: about 2 * DELTA of the bytes of U are undecided by DELTA, far below its 1 % cap."""
    steps, sols = PR.blend_chain(z["dst_image"], golden_pastes(z), z["possion_modes"])
    for (x, U) in sols:
        assert PR.band(x, U).sum() <= 0.01 * 3 * U.sum()


# ---------------------------------------------------------------- (b) the key, the draws, the hand-over
def test_possion_needs_the_key():
    from divergen_amd.data.copypaste import InstPool, check_cp_method
    with pytest.raises(NotImplementedError, match="possion") as e:
        InstPool({"0": ["x.png"]}, 64, cp_method=["basic", "possion"])
    assert "solve" in str(e.value)
    with pytest.raises(NotImplementedError):
        check_cp_method(["possion"])
    assert check_cp_method(["basic", "possion"], allow_poisson=True) == ["basic", "possion"]
    ip = InstPool({"0": ["x.png"]}, 64, cp_method=["possion"], allow_poisson=True)
    assert ip.cp_method == ["possion"] and ip.allow_poisson
    for bad in (["poisson"], ["possion", "soft"]):                    # the usual spelling is not the reference's name
        with pytest.raises(NotImplementedError):
            InstPool({"0": ["x.png"]}, 64, cp_method=bad, allow_poisson=True)


def test_from_config_reads_cp_poisson(tmp_path):
    from divergen_amd.config import get_cfg
    from divergen_amd.data.copypaste import InstPool
    pool_json = tmp_path / "pool.json"
    pool_json.write_text('{"3": ["a.png"]}')
    cfg = get_cfg()
    assert cfg.INPUT.CP_POISSON is False
    cfg.merge_from_list(["INPUT.INST_POOL_PATH", str(pool_json), "MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH", "",
                         "INPUT.CP_METHOD", ["gaussian", "possion"]])
    with pytest.raises(NotImplementedError, match="possion"):
        InstPool.from_config(cfg)
    cfg.merge_from_list(["INPUT.CP_POISSON", True])
    ip = InstPool.from_config(cfg)
    assert ip.cp_method == ["gaussian", "possion"] and ip.allow_poisson
    cfg.merge_from_list(["INPUT.CP_METHOD", ["poisson"]])
    with pytest.raises(NotImplementedError, match="poisson"):
        InstPool.from_config(cfg)


@pytest.mark.parametrize("case", CASES)
def test_prepare_draws_the_reference_sequence(z, case):
    from divergen_amd.data.build import _worker_init
    methods = [str(m) for m in z["%s_methods" % case]]
    from divergen_amd.data.copypaste import InstPool
    zd = np.load(os.path.join(GOLD, "pool_draws.npz"))
    keys = [str(k) for k in np.load(os.path.join(GOLD, "pool_decode.npz"))["keys"]]
    pool = {}
    for k, c in zip(keys, zd["pool_cats"].tolist()):
        pool.setdefault(str(c), []).append(k)
    ip = InstPool(pool, tuple(int(v) for v in zd["hw"]), max_samples=int(zd["max_samples"]), random_scale=False,
                  random_scale_min=0.5, random_scale_max=2.0, random_scale_min_size=5, use_largest_part=False, cp_method=methods,
                  allow_poisson=True)
    ip.HWms = {str(k): [float(a), float(b)] for k, (a, b) in zip(zd["HWms_keys"], zd["HWms_vals"])}
    seed = int(z["%s_seed" % case])
    _worker_init(seed, 0, in_worker=False, pool=ip)
    got = []
    state = random.getstate()
    cwd = os.getcwd()
    os.chdir(GOLD)
    try:
        for ci in HB.pool_cases(zd):
            np.random.seed(int(zd["c%d_seed" % ci]))
            d = ip.prepare(HB.sample_of(zd, ci))
            assert np.random.randint(0, 2 ** 31 - 1) == int(zd["c%d_after" % ci]), "the mode draws moved np.random (case %d)" % ci
            pk = d["paste_pack"]
            assert isinstance(pk["modes"], np.ndarray) and pk["modes"].dtype == np.uint8 and pk["modes"].shape == (pk["K"],)
            got += pk["modes"].tolist()
            if len(got) >= int(z["seq_draws"]):
                break
    finally:
        os.chdir(cwd)
    assert random.getstate() == state, "InstPool drew from the process's global random"
    n = min(len(got), int(z["seq_draws"]))
    assert n >= 12 and got[:n] == z["%s_seq" % case][:n].tolist()
    assert got[:int(z["K"])] == z["%s_modes" % case].tolist()[:len(got)]        # the golden's own paste sequence
    assert 3 in got


def test_mode_3_survives_pack_ring_unpack():
    """pack_sample -> _RingCollate (slot write) -> unpack_sample: the modes arrive as the host uint8 array with its 3s, and the
    descriptors of such a sample arrive once more in host memory (the solver's workspace is sized from them without a read-back)."""
    from divergen_amd.data.build import _RingCollate, unpack_sample
    modes = np.array([0, 3, 1, 3, 2], np.uint8)
    packed = HB._packed(modes)
    assert isinstance(packed["blob_modes"], np.ndarray) and packed["blob_modes"].tolist() == modes.tolist()
    assert isinstance(packed["blob_desc"], np.ndarray) and packed["blob_desc"].dtype == np.int32 and packed["blob_desc"].shape == (5, 5)
    assert not any(torch.is_tensor(v) for k, v in packed.items() if k != "blob")
    assert "blob_desc" not in HB._packed(np.array([0, 2, 1, 0, 0], np.uint8))     # modes 0-2 cross exactly as before
    ring = HB._FakeRing(1, 2, 4096)
    (d,) = _RingCollate(ring)([packed])
    if d.get("blob_slot") is not None:
        off, n = d["blob_slot"]
        d = dict(d, blob=ring.buf[off:off + n].clone(), blob_slot=None)
    out = unpack_sample(d, "cpu")
    pk = out["paste_pack"]
    assert pk["modes"].dtype == np.uint8 and pk["modes"].tolist() == modes.tolist()
    assert np.array_equal(pk["desc_host"], pk["desc"].numpy()) and pk["K"] == 5


# ---------------------------------------------------------------- (c) host_modes
def test_host_modes_forms_with_poisson():
    from divergen_amd.layers.copy_paste import BLEND_MODES, BLEND_MODES_ALL, host_modes
    assert BLEND_MODES == {"basic": 0, "alpha": 1, "gaussian": 2} and BLEND_MODES_ALL == {**BLEND_MODES, "possion": 3}
    assert host_modes(["basic", "possion", "gaussian"], 3, allow_poisson=True).tolist() == [0, 3, 2]
    assert host_modes([3, 0], 2, allow_poisson=True).tolist() == [3, 0]
    assert host_modes(np.array([3, 3], np.uint8), 2, allow_poisson=True).tolist() == [3, 3]
    assert host_modes(["possion", 1, 3, "basic"], 4, allow_poisson=True).tolist() == [3, 1, 3, 0]
    assert host_modes(["basic", 0], 2, allow_poisson=True) is None
    m = host_modes(torch.tensor([3], dtype=torch.uint8), 1, allow_poisson=True)
    assert m.dtype == np.uint8 and m.flags["C_CONTIGUOUS"]
    for bad in ([0, 4], ["poisson"], [-1]):
        with pytest.raises(ValueError):
            host_modes(bad, len(bad), allow_poisson=True)
    for bad in ([0, 3], ["basic", "possion"]):                        # the default call still rejects it
        with pytest.raises(ValueError):
            host_modes(bad, 2)


def test_poisson_unknowns_bound_and_report_check():
    from divergen_amd.layers.copy_paste import check_poisson_report, poisson_unknowns
    assert poisson_unknowns([0, 10, 12, 5, 6], 60, 80) == 2 * 60 + 2 * 80 - 4 + 120
    assert poisson_unknowns([0, 10, 12, -4, 55], 60, 80) == 276 + 5 * 8          # clipped to the image
    assert poisson_unknowns([0, 10, 12, 200, 0], 60, 80) == 276                  # wholly outside: the frame alone
    assert poisson_unknowns([0, 100, 100, -5, -5], 60, 80) == 60 * 80
    ok = np.array([[0, 0, 0, 0], [88, 1e-7, 1, 724]])
    assert check_poisson_report(ok, [0, 3]).shape == (2, 4)
    bad = np.array([[0, 0, 0, 0], [1, 35.0, 0, 724]])
    with pytest.raises(RuntimeError, match="paste 1"):
        check_poisson_report(bad, [0, 3])
    with pytest.raises(RuntimeError, match="paste 1"):
        check_poisson_report(torch.from_numpy(bad))
