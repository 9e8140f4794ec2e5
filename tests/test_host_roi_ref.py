"""CPU: the float64 restatements of tests/_roi_ref64.py and the plain-C++ geometry of divergen_amd/csrc/roi_tables.h, without a GPU:

* tests/native/roi_tables_check.cpp runs the real header code with bounds-checked host arrays sized as the launches size their LDS,
  once as an ordinary build and once under -fsanitize=address,undefined (a plain executable); what it prints -- level, grid, count,
  starts and bin sizes, spans and table weights -- equals the restatement's fp32 geometry bit for bit on every box of the tables, and
  the gather's hit lists contain every box that weighs a tile;
* the restatement agrees with the oracle's C ROIAlign (forward, backward, crop_and_resize), with tests/golden/refcpp.npz and with D2's
  known-answer values;
* fp32 evaluations of the contract in three summation orders stay inside every bound, and every mutant leaves one where it is defined;
* the form tables name what the header decides (vector / separable, nsplit, TH, slices);
* the level rule differs from the reference's fp32 log2 rule exactly on the boxes 1 - 2 ulps below a power of two."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _roi_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = list(R.BOXES) + list(R.LEVEL_BOXES)
# name -> (maps, min_level, scale0, aligned)
CONFIGS = {
    "multi": (R.LEVELS, R.MIN_LEVEL, R.SCALE0, 1),
    "single1": (R.LEVELS[:1], 0, R.SCALE0, 1),
    "single0": (R.LEVELS[:1], 0, R.SCALE0, 0),
    "small": ([R.SMALL], 0, R.SCALE0, 1),
}


def _hex(v):
    return "%08x" % int(np.asarray(v, f32).reshape(1).view(np.uint32)[0])


def _scales(cfg):
    maps, min_level, s0, _ = CONFIGS[cfg]
    return R.pooler_scales(len(maps), s0) if len(maps) > 1 else [s0]


def _maps_req(maps, min_level=None):
    head = "%d " % len(maps) + ("%d " % min_level if min_level is not None else "")
    return head + " ".join(str(h) for h, _ in maps) + " " + " ".join(str(w) for _, w in maps)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("roi_tables")
    src = os.path.join(ROOT, "tests", "native", "roi_tables_check.cpp")
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]
    exe, san = str(d / "roi_tables_check"), str(d / "roi_tables_check_san")
    subprocess.check_call(base + ["-O1", "-o", exe, src])
    # the sanitizer runtimes linked into the executable: it then runs the same wherever the suite runs, whatever else the process loads
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                                  "-o", san, src])

    def run(lines):
        p = str(d / "cases.txt")
        with open(p, "w") as f:
            f.write("\n".join(lines) + "\n")
        outs = []
        for e in (exe, san):
            o = subprocess.run([e, p], capture_output=True, text=True, timeout=600)
            got = o.stdout.strip().split("\n")
            assert o.returncode == 0 and got[-1].startswith("ok "), (e, o.stdout[-2000:], o.stderr[-2000:])
            assert int(got[-1].split()[1]) == len(lines)
            outs.append(got)
        assert outs[0] == outs[1], "the sanitizer build printed something else"
        return outs[0][:-1], int(outs[0][-1].split()[2])
    return run


def _roi_cases():
    for cfg, (maps, min_level, s0, aligned) in CONFIGS.items():
        for S in (7, 14):
            for sr in (0, 2):
                for nm in NAMES:
                    yield cfg, S, sr, nm


def test_header_geometry_equals_the_restatement_bit_for_bit(checker):
    cases = list(_roi_cases())
    lines = []
    for cfg, S, sr, nm in cases:
        maps, min_level, s0, aligned = CONFIGS[cfg]
        roi = R.rois_of([nm])[0]
        lines.append("roi %s %s %d %d %d %d %s" % (_maps_req(maps, min_level), _hex(s0), aligned, S, S, sr, " ".join(_hex(v) for v in roi)))
    got, checked = checker(lines)
    assert len(got) == len(cases) and checked > 100000
    descending = 0
    for (cfg, S, sr, nm), line in zip(cases, got):
        maps, min_level, s0, aligned = CONFIGS[cfg]
        t = R.roi_tables(R.rois_of([nm])[0], maps, _scales(cfg), min_level, S, S, sr, aligned)
        G = t.G
        want = ["roi", str(t.lvl), str(G.gh), str(G.gw), _hex(G.count), _hex(G.sw), _hex(G.sh), _hex(G.bin_w), _hex(G.bin_h)]
        for tag, T in (("Y", t.Y), ("X", t.X)):
            want.append(tag)
            for i in range(S):
                want += [str(int(T.base[i])), str(int(T.n[i]))] + [_hex(T.W32[i, T.base[i] + k]) for k in range(int(T.n[i]))]
        assert line.split() == want, (cfg, S, sr, nm)
        descending += int(sr > 0 and (G.bin_h < 0 or G.bin_w < 0) and bool(t.Y.n.any() or t.X.n.any()))
    assert descending >= 4          # the inverted box with a fixed grid went through the header's tables


def _gather_sets():
    named = R.cycled_rois(len(NAMES))
    return {
        "multi_c256": ("multi", 256, 7, named),
        "multi_c64_257": ("multi", 64, 7, R.cycled_rois(257)),
        "multi_c2048_s14": ("multi", 2048, 14, named),
        "single0_c256": ("single0", 256, 7, named),
        "small_c256": ("small", 256, 7, named),
    }


def test_gather_hit_lists_contain_every_box_that_weighs_a_tile(checker):
    sets, lines, keys = _gather_sets(), [], []
    for key, (cfg, C, S, rois) in sets.items():
        maps, min_level, s0, aligned = CONFIGS[cfg]
        for sr in (0, 2):
            lines.append("gather %s %s %d %d %d %d %d %d %d %s" % (_maps_req(maps, min_level), _hex(s0), aligned, R.N_IMG, C, S, S, sr, len(rois),
                                                                " ".join(_hex(v) for v in rois.reshape(-1))))
            keys.append((key, sr))
    got, _ = checker(lines)
    pos, inverted_hits = 0, 0
    for (key, sr) in keys:
        cfg, C, S, rois = sets[key]
        maps, min_level, s0, aligned = CONFIGS[cfg]
        tw, th = 256 // (C // 8), 4
        tabs = [R.roi_tables(r, maps, _scales(cfg), min_level, S, S, sr, aligned) for r in rois]
        ntiles = sum(R.N_IMG * -(-H // th) * -(-W // tw) for H, W in maps)
        for line in got[pos:pos + ntiles]:
            f = line.split()
            assert f[0] == "tile"
            l, n, y0, x0 = map(int, f[1:5])
            listed = {int(f[k]): (int(f[k + 1]), int(f[k + 2])) for k in range(5, len(f), 3)}
            for r, t in enumerate(tabs):
                if t.lvl != l or t.G.b != n:
                    assert r not in listed
                    continue
                rows = t.Y.W[:, y0:y0 + th].any(1)
                if rows.any() and t.X.W[:, x0:x0 + tw].any():
                    assert r in listed, (key, sr, line, r)
                    lo, hi = listed[r]
                    assert not rows[:lo].any() and not rows[hi:].any(), (key, sr, line, r)
                    inverted_hits += int(t.G.bin_h < 0)
        pos += ntiles
    assert pos == len(got) and inverted_hits > 0


def test_restatement_agrees_with_the_oracle_the_golden_file_and_the_known_answers():
    from oracle import roi as OR
    # D2's known-answer test (tests/layers/test_roi_align.py): 5 x 5 ramp, box (1, 1, 3, 3), 4 x 4 bins
    inp = np.arange(25, dtype=np.float64).reshape(1, 5, 5, 1)
    ref, A, n, _ = R.forward64([inp], np.array([[0, 1, 1, 3, 3]], f32), [1.0], 0, 4, 4, 0, True)
    assert np.array_equal(ref[0, :, :, 0], [[4.5, 5.0, 5.5, 6.0], [7.0, 7.5, 8.0, 8.5], [9.5, 10.0, 10.5, 11.0], [12.0, 12.5, 13.0, 13.5]])
    ref0, _, _, _ = R.forward64([inp], np.array([[0, 1, 1, 3, 3]], f32), [1.0], 0, 4, 4, 0, False)      # the old, unaligned op
    assert np.allclose(ref0[0, :, :, 0], np.array([[4.5, 5.0, 5.5, 6.0], [7.0, 7.5, 8.0, 8.5], [9.5, 10.0, 10.5, 11.0], [12.0, 12.5, 13.0, 13.5]]) + 3.0)

    g = np.random.default_rng(5)
    H, W = R.LEVELS[0]
    feat = g.standard_normal((R.N_IMG, H, W, 8)).astype(f32)
    rois = R.rois_of(NAMES)
    go = g.standard_normal((len(rois), 7, 7, 8)).astype(f32)
    tf = torch.from_numpy(feat).permute(0, 3, 1, 2).contiguous()
    for sr in (0, 2):
        for aligned in (True, False):
            ref, A, n, tabs = R.forward64([feat], rois, [R.SCALE0], 0, 7, 7, sr, aligned)
            o = OR.roi_align(tf, torch.from_numpy(rois), R.SCALE0, 7, sr, aligned).permute(0, 2, 3, 1).numpy()
            # the oracle sums 4 gh gw weighted taps per bin in fp32, each weight a product: its own error against float64
            n_or = np.array([4 * max(t.G.gh, 1) * max(t.G.gw, 1) + 4 for t in tabs], np.float64).reshape(-1, 1, 1, 1)
            assert R.worst_ratio(o, ref, R.f32_bound(ref, A, n_or)) <= 1.0, (sr, aligned)
            (gr, gA, gn), = R.scatter64(go, rois, [(H, W)], R.N_IMG, [R.SCALE0], 0, sr, aligned)[0]
            ob = OR.roi_align_backward(torch.from_numpy(go).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(rois), R.SCALE0,
                                       (R.N_IMG, 8, H, W), sr, aligned).permute(0, 2, 3, 1).numpy()
            assert R.worst_ratio(ob, gr, R.f32_bound(gr, gA, gn + 4 * 2 * 2)) <= 1.0, (sr, aligned)
    # the reference's own C++ on the inputs of tests/test_gpu_kernels.py (tests/golden/refcpp.npz)
    z = np.load(os.path.join(ROOT, "tests", "golden", "refcpp.npz"))
    tg = torch.Generator().manual_seed(31)
    feat = torch.rand(2, 64, 20, 16, generator=tg)
    xy = torch.rand(48, 2, generator=tg) * torch.tensor([16 * 4 * 0.7, 20 * 4 * 0.7])
    wh = torch.rand(48, 2, generator=tg) * torch.tensor([16 * 4 * 0.6, 20 * 4 * 0.6]) + 0.5
    b = torch.randint(0, 2, (48, 1), generator=tg).float()
    rois = torch.cat([b, xy, xy + wh], 1).numpy()
    go = torch.rand(48, 64, 7, 7, generator=tg)
    ref, A, n, tabs = R.forward64([feat.permute(0, 2, 3, 1).numpy()], rois, [0.25], 0, 7, 7, 0, True)
    # (the rotated op at angle 0 reaches its sample positions through a centre, a size and cos / sin: another fp32 sequence, so it is
    # held to the tolerances of the reference's own comparison of the two ops, D2 tests/modeling/test_roi_pooler.py: atol 1e-4)
    assert np.abs(z["roi_align_fwd_hip"].transpose(0, 2, 3, 1) - ref).max() <= 1e-4
    (gr, gA, gn), = R.scatter64(go.permute(0, 2, 3, 1).numpy(), rois, [(20, 16)], 2, [0.25], 0, 0, True)[0]
    assert bool((np.abs(z["roi_align_bwd_hip"].transpose(0, 2, 3, 1) - gr) <= 1e-3 + 1e-4 * np.abs(gr)).all())
    # mask crop: the oracle's crop_and_resize, bit for bit
    for case in R.CROP_CASES:
        masks, boxes, idx = R.crop_inputs(case)
        bits, avg = R.mask_crop32(masks, boxes, idx, R.CROP_CASES[case]["S"])
        o = OR.crop_and_resize(torch.from_numpy(masks[idx]), torch.from_numpy(boxes), R.CROP_CASES[case]["S"]).numpy()
        assert np.array_equal(bits.astype(bool), o), case
        assert (avg[6] == 0.5).any() and (avg[7] == 0.5).any(), case          # the >= of the threshold decides there
        assert not np.array_equal(R.mask_crop32(masks, boxes, idx, R.CROP_CASES[case]["S"], "crop_gt")[0], bits)


def _case_inputs(cfg, C, S, seed):
    maps, min_level, s0, aligned = CONFIGS[cfg]
    g = np.random.default_rng(seed)
    feats = [g.standard_normal((R.N_IMG, H, W, C)).astype(f32) for H, W in maps]
    rois = R.rois_of(NAMES)
    go = g.standard_normal((len(rois), S, S, C)).astype(f32)
    return feats, rois, go


def test_fp32_evaluations_stay_inside_every_bound_and_every_mutant_leaves_one():
    left = {m: False for m in R.MUTANTS}
    left["log2_level"] = left["crop_gt"] = None          # the level test below and the crop test above
    fwd_mut = ["gate_exclusive", "no_last_clamp", "count_valid", "no_half", "minsize_aligned", "round_grid", "first_base", "span_last",
               "batch_ignored", "log2_level"]
    for cfg in CONFIGS:
        maps, min_level, s0, aligned = CONFIGS[cfg]
        sc = _scales(cfg)
        for sr in (0, 2):
            feats, rois, go = _case_inputs(cfg, 4, 7, 11 + sr)
            ref, A, n, _ = R.forward64(feats, rois, sc, min_level, 7, 7, sr, aligned)
            bnd = R.f32_bound(ref, A, n)
            for order in ("rows", "cols", "flat"):
                got = R.forward32(feats, rois, sc, min_level, 7, 7, sr, aligned, order)
                assert R.worst_ratio(got, ref, bnd) <= 1.0, (cfg, sr, order)
                assert R.worst_ratio(R.to_bf16(got), ref, R.bf16_bound(ref, A, n)) <= 1.0, (cfg, sr, order)
            for m in fwd_mut:
                mref = R.forward64(feats, rois, sc, min_level, 7, 7, sr, aligned, m)[0]
                if not np.array_equal(mref, ref) and R.worst_ratio(mref, ref, bnd) > 1.0:
                    left[m] = True
            sref, _ = R.scatter64(go, rois, maps, R.N_IMG, sc, min_level, sr, aligned)
            for rev in (False, True):
                got = R.scatter32(go, rois, maps, R.N_IMG, sc, min_level, sr, aligned, rev)
                for l in range(len(maps)):
                    assert R.worst_ratio(got[l], sref[l][0], R.f32_bound(*sref[l])) <= 1.0, (cfg, sr, rev, l)
            # the gather: its reach test and bin ranges change nothing, its mutants do
            for C, tw in ((64, 32), (256, 8)):
                prev = [np.full((R.N_IMG, H, W, 4), 0.75) for H, W in maps]
                plain, _ = R.gather64(go, rois, maps, R.N_IMG, sc, min_level, sr, aligned, prev, 1.0 / 3.0)
                tiled, _ = R.gather64(go, rois, maps, R.N_IMG, sc, min_level, sr, aligned, prev, 1.0 / 3.0, tiles=(4, tw))
                for l in range(len(maps)):
                    assert np.array_equal(plain[l][0], tiled[l][0]), (cfg, sr, C, l)
                for m in ("range_no_slack", "hit_no_pm1", "accum_overwrites", "gscale_both", "first_base"):
                    mut, _ = R.gather64(go, rois, maps, R.N_IMG, sc, min_level, sr, aligned, prev, 1.0 / 3.0, tiles=(4, tw), mutant=m)
                    for l in range(len(maps)):
                        if not np.array_equal(mut[l][0], plain[l][0]) and R.worst_ratio(mut[l][0], plain[l][0], R.bf16_bound(*plain[l])) > 1.0:
                            left[m] = True
    assert [m for m, v in left.items() if v is False] == []


def test_inverted_box_with_a_fixed_grid_needs_the_min_max_span():
    """x 200 -> 100 at scale 1/8, 7 bins, 2 samples: with the span taken from the first sample's lo (the kernels before the fix) six of
    the seven bins lose the weight below it; the oracle pools ordinary averages there"""
    from oracle import roi as OR
    roi = R.rois_of(["inverted"])
    t = R.roi_tables(roi[0], R.LEVELS[:1], [R.SCALE0], 0, 7, 7, 2, 1)
    b = R.roi_tables(roi[0], R.LEVELS[:1], [R.SCALE0], 0, 7, 7, 2, 1, "first_base")
    assert t.G.bin_w < 0 and int((t.X.W.sum(1) != b.X.W.sum(1)).sum()) == 6
    assert np.allclose(t.X.W.sum(1), 2.0) and np.allclose(t.Y.W.sum(1), 2.0)
    H, W = R.LEVELS[0]
    feat = np.random.default_rng(1).standard_normal((R.N_IMG, H, W, 4)).astype(f32)
    ref, A, n, _ = R.forward64([feat], roi, [R.SCALE0], 0, 7, 7, 2, True)
    o = OR.roi_align(torch.from_numpy(feat).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(roi), R.SCALE0, 7, 2, True).permute(0, 2, 3, 1).numpy()
    assert R.worst_ratio(o, ref, R.f32_bound(ref, A, 20.0 + 0 * n)) <= 1.0 and np.abs(ref).min() > 0
    bug = R.forward64([feat], roi, [R.SCALE0], 0, 7, 7, 2, True, "first_base")[0]
    assert R.worst_ratio(bug, ref, R.f32_bound(ref, A, n)) > 1.0


def test_form_tables_name_what_the_header_decides(checker):
    lines, want = [], []
    multi = _maps_req(R.LEVELS)
    for name, c in R.FORWARD_FORMS.items():
        maps = {"single": R.LEVELS[:1], "small": [R.SMALL]}.get(c.get("levels"), R.LEVELS)
        lines.append("pool %s %d %d %d %d %d %d" % (_maps_req(maps), c["C"], len(NAMES), c["S"], c["S"], c["nhwc"], int(not c.get("offset"))))
        want.append((name, c["form"]))
    got, _ = checker(lines + ["pool %s 24 %d 7 7 1 1" % (multi, r) for r in R.R_THRESHOLDS]
                     + ["gplan %s %d %d %d %d" % (_maps_req({"single": R.LEVELS[:1], "small": [R.SMALL]}.get(c.get("levels"), R.LEVELS)),
                                                  R.N_IMG, c["C"], c["S"], c["S"]) for c in R.GATHER_FORMS.values()]
                     + ["gplan 1 %d %d %d %d 7 7" % (R.GATHER_TH8["H"], R.GATHER_TH8["W"], R.GATHER_TH8["N"], R.GATHER_TH8["C"]),
                        "gplan 1 %d %d %d %d 7 7" % (R.GATHER_TH8["H"] - 8, R.GATHER_TH8["W"], R.GATHER_TH8["N"], R.GATHER_TH8["C"]),
                        "gplan %s 2 256 17 17" % multi, "gplan %s 2 24 7 7" % multi, "gplan %s 2 32 7 7" % multi]
                     + ["crop %d" % c["S"] for c in R.CROP_CASES.values()])
    k = len(want)
    for (name, form), line in zip(want, got[:k]):
        f = line.split()
        assert f[1] == form and f[2] == "1", (name, line)
        if name == "sep_nchw_c96_s14":
            assert (int(f[3]), int(f[4])) == (162, 2) and 196 % 162 != 0, line          # two slices, the last one 34 of 162 bins
        if name in ("sep_nchw_c1", "sep_nchw_c300"):
            assert int(f[4]) == 1, line
    assert [int(line.split()[4]) for line in got[k:k + 5]] == [4, 4, 2, 2, 1]
    k += 5
    for c, line in zip(R.GATHER_FORMS.values(), got[k:]):
        f = line.split()
        assert f[1] == "1" and int(f[2]) == 256 // (c["C"] // 8) and int(f[3]) == 4, line
    k += len(R.GATHER_FORMS)
    assert got[k].split()[1:5] == ["1", "8", "8", "1024"] and got[k + 1].split()[3] == "4"
    assert got[k + 2:k + 5] == ["gplan 0"] * 3          # ph = 17, C % 8 != 0 and C < 64: refused
    assert got[k + 5:] == ["crop 1", "crop 4", "crop 8"]


def test_level_rule_differs_from_the_log2_rule_exactly_below_the_powers_of_two():
    differ, boundary = [], []
    for nm in NAMES:
        roi = R.rois_of([nm])[0]
        mine, theirs = R.level_of(roi, 0, 64), R.level_of(roi, 0, 64, "log2_level")
        t = float(R.level_t(roi))
        if mine != theirs:
            differ.append(nm)
        p = 2.0 ** np.ceil(np.log2(t)) if t > 0 else 0.0
        if t > 0 and t < p and (p - t) <= 2.5 * p * 2.0 ** -24:          # 1 - 2 ulps below a power of two (ulp = p 2^-24 there)
            boundary.append(nm)
    # nowhere else: every difference sits 1 - 2 ulps below a power of two (where the fp32 log2 rounds 4 + log2(t) up to the integer; not
    # every such box differs: whether log2 rounds up there is the host library's business), and the exact rule is the lower level
    assert set(differ) <= set(boundary) and len(differ) >= 1, (differ, boundary)
    assert all(nm.startswith("lvl_k") and R.LEVEL_BOXES[nm][1] < 0 for nm in boundary)
    assert all(R.level_of(R.rois_of([nm])[0], 0, 64) == R.level_of(R.rois_of([nm])[0], 0, 64, "log2_level") - 1 for nm in differ)
    # the levels the pooler gives the table: both clamps and every level are reached
    lv = [R.level_of(R.rois_of([nm])[0], R.MIN_LEVEL, 3) for nm in NAMES]
    assert set(lv) == {0, 1, 2}
    assert R.level_of(R.rois_of(["lvl_k0_+0"])[0], R.MIN_LEVEL, 3) == 1 and R.level_of(R.rois_of(["lvl_k0_-1"])[0], R.MIN_LEVEL, 3) == 0
