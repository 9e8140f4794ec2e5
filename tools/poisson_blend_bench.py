"""Time the 'possion' blend (INPUT.CP_POISSON; csrc/poisson_blend.hip) on one 1024 x 1024 image:
  * one paste through dgx_poisson_blend for soft-edged elliptical footprints in rectangles of 32 x 32, 128 x 128, 256 x 256 and
    400 x 500 px: milliseconds per paste, iterations used, the iteration bound and |U|;
  * the compositor with 10 pastes of 51..307 px, CP_METHOD ['basic'] against ['possion'] (dgx_copy_paste / dgx_copy_paste_blend_ws).
Device-event timing around `--iters` calls after `--warmup`; prints one JSON line.

    python tools/poisson_blend_bench.py [--iters 5] [--out FILE]

Every solve's report is checked (converged within the bound) before its time is taken."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from divergen_amd import _lib as L  # noqa: E402
from divergen_amd import layers as la  # noqa: E402
from divergen_amd.layers.copy_paste import check_poisson_report, pack_pastes, poisson_unknowns  # noqa: E402
from compositor_modes_bench import problem  # noqa: E402

SIZE = 1024
FOOTPRINTS = ((32, 32), (128, 128), (256, 256), (400, 500))


def soft(rng, h, w):
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.sqrt(((xx + 0.5 - w / 2) / (w / 2)) ** 2 + ((yy + 0.5 - h / 2) / (h / 2)) ** 2)
    rgba[..., 3] = np.clip((1.0 - d) * 600.0, 0, 255).astype(np.uint8)
    return rgba


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "poisson_blend_bench needs a GPU"
    dev = "cuda:0"
    rng = np.random.default_rng(3)
    img = torch.from_numpy(rng.integers(0, 256, (3, SIZE, SIZE), dtype=np.uint8)).to(dev)
    res = {"what": "possion blend on 1 image %dx%d, ms per call (device events, %d calls)" % (SIZE, SIZE, a.iters), "paste": {}}
    for h, w in FOOTPRINTS:
        rgba, x0, y0 = soft(rng, h, w), (SIZE - w) // 2, (SIZE - h) // 2
        _, rep = la.poisson_blend(img, rgba, x0, y0)
        rep = check_poisson_report(rep[None])[0]
        ms = timed(lambda: la.poisson_blend(img, rgba, x0, y0), a.warmup, a.iters)
        res["paste"]["%dx%d" % (h, w)] = {"ms": round(ms, 3), "iterations": int(rep[0]), "unknowns": int(rep[3]),
                                           "max_iter": int(L.lib().dgx_poisson_max_iter(SIZE, SIZE, poisson_unknowns([0, h, w, x0, y0], SIZE, SIZE)))}
    im, masks, boxes, labels, pastes = problem(K=10)
    di, dm, db, dl = (torch.from_numpy(x).to(dev) for x in (im, masks, boxes, labels))
    pk = pack_pastes(pastes, dev)
    K = len(pastes)
    out = la.copy_paste(di, dm, db, dl, pk, lazy_masks=True, modes=[3] * K, allow_poisson=True)
    rep = check_poisson_report(out["poisson_report"], [3] * K)
    res["compositor_K10"] = {
        "ms_basic": round(timed(lambda: la.copy_paste(di, dm, db, dl, pk, lazy_masks=True), 10, 20 * a.iters), 4),
        "ms_possion": round(timed(lambda: la.copy_paste(di, dm, db, dl, pk, lazy_masks=True, modes=[3] * K, allow_poisson=True), a.warmup, a.iters), 3),
        "iterations": [int(v) for v in rep[:, 0]], "paste_px": [int(p[0].shape[0]) for p in pastes]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
