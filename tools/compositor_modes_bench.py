"""Time the copy-paste compositor per blend mode: 'basic' (dgx_copy_paste), 'alpha', 'gaussian' and a mixed list
(dgx_copy_paste_blend) on one 1024 x 1024 image with 10 original instances and 19 soft-edged pastes of 51..307 px -- the
shape of one image of the bench step.  Device-event timing around `--iters` calls after `--warmup`; prints one JSON line.

    python tools/compositor_modes_bench.py [--iters 200] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o modes -- python tools/compositor_modes_bench.py --iters 50

The pixel outputs of each mode are checked against tests/_blend_ref.py once before timing (a wrong kernel is not timed)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from divergen_amd import layers as la  # noqa: E402
from divergen_amd.layers.copy_paste import pack_pastes  # noqa: E402
from oracle import compositor as OK  # noqa: E402


def problem(size=1024, n=10, K=19, seed=11):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    masks = np.zeros((n, size, size), np.uint8)
    for i in range(n):
        cx, cy, rx, ry = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(8, 200), rng.uniform(8, 200)
        masks[i] = (((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2) <= 1
    img = rng.integers(0, 256, (3, size, size), dtype=np.uint8)
    pastes = []
    for k in range(K):
        s = int(rng.uniform(51, 307))
        rgba = rng.integers(0, 256, (s, s, 4), dtype=np.uint8)
        y2, x2 = np.mgrid[0:s, 0:s]
        d = np.sqrt(((x2 + 0.5 - s / 2) / (s / 2)) ** 2 + ((y2 + 0.5 - s / 2) / (s / 2)) ** 2)
        rgba[..., 3] = np.clip((1.0 - d) * 600.0, 0, 255).astype(np.uint8)
        pastes.append((rgba, int(rng.integers(-s // 2, size - s // 2)), int(rng.integers(-s // 2, size - s // 2)), 2000 + k))
    return img, masks, OK.get_bboxes(masks), rng.integers(0, 1203, n).astype(np.int64), pastes


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--no-check", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "compositor_modes_bench needs a GPU"
    dev = "cuda:0"
    img, masks, boxes, labels, pastes = problem()
    K = len(pastes)
    modes = {"basic": None, "alpha": [1] * K, "gaussian": [2] * K, "mixed": [k % 3 for k in range(K)]}
    di, dm, db, dl = (torch.from_numpy(x).to(dev) for x in (img, masks, boxes, labels))
    pk = pack_pastes(pastes, dev)
    if not a.no_check:
        import _blend_ref as BR
        for name, m in modes.items():
            ref = BR.blend_chain(img, pastes, m or [0] * K)[-1]
            got = la.copy_paste(di, dm, db, dl, pk, modes=m)["image"].cpu().numpy()
            assert np.array_equal(got, ref), name
    res = {"what": "compositor per blend mode, 1 image 1024x1024, n0=10, K=19, ms per call (device events, %d calls)" % a.iters}
    for name, m in modes.items():
        for _ in range(a.warmup):
            la.copy_paste(di, dm, db, dl, pk, lazy_masks=True, modes=m)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            la.copy_paste(di, dm, db, dl, pk, lazy_masks=True, modes=m)
        t1.record()
        torch.cuda.synchronize()
        res["ms_" + name] = round(t0.elapsed_time(t1) / a.iters, 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
