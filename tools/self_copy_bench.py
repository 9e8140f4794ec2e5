"""Time the self copy-paste kernels (dgx_self_copy_paste) on the 1024 x 1024 case of tests/test_gpu_self_copy.py (n0 = 20 destination
objects, ns = 40 source objects, m = 25 selected) next to the pool compositor (dgx_copy_paste, n0 = 10, K = 19: the problem of
tools/compositor_modes_bench.py) in the same process, and next to the same paste from S = 2 and S = 3 source images of that frame
(layers.self_copy_paste_multi: dgx_self_copy_merge, the read-back of validity and boxes, dgx_self_copy_paste_merged; every source
brings m = 25 objects), in milliseconds per sample.  Device-event timing around `--iters` calls after `--warmup`; one JSON line.

    python tools/self_copy_bench.py [--iters 100] [--paste-all NS] [--rm-bg] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o selfcopy -- python tools/self_copy_bench.py --iters 50

--paste-all NS adds the same destination with a source of NS objects pasted whole (layers.self_copy_paste_all: dgx_self_copy_paste_all,
no bound of 99), --rm-bg background removal of the destination (layers.remove_background: dgx_remove_background, n = 20 masks,
algorithmic bytes (n + 6) * H * W), both in the same run as the single-source figure they are compared with.
The outputs are checked against tests/_selfcopy_ref.py / _selfcopy_multi_ref.py once before timing (a wrong kernel is not timed).  Algorithmic bytes of one
self copy: (n0 + m) * H * W * 2 + 9 * H * W (every mask plane read and written once, two images read, one written)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from divergen_amd import layers as la  # noqa: E402
from divergen_amd.layers.copy_paste import pack_pastes  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--paste-all", type=int, default=0, metavar="NS", help="also time a source of NS objects pasted whole")
    p.add_argument("--rm-bg", action="store_true", help="also time background removal of the destination")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "self_copy_bench needs a GPU"
    import _selfcopy_multi_ref as MR
    import _selfcopy_ref as SR
    from compositor_modes_bench import problem
    from test_gpu_self_copy import _scene
    dev = "cuda:0"
    size, n0, ns, m = 1024, 20, 40, 25
    rng = np.random.default_rng(1024)
    dst, src = _scene(rng, n0, size, size), _scene(rng, ns, size, size)
    sel = rng.permutation(ns)[:m]
    d = [torch.from_numpy(x).to(dev) for x in dst]
    s = [torch.from_numpy(x).to(dev) for x in src]
    ref = SR.self_copy(*dst, *src, sel)
    got = la.self_copy_paste(*d, *s, sel, canvas_hw=(size, size))
    for k in ("image", "masks", "boxes", "labels"):
        assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
    # S source images of the same frame, each with its own m selected objects (the first is the single source above)
    more = [_scene(rng, m, size, size) for _ in range(2)]
    multi = [[(src[0], src[1][sel], src[2][sel], src[3][sel])] + more[:k] for k in (1, 2)]
    multi_dev = [[tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in sc) for sc in srcs] for srcs in multi]
    for srcs, srcs_dev in zip(multi, multi_dev):
        ref = MR.self_copy_multi(*dst, srcs)
        got = la.self_copy_paste_multi(*d, srcs_dev)
        for k in ("image", "masks", "boxes", "labels"):
            assert np.array_equal(got[k].cpu().numpy(), ref[k]), (len(srcs), k)
    img, masks, boxes, labels, pastes = problem()
    c = [torch.from_numpy(x).to(dev) for x in (img, masks, boxes, labels)]
    pk = pack_pastes(pastes, dev)
    calls = {"self_copy": lambda: la.self_copy_paste(*d, *s, sel, canvas_hw=(size, size), lazy_masks=True),
             "self_copy_s2": lambda: la.self_copy_paste_multi(*d, multi_dev[0], lazy_masks=True),
             "self_copy_s3": lambda: la.self_copy_paste_multi(*d, multi_dev[1], lazy_masks=True),
             "copy_paste_k19": lambda: la.copy_paste(*c, pk, lazy_masks=True)}
    if a.paste_all:
        import _scp_modes_ref as PR
        whole = _scene(rng, a.paste_all, size, size)
        wd = [torch.from_numpy(x).to(dev) for x in whole]
        ref = PR.paste_all(*dst, *whole)
        got = la.self_copy_paste_all(*d, *wd, canvas_hw=(size, size))
        for k in ("image", "masks", "boxes", "labels"):
            assert np.array_equal(got[k].cpu().numpy(), ref[k]), ("paste_all", k)
        calls["paste_all_%d" % a.paste_all] = lambda: la.self_copy_paste_all(*d, *wd, canvas_hw=(size, size), lazy_masks=True)
    if a.rm_bg:
        assert torch.equal(la.remove_background(d[0], d[1]), d[0] * d[1].any(0).to(torch.uint8)[None])
        calls["rm_bg"] = lambda: la.remove_background(d[0], d[1])
    nbytes = (n0 + m) * size * size * 2 + 9 * size * size
    res = {"what": "1 image 1024x1024; self copy n0=20 ns=40 m=25 (s2 / s3: merge + read-back + paste from 2 / 3 sources of m=25 each); pool compositor n0=10 K=19; ms per call (device events, %d calls)" % a.iters,
           "self_copy_algorithmic_bytes": nbytes}
    for name, fn in calls.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        res["ms_" + name] = round(t0.elapsed_time(t1) / a.iters, 4)
    res["self_copy_GBps_per_call"] = round(nbytes / (res["ms_self_copy"] * 1e-3) / 1e9, 1)
    if a.paste_all:
        res["paste_all_algorithmic_bytes"] = (n0 + a.paste_all) * size * size * 2 + 9 * size * size
    if a.rm_bg:
        res["rm_bg_algorithmic_bytes"] = (n0 + 6) * size * size
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
