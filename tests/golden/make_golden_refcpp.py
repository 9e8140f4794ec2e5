"""Generate tests/golden/refcpp.npz: the answers of the reference's own C++ (ROIAlignRotated_cpu.cpp, nms_rotated_cpu.cpp and
cocoeval.cpp, compiled where they lie into oracle/_ref/dgref.so by oracle/build.py) on the inputs of the tests that compare
against them, so that those tests also run where the library cannot be built.  Run in the authoring container only, after
oracle/build.py has built the library:

    python tests/golden/make_golden_refcpp.py

Only outputs are stored; the inputs are the seeded recipes of the tests themselves.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from divergen_amd.evaluation import lvis_eval as LE  # noqa: E402
from tests import _recipes as R  # noqa: E402
from tests import test_gpu_kernels as TK  # noqa: E402
from tests import test_oracle_eval as TE  # noqa: E402
from tests import test_oracle_roi as TR  # noqa: E402


def main():
    ref = R.load_refcpp()
    assert ref is not None, "oracle/_ref/dgref.so is not built (python oracle/build.py where the reference sources are present)"
    out = {}
    feat, rois, go = TR._roi_align_ref_case()
    out["roi_align_fwd_oracle"], out["roi_align_bwd_oracle"] = R.ref_roi_align(ref, feat, rois, go, 0.25, 14)
    boxes, wh, scores = TR._nms_ref_case()
    for thr in (0.3, 0.5, 0.9):
        out["nms_keep_oracle_%02d" % round(thr * 10)] = R.ref_nms(ref, boxes, wh, scores, thr)
    feat, rois, go, boxes, wh, scores = TK._reference_sources_case()
    out["roi_align_fwd_hip"], out["roi_align_bwd_hip"] = R.ref_roi_align(ref, feat, rois, go, 0.25, 7)
    for thr in (0.3, 0.5, 0.7):
        out["nms_keep_hip_%02d" % round(thr * 10)] = R.ref_nms(ref, boxes, wh, scores, thr)
    for seed in (0, 1, 2):
        gt, dets = TE._dataset(seed)
        ev = LE.LVISEval(gt, dets, iou_type="bbox", max_dets=300)
        ev.run()
        out["cocoeval_precision_%d" % seed], out["cocoeval_recall_%d" % seed] = R.ref_cocoeval(ref, ev, gt, dets)
    out = {k: v.numpy() if hasattr(v, "numpy") else np.asarray(v) for k, v in out.items()}
    path = os.path.join(HERE, "refcpp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s %.1f KB: %s" % (path, os.path.getsize(path) / 1024, ", ".join("%s %s %s" % (k, v.dtype, v.shape) for k, v in out.items())))


if __name__ == "__main__":
    main()
