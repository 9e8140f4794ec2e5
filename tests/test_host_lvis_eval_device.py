"""Host side of the device LVIS evaluator (TEST.LVIS_EVAL_DEVICE): the batched RLE string decode against
lvis_eval.rle_string_to_counts, the build key and its default, and the wrappers' refusal of CPU tensors."""
import ctypes
import json
import sys

import numpy as np
import pytest
import torch

from divergen_amd.evaluation.lvis_eval import rle_string_to_counts


def _to_string(counts):
    """dgx_rle_to_string (maskApi.c rleToString) of one run-length list."""
    from divergen_amd import _lib
    c = np.asarray(counts, dtype=np.int32)
    cap = 8 * max(len(c), 1)
    buf = ctypes.create_string_buffer(cap)
    n = _lib.lib().dgx_rle_to_string(c.ctypes.data_as(ctypes.c_void_p), len(c), buf, cap)
    assert 0 <= n <= cap
    return buf.raw[:n]


def _run_lists():
    rng = np.random.RandomState(7)
    lists = [
        [],                                                    # the empty mask's string is empty only for no runs at all
        [480 * 640],                                           # a single run: an all-background image
        [0, 17, 5, 3],                                         # a leading zero run: the mask is set at pixel 0
        [0, 2 ** 15, 1, 2 ** 15 + 7, 2, 2 ** 20, 3],           # runs >= 2^15: four and more characters
        [1, 2 ** 17, 1, 1, 2 ** 17, 1, 2 ** 16, 2, 1, 70000],  # long and short alternate: deltas against two back are negative
        [5, 1, 100000, 1, 5, 100000, 1, 1],
    ]
    for _ in range(20):
        n = int(rng.randint(1, 60))
        big = rng.rand(n) < 0.3
        c = np.where(big, rng.randint(2 ** 15, 2 ** 22, n), rng.randint(1, 40, n))
        if rng.rand() < 0.3:
            c[0] = 0
        lists.append([int(v) for v in c])
    return lists


def test_rle_from_string_equals_python_decoder():
    from divergen_amd.layers.eval_ops import rle_from_strings
    lists = _run_lists()
    strings = [_to_string(c) for c in lists]
    # the cases this test is about are really present
    assert any(len(s) == 0 for s in strings)
    assert any(max(c, default=0) >= 2 ** 15 for c in lists)
    assert any(any(c[i] < c[i - 2] for i in range(3, len(c))) for c in lists)             # a negative delta: the sign-extension branch
    assert any(len(c) > 0 and c[0] == 0 for c in lists) and any(len(c) == 1 for c in lists)
    counts, off = rle_from_strings(strings)
    assert off.dtype == np.int64 and off.shape == (len(strings) + 1,) and off[0] == 0
    for i, (s, c) in enumerate(zip(strings, lists)):
        want = rle_string_to_counts(s)
        assert want == c                                      # the writer and the Python reader agree to begin with
        assert counts[off[i]:off[i + 1]].tolist() == want, i
    # str and bytes are both taken
    c2, o2 = rle_from_strings([s.decode("ascii") for s in strings])
    assert np.array_equal(c2, counts) and np.array_equal(o2, off)


def test_rle_from_string_batch_with_empty_first_and_last():
    from divergen_amd.layers.eval_ops import rle_from_strings
    strings = [b"", _to_string([3, 4, 5]), b"", _to_string([0, 2 ** 16, 9, 1, 2 ** 16]), b""]
    counts, off = rle_from_strings(strings)
    assert off.tolist() == [0, 0, 3, 3, 8, 8]
    assert counts.tolist() == [3, 4, 5, 0, 2 ** 16, 9, 1, 2 ** 16]
    counts, off = rle_from_strings([])
    assert counts.size == 0 and off.tolist() == [0]
    counts, off = rle_from_strings([b""])
    assert counts.size == 0 and off.tolist() == [0, 0]


def test_rle_from_string_reports_the_needed_size():
    from divergen_amd import _lib
    s = _to_string([7, 2 ** 15, 3, 1, 2 ** 15])
    off = np.array([0, len(s)], dtype=np.int64)
    co = np.full(2, -9, dtype=np.int64)
    fn = _lib.lib().dgx_rle_from_string
    assert fn(ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p), off.ctypes.data, 1, None, 0, co.ctypes.data) == -5
    assert co.tolist() == [0, 5]
    out = np.full(6, -1, dtype=np.int64)
    assert fn(ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p), off.ctypes.data, 1, out.ctypes.data, 5, co.ctypes.data) == 5
    assert out.tolist() == [7, 2 ** 15, 3, 1, 2 ** 15, -1]


def test_run_layout_equals_rle_runs():
    """The host layout the IoU kernel reads (start, end, cumulative length per foreground run, CSR over masks) is
    lvis_eval.rle_runs of every mask: odd and even run counts, empty lists, a leading zero run, an empty mask first and last."""
    from divergen_amd.evaluation.lvis_eval import rle_runs
    from divergen_amd.evaluation.lvis_eval_device import _runs_csr
    lists = [[]] + _run_lists() + [[12], []]
    counts = np.asarray([v for c in lists for v in c], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
    s, e, cum, run_off = _runs_csr(counts, off)
    assert s.dtype == e.dtype == cum.dtype == np.int32 and run_off.dtype == np.int64
    assert run_off.tolist() == np.concatenate([[0], np.cumsum([len(c) // 2 for c in lists])]).tolist()
    for i, c in enumerate(lists):
        ws, wt, wc = rle_runs({"counts": c})
        a, b = run_off[i], run_off[i + 1]
        assert s[a:b].tolist() == ws.tolist() and e[a:b].tolist() == wt.tolist() and cum[a:b].tolist() == wc[1:].tolist(), i
    z = _runs_csr(np.zeros(0, dtype=np.int64), np.zeros(3, dtype=np.int64))
    assert z[0].size == 0 and z[3].tolist() == [0, 0, 0]


def test_key_exists_and_defaults_to_off():
    from divergen_amd.config import get_cfg
    cfg = get_cfg()
    assert cfg.TEST.LVIS_EVAL_DEVICE is False
    cfg.merge_from_list(["TEST.LVIS_EVAL_DEVICE", True])
    assert cfg.TEST.LVIS_EVAL_DEVICE is True


def _tiny_split(tmp_path, name):
    from divergen_amd.data.build import register_lvis_instances
    gt = {"images": [{"id": 1, "height": 40, "width": 50, "neg_category_ids": [], "not_exhaustive_category_ids": []}],
          "categories": [{"id": 1, "frequency": "f"}],
          "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "bbox": [5, 5, 20, 10], "area": 200.0,
                           "segmentation": [[5, 5, 25, 5, 25, 15, 5, 15]]}]}
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(gt))
    register_lvis_instances(name, str(path), str(tmp_path))


def test_evaluator_with_the_key_off_does_not_import_the_device_module(tmp_path):
    from divergen_amd.config import get_cfg
    from divergen_amd.evaluation import LVISEvaluator
    from divergen_amd.structures import Boxes, Instances
    _tiny_split(tmp_path, "lvis_eval_device_host_test")
    name = "divergen_amd.evaluation.lvis_eval_device"
    saved = sys.modules.pop(name, None)
    try:
        cfg = get_cfg()
        outs = {}
        for how, ev in (("arg", LVISEvaluator("lvis_eval_device_host_test", None, False, None, device_eval=False)),
                        ("cfg", LVISEvaluator("lvis_eval_device_host_test", cfg, False, None))):
            assert ev._device_eval is False
            ev.reset()
            inst = Instances((40, 50), pred_boxes=Boxes(torch.tensor([[5.0, 5.0, 25.0, 15.0]])), scores=torch.tensor([0.9]),
                             pred_classes=torch.tensor([0]))
            ev.process([{"image_id": 1}], [{"instances": inst}])
            outs[how] = ev.evaluate()
            assert abs(outs[how]["bbox"]["AP"] - 100.0) < 1e-9
        assert name not in sys.modules
        cfg.TEST.LVIS_EVAL_DEVICE = True
        assert LVISEvaluator("lvis_eval_device_host_test", cfg, False, None)._device_eval is True
        assert LVISEvaluator("lvis_eval_device_host_test", cfg, False, None, device_eval=False)._device_eval is False
    finally:
        if saved is not None:
            sys.modules[name] = saved


def test_image_too_large_for_int32_run_positions_is_refused_by_name():
    from divergen_amd import _lib
    from divergen_amd.evaluation.lvis_eval_device import LVISEvalDevice
    gt = {"images": [{"id": 7, "height": 40, "width": 50}, {"id": 4711, "height": 65536, "width": 32768}],
          "categories": [{"id": 1, "frequency": "f"}], "annotations": []}
    with pytest.raises(_lib.DgxError, match="4711"):
        LVISEvalDevice(gt, [], "segm")
    LVISEvalDevice(gt, [], "bbox")                            # boxes carry no run positions


def test_wrappers_refuse_cpu_tensors():
    from divergen_amd import _lib
    from divergen_amd.layers import eval_ops as E
    off = torch.tensor([0, 1], dtype=torch.int64)
    box = torch.zeros(1, 4, dtype=torch.float64)
    with pytest.raises(_lib.DgxError):
        E.box_iou_xywh(box, box, off, off, off, 1)
    runs = (torch.zeros(1, dtype=torch.int32),) * 3 + (off,)
    with pytest.raises(_lib.DgxError):
        E.rle_iou(runs, runs, off, off, off, 1)
    f, b, i = torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.uint8), torch.ones(1, dtype=torch.int64)
    with pytest.raises(_lib.DgxError):
        E.lvis_match(f, off, off, off, f, b, i, f, b, torch.tensor([0.5], dtype=torch.float64), torch.tensor([[0.0, 1e10]], dtype=torch.float64))
    with pytest.raises(_lib.DgxError):
        E.lvis_accumulate(torch.zeros(1, 1, 1, dtype=torch.uint8), torch.zeros(1, 1, 1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), off,
                          torch.ones(1, 1, dtype=torch.int64), torch.tensor([0.0, 1.0], dtype=torch.float64))
