"""Record tests/golden/wgrad_plans.json: what the weight-gradient family's host-only entry points answer for the shapes of the
weight-gradient tests, the groups the layers form and a sweep of small sizes.  Recorded ONCE from the library as it was BEFORE
csrc/wgrad_plan.h existed (the planner written out in wgrad256.hip / wgrad_lw.hip / wgrad_gemm.hip); tests/test_host_wgrad_plan.py
reproduces every row from the header.

    DGX_LIB=<the library to record from> python tests/golden/make_golden_wgrad_plans.py

None of the entry points used makes a HIP call, so the library is loaded with ctypes on a machine without a GPU.

Rows:
  group   probs [[M, Nn, Kk, has_gb], ...]   form / ws at dgx_dev_set("wgrad_lw", 0 | 1 | 2): dgx_wgrad_grouped_form,
                                             dgx_wgrad_grouped_workspace_bytes
  single  M Nn Kk                            parent_bytes: dgx_wgrad_workspace_bytes of the retired 128 x 128 kernel (kept as a record: the
                                             entry point now reports the one-problem size of the grouped path)
  conv    N H W Cin Cout                     ws, ws_bias: dgx_conv3x3_wgrad_workspace_bytes, dgx_conv3x3_wgrad_bias_workspace_bytes
  multi   levels [[N, H, W], ...] Cin Cout   ws: dgx_conv3x3_wgrad_bias_multi_workspace_bytes
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

c_i, c_p, c_i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64


class Prob(ctypes.Structure):
    _fields_ = [("dy", c_p), ("x", c_p), ("gw", c_p), ("M", c_i), ("Nn", c_i), ("Kk", c_i), ("gb", c_p)]


class Item(ctypes.Structure):
    _fields_ = [("dypad", c_p), ("xpad", c_p), ("N", c_i), ("H", c_i), ("W", c_i)]


def swin_block(C, Mt, Mw):
    """the four Linears of a block in the order swin_block.backward queues them: fc2, fc1, proj, qkv (all with a bias)"""
    return [(Mt, C, 4 * C, 1), (Mt, 4 * C, C, 1), (Mw, C, C, 1), (Mw, 3 * C, C, 1)]


def groups():
    out = []
    # tests/test_gpu_kernels.py
    for s in [(16384, 576, 192), (20000, 192, 768), (16384 + 17, 1152, 384), (17000, 64, 72)]:                  # test_linear_wgrad_split_m
        out.append([s + (0,)])
    for g in [[(8192, 768, 3072), (8192, 3072, 768), (10368, 768, 768), (10368, 2304, 768)], [(100, 192, 264), (8192, 40, 768), (4000, 768, 776)],
              [(2048, 1536, 1536)], [(33, 8, 8)]]:                                                               # test_linear_wgrad_grouped
        out.append([s + (0,) for s in g])
    for M in (1100, 2048):                                                                                       # ..._loader_wave
        out.append([(M, 1536, 1536, int(k != 1)) for k in range(5)] + [(M + 8, 520, 392, 1), (M, 8, 8, 1)])
    for g in [[(16384, 576, 192)], [(1024, 1464, 1024)], [(8192, 768, 3072), (8192, 3072, 768), (10368, 768, 768), (10368, 2304, 768)],
              [(1024, 1024, 12544), (1024, 1024, 1024), (1024, 1464, 1024)], [(20000, 192, 768), (17000, 64, 72)]]:   # ..._with_bias_gradients
        out.append([s + (1,) for s in g])
    # tests/test_gpu_pins.py: 7 stage-2 blocks, 32 problems, ragged contraction (every fifth problem without a bias)
    for blocks, C, Mw, Mt in [(7, 768, 10368, 8192), (8, 576, 4608 + 16, 4096), (3, 776, 10368 - 24, 8192 + 40)]:
        g = [p for _ in range(blocks) for p in swin_block(C, Mt, Mw)]
        out.append([(M, Nn, Kk, int(k % 5 != 4)) for k, (M, Nn, Kk, _) in enumerate(g)])
    # layers/box_stage.py: fc1, fc2, the predictor pair (R sampled boxes; 512 per image)
    for R in (512, 1024, 2048):
        out.append([(R, 1024, 12544, 1), (R, 1024, 1024, 1), (R, 1464, 1024, 1)])
    # layers/swin_block.py: per-block groups of Swin-T (C = 96, window 7) and Swin-L (C = 192, window 12), stages 0-3, 2 images of 1024^2
    # and of 512 x 640; then what flush_wgrads packs from them: two blocks, and two blocks + the fc2 / fc1 of a third (<= 12 problems)
    for C0, ws in ((96, 7), (192, 12)):
        for B, H, W in ((2, 256, 256), (2, 128, 160)):
            for st in range(4):
                h, w, C = H >> st, W >> st, C0 << st
                Mt, Mw = B * h * w, B * (-(-h // ws) * ws) * (-(-w // ws) * ws)
                blk = swin_block(C, Mt, Mw)
                out += [blk, blk + blk, blk + blk + blk[:2], blk + blk + blk]
    return out


def sweep():
    out = []
    shapes = [(8, 8), (64, 72), (264, 200), (512, 264), (1536, 1536)]
    for n in (1, 2, 9, 12, 13, 32, 33):
        for M in (1, 32, 33, 300, 1023, 1024, 4000):
            for k, (Nn, Kk) in enumerate(shapes):
                for gb in (0, 1):
                    if (n > 12 and k < 3 and M < 1023) or (k == 4 and gb and n > 2 and M != 1024):
                        continue             # (keeps the file small: rows the n <= 12 ones already cover)
                    out.append([(M + 8 * (i % 3 == 1), Nn, Kk, gb if i % 2 == 0 else 0) for i in range(n)])
    # the 192-item and 0.74-fill thresholds of the loader-wave form: 48-item problems plus one of 47 / 43 / 42 items
    big = (1024, 1536, 1536, 1)
    for g in ([big] * 4, [big] * 3 + [(1024, 47 * 256, 192, 0)], [big] * 3 + [(1024, 47 * 256, 200, 0)], [big] * 7 + [(1024, 43 * 256, 192, 1)],
              [big] * 7 + [(1024, 42 * 256, 192, 1)], [big] * 5 + [(2048, 17 * 256, 192, 0)], [big] * 5 + [(1024, 16 * 256, 192, 0)],
              [big] * 4 + [(1023, 8, 8, 0)], [big] * 12, [big] * 13, [big] * 32, [(1024, 256, 192, 0)], [(1023, 256, 192, 0)]):
        out.append(list(g))
    return out


def main():
    import _conv_ref64 as R
    lib = ctypes.CDLL(os.environ.get("DGX_LIB", os.path.join(ROOT, "divergen_amd", "csrc", "libdgx.so")))
    lib.dgx_wgrad_grouped_workspace_bytes.restype = c_i64
    lib.dgx_wgrad_workspace_bytes.restype = c_i64
    lib.dgx_conv3x3_wgrad_workspace_bytes.restype = c_i64
    lib.dgx_conv3x3_wgrad_bias_workspace_bytes.restype = c_i64
    lib.dgx_conv3x3_wgrad_bias_multi_workspace_bytes.restype = c_i64
    rows, singles = [], set()
    for g in groups() + sweep():
        n = len(g)
        arr = (Prob * n)()
        for i, (M, Nn, Kk, gb) in enumerate(g):
            arr[i].dy, arr[i].x, arr[i].gw, arr[i].gb = 16, 16, 16, (16 if gb else None)      # never dereferenced
            arr[i].M, arr[i].Nn, arr[i].Kk = M, Nn, Kk
            singles.add((M, Nn, Kk))
        form, ws = [], []
        for knob in (0, 1, 2):
            assert lib.dgx_dev_set(b"wgrad_lw", knob) == 0
            form.append(int(lib.dgx_wgrad_grouped_form(arr, n)))
            ws.append(int(lib.dgx_wgrad_grouped_workspace_bytes(arr, n)))
        assert lib.dgx_dev_set(b"reset", 0) == 0
        rows.append({"kind": "group", "probs": [list(p) for p in g], "form": form, "ws": ws})
    for M, Nn, Kk in sorted(singles) + [(0, 8, 8), (8, 0, 8)]:
        rows.append({"kind": "single", "M": M, "Nn": Nn, "Kk": Kk, "parent_bytes": int(lib.dgx_wgrad_workspace_bytes(M, Nn, Kk))})
    geoms = list(R.WGRAD_ROWS) + [g for g in R.GEOMS if g not in R.WGRAD_ROWS] + [(2, 128, 128, 256, 256), (2, 64, 64, 256, 256), (1, 1, 1, 8, 8)]
    for N, H, W, Cin, Cout in geoms:
        rows.append({"kind": "conv", "N": N, "H": H, "W": W, "Cin": Cin, "Cout": Cout,
                     "ws": int(lib.dgx_conv3x3_wgrad_workspace_bytes(N, H, W, Cin, Cout)),
                     "ws_bias": int(lib.dgx_conv3x3_wgrad_bias_workspace_bytes(N, H, W, Cin, Cout))})
    fpn = [(2, 128, 128), (2, 64, 64), (2, 32, 32), (2, 16, 16), (2, 8, 8)]
    for levels in (R.MULTI_LEVELS, R.WGRAD_MULTI_LEVELS, fpn, fpn[1:], fpn[2:]):
        for Cin, Cout in R.MULTI_WIDTHS + [w for w in R.WGRAD_MULTI_WIDTHS if w not in R.MULTI_WIDTHS]:
            for n in range(1, len(levels) + 1):
                items = (Item * n)()
                for i, (b, h, w) in enumerate(levels[:n]):
                    items[i].N, items[i].H, items[i].W = b, h, w
                rows.append({"kind": "multi", "levels": [list(v) for v in levels[:n]], "Cin": Cin, "Cout": Cout,
                             "ws": int(lib.dgx_conv3x3_wgrad_bias_multi_workspace_bytes(items, n, Cin, Cout))})
    head = {"recorded": "on a machine without a GPU, through ctypes, from the library built at the parent of the commit that added "
                        "csrc/wgrad_plan.h (the entry points make no HIP call)",
            "rows": rows}
    with open(os.path.join(ROOT, "tests", "golden", "wgrad_plans.json"), "w") as f:
        f.write('{"recorded": %s,\n "rows": [\n' % json.dumps(head["recorded"]))
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n ]}\n")
    print(len(rows), "rows")


if __name__ == "__main__":
    main()
