"""CPU: divergen_amd/csrc/gemm_plan.h (which kernel form, tile and split-K plan a forward / input-gradient GEMM gets) compiled for the
host and checked without a GPU:

* the pins of tests/test_gpu_pins.py (BENCH_GEMMS, the resident-panel edge shapes) get the form the GPU test expects, at reserved
  CUs 0 and 16;
* tests/golden/gemm_plans.json -- what dgx_gemm_last_form reported for the shapes of the GEMM and convolution tests on an MI355X, at
  default knobs and with gemm_lw forced to 0 and 1, recorded from the library BEFORE the planner existed -- is reproduced row by row;
* the invariants of a plan (no empty split, slabs fit the workspace, the grid covers every tile, every tile is instantiated, ...)
  over a grid of small shapes, modes, workspaces and knob settings (tests/native/gemm_plan_check.cpp)."""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pins():
    spec = importlib.util.spec_from_file_location("_gpu_pins_for_plan", os.path.join(ROOT, "tests", "test_gpu_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    edges = None
    for mark in mod.test_resident_panel_gemm_edges.pytestmark:
        if mark.name == "parametrize" and mark.args[0].startswith("M,N,K"):
            edges = mark.args[1]
    return mod.BENCH_GEMMS, edges


def _ws(M, N):
    from divergen_amd.layers import gemm_ops
    return gemm_ops.WS_BYTES if M * N * 8 <= gemm_ops.WS_BYTES else 0      # gemm_ops._launch


def _cases():
    bench, edges = _pins()
    assert len(bench) >= 20 and len(edges) == 5
    lines = []
    for M, N, K, mode, wmap, expect in bench:
        bf = int(wmap is not None and wmap[5] == torch.bfloat16)
        form, bm, bn = expect if expect is not None else (-1, 0, 0)
        lines.append("pin %d %d %d %d %d %d %d %d %d" % (M, N, K, mode, bf, _ws(M, N), form, bm, bn))
    for M, N, K, mode, wmap in edges:
        bf = int(wmap is not None and wmap[5] == torch.bfloat16)
        lines.append("k192 %d %d %d %d %d %d" % (M, N, K, mode, bf, _ws(M, N)))
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plans.json")) as f:
        rows = json.load(f)
    assert len(rows) >= 300
    for r in rows:
        ms = r.get("Ms", [])
        got = [r["form"], r["bm"], r["bn"], r["splits"]] if r["form"] is not None else [-1, 0, 0, 0]
        lines.append("row %d %s %d %d %d %d %d %d %d %d %d %d %d %d %d" % (
            len(ms), " ".join(str(m) for m in ms), r.get("M", 0), r["N"], r["K"], r["mode"], int(r["res_dtype"] == 1),
            int(r["kind"] != "gemm"), r["ws"], r["lw"], r["reserved"], *got))
    return lines


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_gemm_plan_pins_golden_table_and_invariants(tmp_path):
    exe, cases = str(tmp_path / "gemm_plan_check"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "gemm_plan_check.cpp")])
    lines = _cases()
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) == len(lines) and int(out.stdout.split()[2]) >= 100000
