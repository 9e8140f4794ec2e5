"""CPU: divergen_amd/csrc/winmap.h (the window map shared by the LayerNorm, residual, window gather / scatter, GEMM-epilogue and
attention kernels) compiled for the host and checked against a brute-force enumeration of the reference's pad -> roll -> partition
(swintransformer.py:216-233).  Compact order: real / padding classification, compact row of every token, its inverse, the padding
rows' order.  Classic order: row -> token against the materialised table for every H, W in 1..30, ws in {2, 3, 7, 12}, every shift
and B in {1, 2}; token -> row its inverse; the count of padding rows; the 32- and 64-bit instantiations against each other.  The host
validity check against the per-entry-point checks it replaced."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    """(compact cases, classic cases, validity cases) the stand-alone program checked"""
    exe = str(tmp_path_factory.mktemp("winmap") / "winmap_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "winmap_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    return [int(v) for v in out.stdout.split()[1:4]]


def test_compact_window_map_against_brute_force(counts):
    assert counts[0] >= 30


def test_classic_window_map_against_brute_force(counts):
    # 30 x 30 grids x (2 + 3 + 7 + 12) (ws, shift) pairs x 2 batch sizes
    assert counts[1] == 30 * 30 * 24 * 2


def test_map_validity_check_matches_the_entry_points_it_replaced(counts):
    assert counts[2] > 20000
