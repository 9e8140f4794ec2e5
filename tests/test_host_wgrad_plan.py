"""CPU: divergen_amd/csrc/wgrad_plan.h (which form runs a group of weight gradients, how the split form cuts its rows into slabs, the
reduce it needs and the workspace every entry point reports) compiled for the host and checked without a GPU:

* tests/golden/wgrad_plans.json -- what the host-only entry points of the library answered BEFORE the header existed (the planner then
  written out in wgrad256.hip and wgrad_lw.hip), for the shapes of the weight-gradient tests, the groups the layers form and a sweep of
  small sizes, the grouped form at wgrad_lw 0 / 1 / 2 -- is reproduced row by row.  The `single` rows are the exception by design:
  dgx_wgrad_workspace_bytes answered for the retired 128 x 128 kernel and now reports the size of a one-problem group;
* the full plans of WGRAD_ROWS, LINEAR_WGRAD_ROWS and MULTI_LEVELS equal their restatements in tests/_conv_ref64.py (wgrad_plan, wgrad_group_plan,
  wgrad_multi_plan, wgrad_workspace_floats), which the GPU numerics tests keep using;
* the invariants of every plan over a sweep (tests/native/wgrad_plan_check.cpp): every row in exactly one slab, no slab straddles an
  image, one round of workgroups or R >= max M, disjoint workspace regions inside the reported size, increasing reduce offsets,
  8 * per_xcd covers the total, and the split form's workspace for every group that may fall back to it."""
import json
import os
import shutil
import subprocess

import pytest

import _conv_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCE = {0: "direct", 1: "lpq1", 16: "lpq16"}


def _cases():
    with open(os.path.join(ROOT, "tests", "golden", "wgrad_plans.json")) as f:
        rows = json.load(f)["rows"]
    assert len(rows) >= 300
    lines = []
    for r in rows:
        if r["kind"] == "group":
            lines.append("group %d %s %s %s" % (len(r["probs"]), " ".join("%d %d %d %d" % tuple(p) for p in r["probs"]),
                                                " ".join(map(str, r["form"])), " ".join(map(str, r["ws"]))))
        elif r["kind"] == "single":
            lines.append("single %d %d %d" % (r["M"], r["Nn"], r["Kk"]))
        elif r["kind"] == "conv":
            lines.append("conv %d %d %d %d %d %d %d" % (r["N"], r["H"], r["W"], r["Cin"], r["Cout"], r["ws"], r["ws_bias"]))
        else:
            lines.append("multi %d %s %d %d %d" % (len(r["levels"]), " ".join("%d %d %d" % tuple(v) for v in r["levels"]), r["Cin"], r["Cout"], r["ws"]))
    kinds = {k: sum(r["kind"] == k for r in rows) for k in ("group", "single", "conv", "multi")}
    assert all(v >= 10 for v in kinds.values()), kinds
    return lines


def _plan_lines():
    """(request line, expected printed line) from the restatements of tests/_conv_ref64.py"""
    out = []
    for (N, H, W, Cin, Cout), row in R.WGRAD_ROWS.items():
        S, slab, stages, form = R.wgrad_plan(N, H, W, Cin, Cout)
        assert (S, stages, form) == row
        out.append(("planconv %d %d %d %d %d" % (N, H, W, Cin, Cout),
                    "planconv %d %d %d %s %d" % (S, slab, stages, form, R.wgrad_workspace_floats(S, Cin, Cout))))
    for shapes, row in R.LINEAR_WGRAD_ROWS.items():
        S, slab, form = R.wgrad_group_plan(shapes)
        assert (S, slab[-1] // 32, form) == row, (shapes, S, slab, form)
        out.append(("plangroup %d %s" % (len(shapes), " ".join("%d %d %d" % v for v in shapes)),
                    "plangroup %s %s" % (form, " ".join("%d %d" % v for v in zip(S, slab)))))
    for levels in (R.MULTI_LEVELS, R.WGRAD_MULTI_LEVELS):
        for Cin, Cout in R.MULTI_WIDTHS + R.WGRAD_MULTI_WIDTHS:
            for n in range(2, len(levels) + 1):
                Rr, nsl = R.wgrad_multi_plan(levels[:n], Cin, Cout)
                out.append(("planmulti %d %s %d %d" % (n, " ".join("%d %d %d" % v for v in levels[:n]), Cin, Cout),
                            "planmulti %d %s %d" % (Rr, " ".join(map(str, nsl)), R.wgrad_workspace_floats(sum(nsl), Cin, Cout))))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_wgrad_plan_golden_rows_restatements_and_invariants(tmp_path):
    exe, cases = str(tmp_path / "wgrad_plan_check"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "wgrad_plan_check.cpp")])
    lines, plans = _cases(), _plan_lines()
    with open(cases, "w") as f:
        f.write("\n".join(lines + [p[0] for p in plans]) + "\n")
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    got = out.stdout.strip().split("\n")
    assert out.returncode == 0 and got[-1].startswith("ok "), out.stdout[-2000:] + out.stderr
    assert int(got[-1].split()[1]) == len(lines) + len(plans) and int(got[-1].split()[2]) >= 40000
    printed = got[:-1]
    assert len(printed) == len(plans)
    for (req, want), line in zip(plans, printed):
        f = line.split()
        if f[0] == "planconv":
            f[4] = REDUCE[int(f[4])]
        if f[0] == "plangroup":
            f[1] = REDUCE[int(f[1])]
        assert " ".join(f) == want, (req, line, want)
