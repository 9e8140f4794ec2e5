"""Hash every output buffer of the weight-gradient entry points, for comparing two builds of the library bit for bit:

    DGX_LIB=<library A> python tools/wgrad_hash.py a.txt ; DGX_LIB=<library B> python tools/wgrad_hash.py b.txt ; diff a.txt b.txt

One process per library.  Fixed seeds; every output-only buffer (gw and gb at beta 0, the workspace up to its reported size) is filled
with NaN beforehand, so a byte one build writes and the other does not shows.  One line per launch: the case and the SHA-256 of gw, gb
and the workspace.  Cases: the linear groups of tests/_conv_ref64.py (LINEAR_WGRAD_ROWS on the split form, LINEAR_WGRAD_LW on the forced
loader-wave form at reserved CUs 0 and 16), dgx_conv3x3_wgrad / _bias at every WGRAD_ROWS geometry, dgx_conv3x3_wgrad_bias_multi at
MULTI_LEVELS x MULTI_WIDTHS; beta 0 and 1, with and without gb.  dgx_linear_wgrad is left out (its summation order is the grouped
path's since the 128 x 128 kernel was retired)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _conv_ref64 as R  # noqa: E402
from divergen_amd import _lib as L  # noqa: E402

DEV, F32 = "cuda", torch.float32
NAN = float("nan")


def sha(*bufs):
    h = hashlib.sha256()
    for b in bufs:
        if b is not None:
            h.update(b.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:24]


def out_buf(n, src, beta):
    return src.reshape(-1).to(DEV).clone() if beta else torch.full((n,), NAN, dtype=F32, device=DEV)


def linear(lines):
    lib = L.lib()
    for form, groups in (("split", list(R.LINEAR_WGRAD_ROWS)), ("lw", R.LINEAR_WGRAD_LW)):
        for shapes in groups:
            gen = torch.Generator().manual_seed(31 + sum(M + Nn + Kk for M, Nn, Kk in shapes))
            ops = [(R.bf(torch.randn(M, Nn, generator=gen)).to(DEV), R.bf(torch.randn(M, Kk, generator=gen)).to(DEV),
                    torch.randn(Nn, Kk, generator=gen), torch.randn(Nn, generator=gen)) for M, Nn, Kk in shapes]
            for reserved in ((0, 16) if form == "lw" else (0,)):
                for beta in (0.0, 1.0):
                    for with_gb in (True, False):
                        assert lib.dgx_dev_set(b"wgrad_lw", 2 if form == "lw" else 0) == 0
                        lib.dgx_set_reserved_cus(reserved)
                        n = len(shapes)
                        arr = (L.WgradProblem * n)()
                        gws = [out_buf(Nn * Kk, o[2], beta) for (M, Nn, Kk), o in zip(shapes, ops)]
                        gbs = [out_buf(Nn, o[3], beta) if with_gb else None for (M, Nn, Kk), o in zip(shapes, ops)]
                        for i, ((M, Nn, Kk), o) in enumerate(zip(shapes, ops)):
                            arr[i].dy, arr[i].x, arr[i].gw, arr[i].gb = L.ptr(o[0]), L.ptr(o[1]), L.ptr(gws[i]), L.ptr(gbs[i])
                            arr[i].M, arr[i].Nn, arr[i].Kk = M, Nn, Kk
                        assert int(lib.dgx_wgrad_grouped_form(arr, n)) == (form == "lw")
                        nbytes = int(lib.dgx_wgrad_grouped_workspace_bytes(arr, n))
                        ws = torch.full((max(nbytes // 4, 4),), NAN, dtype=F32, device=DEV)
                        L.check(lib.dgx_linear_wgrad_grouped(arr, n, beta, L.ptr(ws), L.stream()), "dgx_linear_wgrad_grouped")
                        torch.cuda.synchronize()
                        lib.dgx_set_reserved_cus(0)
                        assert lib.dgx_dev_set(b"reset", 0) == 0
                        lines.append("linear %s %dx%s reserved%d beta%d gb%d ws%d  %s" % (form, n, shapes[0] if n == 1 or form == "lw" else shapes,
                                                                                       reserved, beta, with_gb, nbytes, sha(*gws, *gbs, ws)))


def conv(lines):
    lib = L.lib()
    for geom in R.WGRAD_ROWS:
        N, H, W, Cin, Cout = geom
        inp = R.make_inputs("ordinary", geom, R.seed_of(geom, "ordinary"))
        gp, xp = R.pad_layout(inp["dy"]).contiguous().to(DEV), R.pad_layout(inp["x"]).contiguous().to(DEV)
        for beta in (0.0, 1.0):
            for entry in ("bias", "bias.nogb", "plain"):
                gw = out_buf(Cout * 9 * Cin, inp["g0"][0], beta)
                gb = out_buf(Cout, inp["g0"][1], beta) if entry == "bias" else None
                size = lib.dgx_conv3x3_wgrad_workspace_bytes if entry == "plain" else lib.dgx_conv3x3_wgrad_bias_workspace_bytes
                nbytes = int(size(N, H, W, Cin, Cout))
                ws = torch.full((max(nbytes // 4, 4),), NAN, dtype=F32, device=DEV)
                if entry == "plain":
                    L.check(lib.dgx_conv3x3_wgrad(L.ptr(gp), L.ptr(xp), L.ptr(gw), N, H, W, Cin, Cout, beta, L.ptr(ws), L.stream()), "dgx_conv3x3_wgrad")
                else:
                    L.check(lib.dgx_conv3x3_wgrad_bias(L.ptr(gp), L.ptr(xp), L.ptr(gw), L.ptr(gb), N, H, W, Cin, Cout, beta, L.ptr(ws), L.stream()),
                            "dgx_conv3x3_wgrad_bias")
                torch.cuda.synchronize()
                lines.append("conv %s %s beta%d ws%d  %s" % (entry, geom, beta, nbytes, sha(gw, gb, ws)))


def multi(lines):
    lib = L.lib()
    for Cin, Cout in R.MULTI_WIDTHS:
        levels = R.MULTI_LEVELS
        inps = [R.make_inputs("ordinary", lv + (Cin, Cout), R.seed_of(lv + (Cin, Cout), "ordinary")) for lv in levels]
        gps = [R.pad_layout(i["dy"]).contiguous().to(DEV) for i in inps]
        xps = [R.pad_layout(i["x"]).contiguous().to(DEV) for i in inps]
        for n in range(1, len(levels) + 1):
            items = (L.ConvWgradItem * n)()
            for i in range(n):
                items[i].dypad, items[i].xpad = L.ptr(gps[i]), L.ptr(xps[i])
                items[i].N, items[i].H, items[i].W = levels[i]
            nbytes = int(lib.dgx_conv3x3_wgrad_bias_multi_workspace_bytes(items, n, Cin, Cout))
            for beta in (0.0, 1.0):
                for with_gb in (True, False):
                    gw = out_buf(Cout * 9 * Cin, inps[0]["g0"][0], beta)
                    gb = out_buf(Cout, inps[0]["g0"][1], beta) if with_gb else None
                    ws = torch.full((max(nbytes // 4, 4),), NAN, dtype=F32, device=DEV)
                    L.check(lib.dgx_conv3x3_wgrad_bias_multi(items, n, L.ptr(gw), L.ptr(gb), Cin, Cout, beta, L.ptr(ws), L.stream()), "multi")
                    torch.cuda.synchronize()
                    lines.append("multi %d levels (%d, %d) beta%d gb%d ws%d  %s" % (n, Cin, Cout, beta, with_gb, nbytes, sha(gw, gb, ws)))


def main():
    lines = []
    linear(lines)
    conv(lines)
    multi(lines)
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    print(text, end="")
    print("%d launches hashed from %s" % (len(lines), L.LIB_PATH))


if __name__ == "__main__":
    main()
