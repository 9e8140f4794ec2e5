"""Numpy / scipy restatement of the 'possion' blend (INPUT.CP_METHOD with INPUT.CP_POISSON; the reference's poisson_edit,
DG/divergen/data/transforms/possion_blending.py:27-64) as include/divergen_hip.h states it for dgx_poisson_blend: the REDUCED system
over U = F + image frame, float64, scipy's sparse LU, clamp, truncate.  Test helper: tests/test_host_poisson.py pins it on
tests/golden/poisson_blend.npz (the reference's own poisson_edit), tests/test_gpu_poisson.py checks the kernel against it.
The other modes come from tests/_blend_ref.py; masks, boxes, labels and instance_source from oracle.compositor."""
import numpy as np
import scipy.sparse
from scipy.sparse.linalg import spsolve

import _blend_ref as BR
from oracle import compositor as OK

DELTA = 1e-3          # the kernel's accuracy contract, grey levels before the clamp
MODES = {**BR.MODES, "possion": 3}


def unknowns(mask):
    """U of an (H, W) footprint: the footprint and the 1-pixel image frame."""
    u = mask.astype(bool).copy()
    u[0, :] = u[-1, :] = True
    u[:, 0] = u[:, -1] = True
    return u


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies inside, else fill."""
    H, W = a.shape
    b = np.full_like(a, fill)
    ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    b[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return b


NEIGHBOURS = ((0, -1), (0, 1), (-1, 0), (1, 0))


def solve(target, src, mask):
    """One 'possion' paste.  target u8 (3,H,W): the image the previous paste left; src u8 (3,H,W): the placed RGB (0 outside the
    rectangle); mask (H,W): placed alpha > 0.  Returns (image u8 (3,H,W), x float64 (3,H,W): the solution before the clamp, the
    target itself outside U, U bool (H,W))."""
    H, W = mask.shape
    assert H >= 3 and W >= 3
    m = mask.astype(bool)
    U = unknowns(m)
    idx = np.full((H, W), -1, np.int64)
    n = int(U.sum())
    idx[U] = np.arange(n)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [np.full(n, 4.0)]
    known = []                                  # per direction: (rows of U whose neighbour is a known pixel, that pixel's y, x)
    ys, xs = np.nonzero(U)
    for dy, dx in NEIGHBOURS:
        j = _shift(idx, dy, dx, -1)[U]          # unknown index of the neighbour, -1: known or outside the image
        inside = (ys + dy >= 0) & (ys + dy < H) & (xs + dx >= 0) & (xs + dx < W)
        has = j >= 0
        rows.append(np.flatnonzero(has)); cols.append(j[has]); vals.append(np.full(int(has.sum()), -1.0))
        kn = inside & ~has
        known.append((np.flatnonzero(kn), ys[kn] + dy, xs[kn] + dx))
    A = scipy.sparse.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    x_full = target.astype(np.float64)
    for c in range(3):
        S, T = src[c].astype(np.float64), target[c].astype(np.float64)
        lap = 4.0 * S
        for dy, dx in NEIGHBOURS:
            lap = lap - _shift(S, dy, dx, 0.0)
        b = np.where(m, lap, T)[U]
        for r, ky, kx in known:
            np.add.at(b, r, T[ky, kx])
        x_full[c][U] = spsolve(A, b)
    out = np.clip(x_full, 0.0, 255.0).astype(np.uint8)
    return out, x_full, U


def band(x, U):
    """Bytes of U (3 channels) whose truncation DELTA does not decide: frac(x) within DELTA of an integer, or x within DELTA of the
    clamp's ends.  Returns the bool (3,H,W) map."""
    fr = x - np.floor(x)
    amb = (fr <= DELTA) | (fr >= 1.0 - DELTA)
    amb &= (x > -DELTA) & (x < 255.0 + DELTA)       # beyond the clamp by more than DELTA the byte is decided (0 or 255)
    return amb & U[None]


def check_band(got, before, x, U, what=""):
    """The band rule: `got` u8 (3,H,W) against the restatement's solution x of the paste applied to `before`.  Outside U: equal to
    `before`.  In U outside the band: trunc(clamp(x)).  In the band: either adjacent value.  Returns the number of band bytes."""
    want = np.clip(x, 0.0, 255.0).astype(np.uint8)
    out = ~np.broadcast_to(U[None], got.shape)
    assert np.array_equal(got[out], before[out]), "%s: bytes outside U changed" % what
    amb = band(x, U)
    sure = np.broadcast_to(U[None], got.shape) & ~amb
    bad = np.argwhere(sure & (got != want))
    assert len(bad) == 0, "%s: %d bytes of U differ outside the band, first (c,y,x)=%s: %d vs %d (x* = %.6f)" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], x[tuple(bad[0])])
    lo = np.clip(np.floor(x - DELTA), 0.0, 255.0).astype(np.int64)
    hi = np.clip(np.floor(x + DELTA), 0.0, 255.0).astype(np.int64)
    g = got.astype(np.int64)
    assert ((g[amb] == lo[amb]) | (g[amb] == hi[amb])).all(), "%s: a band byte is neither adjacent value" % what
    return int(amb.sum())


def blend_chain(image, pastes, modes):
    """image u8 (3,H,W); pastes [(rgba (h,w,4), x0, y0, label)]; modes: names or codes 0..3.  Returns (the image after every paste,
    per paste None or (x, U) of a 'possion' step)."""
    H, W = image.shape[1:]
    out, steps, sols = image.copy(), [], []
    for (rgba, x0, y0, _), mode in zip(pastes, modes):
        mode = MODES.get(mode, mode) if isinstance(mode, str) else int(mode)
        placed, m = OK.place(np.asarray(rgba), int(x0), int(y0), H, W)
        if mode == 3:
            out, x, U = solve(out, placed[:3], m[0])
            sols.append((x, U))
        else:
            out = BR.blend(out, placed[:3], placed[3], mode)
            sols.append(None)
        steps.append(out)
    return steps, sols
