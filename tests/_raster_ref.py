"""Test helper for INPUT.DEVICE_RASTER: a plain model of the fill rule dgx_polygons_to_bitmask implements, as include/divergen_hip.h
states it, and the seeded polygon set the host and GPU tests share.

The rule: pixel (y, x) of ONE polygon is set iff an odd number of that polygon's crossings lie at column-major flat positions
<= x * H + y (an inclusive prefix, taken in flat order: parity carries over column boundaries and an odd list leaves the rest of the
canvas set); an instance is the OR of its polygons.  tests/test_host_device_raster.py holds this model to the host rasteriser
(data/build.py:polygons_to_bitmask), so the rule the kernel is written from cannot drift from the code it must match."""
import numpy as np

CANVASES = ((5, 6), (37, 70), (64, 64))


def fill_model(crossings, H, W):
    """crossings: the polygons of one instance, each a sorted int array of flat positions < H * W  ->  (H, W) bool."""
    m = np.zeros((H, W), dtype=bool)
    for pos in crossings:
        count = np.zeros(H * W, dtype=np.int64)
        for p in pos:
            count[int(p)] += 1
        parity = (np.cumsum(count) & 1).astype(bool)          # inclusive prefix, flat (column-major) order
        m |= parity.reshape(W, H).T
    return m


def sorted_crossings(poly, H, W):
    """What the worker ships for one polygon: polygon_crossings, positions >= H * W dropped, ascending."""
    from divergen_amd.data.build import polygon_crossings
    pos = polygon_crossings([float(c) for c in poly], H, W)
    return np.sort(pos[pos < H * W]).astype(np.int32)


def _tags(poly, H, W):
    """The branches one polygon exercises (the tests assert that the set covers every one)."""
    xy = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
    x0, y0, x1, y1 = xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max()
    pos = sorted_crossings(poly, H, W)
    tags = set()
    if x1 < 0 or y1 < 0 or x0 > W or y0 > H:
        tags.add("outside")
    else:
        for name, hit in (("clip_left", x0 < 0 < x1), ("clip_top", y0 < 0 < y1), ("clip_right", x0 < W < x1), ("clip_bottom", y0 < H < y1)):
            if hit:
                tags.add(name)
    d = xy[1:] - xy[0]
    if len(xy) >= 3 and np.all(d[:, 0] * d[0, 1] == d[:, 1] * d[0, 0]):
        tags.add("collinear")
    if 0 < x1 - x0 < 1 and 0 < y1 - y0 < 1 and "collinear" not in tags:
        tags.add("subpixel")
    if pos.size & 1:
        tags.add("odd")
    if pos.size >= 2 and (np.diff(pos) == 0).any():
        tags.add("duplicate")
    # a crossing clipped to yd == H lands on the first position of the NEXT column; with the whole polygon below y = 1 no crossing
    # has yd == 0, so a position that is a multiple of H can only be such a clipped one
    if y0 >= 1 and pos.size and (pos % H == 0).any():
        tags.add("carry")
    return tags


def polygon_set():
    """[(H, W, polygon as a flat [x0, y0, x1, y1, ...] list, tags)], seeded: at least 2000 polygons over CANVASES -- random ones
    reaching past every border, and per canvas the deliberate cases (outside, collinear, sub-pixel, bottom clip, bottom-right corner)."""
    rng = np.random.default_rng(20240611)
    out = []

    def add(H, W, poly):
        poly = [float(v) for v in np.asarray(poly, dtype=np.float64).reshape(-1)]
        out.append((H, W, poly, _tags(poly, H, W)))

    for H, W in CANVASES:
        for _ in range(560):                               # anywhere, reaching past the borders
            k = int(rng.integers(3, 9))
            cx, cy = rng.uniform(-0.2 * W, 1.2 * W), rng.uniform(-0.2 * H, 1.2 * H)
            r = rng.uniform(0.3, 0.6 * max(H, W))
            add(H, W, np.stack([cx + r * rng.uniform(-1, 1, k), cy + r * rng.uniform(-1, 1, k)], 1).round(2))
        for _ in range(40):                                # fully outside
            k = int(rng.integers(3, 7))
            add(H, W, np.stack([W + 3 + rng.uniform(0, W, k), rng.uniform(-H, 2 * H, k)], 1).round(2))
        for _ in range(20):                                # zero area: points on one line
            k = int(rng.integers(3, 6))
            t = rng.integers(-2, 8, k).astype(np.float64)
            ax, ay, dx, dy = rng.integers(0, W), rng.integers(0, H), rng.integers(-3, 4), rng.integers(-3, 4)
            add(H, W, np.stack([ax + t * dx, ay + t * dy], 1))
        for _ in range(20):                                # smaller than a pixel
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            add(H, W, np.stack([cx + rng.uniform(0, 0.9, 3), cy + rng.uniform(0, 0.9, 3)], 1).round(3))
        for _ in range(20):                                # clipped at the bottom only: crossings at yd == H (the carry)
            xa = rng.uniform(0, W - 2)
            add(H, W, [xa, H - rng.uniform(1, 3), xa + rng.uniform(1, 0.5 * W), H - rng.uniform(1, 3), xa + rng.uniform(1, 0.5 * W),
                       H + rng.uniform(1, 4), xa, H + rng.uniform(1, 4)])
        for _ in range(40):                                # around the bottom-right corner: the last crossing may fall off the canvas
            k = int(rng.integers(3, 7))
            add(H, W, np.stack([W - 1 + rng.uniform(-3, 3, k), H - 1 + rng.uniform(-3, 3, k)], 1).round(2))
    return out
