"""A numpy model of Pillow's 8-bit BILINEAR `Image.resize` (Resample.c), written from its definition with plain loops -- its own
coefficient code, nothing shared with divergen_amd/data/resize_tables.py.  tests/test_host_device_resize.py holds it to the installed
Pillow byte for byte; the GPU tests and the key-on / key-off tests then use either as the expected value.

    coefficients (float64 = C double), per axis in -> out:  scale = in / out, fs = max(scale, 1), support = fs, ksize = 2 ceil(support) + 1;
        per output xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in),
        w[x] = max(0, 1 - |(x + xmin - center + 0.5) * (1 / fs)|) (Resample.c multiplies by the reciprocal) normalised by their sum,
        added in order, k[x] = int(0.5 + w[x] 2^22)
    one pass: clamp((2^21 + sum src[xmin + x] k[x]) >> 22, 0, 255); horizontal first, rounded to bytes, then vertical; a pass whose size
        does not change is skipped; RGBA premultiplies before and un-premultiplies after unless both sizes are unchanged (a copy)."""
import math

import numpy as np


def coefficients(in_size, out_size):
    """-> (bounds [(xmin, n)], k [[int]]) for every output of the axis."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    bounds, ks = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = []
        for x in range(xmax - xmin):
            v = abs((x + xmin - center + 0.5) * (1.0 / fs))
            w.append(1.0 - v if v < 1.0 else 0.0)
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds.append((xmin, xmax - xmin))
        ks.append([int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w])
    assert max(len(k) for k in ks) <= 2 * math.ceil(support) + 1
    return bounds, ks


def _pass(img, out_size, axis):
    """One resample pass of an (h, w, c) uint8 array along `axis` (0 vertical, 1 horizontal)."""
    if img.shape[axis] == out_size:
        return img
    bounds, ks = coefficients(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for xx, ((xmin, n), k) in enumerate(zip(bounds, ks)):
        acc = (1 << 21) + np.tensordot(np.asarray(k, dtype=np.int64), src[xmin:xmin + n], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31              # Pillow accumulates in int
        out[xx] = np.clip(acc >> 22, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def premultiply(rgba):
    a = rgba[..., 3:].astype(np.int64)
    t = rgba[..., :3].astype(np.int64) * a + 128
    return np.concatenate([((t >> 8) + t) >> 8, a], -1).astype(np.uint8)


def unpremultiply(rgba):
    a = rgba[..., 3:].astype(np.int64)
    c = rgba[..., :3].astype(np.int64)
    d = np.minimum(255 * c // np.maximum(a, 1), 255)
    return np.concatenate([np.where((a == 0) | (a == 255), c, d), a], -1).astype(np.uint8)


def resize(img, out_h, out_w):
    """img (h, w, 3 | 4) uint8 -> (out_h, out_w, c): Image.fromarray(img, 'RGB' | 'RGBA').resize((out_w, out_h), Image.BILINEAR)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.shape[:2] == (out_h, out_w):
        return img.copy()
    rgba = img.shape[2] == 4
    if rgba:
        img = premultiply(img)
    out = _pass(_pass(img, out_w, 1), out_h, 0)
    return unpremultiply(out) if rgba else out


def job_result(src, out_hw, crop_yx, crop_hw, flip):
    """The window of one resize job as (ch, cw, c): resize, crop, mirror."""
    r = resize(src, out_hw[0], out_hw[1])[crop_yx[0]:crop_yx[0] + crop_hw[0], crop_yx[1]:crop_yx[1] + crop_hw[1]]
    return np.ascontiguousarray(r[:, ::-1] if flip else r)


def apply_tables(src, table_row, tab):
    """One row of a shipped job table (13 int32 words) and its coefficient words applied to the shipped source bytes with the kernel's
    arithmetic -> the window as (ch, cw, c) before it is laid out (mirror applied).  Reads what the worker SHIPPED, not what the model
    would compute: the key-on tests hold this to the key-off bytes."""
    so, sh, sw, C, ch, cw, flags, _, ho, hks, vo, vks, _ = (int(v) for v in table_row)
    img = src[so:so + sh * sw * C].reshape(sh, sw, C)
    if flags & 4:
        img = premultiply(img)
    img = img.astype(np.int64)
    hb, hk = tab[ho:ho + 2 * cw].reshape(cw, 2), tab[ho + 2 * cw:ho + 2 * cw + cw * hks].reshape(cw, hks).astype(np.int64)
    vb, vk = tab[vo:vo + 2 * ch].reshape(ch, 2), tab[vo + 2 * ch:vo + 2 * ch + ch * vks].reshape(ch, vks).astype(np.int64)
    mid = np.empty((sh, cw, C), dtype=np.int64)
    for x in range(cw):
        s, n = int(hb[x, 0]), int(hb[x, 1])
        mid[:, x] = np.clip(((1 << 21) + np.tensordot(img[:, s:s + n], hk[x, :n], axes=(1, 0))) >> 22, 0, 255)
    out = np.empty((ch, cw, C), dtype=np.uint8)
    for y in range(ch):
        s, n = int(vb[y, 0]), int(vb[y, 1])
        out[y] = np.clip(((1 << 21) + np.tensordot(vk[y, :n], mid[s:s + n], axes=(0, 0))) >> 22, 0, 255)
    if flags & 4:
        out = unpremultiply(out)
    return np.ascontiguousarray(out[:, ::-1] if flags & 1 else out)
