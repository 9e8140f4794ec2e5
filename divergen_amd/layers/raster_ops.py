"""Ground-truth polygon fill on the GPU (INPUT.DEVICE_RASTER): the (N, H, W) byte masks of one sample from the sorted crossing lists
of its polygons, through libdgx's dgx_polygons_to_bitmask (csrc/polygon_raster.hip) -- byte for byte what
data/build.py:polygons_to_bitmask fills on the host.  No torch fallback: a missing extension raises in `_lib.lib()`."""
import numpy as np
import torch

from .. import _lib as L


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise L.DgxError("libdgx ops need GPU (ROCm) tensors; got a %s tensor -- no CPU fallback exists" % t.device)


def _typed(t, dtype, what):
    if t.dtype != dtype:
        raise L.DgxError("%s must be %s, got %s" % (what, dtype, t.dtype))
    return t.contiguous()


def _host_offsets(off, what):
    """Offsets as a contiguous host int64 array (numpy array or CPU tensor in, never a device tensor: they are validated on the host)."""
    if torch.is_tensor(off):
        if off.is_cuda:
            raise L.DgxError("%s: the offsets to validate are host arrays, got a %s tensor" % (what, off.device))
        off = off.numpy()
    off = np.asarray(off)
    if off.dtype != np.int64 or off.ndim != 1 or off.size < 1:
        raise L.DgxError("%s must be a 1-d int64 array of at least one entry, got %s %s" % (what, off.dtype, off.shape))
    return np.ascontiguousarray(off)


def _offsets_ok(off, last):
    return int(off[0]) == 0 and int(off[-1]) == int(last) and bool((off[1:] >= off[:-1]).all())


def polygons_to_bitmask(pos, poly_off, inst_off, H, W, out=None, poly_off_dev=None, inst_off_dev=None):
    """pos int32 (n_pos) on the device: per polygon the sorted column-major crossing positions (< H * W); poly_off int64 (P + 1) and
    inst_off int64 (N + 1) on the HOST -> uint8 (N, H, W) of 0 / 1 on pos's device, ONE launch on the current stream; every byte of
    `out` (a fresh tensor unless given) is written.  The offsets are held to the sizes of what they index -- start at 0, never decrease,
    inst_off ends at P, poly_off ends at n_pos -- before the kernel indexes with them; it reads their device copies (poly_off_dev /
    inst_off_dev, e.g. views of the uploaded sample blob; uploaded here when not given)."""
    _need_gpu(pos, out, poly_off_dev, inst_off_dev)
    pos = _typed(pos, torch.int32, "pos").reshape(-1)
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise L.DgxError("polygons_to_bitmask: a canvas of %d x %d (flat positions are int32: H * W < 2^31)" % (H, W))
    poly_off, inst_off = _host_offsets(poly_off, "poly_off"), _host_offsets(inst_off, "inst_off")
    N, P, n_pos = inst_off.size - 1, poly_off.size - 1, int(pos.numel())
    if not _offsets_ok(inst_off, P) or not _offsets_ok(poly_off, n_pos):
        raise L.DgxError("polygons_to_bitmask: inst_off spans [%d, %d] over %d polygons, poly_off spans [%d, %d] over %d crossings, "
                         "or one of them decreases" % (inst_off[0], inst_off[-1], P, poly_off[0], poly_off[-1], n_pos))
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.uint8, device=pos.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W):
        raise L.DgxError("polygons_to_bitmask: out must be uint8 %s, got %s %s" % ((N, H, W), out.dtype, tuple(out.shape)))
    if N == 0:
        return out
    devs = []
    for given, host, what in ((poly_off_dev, poly_off, "poly_off_dev"), (inst_off_dev, inst_off, "inst_off_dev")):
        if given is None:
            given = torch.from_numpy(host).to(pos.device)
        given = _typed(given, torch.int64, what).reshape(-1)
        if given.numel() != host.size:
            raise L.DgxError("%s has %d entries, the host offsets %d" % (what, given.numel(), host.size))
        devs.append(given)
    L.check(L.lib().dgx_polygons_to_bitmask(L.ptr(pos) if n_pos else None, n_pos, L.ptr(devs[0]), L.ptr(devs[1]), poly_off.ctypes.data,
                                            inst_off.ctypes.data, N, P, H, W, L.ptr(out), L.stream()), "dgx_polygons_to_bitmask")
    return out
