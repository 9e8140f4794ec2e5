"""Pillow-exact 8-bit bilinear resize on the GPU (INPUT.DEVICE_RESIZE): a table of jobs through libdgx's dgx_resize_bilinear_u8
(csrc/resize_u8.hip) in ONE launch -- byte for byte `Image.resize(..., Image.BILINEAR)` restricted to each job's crop window.  The
tables are built on the host (data/resize_tables.py).  No torch fallback: a missing extension raises in `_lib.lib()`."""
import numpy as np
import torch

from .. import _lib as L
from ..data.resize_tables import JOB_WORDS


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise L.DgxError("libdgx ops need GPU (ROCm) tensors; got a %s tensor -- no CPU fallback exists" % t.device)


def _host_i32(a, what, shape):
    """A host int32 array to validate (numpy array or CPU tensor in, never a device tensor)."""
    if torch.is_tensor(a):
        if a.is_cuda:
            raise L.DgxError("%s: the table to validate is a host array, got a %s tensor" % (what, a.device))
        a = a.numpy()
    a = np.asarray(a)
    if a.dtype != np.int32:
        raise L.DgxError("%s must be int32, got %s" % (what, a.dtype))
    try:
        return np.ascontiguousarray(a).reshape(shape)
    except ValueError:
        raise L.DgxError("%s has %d entries, not a multiple of %s" % (what, a.size, shape))


def _dev(t, dtype, what, n=None):
    if t.dtype != dtype:
        raise L.DgxError("%s must be %s, got %s" % (what, dtype, t.dtype))
    t = t.contiguous().reshape(-1)
    if n is not None and t.numel() != n:
        raise L.DgxError("%s has %d entries on the device, the host copy %d" % (what, t.numel(), n))
    return t


def resize_bilinear_u8(src, jobs, tab, image=None, flat=None, jobs_dev=None, tab_dev=None):
    """src uint8 on the device: the jobs' interleaved sources; jobs int32 (J, 13) and tab int32 on the HOST (resize_tables.assemble_jobs)
    -> ONE launch on the current stream that writes every job's window into `image` (planar jobs) or `flat` (interleaved RGBA jobs), both
    uint8 on src's device, and nothing else.  The host copies are validated against the sizes of src, image, flat and tab before the
    kernel indexes with them; a table that fails raises DgxError and nothing is launched.  The kernel reads the device copies
    (jobs_dev / tab_dev, e.g. views of the uploaded sample blob; uploaded here when not given)."""
    _need_gpu(src, image, flat, jobs_dev, tab_dev)
    jobs, tab = _host_i32(jobs, "jobs", (-1, JOB_WORDS)), _host_i32(tab, "tab", (-1,))
    J = jobs.shape[0]
    if J == 0:
        return
    src = _dev(src, torch.uint8, "src")
    bufs = []
    for t, what in ((image, "image"), (flat, "flat")):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous()):
            raise L.DgxError("%s must be a contiguous uint8 tensor, got %s" % (what, t.dtype))
        bufs.append((L.ptr(t), int(t.numel())) if t is not None else (None, 0))
    jobs_dev = _dev(torch.from_numpy(jobs).to(src.device) if jobs_dev is None else jobs_dev, torch.int32, "jobs_dev", jobs.size)
    tab_dev = _dev(torch.from_numpy(tab).to(src.device) if tab_dev is None else tab_dev, torch.int32, "tab_dev", tab.size)
    rc = L.lib().dgx_resize_bilinear_u8(L.ptr(src), int(src.numel()), L.ptr(jobs_dev), L.ptr(tab_dev), jobs.ctypes.data, tab.ctypes.data,
                                        J, int(tab.size), bufs[0][0], bufs[0][1], bufs[1][0], bufs[1][1], L.stream())
    if rc == -1:
        raise L.DgxError("dgx_resize_bilinear_u8: the job table does not fit its buffers (src %d bytes, image %d, flat %d, tab %d words): "
                         "a source, destination or coefficient range past its buffer, xmin + n past the source, a size < 1, or a "
                         "wrong tile0 -- nothing was launched" % (src.numel(), bufs[0][1], bufs[1][1], tab.size))
    L.check(rc, "dgx_resize_bilinear_u8")
