"""Where a dataset variable crosses to the device: every public entry point turns its ``DataArray`` (host NumPy data,
or a ``DeviceArray`` / ``LazyDeviceArray`` already in HBM) into a contiguous device tensor through these helpers.
Dimension checks and their error messages stay with the callers."""
import numpy as np
import torch

from . import ops
from .xr_lite import DataArray, DeviceArray

_FLOAT_T = (torch.float32, torch.float64)
_FLOAT_NP = (np.float32, np.float64)


def resolve_device(device):
    """``device`` as a ``torch.device``; None: the current CUDA device."""
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def as_tensor(a, dtype=None, device=None):
    """The data of ``a`` (a DataArray, a DeviceArray or host data) as a device tensor in the order it is stored in: a
    DeviceArray's own tensor where dtype and device already fit, host data uploaded."""
    data = a.data if isinstance(a, DataArray) else a
    if isinstance(data, DeviceArray):
        t = data.tensor
        if device is not None and t.device != device:
            t = t.to(device)
        return t if dtype is None or t.dtype == dtype else t.to(dtype)
    return ops.to_device(np.asarray(data), dtype=dtype, device=device)


def device_view(var, order, *, device=None, index=None, dtype=None, floating=False):
    """The data of ``var`` as a contiguous device tensor, its dimensions in the sequence in which they occur in
    ``order`` (those ``var`` lacks are skipped).  ``index``: an int selects that position along the leading axis and
    drops the axis, a list gathers those positions and keeps it.  ``floating``: anything but float32 / float64 becomes
    float64; ``dtype`` forces one.  A device array is worked on where it lives (read once: a lazy array is materialised
    once; moved only from another device, copied only if the result is not contiguous as it is), host data in NumPy
    and uploaded once.  The selection comes before the conversions: one plane is converted, not the cube."""
    dims = list(var.dims)
    perm = [dims.index(d) for d in order if d in dims]
    dev = resolve_device(device)
    d = var.data
    if isinstance(d, DeviceArray):
        t = d.tensor
        if t.device != dev:
            t = t.to(dev)
        t = t.permute(perm)
        if isinstance(index, (int, np.integer)):
            t = t[index]
        elif index is not None:
            t = t.index_select(0, torch.as_tensor(index, device=t.device))
        if floating and t.dtype not in _FLOAT_T:
            t = t.double()
        if dtype is not None:
            t = t.to(dtype)
        return t.contiguous()
    a = np.asarray(d).transpose(perm)
    if index is not None:
        a = a[index]
    if floating and a.dtype not in _FLOAT_NP:
        a = a.astype(np.float64)
    return ops.to_device(a, dtype=dtype, device=dev)


def strided_view(var, order, device=None):
    """The data of ``var`` as a float32 / float64 device tensor with one axis per dimension of ``order``, for a kernel
    that reads it through its strides: the array where it lies (a device array is neither moved nor copied, host data
    are uploaded once; anything but float32 / float64 becomes float64), its dimensions permuted into the sequence of
    ``order`` (a view), an axis of length 1 for every dimension ``var`` lacks.  Nothing is expanded."""
    dims = tuple(var.dims)
    d = var.data
    if isinstance(d, DeviceArray):
        t = d.tensor
    else:
        a = np.asarray(d)
        t = ops.to_device(a if a.dtype in _FLOAT_NP else a.astype(np.float64), device=device).reshape(a.shape)
    if t.dtype not in _FLOAT_T:
        t = t.double()
    t = t.permute([dims.index(x) for x in order if x in dims])
    for i, x in enumerate(order):
        if x not in dims:
            t = t.unsqueeze(i)
    return t


def channel_position(labels, channel):
    """Position of ``channel`` among the channel ``labels``, compared by their ``str()``: ``sel(channel=channel)``."""
    chans = [str(c) for c in np.asarray(getattr(labels, "values", labels)).reshape(-1)]
    if str(channel) not in chans:
        raise KeyError(channel)
    return chans.index(str(channel))


def broadcast_to_dims(da, ds, order):
    """Broadcast a variable to the (dim_0, ping_time, range_sample) cube if it is lower-dimensional."""
    if tuple(da.dims) == tuple(order):
        return da
    a = np.asarray(da.values)
    shape = [ds.sizes[d] for d in order]
    idx = [slice(None) if d in da.dims else None for d in order]
    src = np.transpose(a, [da.dims.index(d) for d in order if d in da.dims])
    return DataArray(np.ascontiguousarray(np.broadcast_to(src[tuple(idx)], shape)), order)
