"""What the two shoal detectors share: the (ping_time, range_sample) device plane of the selected variable, the
error-word read-back, and the result container."""
import numpy as np
import torch

from ... import ops
from ...xr_lite import DataArray, DeviceArray

_CORE = ("ping_time", "range_sample")


def _to_host(t):
    """The one place the detectors copy device data to the host (a synchronisation: the tests count them)."""
    return t.cpu()


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _select_channel(var, channel):
    """-> (the variable's dimensions without ``channel``, index along it or None): ``var.sel(channel=channel)``."""
    dims = list(var.dims)
    if "channel" not in dims:
        return dims, None
    labels = var.coords["channel"] if "channel" in var.coords else np.arange(var.shape[dims.index("channel")])
    chans = [str(c) for c in np.asarray(getattr(labels, "values", labels)).reshape(-1)]
    if str(channel) not in chans:
        raise KeyError(channel)
    return [d for d in dims if d != "channel"], chans.index(str(channel))


def _plane(var, channel, device, var_name):
    """The selected channel of ``var`` as a contiguous (ping_time, range_sample) float32 / float64 device tensor.  A
    variable without a channel dimension is the plane itself.  Device arrays are sliced where they are, host arrays
    uploaded."""
    rest, ci = _select_channel(var, channel)
    if set(rest) != set(_CORE):
        raise ValueError(f"{var_name!r}: one (ping_time, range_sample) plane expected after the channel selection, got "
                         f"dimensions {tuple(rest)}")
    dims = list(var.dims)
    perm = ([dims.index("channel")] if ci is not None else []) + [dims.index(d) for d in _CORE]
    dev = _device(device)
    d = var.data
    if isinstance(d, DeviceArray):
        t = d.tensor
        if t.device != dev:
            t = t.to(dev)
        t = t.permute(*perm)
        if ci is not None:
            t = t[ci]
        if t.dtype not in (torch.float32, torch.float64):
            t = t.double()
        return t.contiguous()
    a = np.asarray(d).transpose(perm)
    if ci is not None:
        a = a[ci]
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return ops.to_device(np.ascontiguousarray(a), device=dev)


def _check_state(state, who):
    """Read the error word of a call (its one host synchronisation) and raise if a union-find loop hit its bound."""
    err = int(_to_host(state[:1])[0])
    if err:
        raise RuntimeError(f"{who}: {err} union-find loops reached their bound")


def _mask_array(ds, plane, name, attrs):
    return DataArray(
        DeviceArray(plane),
        _CORE,
        coords={"ping_time": np.asarray(ds["ping_time"].values), "range_sample": np.asarray(ds["range_sample"].values)},
        name=name,
        attrs=attrs,
    )
