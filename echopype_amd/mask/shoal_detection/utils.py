"""What the two shoal detectors share: the (ping_time, range_sample) device plane of the selected variable, the
error-word read-back, and the result container."""
import numpy as np

from ...device_view import channel_position, device_view
from ...xr_lite import DataArray, DeviceArray

_CORE = ("ping_time", "range_sample")


def _to_host(t):
    """The one place the detectors copy device data to the host (a synchronisation: the tests count them)."""
    return t.cpu()


def _channel_plane(var, channel, device, var_name):
    """The selected channel of ``var`` (``var.sel(channel=channel)``) as a contiguous (ping_time, range_sample)
    float32 / float64 device tensor.  A variable without a channel dimension is the plane itself.  Device arrays are
    sliced where they are, host arrays uploaded."""
    dims = list(var.dims)
    ci = None
    if "channel" in dims:
        labels = var.coords["channel"] if "channel" in var.coords else np.arange(var.shape[dims.index("channel")])
        ci = channel_position(labels, channel)
    rest = [d for d in dims if d != "channel"]
    if set(rest) != set(_CORE):
        raise ValueError(f"{var_name!r}: one (ping_time, range_sample) plane expected after the channel selection, got "
                         f"dimensions {tuple(rest)}")
    return device_view(var, ("channel",) + _CORE, device=device, index=ci, floating=True)


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
