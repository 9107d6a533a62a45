"""Checks and threshold parsers of the seafloor detectors (reference: echopype mask/seafloor_detection/utils.py), and
the device planes they run on.

``_check_inputs`` raises what the reference raises, in its order.  Its depth-grid decision ("max over range of
|depth - depth[ping 0]| < 1e-16 for every ping", NaN skipped, a ping without a finite difference failing) is made by
one kernel over the selected channel's depth (epa_seafloor_depth_uniform); the host reads its flag together with the
ping-0 depth row, in one copy.  A lazy ``depth`` (``consolidate.add_depth`` on a lazy echo_range) is materialised
for this: 8 B per sample of every channel written once, kept with the dataset as it is for any other reader."""
import numpy as np
import torch

from ... import ops
from ...device_view import channel_position, device_view, resolve_device

_DIMS = ("channel", "ping_time", "range_sample")


def _to_host(t):
    """The one place the detectors copy device data to the host (a synchronisation: the tests count them)."""
    return t.cpu()


def _channel_plane(da, ci, dev, name):
    """One channel of a (channel, ping_time, range_sample) variable as a contiguous (P, S) float32 / float64 device
    tensor: device arrays are sliced where they are (a lazy array is materialised), host arrays uploaded."""
    if set(da.dims) != set(_DIMS) or len(da.dims) != 3:
        raise ValueError(f"{name!r} must have the dimensions {_DIMS}, got {tuple(da.dims)}")
    return device_view(da, _DIMS, device=dev, index=ci, floating=True)


def _check_inputs(ds, var_name, channel, required_vars=None, device=None):
    """Validate dataset and select the reference channel for bottom detection -> (Sv (P, S) device plane, depth (P, S)
    device plane, depth at ping 0 as a host array of depth's dtype)."""
    if var_name not in ds:
        raise KeyError(f"{var_name!r} not found in dataset")
    if "depth" not in ds:
        raise KeyError("'depth' variable not found in dataset")
    if "channel" not in ds.coords:
        raise ValueError("Dataset must have 'channel' coordinate")

    required_vars = required_vars or []
    for var in required_vars:
        if var not in ds:
            raise KeyError(f"Required variable {var!r} not found in dataset")

    ci = channel_position(ds["channel"].values, channel)
    dev = resolve_device(device)
    sv = _channel_plane(ds[var_name], ci, dev, var_name)
    depth = _channel_plane(ds["depth"], ci, dev, "depth")
    if depth.shape[0] == 0:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    bad = ops.seafloor_depth_uniform(depth)
    host = _to_host(torch.cat([bad.double(), depth[0].double()])).numpy()
    if host[0] != 0:
        raise ValueError("Depth grid varies across ping_time for the selected channel.")
    depth_ref = host[1:].astype(np.float32 if depth.dtype == torch.float32 else np.float64)
    return sv, depth, depth_ref


def _validate_threshold(threshold):
    """Ensure threshold is a valid tuple (tmin, tmax)."""
    if isinstance(threshold, (int, float)):
        tmin, tmax = float(threshold), float(threshold) + 10.0
    else:
        tmin, tmax = map(float, threshold)
        if tmax <= tmin:
            raise ValueError("threshold upper bound must be > lower bound")
    return tmin, tmax


def _parse_blackwell_thresholds(threshold):
    """Parse threshold for Blackwell detection -> (tSv, ttheta, tphi): Sv (dB), angle_major, angle_minor."""
    if isinstance(threshold, (list, tuple)):
        if len(threshold) == 3:
            tSv, ttheta, tphi = threshold
        elif len(threshold) == 2:
            tSv, ttheta, tphi = threshold[0], 702, 282
        else:
            raise ValueError("`threshold` must have 1, 2, or 3 values")
    elif isinstance(threshold, (int, float)):
        tSv, ttheta, tphi = threshold, 702, 282
    else:
        raise TypeError("`threshold` must be float or tuple/list of 1–3 floats")

    return float(tSv), float(ttheta), float(tphi)
