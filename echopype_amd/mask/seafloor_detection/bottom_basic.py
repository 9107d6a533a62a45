"""mask.detect_seafloor(method="basic") (reference: echopype mask/seafloor_detection/bottom_basic.py)."""
import numpy as np

from ... import ops
from ...xr_lite import DataArray, DeviceArray, xarray_io
from .utils import _check_inputs, _validate_threshold


@xarray_io()
def bottom_basic(ds, var_name, channel, threshold=-50.0, offset_m=0.5, bin_skip_from_surface=200, *, device=None):
    """Simple threshold-based seafloor detection returning a 1-D bottom line (depth).

    For the selected ``channel``, the first range sample at or after ``bin_skip_from_surface`` with
    ``tmin < Sv < tmax`` is found in every ping (one wave per ping scanning 64 samples per ballot:
    epa_seafloor_basic); the bottom is ``depth[ping 0][sample] - offset_m``.  A ping without such a sample gets the
    sample ``bin_skip_from_surface`` (the reference's argmax of an all-False row), not NaN.  A single ``threshold`` is
    ``(threshold, threshold + 10)``.  ``bin_skip_from_surface`` at or beyond the row length raises as the reference's
    empty argmax does.

    ``Sv`` and ``depth`` (channel, ping_time, range_sample), float32 or float64, on the device or the host.  Returns
    the f64 ``bottom_depth`` (ping_time) DataArray with the reference's attributes; its data stays on the device.
    Host synchronisation: one, the depth-grid check of ``_check_inputs`` (its flag and the ping-0 depth row)."""
    sv, depth, _ = _check_inputs(ds, var_name, channel, device=device)
    tmin, tmax = _validate_threshold(threshold)

    S = sv.shape[1]
    skip = int(bin_skip_from_surface)
    start = range(S)[slice(skip, None)]
    if len(start) == 0:
        raise ValueError("attempt to get argmax of an empty sequence")
    if skip < 0 and skip < -S:
        raise IndexError(f"index {skip} is out of bounds for axis 0 with size {S}")
    bottom = ops.seafloor_basic(sv, start.start, tmin, tmax, depth[0].double().contiguous(), float(offset_m))

    return DataArray(
        DeviceArray(bottom),
        ("ping_time",),
        coords={"ping_time": np.asarray(ds["ping_time"].values)},
        name="bottom_depth",
        attrs={
            "detector": "basic",
            "threshold_min": float(tmin),
            "threshold_max": float(tmax),
            "offset_m": float(offset_m),
            "bin_skip_from_surface": int(bin_skip_from_surface),
            "channel": str(channel),
        },
    )

