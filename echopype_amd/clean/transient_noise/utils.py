"""What the two transient-noise detectors share: the (channel, ping_time, range_sample) device cube of the selected
variable, the range rows on the host (the one device-to-host copy of a call), and the result container."""
import numpy as np

from ... import ops
from ...device_view import device_view
from ...xr_lite import DataArray, DeviceArray

_CPS = ("channel", "ping_time", "range_sample")
MEANING = "True = VALID (False = transient noise)"


def _to_host(t):
    """The one place the detectors copy device data to the host (a synchronisation: the tests count them).  The copy
    is ordered after the work already queued on the current stream -- the rows may have just been written -- so the host
    waits for that work and for the copy, not for anything queued later."""
    return ops.fetch_async(t).cpu()


def _channel_cube(var, var_name, device):
    """``var`` as a contiguous (C, P, S) float32 / float64 device tensor; a variable without a channel dimension is
    one channel.  Device arrays are read where they are, host arrays uploaded."""
    dims = list(var.dims)
    if not {"ping_time", "range_sample"}.issubset(dims) or not set(dims).issubset(_CPS):
        raise NotImplementedError(f"{var_name!r} must have dims (channel, ping_time, range_sample) in some order, "
                                  f"got {tuple(dims)}")
    t = device_view(var, _CPS, device=device, floating=True)
    return t if "channel" in dims else t[None]


def _range_rows(r_da, range_var, ping_dim, C, S):
    """The first ping's row of the range variable per channel (``isel(ping_time=0)``), or the 1-D ``range_sample``
    vector, as a host (C, S) array of the variable's own float type.  A device array is cut on the device and the
    C x S numbers copied: the one host synchronisation of a detector call."""
    dims = list(r_da.dims)
    d = r_da.data
    on_dev = isinstance(d, DeviceArray)
    a = d.tensor if on_dev else np.asarray(d)
    if ping_dim in dims:
        ax = dims.index(ping_dim)
        a = a.select(ax, 0) if on_dev else np.take(a, 0, axis=ax)
        dims.pop(ax)
    if on_dev:
        a = _to_host(a).numpy()
    if "range_sample" not in dims or not set(dims).issubset(("channel", "range_sample")):
        raise NotImplementedError(f"{range_var!r}: one range row per channel expected, got dimensions {tuple(dims)} "
                                  "after the first ping was taken")
    if dims == ["range_sample", "channel"]:
        a = a.T
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    if a.ndim == 1:
        a = np.broadcast_to(a, (C, a.shape[0]))
    if a.shape != (C, S):
        raise ValueError(f"{range_var!r}: range rows of shape {a.shape}, Sv has {C} channels x {S} samples")
    return np.ascontiguousarray(a)


def _mask_array(var, mask_cps, name):
    """bool (C, P, S) device tensor -> DataArray with the dims, order and coordinates of ``var``."""
    dims = list(var.dims)
    t = mask_cps if "channel" in dims else mask_cps[0]
    have = [d for d in _CPS if d in dims]
    t = t.permute(*[have.index(d) for d in dims])
    return DataArray(DeviceArray(t), tuple(dims), coords={d: np.asarray(var.coords[d]) for d in dims if d in var.coords},
                     name=name, attrs={"meaning": MEANING})
