"""mask.detect_shoal(method="echoview") (reference: echopype mask/shoal_detection/shoal_echoview.py, after the
school detection of Echoview: candidates, linking, minimum school size)."""
import numpy as np

from ... import ops
from ...xr_lite import xarray_io
from .utils import _channel_plane, _check_state, _mask_array


def _axis(a, name, need):
    """``idim`` / ``jdim`` as the f64 host vector the device searches: nondecreasing and finite, ``need`` entries at
    least."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    if a.size < need:
        raise IndexError(f"{name} has {a.size} entries: one more than the plane's extent ({need}) needed")
    if not np.all(np.isfinite(a)):
        raise NotImplementedError(f"{name} with infinite entries is not supported")
    if np.any(np.diff(a) < 0):
        raise NotImplementedError(f"{name} must be nondecreasing: the nearest-entry search on the device is a binary one")
    return a


@xarray_io()
def shoal_echoview(ds, var_name, channel, idim, jdim, thr=-70.0, mincan=(3.0, 10.0), maxlink=(3.0, 15.0),
                   minsho=(3.0, 15.0), *, device=None):
    """Echoview-style shoal mask of one channel: candidates, linking, minimum shoal size.

    ``idim`` (range_sample edges, one more entry than samples) and ``jdim`` (ping edges, one more than pings) give the
    plane its units; heights are differences of ``idim``, widths of ``jdim``, taken in float64.

    1. Candidates: the 8-connected components of ``Sv > thr`` (compared in float64, as the reference's masked-array comparison does; NaN is
       background).  A component spanning samples i0..i1 and pings j0..j1 is ``idim[i1 + 1] - idim[i0]`` high and
       ``jdim[j1 + 1] - jdim[j0]`` wide; those below ``mincan`` (height, width) are removed.
    2. Linking: around every remaining component the box from the ``idim`` entry nearest ``idim[i0] - (maxlink[0] + 1)``
       to the one nearest ``idim[i1] + (maxlink[0] + 1)`` (and likewise along pings with ``maxlink[1]``) is searched;
       all remaining components with a pixel inside it become one shoal, transitively.
    3. Shoals whose united bounding box is below ``minsho`` are removed.  A component no search box met (its own
       included: possible with a negative ``maxlink`` or repeated edge values) is kept whatever its size.

    ``idim`` / ``jdim`` must be nondecreasing and finite (NotImplementedError otherwise: the nearest entry is found by
    binary search, resolved to the first index of the smallest float64 distance as ``argmin`` does).  ``Sv`` may be
    (channel, ping_time, range_sample) or a plane without a channel dimension; float32 or float64, on the device or the
    host.  Returns the boolean ``shoal_mask`` (ping_time, range_sample); its data stays on the device (a ``torch.bool``
    tensor) and goes straight into ``mask.apply_mask``.

    Host synchronisations: one, the union-find error word at the end.  Scratch on the device: 8 B (component codes) per
    pixel and 24 B per table entry, one entry per four pixels."""
    if var_name not in ds:
        raise ValueError(f"Variable '{var_name}' not found in dataset")
    var = ds[var_name]
    if "channel" in var.dims and channel is None:
        raise ValueError("Please specify channel for multi-channel data")
    if np.isnan(idim).any() or np.isnan(jdim).any():
        raise ValueError("idim and jdim must not contain NaN")
    sv = _channel_plane(var, channel, device, var_name)

    P, S = sv.shape
    if P == 0 or S == 0:
        plane = sv.new_zeros((P, S), dtype=bool)
    else:
        idim_h, jdim_h = _axis(idim, "idim", S + 1), _axis(jdim, "jdim", P + 1)
        sizes = [tuple(float(x) for x in v) for v in (mincan, maxlink, minsho)]
        if any(x != x for x in sizes[1]):
            raise ValueError("All-NaN slice encountered")  # what the nearest-entry search makes of a NaN distance
        plane = ops.shoal_threshold_fill(sv, float(thr))
        state = ops.shoal_state(sv.device)
        parent, table = ops.shoal_label(plane, 8, state, with_groups=True)
        ops.shoal_echoview_link(plane, parent, table, ops.to_device(idim_h, device=sv.device),
                                ops.to_device(jdim_h, device=sv.device), *sizes, state)
        _check_state(state, "shoal_echoview")

    return _mask_array(ds, plane, "shoal_mask",
                       {"description": f"Shoal mask using Echoview algorithm on {var_name}"})
