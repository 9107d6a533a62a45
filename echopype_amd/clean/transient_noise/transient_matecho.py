"""clean.detect_transient(method="matecho") (reference: echopype clean/transient_noise/transient_matecho.py, after
DeepSpikeDetection.m of Matecho, Perrot et al. 2018)."""
import numpy as np
import torch

from ... import ops
from ...device_view import device_view
from ...xr_lite import xarray_io
from .utils import _channel_cube, _mask_array, _range_rows


def _window_rows(r, start_depth, window_meter, range_var):
    """(s_lo, s_top, r[1] - r[0], r[-1]) of one range row: ``depth_mask`` by the reference's own expression, in the
    type NumPy compares in (a Python float against a float32 row is rounded to float32 first)."""
    depth_mask = (r >= start_depth) & (r <= start_depth + window_meter)
    fin = r[~np.isnan(r)]
    if fin.size > 1 and (np.diff(fin) < 0).any():
        raise NotImplementedError(f"range_var={range_var!r} must be nondecreasing along range_sample (NaN aside): the "
                                  "device search takes the window as one run of samples")
    idx = np.flatnonzero(depth_mask)
    if idx.size == 0:
        return 0, 0, 0.0, r[-1]
    s_lo, s_top = int(idx[0]), int(idx[-1]) + 1
    if idx.size != s_top - s_lo:
        raise NotImplementedError(f"range_var={range_var!r} has NaN between the samples of the window: the device search "
                                  "takes the window as one run of samples")
    return s_lo, s_top, r[1] - r[0], r[-1]


@xarray_io()
def transient_noise_matecho(ds, var_name="Sv", range_var="depth", time_var="ping_time", bottom_var=None,
                            start_depth=220, window_meter=450, window_ping=100, percentile=25, delta_db=12,
                            extend_ping=0, min_window=20, *, device=None):
    """Matecho's transient-noise mask: True = VALID (keep), False = transient noise; whole pings, all channels in one
    call.

    Per channel, with the range vector ``r`` = the first ping's row of ``range_var``, ``h = window_ping // 2`` and, for
    ping ``j``, the pings ``[j0, j1) = [max(0, j - h), min(P, j + h))``:

    1. the window samples are those with ``start_depth <= r <= start_depth + window_meter`` and ``r`` below the
       minimum of the bottom over ``[j0, j1)``; ``bottom_var`` names a ``(ping_time)`` or ``(channel, ping_time)``
       variable of ``ds`` (``mask.detect_seafloor``'s ``bottom_depth`` as it is); NaN entries, ``None`` or a name not in
       ``ds`` mean ``r[-1]``.  The ping is skipped when there is no such sample, when ``(r[1] - r[0]) * count`` is below
       ``min_window`` or when the window holds no value;
    2. it is flagged when the mean of its window samples (linear domain, NaN skipped, back in dB) exceeds the
       ``percentile`` of the window's dB values (``np.percentile``, NaN dropped) by more than ``delta_db``;
    3. flags are dilated by ``extend_ping`` pings on each side; a flagged ping is masked over its whole column.

    ``time_var`` must name the ping dimension of ``Sv``.  A ``percentile`` outside [0, 100] raises NumPy's
    ``ValueError`` before any launch; the reference raises it only if some ping gets as far as its percentile.  ``range_var`` must be nondecreasing along ``range_sample``
    (NaN aside), else ``NotImplementedError``.  ``Sv`` float32 or float64, on the device or the host; the arithmetic is
    float64, the comparison of ``r`` with the bottom too (as NumPy's against an ``np.float64`` scalar).  Returns the
    boolean ``matecho_mask_valid`` with the dims, order and coordinates of ``ds[var_name]``; its data stays on the
    device (a ``torch.bool`` tensor) and goes straight into ``mask.apply_mask``.

    Device work: a per-ping prologue (bottom minimum, last window sample by binary search), one workgroup per ping
    for the mean and one counting sweep of the window (the percentile itself is selected only when the decision needs
    it), the dilation and fill.  Host synchronisations: one, the copy of the C range rows from which the window rows
    are derived with the reference's own NumPy expressions (the copy waits for the work already queued on the stream); none when
    ``range_var`` is on the host."""
    if var_name not in ds:
        raise ValueError(f"{var_name!r} not found.")
    if range_var not in ds:
        raise ValueError(f"{range_var!r} not found.")
    var = ds[var_name]
    if time_var not in var.dims:
        raise ValueError(f"{time_var!r} must be a dim of {var_name!r}.")
    if time_var != "ping_time":
        raise NotImplementedError(f"time_var={time_var!r}: only the ping dimension 'ping_time' of {var_name!r} is "
                                  "supported")
    r_da = ds[range_var]
    if time_var not in r_da.dims:
        raise ValueError(f"Dimensions {{{time_var!r}}} do not exist. Expected one or more of {tuple(r_da.dims)}")
    if not 0 <= percentile <= 100:
        raise ValueError("Percentiles must be in the range [0, 100]")
    sv = _channel_cube(var, var_name, device)
    C, P, S = sv.shape
    if P == 0 or S == 0:
        return _mask_array(var, torch.ones((C, P, S), dtype=torch.bool, device=sv.device), "matecho_mask_valid")
    if window_ping // 2 == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    rows = _range_rows(r_da, range_var, time_var, C, S)
    chan_i = np.zeros((C, 2), dtype=np.int32)
    chan_d = np.zeros((C, 2), dtype=np.float64)
    for c in range(C):
        s_lo, s_top, dz, r_last = _window_rows(rows[c], start_depth, window_meter, range_var)
        chan_i[c] = s_lo, s_top
        chan_d[c] = dz, r_last
    bottom = None
    if bottom_var is not None and bottom_var in ds:
        b_da = ds[bottom_var]
        if tuple(b_da.dims) not in (("ping_time",), ("channel", "ping_time"), ("ping_time", "channel")):
            raise NotImplementedError(f"bottom_var={bottom_var!r} must have dims (ping_time) or (channel, ping_time), got "
                                      f"{tuple(b_da.dims)}")
        bottom = device_view(b_da, ("channel", "ping_time"), device=sv.device, dtype=torch.float64)
    mask = ops.transient_matecho(sv, rows, chan_i, chan_d, bottom, int(window_ping // 2), percentile, delta_db,
                                 max(int(extend_ping), 0), min_window)
    return _mask_array(var, mask, "matecho_mask_valid")
