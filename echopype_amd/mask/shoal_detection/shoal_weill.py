"""mask.detect_shoal(method="weill") (reference: echopype mask/shoal_detection/shoal_weill.py; Weill et al. 1993,
"MOVIES-B -- an acoustic detection description software. Application to shoal species' classification")."""
from ... import ops
from ...xr_lite import xarray_io
from .utils import _channel_plane, _check_state, _mask_array


@xarray_io()
def shoal_weill(ds, var_name, channel=None, thr=-70.0, maxvgap=5, maxhgap=0, minvlen=0, minhlen=0, *, device=None):
    """Weill-style shoal mask of one channel: threshold, gap filling along both axes, size filter.

    1. Foreground is ``Sv > thr`` (compared in float64, as the reference's masked-array comparison does: ``thr`` is not rounded to a float32 array's type; NaN is background).
    2. In every ping, a run of background samples with foreground on both sides and at most ``maxvgap`` samples long
       becomes foreground; runs that reach the first or the last sample stay.
    3. On that result the same along pings, at every sample, with ``maxhgap``.
    4. The 4-connected components of the result whose extent is below ``minvlen`` samples or below ``minhlen`` pings
       are removed (extent = last index - first index + 1).

    The gap and length parameters are compared as they are given; the attributes carry ``int()`` of them.  ``Sv`` may be
    (channel, ping_time, range_sample) -- ``channel`` then selects the plane -- or a plane without a channel dimension;
    float32 or float64, on the device or the host.  Returns the boolean ``shoal_mask_weill`` (ping_time, range_sample)
    with the reference's attributes; its data stays on the device (a ``torch.bool`` tensor) and goes straight into
    ``mask.apply_mask``.

    Device work: one pass for steps 1-2 (a wave per ping), one in-place pass for step 3 when ``maxhgap >= 1``, and, only
    when a length can remove anything (``minvlen > 1`` or ``minhlen > 1``), union-find labelling with per-component
    bounding boxes.  Host synchronisations: one with the size filter (the union-find error word), none without.
    Scratch on the device: 8 B (component codes) per pixel and 20 B per table entry, one entry per two pixels."""
    if var_name not in ds:
        raise ValueError(f"Variable '{var_name}' not found in dataset")
    var = ds[var_name]
    if "channel" in var.dims and channel is None:
        raise ValueError("Please specify 'channel' for multi-channel data.")
    rest = [d for d in var.dims if d != "channel"]
    if not {"ping_time", "range_sample"}.issubset(set(rest)):
        raise ValueError(f"'{var_name}' must have dims including 'ping_time' and 'range_sample', got {tuple(rest)}")
    sv = _channel_plane(var, channel, device, var_name)

    P, S = sv.shape
    if P == 0 or S == 0:
        plane = sv.new_zeros((P, S), dtype=bool)
    else:
        plane = ops.shoal_threshold_fill(sv, float(thr), maxvgap, maxhgap)
        if (minvlen > 1) or (minhlen > 1):  # every component is at least 1 x 1
            state = ops.shoal_state(sv.device)
            parent, table = ops.shoal_label(plane, 4, state)
            ops.shoal_weill_filter(plane, parent, table, minvlen, minhlen, state)
            _check_state(state, "shoal_weill")

    return _mask_array(ds, plane, "shoal_mask_weill", {
        "description": f"Weill-style threshold+gap-fill mask on '{var_name}'",
        "threshold_dB": float(thr),
        "maxvgap": int(maxvgap),
        "maxhgap": int(maxhgap),
        "minvlen": int(minvlen),
        "minhlen": int(minhlen),
        **({"channel": str(channel)} if channel is not None else {}),
    })
