"""apply_mask with the reference's signature (/root/reference/echopype/mask/api.py:307-464;
SURVEY 8f row 2).  Validation is host Python with the reference's error types and messages
(:39-70 dim alignment, :72-190 mask input, :193-247 var_name / fill_value); the array work is
epa_mask_and (logical AND of broadcast masks, :402-408) and epa_apply_mask (xr.where, :428-432).
Masks and sources given as file paths are out of scope (no zarr / netCDF IO in this package).
"""
import datetime
import pathlib
from collections import OrderedDict

import numpy as np
import torch

from .. import ops
from ..device_view import as_tensor, device_view
from ..utils.prov import echopype_prov_attrs, insert_processing_level
from ..xr_lite import DataArray, DeviceArray, from_xarray, is_device, xarray_io

_ALLOWED_DIMS = [
    {"ping_time", "range_sample"}, {"ping_time", "depth"}, {"ping_time", "echo_range"},
    {"channel", "ping_time", "range_sample"}, {"channel", "ping_time", "depth"},
    {"channel", "ping_time", "echo_range"},
]


def _no_paths(obj, what):
    if isinstance(obj, (str, pathlib.Path)):
        raise NotImplementedError(f"{what} given as a file path is not supported: pass the Dataset / DataArray")


def _validate_and_collect_mask_input(mask, storage_options_mask):
    single = not isinstance(mask, list)
    if single:
        mask = [mask]
        if not isinstance(storage_options_mask, dict):
            raise ValueError("The provided input storage_options_mask should be a single "
                             "dict because mask is a single value!")
        storage_options_mask = [storage_options_mask]
    if not isinstance(storage_options_mask, list):
        if not isinstance(storage_options_mask, dict):
            raise TypeError("storage_options_mask must be a list of dict or a dict!")
    elif not all(isinstance(e, dict) for e in storage_options_mask):
        raise TypeError("storage_options_mask must be a list of dict or a dict!")
    out = []
    for m in mask:
        _no_paths(m, "mask")
        m = from_xarray(m)
        if not isinstance(m, DataArray):
            raise TypeError("mask must be a DataArray or a list of DataArrays")
        if set(m.dims) not in _ALLOWED_DIMS:
            raise ValueError(
                "Masks must have one of the following dimensions: "
                "{'ping_time', 'range_sample'}, {'ping_time', 'depth'}, {'ping_time', 'echo_range'}, "
                "{'channel', 'ping_time', 'range_sample'}, {'channel', 'ping_time', 'depth'}"
                "{'channel', 'ping_time', 'echo_range'}")
        # boolean-like values only (:166-175); bool / uint8 device masks from this package's own
        # mask functions are boolean by construction
        if not (is_device(m.data) and m.data.tensor.dtype == torch.bool) and m.dtype != np.bool_:
            v = m.values
            if np.issubdtype(v.dtype, np.floating) and np.any(np.isnan(v)):
                raise TypeError("Mask cannot contain NaN")
            if not np.all(np.isin(np.unique(v), [0, 1, True, False])):
                raise TypeError("Mask must be boolean (True/False or 1/0)")
        out.append(m)
    shapes = set()
    for m in out:
        if "channel" in m.dims:
            # by dimension NAME: the reference compares positional shapes and so rejects its own
            # (channel, range_sample, ping_time) impulse mask next to a (channel, ping_time, ...) one
            shapes.add(frozenset((d, n) for d, n in zip(m.dims, m.shape) if d != "channel"))
    if len(shapes) > 1:
        raise ValueError("All masks must have the same shape in the 'channel' dimension.")
    return out[0] if single else out


def _check_mask_dim_alignment(source_ds, mask, var_name):
    masks = mask if isinstance(mask, list) else [mask]
    mask_dims = set()
    for m in masks:
        mask_dims.update(m.dims)
    target = set(source_ds[var_name].dims)
    if "channel" in mask_dims and "channel" not in target:
        raise ValueError("'channel' is a dimension in mask but not a dimension in source.")
    mask_dims.discard("channel")
    target.discard("channel")
    if mask_dims != target:
        raise ValueError(f"The dimensions of mask: ({mask_dims}) do not match the dimensions of source "
                         f"({target}) when not considering 'channel'.")
    return source_ds


def _check_var_name_fill_value(source_ds, var_name, fill_value):
    if not isinstance(var_name, str):
        raise TypeError("The input var_name must be a string!")
    if var_name not in source_ds.variables:
        raise ValueError("The Dataset source_ds does not contain the variable var_name!")
    fill_value = from_xarray(fill_value)
    if not isinstance(fill_value, (int, float, DataArray)):
        raise TypeError("The input fill_value must be of type int, float, or xr.DataArray!")
    if isinstance(fill_value, DataArray):
        da = source_ds[var_name]
        chan_shape = tuple(n for d, n in zip(da.dims, da.shape) if d != "channel")
        data = fill_value.data
        shape = tuple(n for n in data.shape if n != 1) if len(data.shape) != len(chan_shape) else tuple(data.shape)
        if shape != chan_shape:
            raise ValueError(f"If fill_value is an array it must be of the same shape as {var_name}!")
    return fill_value


def _mask_tensor(m, order):
    """uint8 device tensor of a mask with its dims in the order they appear in ``order``."""
    t = device_view(m, order)
    if t.dtype == torch.bool:  # the masks of echopype_amd.clean: reinterpreted, not copied
        return t.view(torch.uint8)
    return (t != 0).to(torch.uint8)


@xarray_io()
def apply_mask(source_ds, mask, var_name="Sv", fill_value=np.nan, storage_options_ds={},
               storage_options_mask={}):
    """Dataset like ``source_ds`` with ``var_name`` replaced by where(AND of masks, var, fill_value)."""
    _no_paths(source_ds, "source_ds")
    source_ds = from_xarray(source_ds)
    mask = _validate_and_collect_mask_input(mask, storage_options_mask)
    # (the reference checks var_name after the alignment, where a missing variable surfaces as a
    # KeyError from the dataset lookup; here the explicit messages come first)
    fill_value = _check_var_name_fill_value(source_ds, var_name, fill_value)
    source_ds = _check_mask_dim_alignment(source_ds, mask, var_name)

    source_da = source_ds[var_name]
    order = tuple(source_da.dims)
    src_t = as_tensor(source_da)
    if src_t.dtype not in (torch.float32, torch.float64):
        src_t = src_t.double()
    masks = mask if isinstance(mask, list) else [mask]
    # channel-carrying masks first so that the channel-less ones broadcast into them (xr.broadcast, :403)
    tensors = sorted((_mask_tensor(m, order) for m in masks), key=lambda t: -t.dim())
    final = tensors[0]  # (its shape is the shape of the AND of all: the others broadcast into it)
    for t in tensors[1:]:
        if final.numel() % t.numel() != 0 or tuple(final.shape[-t.dim():]) != tuple(t.shape):
            raise ValueError("All masks must have the same shape in the 'channel' dimension.")
    # up to four masks go to the kernel as they are (one sweep: the AND, the selection and the result's min / max); a
    # fifth and further ones are folded into the first beforehand
    while len(tensors) > 4:
        tensors = [ops.mask_and(tensors[0], tensors.pop())] + tensors[1:]
        final = tensors[0]
    has_chan = "channel" in order
    src_chan_shape = tuple(src_t.shape[1:]) if has_chan and order[0] == "channel" else tuple(
        n for d, n in zip(order, src_t.shape) if d != "channel")
    mask_has_chan = final.dim() == len(order) and has_chan
    mask_chan_shape = tuple(final.shape[1:]) if mask_has_chan else tuple(final.shape)
    if mask_chan_shape != src_chan_shape:
        raise ValueError(f"The final constructed mask is not of the same shape as source_ds[{var_name}] "
                         "along the ping_time, and range_sample dimensions!")
    if mask_has_chan and final.shape[0] != src_t.shape[0]:
        raise ValueError(f"If both the final constructed mask and source_ds[{var_name}] "
                         "have the channel dimension, that dimension should match between the two.")
    if has_chan and order[0] != "channel":
        raise NotImplementedError("the channel dimension of the source variable must come first")

    if isinstance(fill_value, DataArray):
        fill_t = as_tensor(fill_value, src_t.dtype).reshape(src_chan_shape).contiguous()
        out_t, mm = ops.apply_masks(src_t, tensors, fill_array=fill_t, want_minmax=True)
    else:
        out_t, mm = ops.apply_masks(src_t, tensors, fill_value=float(fill_value), want_minmax=True)

    output_ds = source_ds.copy()
    attrs = dict(source_da.attrs)
    lo, hi = mm.cpu().tolist()  # (a by-product of the sweep that wrote the array)
    attrs.update({
        "long_name": "Volume backscattering strength, masked (Sv re 1 m-1)",
        "actual_range": [round(lo, 2), round(hi, 2)],
        "history": f"{datetime.datetime.now(datetime.timezone.utc)}. `depth` calculated using:. "
                   "Created masked Sv dataarray.",
    })
    mattrs = dict(masks[0].attrs)
    if "history" in mattrs:
        attrs["history"] += f"\n{mattrs.pop('history')}"
    attrs.update(mattrs)
    output_ds[var_name] = DataArray(DeviceArray(out_t), order, attrs=attrs)
    prov = echopype_prov_attrs(process_type="mask")
    prov["mask_function"] = "mask.apply_mask"
    output_ds.attrs.update(prov)
    return insert_processing_level(output_ds, "L3*", input_ds=source_ds)


# ---- seafloor detection (reference: mask/api.py:866-945) ------------------------------------------------------------
from .seafloor_detection.bottom_basic import bottom_basic  # noqa: E402
from .seafloor_detection.bottom_blackwell import bottom_blackwell  # noqa: E402

# Registry of supported methods for bottom detection
METHODS_BOTTOM = {
    "basic": bottom_basic,
    "blackwell": bottom_blackwell,
}


def detect_seafloor(ds, method, params):
    """Dispatch seafloor detection to a chosen method and return a 1-D bottom line (``bottom_depth`` per
    ``ping_time``, data on the device).  ``method``: ``"basic"`` (threshold-only) or ``"blackwell"`` (Sv + split-beam
    angles); ``params``: that method's keyword arguments, omitted ones take its defaults (see
    seafloor_detection.bottom_basic / bottom_blackwell).  Sharded datasets are not supported.

    Raises ValueError if ``method`` is not supported."""
    if method not in METHODS_BOTTOM:
        raise ValueError(f"Unsupported bottom detection method: {method}")
    return METHODS_BOTTOM[method](ds, **params)


# ---- shoal detection (reference: mask/api.py:963-996) -----------------------------------------------------------------
from .shoal_detection.shoal_echoview import shoal_echoview  # noqa: E402
from .shoal_detection.shoal_weill import shoal_weill  # noqa: E402

# Registry of supported methods for shoal detection
METHODS_SHOAL = {
    "echoview": shoal_echoview,
    "weill": shoal_weill,
}


def detect_shoal(ds, method, params):
    """Dispatch shoal detection to a chosen method and return a 2-D boolean mask (``ping_time`` x ``range_sample``,
    True inside a shoal, data on the device).  ``method``: ``"weill"`` (threshold, gap filling, length filter) or
    ``"echoview"`` (candidates, linking, minimum shoal size); ``params``: that method's keyword arguments (see
    shoal_detection.shoal_weill / shoal_echoview).  One channel per call; sharded datasets are not supported.

    Raises ValueError if ``method`` is not supported."""
    if method not in METHODS_SHOAL:
        raise ValueError(f"Unsupported shoal detection method: {method}")
    return METHODS_SHOAL[method](ds, **params)


# ---- frequency differencing (reference: mask/api.py:467-675) ---------------------------------------------------------
from .freq_diff import _check_freq_diff_source_Sv, _parse_freq_diff_eq  # noqa: E402


@xarray_io()
def frequency_differencing(source_Sv, storage_options={}, freqABEq=None, chanABEq=None):
    """Boolean mask ``Sv[chanA] - Sv[chanB] operator diff`` ("frequency differencing", "dB differencing").

    The criterion is one string: ``freqABEq`` such as ``"38.0kHz - 120 kHz >= 10.0dB"`` (frequencies with the prefixes
    "", k, M, G, matched against ``frequency_nominal`` by exact equality) or ``chanABEq`` such as
    ``'"chan1" - "chan2" < 5dB'`` (channel names in double quotes); the operators are ``> < <= >= ==``.  Exactly one
    of the two is given.  ``source_Sv`` holds ``Sv`` with a ``channel`` dimension in any position, the coordinate
    ``channel`` and the variable ``frequency_nominal``; a file path raises ``NotImplementedError``
    (``storage_options`` is unused), and sharded datasets are not supported.

    The rule is NumPy's for an array and a Python scalar: the difference is rounded in the type of ``Sv`` and ``diff``
    is converted to that type before the comparison (float32 data is compared in float32; anything but float32 /
    float64 is converted to float64 first).  NaN in either channel, and inf - inf, give False for every operator.

    The two channels are compared element by element along the last dimension: where their sample intervals differ,
    index ``s`` is another range in each, and ``commongrid.regrid_Sv`` brings them onto one range grid first.

    Returns the DataArray ``mask`` over the dimensions of ``Sv`` without ``channel``, with the coordinates of ``Sv``
    that do not carry ``channel`` and the reference's attributes ``mask_type`` and ``history``.  Its data stays on the
    device (a ``torch.bool`` tensor) and goes straight into ``mask.apply_mask``.

    Device work: one streaming pass over the two selected planes (16-byte loads, four mask bytes per store); a device
    array with ``channel`` first is read where it lies, otherwise the two planes are gathered (device) or uploaded
    (host) first.  Host synchronisations: none."""
    freqAB, chanAB, operator, diff = _parse_freq_diff_eq(freqABEq, chanABEq)
    _no_paths(source_Sv, "source_Sv")
    source_Sv = from_xarray(source_Sv)
    _check_freq_diff_source_Sv(source_Sv, freqAB, chanAB)

    channels = [str(c) for c in source_Sv["channel"].values]
    if freqAB is not None:
        freqs = np.asarray(source_Sv["frequency_nominal"].values)
        pos = [int(np.flatnonzero(freqs == f)[0]) for f in freqAB]
    else:
        pos = [channels.index(c) for c in chanAB]
    chanA, chanB = channels[pos[0]], channels[pos[1]]

    sv_da = source_Sv["Sv"]
    rest = tuple(d for d in sv_da.dims if d != "channel")
    in_place = (is_device(sv_da.data) and sv_da.dims[0] == "channel" and sv_da.data.tensor.is_contiguous()
                and sv_da.data.tensor.dtype in (torch.float32, torch.float64))
    if in_place:
        sv_t, a, b = sv_da.data.tensor, pos[0], pos[1]
        if sv_t.device != torch.device("cuda", torch.cuda.current_device()):
            sv_t = sv_t.to(torch.device("cuda", torch.cuda.current_device()))
    else:  # the two planes alone are gathered / uploaded and converted
        sv_t, a, b = device_view(sv_da, ("channel",) + rest, index=pos, floating=True), 0, 1
    plane = ops.freq_diff_mask(sv_t, a, b, operator, diff)

    return DataArray(
        DeviceArray(plane), rest,
        coords={k: v for k, v in sv_da.coords.items() if k != "channel"},
        name="mask",
        attrs={
            "mask_type": "frequency differencing",
            "history": f"{datetime.datetime.now(datetime.timezone.utc)}. `depth` calculated using:. "
                       "Mask created by mask.frequency_differencing. "
                       f"Operation: Sv['{chanA}'] - Sv['{chanB}'] {operator} {diff}",
        })


# ---- a mask on the MVBS grid (reference: mask/api.py:678-863) ----------------------------------------------------------
from ..commongrid.utils import _parse_x_bin, ping_time_bin_parsing_and_conversion, resample_edges  # noqa: E402


@xarray_io()
def regrid_mask(mask_da, range_da, range_bin="20m", ping_time_bin="20s", third_dim=None, func="logical-AND",
                method="map-reduce", reindex=False, closed="left", range_var_max=None, **flox_kwargs):
    """``mask_da`` brought onto the (ping-time bin, range bin) grid of ``compute_MVBS``.

    A cell of the result is 1 / True where samples fall into it and, ``func="logical-AND"``, all of them are 1, or,
    ``func="logical-OR"``, one of them is; a cell without samples is 0 for both (the reference takes the group-by mean
    with ``fill_value=0.0`` and tests it for ``== 1.0`` / ``!= 0.0``).  The range edges are
    ``np.arange(0, range_var_max + 1e-8 + range_bin, range_bin)``, ``range_var_max`` the NaN-skipping maximum of
    ``range_da`` unless given (a string such as ``"250m"``); the time edges are those of
    ``ping_time.resample(ping_time=ping_time_bin)`` plus one closing edge; ``closed`` says which side of the intervals
    of both axes is closed.  Samples beyond the last range edge or with a NaN range belong to no cell.

    ``mask_da``: dimensions ``ping_time`` and ``depth`` plus ``third_dim`` if given, in any order; bool, uint8, any
    integer or float type holding only 0 and 1 (else ``ValueError``); on the device or the host.  ``range_da``: the range
    of every sample over ``depth``, or over ``(ping_time, depth)``; its name is the name of the result's range
    dimension.  With ``third_dim``, the result has one slice per distinct value of that coordinate, in sorted order;
    slices of ``mask_da`` with the same value merge their samples.  ``method``, ``reindex`` and ``flox_kwargs`` are
    checked as the reference checks them and otherwise ignored.  ``ping_time`` must be non-decreasing without NaT
    (``NotImplementedError`` otherwise: the time bins are offsets into the sorted pings); sharded datasets are not
    supported.

    Returns a DataArray with ``mask_da``'s name and type over ``(third_dim,) ping_time, <range_da.name>``, the
    coordinates the left edges of the bins, and the reference's attributes.  Its data stays on the device.

    Device work: one sweep over the mask (16 mask bytes per lane and load).  A workgroup takes a run of consecutive
    pings of one slice; with a 1-D range its lanes OR / AND the rows of a time bin in registers, the flags "a sample
    fell into the cell" and "a zero (AND) / a one (OR) fell into it" meet in LDS and are merged into the result with
    atomic OR, so a time bin of any length is shared by many workgroups and the result does not depend on their
    order; a range grid too large for LDS (more than 32768 bins) merges into the result directly.  A small launch
    before clears the flags, one after turns them into the result.  Host synchronisations: one for a bool / uint8 mask
    (the kernel's "a byte is neither 0 nor 1" word, read after the sweep) plus one for the maximum of a ``range_da``
    that lies on the device and no ``range_var_max``; masks of other types are checked and narrowed with torch first
    (one more)."""
    if method != "map-reduce" and reindex is not None:
        raise ValueError(f"Passing in reindex={reindex} is only allowed when method='map_reduce'.")
    if not isinstance(ping_time_bin, str):
        raise TypeError("ping_time_bin must be a string")
    mask_da = from_xarray(mask_da)
    range_da = from_xarray(range_da)
    if third_dim is None and len(mask_da.dims) != 2:
        raise ValueError("Mask must have only 2 dimensions unless 'third_dim' is specified.")
    if third_dim is not None and third_dim not in mask_da.dims:
        raise ValueError(f"Mask must contain the specified '{third_dim}' as a dimension.")
    if third_dim is not None and len(mask_da.dims) != 3:
        raise ValueError("Mask must have 3 dimensions when 'third_dim' is specified.")
    core = ("ping_time", "depth")
    if set(mask_da.dims) != set(core) | ({third_dim} if third_dim is not None else set()):
        raise ValueError(f"Mask must have the dimensions 'ping_time' and 'depth', got {tuple(mask_da.dims)}")
    order = ((third_dim,) if third_dim is not None else ()) + core

    in_dtype = mask_da.data.tensor.dtype if is_device(mask_da.data) else None
    if in_dtype is None and mask_da.dtype in (np.bool_, np.uint8):
        in_dtype = torch.bool if mask_da.dtype == np.bool_ else torch.uint8
    by_kernel = in_dtype in (torch.bool, torch.uint8)  # the sweep itself reports a byte that is neither 0 nor 1
    m_t = None
    if by_kernel:
        pass
    elif is_device(mask_da.data):
        m_t = device_view(mask_da, order)
        if not bool(((m_t == 0) | (m_t == 1)).all()):
            raise ValueError("Mask must be binary True/False or 1/0.")
        m_t = m_t.to(torch.uint8)
    else:
        host = np.asarray(mask_da.data)
        if not np.isin(host, [1, 0]).all():
            raise ValueError("Mask must be binary True/False or 1/0.")
        in_dtype = host.dtype
        mask_da = DataArray(host.astype(np.uint8), mask_da.dims, mask_da.coords, name=mask_da.name)
    if func not in ["logical-AND", "logical-OR"]:
        if in_dtype == torch.uint8:  # (the reference's order: the binary check comes first; no sweep will run to make it)
            d = mask_da.data
            if bool((d.tensor > 1).any()) if is_device(d) else bool((np.asarray(d) > 1).any()):
                raise ValueError("Mask must be binary True/False or 1/0.")
        raise ValueError("'func' must be 'logical-AND' or 'logical-OR'.")
    if closed not in ["right", "left"]:
        raise ValueError(f"{closed} is not a valid option. Options are 'left' or 'right'.")
    if m_t is None:
        m_t = device_view(mask_da, order)
    if m_t.dim() == 2:
        m_t = m_t.unsqueeze(0)
    T, P, D = m_t.shape

    # the range grid
    range_bin = _parse_x_bin(range_bin)
    if range_da.name is None:
        raise ValueError("range_da must have a name: it names the range dimension of the result")
    if set(range_da.dims) not in ({"depth"}, set(core)):
        raise ValueError(f"range_da must have the dimensions ('depth',) or ('ping_time', 'depth'), got {tuple(range_da.dims)}")
    r_t = device_view(range_da, core, dtype=torch.float64)
    if tuple(r_t.shape) not in ((D,), (P, D)):
        raise ValueError(f"range_da of shape {tuple(r_t.shape)} does not match the mask ({P} pings, {D} samples)")
    if range_var_max is None:
        if is_device(range_da.data):
            range_var_max = ops.nanminmax(r_t)[1]
        else:
            a = np.asarray(range_da.data, dtype=np.float64)
            range_var_max = float(np.max(a[~np.isnan(a)])) if np.any(~np.isnan(a)) else float("nan")
        if not np.isfinite(range_var_max):
            raise ValueError("range_da holds no finite maximum to size the range grid with")
    else:
        range_var_max = _parse_x_bin(range_var_max)
    range_var_max = range_var_max + 1e-8  # (the reference: "to ensure that we grab the last value")
    range_edges = np.arange(0, range_var_max + range_bin, range_bin)
    n_rbins = len(range_edges) - 1

    # the time grid
    ping_time = np.asarray(mask_da.coords["ping_time"])
    _, sorted_valid, pt_dev = ops.ping_time_facts(ping_time)
    if not sorted_valid:
        raise NotImplementedError("regrid_mask needs a non-decreasing ping_time without NaT")
    e0, dt, n_tbins = resample_edges(ping_time, ping_time_bin, sorted_valid=True)
    bin_start = ops.time_bin_offsets(pt_dev, e0, dt, n_tbins, closed)

    # the slices of the third dimension: one per distinct coordinate value, sorted (expected_groups=None)
    group = third_vals = None
    n_groups = T
    if third_dim is not None:
        vals = np.asarray(mask_da.coords[third_dim]) if third_dim in mask_da.coords else np.arange(T)
        third_vals, inverse = np.unique(vals, return_inverse=True)
        n_groups = len(third_vals)
        if not np.array_equal(inverse, np.arange(T)):
            group = ops.to_device_small(inverse.astype(np.int32), device=m_t.device)

    out, nonbinary = ops.regrid_mask(m_t, r_t, bin_start, n_tbins, range_bin, n_rbins, group=group, n_groups=n_groups,
                                     func=func, closed=closed)
    if by_kernel and int(nonbinary.item()):
        raise ValueError("Mask must be binary True/False or 1/0.")
    if third_dim is None:
        out = out[0]
    if isinstance(in_dtype, torch.dtype):
        out = out.view(torch.bool) if in_dtype == torch.bool else out.to(in_dtype)
        data = DeviceArray(out)
    else:  # a host mask of a type torch may lack: the small result is given that type on the device where it has it
        td = getattr(torch, np.dtype(in_dtype).name, None)
        data = DeviceArray(out.to(td)) if isinstance(td, torch.dtype) else out.cpu().numpy().astype(in_dtype)

    range_var = range_da.name
    value, unit = ping_time_bin_parsing_and_conversion(ping_time_bin)
    coords = OrderedDict()
    if third_dim is not None:
        coords[third_dim] = third_vals
    coords["ping_time"] = (np.int64(e0) + np.int64(dt) * np.arange(n_tbins, dtype=np.int64)).view("datetime64[ns]")
    coords[range_var] = DataArray(range_edges[:-1].astype(np.float64), (range_var,),
                                  attrs={"long_name": "Range distance", "units": "m"})
    return DataArray(
        data, ((third_dim,) if third_dim is not None else ()) + ("ping_time", range_var), coords=coords,
        name=mask_da.name,
        attrs={
            "cell_methods": f"ping_time: mean (interval: {value} {unit} comment: ping_time is the interval start) "
                            f"{range_var}: mean (interval: {range_bin} meter comment: {range_var} is the interval start)",
            "binning_mode": "physical units",
            "range_meter_interval": str(range_bin) + "m",
            "ping_time_interval": ping_time_bin,
        })


# ---- the samples between two lines (no counterpart in the reference: there it is ``ds["depth"] < bottom``) -------------
from numbers import Real  # noqa: E402

from ..device_view import resolve_device, strided_view  # noqa: E402
from ..xr_lite import LazyDeviceArray  # noqa: E402

_LINE_DIMS = ("channel", "ping_time")


def _check_bound(ds, bound, what, sizes):
    """A bound of ``line_mask`` checked on the host: None, a float, or the DataArray that holds the line."""
    if bound is None:
        return None
    if isinstance(bound, str):
        if bound in ds:  # the name of a variable first (the precedent: detect_transient(matecho)'s bottom_var)
            bound = ds[bound]
        else:
            bound = _parse_x_bin(bound)
    bound = from_xarray(bound)
    if isinstance(bound, (Real, np.number)) and not isinstance(bound, (bool, np.bool_)):
        return float(bound)
    if not isinstance(bound, DataArray):
        raise TypeError(f"{what} must be a number, a string such as '250.0m', the name of a variable or a DataArray, "
                        f"got {type(bound).__name__}")
    dims = tuple(bound.dims)
    if len(set(dims)) != len(dims) or not set(dims) <= set(_LINE_DIMS):
        raise ValueError(f"{what} must have dimensions among ('channel', 'ping_time'), got {dims}")
    for d, n in zip(dims, bound.shape):
        if d not in sizes:
            raise ValueError(f"{what} has the dimension {d!r}, which the masked variable lacks")
        if n != sizes[d]:
            raise ValueError(f"{what}: dimension {d!r} has length {n}, the dataset has {sizes[d]}")
    if "ping_time" in dims and "ping_time" in bound.coords and "ping_time" in ds.coords:
        if not np.array_equal(np.asarray(bound.coords["ping_time"]), np.asarray(ds["ping_time"].values)):
            raise ValueError(f"{what} lies on another ping_time than the dataset: a line from another dataset")
    kind = bound.data.tensor.dtype if is_device(bound.data) else np.asarray(bound.data).dtype
    if (kind.is_complex or kind == torch.bool) if isinstance(kind, torch.dtype) else kind.kind not in "fiu":
        raise TypeError(f"{what} must hold real numbers, got {kind}")
    return bound


def _bound_tensor(bound, dev):
    """What ``_check_bound`` returned as a float64 device tensor that broadcasts against (C, P), or None."""
    if bound is None:
        return None
    if isinstance(bound, float):
        return torch.full((1, 1), bound, dtype=torch.float64, device=dev)
    if is_device(bound.data):
        t = bound.data.tensor
        t = (t if t.device == dev else t.to(dev)).to(torch.float64)
    else:
        t = ops.to_device(np.ascontiguousarray(np.asarray(bound.data), dtype=np.float64), device=dev)
    dims = tuple(bound.dims)
    if dims == ("ping_time", "channel"):
        return t.t()  # (a view: the kernel reads the line through its strides)
    if dims == ("ping_time",):
        return t.unsqueeze(0)
    if dims == ("channel",):
        return t.unsqueeze(1)
    return t.reshape(1, 1) if dims == () else t


def _lazy_range_rows(da, order):
    """What a still unwritten ``echo_range`` / ``depth`` of ``compute_Sv`` / ``add_depth`` is a function of: (coefficient
    rows, raw samples whose NaNs are its NaNs, scale, offset) with scale = offset = None for an echo_range.  None when
    the variable is not of that kind (any longer): it is then read as an array."""
    d = da.data
    if not isinstance(d, LazyDeviceArray) or d.materialized or tuple(da.dims) != tuple(order) or len(order) != 3:
        return None
    base, scale, offset = d, None, None
    rows = d.coef_rows()
    if rows is None:
        aff = d.affine_of()
        if aff is None:
            return None
        base, scale, offset = aff
        rows = base.coef_rows()
    raw = base.nan_source()
    if rows is None or raw is None or raw.dtype != torch.float32 or tuple(raw.shape) != d.shape \
            or not raw.is_contiguous() or d.dtype not in (np.dtype("float32"), np.dtype("float64")):
        return None
    return rows, raw, scale, offset


@xarray_io()
def line_mask(ds, upper=None, lower=None, range_var="depth", var_name="Sv", closed="left", nan_line="exclude",
              upper_offset=0.0, lower_offset=0.0, *, device=None):
    """Boolean mask of the samples of ``ds[var_name]`` that lie between two lines: True where
    ``upper + upper_offset <= r < lower + lower_offset`` (``closed="left"``) or
    ``upper + upper_offset < r <= lower + lower_offset`` (``closed="right"``), ``r`` the value of ``ds[range_var]`` at the
    sample -- what ``(ds["depth"] >= upper) & (ds["depth"] < lower)`` is with xarray.  It is the step between
    ``detect_seafloor`` and ``apply_mask``: ``line_mask(ds_Sv, upper="10m", lower=bottom, lower_offset=-5.0)``.

    ``upper`` / ``lower``: None (that side is not tested; at least one is given), a number, a string ``"<number>m"``, the
    name of a variable of ``ds`` (looked up first), or a DataArray over ``()``, ``(ping_time,)``, ``(channel,)`` or
    ``(channel, ping_time)`` in either order, of any real type, on the host or the device, whose sizes -- and, if it
    carries one, whose ``ping_time`` coordinate -- are those of ``ds``.  The bound is the line converted to float64 plus
    the (finite) offset, one float64 addition.  ``ds[var_name]`` gives the dimensions and shape only:
    ``(channel, ping_time, X)`` or ``(ping_time, X)`` (another order: ``NotImplementedError``).  ``ds[range_var]`` has any
    subset of them, so the 1-D ``depth`` / ``echo_range`` coordinate of an MVBS dataset serves as well as a cube.

    Every comparison is made in float64 on the value ``ds[range_var]`` holds in its own type (float32 promotes exactly;
    other types are converted to float64 first): the result is NumPy's, without a tolerance.  A NaN range gives False,
    infinities compare as numbers.  Where a line is NaN, ``nan_line="exclude"`` makes the whole ping False (what
    ``depth < NaN`` gives) and ``nan_line="ignore"`` leaves that side untested there (a ping without a detected bottom
    keeps its column).

    Returns the bool DataArray ``line_mask`` with the dimensions, shape and coordinates of ``ds[var_name]``, its data on
    the device: it goes straight into ``apply_mask`` or ``regrid_mask``.  Sharded datasets are not supported.

    Device work: one launch (``epa_line_mask``), 1 byte written per sample.  A range array is read where it lies, a
    lower-dimensional one through zero strides.  An ``echo_range`` / ``depth`` that ``compute_Sv`` / ``add_depth`` left
    unwritten is evaluated from its coefficient rows with the arithmetic that would write it, rounding to its type
    included, so the decisions are those on the written array, which stays unwritten.  Host synchronisations: none."""
    ds = from_xarray(ds)
    if closed not in ("left", "right"):
        raise ValueError(f"{closed} is not a valid option. Options are 'left' or 'right'.")
    if nan_line not in ("exclude", "ignore"):
        raise ValueError(f"{nan_line} is not a valid option. Options are 'exclude' or 'ignore'.")
    if upper is None and lower is None:
        raise ValueError("At least one of upper and lower must be given.")
    for name, off in (("upper_offset", upper_offset), ("lower_offset", lower_offset)):
        if isinstance(off, (bool, np.bool_)) or not isinstance(off, (Real, np.number)) or not np.isfinite(off):
            raise ValueError(f"{name} must be a finite number, got {off!r}")
    for name, v in (("var_name", var_name), ("range_var", range_var)):
        if not isinstance(v, str):
            raise TypeError(f"The input {name} must be a string!")
        if v not in ds:
            raise ValueError(f"The Dataset ds does not contain the variable {v}!")
    src = ds[var_name]
    order = tuple(src.dims)
    has_chan = "channel" in order
    if not ((len(order) == 3 and order[:2] == _LINE_DIMS) or (len(order) == 2 and order[0] == "ping_time")):
        raise NotImplementedError(f"the dimensions of {var_name} must be (channel, ping_time, X) or (ping_time, X), "
                                  f"got {order}")
    shape = tuple(src.shape)
    C, P, S = ((1,) + shape) if not has_chan else shape
    sizes = dict(zip(order, shape))
    rng = ds[range_var]
    rdims = tuple(rng.dims)
    if len(set(rdims)) != len(rdims) or not set(rdims) <= set(order):
        raise ValueError(f"The dimensions of {range_var}, {rdims}, must be among those of {var_name}, {order}.")
    if any(n != sizes[d] for d, n in zip(rdims, rng.shape)):
        raise ValueError(f"The shape of {range_var}, {dict(zip(rdims, rng.shape))}, does not match {var_name}, {sizes}.")

    if not is_device(rng.data) and np.asarray(rng.data).dtype.kind not in "fiu":
        raise TypeError(f"{range_var} must hold real numbers, got {np.asarray(rng.data).dtype}")
    upper, lower = _check_bound(ds, upper, "upper", sizes), _check_bound(ds, lower, "lower", sizes)

    lazy = _lazy_range_rows(rng, order)
    if lazy is not None:
        dev = lazy[0].device
    elif is_device(rng.data):
        dev = rng.data.tensor.device
    elif is_device(src.data) and not isinstance(src.data, LazyDeviceArray):
        dev = src.data.tensor.device
    else:
        dev = resolve_device(device)
    up_t, lo_t = _bound_tensor(upper, dev), _bound_tensor(lower, dev)

    kw = dict(upper=up_t, lower=lo_t, upper_offset=float(upper_offset), lower_offset=float(lower_offset), closed=closed,
              nan_line=nan_line)
    if lazy is not None:
        rows, raw, scale, offset = lazy
        out = ops.line_mask((C, P, S), coef=rows, nan_raw=raw, scale=scale, offset=offset,
                            dtype=torch.float64 if rng.data.dtype == np.dtype("float64") else torch.float32, **kw)
    else:
        # the dimensions in the order of the cube (a view), a broadcast axis of length 1 for those the range lacks
        r_t = strided_view(rng, order, dev)
        out = ops.line_mask((C, P, S), range=r_t if has_chan else r_t.unsqueeze(0), **kw)
    if not has_chan:
        out = out[0]
    return DataArray(
        DeviceArray(out), order, coords=dict(src.coords), name="line_mask",
        attrs={"mask_type": "line", "range_var": range_var, "closed": closed, "nan_line": nan_line,
               "upper_offset": float(upper_offset), "lower_offset": float(lower_offset)})
