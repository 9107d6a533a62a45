"""Single targets: the echoes of individual fish, found along every ping and compensated for their position in the
beam (no counterpart in the reference; on the host this is a Python loop over pings and peaks).

``detect_single_targets`` brings together two results the package already leaves in HBM -- the point-scattering strength
of ``calibrate.compute_TS`` and the mechanical angles of ``consolidate.add_splitbeam_angle`` -- and returns a table with
one row per target, so that ``open_raw -> compute_TS -> add_splitbeam_angle -> detect_single_targets`` runs from a file
to a target table without the sample cubes leaving the device.  The rules are THIS PROJECT'S restatement of Echoview's
"single target detection, split beam" step; they have never been run against Echoview.  ``tests/single_target_ref.py``
restates them in NumPy and is the judge of the kernels.

Device work (csrc/single_target.hip): a count pass over ``TS`` (``epa_single_target_count``: the number of targets of
every (channel, ping), the candidates and rejections per channel), an exclusive scan of those numbers (torch
``cumsum``), and an emit pass (``epa_single_target_emit``) that reads the rows holding targets once more and writes the
table at the scanned offsets, in sample order.  The angles and the range are read only at the envelopes of candidates
that pass rules 1 and 2.  Host synchronisations: one, through ``_to_host``: the total count, which sizes the table.
Nothing detected ends after it, without an emit launch.  Device memory besides the result: the (5, C, P) float64
parameter rows and the int64 offsets."""
import numbers

import numpy as np
import torch

from .. import _lib, ops
from ..calibrate.calibrate_ek import retrieve_correct_beam_group
from ..device_view import device_view, resolve_device
from ..echodata import EchoData, as_lite_echodata
from ..xr_lite import DataArray, Dataset, DeviceArray, from_xarray, is_device, xarray_io

_DIMS = ("channel", "ping_time", "range_sample")
_LIMITS = _lib.SINGLE_TARGET_LIMITS
_OPTIONAL = ("var_name", "range_var", "channel", "pulse_length_samples")
_BEAM_PARAMS = ("beamwidth_alongship", "beamwidth_athwartship", "angle_offset_alongship", "angle_offset_athwartship")
_ANGLES = ("angle_alongship", "angle_athwartship")
RULES = ("normalized_pulse_length", "not_envelope_maximum", "beam_compensation", "angle_std")


def _to_host(t):
    """The one place this module copies device data to the host (a synchronisation: the tests count them)."""
    return t.cpu()


def _check_params(params):
    """The keys and numbers of ``params``, checked on the host -> the seven limits as a float64 array."""
    if not isinstance(params, dict):
        raise ValueError(f"params must be a dict, got {type(params).__name__}")
    unknown = sorted(k for k in params if k not in _LIMITS + _OPTIONAL)
    if unknown:
        raise ValueError(f"Unknown single-target parameter(s) {unknown}; known: {sorted(_LIMITS + _OPTIONAL)}")
    missing = [k for k in _LIMITS if k not in params]
    if missing:
        raise ValueError(f"Missing single-target parameter(s) {missing}")
    lim = np.empty(len(_LIMITS), dtype=np.float64)
    for i, k in enumerate(_LIMITS):
        v = params[k]
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.integer, np.floating)) \
                or not np.isfinite(float(v)):
            raise ValueError(f"{k} must be a finite real number, got {v!r}")
        lim[i] = float(v)
    if not params["pldl"] > 0:
        raise ValueError(f"pldl must be positive, got {params['pldl']!r}")
    if params["min_norm_pulse_length"] > params["max_norm_pulse_length"]:
        raise ValueError(f"min_norm_pulse_length {params['min_norm_pulse_length']!r} exceeds max_norm_pulse_length "
                         f"{params['max_norm_pulse_length']!r}")
    for k in ("var_name", "range_var"):
        if k in params and not isinstance(params[k], str):
            raise ValueError(f"{k} must be a string, got {params[k]!r}")
    return lim


def _channel_index(ds, channel):
    """Positions along ``ds.channel`` of the label(s) ``channel`` (compared by their ``str()``); None: all."""
    if channel is None:
        return None
    if "channel" not in ds.coords:
        raise ValueError("params['channel'] is given but the Dataset has no channel coordinate")
    have = [str(c) for c in np.asarray(ds["channel"].values).reshape(-1)]
    want = [channel] if isinstance(channel, (str, bytes)) or np.ndim(channel) == 0 else list(channel)
    missing = [str(c) for c in want if str(c) not in have]
    if missing or not want:
        raise ValueError(f"channel(s) {missing} are not among the Dataset's channels {have}")
    return [have.index(str(c)) for c in want]


def _cp_rows(da, idx, C, P, dev, what):
    """A parameter over (), (channel,) or (channel, ping_time) as a float64 (C, P) device view."""
    dims = tuple(da.dims)
    if len(set(dims)) != len(dims) or not set(dims) <= {"channel", "ping_time"}:
        raise ValueError(f"{what} must be over (channel) or (channel, ping_time), got {dims}")
    t = device_view(da, ("channel", "ping_time"), device=dev, dtype=torch.float64,
                    index=idx if "channel" in dims else None)
    if not dims:
        t = t.reshape(())
    t = t[tuple(slice(None) if d in dims else None for d in ("channel", "ping_time"))]
    try:
        return t.expand(C, P)
    except RuntimeError:
        raise ValueError(f"{what} of shape {tuple(da.shape)} does not match {C} channels and {P} pings") from None


def _spp_rows(params, echodata, ds, idx, n_chan, C, P, dev):
    """Samples per pulse as a float64 (C, P) device view: ``params['pulse_length_samples']`` (a scalar, one per channel
    of the Dataset, or (channel, ping_time)), else ``transmit_duration_nominal / sample_interval`` of the echodata's
    power beam group at the Dataset's channels."""
    if params.get("pulse_length_samples") is not None:
        a = np.asarray(params["pulse_length_samples"])
        if a.dtype.kind not in "fiu" or a.ndim > 2:
            raise ValueError("pulse_length_samples must hold real numbers: a scalar, one per channel, or "
                             "(channel, ping_time)")
        a = a.astype(np.float64)
        if a.ndim >= 1:
            if a.shape[0] != n_chan or (a.ndim == 2 and a.shape[1] != P):
                raise ValueError(f"pulse_length_samples of shape {a.shape} does not match {n_chan} channels and {P} "
                                 "pings")
            if idx is not None:
                a = a[idx]
        da = DataArray(a, ("channel", "ping_time")[:a.ndim])
        return _cp_rows(da, None, C, P, dev, "pulse_length_samples")
    if not isinstance(echodata, EchoData):
        echodata = as_lite_echodata(echodata)
    beam = echodata[retrieve_correct_beam_group(echodata, "CW", "power")]
    for k in ("transmit_duration_nominal", "sample_interval"):
        if k not in beam:
            raise ValueError(f"The echodata's beam group does not contain {k}")
    have = [str(c) for c in np.asarray(beam["channel"].values).reshape(-1)]
    chans = [str(c) for c in np.asarray(ds["channel"].values).reshape(-1)] if "channel" in ds.coords else have
    if idx is not None:
        chans = [chans[i] for i in idx]
    missing = [c for c in chans if c not in have]
    if missing:
        raise ValueError(f"channel(s) {missing} of the Dataset are not in the echodata's beam group")
    bidx = [have.index(c) for c in chans]
    tau = _cp_rows(beam["transmit_duration_nominal"], bidx, C, P, dev, "transmit_duration_nominal")
    si = _cp_rows(beam["sample_interval"], bidx, C, P, dev, "sample_interval")
    return tau / si


def _empty_columns(dev):
    return (torch.zeros((_lib.SINGLE_TARGET_ICOLS, 0), dtype=torch.int32, device=dev),
            torch.zeros((_lib.SINGLE_TARGET_FCOLS, 0), dtype=torch.float64, device=dev))


def _split_beam(ds, params, echodata, device):
    lim = _check_params(params)
    var_name, range_var = params.get("var_name", "TS"), params.get("range_var", "echo_range")
    for name in (var_name,) + _ANGLES + (range_var,) + _BEAM_PARAMS:
        if name not in ds:
            raise ValueError(f"The Dataset does not contain the variable {name!r}!")
    src, rng = ds[var_name], ds[range_var]
    order = tuple(src.dims)
    if len(set(order)) != len(order) or set(order) != set(_DIMS):
        raise ValueError(f"{var_name} must have the dimensions {_DIMS} (in any order), got {order}")
    sizes = dict(zip(order, src.shape))
    for name in _ANGLES:
        a = ds[name]
        if set(a.dims) != set(_DIMS) or any(n != sizes[d] for d, n in zip(a.dims, a.shape)):
            raise ValueError(f"{name} must have the dimensions and shape of {var_name}, {sizes}, got "
                             f"{dict(zip(a.dims, a.shape))}")
    rdims = tuple(rng.dims)
    if len(set(rdims)) != len(rdims) or not set(rdims) <= set(order):
        raise ValueError(f"The dimensions of {range_var}, {rdims}, must be among those of {var_name}, {order}.")
    if any(n != sizes[d] for d, n in zip(rdims, rng.shape)):
        raise ValueError(f"The shape of {range_var}, {dict(zip(rdims, rng.shape))}, does not match {var_name}, {sizes}.")
    for da, what in ((src, var_name), (rng, range_var)) + tuple((ds[n], n) for n in _ANGLES):
        if not is_device(da.data) and np.asarray(da.data).dtype.kind not in "fiu":
            raise TypeError(f"{what} must hold real numbers, got {np.asarray(da.data).dtype}")
    idx = _channel_index(ds, params.get("channel"))
    n_chan, P, S = sizes["channel"], sizes["ping_time"], sizes["range_sample"]
    C = n_chan if idx is None else len(idx)
    if params.get("pulse_length_samples") is None and echodata is None:
        raise ValueError("The samples per pulse are needed: give params['pulse_length_samples'] or the echodata whose "
                         "power beam group holds transmit_duration_nominal and sample_interval")

    dev = src.data.tensor.device if device is None and is_device(src.data) else resolve_device(device)
    spp = _spp_rows(params, echodata, ds, idx, n_chan, C, P, dev)
    prm = torch.stack([spp] + [_cp_rows(ds[k], idx, C, P, dev, k) for k in _BEAM_PARAMS]).contiguous()

    cubes = [device_view(ds[k], _DIMS, device=dev, index=idx, floating=True) for k in (var_name,) + _ANGLES]
    r_t = device_view(rng, _DIMS, device=dev, index=idx if "channel" in rdims else None, floating=True)
    if len({t.dtype for t in cubes + [r_t]}) > 1:
        cubes, r_t = [t.double() for t in cubes], r_t.double()
    r_t = r_t[tuple(slice(None) if d in rdims else None for d in _DIMS)]  # a broadcast axis where the range has none
    ts, al, at = cubes

    if C * P * S == 0:
        n_targets = torch.zeros((C, P), dtype=torch.int32, device=dev)
        n_cand = torch.zeros(C, dtype=torch.int64, device=dev)
        n_rej = torch.zeros((C, 4), dtype=torch.int64, device=dev)
        icols, fcols = _empty_columns(dev)
    else:
        n_targets, n_cand, n_rej = ops.single_target_count(ts, al, at, r_t, prm, lim)
        flat = n_targets.reshape(-1).to(torch.int64)
        incl = torch.cumsum(flat, 0)
        n = int(_to_host(incl[-1:])[0])  # the one synchronisation: the total sizes the table
        if n == 0:
            icols, fcols = _empty_columns(dev)
        else:
            icols, fcols = ops.single_target_emit(ts, al, at, r_t, prm, lim, n_targets, (incl - flat).reshape(C, P), n)

    coords = {"target": np.arange(icols.shape[1], dtype=np.int64), "rule": np.asarray(RULES)}
    for d, size in (("channel", n_chan), ("ping_time", P)):
        if d in src.coords and np.ndim(src.coords[d]) == 1 and len(src.coords[d]) == size:
            c = np.asarray(getattr(src.coords[d], "values", src.coords[d]))
            coords[d] = c[idx] if d == "channel" and idx is not None else c
        else:
            coords[d] = np.arange(C if d == "channel" else P)
    out = Dataset(coords=coords, attrs={"method": "split_beam", **{k: float(v) for k, v in zip(_LIMITS, lim)},
                                        "var_name": var_name, "range_var": range_var})
    for k, name in enumerate(_lib.SINGLE_TARGET_ICOL_NAMES):
        out[name] = DataArray(DeviceArray(icols[k]), ("target",), name=name)
    for k, name in enumerate(_lib.SINGLE_TARGET_FCOL_NAMES):
        out[name] = DataArray(DeviceArray(fcols[k]), ("target",), name=name)
    pt = np.asarray(coords["ping_time"])
    if pt.dtype.kind == "M":
        pt_dev = ops.to_device(pt.astype("datetime64[ns]").view(np.int64), device=dev)
        attrs = {"units": "nanoseconds since 1970-01-01"}
    else:
        pt_dev, attrs = ops.to_device(pt, device=dev), {}
    out["target_ping_time"] = DataArray(DeviceArray(pt_dev.index_select(0, icols[1].to(torch.int64))), ("target",),
                                        attrs=attrs, name="target_ping_time")
    out["n_targets"] = DataArray(DeviceArray(n_targets), ("channel", "ping_time"), name="n_targets")
    out["n_candidates"] = DataArray(DeviceArray(n_cand), ("channel",), name="n_candidates")
    out["n_rejected"] = DataArray(DeviceArray(n_rej), ("channel", "rule"), name="n_rejected")
    return out


# Registry of supported methods for single-target detection
METHODS_SINGLE_TARGET = {
    "split_beam": _split_beam,
}


@xarray_io()
def detect_single_targets(ds, method, params, echodata=None, *, device=None):
    """Detect single targets along every (channel, ping) of a TS dataset and return one table row per target.

    ``method``: ``"split_beam"`` (the only one; another raises ``ValueError`` naming the methods).  ``params``: the
    seven thresholds ``TS_threshold``, ``pldl``, ``min_norm_pulse_length``, ``max_norm_pulse_length``,
    ``max_beam_compensation``, ``max_std_alongship``, ``max_std_athwartship`` -- all required, each a finite real
    number -- and optionally ``var_name`` ("TS"), ``range_var`` ("echo_range"), ``channel`` (a label or a list of
    labels; default: all channels) and ``pulse_length_samples``.  An unknown key, a missing key, a non-number,
    ``pldl <= 0`` or ``min > max`` raises ``ValueError`` before any device work.

    Read from ``ds``: ``ds[var_name]`` over (channel, ping_time, range_sample) in any order, float32 or float64;
    ``angle_alongship`` and ``angle_athwartship`` of the same shape; ``ds[range_var]`` over any subset of those
    dimensions, read through its strides; ``beamwidth_alongship``, ``beamwidth_athwartship``,
    ``angle_offset_alongship`` and ``angle_offset_athwartship`` over (channel) or (channel, ping_time).  A missing
    variable raises ``ValueError`` and names it.  The samples per pulse ``spp`` (channel, ping_time) are
    ``params["pulse_length_samples"]`` if given (a scalar, one per channel of ``ds``, or (channel, ping_time)),
    otherwise ``transmit_duration_nominal / sample_interval`` of the power beam group of ``echodata``, selected by
    ``ds.channel``; with neither, ``ValueError``.  All arithmetic is float64 (float32 inputs are converted, which is
    exact; if ``TS``, the angles and the range differ in type, all go to float64 first).  Sharded datasets are not
    supported.

    The detection rules are this project's restatement of Echoview's "single target detection, split beam"; they have
    never been run against Echoview.  Per channel and ping, along range_sample:

    1. **Candidate.**
       - A sample ``s`` is a candidate when ``TS[s] >= TS_threshold`` (so not NaN) and both neighbour tests hold.
       - Left neighbour: either ``s`` is the first sample, or ``TS[s-1] >= TS[s]`` is false. A lower or NaN left
         neighbour passes.
       - Right neighbour: either ``s`` is the last sample, or ``TS[s+1] > TS[s]`` is false.
       - Of a plateau of equal values, the leftmost sample is the candidate.
    2. **Envelope.**
       - ``L = TS[s] - pldl``.
       - ``l`` is the smallest index such that every ``k`` in ``[l, s]`` has ``TS[k] >= L``. ``r`` is found likewise
         to the right.
       - NaN and the row ends stop the walk.
       - ``n = r - l + 1``. ``npl = n / spp`` is a single division.
       - Rule 1 rejects unless ``npl >= min && npl <= max``. A NaN or non-positive ``spp`` therefore rejects.
       - Work per candidate must be bounded. A walk may stop as soon as ``n`` alone already exceeds what ``max``
         allows.
    3. **Not the envelope's maximum.** Rule 2 rejects if any ``TS[k] > TS[s]`` for ``k`` in ``[l, r]``. The envelope
       then belongs to a stronger echo.
    4. **Position and compensation.**
       - ``a`` and ``b`` are the arithmetic means of the two angles over ``[l, r]``.
       - ``x = 2 (a - off_al) / bw_al``, and ``y`` likewise.
       - ``B = 6.0206 (x² + y² - 0.18 x² y²)``. This is the Simrad LOBE model.
       - Rule 3 rejects unless ``B <= max_beam_compensation``. NaN angles therefore reject.
       - ``TS_comp = TS[s] + B``.
    5. **Angular spread.** Take the population standard deviations (ddof 0, about those means) of both angles over
       ``[l, r]``. Rule 4 rejects unless both are ``<=`` their limits.
    6. **Range.** ``target_range = sum(w r) / sum(w)`` with ``w = 10^(TS/10)``, over the samples of ``[l, r]`` whose
       range is not NaN. It is NaN if there are none.

    The rules are tried in this order. A rejected candidate counts under the first rule that rejects it.  (A
    non-positive ``spp`` is rejected under rule 1 as stated, whatever the sign of ``min``.)

    Returns a Dataset on the dimension ``target``, ordered by (channel, ping, sample), all of it resident on the
    device: the int32 columns ``channel_index``, ``ping_index``, ``range_sample`` (the peak), ``sample_first``,
    ``sample_last``; the float64 columns ``TS_uncomp``, ``TS_comp``, ``beam_compensation``, ``target_range``,
    ``angle_alongship``, ``angle_athwartship``, ``std_angle_alongship``, ``std_angle_athwartship``,
    ``normalized_pulse_length``; ``target_ping_time``, the ``ping_time`` of every target gathered on the device (int64
    nanoseconds for a datetime coordinate; named so because ``ping_time`` is the coordinate of ``n_targets``); and the
    counts ``n_targets`` (channel, ping_time) int32, ``n_candidates`` (channel) and ``n_rejected`` (channel, rule)
    over the four rules.  ``channel_index`` counts along the result's ``channel`` coordinate (the selected channels).
    No pings, no samples, or nothing detected gives the same variables with ``target`` of length 0.  The order is
    fully defined and no sum depends on scheduling: two calls give identical tables.  ``track_targets`` groups the rows
    of this table into fish tracks.

    Device work and the one host synchronisation: see the module."""
    ds = from_xarray(ds)
    if method not in METHODS_SINGLE_TARGET:
        raise ValueError(f"Unsupported single-target detection method: {method!r}; supported: "
                         f"{sorted(METHODS_SINGLE_TARGET)}")
    return METHODS_SINGLE_TARGET[method](ds, params, echodata, device)
