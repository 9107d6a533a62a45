"""Target strength spectra: TS(f) of every single target of an EK80 FM (broadband) file -- the frequency response that
separates swimbladdered fish from krill, and what an FM ping is recorded for (no counterpart in the reference; on the
host this is a Python loop over targets: pulse compression around each one, a Fourier sum, a frequency-dependent
calibration).

``target_spectra`` brings together what the package already leaves in HBM or in the host code -- the complex sector
samples, the matched-filter replicas of ``calibrate/ek80_complex.py``, the target table of ``detect_single_targets`` and
the rules that evaluate calibration and environment parameters at a frequency -- so that ``compute_TS(BB) ->
add_splitbeam_angle(pulse_compression=True) -> detect_single_targets -> target_spectra`` goes from a file to TS(f) per
target without the sample cubes leaving the device.  The rules are THIS PROJECT'S restatement of Andersen et al.,
"Quantitative processing of broadband data as implemented in a scientific split-beam echosounder" (2021); they have never
been run against Echoview or the CRIMAC code, nor on recorded data.  ``tests/target_spectra_ref.py`` restates them in
NumPy and is the judge of the kernel.

Device work (csrc/target_spectrum.hip, ``epa_target_spectra``): one small kernel per call that leaves, per replica and
frequency, the Fourier step and 1 / |A(f)|^2, then one kernel with a workgroup per target.  Host work: the O(C F)
parameter tables.  Host synchronisations: one, through ``_to_host``: which pings hold targets (their sample interval must
be one value per replica).  An empty table ends before it, without a launch."""
import numbers

import numpy as np
import torch

from .. import _lib, ops
from ..calibrate.cal_params import get_cal_params_EK
from ..calibrate.calibrate_base import cp_array
from ..calibrate.calibrate_ek import CalibrateEK80, retrieve_correct_beam_group
from ..calibrate.env_params import get_env_params_EK
from ..device_view import as_tensor, resolve_device
from ..echodata import EchoData, as_lite_echodata
from ..xr_lite import DataArray, Dataset, DeviceArray, from_xarray, is_device, xarray_io

_REQUIRED = ("half_window", "n_frequencies")
_OPTIONAL = ("band_margin", "frequency_limits")
_ICOLS = ("channel_index", "ping_index", "range_sample")
_FCOLS = ("target_range", "angle_alongship", "angle_athwartship")


def _to_host(t):
    """The one place this module copies device data to the host (a synchronisation: the tests count them)."""
    return t.cpu()


def _is_real(v):
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (numbers.Real, np.integer, np.floating)) \
        and np.isfinite(float(v))


def _check_params(params):
    """The keys and numbers of ``params``, checked on the host -> (half_window, n_frequencies, band_margin,
    frequency_limits as a float64 (n, 2) array or None)."""
    if not isinstance(params, dict):
        raise ValueError(f"params must be a dict, got {type(params).__name__}")
    unknown = sorted(k for k in params if k not in _REQUIRED + _OPTIONAL)
    if unknown:
        raise ValueError(f"Unknown target-spectra parameter(s) {unknown}; known: {sorted(_REQUIRED + _OPTIONAL)}")
    missing = [k for k in _REQUIRED if k not in params]
    if missing:
        raise ValueError(f"Missing target-spectra parameter(s) {missing}")
    for k, lo, hi in (("half_window", 0, _lib.TARGET_SPECTRA_MAX_HALF_WINDOW),
                      ("n_frequencies", 1, _lib.TARGET_SPECTRA_MAX_FREQ)):
        v = params[k]
        if not _is_real(v) or float(v) != int(v) or not lo <= int(v) <= hi:
            raise ValueError(f"{k} must be an integer from {lo} to {hi}, got {v!r}")
    m = params.get("band_margin", 0.1)
    if not _is_real(m) or not 0.0 <= float(m) < 0.5:
        raise ValueError(f"band_margin must be a real number in [0, 0.5), got {m!r}")
    lim = params.get("frequency_limits")
    if lim is not None:
        try:
            lim = np.asarray(lim, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"frequency_limits must hold real numbers, got {params['frequency_limits']!r}") from None
        if lim.ndim not in (1, 2) or lim.shape[-1] != 2 or not np.isfinite(lim).all():
            raise ValueError(f"frequency_limits must be one finite (lo, hi) pair or one per channel, got shape {lim.shape}")
        lim = lim.reshape(-1, 2)
        if not ((lim[:, 0] > 0) & (lim[:, 0] <= lim[:, 1])).all():
            raise ValueError(f"frequency_limits need 0 < lo <= hi, got {lim.tolist()}")
    return int(params["half_window"]), int(params["n_frequencies"]), float(m), lim


def frequency_grid(f_start, f_stop, n_frequencies, band_margin=0.1, frequency_limits=None):
    """The frequencies (channel, frequency_index) in Hz: ``f_j = lo + j (hi - lo) / (F - 1)`` with
    ``lo = f_start + m (f_stop - f_start)`` and ``hi = f_stop - m (f_stop - f_start)``; ``F = 1`` gives the centre
    ``(lo + hi) / 2``.  ``frequency_limits`` ((lo, hi), or one pair per channel) overrides the band."""
    f0 = np.atleast_1d(np.asarray(f_start, dtype=np.float64))
    f1 = np.atleast_1d(np.asarray(f_stop, dtype=np.float64))
    F = int(n_frequencies)
    lo, hi = f0 + band_margin * (f1 - f0), f1 - band_margin * (f1 - f0)
    if frequency_limits is not None:
        lim = np.asarray(frequency_limits, dtype=np.float64).reshape(-1, 2)
        if lim.shape[0] not in (1, f0.size):
            raise ValueError(f"frequency_limits holds {lim.shape[0]} pairs for {f0.size} channels")
        lim = np.broadcast_to(lim, (f0.size, 2))
        lo, hi = lim[:, 0].copy(), lim[:, 1].copy()
    if F == 1:
        return ((lo + hi) / 2)[:, None]
    return lo[:, None] + np.arange(F, dtype=np.float64)[None, :] * (hi - lo)[:, None] / (F - 1)


def _first_valid(a):
    """Per row of a (C, P) array its first value that is not NaN (NaN if there is none)."""
    ok = ~np.isnan(a)
    first = np.where(ok.any(axis=1), ok.argmax(axis=1), 0)
    return a[np.arange(a.shape[0]), first]


def frequency_params(cal, freq, env_params=None, cal_params=None):
    """The parameters of rule 8 on the (channel, frequency) grid ``freq`` -> float64 (8, C, F) in the order of
    ``_lib.TARGET_SPECTRA_FPARAM_NAMES``.  ``cal``: the file's ``CalibrateEK80`` (its beam group and vendor group).

    ``get_cal_params_EK("BB", ...)`` and ``get_env_params_EK(..., freq=...)`` -- the routines ``compute_TS`` evaluates at
    the centre frequency -- are handed the grid in place of the centre frequency, on a stand-in beam group whose ping
    axis is the frequency axis: a file's calibration tables, the user's dictionaries and the fallbacks
    (beamwidth x f_n / f, ...) are the same rules.  The pulse-length table of the gain fallback is read at the pulse
    duration of each channel's first valid ping (the replica's: the transmit parameters do not change along a file or
    filter interval)."""
    beam, vend = cal.beam, cal.vend
    C, F = freq.shape
    P = beam["backscatter_r"].shape[1]
    pt = np.asarray(beam["ping_time"].values)
    stand = Dataset(coords={"channel": np.asarray(beam["channel"].values), "ping_time": np.repeat(pt[:1], F)})
    tau = _first_valid(cp_array(beam["transmit_duration_nominal"], C, P))
    stand["transmit_duration_nominal"] = (("channel", "ping_time"), np.repeat(tau[:, None], F, axis=1))
    for name, da in beam.data_vars.items():
        if tuple(da.dims) == ("channel",):
            stand[name] = (("channel",), np.asarray(da.values))
    grid = DataArray(np.ascontiguousarray(freq), ("channel", "ping_time"))
    env = get_env_params_EK("EK80", stand, cal.echodata["Environment"], dict(env_params or {}), freq=grid)
    calp = get_cal_params_EK("BB", grid, stand, vend, dict(cal_params or {}), sonar_type="EK80")

    def on_grid(v, name):
        dims = tuple(v.dims) if isinstance(v, DataArray) else None
        a = np.asarray(getattr(v, "values", v), dtype=np.float64)
        if dims == ("ping_time", "channel"):
            a = a.T
        if a.ndim == 1 and a.shape[0] == C and dims != ("ping_time",):
            a = a[:, None]
        try:
            return np.broadcast_to(a, (C, F))
        except ValueError:
            raise ValueError(f"{name} of shape {a.shape} cannot be evaluated on the (channel={C}, frequency={F}) grid") \
                from None

    rows = [freq, on_grid(env["sound_absorption"], "sound_absorption")]
    rows += [on_grid(calp[k], k) for k in _lib.TARGET_SPECTRA_FPARAM_NAMES[2:]]
    return np.ascontiguousarray(np.stack(rows), dtype=np.float64)


def _index_column(da, dev):
    """An index column as int32; what int32 cannot hold stays out of range instead of wrapping."""
    t = as_tensor(da, None, dev)
    if t.dtype != torch.int32:
        t = t.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    return t.contiguous()


def spectra_inputs(cal, freq, chan_map, env_params=None, cal_params=None):
    """Everything ``ops.target_spectra`` needs besides the table and ``rep_dt``, from the file's ``CalibrateEK80``:
    a dict of device tensors (``re``, ``im``, ``replica``, ``replica_off``, ``replica_id`` or None, ``fparams``,
    ``pparams``, ``chan_map``), ``max_taps`` and the host arrays ``replica_id_host`` (C, P) and ``sample_interval`` (C, P).
    The replicas are the complex64 values ``compute_TS`` uploads, picked through the same triple."""
    beam = cal.beam
    C, P = beam["backscatter_r"].shape[:2]
    _, tx = cal._transmit_replicas()
    flat, off_h, max_taps = cal._replica_arrays(tx)
    if max_taps > _lib.TARGET_SPECTRA_MAX_TAPS:
        raise ValueError(f"a replica of {max_taps} taps: target_spectra serves up to {_lib.TARGET_SPECTRA_MAX_TAPS}")
    plan = cal._plan
    rid_h = np.ascontiguousarray(plan["replica_id"]) if plan is not None else \
        np.ascontiguousarray(np.broadcast_to(np.arange(C, dtype=np.int32)[:, None], (C, P)))
    rep_chan = np.asarray([p[0] for p in plan["pairs"]], dtype=np.int64) if plan is not None else np.arange(C)
    fp = frequency_params(cal, freq, env_params, cal_params)  # (8, C, F)
    fparams = np.ascontiguousarray(fp[:, rep_chan].transpose(1, 0, 2))  # (R, 8, F)
    f64 = torch.float64
    pparams = torch.stack([cal._cp_dev(beam["transmit_power"], C, P, "transmit_power", f64),
                           cal._cp_dev(cal.env_params["sound_speed"], C, P, "sound_speed", f64),
                           cal._cp_dev(cal.cal_params["impedance_transceiver"], C, P, "impedance_transceiver", f64)])
    re, im = cal._dev(beam["backscatter_r"].data), cal._dev(beam["backscatter_i"].data)
    if re.dtype not in (torch.float32, torch.float64) or im.dtype != re.dtype:
        re, im = re.double(), im.double()
    return dict(re=re.contiguous(), im=im.contiguous(),
                replica=cal._dev(np.ascontiguousarray(flat.view(np.float32))), replica_off=cal._dev(off_h),
                replica_id=cal._dev(rid_h) if plan is not None else None,
                fparams=cal._dev(fparams), pparams=pparams.contiguous(),
                chan_map=cal._dev(np.asarray(chan_map, dtype=np.int32)),
                max_taps=max_taps, replica_id_host=rid_h,
                sample_interval=cp_array(beam["sample_interval"], C, P))


def replica_sample_interval(rid, si, hold):
    """``sample_interval`` per replica: the one value of the pings that hold targets (``hold`` (C, P) bool), of the
    replica's first ping where none does (NaN for a replica without pings).  Several values over the pings that hold
    targets raise ``ValueError``: A(f) is a function of the replica and the sample interval."""
    R = int(rid.max()) + 1 if rid.size else 0
    dt = np.full(max(R, 0), np.nan)
    for r in range(R):
        mine = rid == r
        held = si[mine & hold]
        if held.size:
            if not (held == held[0]).all():
                raise ValueError(f"sample_interval takes several values ({np.unique(held)[:4].tolist()} ...) over the pings "
                                 f"of replica {r} that hold targets: one value per replica is required")
            dt[r] = held[0]
        elif mine.any():
            dt[r] = si[mine][0]
    return dt


@xarray_io()
def target_spectra(targets, echodata, params, *, env_params=None, cal_params=None, dtype="float64", device=None):
    """The target strength spectrum TS(f) of every row of a single-target table, from the complex sector samples of an
    EK80 FM (broadband) file.

    ``targets``: the Dataset ``detect_single_targets`` returns (or ``track_targets``' input after rows were removed):
    the columns ``channel_index``, ``ping_index``, ``range_sample``, ``target_range``, ``angle_alongship``,
    ``angle_athwartship`` on ``target`` and the ``channel`` coordinate ``channel_index`` counts along, mapped BY LABEL to
    the complex beam group of ``echodata``.  ``params``: ``half_window`` (h in samples, an int from 0 to 127) and
    ``n_frequencies`` (F, an int from 1 to 1024), both required; ``band_margin`` m in [0, 0.5), default 0.1; optionally
    ``frequency_limits`` (lo, hi) in Hz, one pair or one per channel of the table, which overrides the band.  The grid
    is ``f_j = lo + j (hi - lo) / (F - 1)`` with ``lo = f_start + m (f_stop - f_start)``, ``hi = f_stop - m (f_stop -
    f_start)``; ``F = 1`` gives the centre.  An unknown key, a missing key or a non-number raises ``ValueError`` before
    any device work; so does a table channel the echodata lacks.  A file without BB complex samples raises
    ``TypeError``.  ``env_params`` / ``cal_params``: as for ``compute_TS``.  ``dtype``: the type of the two spectra
    ("float64", or "float32": the float64 result rounded once).

    Per target ``t`` of the table: ``c`` = channel, ``p`` = ``ping_index``, ``s`` = ``range_sample`` (the peak), ``r`` =
    ``target_range``, ``theta``, ``phi`` = the two angles.  Per (c, p): ``dt`` = ``sample_interval``; ``tx`` the replica of
    that ping with ``L`` taps -- the complex64 values ``compute_TS`` uploads, files with several filter intervals are
    served --; ``E = sum |tx(k)|^2``; ``B`` the size of the ``beam`` dimension.

    1. **Zero fill.** A sector is valid at sample ``n`` when both parts are not NaN.  ``z_b(n) = backscatter_r + i
       backscatter_i`` there; 0 where the sector is invalid and for ``n >= S``.
    2. **Pulse compression in the window only.** ``pc_b(n) = (1/E) sum_{k<L} z_b(n+k) conj(tx(k))`` (the formula of
       csrc/ek80_complex.hip); ``pc(n)`` is the mean of ``pc_b(n)`` over the sectors valid at ``n``; it is 0 when no
       sector is valid or ``n`` is outside ``[0, S)``, and such samples are not counted in ``n_window_samples``.
    3. **Target spectrum.** ``Y(f) = sum_{n=-h..h} pc(s+n) exp(-2 pi i f n dt)`` with ``f`` the PHYSICAL frequency in
       Hz: the samples are band-pass sampled, not demodulated, and the exponential is periodic in ``f`` with ``1/dt``,
       so the aliased band is addressed correctly.
    4. **Replica spectrum, reduced to the same window.** ``a(m) = (1/E) sum_k tx(k+m) conj(tx(k))``; ``A(f) = sum_{|m|
       <= min(h, L-1)} a(m) exp(-2 pi i f m dt)``.  ``A`` depends on the replica, ``dt``, ``h`` and ``f`` only:
       ``sample_interval`` must be one value per replica over the pings that hold targets, otherwise ``ValueError``.
    5. **Received power.** ``P(f) = B |Y/A|^2 / 8 (|z_er + z_et(f)| / z_er)^2 / z_et(f)``, ``z_er`` per channel;
       ``P <= 0`` or not finite gives NaN.
    6. **Uncompensated spectrum.** ``TS_uncomp(f) = 10 log10 P + 40 log10 r + 2 alpha(f) r - 10 log10(p_t lambda^2 /
       (16 pi^2)) - 2 G(f)`` with ``lambda = c_w(c, p) / f`` and ``p_t = transmit_power[c, p]``.  ``r <= 0`` or NaN
       gives a NaN row.  No beam term goes in here (not the transceiver term of ``compute_TS`` either).
    7. **Compensation.** ``x = 2 (theta - theta_off(f)) / bw_al(f)``, ``y`` likewise; ``B_t(f) = 6.0206 (x^2 + y^2 -
       0.18 x^2 y^2)``; ``TS(f) = TS_uncomp(f) + B_t(f)``.  NaN angles give NaN here only.
    8. **Parameters at frequency f** (``alpha``, ``G``, ``z_et``, the two beamwidths, the two offsets): evaluated by
       the routines ``compute_TS`` uses at the centre frequency, ``get_cal_params_EK("BB", ...)`` and
       ``get_env_params_EK(..., freq=...)``, handed the (channel, frequency) grid in place of the centre frequency: a
       file's calibration table, the user's dictionaries and the fallbacks (beamwidth x f_n / f, ...) are the same
       rules.  Known consequence: WITHOUT A ``gain`` TABLE IN THE FILE (or the user's ``cal_params``) THE GAIN DOES
       NOT VARY WITH ``f`` -- it is the pulse-length table's value at the replica's pulse duration.

    All arithmetic is float64 (float32 cubes convert exactly).  A row whose ``channel_index``, ``ping_index`` or
    ``range_sample`` is outside the cube, or whose ping no filter interval covers, gives a NaN row and
    ``n_window_samples`` 0; no byte outside the cubes is read whatever the table holds.

    Returns a Dataset on (target, frequency_index), resident on the device: ``TS_spectrum``, ``TS_spectrum_uncomp``,
    ``n_window_samples`` (int32 per target), ``frequency`` over (channel, frequency_index) on the host, and the table's
    ``channel`` coordinate.  An empty table gives the same variables with length 0 and no launch.  No sum depends on
    scheduling: two calls give identical results.  Device work and the one host synchronisation: see the module."""
    ds = from_xarray(targets)
    h, F, margin, limits = _check_params(params)
    td = ops.torch_dtype(dtype)
    for name in _ICOLS + _FCOLS:
        if name not in ds:
            raise ValueError(f"The target table does not contain the column {name!r}!")
    if "channel" not in ds.coords or np.ndim(ds.coords["channel"]) != 1:
        raise ValueError("The target table has no channel coordinate")
    n = int(ds["channel_index"].shape[0]) if ds["channel_index"].ndim == 1 else -1
    for name in _ICOLS + _FCOLS:
        da = ds[name]
        if tuple(da.dims) != ("target",) or da.shape != (n,):
            raise ValueError(f"{name} must be a column on target of {n} rows, got {dict(zip(da.dims, da.shape))}")
        if da.dtype.kind not in ("iu" if name in _ICOLS else "fiu"):
            raise ValueError(f"{name} holds {da.dtype.kind!r} data")
    if n >= 2 ** 31 - 1:
        raise ValueError(f"target_spectra takes fewer than 2**31 - 1 rows, got {n}")
    chan = np.asarray(getattr(ds.coords["channel"], "values", ds.coords["channel"]))

    if not isinstance(echodata, EchoData):
        echodata = as_lite_echodata(echodata)
    if echodata.sonar_model not in ("EK80", "ES80", "EA640"):
        raise TypeError(f"target_spectra needs the complex samples of EK80 FM pings, got a {echodata.sonar_model} file")
    try:
        group = retrieve_correct_beam_group(echodata, "BB", "complex")
    except RuntimeError as e:
        raise TypeError(f"File does not contain BB mode complex samples! ({e})") from None
    beam = echodata[group]
    if "backscatter_i" not in beam or beam["backscatter_r"].ndim != 4:
        raise TypeError("File does not contain BB mode complex samples!")
    have = [str(c) for c in np.asarray(beam["channel"].values).reshape(-1)]
    missing = [str(c) for c in chan if str(c) not in have]
    if missing:
        raise ValueError(f"channel(s) {missing} of the target table are not in the echodata's beam group {have}")
    chan_map = [have.index(str(c)) for c in chan]
    if limits is not None and limits.shape[0] not in (1, len(chan)):
        raise ValueError(f"frequency_limits holds {limits.shape[0]} pairs for {len(chan)} channels of the table")

    n_filter = echodata["Vendor_specific"].sizes.get("filter_time", 1)
    cal = CalibrateEK80(echodata, env_params=env_params, cal_params=cal_params, ecs_file=None, waveform_mode="BB",
                        encode_mode="complex", slice_dict={"filter_intervals": True} if n_filter > 1 else {},
                        dtype="float64", device=device)
    C, P = cal.beam["backscatter_r"].shape[:2]
    f0 = _first_valid(cp_array(cal.beam["transmit_frequency_start"], C, P))
    f1 = _first_valid(cp_array(cal.beam["transmit_frequency_stop"], C, P))
    freq = frequency_grid(f0, f1, F, margin)
    if limits is not None and len(chan):
        freq[chan_map] = frequency_grid(f0[chan_map], f1[chan_map], F, margin, limits)

    first = ds["channel_index"].data
    dev = first.tensor.device if device is None and is_device(first) else resolve_device(device)
    out = Dataset(coords={"target": np.arange(max(n, 0), dtype=np.int64), "frequency_index": np.arange(F), "channel": chan},
                  attrs={"half_window": h, "n_frequencies": F, "band_margin": margin})
    if n == 0:
        ts = torch.zeros((0, F), dtype=td, device=dev)
        tu, nw = torch.zeros((0, F), dtype=td, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    else:
        k = spectra_inputs(cal, freq, chan_map, env_params, cal_params)
        dev = k["re"].device
        ci, pi, si = (_index_column(ds[name], dev) for name in _ICOLS)
        rng, al, at = (as_tensor(ds[name], torch.float64, dev).contiguous() for name in _FCOLS)
        # which pings hold targets (rows with indices outside the cube hold none): one flag per ping, the one copy
        ok = (ci >= 0) & (ci < len(chan_map)) & (pi >= 0) & (pi < P)
        c_beam = k["chan_map"].to(torch.int64)[ci.clamp(0, len(chan_map) - 1).to(torch.int64)]
        slot = torch.where(ok, c_beam * P + pi.to(torch.int64), torch.full_like(c_beam, C * P))
        hold = torch.zeros(C * P + 1, dtype=torch.bool, device=dev)
        hold[slot] = True
        hold_h = _to_host(hold).numpy()[:C * P].reshape(C, P)
        rep_dt = replica_sample_interval(k["replica_id_host"], k["sample_interval"], hold_h)
        R = k["replica_off"].numel() - 1
        rep_dt = np.concatenate([rep_dt, np.full(R - rep_dt.size, np.nan)])[:R]
        ts, tu, nw = ops.target_spectra(k["re"], k["im"], k["replica"], k["replica_off"], k["max_taps"],
                                        cal._dev(rep_dt, torch.float64), k["fparams"], k["pparams"], h, k["chan_map"], ci,
                                        pi, si, rng, al, at, replica_id=k["replica_id"], dtype=td)
    dims = ("target", "frequency_index")
    out["TS_spectrum"] = DataArray(DeviceArray(ts), dims, attrs={"units": "dB", "long_name": "Target strength spectrum "
                                                                 "(TS re 1 m^2), compensated for the position in the beam"},
                                   name="TS_spectrum")
    out["TS_spectrum_uncomp"] = DataArray(DeviceArray(tu), dims, attrs={"units": "dB"}, name="TS_spectrum_uncomp")
    out["n_window_samples"] = DataArray(DeviceArray(nw), ("target",), name="n_window_samples")
    out["frequency"] = DataArray(np.ascontiguousarray(freq[chan_map]) if len(chan) else np.zeros((0, F)),
                                 ("channel", "frequency_index"), attrs={"units": "Hz"}, name="frequency")
    return out
