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
import numpy as np
import torch

from .. import _lib, ops
from ..calibrate.spectrum_common import (_first_valid, band_edges, check_band, check_int, fm_beam_group,  # noqa: F401
                                         fm_calibrator, frequency_grid, frequency_params, replica_inputs,
                                         replica_sample_interval)
from ..device_view import as_tensor, resolve_device
from ..xr_lite import DataArray, Dataset, DeviceArray, from_xarray, is_device, xarray_io

_REQUIRED = ("half_window", "n_frequencies")
_OPTIONAL = ("band_margin", "frequency_limits")
_ICOLS = ("channel_index", "ping_index", "range_sample")
_FCOLS = ("target_range", "angle_alongship", "angle_athwartship")


def _to_host(t):
    """The one place this module copies device data to the host (a synchronisation: the tests count them)."""
    return t.cpu()


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
    h = check_int(params, "half_window", 0, _lib.TARGET_SPECTRA_MAX_HALF_WINDOW)
    F = check_int(params, "n_frequencies", 1, _lib.TARGET_SPECTRA_MAX_FREQ)
    m, lim = check_band(params)
    return h, F, m, lim


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
    k = replica_inputs(cal, "target_spectra", _lib.TARGET_SPECTRA_MAX_TAPS)
    fp = frequency_params(cal, freq, env_params, cal_params)  # (8, C, F)
    fparams = np.ascontiguousarray(fp[:, k.pop("rep_chan")].transpose(1, 0, 2))  # (R, 8, F)
    f64 = torch.float64
    pparams = torch.stack([cal._cp_dev(beam["transmit_power"], C, P, "transmit_power", f64),
                           cal._cp_dev(cal.env_params["sound_speed"], C, P, "sound_speed", f64),
                           cal._cp_dev(cal.cal_params["impedance_transceiver"], C, P, "impedance_transceiver", f64)])
    return dict(k, fparams=cal._dev(fparams), pparams=pparams.contiguous(),
                chan_map=cal._dev(np.asarray(chan_map, dtype=np.int32)))


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

    echodata, beam = fm_beam_group(echodata, "target_spectra")
    have = [str(c) for c in np.asarray(beam["channel"].values).reshape(-1)]
    missing = [str(c) for c in chan if str(c) not in have]
    if missing:
        raise ValueError(f"channel(s) {missing} of the target table are not in the echodata's beam group {have}")
    chan_map = [have.index(str(c)) for c in chan]
    if limits is not None and limits.shape[0] not in (1, len(chan)):
        raise ValueError(f"frequency_limits holds {limits.shape[0]} pairs for {len(chan)} channels of the table")

    cal = fm_calibrator(echodata, env_params, cal_params, device)
    C, P = cal.beam["backscatter_r"].shape[:2]
    f0, f1 = band_edges(cal)
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
