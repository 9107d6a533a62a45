"""Volume backscattering spectra: Sv(f) of range cells of an EK80 FM (broadband) file -- the frequency response of
layers and aggregations, what separates krill, mesopelagic layers and swimbladdered fish where no individual can be
resolved (no counterpart in the reference; on the host this is a Python loop over pings and range cells, in torch a
gather of overlapping windows many times the size of the input).

``compute_Sv_spectrum`` is the volume half of what ``targets.target_spectra`` does for single targets, from the same
pieces: the complex sector samples, the matched-filter replicas of ``calibrate/ek80_complex.py`` and the rules that
evaluate calibration and environment parameters at a frequency (``calibrate/spectrum_common.py``).  The rules are THIS
PROJECT'S restatement of Andersen et al., "Quantitative processing of broadband data as implemented in a scientific
split-beam echosounder" (2021); they have never been run against Echoview or the CRIMAC code, nor on recorded data.
``tests/sv_spectrum_ref.py`` restates them in NumPy and is the judge of the kernel.

Device work (csrc/sv_spectrum.hip, ``epa_sv_spectrum``): one small kernel per call that leaves, per replica and
frequency, the Fourier step and 1 / |A(f)|^2, then one kernel with a workgroup per (ping, tile of consecutive cells):
the span of the tile is pulse-compressed in LDS and shared by its overlapping cells; no compressed cube goes to HBM.
Host work: the O(C F) parameter tables and the window.  Host synchronisations: none -- ``sample_interval``, the
filter-interval plan and the parameter tables are host data."""
import math

import numpy as np
import torch

from .. import _lib, ops
from ..xr_lite import DataArray, Dataset, DeviceArray, xarray_io
from .spectrum_common import (band_edges, check_band, check_int, fm_beam_group, fm_calibrator, frequency_grid,
                              frequency_params, replica_inputs, replica_plan, replica_sample_interval)

_REQUIRED = ("window_samples", "n_frequencies")
_OPTIONAL = ("step_samples", "window", "band_margin", "frequency_limits")
WINDOWS = ("hann", "rectangular")


def _check_params(params):
    """The keys and numbers of ``params``, checked on the host -> (window_samples, n_frequencies, step_samples, window,
    band_margin, frequency_limits as a float64 (n, 2) array or None)."""
    if not isinstance(params, dict):
        raise ValueError(f"params must be a dict, got {type(params).__name__}")
    unknown = sorted(k for k in params if k not in _REQUIRED + _OPTIONAL)
    if unknown:
        raise ValueError(f"Unknown Sv-spectrum parameter(s) {unknown}; known: {sorted(_REQUIRED + _OPTIONAL)}")
    missing = [k for k in _REQUIRED if k not in params]
    if missing:
        raise ValueError(f"Missing Sv-spectrum parameter(s) {missing}")
    Nw = check_int(params, "window_samples", 2, _lib.SV_SPECTRUM_MAX_WINDOW)
    F = check_int(params, "n_frequencies", 1, _lib.SV_SPECTRUM_MAX_FREQ)
    hop = check_int(params, "step_samples", 1, 2 ** 31 - 2) if "step_samples" in params else -(-Nw // 2)
    window = params.get("window", "hann")
    if not isinstance(window, str) or window not in WINDOWS:
        raise ValueError(f"window must be one of {list(WINDOWS)}, got {window!r}")
    if window == "hann" and Nw == 2:
        raise ValueError("the hann window of 2 samples is zero at both: window_samples >= 3, or window='rectangular'")
    m, lim = check_band(params)
    return Nw, F, hop, window, m, lim


def normalised_window(window_samples, window="hann"):
    """Rule 4: ``w~ = w / sqrt(sum w^2 / N_w)`` in float64, ``w(k) = 0.5 (1 - cos(2 pi k / (N_w - 1)))`` ("hann") or 1
    ("rectangular"); ``sum w~^2 = N_w``."""
    n = int(window_samples)
    if window == "hann":
        w = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / (n - 1)))
    elif window == "rectangular":
        w = np.ones(n, dtype=np.float64)
    else:
        raise ValueError(f"window must be one of {list(WINDOWS)}, got {window!r}")
    return w / math.sqrt(float(np.sum(w * w)) / n)


@xarray_io()
def compute_Sv_spectrum(echodata, params, *, env_params=None, cal_params=None, dtype="float64", device=None):
    """The volume backscattering spectrum Sv(f) of every range cell of every ping, from the complex sector samples of an
    EK80 FM (broadband) file.

    ``params``: ``window_samples`` (N_w, an int from 2 to 1024) and ``n_frequencies`` (F, an int from 1 to 1024), both
    required; ``step_samples`` (hop, an int >= 1, default ``ceil(N_w / 2)``); ``window``: "hann" (default) or
    "rectangular" (the Hann window of 2 samples is all zero and raises ``ValueError``); ``band_margin`` m in [0, 0.5),
    default 0.1, and optionally ``frequency_limits`` (lo, hi) in Hz, one
    pair or one per channel, exactly as in ``targets.target_spectra``: the grid is ``f_j = lo + j (hi - lo) / (F - 1)``
    with ``lo = f_start + m (f_stop - f_start)``, ``hi = f_stop - m (f_stop - f_start)``; ``F = 1`` gives the centre.
    An unknown key, a missing key or a non-number raises ``ValueError`` before any device work.  A file without BB
    complex samples raises ``TypeError``; pings shorter than the window (``S < N_w``) raise ``ValueError``.
    ``env_params`` / ``cal_params``: as for ``compute_Sv``.  ``dtype``: the type of the spectra ("float64", or
    "float32": the float64 result rounded once).

    Per (channel c, ping p): ``dt`` = ``sample_interval``; ``tx`` the replica of that ping with ``L`` taps -- the
    complex64 values ``compute_TS`` uploads, files with several filter intervals are served --; ``E = sum |tx(k)|^2``;
    ``B`` the size of the ``beam`` dimension; ``c_w`` the sound speed; ``p_t`` = ``transmit_power``.  A ping has
    ``M = floor((S - N_w) / hop) + 1`` cells.

    1. **Zero fill.** A sector is valid at sample ``n`` when both parts are not NaN.  ``z_b(n) = backscatter_r + i
       backscatter_i`` there; 0 where the sector is invalid and for ``n >= S``.
    2. **Pulse compression of the whole row.** ``pc_b(n) = (1/E) sum_{k<L} z_b(n+k) conj(tx(k))`` (the formula of
       csrc/ek80_complex.hip); ``pc(n)`` is the mean of ``pc_b(n)`` over the sectors valid at ``n``.  Sample ``n`` is
       VALID when at least one sector is valid at ``n``.
    3. **Spreading.** ``r(n) = n dt c_w / 2`` (the float64 expression behind ``echo_range`` of
       ``compute_Sv(waveform_mode="BB")``); ``ps(n) = r(n) pc(n)``.
    4. **Cells and window.** Cell ``m`` holds the samples ``n_m + k``, ``n_m = m hop``, ``k = 0 .. N_w - 1``.  Hann:
       ``w(k) = 0.5 (1 - cos(2 pi k / (N_w - 1)))``; rectangular: ``w = 1``.  ``w~ = w / sqrt(sum w^2 / N_w)``, so that
       ``sum w~^2 = N_w``; the host computes it in float64 (``normalised_window``) and the kernel takes it as a table.
    5. **Cell spectrum.** ``Y_m(f) = sum_k w~(k) ps(n_m + k) exp(-2 pi i f k dt)`` with ``f`` the PHYSICAL frequency in
       Hz: the samples are band-pass sampled, not demodulated, and the exponential is periodic in ``f`` with ``1/dt``,
       so the aliased band is addressed correctly.
    6. **Replica spectrum, reduced to the window.** ``a(j) = (1/E) sum_k tx(k+j) conj(tx(k))``; ``A(f) = sum_{|j| <=
       min(floor((N_w - 1) / 2), L - 1)} a(j) exp(-2 pi i f j dt)``.  ``A`` depends on the replica, ``dt``, ``N_w`` and
       ``f`` only: ``sample_interval`` must be one value per replica over ALL the pings the replica covers, otherwise
       ``ValueError``.
    7. **Received power.** ``P_m(f) = B |Y_m / A|^2 / 8 (|z_er + z_et(f)| / z_er)^2 / z_et(f)``, ``z_er`` per channel;
       ``P <= 0`` or not finite gives NaN.
    8. **Sv(f).** ``Sv_m(f) = 10 log10 P + 2 alpha(f) r_m - 10 log10(p_t lambda^2 c_w / (32 pi^2)) - 2 G(f) - 10 log10(N_w
       dt) - Psi(f)`` with ``lambda = c_w / f`` and ``r_m = (r(n_m) + r(n_m + N_w - 1)) / 2``, which is also the
       ``echo_range`` output.
    9. **Parameters at frequency f** (``alpha``, ``G``, ``z_et``, ``Psi``): evaluated by the routines ``compute_Sv`` uses
       at the centre frequency, ``get_cal_params_EK("BB", ...)`` and ``get_env_params_EK(..., freq=...)``, handed the
       (channel, frequency) grid in place of the centre frequency: a file's calibration table, the user's dictionaries
       and the fallbacks are the same rules; ``Psi(f) = Psi_nominal + 20 log10(f_nominal / f)`` is the existing
       ``equivalent_beam_angle`` rule.  Known consequence: WITHOUT A ``gain`` TABLE IN THE FILE (or the user's
       ``cal_params``) THE GAIN DOES NOT VARY WITH ``f`` -- it is the pulse-length table's value at the replica's pulse
       duration.
    10. **Validity.** A cell is NaN at every ``f`` -- its ``echo_range`` is still written -- when any of its ``N_w``
        samples is not valid (the NaN tail of a padded ping), when ``r_m <= 0``, or when no filter interval covers its
        ping (``replica_id`` -1).  A cell that ends on the last valid sample of a ping is finite: the taps reaching past
        it zero-fill, as in ``compute_Sv``.

    All arithmetic is float64 (float32 cubes convert exactly).  No sum depends on scheduling: two calls give identical
    bits.  No byte outside the cubes is read.

    Returns a Dataset resident on the device: ``Sv_spectrum`` on (channel, ping_time, range_bin, frequency_index) in
    ``dtype``, ``echo_range`` on (channel, ping_time, range_bin) in float64 (the cell centres ``r_m``), ``frequency`` on
    (channel, frequency_index) on the host, and the parameters as attrs.  Cells are not averaged over pings (average
    ``10^(Sv/10)``).  Device work and host synchronisations (none): see the module."""
    Nw, F, hop, window, margin, limits = _check_params(params)
    td = ops.torch_dtype(dtype)
    echodata, beam = fm_beam_group(echodata, "compute_Sv_spectrum")
    C, P, S = (int(v) for v in beam["backscatter_r"].shape[:3])
    if S < Nw:
        raise ValueError(f"window_samples {Nw} is larger than the {S} samples of a ping")
    if limits is not None and limits.shape[0] not in (1, C):
        raise ValueError(f"frequency_limits holds {limits.shape[0]} pairs for {C} channels")
    win = normalised_window(Nw, window)

    cal = fm_calibrator(echodata, env_params, cal_params, device)
    f0, f1 = band_edges(cal)
    freq = frequency_grid(f0, f1, F, margin, limits)
    rid_h, _, si = replica_plan(cal)
    rep_dt = replica_sample_interval(rid_h, si, np.ones((C, P), dtype=bool), "it covers")  # (before any device work)
    k = replica_inputs(cal, "compute_Sv_spectrum", _lib.SV_SPECTRUM_MAX_TAPS)
    R = k["replica_off"].numel() - 1
    rep_dt = np.concatenate([rep_dt, np.full(max(R - rep_dt.size, 0), np.nan)])[:R]
    fp = frequency_params(cal, freq, env_params, cal_params, names=_lib.SV_SPECTRUM_FPARAM_NAMES)  # (5, C, F)
    fparams = np.ascontiguousarray(fp[:, k["rep_chan"]].transpose(1, 0, 2))  # (R, 5, F)
    f64 = torch.float64
    pparams = torch.stack([cal._cp_dev(cal.beam["transmit_power"], C, P, "transmit_power", f64),
                           cal._cp_dev(cal.env_params["sound_speed"], C, P, "sound_speed", f64),
                           cal._cp_dev(cal.cal_params["impedance_transceiver"], C, P, "impedance_transceiver", f64),
                           cal._dev(np.ascontiguousarray(si, dtype=np.float64), f64)]).contiguous()
    sv, rng = ops.sv_spectrum(k["re"], k["im"], k["replica"], k["replica_off"], k["max_taps"], cal._dev(rep_dt, f64),
                              cal._dev(fparams), pparams, cal._dev(win, f64), hop, replica_id=k["replica_id"], dtype=td)
    M = sv.shape[2]
    out = Dataset(coords={"channel": np.asarray(cal.beam["channel"].values), "ping_time": cal.beam["ping_time"].values,
                          "range_bin": np.arange(M, dtype=np.int64), "frequency_index": np.arange(F)},
                  attrs={"window_samples": Nw, "n_frequencies": F, "step_samples": hop, "window": window,
                         "band_margin": margin})
    out["Sv_spectrum"] = DataArray(DeviceArray(sv), ("channel", "ping_time", "range_bin", "frequency_index"),
                                   attrs={"units": "dB", "long_name": "Volume backscattering strength spectrum "
                                          "(Sv re 1 m-1)"}, name="Sv_spectrum")
    out["echo_range"] = DataArray(DeviceArray(rng), ("channel", "ping_time", "range_bin"), attrs={"units": "m"},
                                  name="echo_range")
    out["frequency"] = DataArray(np.ascontiguousarray(freq), ("channel", "frequency_index"), attrs={"units": "Hz"},
                                 name="frequency")
    return out
