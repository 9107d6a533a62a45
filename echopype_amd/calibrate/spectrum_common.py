"""What the two broadband spectrum products share on the host (``targets.target_spectra``: TS(f) of single targets;
``calibrate.compute_Sv_spectrum``: Sv(f) of range cells): the frequency grid and its parameter checks, the calibration
and environment parameters evaluated on the (channel, frequency) grid, the file checks, and the replicas and sample
cubes as the kernels take them.  One definition each."""
import numbers

import numpy as np
import torch

from .. import _lib
from ..echodata import EchoData, as_lite_echodata
from ..xr_lite import DataArray, Dataset
from .cal_params import get_cal_params_EK
from .calibrate_base import cp_array
from .calibrate_ek import CalibrateEK80, retrieve_correct_beam_group
from .env_params import get_env_params_EK


def _is_real(v):
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (numbers.Real, np.integer, np.floating)) \
        and np.isfinite(float(v))


def check_int(params, key, lo, hi):
    """``params[key]`` as an int in ``lo .. hi`` (``ValueError`` otherwise)."""
    v = params[key]
    if not _is_real(v) or float(v) != int(v) or not lo <= int(v) <= hi:
        raise ValueError(f"{key} must be an integer from {lo} to {hi}, got {v!r}")
    return int(v)


def check_band(params):
    """``band_margin`` and ``frequency_limits`` of ``params``, checked on the host -> (band_margin, frequency_limits as a
    float64 (n, 2) array or None)."""
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
    return float(m), lim


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


def frequency_params(cal, freq, env_params=None, cal_params=None, names=_lib.TARGET_SPECTRA_FPARAM_NAMES):
    """The parameters that vary with frequency on the (channel, frequency) grid ``freq`` -> float64 (len(names), C, F) in
    the order of ``names`` (``frequency``, ``sound_absorption``, then calibration parameters by name).  ``cal``: the
    file's ``CalibrateEK80`` (its beam group and vendor group).

    ``get_cal_params_EK("BB", ...)`` and ``get_env_params_EK(..., freq=...)`` -- the routines ``compute_TS`` evaluates at
    the centre frequency -- are handed the grid in place of the centre frequency, on a stand-in beam group whose ping
    axis is the frequency axis: a file's calibration tables, the user's dictionaries and the fallbacks
    (beamwidth x f_n / f, psi + 20 log10(f_n / f), ...) are the same rules.  The pulse-length table of the gain fallback is
    read at the pulse duration of each channel's first valid ping (the replica's: the transmit parameters do not change
    along a file or filter interval)."""
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
    rows += [on_grid(calp[k], k) for k in names[2:]]
    return np.ascontiguousarray(np.stack(rows), dtype=np.float64)


def fm_beam_group(echodata, who):
    """(echodata as an ``EchoData``, its beam group of BB complex samples); ``TypeError`` for a file without them."""
    if not isinstance(echodata, EchoData):
        echodata = as_lite_echodata(echodata)
    if echodata.sonar_model not in ("EK80", "ES80", "EA640"):
        raise TypeError(f"{who} needs the complex samples of EK80 FM pings, got a {echodata.sonar_model} file")
    try:
        group = retrieve_correct_beam_group(echodata, "BB", "complex")
    except RuntimeError as e:
        raise TypeError(f"File does not contain BB mode complex samples! ({e})") from None
    beam = echodata[group]
    if "backscatter_i" not in beam or beam["backscatter_r"].ndim != 4:
        raise TypeError("File does not contain BB mode complex samples!")
    return echodata, beam


def fm_calibrator(echodata, env_params=None, cal_params=None, device=None):
    """The file's ``CalibrateEK80`` for BB complex samples in float64, with the filter-interval plan when the file holds
    several ``filter_time``s."""
    n_filter = echodata["Vendor_specific"].sizes.get("filter_time", 1)
    return CalibrateEK80(echodata, env_params=env_params, cal_params=cal_params, ecs_file=None, waveform_mode="BB",
                         encode_mode="complex", slice_dict={"filter_intervals": True} if n_filter > 1 else {},
                         dtype="float64", device=device)


def band_edges(cal):
    """(f_start, f_stop) per channel: the values of each channel's first valid ping."""
    C, P = cal.beam["backscatter_r"].shape[:2]
    return (_first_valid(cp_array(cal.beam["transmit_frequency_start"], C, P)),
            _first_valid(cp_array(cal.beam["transmit_frequency_stop"], C, P)))


def replica_plan(cal):
    """Host data only: (``replica_id`` int32 (C, P): the replica of every ping, -1 where no filter interval covers it;
    ``rep_chan`` (R,): the channel of every replica; ``sample_interval`` (C, P))."""
    beam = cal.beam
    C, P = beam["backscatter_r"].shape[:2]
    plan = cal._plan
    rid_h = np.ascontiguousarray(plan["replica_id"]) if plan is not None else \
        np.ascontiguousarray(np.broadcast_to(np.arange(C, dtype=np.int32)[:, None], (C, P)))
    rep_chan = np.asarray([p[0] for p in plan["pairs"]], dtype=np.int64) if plan is not None else np.arange(C)
    return rid_h, rep_chan, cp_array(beam["sample_interval"], C, P)


def replica_inputs(cal, who, max_taps_served):
    """The sample cubes and replicas as the spectrum kernels take them, from the file's ``CalibrateEK80``: a dict of the
    device tensors ``re``, ``im``, ``replica``, ``replica_off``, ``replica_id`` (or None), of ``max_taps`` and of the host
    arrays of ``replica_plan``: ``replica_id_host``, ``rep_chan`` and ``sample_interval``.
    The replicas are the complex64 values ``compute_TS`` uploads, picked through the same triple."""
    beam = cal.beam
    _, tx = cal._transmit_replicas()
    flat, off_h, max_taps = cal._replica_arrays(tx)
    if max_taps > max_taps_served:
        raise ValueError(f"a replica of {max_taps} taps: {who} serves up to {max_taps_served}")
    rid_h, rep_chan, si = replica_plan(cal)
    re, im = cal._dev(beam["backscatter_r"].data), cal._dev(beam["backscatter_i"].data)
    if re.dtype not in (torch.float32, torch.float64) or im.dtype != re.dtype:
        re, im = re.double(), im.double()
    return dict(re=re.contiguous(), im=im.contiguous(),
                replica=cal._dev(np.ascontiguousarray(flat.view(np.float32))), replica_off=cal._dev(off_h),
                replica_id=cal._dev(rid_h) if cal._plan is not None else None, max_taps=max_taps, replica_id_host=rid_h,
                rep_chan=rep_chan, sample_interval=si)


def replica_sample_interval(rid, si, hold, what="that hold targets"):
    """``sample_interval`` per replica: the one value of the pings that count (``hold`` (C, P) bool), of the replica's
    first ping where none does (NaN for a replica without pings).  Several values over the pings that count raise
    ``ValueError``: A(f) is a function of the replica and the sample interval."""
    R = int(rid.max()) + 1 if rid.size else 0
    dt = np.full(max(R, 0), np.nan)
    for r in range(R):
        mine = rid == r
        held = si[mine & hold]
        if held.size:
            if not (held == held[0]).all():
                raise ValueError(f"sample_interval takes several values ({np.unique(held)[:4].tolist()} ...) over the pings "
                                 f"of replica {r} {what}: one value per replica is required")
            dt[r] = held[0]
        elif mine.any():
            dt[r] = si[mine][0]
    return dt
