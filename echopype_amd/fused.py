"""compute_Sv -> compute_MVBS in ONE pass over the raw power samples (12 B/sample in fp64 instead of
12 + 8 for the two separate calls with echo_range left lazy, 20 + 16 with the array) -- the path BASELINE.json's
metric is quoted on.

``compute_Sv_MVBS`` takes the union of the two reference signatures (calibrate/api.py:249-345 and
commongrid/api.py:30-191) and returns ``(ds_Sv, ds_MVBS)`` exactly as the two calls would;
``ds_Sv["echo_range"]`` is lazy (an ``xr_lite.LazyDeviceArray``: written by ``epa_range_power`` when somebody
reads it; ``materialize_echo_range=True`` runs the two calls instead).  The fused kernel serves power-sample sonars
(EK60, EK80 CW power, AZFP) with the default binning flags; everything else falls back to the two
calls as well -- same results either way.
"""
import numpy as np
import torch

from . import _lib, ops
from .calibrate.api import CALIBRATOR, _compute_cal, _finalize_cal_ds
from .clean.api import remove_background_noise
from .clean.utils import add_remove_background_noise_attrs, extract_dB
from .commongrid.api import _assemble_mvbs, compute_MVBS
from .commongrid.deferred import (CPS, deferred_mvbs, launch_or_decline, n_range_bins, nan_coordinate_warning, range_cap,
                                  range_edges, sorted_time_grid, time_bin_start)
from .commongrid.utils import _parse_x_bin, resample_edges
from .utils.prov import echopype_prov_attrs, insert_processing_level
from .xr_lite import DataArray, Dataset, DeviceArray, defer_mvbs_enabled, xarray_io


@xarray_io()
def compute_Sv_MVBS(echodata, *, range_bin="20m", ping_time_bin="20s", skipna=True, fill_value=np.nan,
                    closed="left", range_var_max=None, materialize_echo_range=False, env_params=None,
                    cal_params=None, ecs_file=None, waveform_mode=None, encode_mode=None, dtype="float64",
                    device=None, _shard=None, _file=None):
    cal_kw = dict(env_params=env_params, cal_params=cal_params, ecs_file=ecs_file, waveform_mode=waveform_mode,
                  encode_mode=encode_mode, dtype=dtype, device=device)
    mv_kw = dict(range_bin=range_bin, ping_time_bin=ping_time_bin, skipna=skipna, fill_value=fill_value,
                 closed=closed, range_var_max=range_var_max, _shard=_shard)
    is_power = echodata.sonar_model in ("EK60", "ES70", "AZFP") or (
        echodata.sonar_model in ("EK80", "ES80", "EA640") and encode_mode == "power")
    fast = is_power and not materialize_echo_range and skipna and closed == "left" and \
        echodata.sonar_model != "AZFP"  # AZFP rows carry no guard/mask flags -> generic kernel, two calls
    if not fast:  # (EK80 complex samples, AZFP, other binning flags: the two calls -- on a ping shard with the file's scalars)
        ds_Sv = _compute_cal("Sv", echodata, _file=_file, **cal_kw)
        return ds_Sv, compute_MVBS(ds_Sv, **mv_kw)

    # argument checks in the reference's order (_compute_cal, then _setup_and_validate)
    if echodata.sonar_model in ("EK80", "ES80", "EA640") and (waveform_mode is None or encode_mode is None):
        raise ValueError("waveform_mode and encode_mode must be specified for EK80 calibration")
    if not isinstance(range_bin, str):
        raise TypeError("range_bin must be a string")
    range_bin_m = _parse_x_bin(range_bin, "range_bin")
    if not isinstance(ping_time_bin, str):
        raise TypeError("ping_time_bin must be a string")

    cal = CALIBRATOR[echodata.sonar_model](echodata, env_params=env_params, cal_params=cal_params,
                                           ecs_file=ecs_file, waveform_mode=waveform_mode,
                                           encode_mode=encode_mode, dtype=dtype, device=device, file_scalars=_file)
    cal._check_echodata_backscatter_size()
    raw, coef, flags, tau_eff = cal._power_inputs("Sv")
    C, P, S = raw.shape
    grid = sorted_time_grid(cal.beam["ping_time"].values, ping_time_bin)
    if grid is None:  # unsorted pings, NaT (INT64_MIN), no ping at all
        if _shard is not None:
            raise NotImplementedError("a ping shard needs sorted, valid ping times")
        ds_Sv = _compute_cal("Sv", echodata, **cal_kw)  # generic path
        return ds_Sv, compute_MVBS(ds_Sv, **mv_kw)
    ping_time, ns, e0, dt, n_t = grid
    first_bin = last_bin = 0

    # the conservative range grid (commongrid/deferred.py); the host bound: from host copies of sample_interval / sound_speed
    r_cap = range_cap(range_var_max, cal._host_reach_bound(S) if range_var_max is None else None, coef, S)
    if _shard is not None:
        # the time grid of the whole dataset (this shard covers global bins first_bin .. last_bin) and its range cap:
        # ONE control message
        e0, _, first_bin, last_bin, g_cap = _shard.grid(ns, dt, "left", r_cap if range_var_max is None else float("nan"),
                                                        sorted_valid=True)  # (checked above)
        e0, n_t = e0 + first_bin * dt, last_bin - first_bin + 1
        if range_var_max is None:
            r_cap = g_cap
    bin_start = time_bin_start(ping_time, e0, dt, n_t)
    n_cap = n_range_bins(r_cap, range_bin_m)

    def launch():  # (a degenerate grid -- one sample per ping, no valid range -- declines like the kernel would)
        return None if n_cap < 1 else ops.sv_mvbs_fused(
            raw, coef, bin_start, n_t, range_bin_m, n_cap, cal_flags=flags, skipna=True, closed="left",
            fill_value=fill_value, dtype=cal.dtype, want_range_stats=True, want_partials=_shard is not None)

    # declined: the two calls deal with it (on a shard: every rank, the collectives that follow differ)
    got = launch_or_decline(launch, shard=_shard, vote=(first_bin, last_bin, fill_value, (C, n_t, n_cap), raw.device))
    if got is None:
        ds_Sv = _compute_cal("Sv", echodata, _file=_file, **cal_kw)
        return ds_Sv, compute_MVBS(ds_Sv, **mv_kw)
    res, mv_full, lo = got
    # nanmax(echo_range) stays in HBM: on a shard it is all-reduced (MAX) there, behind the kernel; the host reads it
    # when the MVBS dataset is first used -- nothing in this call waits for the GPU
    rmax_t = res["range_max"]
    if _shard is not None and range_var_max is None:
        rmax_t = _shard.range_max_device(rmax_t)
    rmax_f = ops.fetch_async(rmax_t)  # (on its way to the host behind this kernel / all-reduce, on a side stream)
    # ... and the number of NaN echo_range values, for the reference's NaN-coordinate warning (utils.py:595-608): the
    # fused kernel counts them; the generic kernel leaves no count, there they are the NaN raw samples
    if res["range_stats_filled"]:
        nan_f = ops.fetch_async(res["range_stats"][2:3])
    else:
        nan_f = ops.fetch_async(torch.isnan(raw).sum().reshape(1)) if flags & _lib.FLAG_MASK_RANGE else None

    # (echo_range is not written: coefficient rows + the raw samples' NaN pattern; epa_range_power on first read)
    ds_Sv = _sv_dataset(cal, echodata, res["Sv"], None, raw, coef, flags, tau_eff, waveform_mode, encode_mode,
                        range_last=True)
    # off a shard a trim that cannot be done bins again from the Sv array, exactly: the public call on the snapshot
    return ds_Sv, deferred_mvbs(ds_Sv, mv_full, n_cap,
                                lambda: (float(rmax_f.item()) if range_var_max is None else r_cap,
                                         int(nan_f.item()) if nan_f is not None else 0), range_var_max,
                                r_cap, (ping_time, e0 + lo * dt, dt), "echo_range", range_bin_m, ping_time_bin,
                                fallback=(lambda ds: compute_MVBS(ds, **mv_kw)) if _shard is None else None,
                                defer=defer_mvbs_enabled())


def _sv_dataset(cal, echodata, sv_t, range_t, raw, coef, flags, tau_eff, waveform_mode, encode_mode, range_last=False):
    """The Sv dataset compute_Sv would return for the array ``sv_t`` of a power-sample calibrator: ``echo_range`` the
    array ``range_t``, or lazy (None), as after compute_Sv.  (``range_last``: the variable goes in after the
    parameters, where compute_Sv_MVBS has always had it.)"""
    ds_Sv = Dataset(coords={k: cal.beam.coords[k] for k in CPS})
    ds_Sv["Sv"] = DataArray(DeviceArray(sv_t), CPS)
    echo_range = DataArray(DeviceArray(range_t) if range_t is not None else cal._lazy_power_range(raw, coef, flags), CPS)
    if not range_last:
        ds_Sv["echo_range"] = echo_range
    if range_t is None:
        ds_Sv.attrs["echo_range_form"] = ("echo_range[c,p,s] = s * sample_interval[c,p] * sound_speed[c,p] / 2 "
                                          "(NaN where Sv input was NaN)")
    ds_Sv["sample_interval"] = cal.beam["sample_interval"]
    if tau_eff is not None:
        ds_Sv["tau_effective"] = DataArray(np.asarray(tau_eff), ("channel",))
    ds_Sv["frequency_nominal"] = cal.beam["frequency_nominal"]
    ds_Sv = cal._add_params_to_output(ds_Sv)
    if range_last:
        ds_Sv["echo_range"] = echo_range
    return _finalize_cal_ds(ds_Sv, "Sv", echodata, waveform_mode, encode_mode)


@xarray_io()
def compute_Sv_clean_MVBS(echodata, ping_num, range_sample_num, *, background_noise_max=None,
                          SNR_threshold="3.0dB", range_bin="20m", ping_time_bin="20s", skipna=True,
                          fill_value=np.nan, closed="left", range_var_max=None, keep_Sv_noise=True,
                          materialize_echo_range=False, env_params=None, cal_params=None, ecs_file=None,
                          waveform_mode=None, encode_mode=None, dtype="float64", device=None):
    """The whole north-star chain ``compute_Sv -> remove_background_noise -> compute_MVBS`` (MVBS of the
    noise-corrected ``Sv_corrected``) in TWO passes over the raw power instead of four array sweeps:

        pass 1  raw -> Sv written once, noise estimate (clean/api.py:397-422) from the values in registers
        pass 2  raw -> Sv_noise / Sv_corrected (api.py:425-430,485-487) written once, MVBS of Sv_corrected
                binned in the same sweep (commongrid/utils.py:592-627)

    24-40 B/sample in fp64 instead of 84.  Returns ``(ds_Sv, ds_MVBS)``: ``ds_Sv`` as
    ``remove_background_noise(compute_Sv(echodata), ...)`` would leave it (``Sv``, ``Sv_corrected``, ``Sv_noise``
    unless ``keep_Sv_noise=False``; ``echo_range`` lazy unless ``materialize_echo_range=True``), ``ds_MVBS`` as
    ``compute_MVBS`` of that dataset with ``Sv := Sv_corrected``.  Served for power-sample EK data with sorted
    pings; anything else runs the three separate calls -- same results either way."""
    cal_kw = dict(env_params=env_params, cal_params=cal_params, ecs_file=ecs_file, waveform_mode=waveform_mode,
                  encode_mode=encode_mode, dtype=dtype, device=device)
    mv_kw = dict(range_bin=range_bin, ping_time_bin=ping_time_bin, skipna=skipna, fill_value=fill_value,
                 closed=closed, range_var_max=range_var_max)

    def separate_calls():
        ds = _compute_cal("Sv", echodata, **cal_kw)
        remove_background_noise(ds, ping_num, range_sample_num, background_noise_max=background_noise_max,
                                SNR_threshold=SNR_threshold)
        corrected = ds.copy()
        corrected["Sv"] = ds["Sv_corrected"]
        return ds, compute_MVBS(corrected, **mv_kw)

    is_power = echodata.sonar_model in ("EK60", "ES70") or (
        echodata.sonar_model in ("EK80", "ES80", "EA640") and encode_mode == "power")
    if not is_power:
        return separate_calls()
    # argument checks in the reference's order
    if echodata.sonar_model in ("EK80", "ES80", "EA640") and (waveform_mode is None or encode_mode is None):
        raise ValueError("waveform_mode and encode_mode must be specified for EK80 calibration")
    nmax = extract_dB(background_noise_max) if background_noise_max is not None else None
    snr = extract_dB(SNR_threshold) if SNR_threshold is not None else None
    if not isinstance(range_bin, str):
        raise TypeError("range_bin must be a string")
    range_bin_m = _parse_x_bin(range_bin, "range_bin")
    if not isinstance(ping_time_bin, str):
        raise TypeError("ping_time_bin must be a string")
    if closed not in ["right", "left"]:
        raise ValueError(f"{closed} is not a valid option. Options are 'left' or 'right'.")

    cal = CALIBRATOR[echodata.sonar_model](echodata, env_params=env_params, cal_params=cal_params,
                                           ecs_file=ecs_file, waveform_mode=waveform_mode,
                                           encode_mode=encode_mode, dtype=dtype, device=device)
    cal._check_echodata_backscatter_size()
    raw, coef, flags, tau_eff = cal._power_inputs("Sv")
    ping_time = np.asarray(cal.beam["ping_time"].values).astype("datetime64[ns]")
    ns = ping_time.astype(np.int64)
    if np.any(np.diff(ns) < 0) or np.isnat(ping_time).any():
        return separate_calls()
    alpha2 = coef[..., _lib.CF_ALPHA2].contiguous()  # 2 * sound_absorption per (channel, ping)

    sv_t, _, noise, rmax, rstats = ops.sv_noise_fused(
        raw, coef, alpha2, ping_num, range_sample_num, flags=flags, dtype=cal.dtype,
        noise_max=float("nan") if nmax is None else float(nmax), want_range_max=True, want_range_stats=True)
    n_nan_range = int(rstats[2].item())  # (rmax: waited for, by design -- the grid is built from it)
    if n_nan_range < 0:  # the generic kernel leaves the maximum only: the NaN echo_range values are the NaN raw samples
        rstats = None
        n_nan_range = int(torch.isnan(raw).sum().item()) if flags & _lib.FLAG_MASK_RANGE else 0
    e0, dt, n_t = resample_edges(ping_time, ping_time_bin)
    bin_start = ops.time_bin_offsets(ops.to_device(ns), e0, dt, n_t, closed=closed)
    r_edges = range_edges(range_cap(range_var_max, rmax), range_bin_m)
    n_r = len(r_edges) - 1
    if n_r < 1:  # no valid range, or a degenerate grid: the separate calls raise / return the empty MVBS the reference would
        return separate_calls()
    try:
        res = ops.sv_denoise_mvbs(raw, coef, alpha2, noise, ping_num, float(snr), bin_start, n_t, range_bin_m,
                                  n_r, flags=flags, dtype=cal.dtype, skipna=skipna, closed=closed,
                                  fill_value=fill_value, want_noise=keep_Sv_noise,
                                  want_range=materialize_echo_range, want_minmax=True)
    except _lib.EpaError:  # e.g. a range grid too fine for the LDS accumulators
        return separate_calls()

    ds_Sv = _sv_dataset(cal, echodata, sv_t, res["echo_range"] if materialize_echo_range else None, raw, coef, flags,
                        tau_eff, waveform_mode, encode_mode)
    mm = res["minmax"]  # actual_range of both outputs comes out of the kernel: no extra sweep
    outs = [("Sv_corrected", res["Sv_corrected"], "corrected", mm[2:4])]
    if keep_Sv_noise:
        outs.insert(0, ("Sv_noise", res["Sv_noise"], "noise", mm[0:2]))
    for name, t, kind, rng_mm in outs:  # clean/api.py:490-502
        ds_Sv[name] = add_remove_background_noise_attrs(DataArray(DeviceArray(t), CPS), kind, ping_num,
                                                        range_sample_num, snr, nmax, rng_mm)
    prov = echopype_prov_attrs(process_type="processing")
    prov["processing_function"] = "clean.remove_background_noise"
    ds_Sv.attrs.update(prov)
    ds_Sv = insert_processing_level(ds_Sv, "L*B", input_ds=ds_Sv)
    if rstats is not None and not materialize_echo_range:  # (the lazy echo_range carries what pass 1 found)
        ds_Sv["echo_range"].data.set_stats(rstats)
    if n_nan_range > 0:
        nan_coordinate_warning("echo_range")
    ds_MVBS = _assemble_mvbs(ds_Sv, res["MVBS"], "channel", ping_time, e0, dt, n_t, r_edges, "echo_range",
                             range_bin_m, ping_time_bin, closed)
    return ds_Sv, ds_MVBS
