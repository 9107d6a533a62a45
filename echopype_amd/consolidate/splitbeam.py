"""consolidate.add_splitbeam_angle -- split-beam (alongship / athwartship) angles of every sample
(reference: /root/reference/echopype/consolidate/api.py:345-560 and consolidate/split_beam_angle.py).

Host Python does what is O(C) or O(C*P): the reference's checks in its order and with its exception types, the beam
group, the beam types, the angle parameters and -- broadband with pulse compression -- the transmit replicas
(calibrate/ek80_complex.py: get_filter_coeff, get_transmit_signal).  The (channel, ping_time, range_sample) pass is
one kernel launch (csrc/splitbeam.hip): epa_splitbeam_power for power/angle samples, epa_splitbeam_complex[_fft] for
complex samples.  The two angle arrays stay in HBM (xr_lite device arrays), copied to the host when read.
"""
import datetime
import logging
import pathlib

import numpy as np
import torch

from .. import ops
from ..device_view import device_view, resolve_device
from ..calibrate.calibrate_ek import retrieve_correct_beam_group
from ..calibrate.ek80_complex import get_filter_coeff, get_transmit_signal
from ..echodata import EchoData, as_lite_echodata
from ..xr_lite import DataArray, Dataset, DeviceArray, from_xarray, xarray_io

logger = logging.getLogger("echopype_amd.consolidate")

_SONARS = ("EK60", "ES70", "EK80", "ES80", "EA640")
_DIMS = ("channel", "ping_time", "range_sample")


def _no_paths(obj, what):
    if isinstance(obj, (str, pathlib.Path)):
        raise NotImplementedError(f"{what} given as a file path is not supported: pass the Dataset / EchoData")


def _channel_index(ds_beam, channels):
    """Positions of ``channels`` along the beam group's channel axis (ds_beam.sel(channel=...)); None = all, in order."""
    have = [str(c) for c in np.asarray(ds_beam["channel"].values)]
    want = [str(c) for c in np.asarray(channels)]
    if want == have:
        return None
    missing = [c for c in want if c not in have]
    if missing:
        raise KeyError(f"channels {missing} of source_Sv are not in the beam group")
    return [have.index(c) for c in want]


def _samples(da, idx, device):
    """A beam-group variable as a device tensor, channels picked by ``idx`` (read where it lives after to_device())."""
    return device_view(da, _DIMS + ("beam",), device=device, index=idx)


def _param(da, device):
    """An angle parameter of source_Sv (scalar, (channel,) or (channel, ping_time)) as an f64 device tensor."""
    return device_view(da, ("channel", "ping_time"), device=device, dtype=torch.float64)


def _complex_beam_types(ds_beam):
    """Per-channel beam types for the kernel (-1: skipped), with the reference's rules (split_beam_angle.py:240-264):
    one type for every channel -> it must be supported (97: NotImplementedError, other: ValueError); mixed types ->
    unsupported channels are skipped with a warning and come out as NaN rows."""
    bt = np.asarray(ds_beam["beam_type"].values).reshape(-1).astype(np.int64)
    uniq = np.unique(bt)
    if uniq.size == 1:
        if int(uniq[0]) == 97:
            raise NotImplementedError
        if int(uniq[0]) not in ops.SPLITBEAM_BEAM_TYPES:
            raise ValueError("beam_type not recognized!")
        return bt.astype(np.int32)
    chans = np.asarray(ds_beam["channel"].values)
    out = bt.copy()
    for k, (ch, t) in enumerate(zip(chans, bt)):
        if int(t) not in ops.SPLITBEAM_BEAM_TYPES:
            logger.warning(f"Skipping channel {ch}: unsupported beam_type {int(t)}")
            out[k] = -1
    return out.astype(np.int32)


def _replicas(echodata, ds_beam, source_Sv, channels, drop_last_hanning_zero, device):
    """The transmit replica of every channel as get_angle_complex_samples builds it (split_beam_angle.py:208-219 with
    api.py:504-514): filter coefficients from Vendor_specific, fs = source_Sv["receiver_sampling_frequency"]."""
    vend = echodata["Vendor_specific"]
    vidx = _channel_index(vend, channels)
    if vidx is not None:
        vend = vend.isel(channel=vidx)
    coeff = get_filter_coeff(vend)
    tx, _ = get_transmit_signal(ds_beam, coeff, "BB", source_Sv["receiver_sampling_frequency"],
                                drop_last_hanning_zero)
    taps = [np.asarray(tx[ch]) for ch in np.asarray(ds_beam["channel"].values)]
    off = np.concatenate([[0], np.cumsum([t.size for t in taps])]).astype(np.int32)
    flat = np.concatenate(taps).astype(np.complex64)
    rep = ops.to_device(np.ascontiguousarray(flat.view(np.float32)), device=device)
    return rep, ops.to_device(off, device=device), int(max(t.size for t in taps))


@xarray_io(in_place=("angle_alongship", "angle_athwartship"))
def add_splitbeam_angle(source_Sv, echodata, waveform_mode, encode_mode, pulse_compression=False, storage_options={},
                        to_disk=True, drop_last_hanning_zero=False, *, dtype=None, device=None, fft_dtype=None):
    """Add ``angle_alongship`` / ``angle_athwartship`` (channel, ping_time, range_sample) to an Sv dataset (in place,
    like the reference) and return it.  ``source_Sv`` / ``echodata`` given as paths are not supported (this package
    does no file I/O).  Keyword-only extras: ``dtype`` of the angles (float64 as the reference; float32 halves the
    bytes written), ``device``, ``fft_dtype`` (arithmetic of the FFT form of the pulse compression, default float64)."""
    if not isinstance(source_Sv, (str, pathlib.Path)) and to_disk:
        raise ValueError("The input source_Sv must be a path when to_disk=True, "
                         "so that the split-beam angles can be written to disk!")
    _no_paths(source_Sv, "source_Sv")
    _no_paths(echodata, "echodata")
    source_Sv = from_xarray(source_Sv)
    if not isinstance(echodata, EchoData):
        echodata = as_lite_echodata(echodata)
    if echodata.sonar_model not in _SONARS:
        raise ValueError("The sonar model that produced echodata does not have split-beam "
                         "transducers, split-beam angles cannot be added to source_Sv!")
    if source_Sv.attrs.get("processing_function") == "commongrid.compute_MVBS":
        raise NotImplementedError("Adding split-beam data to MVBS has not been implemented!")
    ed_beam_group = retrieve_correct_beam_group(echodata, waveform_mode, encode_mode)
    if "channel" not in source_Sv.variables:
        raise ValueError("The input source_Sv Dataset must have a channel dimension!")
    channels = np.asarray(source_Sv["channel"].values)
    ds_full = echodata[ed_beam_group]
    idx = _channel_index(ds_full, channels)
    # ds_beam.sel(channel=source_Sv.channel) of the per-channel / per-ping variables (the sample planes are picked on
    # the device by _samples: never copied to the host for a selection)
    ds_beam = ds_full
    if idx is not None:
        ds_beam = Dataset(coords={k: c for k, c in ds_full.coords.items()}, attrs=dict(ds_full.attrs))
        for k, v in ds_full.data_vars.items():
            if v.ndim <= 2:
                ds_beam[k] = v
        ds_beam = ds_beam.isel(channel=idx)
    params = {}
    for name in ops.SPLITBEAM_PARAMS:
        if name not in source_Sv:
            raise ValueError(f"source_Sv does not contain the necessary parameter {name}!")
        params[name] = source_Sv[name]

    # the rest of the reference's checks are host work too: nothing is allocated on the device before they pass
    power = waveform_mode == "CW" and encode_mode == "power"
    if power:
        if np.all(np.asarray(ds_beam["beam_type"].values) == 0):
            raise ValueError("Computing physical split-beam angle is only available for data "
                             "from split-beam transducers!")
    else:
        bt = _complex_beam_types(ds_beam)

    dev = resolve_device(device)
    out_dt = ops.torch_dtype(dtype) if dtype is not None else torch.float64
    prm = [_param(params[n], dev) for n in ops.SPLITBEAM_PARAMS]
    if power:
        along = _samples(ds_full["angle_alongship"], idx, dev)
        athw = _samples(ds_full["angle_athwartship"], idx, dev)
        if along.dtype not in (torch.int8, torch.float32, torch.float64):
            along, athw = along.double(), athw.double()
        theta, phi = ops.splitbeam_power(along, athw, prm, dtype=out_dt)
    else:
        re = _samples(ds_full["backscatter_r"], idx, dev)
        im = _samples(ds_full["backscatter_i"], idx, dev)
        if re.dtype not in (torch.float32, torch.float64):
            re, im = re.double(), im.double()
        rep = off = None
        max_taps = 0
        if waveform_mode == "BB" and pulse_compression:
            rep, off, max_taps = _replicas(echodata, ds_beam, source_Sv, channels, drop_last_hanning_zero, dev)
        theta, phi = ops.splitbeam_complex(re, im, bt, prm, replica=rep, replica_off=off, max_taps=max_taps,
                                           dtype=out_dt, fft_dtype=fft_dtype)

    now = datetime.datetime.now(datetime.timezone.utc)
    history = f"{now}. `depth` calculated using:Calculated using data stored in the Beam groups of the echodata object."
    for name, t, long_name in (("angle_alongship", theta, "split-beam alongship angle"),
                               ("angle_athwartship", phi, "split-beam athwartship angle")):
        source_Sv[name] = DataArray(DeviceArray(t), _DIMS, attrs={"long_name": long_name, "history": history}, name=name)
    return source_Sv
