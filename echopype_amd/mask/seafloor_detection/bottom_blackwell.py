"""mask.detect_seafloor(method="blackwell") (reference: echopype mask/seafloor_detection/bottom_blackwell.py;
Blackwell et al. 2019, "Aliased seabed detection in fisheries acoustic data", arXiv:1904.10736)."""
import warnings

import numpy as np
import torch

from ... import ops
from ...xr_lite import DataArray, DeviceArray, xarray_io
from ...device_view import channel_position
from . import utils
from .utils import _channel_plane, _check_inputs, _parse_blackwell_thresholds


def _log2lin(data):
    return 10 ** (data / 10)


def _lin2log(data):
    return 10 * np.log10(data)


_STATE_MASKED, _STATE_COUNT, _STATE_LO, _STATE_HI, _STATE_ERROR = 0, 1, 6, 7, 8


def _median_threshold(state_host, dtype):
    """The reference's ``lin2log(nanmedian(log2lin(Sv[mask])))`` from the one or two middle values the device selected
    (in dB: 10^(x/10) is monotone): NumPy's own expression on them, so the threshold has the reference's bits."""
    n = int(state_host[_STATE_COUNT])
    if n == 0:
        return float("nan")
    bits = state_host[[_STATE_LO, _STATE_HI]].astype(np.int64).view(np.float64)
    mid = np.array(bits[:1] if n % 2 else bits, dtype=dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return float(_lin2log(np.nanmedian(_log2lin(mid))))


@xarray_io()
def bottom_blackwell(ds, var_name, channel, threshold=-75, offset=0.3, r0=0, r1=500, wtheta=28, wphi=52, *,
                     device=None):
    """Blackwell seabed detection on one channel, returning a 1-D bottom line (depth).

    1. Range crop [r0_idx, r1_idx) of the ping-0 depth nearest ``r0`` / ``r1`` (r1's sample included).
    2. Both angles box-filtered as ``convolve2d(angle, ones(w, w) / w**2, "same", boundary="symm")`` (windows
       ``wtheta`` / ``wphi``; summed in f64, NaN in a window makes the mean NaN); the angle mask is
       ``theta_mean**2 > ttheta | phi_mean**2 > tphi``.
    3. If the mask is empty every ping's bottom is ``depth[ping 0][0] - offset``.  Otherwise the Sv threshold is
       ``lin2log(nanmedian(log2lin(Sv[mask])))`` (NaN -> +inf, raised to ``tSv`` when below it): the device selects the
       middle values by radix select, the host finishes them with NumPy.
    4. The 8-connected components of ``Sv > threshold`` that contain an angle-masked pixel are kept (union-find on the
       device); each ping's bottom is the depth of its first kept sample minus ``offset``, else
       ``depth[ping 0][0] - offset``.

    ``threshold``: ``tSv`` alone (angle thresholds 702 / 282), ``(tSv, x)`` (x ignored, 702 / 282 as the reference),
    or ``(tSv, ttheta, tphi)``.  The angles are used in the units the dataset holds them in: ``add_splitbeam_angle``
    writes degrees, while the 702 / 282 defaults were chosen for the raw electrical angle steps -- pass thresholds for
    the units at hand; nothing is rescaled.

    ``Sv``, ``angle_alongship``, ``angle_athwartship`` and ``depth``: (channel, ping_time, range_sample), float32 or
    float64, on the device or the host.  Returns ``bottom_depth`` (ping_time) of depth's dtype with the reference's
    attributes; its data stays on the device.  Host synchronisations: three small reads -- the depth-grid check of
    ``_check_inputs`` (its flag and the ping-0 depth row, which also places the crop), the angle-mask count together
    with the median's middle values (the ``any()`` check and the median read-back), and the union-find error word.
    Scratch on the device: 16 B (box sums) + 1 B (mask) + 8 B (component roots) per crop pixel."""
    sv, depth, r = _check_inputs(ds, var_name=var_name, channel=channel,
                                 required_vars=["angle_alongship", "angle_athwartship"], device=device)

    tSv, ttheta, tphi = _parse_blackwell_thresholds(threshold)

    ci = channel_position(ds["channel"].values, channel)
    theta = _channel_plane(ds["angle_alongship"], ci, sv.device, "angle_alongship")
    phi = _channel_plane(ds["angle_athwartship"], ci, sv.device, "angle_athwartship")
    if theta.dtype != phi.dtype:
        theta, phi = theta.double(), phi.double()
    P, S = sv.shape
    if theta.shape != (P, S) or phi.shape != (P, S):
        raise ValueError("angle_alongship / angle_athwartship must have the shape of the Sv variable")

    r0_idx = int(np.nanargmin(abs(r - r0)))
    r1_idx = int(np.nanargmin(abs(r - r1))) + 1
    R = len(range(S)[r0_idx:r1_idx])
    depth0 = depth[0].double().contiguous()
    out_dtype = depth.dtype

    parent = mask = None
    if R > 0 and P > 0:
        state = ops.seafloor_state(sv.device)
        mask = ops.seafloor_angle_mask(theta, phi, r0_idx, R, wtheta, wphi, ttheta, tphi, state)
        ops.seafloor_median(sv, r0_idx, R, mask, state)
        st = utils._to_host(state[:8]).numpy()
        if st[_STATE_MASKED] > 0:
            thr = _median_threshold(st, np.float32 if sv.dtype == torch.float32 else np.float64)
            if np.isnan(thr):
                thr = np.inf
            if thr < tSv:
                thr = tSv
            parent = ops.seafloor_components(sv, r0_idx, R, thr, mask, state)
            err = int(utils._to_host(state[_STATE_ERROR:_STATE_ERROR + 1])[0])
            if err:
                raise RuntimeError(f"epa_seafloor_components: {err} union-find loops reached their bound")
    bottom = ops.seafloor_bottom(parent, mask, P, r0_idx, depth0, float(offset), out_dtype)

    return DataArray(
        DeviceArray(bottom),
        ("ping_time",),
        coords={"ping_time": np.asarray(ds["ping_time"].values)},
        name="bottom_depth",
        attrs={
            "detector": "blackwell",
            "threshold_Sv": float(tSv),
            "threshold_angle_major": float(ttheta),
            "threshold_angle_minor": float(tphi),
            "offset_m": float(offset),
            "channel": channel,
        },
    )
