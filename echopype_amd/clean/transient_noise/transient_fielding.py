"""clean.detect_transient(method="fielding") (reference: echopype clean/transient_noise/transient_fielding.py, after
the "fielding" function of Echopy's mask_transient.py, A. Ariza 2020)."""
import warnings

import numpy as np
import torch

from ... import ops
from ...xr_lite import xarray_io
from .utils import _channel_cube, _mask_array, _range_rows


def _layer_rows(r, r0, r1, roff, jumps):
    """up, lw, rmin, sf of one range row by the reference's own expressions (bit-identical by construction), or None
    where it returns early with nothing masked."""
    if r0 > r1:
        return None
    if (r0 > r[-1]) or (r1 < r[0]):
        return None
    up = np.argmin(abs(r - r0))
    lw = np.argmin(abs(r - r1))
    rmin = np.argmin(abs(r - roff))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        dr = float(np.nanmedian(np.diff(r)))
    sf = max(1, int(round(jumps / dr)))
    return int(up), int(lw), int(rmin), min(sf, 2 ** 31 - 1)


@xarray_io()
def transient_noise_fielding(ds_Sv, var_name="Sv", range_var="depth", r0=900, r1=1000, n=30, thr=(3, 1), roff=20,
                             jumps=5, maxts=-35, start=0, *, device=None):
    """Fielding's transient-noise mask: True = VALID (keep), False = transient noise; all channels in one call.

    Per channel, with the range vector ``r`` = the first ping's row of ``range_var`` (or a 1-D ``range_sample``
    vector), ``up`` / ``lw`` / ``rmin`` = argmin |r - r0| / |r - r1| / |r - roff| and
    ``sf = max(1, round(jumps / nanmedian(diff(r))))``:

    1. ping ``j`` is left alone when ``j - n < 0``, ``j + n > P - 1`` or its layer ``[up, lw)`` is all NaN (an empty
       layer, ``up >= lw``, counts as all NaN);
    2. it is flagged when the 75th percentile of its layer is below ``maxts`` and its median exceeds the median of the
       block of pings ``[j - n, j + n)`` by more than ``thr[0]`` (medians and percentile of the linear values, NaN
       skipped, back in dB);
    3. a flagged ping walks up in windows of ``sf`` samples from ``[up - sf, up)`` while the window start is above
       ``rmin``, and stops after the first window whose ping-minus-block median difference is below ``thr[1]``; it is
       masked from one step above the last window compared to the end of the column (Python slice semantics: a
       negative start counts from the end).

    ``r0 > r1`` or a layer outside the range row masks nothing.  ``start > 0`` raises ``NotImplementedError`` (the
    reference's padding fails for every shape).  ``Sv`` float32 or float64, on the device or the host; the arithmetic
    is float64.  Returns the boolean ``fielding_mask_valid`` with the dims, order and coordinates of ``ds_Sv[var_name]``;
    its data stays on the device (a ``torch.bool`` tensor) and goes straight into ``mask.apply_mask``.

    Device work: one workgroup per ping for step 2, one per flagged ping for step 3 (quiet data costs step 2 alone).
    Host synchronisations: one, the copy of the C range rows from which the window rows are derived with the
    reference's own NumPy expressions (the copy waits for the work already queued on the stream); none when
    ``range_var`` is on the host."""
    if var_name not in ds_Sv:
        raise ValueError(f"{var_name!r} not found in Dataset.")
    if range_var not in ds_Sv:
        raise ValueError(f"{range_var!r} not found in Dataset.")
    var = ds_Sv[var_name]
    r_da = ds_Sv[range_var]
    if not ({"ping_time", "range_sample"}.issubset(r_da.dims) or (r_da.ndim == 1 and "range_sample" in r_da.dims)):
        raise ValueError(f"Cannot infer 1D '{range_var}' from dims {r_da.dims}.")
    if start > 0:
        raise NotImplementedError("start > 0 is not supported: the reference pads the mask to the wrong shape and fails "
                                  "(ValueError from np.vstack, or a result of P + start pings)")
    sv = _channel_cube(var, var_name, device)
    C, P, S = sv.shape
    if P == 0 or S == 0:
        return _mask_array(var, torch.ones((C, P, S), dtype=torch.bool, device=sv.device), "fielding_mask_valid")
    rows = _range_rows(r_da, range_var, "ping_time", C, S)
    chan = np.zeros((C, 4), dtype=np.int64)
    chan[:, 3] = 1
    for c in range(C):
        got = _layer_rows(rows[c], r0, r1, roff, jumps)
        if got is not None and n >= 0:  # (a negative n: every block is empty, nothing is flagged)
            chan[c] = got
    mask = ops.transient_fielding(sv, chan, max(int(n), 0), thr[0], thr[1], maxts)
    return _mask_array(var, mask, "fielding_mask_valid")
