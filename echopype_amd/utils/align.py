"""``align_to_ping_time`` with the reference's signature (echopype utils/align.py:5-61): a 1-D variable recorded on its own
clock -- a navigation track, a depth offset, a tilt -- brought onto the echosounder's ``ping_time``.

The reference's four branches, in its order: times equal to ``ping_time`` -> the variable renamed; one time -> that value
on every ping (float64); no time -> NaN on every ping; otherwise ``interp(method, fill_value="extrapolate")``, which is
``scipy.interpolate.interp1d``.  The last branch is one launch of ``epa_align_to_ping_time`` (``ops.align_to_ping_time``):
``"linear"`` reproduces interp1d bit for bit -- float64 nanoseconds from the first external time, ``searchsorted``, the
slope form, the end segments extrapolating, a NaN value spoiling the two segments it belongs to --, ``"nearest"`` takes
the closer sample, the earlier one on a tie and the end sample outside the track.  A NaT ping gives NaN.

External times are sorted on the host first (interp1d runs with ``assume_sorted=False``), the values permuted alike.

The one deviation: a NaT among the EXTERNAL times raises ``ValueError``.  The reference's result there is undefined (the
NaT becomes the smallest float, or NaN, depending on the xarray version, and poisons the search).

Several variables on the same clock share one search and one launch (``align_many_to_ping_time``: latitude and longitude
in ``consolidate.add_location``)."""
import numpy as np
import torch

from .. import ops
from ..xr_lite import DataArray, DeviceArray, from_xarray

METHODS = ("linear", "nearest")


def _times(a):
    a = np.asarray(getattr(a, "values", a))  # (as it is when it already is datetime64[ns]: a resident ping_time is known
    return a if a.dtype == np.dtype("datetime64[ns]") else a.astype("datetime64[ns]")  # to ops.ping_time_facts by identity)


def align_many_to_ping_time(external_das, external_time_name, ping_time_da, method="nearest"):
    """``align_to_ping_time`` of several 1-D variables that share the time coordinate ``external_time_name`` (the first
    one's is read) -> list of DataArrays on ("ping_time",).  The kernel branch is ONE launch for all of them."""
    if method not in METHODS:
        raise ValueError(f"method must be 'linear' or 'nearest', got {method!r}")
    das = [from_xarray(da) for da in external_das]
    for da in das:
        if da.ndim != 1:
            raise ValueError(f"the external variable must have a single (time) dimension, it has {da.dims}")
    pt = _times(from_xarray(ping_time_da))
    t = _times(das[0].coords[external_time_name])
    P = len(pt)

    def result(data, da):
        return DataArray(data, ("ping_time",), {"ping_time": pt}, da.attrs, da.name)

    if t.shape == pt.shape and np.array_equal(t, pt):  # (NaT != NaT, as in xarray's equals on datetimes)
        return [result(da.data, da) for da in das]
    if len(t) == 1:
        return [result(da.values[0] * np.ones(P, dtype=np.float64), da) for da in das]
    if len(t) == 0:
        return [result(np.full(P, np.nan, dtype=np.float64), da) for da in das]
    if np.isnat(t).any():
        raise ValueError(f"{external_time_name} contains NaT: the external times must all be valid")
    if P == 0:
        return [result(np.empty(0, dtype=np.float64), da) for da in das]
    ns = t.astype(np.int64)
    order = None
    if np.any(ns[1:] < ns[:-1]):
        order = np.argsort(ns, kind="stable")
        ns = ns[order]
    _, _, pt_dev = ops.ping_time_facts(pt)
    rows = []
    for da in das:
        if isinstance(da.data, DeviceArray):
            r = da.data.tensor.to(device=pt_dev.device, dtype=torch.float64)
            rows.append(r if order is None else r.index_select(0, ops.to_device(order, device=pt_dev.device)))
        else:
            a = np.asarray(da.data, dtype=np.float64)
            rows.append(a if order is None else a[order])
    if all(isinstance(r, np.ndarray) for r in rows):
        y = ops.to_device(np.stack(rows), device=pt_dev.device)
    else:
        y = torch.stack([r if isinstance(r, torch.Tensor) else ops.to_device(r, device=pt_dev.device) for r in rows])
    out = ops.align_to_ping_time(ops.to_device(ns, device=pt_dev.device), y.contiguous(), pt_dev, method)
    return [result(DeviceArray(out[i]), da) for i, da in enumerate(das)]


def align_to_ping_time(external_da, external_time_name, ping_time_da, method="nearest"):
    """Align ``external_da`` (one dimension, ``external_time_name``; host data or a ``DeviceArray``) with ``ping_time_da``.

    ``method``: ``"nearest"`` (default) or ``"linear"``; not used when the external times equal ``ping_time`` or the
    variable holds a single value.  Anything else raises ``ValueError``.  A NaT among the external times raises
    ``ValueError`` (the reference's result there is undefined: the one deviation).

    Returns a DataArray on ("ping_time",) with the input's attributes and without the external time coordinate; float64
    in HBM (a ``DeviceArray``) when the kernel ran."""
    return align_many_to_ping_time([external_da], external_time_name, ping_time_da, method)[0]


__all__ = ["align_to_ping_time"]
