"""The conservative range grid behind the compute_MVBS routes that do not wait for the GPU (commongrid.api
._mvbs_of_deferred_sv, ._mvbs_of_deferred_clean, ._mvbs_of_array_without_waiting, fused.compute_Sv_MVBS).  The size of
the reference's grid, ``np.arange(0, nanmax(range) + bin, bin)`` (commongrid/api.py:108-115), depends on a number only
a kernel can produce, so a route sizes the grid from an upper bound known without waiting (``range_cap``), launches its
kernel on those ``n_cap`` bins (``launch_or_decline``), leaves the range statistics on their way to the host, and the
dataset is trimmed to the reference's grid when first read (``deferred_mvbs``).  Gate, kernel, by-products and
fallback stay with the routes."""
import logging

import numpy as np
import torch

from .. import _lib, ops
from ..xr_lite import DeferredDataset
from .utils import _parse_x_bin, resample_edges

CPS = ("channel", "ping_time", "range_sample")

_AGG_MSG = ("Aggregation may be negatively impacted since Flox will not aggregate any "
            "```Sv``` values that have corresponding NaN coordinate values. Consider handling "
            "these values before calling your intended commongrid function.")


def nan_coordinate_warning(name):
    """NaN coordinates are not aggregated (utils.py:595-608: same warning text)."""
    logging.warning(f"The ```{name}``` coordinate array contain NaNs. {_AGG_MSG}")


def range_edges(rmax, range_bin_m):
    """The reference's range edges for a maximum ``rmax``: np.arange defines the grid (its floating-point length, not a
    ceil).  A non-finite maximum (no valid range at all) has no grid: one edge, no bin."""
    return np.arange(0, rmax + range_bin_m, range_bin_m) if np.isfinite(rmax) else np.zeros(1)


def n_range_bins(rmax, range_bin_m):
    """Bins of that grid; 0 when the only valid range is 0 (one sample per ping): an empty grid, as in the reference."""
    return len(range_edges(rmax, range_bin_m)) - 1


def reach_cap(coef, S, affine=None):
    """The farthest any coefficient row reaches, reduced on the device: one scalar comes back, NaN when no row is valid.
    ``affine`` = (scale, offset): of ``offset + scale * range`` (a lazy depth), whichever end is the deeper one."""
    r0 = coef[..., _lib.CF_R0]
    reach = (S - 1) * coef[..., _lib.CF_RA] * coef[..., _lib.CF_RB] + r0
    if affine is not None:
        reach = torch.fmax(affine[1] + affine[0] * reach, affine[1] + affine[0] * r0) * (1 + 1e-6)
    r = float(torch.nan_to_num(reach, nan=float("-inf")).max().item())
    return r if r > float("-inf") else float("nan")


def range_cap(range_var_max, host_bound, coef=None, S=None, affine=None):
    """What the grid is sized from: the caller's ``range_var_max`` (then it IS the grid's maximum), else a bound known on
    the host (no device reduction, no wait), else the device reduction of the rows (``reach_cap``; None without rows)."""
    if range_var_max is not None:
        return _parse_x_bin(range_var_max) + 1e-8
    if host_bound is not None:
        return host_bound
    return reach_cap(coef, S, affine) if coef is not None else None


def sorted_time_grid(ping_time, ping_time_bin):
    """(ping_time as datetime64[ns], its int64 view, first edge, step, number of time bins), or None: unsorted pings, NaT,
    no ping at all.  No upload (a route may still bail), and no O(P) pass either when the array is resident data."""
    ping_time = np.asarray(ping_time).astype("datetime64[ns]", copy=False)
    ns, sorted_valid, _ = ops.ping_time_facts(ping_time, want_device=False)
    if not sorted_valid:
        return None
    e0, dt, n_t = resample_edges(ping_time, ping_time_bin, sorted_valid=True)
    return ping_time, ns, e0, dt, n_t


def time_bin_start(ping_time, e0, dt, n_t, closed="left"):
    """First ping of every time bin, from the device twin of the array ``sorted_time_grid`` returned (uploaded once per
    file when it is resident data).  Called once the route is certain to launch."""
    return ops.time_bin_offsets(ops.ping_time_facts(ping_time)[2], e0, dt, n_t, closed=closed)


def launch_or_decline(launch, served=None, shard=None, vote=None):
    """``launch()`` is the route's kernel call.  Returns None when it declines -- it raises EpaError (e.g. a range grid
    too fine for the LDS accumulators), returns None, or ``served(res)`` is false (it ran but left no statistics) --
    else (res, the bins, index of the first of them among the local time bins: 0).  On a ping shard the plain route runs
    other collectives, so every rank takes it if any has to: the vote rides with the exchange plan's message
    (``shard.finish``; ``vote`` = (first_bin, last_bin, fill_value, shape of the local bins, device)), and the bins are
    those this rank reports: a cut bin holds the total over all ranks, on the lowest rank that has it."""
    try:
        res = launch()
    except _lib.EpaError:
        res = None
    if res is not None and served is not None and not served(res):
        res = None
    if shard is None:
        return None if res is None else (res, res["MVBS"], 0)
    first_bin, last_bin, fill_value, shape, device = vote
    done = shard.finish(res, first_bin, last_bin, fill_value, shape=shape, device=device)
    return None if done is None else (res, *done)


def trim_decision(stats, n_cap, range_bin_m, range_var, range_var_max=None, r_cap=None, has_fallback=True):
    """What becomes of bins launched on ``n_cap`` range bins once ``stats`` = (nanmax of the range, its NaN count) are
    known (None: nobody left any): the edges of the reference's grid -- keep the first ``len(edges) - 1`` bins -- or
    None: the route's fallback runs.  With ``range_var_max`` the maximum is ``r_cap`` whatever the statistics say.
    The fallback is due without statistics, without a valid range (the plain route raises the reference's error), for an
    empty grid (it returns the reference's) and for a maximum beyond the conservative grid (it must not happen, the cap
    is an upper bound: binned again, exactly).  ``has_fallback`` False -- a ping shard: a fallback would be a collective
    at a time only this rank chooses -- no valid range on any rank and a maximum beyond the grid raise, an empty grid stays."""
    rmax, n_nan_range = stats if stats is not None else (float("nan"), 0)
    if stats is not None and range_var_max is not None:
        rmax = r_cap
    r_edges = range_edges(rmax, range_bin_m)
    n_r = len(r_edges) - 1
    if not 1 <= n_r <= n_cap:
        if has_fallback:
            return None
        if not np.isfinite(rmax):  # the reference's grid does not exist
            raise ValueError("range bins are empty: the range variable holds no valid values")
        if n_r > n_cap:
            raise RuntimeError(f"nanmax({range_var}) = {rmax} lies beyond the range grid the shards agreed on "
                               f"({n_cap} bins of {range_bin_m} m)")
    if n_nan_range > 0:
        nan_coordinate_warning(range_var)
    return r_edges


def deferred_mvbs(ds_Sv, mv_full, n_cap, get_stats, range_var_max, r_cap, time_grid, range_var, range_bin_m,
                  ping_time_bin, fallback=None, dim_0="channel", closed="left", defer=True):
    """The MVBS dataset of bins ``mv_full`` launched on ``n_cap`` range bins: trimmed to the reference's grid and
    assembled when first read (a ``DeferredDataset``; ``defer`` False: now).  ``get_stats()`` is called then and returns
    what ``trim_decision`` takes; ``fallback(snapshot)`` returns the dataset when the trim cannot be done (None: a ping
    shard); ``time_grid`` = (ping_time, left edge of the first time bin of ``mv_full``, step).  What the assembly needs
    of ``ds_Sv`` is taken NOW: the caller may replace variables or edit attributes between the call and the first use of
    the result, and the result must not change with them.  Only the bins are held: the kernel's sums / counts die with
    the caller."""
    ds_snap, n_t = ds_Sv.copy(), mv_full.shape[1]
    ping_time, e0, dt = time_grid

    def build():
        from .api import _assemble_mvbs  # (api imports this module)

        r_edges = trim_decision(get_stats(), n_cap, range_bin_m, range_var, range_var_max, r_cap, fallback is not None)
        if r_edges is None:
            return fallback(ds_snap)
        n_r = len(r_edges) - 1
        mvbs_t = mv_full[..., :n_r].contiguous() if n_r != n_cap else mv_full
        return _assemble_mvbs(ds_snap, mvbs_t, dim_0, ping_time, e0, dt, n_t, r_edges, range_var, range_bin_m,
                              ping_time_bin, closed)

    return DeferredDataset(build) if defer else build()
