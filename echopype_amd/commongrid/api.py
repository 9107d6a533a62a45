"""compute_MVBS / compute_MVBS_index_binning with the reference's signatures
(/root/reference/echopype/commongrid/api.py:30-191, :194-266).  Validation, bin edges, coordinates
and attributes are host Python (O(P)); the (channel, ping_time, range_sample) reduction is one HIP
kernel launch through the C ABI (epa_mvbs / epa_mvbs_index).  ``method``, ``reindex`` and
``**flox_kwargs`` are accepted for signature compatibility (flox is not involved).
"""
import logging
import os

import numpy as np
import torch

from .. import _lib, ops
from ..device_view import as_tensor, broadcast_to_dims, resolve_device, strided_view
from ..utils.prov import echopype_prov_attrs, insert_processing_level
from ..xr_lite import DataArray, Dataset, DeviceArray, LazyDeviceArray, defer_mvbs_enabled, from_xarray, xarray_io
from .deferred import (CPS, deferred_mvbs, launch_or_decline, n_range_bins, nan_coordinate_warning, range_cap, range_edges,
                       sorted_time_grid, time_bin_start)
from .utils import (_parse_x_bin, _set_MVBS_attrs, _setup_and_validate, coarsen_time_mean, get_distance_from_latlon,
                    ping_time_bin_parsing_and_conversion, resample_edges)

logger = logging.getLogger("echopype_amd.commongrid")
_TORCH_DT = {"float64": torch.float64, "float32": torch.float32}


def _range_stats(da, t):
    """(nanmin, nanmax, NaN count) of a range variable: left with the array by the kernel that wrote it
    (compute_Sv), or one sweep of the device tensor ``t`` actually handed to the kernels (None: a lazy array binned
    through its coefficient rows; it is written only if it carries no statistics)."""
    d = da.data if isinstance(da, DataArray) else None
    if isinstance(d, DeviceArray) and (t is None or (_TORCH_DT.get(d.dtype.name) == t.dtype and d.shape == tuple(t.shape))):
        st = d.cached_stats()
        if st is not None:
            return st
    return ops.nanminmax(d.tensor if t is None else t, with_nan_count=True)


def _coef_rows(da, order, sv_t):
    """The coefficient rows a lazy echo_range (xr_lite.LazyDeviceArray, left by compute_Sv on power samples) is an
    affine function of, when the binning kernels can take them in place of the array: same dims, shape and dtype as
    Sv, array untouched since.  The kernels evaluate ``fl(fl(s * ra) * rb) + r0`` rounded to the array's dtype --
    what the array holds wherever the raw sample is not NaN; where it is NaN, so is Sv, which a NaN-skipping mean
    drops like the reference drops the NaN coordinate."""
    d = da.data if isinstance(da, DataArray) else None
    if not isinstance(d, LazyDeviceArray) or tuple(da.dims) != tuple(order):
        return None
    if d.shape != tuple(sv_t.shape) or _TORCH_DT.get(d.dtype.name) != sv_t.dtype:
        return None
    return d.coef_rows()


@xarray_io()
def compute_MVBS(ds_Sv, range_var="echo_range", range_bin="20m", ping_time_bin="20s", method="map-reduce",
                 reindex=False, skipna=True, fill_value=np.nan, closed="left", range_var_max=None, *, _shard=None,
                 **flox_kwargs):
    """Mean volume backscattering strength on a (ping_time, range) grid in physical units.
    (``_shard``: set by echopype_amd.sharding.compute_MVBS when ``ds_Sv`` is one rank's ping shard.)"""
    if method != "map-reduce" and reindex is not None:
        raise ValueError(f"Passing in reindex={reindex} is only allowed when method='map_reduce'.")
    ds_Sv = from_xarray(ds_Sv)
    ds_Sv, range_bin_m = _setup_and_validate(ds_Sv, range_var, range_bin, closed)
    if not isinstance(ping_time_bin, str):
        raise TypeError("ping_time_bin must be a string")

    hint = None
    if skipna and closed == "left":
        # Sv still deferred by compute_Sv: written by THIS pass over the raw samples, next to the bins ...
        # ... or the Sv_corrected remove_background_noise deferred: its pass 2 bins as well
        if _shard is None:
            done = _mvbs_of_deferred_sv(ds_Sv, range_var, range_bin_m, ping_time_bin, fill_value, range_var_max)
            if done is None:
                done = _mvbs_of_deferred_clean(ds_Sv, range_var, range_bin_m, ping_time_bin, fill_value, range_var_max)
        else:  # a ping shard: the grid is the whole dataset's, cut bins are exchanged in HBM; the route is voted on
            done, hint = _sharded_deferred(ds_Sv, range_var, range_bin_m, ping_time_bin, fill_value, range_var_max, _shard)
        if done is not None:
            return done
    return _mvbs_plain(ds_Sv, range_var, range_bin_m, ping_time_bin, skipna, fill_value, closed, range_var_max, _shard,
                       grid_hint=hint)


def _sharded_deferred(ds_Sv, range_var, range_bin_m, ping_time_bin, fill_value, range_var_max, _shard):
    """One rank's ping shard: which route the call takes is decided TOGETHER.  Whether a rank could take a deferred route
    depends on rank-local state (its Sv already read or replaced, its pings unsorted, its raw samples written to ...), and
    the routes run different collectives -- so every rank names the route it could take (1: Sv deferred by compute_Sv,
    2: Sv_corrected deferred by remove_background_noise, 0: neither) in the call's FIRST control message, the one that
    also carries the time grid and the range cap of the whole dataset (sharding.MVBSShard.grid), and a deferred route
    runs only if all ranks named it.  Returns (the MVBS dataset or None, the time grid for the plain route: it does not
    ask for it again)."""
    from .utils import timedelta_ns

    args = (ds_Sv, range_var, range_bin_m, ping_time_bin, fill_value, range_var_max, _shard)
    route, fn, prep = 0, None, None
    for rid, f in ((1, _mvbs_of_deferred_sv), (2, _mvbs_of_deferred_clean)):
        prep = f(*args, _grid="probe")
        if prep is not None:
            route, fn = rid, f
            break
    if route:
        ns, dt, r_cap = prep
    else:  # (unsorted pings, NaT, an empty shard: the message takes them as they are)
        ns = np.asarray(ds_Sv["ping_time"].values).astype("datetime64[ns]", copy=False).view(np.int64)
        dt, r_cap = timedelta_ns(ping_time_bin), float("nan")
    reach = r_cap if (route and range_var_max is None) else float("nan")
    e0g, n_glob, first_bin, last_bin, g_cap, agreed = _shard.grid(ns, dt, "left", reach, sorted_valid=bool(route), route=route)
    hint = (e0g, n_glob, first_bin, last_bin)
    if not route or agreed != route:
        return None, hint
    grid = (e0g + first_bin * dt, last_bin - first_bin + 1, first_bin, last_bin, g_cap if range_var_max is None else r_cap)
    return fn(*args, _grid=grid), hint


def _mvbs_plain(ds_Sv, range_var, range_bin_m, ping_time_bin, skipna, fill_value, closed, range_var_max, _shard,
                allow_defer=True, grid_hint=None):
    """The binning of an existing Sv array (arguments validated by compute_MVBS).  ``allow_defer=False``: the dataset is
    assembled before the call returns (the fallback of the deferred routes' own assembly).  ``grid_hint``: the time grid
    of the whole dataset, when the call's route vote has fetched it already (_sharded_deferred)."""
    sv_da = ds_Sv["Sv"]
    order = tuple(sv_da.dims)
    dim_0 = order[0]
    sv_t = as_tensor(sv_da)
    if sv_t.dtype not in (torch.float32, torch.float64):
        sv_t = sv_t.double()
    # (a lazy echo_range straight from compute_Sv: binned through its coefficient rows, never written)
    rows = _coef_rows(ds_Sv[range_var], order, sv_t) if skipna else None
    rg_t = as_tensor(broadcast_to_dims(ds_Sv[range_var], ds_Sv, order), sv_t.dtype) if rows is None else None
    C, P, S = sv_t.shape

    if _shard is None and rows is not None and allow_defer and defer_mvbs_enabled():
        # a lazy range (coefficient rows) that knows on the host how far it can reach and whose exact statistics are a
        # kernel's by-product still in HBM: the bins are launched on the conservative grid, the dataset trimmed when read
        done = _mvbs_of_array_without_waiting(ds_Sv, sv_t, rows, range_var, range_bin_m, ping_time_bin, skipna,
                                              fill_value, closed, range_var_max)
        if done is not None:
            return done

    # range edges: np.arange(0, max + bin, bin)  (api.py:108-115)
    lo, hi, n_nan_range = _range_stats(ds_Sv[range_var], rg_t)
    if range_var_max is None:
        rmax = hi if _shard is None else _shard.range_max(hi)  # the range grid of the whole dataset
    else:
        rmax = _parse_x_bin(range_var_max) + 1e-8
    if not np.isfinite(rmax):
        raise ValueError("range bins are empty: the range variable holds no valid values")
    r_edges = range_edges(rmax, range_bin_m)
    n_r = len(r_edges) - 1  # 0 when the only valid range is 0 (one sample per ping): an empty grid, as in the reference

    ping_time = np.asarray(ds_Sv["ping_time"].values).astype("datetime64[ns]")
    if np.isnat(ping_time).any():
        nan_coordinate_warning("ping_time")
    if n_nan_range > 0:
        nan_coordinate_warning(range_var)

    # ping bins: pandas-resample edges, anchored at midnight (api.py:118-128)
    e0, dt, n_t = resample_edges(ping_time, ping_time_bin)
    ns = ping_time.astype(np.int64)
    first_bin = 0
    if _shard is not None:  # day origin of the whole dataset; this shard covers global bins first_bin .. last_bin
        e0, _, first_bin, last_bin = grid_hint if grid_hint is not None else _shard.time_grid(ns, dt, closed)
        e0, n_t = e0 + first_bin * dt, last_bin - first_bin + 1
    perm = None
    # unsorted pings: sort once on the host, kernels follow the permutation.  NaT is INT64_MIN: the stable sort puts
    # such pings first, below the first edge, i.e. in no bin -- flox drops values with a NaT coordinate.  (np.diff
    # would wrap in int64 on a trailing NaT and report the array as sorted.)
    if np.any(ns[1:] < ns[:-1]) or np.isnat(ping_time).any():
        order_idx = np.argsort(ns, kind="stable")
        perm = ops.to_device(order_idx.astype(np.int32))
        ns = ns[order_idx]
    bin_start = ops.time_bin_offsets(ops.to_device(ns), e0, dt, n_t, closed=closed)

    if n_r == 0:
        mvbs_t = torch.empty((C, n_t, 0), dtype=sv_t.dtype, device=sv_t.device)
    else:
        res = ops.mvbs(sv_t, bin_start, n_t, range_bin_m, n_r, range=rg_t, coef=rows, coef_as_stored=True, skipna=skipna, closed=closed,
                       fill_value=fill_value, ping_perm=perm, want_partials=_shard is not None)
        mvbs_t = res["MVBS"]
        if _shard is not None:  # bins cut by a shard edge: totals over all ranks, reported by the lowest holder
            mvbs_t, lo = _shard.finish(res, first_bin, last_bin, fill_value)
            e0, n_t = e0 + lo * dt, mvbs_t.shape[1]

    return _assemble_mvbs(ds_Sv, mvbs_t, dim_0, ping_time, e0, dt, n_t, r_edges, range_var, range_bin_m,
                          ping_time_bin, closed)


def _binned_through_rows(p, sv_da, rng_da, rng_d):
    """Can a pass over the raw samples of ``p`` (calibrate_base.PowerSource) bin ``sv_da`` on ``rng_da``?  It holds
    ``rng_d``, both have the samples' dimensions, and p's echo_range still is the function of p's coefficient rows."""
    return rng_da.data is rng_d and tuple(sv_da.dims) == CPS and tuple(rng_da.dims) == CPS \
        and p.echo_range.coef_rows() is p.coef


def _plain_fallback(range_var, range_bin_m, ping_time_bin, fill_value, range_var_max, skipna=True, closed="left"):
    """The fallback of a deferred route: the plain route on the snapshot, assembled at once."""
    return lambda ds: _mvbs_plain(ds, range_var, range_bin_m, ping_time_bin, skipna, fill_value, closed, range_var_max,
                                  None, allow_defer=False)


def _mvbs_of_array_without_waiting(ds_Sv, sv_t, rows, range_var, range_bin_m, ping_time_bin, skipna, fill_value, closed,
                                   range_var_max):
    """The binning of an Sv ARRAY whose range variable is still lazy (``compute_Sv`` on EK80 complex samples; an EK60 Sv
    somebody has read already) -- without the wait ``_mvbs_plain`` pays for nanmax(range) before it can size its grid:
    the kernel runs on ``np.arange(0, bound + bin, bin)`` with the host-side bound the lazy range carries
    (``reach_bound``) and the dataset, a ``DeferredDataset``, is trimmed to ``nanmax`` when somebody reads it.  None: the
    plain route (no bound, no statistics, unsorted pings, a grid the kernels refuse)."""
    rng_d = ds_Sv[range_var].data
    if not isinstance(rng_d, LazyDeviceArray):
        return None
    bound = range_cap(range_var_max, rng_d.reach_bound)  # (no bound on the host: no device reduction here)
    grid = sorted_time_grid(ds_Sv["ping_time"].values, ping_time_bin) if bound is not None else None
    if grid is None:
        return None
    n_cap = n_range_bins(bound, range_bin_m)
    stats = rng_d.stats_async() if n_cap >= 1 else None
    if stats is None:
        return None
    ping_time, _, e0, dt, n_t = grid
    bin_start = time_bin_start(ping_time, e0, dt, n_t, closed)
    got = launch_or_decline(lambda: ops.mvbs(sv_t, bin_start, n_t, range_bin_m, n_cap, coef=rows, coef_as_stored=True,
                                             skipna=skipna, closed=closed, fill_value=fill_value))
    if got is None:
        return None
    plain = _plain_fallback(range_var, range_bin_m, ping_time_bin, fill_value, range_var_max, skipna, closed)
    return deferred_mvbs(ds_Sv, got[1], n_cap, lambda: stats.tolist()[1:], range_var_max, bound, (ping_time, e0, dt),
                         range_var, range_bin_m, ping_time_bin, plain, tuple(ds_Sv["Sv"].dims)[0], closed)


def _mvbs_of_deferred_sv(ds_Sv, range_var, range_bin_m, ping_time_bin, fill_value, range_var_max, _shard=None, _grid=None):
    """``compute_Sv`` on power samples leaves Sv deferred (``LazyDeviceArray`` with a ``source``); binned right after --
    the usual sequence -- one pass over the raw samples (``epa_sv_mvbs_fused``) writes that Sv array AND the bins: the two
    reference calls cost 12 B/sample instead of 12 + 8.  Returns the MVBS dataset, or None when the plain route has to
    run (Sv already written or replaced, another range variable, unsorted / NaT pings, a grid the fused kernel does not
    serve); when the pass ran, its Sv array and range statistics stay with the dataset either way.

    Nothing here waits for the GPU: the kernel runs on a conservative range grid (the farthest any coefficient row can
    reach, bounded on the host from the host copies of sample_interval / sound_speed when there are any), leaves
    {nanmin, nanmax, NaN count} of the echo_range in HBM, and the dataset that needs them -- the grid is
    ``np.arange(0, nanmax + bin, bin)`` (api.py:108-115) -- is a ``DeferredDataset``: read back, trimmed and assembled
    on first use."""
    sv_da, rng_da = ds_Sv["Sv"], ds_Sv[range_var]
    d = sv_da.data
    src = d.source if isinstance(d, LazyDeviceArray) and not d.materialized else None
    # ``depth`` left lazy by add_depth on this dataset's lazy echo_range (offset + scale * echo_range, row by row): binned
    # inside the same pass (epa_sv_mvbs_fused_depth) -- the three reference calls at the 12 B/sample of the two
    rng_d, depth = rng_da.data, None
    if src is not None and rng_d is not getattr(src, "echo_range", None) and isinstance(rng_d, LazyDeviceArray):
        aff = rng_d.affine_of()
        if aff is not None and aff[0] is getattr(src, "echo_range", None) \
                and src.flags == (_lib.FLAG_GUARD_POS | _lib.FLAG_MASK_RANGE) and rng_d.dtype == d.dtype:
            depth = aff[1:]
    if src is None or getattr(src, "cal_type", None) != "Sv" or not src.intact() \
            or not _binned_through_rows(src, sv_da, rng_da, src.echo_range if depth is None else rng_d):
        return None  # (also: an Sv deferred by something else than compute_Sv, e.g. remove_background_noise)
    grid = sorted_time_grid(ds_Sv["ping_time"].values, ping_time_bin)
    if grid is None:
        return None
    ping_time, ns, e0, dt, n_t = grid
    C, P, S = d.shape
    # (the host-side bound of the variable that is binned: no device reduction, no wait)
    r_cap = range_cap(range_var_max, rng_d.reach_bound if depth is not None else getattr(src, "reach_bound", None),
                      src.coef, S, affine=depth)
    first_bin = last_bin = 0
    if _shard is not None:
        if isinstance(_grid, str):  # "probe": this rank could take the route (_sharded_deferred puts it to the vote)
            return ns, dt, r_cap
        e0, n_t, first_bin, last_bin, r_cap = _grid  # (the whole dataset's: the same on every rank)
    n_cap = n_range_bins(r_cap, range_bin_m)
    if n_cap < 1:
        return None
    bin_start = time_bin_start(ping_time, e0, dt, n_t)

    def launch():
        if depth is not None:
            # EPA_DEPTH_WITH_MVBS=1: the depth array is written by this pass as well (+8 B/sample here instead of the
            # 4 + 8 of epa_depth_rows when somebody reads it later); default: it stays lazy
            return ops.sv_mvbs_fused_depth(src.raw, src.coef, depth[0], depth[1], bin_start, n_t, range_bin_m, n_cap,
                                           fill_value=fill_value, dtype=src.dtype, want_partials=_shard is not None,
                                           want_depth=not rng_d.materialized and os.environ.get("EPA_DEPTH_WITH_MVBS") == "1")
        return ops.sv_mvbs_fused(src.raw, src.coef, bin_start, n_t, range_bin_m, n_cap, cal_flags=src.flags, skipna=True,
                                 closed="left", fill_value=fill_value, dtype=src.dtype, want_range_stats=True,
                                 want_partials=_shard is not None)

    # served by the generic kernel (a handful of pings, a grid beyond the LDS)?  It leaves no range statistics, which
    # every later step asks for -- K1 does, on the plain route.  (Known on the host: epa_last_range_stats_filled.)
    got = launch_or_decline(launch, served=lambda res: res["range_stats_filled"], shard=_shard,
                            vote=(first_bin, last_bin, fill_value, (C, n_t, n_cap), src.raw.device))
    if got is None:
        return None
    res, mv_full, lo = got
    rng = rng_d if depth is not None else src.echo_range  # (the statistics are the binned variable's)
    d.fulfil(res["Sv"])
    if res.get("depth") is not None:
        rng_d.fulfil(res["depth"])
    # the three numbers start their way to the host now, on a side stream behind THIS kernel: whoever reads them later
    # (the assembly, the next reader of the echo_range statistics) does not wait for kernels launched after it
    stats = ops.fetch_async(res["range_stats"])
    rng.set_stats(stats)
    # on a shard nanmax(echo_range) of the whole dataset: all-reduced (MAX) where it lies, behind the kernel -- no host wait
    gmax = ops.fetch_async(_shard.range_max_device(res["range_stats"][1:2].clone())) \
        if _shard is not None and range_var_max is None else None
    plain = None if _shard is not None else _plain_fallback(range_var, range_bin_m, ping_time_bin, fill_value, range_var_max)
    return deferred_mvbs(ds_Sv, mv_full, n_cap, lambda: (stats.tolist()[1] if gmax is None else gmax.item(), stats.tolist()[2]),
                         range_var_max, r_cap, (ping_time, e0 + lo * dt, dt), range_var, range_bin_m, ping_time_bin, plain,
                         defer=defer_mvbs_enabled())


def _mvbs_of_deferred_clean(ds_Sv, range_var, range_bin_m, ping_time_bin, fill_value, range_var_max, _shard=None, _grid=None):
    """The chain as the reference's user writes it -- ``compute_Sv``, ``remove_background_noise``, then
    ``compute_MVBS`` of the dataset with ``Sv := Sv_corrected`` -- arrives here with an Sv that
    ``remove_background_noise`` left deferred (``clean.api.DenoiseSource``: pass 1 has run).  Pass 2 runs NOW, on the
    real grid: one sweep of the raw samples writes Sv_noise, Sv_corrected, their minima / maxima AND the bins
    (``epa_sv_denoise_mvbs``) -- 20 B/sample instead of 20 + 8 for the pass and a separate binning of the array it
    wrote.  Nothing waits for the GPU (conservative grid, ``DeferredDataset``: see ``_mvbs_of_deferred_sv``).  None:
    the plain route runs (it reads the array, which runs pass 2 by itself)."""
    from ..clean.api import DenoiseSource

    sv_da, rng_da = ds_Sv["Sv"], ds_Sv[range_var]
    d = sv_da.data
    src = d.source if isinstance(d, LazyDeviceArray) and not d.materialized else None
    if not isinstance(src, DenoiseSource) or d is not src.lazy("corrected") or src.minmax is not None or not src.intact():
        return None
    p = src.power
    if not _binned_through_rows(p, sv_da, rng_da, p.echo_range):
        return None
    grid = sorted_time_grid(ds_Sv["ping_time"].values, ping_time_bin)
    if grid is None:
        return None
    ping_time, ns, e0, dt, n_t = grid
    C, P, S = d.shape
    r_cap = range_cap(range_var_max, getattr(p, "reach_bound", None), p.coef, S)
    first_bin = last_bin = 0
    if _shard is not None:
        if src.global_rmax is None:  # (pass 1 did not run as a shard's: the plain route -- by the vote, if on this rank only)
            return None
        if isinstance(_grid, str):  # "probe": see _mvbs_of_deferred_sv
            return ns, dt, r_cap
        e0, n_t, first_bin, last_bin, r_cap = _grid
    n_cap = n_range_bins(r_cap, range_bin_m)
    if n_cap < 1:
        return None
    bin_start = time_bin_start(ping_time, e0, dt, n_t)
    got = launch_or_decline(
        lambda: ops.sv_denoise_mvbs(p.raw, p.coef, src.a2, src.noise, src.ping_num, float(src.snr), bin_start, n_t,
                                    range_bin_m, n_cap, flags=p.flags, dtype=p.dtype, skipna=True, closed="left",
                                    fill_value=fill_value, want_noise=True, want_corrected=True, want_minmax=True,
                                    minmax_async=True, ping_phase=src.ping_phase, want_partials=_shard is not None),
        shard=_shard, vote=(first_bin, last_bin, fill_value, (C, n_t, n_cap), p.raw.device))
    if got is None:
        return None
    res, mv_full, lo = got
    src.install(res)
    # the statistics of the range were left by pass 1 and have been on their way to the host since then; on a shard the
    # maximum is the one over all shards, all-reduced behind pass 1 (-inf: no valid range on any), the NaN count local
    rng, gmax = p.echo_range, src.global_rmax if _shard is not None else None

    def stats():
        st = rng.cached_stats()
        if gmax is None:
            return st[1:] if st is not None else None
        return float(gmax.item()), st[2] if st is not None else 0

    plain = None if _shard is not None else _plain_fallback(range_var, range_bin_m, ping_time_bin, fill_value, range_var_max)
    return deferred_mvbs(ds_Sv, mv_full, n_cap, stats, range_var_max, r_cap, (ping_time, e0 + lo * dt, dt), range_var,
                         range_bin_m, ping_time_bin, plain, defer=defer_mvbs_enabled())


def _assemble_mvbs(ds_Sv, mvbs_t, dim_0, ping_time, e0, dt, n_t, r_edges, range_var, range_bin_m,
                   ping_time_bin, closed):
    """Coordinates (left bin edges), positions, attributes and provenance of the MVBS dataset
    (commongrid/api.py:146-189)."""
    t_left = (e0 + dt * np.arange(n_t)).astype("datetime64[ns]")
    ds_MVBS = Dataset(coords={"ping_time": t_left, dim_0: ds_Sv[dim_0].values, range_var: r_edges[:-1]})
    ds_MVBS["Sv"] = DataArray(DeviceArray(mvbs_t), (dim_0, "ping_time", range_var))

    # positions: per-bin nanmean of latitude / longitude (utils.py:453-501); O(P) on the host
    if "latitude" in ds_Sv and "longitude" in ds_Sv:
        tb = np.floor_divide(ping_time.astype(np.int64) - e0, dt)
        if closed == "right":
            tb = -np.floor_divide(-(ping_time.astype(np.int64) - e0), dt) - 1
        ok = (tb >= 0) & (tb < n_t) & ~np.isnat(ping_time)
        for var in ("latitude", "longitude"):
            v = np.asarray(ds_Sv[var].values, dtype=np.float64)
            use = ok & ~np.isnan(v)
            ssum = np.bincount(tb[use], weights=v[use], minlength=n_t)
            cnt = np.bincount(tb[use], minlength=n_t)
            with np.errstate(invalid="ignore", divide="ignore"):
                ds_MVBS[var] = (("ping_time",), np.where(cnt > 0, ssum / cnt, np.nan), dict(ds_Sv[var].attrs))
    if range_var == "echo_range" and "water_level" in ds_Sv.data_vars:
        ds_MVBS["water_level"] = ds_Sv["water_level"]

    _set_MVBS_attrs(ds_MVBS)
    ds_MVBS.coords[range_var].attrs = {"long_name": "Range distance", "units": "m"}
    val, unit = ping_time_bin_parsing_and_conversion(ping_time_bin)
    ds_MVBS.data_vars["Sv"].attrs.update({
        "cell_methods": (f"ping_time: mean (interval: {val} {unit} "
                         "comment: ping_time is the interval start) "
                         f"{range_var}: mean (interval: {range_bin_m} meter "
                         f"comment: {range_var} is the interval start)"),
        "binning_mode": "physical units",
        "range_meter_interval": str(range_bin_m) + "m",
        "ping_time_interval": ping_time_bin,
    })
    prov = echopype_prov_attrs(process_type="processing")
    prov["processing_function"] = "commongrid.compute_MVBS"
    ds_MVBS = ds_MVBS.assign_attrs(prov)
    if "frequency_nominal" in ds_Sv:
        ds_MVBS["frequency_nominal"] = ds_Sv["frequency_nominal"]
    if "channel" in ds_Sv and dim_0 != "channel":
        ds_MVBS["channel"] = ds_Sv["channel"]
    return insert_processing_level(ds_MVBS, "L3*", input_ds=ds_Sv)


_REGRID_DIMS = ("channel", "ping_time", "range_sample")
_REGRID_CELLS = ("a sample stands for the interval between the midpoints of its range and its neighbours' (the outer two "
                 "mirrored); a cell holds 10 log10 of the overlap-weighted mean of 10^(Sv/10) over the samples that reach "
                 "into it, NaN samples left out; coverage is the share of the cell those overlaps fill")


def _largest_range(rng, range_var):
    """The largest value of the range variable, NaN skipped: the by-product of the kernel that wrote the array, else one
    reduction on the device -- one host wait either way, as in compute_MVBS; host data are reduced on the host."""
    d = rng.data
    if isinstance(d, DeviceArray):
        t = d.tensor
        if t.dtype in (torch.float32, torch.float64) and t.is_contiguous():
            hi = _range_stats(rng, None)[1]
        else:
            hi = ops.nanminmax(t.double().contiguous())[1]
    else:
        a = np.asarray(d, dtype=np.float64)
        hi = float(np.nanmax(a)) if a.size and not np.isnan(a).all() else float("nan")
    if hi == float("inf"):
        raise ValueError(f"the largest value of {range_var} is not finite: give range_var_max")
    if not np.isfinite(hi):
        raise ValueError("range bins are empty: the range variable holds no valid values")
    return hi


@xarray_io()
def regrid_Sv(ds_Sv, range_var="echo_range", range_bin="0.2m", range_var_max=None, with_coverage=True, *, device=None):
    """``ds_Sv["Sv"]`` resampled along range onto ONE grid shared by all channels and pings, in the linear domain, with
    the integrated backscatter kept: what ``mask.frequency_differencing``, ``mask.detect_shoal`` or ``mask.apply_mask``
    need when channels (or, after ``combine_echodata``, pings) have different sample intervals, so that index ``s`` is
    another range in each.  Pings are not touched.  (No counterpart in the reference, whose ``commongrid.regrid`` is a
    stub; the rule is restated in NumPy in ``tests/regrid_ref.py``.)

    The grid is compute_MVBS's: edges ``e = np.arange(0, rmax + range_bin, range_bin)``, ``rmax`` from ``range_var_max``
    (a string such as ``"250m"``, plus 1e-8 as there) or the largest value of ``ds_Sv[range_var]``; ``J = len(e) - 1`` cells
    (0: an empty range axis), the output coordinate ``range_var`` holds their left edges.

    One row (channel, ping), ``r`` its range in float64 and ``v`` its Sv: ``n`` is the length of the leading run of
    finite ``r`` (samples behind it, the NaN tail of a padded row, are ignored).  Sample ``i`` stands for the interval
    ``[m[i], m[i+1])`` with ``m[i] = (r[i-1] + r[i]) / 2``, ``m[0] = r[0] - (r[1] - r[0]) / 2`` and ``m[n] = r[n-1] +
    (r[n-1] - r[n-2]) / 2``; repeated ranges give intervals of zero width, which contribute nothing.  With ``o_ij`` the
    length sample ``i`` shares with cell ``j``, ``W_j = sum o_ij`` and ``N_j = sum o_ij 10^(v_i/10)`` over the samples
    whose ``v`` is not NaN: ``Sv_j = 10 log10(N_j / W_j)`` where ``W_j > 0``, else NaN, and ``coverage_j = W_j /
    range_bin``.  ``-inf`` is a sample of linear value 0, ``+inf`` gives ``+inf``.  A row with ``n < 2`` or whose
    ``r[:n]`` decreases somewhere is all NaN with coverage 0 and is counted in ``n_rows_unordered``.  All arithmetic is
    float64, rounded once to the type of ``Sv`` (float32 or float64; other types are converted to float64 first).  For
    every row ``sum_j 10^(Sv_j/10) coverage_j range_bin`` equals the integral of the samples over the grid.

    ``ds_Sv["Sv"]`` has the dimensions ``(channel, ping_time, range_sample)`` (another order: ``NotImplementedError``),
    on the host or the device; ``ds_Sv[range_var]`` (``echo_range`` or ``depth``) any subset of them that includes
    ``range_sample``, of any real type.  Sharded datasets are not supported.

    Returns a Dataset with ``Sv`` over ``(channel, ping_time, range_var)`` on the device, ``coverage`` of the same shape
    and type (``with_coverage=False``: not written), ``n_rows_unordered`` (a 0-d int32 on the device, not read here), the
    coordinates ``channel``, ``ping_time`` and ``range_var``, and every variable of ``ds_Sv`` without ``range_sample``.
    It goes straight into ``mask.frequency_differencing`` and ``mask.apply_mask``; ``mask.detect_shoal`` works along a
    dimension called ``range_sample`` and takes the ``Sv`` array under that name.

    Device work: one launch (``epa_regrid_rows``), a workgroup per row; every output element is written exactly once.
    A range array is read where it lies, a lower-dimensional one through zero strides.  A deferred ``Sv`` and a lazy
    ``echo_range`` / ``depth`` are written first, as for any other reader: evaluating the range from its coefficient
    rows inside the kernel, and a float32 path for the exponential, are not built.  Host synchronisations: none with
    ``range_var_max``, else one (the largest range)."""
    ds_Sv = from_xarray(ds_Sv)
    if not isinstance(range_var, str):
        raise TypeError("The input range_var must be a string!")
    if "Sv" not in ds_Sv.variables:
        raise ValueError("Input Sv dataset must contain all of the following variables: {'Sv'}")
    ds_Sv, range_bin_m = _setup_and_validate(ds_Sv, range_var, range_bin)
    if not range_bin_m > 0:
        raise ValueError(f"range_bin must be positive, got {range_bin!r}")
    r_cap = range_cap(range_var_max, None)  # (TypeError / ValueError of a bad range_var_max)
    sv_da, rng = ds_Sv["Sv"], ds_Sv[range_var]
    order = tuple(sv_da.dims)
    if order != _REGRID_DIMS:
        raise NotImplementedError(f"the dimensions of Sv must be {_REGRID_DIMS}, got {order}")
    sizes = dict(zip(order, sv_da.shape))
    rdims = tuple(rng.dims)
    if len(set(rdims)) != len(rdims) or not set(rdims) <= set(order) or "range_sample" not in rdims:
        raise ValueError(f"The dimensions of {range_var}, {rdims}, must be among those of Sv, {order}, and include "
                         "'range_sample'.")
    if any(n != sizes[d] for d, n in zip(rdims, rng.shape)):
        raise ValueError(f"The shape of {range_var}, {dict(zip(rdims, rng.shape))}, does not match Sv, {sizes}.")
    for name, da in (("Sv", sv_da), (range_var, rng)):
        if not isinstance(da.data, DeviceArray) and np.asarray(da.data).dtype.kind not in "fiu":
            raise TypeError(f"{name} must hold real numbers, got {np.asarray(da.data).dtype}")

    if isinstance(sv_da.data, DeviceArray):
        sv_t = sv_da.data.tensor  # (a deferred Sv is written here)
        dev = sv_t.device
    else:
        dev = rng.data.tensor.device if isinstance(rng.data, DeviceArray) else resolve_device(device)
        sv_t = as_tensor(sv_da, device=dev)
    if sv_t.dtype not in (torch.float32, torch.float64):
        sv_t = sv_t.double()
    sv_t = sv_t.contiguous()
    rmax = r_cap if r_cap is not None else _largest_range(rng, range_var)
    r_edges = range_edges(rmax, range_bin_m)
    n_r = len(r_edges) - 1
    r_t = strided_view(rng, order, dev)
    if r_t.device != dev:
        r_t = r_t.to(dev)
    sv_rg, cov, n_bad = ops.regrid_rows(sv_t, r_t, range_bin_m, n_r, with_coverage=bool(with_coverage))

    out = Dataset(coords={"channel": ds_Sv["channel"], "ping_time": ds_Sv["ping_time"], range_var: r_edges[:-1]})
    out.coords[range_var].attrs = {"long_name": "Range distance", "units": "m"}
    dims = ("channel", "ping_time", range_var)
    out["Sv"] = DataArray(DeviceArray(sv_rg), dims, attrs={
        "long_name": "Volume backscattering strength (Sv re 1 m-1)", "units": "dB",
        "cell_methods": f"{range_var}: mean (interval: {range_bin_m} meter comment: {range_var} is the interval start)",
        "binning_mode": "physical units", "range_meter_interval": str(range_bin_m) + "m"})
    if cov is not None:
        out["coverage"] = DataArray(DeviceArray(cov), dims, attrs={
            "long_name": "Share of the cell that samples with a valid Sv fill", "units": "1"})
    out["n_rows_unordered"] = DataArray(DeviceArray(n_bad.reshape(())), (), attrs={
        "long_name": "Rows left NaN: fewer than two leading finite ranges, or ranges that decrease"})
    for k, c in ds_Sv.coords.items():
        if k not in out.coords and k != range_var and "range_sample" not in c.dims:
            out.coords[k] = c
    for k in ds_Sv.data_vars:
        v = ds_Sv[k]
        if k not in ("Sv", range_var) and "range_sample" not in v.dims:
            out[k] = v
    prov = echopype_prov_attrs(process_type="processing")
    prov["processing_function"] = "commongrid.regrid_Sv"
    out = out.assign_attrs({**prov, "range_var": range_var, "range_bin": range_bin, "regrid_cell_definition": _REGRID_CELLS})
    return insert_processing_level(out, "L3*", input_ds=ds_Sv)


@xarray_io()
def compute_MVBS_index_binning(ds_Sv, range_sample_num=100, ping_num=100):
    """MVBS over blocks of ``ping_num`` pings x ``range_sample_num`` samples (api.py:194-266)."""
    ds_Sv = from_xarray(ds_Sv)
    sv_da = ds_Sv["Sv"]
    order = tuple(sv_da.dims)
    sv_t = as_tensor(sv_da)
    if sv_t.dtype not in (torch.float32, torch.float64):
        sv_t = sv_t.double()
    rg_t = as_tensor(broadcast_to_dims(ds_Sv["echo_range"], ds_Sv, order), sv_t.dtype)
    mv, rmin = ops.mvbs_index(sv_t, ping_num, range_sample_num, range=rg_t)
    C, Pb, Sb = mv.shape
    ping_time = np.asarray(ds_Sv["ping_time"].values)
    ds_MVBS = Dataset(coords={order[0]: ds_Sv[order[0]].values, "ping_time": coarsen_time_mean(ping_time, ping_num)[:Pb],
                              "range_sample": np.arange(Sb)})
    ds_MVBS.coords["range_sample"].attrs = {"long_name": "Along-range sample number, base 0"}
    ds_MVBS["Sv"] = DataArray(DeviceArray(mv), (order[0], "ping_time", "range_sample"))
    ds_MVBS["echo_range"] = DataArray(DeviceArray(rmin), (order[0], "ping_time", "range_sample"))
    _set_MVBS_attrs(ds_MVBS)
    lo, hi = ops.nanminmax(mv)
    ds_MVBS.data_vars["Sv"].attrs.update({
        "cell_methods": (f"ping_time: mean (interval: {ping_num} pings "
                         "comment: ping_time is the interval start) "
                         f"range_sample: mean (interval: {range_sample_num} samples along range "
                         "comment: range_sample is the interval start)"),
        "comment": "MVBS binned on the basis of range_sample and ping number specified as index numbers",
        "binning_mode": "sample number",
        "range_sample_interval": f"{range_sample_num} samples along range",
        "ping_interval": f"{ping_num} pings",
        "actual_range": [round(float(lo), 2), round(float(hi), 2)],
    })
    prov = echopype_prov_attrs(process_type="processing")
    prov["processing_function"] = "commongrid.compute_MVBS_index_binning"
    ds_MVBS = ds_MVBS.assign_attrs(prov)
    if "frequency_nominal" in ds_Sv:
        ds_MVBS["frequency_nominal"] = ds_Sv["frequency_nominal"]
    return insert_processing_level(ds_MVBS, "L3*", input_ds=ds_Sv)


POSITION_VARIABLES = ["latitude", "longitude"]


@xarray_io()
def compute_NASC(ds_Sv, range_bin="10m", dist_bin="0.5nmi", method="map-reduce", skipna=True, closed="left",
                 **flox_kwargs):
    """Nautical Areal Scattering Coefficient on a (distance, depth) grid (api.py:269-416).
    ``ds_Sv`` must hold ``Sv``, ``depth``, ``latitude`` and ``longitude``; it may be an Sv dataset
    (dims channel, ping_time, range_sample) or an MVBS dataset gridded on depth."""
    ds_Sv = from_xarray(ds_Sv)
    range_var = "depth"
    ds_Sv, range_bin_m = _setup_and_validate(ds_Sv, range_var, range_bin, closed,
                                             required_data_vars=POSITION_VARIABLES)
    if not isinstance(dist_bin, str):
        raise TypeError("dist_bin must be a string")
    dist_bin_nmi = _parse_x_bin(dist_bin, "dist_bin")

    dist_nmi = get_distance_from_latlon(ds_Sv)  # O(P) on the host
    sv_da = ds_Sv["Sv"]
    order = tuple(sv_da.dims)
    dim_0 = order[0]
    sv_t = as_tensor(sv_da)
    if sv_t.dtype not in (torch.float32, torch.float64):
        sv_t = sv_t.double()
    dp_t = as_tensor(broadcast_to_dims(ds_Sv[range_var], ds_Sv, order), sv_t.dtype)
    C, P, S = sv_t.shape

    lo, hi, _ = _range_stats(ds_Sv[range_var], dp_t)
    r_edges = np.arange(0, hi + range_bin_m, range_bin_m)
    d_edges = np.arange(0, np.nanmax(dist_nmi) + dist_bin_nmi, dist_bin_nmi)
    n_r, n_d = len(r_edges) - 1, len(d_edges) - 1
    if n_r < 1 or n_d < 1:
        raise ValueError("NASC bins are empty: depth / distance hold no valid values")
    # cumulative distance is non-decreasing: the pings of a distance bin are contiguous
    side = "left" if closed == "left" else "right"
    starts = np.searchsorted(dist_nmi, d_edges, side=side).astype(np.int32)
    bin_start = ops.to_device(starts)

    nasc_t = ops.nasc(sv_t, dp_t, bin_start, n_d, range_bin_m, n_r, skipna=skipna, closed=closed)

    ds_NASC = Dataset(coords={"distance": d_edges[:-1], dim_0: ds_Sv[dim_0].values, range_var: r_edges[:-1]})
    ds_NASC["NASC"] = DataArray(DeviceArray(nasc_t), (dim_0, "distance", range_var))
    # per distance bin: mean position and mean ping_time (utils.py:453-501, :162-171)
    idx = np.searchsorted(d_edges, dist_nmi, side="right" if closed == "left" else "left") - 1
    inb = (idx >= 0) & (idx < n_d)
    for var in POSITION_VARIABLES:
        v = np.asarray(ds_Sv[var].values, dtype=np.float64)
        use = inb & ~np.isnan(v)
        ssum = np.bincount(idx[use], weights=v[use], minlength=n_d)
        cnt = np.bincount(idx[use], minlength=n_d)
        with np.errstate(invalid="ignore", divide="ignore"):
            ds_NASC[var] = (("distance",), np.where(cnt > 0, ssum / cnt, np.nan), dict(ds_Sv[var].attrs))
    ping_time = np.asarray(ds_Sv["ping_time"].values).astype("datetime64[ns]")
    ns = ping_time.astype(np.int64)
    valid_t = inb & ~np.isnat(ping_time)
    n_t = np.bincount(idx[valid_t], minlength=n_d)
    t0 = ns[valid_t].min() if valid_t.any() else 0
    tsum = np.bincount(idx[valid_t], weights=(ns[valid_t] - t0).astype(np.float64), minlength=n_d)
    with np.errstate(invalid="ignore", divide="ignore"):
        tmean = np.where(n_t > 0, t0 + np.round(tsum / np.maximum(n_t, 1)), np.iinfo(np.int64).min)
    ds_NASC["ping_time"] = (("distance",), tmean.astype(np.int64).astype("datetime64[ns]"),
                            dict(ds_Sv["ping_time"].attrs))
    if "frequency_nominal" in ds_Sv:
        ds_NASC["frequency_nominal"] = ds_Sv["frequency_nominal"]

    ds_NASC.data_vars["NASC"].attrs = {"long_name": "Nautical Areal Scattering Coefficient (NASC, m2 nmi-2)",
                                       "units": "m2 nmi-2"}
    ds_NASC.coords["distance"].attrs = {"long_name": "Cumulative distance", "units": "nmi"}
    ds_NASC.coords["depth"].attrs = {"long_name": "Cell depth", "units": "m", "standard_name": "depth"}
    tv = ping_time[~np.isnat(ping_time)]
    lat = np.asarray(ds_Sv["latitude"].values, dtype=np.float64)
    lon = np.asarray(ds_Sv["longitude"].values, dtype=np.float64)
    ds_NASC.attrs.update({
        "Conventions": "CF-1.7,ACDD-1.3",
        "time_coverage_start": np.datetime_as_string(tv.min(), timezone="UTC"),
        "time_coverage_end": np.datetime_as_string(tv.max(), timezone="UTC"),
        "geospatial_lat_min": round(float(np.nanmin(lat)), 5),
        "geospatial_lat_max": round(float(np.nanmax(lat)), 5),
        "geospatial_lon_min": round(float(np.nanmin(lon)), 5),
        "geospatial_lon_max": round(float(np.nanmax(lon)), 5),
    })
    return insert_processing_level(ds_NASC, "L4", input_ds=ds_Sv)
