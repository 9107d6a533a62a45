"""Target tracking: the single targets of one fish over consecutive pings grouped into a track (no counterpart in the
reference; on the host this is a Python loop over pings and targets).

``track_targets`` takes the table ``detect_single_targets`` leaves in HBM and returns, still in HBM, the track of every
target and one row of statistics per track.  The rules are THIS PROJECT'S: gated nearest-neighbour linking after
Echoview's "fish track detection" (gates per axis, gate expansion over missed pings, a weighted cost, a maximum gap, a
minimum track length), with the sequential alpha-beta predictor replaced by a fixed number of propose / accept rounds so
that no step waits for another ping.  They have never been run against Echoview nor on recorded data.
``tests/track_ref.py`` restates them in NumPy and is the judge of the kernels.

Device work (csrc/track.hip), in this order: ``track_prepare_kernel`` (positions, the start of every (channel, ping)
segment, the verdict on the table); ``link_rounds`` times ``track_propose_kernel`` and ``track_accept_kernel``;
``ceil(log2(max(P, 2)))`` times ``track_roots_kernel`` (pointer doubling; the host knows the number); ``track_chains_kernel``
(a flag and a length per chain that is a track); one torch ``cumsum`` over both; the ONE host synchronisation, through
``_to_host``: the number of tracks, the number of targets in tracks and the verdict; then, if there is a track,
``track_order_kernel`` and ``track_table_kernel``.  The per-channel counts and the four time columns are torch
plumbing on the finished columns (integer ``index_add_``, ``index_select``, one division)."""
import numbers

import numpy as np
import torch

from .. import _lib, ops
from ..device_view import as_tensor, resolve_device
from ..xr_lite import DataArray, Dataset, DeviceArray, from_xarray, is_device, xarray_io

_ICOLS = ("channel_index", "ping_index")
_FCOLS = ("target_range", "angle_alongship", "angle_athwartship", "TS_comp")
_GATES = ("gate_alongship", "gate_athwartship", "gate_range")
_WEIGHTS = ("weight_alongship", "weight_athwartship", "weight_range", "weight_TS", "weight_ping_gap")
_INTS = {"max_ping_gap": 0, "link_rounds": 1, "min_targets": 1, "min_pings": 1}  # the least value of each
DEFAULTS = {"max_ping_gap": 2, "missed_ping_expansion": 0.0, "weight_alongship": 30.0, "weight_athwartship": 30.0,
            "weight_range": 40.0, "weight_TS": 0.0, "weight_ping_gap": 0.0, "max_TS_difference": None, "link_rounds": 3,
            "min_targets": 3, "min_pings": 3}
_INT_MAX = 2 ** 30


def _to_host(t):
    """The one place this module copies device data to the host (a synchronisation: the tests count them)."""
    return t.cpu()


def _check_params(params):
    """The keys and numbers of ``params``, checked on the host -> all of them, defaults filled in."""
    if not isinstance(params, dict):
        raise ValueError(f"params must be a dict, got {type(params).__name__}")
    known = _GATES + tuple(DEFAULTS)
    unknown = sorted(k for k in params if k not in known)
    if unknown:
        raise ValueError(f"Unknown tracking parameter(s) {unknown}; known: {sorted(known)}")
    missing = [k for k in _GATES if k not in params]
    if missing:
        raise ValueError(f"Missing tracking parameter(s) {missing}")
    out = {**DEFAULTS, **params}
    for k, v in out.items():
        if k == "max_TS_difference" and v is None:
            continue
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.integer, np.floating)) \
                or not np.isfinite(float(v)):
            raise ValueError(f"{k} must be a finite real number, got {v!r}")
    for k in _GATES:
        if not out[k] > 0:
            raise ValueError(f"{k} must be positive, got {out[k]!r}")
        out[k] = float(out[k])
    for k, least in _INTS.items():
        if float(out[k]) != int(out[k]) or not least <= out[k] <= _INT_MAX:
            raise ValueError(f"{k} must be an integer >= {least} (and <= 2**30), got {out[k]!r}")
        out[k] = int(out[k])
    for k in ("missed_ping_expansion",) + _WEIGHTS:
        if out[k] < 0:
            raise ValueError(f"{k} must not be negative, got {out[k]!r}")
        out[k] = float(out[k])
    if not any(out[k] > 0 for k in _WEIGHTS):
        raise ValueError(f"the weights {list(_WEIGHTS)} must not all be zero")
    if out["max_TS_difference"] is not None:
        if not out["max_TS_difference"] > 0:
            raise ValueError(f"max_TS_difference must be positive or None, got {out['max_TS_difference']!r}")
        out["max_TS_difference"] = float(out["max_TS_difference"])
    elif out["weight_TS"] > 0:
        raise ValueError("weight_TS > 0 needs max_TS_difference")
    return out


def _coordinate(ds, name):
    if name not in ds.coords or np.ndim(ds.coords[name]) != 1:
        raise ValueError(f"The target table has no {name} coordinate")
    c = ds.coords[name]
    return np.asarray(getattr(c, "values", c))


def _index_column(da, dev):
    """An index column as int32; what int32 cannot hold stays out of range (-1 or 2**31 - 1) instead of wrapping."""
    t = as_tensor(da, None, dev)
    if t.dtype != torch.int32:
        t = t.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    return t.contiguous()


def _gated_nearest(ds, params, device):
    prm = _check_params(params)
    for name in _ICOLS + _FCOLS:
        if name not in ds:
            raise ValueError(f"The target table does not contain the column {name!r}!")
    chan, ptime = _coordinate(ds, "channel"), _coordinate(ds, "ping_time")
    C, P = len(chan), len(ptime)
    n = int(ds["channel_index"].shape[0]) if ds["channel_index"].ndim == 1 else -1
    has_time = "target_ping_time" in ds
    for name in _ICOLS + _FCOLS + (("target_ping_time",) if has_time else ()):
        da = ds[name]
        if tuple(da.dims) != ("target",) or da.shape != (n,):
            raise ValueError(f"{name} must be a column on target of {n} rows, got {dict(zip(da.dims, da.shape))}")
        kind = da.dtype.kind
        if kind not in ("iu" if name in _ICOLS else "fiu" if name in _FCOLS else "iuM"):
            raise ValueError(f"{name} holds {kind!r} data")
    if C * P >= 2 ** 31 - 256 or n >= 2 ** 31 - 256:
        raise ValueError(f"track_targets takes fewer than 2**31 - 256 rows and segments, got {n} and {C * P}")
    if n > 0 and C * P == 0:
        raise ValueError("The target table has rows but no channel or no ping: every index is out of range")

    first = ds["channel_index"].data
    dev = first.tensor.device if device is None and is_device(first) else resolve_device(device)

    def empty_tracks():
        return (torch.zeros((len(_lib.TRACK_ICOL_NAMES), 0), dtype=torch.int32, device=dev),
                torch.zeros((len(_lib.TRACK_FCOL_NAMES), 0), dtype=torch.float64, device=dev))

    tpt = None
    if n == 0:
        track_id = succ = torch.zeros(0, dtype=torch.int32, device=dev)
        xyz = torch.zeros((3, 0), dtype=torch.float64, device=dev)
        ci = track_id
        if has_time:
            tpt = torch.zeros(0, dtype=torch.int64, device=dev)
        icols, fcols = empty_tracks()
    else:
        ci, pi = (_index_column(ds[k], dev) for k in _ICOLS)
        rng, al, at, ts = (as_tensor(ds[k], torch.float64, dev).contiguous() for k in _FCOLS)
        if has_time:
            d = ds["target_ping_time"].data
            if not is_device(d) and np.asarray(d).dtype.kind == "M":
                d = np.asarray(d).astype("datetime64[ns]").view(np.int64)
            tpt = as_tensor(d, torch.int64, dev).contiguous()
        seg, xyz, succ, pred, bad = ops.track_prepare(ci, pi, rng, al, at, C, P)
        prop = torch.empty(n, dtype=torch.int32, device=dev)
        gates = [0.0 if prm[k] is None else float(prm[k]) for k in _lib.TRACK_PARAM_NAMES]
        for _ in range(prm["link_rounds"]):
            ops.track_link_round(ci, pi, xyz, ts, C, P, seg, gates, succ, pred, prop)
        # a chain's pings strictly increase: it has at most P rows, which this many doubling passes resolve
        root, rank = ops.track_roots(pred, (max(P, 2) - 1).bit_length())
        flag_len = ops.track_chains(pi, xyz, ts, succ, root, rank, prm["min_targets"], prm["min_pings"])
        scans = torch.stack([torch.cumsum(row, 0, dtype=torch.int64) for row in flag_len])  # (1-D scans: device-wide)
        # the one synchronisation: the number of tracks sizes their table; the verdict on the table comes with it
        T, M, wrong = (int(v) for v in _to_host(torch.cat([scans[:, -1], bad.to(torch.int64)])))
        if wrong:
            raise ValueError("The target table is not ordered by (channel_index, ping_index), or holds an index outside "
                             f"its {C} channels and {P} pings")
        if T == 0:
            track_id = torch.zeros(n, dtype=torch.int32, device=dev)
            icols, fcols = empty_tracks()
        else:
            track_id, icols, fcols = ops.track_table(ci, pi, rng, ts, xyz, root, rank, flag_len, scans, T, M)

    T = icols.shape[1]
    out = Dataset(coords={"channel": chan, "ping_time": ptime, "target": np.arange(n, dtype=np.int64),
                          "track": np.arange(1, T + 1, dtype=np.int64)},
                  attrs={"method": "gated_nearest", **{k: (float("nan") if v is None else v) for k, v in prm.items()}})

    def put(name, t, dim):
        out[name] = DataArray(DeviceArray(t), (dim,), name=name)

    put("track_id", track_id, "target")
    for k, name in enumerate("xyz"):
        put(name, xyz[k], "target")
    put("next_target", succ, "target")
    for k, name in enumerate(_lib.TRACK_ICOL_NAMES):
        put(name, icols[k], "track")
    for k, name in enumerate(_lib.TRACK_FCOL_NAMES):
        put(name, fcols[k], "track")
    if has_time:
        t_first = tpt.index_select(0, icols[_lib.TRACK_ICOL_NAMES.index("target_first")].to(torch.int64))
        t_last = tpt.index_select(0, icols[_lib.TRACK_ICOL_NAMES.index("target_last")].to(torch.int64))
        duration = (t_last - t_first).to(torch.float64) / 1e9
        put("time_first", t_first, "track")
        put("time_last", t_last, "track")
        put("duration", duration, "track")
        put("speed", fcols[_lib.TRACK_FCOL_NAMES.index("path_length")] / duration, "track")
    rows = ci.to(torch.int64)

    def per_channel(index, what):
        return torch.zeros(C, dtype=torch.int64, device=dev).index_add_(0, index, what.to(torch.int64))

    put("n_tracks", per_channel(icols[0].to(torch.int64), torch.ones(T, dtype=torch.int64, device=dev)), "channel")
    put("n_links", per_channel(rows, succ >= 0), "channel")
    put("n_tracked_targets", per_channel(rows, track_id > 0), "channel")
    return out


# Registry of supported methods for target tracking
METHODS_TRACK = {
    "gated_nearest": _gated_nearest,
}


@xarray_io()
def track_targets(targets, method, params, *, device=None):
    """Group the single targets of a target table into fish tracks and return the track of every target and one row of
    statistics per track.

    ``method``: ``"gated_nearest"`` (the only one; another raises ``ValueError`` naming the methods).

    ``targets``: the Dataset ``detect_single_targets`` returns, or any Dataset of the same form (that table after rows
    were dropped, for instance).  Read from it: the columns ``channel_index``, ``ping_index``, ``target_range``,
    ``angle_alongship``, ``angle_athwartship``, ``TS_comp`` on ``target``; the lengths C and P of its ``channel`` and
    ``ping_time`` coordinates; and, if present, ``target_ping_time`` as int64 nanoseconds.  Float columns of another
    float type are converted to float64; all arithmetic is float64.  The rows must be ordered by (``channel_index``,
    ``ping_index``), as the detector writes them; the per-(channel, ping) segments are derived from those two columns on
    the device, NOT from ``n_targets`` (stale once rows were dropped).  A table that is not ordered, or holds an index
    outside [0, C) x [0, P), raises ``ValueError``: that verdict comes back with the one host synchronisation, and the
    kernels are memory-safe on any table content.  A missing column raises ``ValueError`` and names it, before any device
    work.  Sharded datasets are not supported.

    ``params``: a dict.  Required and positive, in metres: ``gate_alongship``, ``gate_athwartship``, ``gate_range``.
    Optional: ``max_ping_gap`` (int >= 0, default 2: the pings a track may miss in a row); ``missed_ping_expansion``
    (per cent >= 0, default 0); ``weight_alongship``, ``weight_athwartship``, ``weight_range``, ``weight_TS``,
    ``weight_ping_gap`` (each >= 0; defaults 30, 30, 40, 0, 0; not all zero); ``max_TS_difference`` (dB > 0, default None:
    no TS gate; ``weight_TS > 0`` needs it); ``link_rounds`` (int >= 1, default 3); ``min_targets`` (int >= 1, default
    3); ``min_pings`` (int >= 1, default 3).  An unknown key, a missing required key, a non-finite or non-real value, or
    a value outside its domain raises ``ValueError`` before any device work.

    The rules are this project's; they have never been run against Echoview nor on recorded data.

    1. **Position.**
       - ``u = tan(angle_alongship * pi / 180)``, ``v = tan(angle_athwartship * pi / 180)``.
       - ``z = target_range / sqrt(1 + u² + v²)``, ``x = z u``, ``y = z v``.
       - A target with NaN in ``x``, ``y``, ``z`` or ``TS_comp`` is never linked and gets ``track_id`` 0.
    2. **Gate.**
       - A pair (i, j) is gated only if both targets are in the same channel and ``k = ping_j - ping_i - 1`` satisfies
         ``0 <= k <= max_ping_gap``.
       - ``f = 1 + k * missed_ping_expansion / 100``.
       - ``dx = |x_j - x_i| / (f * gate_alongship)``, and ``dy`` (athwartship), ``dz`` (range) likewise.
       - The pair passes if ``dx <= 1``, ``dy <= 1`` and ``dz <= 1``.
       - With ``max_TS_difference`` set, ``dT = |TS_j - TS_i| / max_TS_difference <= 1`` must hold as well.
       - Targets of different channels never link.
    3. **Cost.** ``c = w_al dx² + w_at dy² + w_r dz² + w_TS dT² + w_gap k / max(max_ping_gap, 1)``, added in this order,
       every operation rounded on its own.  The TS term is left out when ``weight_TS`` is 0.
    4. **Linking.**
       - Every target has at most one successor ``succ`` and one predecessor ``pred``; both start empty.
       - ``link_rounds`` rounds of two steps are run.
       - *Propose*: every target ``i`` without a successor proposes to the gated ``j`` without a predecessor that
         minimises ``(c, j)`` lexicographically: the lower table index wins a tie.
       - *Accept*: every ``j`` without a predecessor accepts, among the targets that proposed to it in this round, the
         one minimising ``(c, i)``.  Then ``pred[j] = i`` and ``succ[i] = j``.
       - All rounds are always run.  No step reads the host.
    5. **Tracks.**
       - The chains of ``succ`` / ``pred`` are the candidate tracks; a lone target is a chain of one.
       - A chain is a track if it has at least ``min_targets`` members and spans at least ``min_pings`` pings, counted
         as ``ping_last - ping_first + 1``.
       - Tracks are numbered 1 .. T by the table index of their first target.  Every other target has ``track_id`` 0.

    Returns one Dataset, all of it resident on the device, with the input's ``channel`` and ``ping_time`` coordinates.
    On ``target``: ``track_id`` (int32), ``x``, ``y``, ``z`` (float64) and ``next_target`` (int32: ``succ``, or -1; the
    links of rejected chains are kept there).  On ``track`` (length T, labelled 1 .. T): ``channel_index``,
    ``n_targets``, ``ping_first``, ``ping_last``, ``target_first``, ``target_last`` (int32); ``TS_mean`` (``10 log10``
    of the mean of ``10^(TS_comp/10)`` over the track's targets), ``TS_max``, ``range_mean``, ``x_first``, ``y_first``,
    ``z_first``, ``x_last``, ``y_last``, ``z_last``, ``path_length`` (the sum of the Euclidean lengths of the track's
    links), ``displacement`` (first to last), ``tortuosity`` (``path_length / displacement``, IEEE division) and
    ``delta_range`` (``z_last - z_first``); with ``target_ping_time`` also ``time_first``, ``time_last`` (int64 ns),
    ``duration`` (seconds) and ``speed`` (``path_length / duration``, IEEE division), without it these four are absent.
    On ``channel``: ``n_tracks``, ``n_links``, ``n_tracked_targets`` (int64).  The parameters go into ``attrs`` (``None``
    as NaN).  An empty table, or no track found, gives the same variables with ``track`` of length 0.  Two calls on the
    same input give bit-identical output: every per-track sum is taken in an order fixed by the data (lane l of a wave
    adds the track's targets l, l + 64, ... in chain order, then the 64 partial sums are added in a fixed tree), and
    there are no floating-point atomics.

    Device work and the one host synchronisation: see the module."""
    ds = from_xarray(targets)
    if method not in METHODS_TRACK:
        raise ValueError(f"Unsupported target tracking method: {method!r}; supported: {sorted(METHODS_TRACK)}")
    return METHODS_TRACK[method](ds, params, device)
