"""Connected regions of a mask and one table row per region (no counterpart in the reference: there it is
``scipy.ndimage.label`` and a loop over the labels on the host).

``label_regions`` numbers the connected regions of a boolean (ping_time, range_sample) plane -- the result of
``detect_shoal``, ``frequency_differencing`` or one channel of ``line_mask`` -- and ``region_statistics`` reduces ``Sv``
and the range of every channel over each of them: where a school is, how big it is, its mean Sv at every frequency, its
NASC.  Regions are numbered 1..N in the raster order of their first pixel (smallest ``ping * S + sample``), which is
the numbering of ``scipy.ndimage.label``: results are reproducible and comparable pixel for pixel.

Device work, both functions: the union-find labelling the shoal detectors use (``epa_shoal_label``), one sweep over the
codes it leaves -- and, for the statistics, over the C planes of ``Sv`` and the range -- that fills one table entry per
(channel, region) (``epa_region_stats``), and one pass that writes the label plane (``epa_region_labels``).  Host
synchronisations: two, both through ``_to_host``: the labelling's error word and region count, then the tables (the host
orders the regions by their first pixel in between the sweep and the relabelling).  An empty mask ends after the
first.  Device memory besides the result: 8 B per pixel (the codes) and 20 B per entry of the labelling's table (one
entry per two pixels with connectivity 4, per four with 8), 4 B per pixel for ``region_label``, and the two result
tables: 88 B per (channel, region) and 16 B per region.

Measured on one MI355X at 4 x 20 000 x 4096 float32 with a full depth cube (``profiles/regions_bench.json``,
``scripts/bench_regions.py``): the sweep takes 14.6 ms on a tiled ``synth.shoal_scene`` mask (1.1 million mostly tiny
regions; 0.22 TB/s by 8 + 8 C bytes per pixel) against 370 ms for the same sums as torch ``index_add_`` on the
foreground pixels, and 3.5 ms on one region covering 5000 x 4096 pixels, where ``index_add_`` needs 37 s for one
channel.  Both sweep times are well above what reading the data alone would take (3.3 GB and 0.8 GB); where the time goes has not been
measured (the table updates, up to 13 words per run of equal code, are the likely place).  The whole call on the tiled
mask takes 1.0 s, with a million table rows ordered and decoded on the host."""
import numpy as np
import torch

from .. import ops
from ..device_view import device_view, resolve_device
from ..xr_lite import DataArray, Dataset, DeviceArray, from_xarray, is_device, xarray_io

_CORE = ("ping_time", "range_sample")
_NASC_FACTOR = 4 * np.pi * 1852.0 ** 2


def _to_host(t):
    """The one place these functions copy device data to the host (a synchronisation: the tests count them)."""
    return t.cpu()


def _check_connectivity(connectivity):
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _mask_array(mask):
    """``mask`` as a DataArray over (ping_time, range_sample) in either order, perhaps with a ``channel`` of length 1;
    checked on the host, nothing is moved."""
    mask = from_xarray(mask)
    if not isinstance(mask, DataArray):
        if isinstance(mask, torch.Tensor):
            data = DeviceArray(mask) if mask.is_cuda else mask.numpy()
        else:
            data = np.asarray(mask)
        if data.ndim != 2:
            raise ValueError(f"mask: a (ping_time, range_sample) plane expected, got an array of shape {tuple(data.shape)}")
        mask = DataArray(data, _CORE)
    dims = tuple(mask.dims)
    if "channel" in dims and mask.shape[dims.index("channel")] != 1:
        raise ValueError(f"mask has a channel dimension of length {mask.shape[dims.index('channel')]}: the regions are "
                         "those of one plane, select one (a mask of its own per channel is not supported)")
    rest = tuple(d for d in dims if d != "channel")
    if len(rest) != 2 or set(rest) != set(_CORE):
        raise ValueError(f"mask must have the dimensions ('ping_time', 'range_sample'), got {dims}")
    return mask


def _mask_plane(mask, device):
    """The checked ``mask`` as a contiguous bool (ping_time, range_sample) tensor on ``device``."""
    t = device_view(mask, ("channel",) + _CORE, device=device, index=0 if "channel" in mask.dims else None)
    return t if t.dtype == torch.bool else (t != 0)


def _mask_device(mask, device):
    if device is None and is_device(mask.data):
        return mask.data.tensor.device
    return resolve_device(device)


def _regions(plane, connectivity, sv=None, rng=None):
    """-> (int32 (P, S) device labels, N, tables): the host tables of ``ops.region_tables`` plus ``box`` (4, N), all
    in the order of the labels; None when N == 0."""
    P, S = plane.shape
    empty = torch.zeros((P, S), dtype=torch.int32, device=plane.device)
    if P == 0 or S == 0:
        return empty, 0, None
    state = ops.shoal_state(plane.device)
    code, table = ops.shoal_label(plane, connectivity, state)
    err, n = (int(v) for v in _to_host(state[:2]))  # synchronisation 1
    if err:
        raise RuntimeError(f"label_regions: {err} union-find loops reached their bound")
    if n == 0:
        return empty, 0, None
    stats, ids = ops.region_stats(code, n, state, sv, rng)
    box = table["box"][:, :n].to(torch.int64)
    flat = _to_host(torch.cat([ids.reshape(-1), stats.reshape(-1), box.reshape(-1), state[:1]])).numpy()  # 2
    if flat[-1]:
        raise RuntimeError(f"region_statistics: {int(flat[-1])} pixels carry a code outside the component table")
    n_ids, n_stats = ids.numel(), stats.numel()
    tabs = ops.region_tables(flat[n_ids:n_ids + n_stats].reshape(stats.shape), flat[:n_ids].reshape(ids.shape), P * S)
    tabs["box"] = flat[n_ids + n_stats:-1].reshape(4, n)
    order = np.argsort(tabs["first"], kind="stable")  # ids by their first pixel: label k + 1 is id order[k]
    rank = np.empty(n, dtype=np.int32)
    rank[order] = np.arange(1, n + 1, dtype=np.int32)
    labels = ops.region_labels(code, ops.to_device(rank, device=plane.device))
    return labels, n, {k: v[..., order] for k, v in tabs.items()}


def _label_array(labels, coords, n, connectivity):
    return DataArray(DeviceArray(labels), _CORE, coords=coords, name="region_label",
                     attrs={"n_regions": int(n), "connectivity": int(connectivity)})


def _core_coords(mask, other=None):
    out = {}
    for d, size in zip(_CORE, (mask.shape[mask.dims.index(_CORE[0])], mask.shape[mask.dims.index(_CORE[1])])):
        for src in (mask, other):
            if src is not None and d in src.coords and np.ndim(src.coords[d]) == 1 and len(src.coords[d]) == size:
                out[d] = np.asarray(getattr(src.coords[d], "values", src.coords[d]))
                break
        else:
            out[d] = np.arange(size)
    return out


@xarray_io()
def label_regions(mask, connectivity=8, *, device=None):
    """The connected regions of a boolean mask, numbered: int32 ``region_label`` (ping_time, range_sample), 0 on
    background and 1..N on the regions in the raster order of their first pixel (``scipy.ndimage.label``'s numbering,
    with the cross structure for ``connectivity=4`` and the full 3 x 3 one for 8).

    ``mask``: a DataArray over ping_time and range_sample in either order (a ``channel`` dimension of length 1 is
    dropped, a longer one raises ``ValueError``: select a plane), a ``torch.bool`` tensor or a NumPy array of that
    shape; on the device or the host; anything but bool counts as ``!= 0``.  Returns the DataArray with the mask's
    coordinates and the attributes ``n_regions`` and ``connectivity``; its data stays on the device, and
    ``region_label > 0`` is the mask again.

    Device work, the two host synchronisations and the memory: see the module."""
    connectivity = _check_connectivity(connectivity)
    mask = _mask_array(mask)
    plane = _mask_plane(mask, _mask_device(mask, device))
    labels, n, _ = _regions(plane, connectivity)
    return _label_array(labels, _core_coords(mask), n, connectivity)


@xarray_io()
def region_statistics(source_ds, mask, var_name="Sv", range_var="depth", connectivity=8, *, device=None):
    """One row per connected region of ``mask``: position, size, and the echo statistics of ``source_ds[var_name]`` at
    every channel.  The regions come from the one 2-D mask and are shared by all channels, so a row gives a school's
    mean Sv at every frequency.

    ``source_ds[var_name]``: (channel, ping_time, range_sample) in any order, or a plane without channel; float32 or
    float64.  ``source_ds[range_var]``: any subset of those dimensions -- (channel, ping_time, range_sample),
    (channel, range_sample), (range_sample,) ... -- read as it is, never expanded.  ``mask`` and ``connectivity``: as
    for ``label_regions``.  A missing variable, or a mask whose ping / sample lengths differ, raises ``ValueError``
    before any device work.

    All arithmetic is float64 (float32 inputs are converted, which is exact).  With ``sv = 10 ** (Sv / 10)``, ``r`` the
    range variable and ``dz[s] = r[s] - r[s-1]`` (``dz[0] = dz[1]``; NaN with a single sample), every sum and extremum
    below runs over the pixels of the region and skips those where one of its own operands is NaN.

    Returns a Dataset with the coordinate ``region`` = 1..N (and ``channel`` when the source has one), the
    device-resident ``region_label`` of ``label_regions``, and NumPy variables.  On ``region``:

    - ``n_samples``: pixels;  ``ping_first``, ``ping_last``, ``sample_first``, ``sample_last``: the bounding box;
      ``n_pings = ping_last - ping_first + 1``;  ``ping_time_start``, ``ping_time_end``: the coordinate at the box.

    On (``channel``, ``region``):

    - ``n_valid``: pixels whose Sv is not NaN;
    - ``Sv_mean = 10 log10(sum sv / n_valid)`` (NaN when ``n_valid == 0``);  ``Sv_max`` (NaN when there is none);
    - ``{range_var}_min``, ``{range_var}_max``, ``{range_var}_mean`` over the non-NaN ``r``;
    - ``center_of_mass = sum(sv r) / sum(sv)`` over the pixels with both;
    - ``height_mean = sum(dz) / n_pings``: the mean thickness;
    - ``NASC = 4 pi 1852**2 sum(sv dz) / n_pings`` over the pixels with Sv and dz.

    An empty mask (or no pings, or no samples) gives the same variables with a ``region`` of length 0; no statistics
    kernel runs.  Counts, the box and the extrema are the same from call to call; the sums are added in the order the
    device delivers them and can differ in their last bits.

    Device work, the two host synchronisations and the memory: see the module; the table comes back in one download."""
    connectivity = _check_connectivity(connectivity)
    source_ds = from_xarray(source_ds)
    for name, v in (("var_name", var_name), ("range_var", range_var)):
        if not isinstance(v, str) or v not in source_ds:
            raise ValueError(f"The Dataset source_ds does not contain the variable {name}={v!r}!")
    mask = _mask_array(mask)
    src, rng = source_ds[var_name], source_ds[range_var]
    order = tuple(src.dims)
    has_chan = "channel" in order
    if len(set(order)) != len(order) or set(order) != set(_CORE) | ({"channel"} if has_chan else set()):
        raise ValueError(f"{var_name} must have the dimensions (channel, ping_time, range_sample) or "
                         f"(ping_time, range_sample), got {order}")
    sizes = dict(zip(order, src.shape))
    for d in _CORE:
        if mask.shape[mask.dims.index(d)] != sizes[d]:
            raise ValueError(f"mask: dimension {d!r} has length {mask.shape[mask.dims.index(d)]}, {var_name} has "
                             f"{sizes[d]}")
    rdims = tuple(rng.dims)
    if len(set(rdims)) != len(rdims) or not set(rdims) <= set(order):
        raise ValueError(f"The dimensions of {range_var}, {rdims}, must be among those of {var_name}, {order}.")
    if any(n != sizes[d] for d, n in zip(rdims, rng.shape)):
        raise ValueError(f"The shape of {range_var}, {dict(zip(rdims, rng.shape))}, does not match {var_name}, {sizes}.")
    for da, what in ((src, var_name), (rng, range_var)):
        if not is_device(da.data) and np.asarray(da.data).dtype.kind not in "fiu":
            raise TypeError(f"{what} must hold real numbers, got {np.asarray(da.data).dtype}")

    if device is None and is_device(src.data):
        dev = src.data.tensor.device
    else:
        dev = _mask_device(mask, device)
    full = ("channel",) + _CORE
    plane = _mask_plane(mask, dev)
    sv = device_view(src, full, device=dev, floating=True)
    if not has_chan:
        sv = sv.unsqueeze(0)
    r_t = device_view(rng, full, device=dev, floating=True)
    if sv.dtype != r_t.dtype:
        sv, r_t = sv.double(), r_t.double()
    r_t = r_t[tuple(slice(None) if d in rdims else None for d in full)]  # a broadcast axis where the range has none
    labels, n, tabs = _regions(plane, connectivity, sv, r_t)

    C = sv.shape[0]
    coords = _core_coords(mask, src)
    out = Dataset(coords={"region": np.arange(1, n + 1, dtype=np.int32)})
    if has_chan and "channel" in src.coords:
        out._set_coord("channel", src.coords["channel"])
    out["region_label"] = _label_array(labels, coords, n, connectivity)
    if tabs is None:
        i0 = np.zeros(0, dtype=np.int64)
        f0 = np.zeros((C, 0), dtype=np.float64)
        tabs = {"n_samples": i0, "box": np.zeros((4, 0), dtype=np.int64), "n_valid": f0.astype(np.int64),
                "n_range": f0.astype(np.int64), **{k: f0 for k in ("sv_max", "range_min", "range_max", "sum_sv", "sum_range",
                                                                   "sum_sv_range", "sum_sv_at_range", "sum_dz",
                                                                   "sum_sv_dz")}}
    s0, s1, p0, p1 = tabs["box"]
    n_pings = p1 - p0 + 1
    pt = coords["ping_time"]
    for k, v in (("n_samples", tabs["n_samples"]), ("ping_first", p0), ("ping_last", p1), ("sample_first", s0),
                 ("sample_last", s1), ("ping_time_start", pt[p0]), ("ping_time_end", pt[p1]), ("n_pings", n_pings)):
        out[k] = (("region",), v)
    with np.errstate(divide="ignore", invalid="ignore"):
        nv, nr = tabs["n_valid"], tabs["n_range"]
        per_chan = {
            "n_valid": nv,
            "Sv_mean": np.where(nv > 0, 10.0 * np.log10(tabs["sum_sv"] / nv), np.nan),
            "Sv_max": tabs["sv_max"],
            f"{range_var}_min": tabs["range_min"],
            f"{range_var}_max": tabs["range_max"],
            f"{range_var}_mean": np.where(nr > 0, tabs["sum_range"] / nr, np.nan),
            "center_of_mass": tabs["sum_sv_range"] / tabs["sum_sv_at_range"],
            "height_mean": tabs["sum_dz"] / n_pings,
            "NASC": _NASC_FACTOR * tabs["sum_sv_dz"] / n_pings,
        }
    for k, v in per_chan.items():
        out[k] = (("channel", "region"), v) if has_chan else (("region",), v[0])
    return out
