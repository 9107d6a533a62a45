"""``combine_echodata``: many files into one ``EchoData`` whose sample volumes are resident in HBM, with the reference's
signature, checks, exception types and messages (echopype echodata/combine.py:104-602, 691-976).

Per group, as the reference's ``_combine``: the append dimensions are ``filenames`` and the seven time dimensions; a group
without one is the first file's; a variable that has exactly one of them is concatenated along it (one that has several
is dropped, as ``drop_dims`` does there); a variable that has none must agree between the files wherever both hold a
value (``compat="no_conflicts"``, else ``ValueError``), the first value that is not null wins.  Variable attributes are the
first file's, group attributes come from ``_merge_attributes``.  ``range_sample`` is the union ``arange(max S_i)``: shorter
files are NaN-padded (xarray's outer join).

Two rules are xarray's, taken from its documented behaviour because xarray is not installed where this was written:

* channel order -- with ``channel_selection`` the sorted selection; otherwise the first file's order when all files agree,
  else the sorted union (the outer alignment of unequal indexes sorts);
* dtypes after a pad (``dtypes.maybe_promote``) -- floats, complex and times keep their type, integers of at most 2 bytes
  become float32, wider ones float64; an integer variable none of whose files is padded stays integer.

Residency: a variable comes out as a ``DeviceArray`` when ``EchoData.to_device`` would move it (float, two or more
dimensions, in a beam group or ``Environment``) or when any input holds it resident.  Host inputs are uploaded file by
file and joined on the device -- the padding never crosses PCIe.  ``(channel, time, range_sample[, beam])`` variables are
ONE launch of ``epa_concat_rows`` each, however many files; ``(channel, time)`` parameters are ``torch.cat`` /
``index_select`` and keep a host mirror that cannot be written to when every input has one; everything else is joined in
NumPy on the host, and a resident variable among that (another layout, float16, bool, complex, unsigned) is uploaded
again with a host mirror -- only a type no device tensor holds stays on the host.  A channel selection is never applied
to the files' cubes: it is the kernel's channel map, so selected data are read once.  The combined ``ping_time`` of a beam group is resident like ``to_device`` leaves it, with the verdict of
``epa_time_reversals`` on it: a seam that steps backwards is known at once and nothing rescans or uploads the times later.

Deviations: an input that is itself combined raises ``NotImplementedError``; a group missing from some inputs raises
``ValueError``; a ``beam`` (or any other non-append, non-``range_sample``) coordinate that differs raises
``NotImplementedError``; a dict ``channel_selection`` whose lists hold anything but strings raises ``TypeError`` (the
reference's check looks at the keys and never fires); an empty ``echodata_list``, like anything that is not a list, raises
``TypeError`` (the reference: ``IndexError``); the parameters of ``Vendor_specific`` are compared channel by channel label, so files whose
channels come in another order combine (the reference's ``Dataset.identical`` refuses them); the inputs are not consumed -- the caller frees them; a ``Provenance`` group is created when no
input has one."""
import itertools
import re
from pathlib import Path
from warnings import warn

import numpy as np

from .echodata import BEAM1, BEAM2, EchoData
from .utils.prov import echopype_prov_attrs
from .xr_lite import DataArray, Dataset, DeviceArray, host_readable

POSSIBLE_TIME_DIMS = {"time1", "time2", "time3", "time4", "nmea_time", "ping_time", "filter_time"}
APPEND_DIMS = {"filenames"}.union(POSSIBLE_TIME_DIMS)
ED_GROUP = "echodata_group"
ED_FILENAME = "echodata_filename"
FILENAMES = "filenames"
RESIDENT_GROUPS = (BEAM1, BEAM2, "Environment")


# ---- the checks: the reference's signatures, exception types and messages, in this package's own words ------------------------
EK80_LIKE = ("EK80", "ES80", "EA640")
SHARED_CHANNEL_GROUPS = ("Sonar", "Platform", "Vendor_specific")  # EK80: these hold the channels of every beam group
_BEAM_GROUP_PATH = re.compile(r"Sonar/Beam_group\d")


def _check_channel_selection_form(channel_selection=None):
    """``channel_selection`` must be None, a list of str, or a dict of beam group path -> list of str (``TypeError``)."""
    if channel_selection is None:
        return
    if isinstance(channel_selection, list):
        if any(not isinstance(name, str) for name in channel_selection):
            raise TypeError("Each element of channel_selection must be a string!")
        return
    if not isinstance(channel_selection, dict):
        raise TypeError("The input channel_selection does not have an acceptable type!")
    for path in channel_selection:
        if not isinstance(path, str):
            raise TypeError("Each key of channel_selection must be a string!")
    for path in channel_selection:
        if _BEAM_GROUP_PATH.match(path) is None:
            raise TypeError("Each key of channel_selection can only be a beam group path of the form Sonar/Beam_group!")
    for names in channel_selection.values():
        if not isinstance(names, list):
            raise TypeError("Each value of channel_selection must be a list!")
    for names in channel_selection.values():
        if any(not isinstance(name, str) for name in names):
            raise TypeError("Each value of channel_selection must be a list of strings!")


def check_eds(echodata_list):
    """-> (sonar_model, file names).  All objects must name one sonar model (``ValueError``).  A file's name is the last
    component of ``source_file``, else of ``converted_raw_path``, else "internal-memory"; a name taken from a path that an
    earlier object already has raises ``ValueError``.  Anything but a non-empty list raises ``TypeError``."""
    if not isinstance(echodata_list, list) or not echodata_list:
        raise TypeError("The input, eds, must be a list of EchoData objects!")
    models = [ed.sonar_model for ed in echodata_list]
    if None in models:
        raise ValueError("all EchoData objects must have non-None sonar_model values")
    if any(m != models[0] for m in models):
        raise ValueError("all EchoData objects must have the same sonar_model value")
    names = []
    for ed in echodata_list:
        path = next((p for p in (ed.source_file, ed.converted_raw_path) if p is not None), None)
        if path is None:  # made in memory: several of those may be combined
            names.append("internal-memory")
            continue
        name = Path(path).name
        if name in names:
            raise ValueError("EchoData objects have conflicting filenames")
        names.append(name)
    return models[0], names


def _check_channel_consistency(all_chan_list, ed_group, channel_selection=None):
    """``all_chan_list``: the channel names of every file's group ``ed_group``.  Without a selection all files must hold the
    same names, in any order (``RuntimeError``); with one, every file must hold every selected name
    (``NotImplementedError``: padding a missing channel is not built)."""
    if channel_selection is not None:
        wanted = set(channel_selection)
        if any(not wanted <= set(names) for names in all_chan_list):
            raise NotImplementedError(
                f"For the EchoData group {ed_group}, some EchoData objects do not contain the selected channels. "
                "This type of combine is not currently implemented.")
        return
    reference_names = sorted(all_chan_list[0])
    if any(sorted(names) != reference_names for names in all_chan_list[1:]):
        unique_channels = set().union(*all_chan_list)
        raise RuntimeError(
            f"For the EchoData group {ed_group} the channels: {unique_channels} are not found in all EchoData objects "
            "being combined. Select which channels should be included in the combination using the keyword argument "
            "channel_selection in combine_echodata.")


def _create_channel_selection_dict(sonar_model, has_chan_dim, user_channel_selection=None):
    """group -> the sorted channel names to keep there, None for a group without a ``channel`` dimension or without a
    selection.  A list selects the same names everywhere.  A dict gives each beam group of an EK80-like sonar its own
    entry (``KeyError`` without one) and the union of all entries to ``Sonar``, ``Platform`` and ``Vendor_specific``; for
    other sonars every group takes the union.  Two observable details are the reference's: the groups that take the
    union share ONE list object, and a dict's own lists are sorted in place (a list argument is copied first)."""
    if user_channel_selection is None:
        return dict.fromkeys(has_chan_dim)
    by_beam_group = isinstance(user_channel_selection, dict) and sonar_model in EK80_LIKE
    if isinstance(user_channel_selection, dict):
        union = list({name for names in user_channel_selection.values() for name in names})
    else:
        union = list(user_channel_selection)
    union.sort()
    selection = {}
    for group, has_channel in has_chan_dim.items():
        if not has_channel:
            selection[group] = None
        elif by_beam_group and group not in SHARED_CHANNEL_GROUPS:
            own = user_channel_selection[group]
            own.sort()
            selection[group] = own
        else:
            selection[group] = union
    return selection


def _channels(ds):
    return [c.item() if hasattr(c, "item") else c for c in np.asarray(ds["channel"].values).reshape(-1)]


def _check_echodata_channels(echodata_list, user_channel_selection=None):
    """group -> selected channels (:func:`_create_channel_selection_dict`), after every group of the first file that has a
    ``channel`` dimension has been checked in all files: the group is there (``ValueError``), no file repeats a channel
    name (``RuntimeError``), and :func:`_check_channel_consistency`."""
    first = echodata_list[0]
    with_channel = {group: "channel" in first[group].dims for group in first.group_paths}
    selection = _create_channel_selection_dict(first.sonar_model, with_channel, user_channel_selection)
    for group in (g for g, has in with_channel.items() if has):
        if any(group not in ed or "channel" not in ed[group] for ed in echodata_list):
            raise ValueError(f"The EchoData group {group} with its channel coordinate is not found in all "
                             "EchoData objects being combined.")
        names_per_file = [_channels(ed[group]) for ed in echodata_list]
        repeating = [_source_name(ed) for ed, names in zip(echodata_list, names_per_file) if len(set(names)) < len(names)]
        if repeating:
            raise RuntimeError("The EchoData objects produced by the following files have a channel dimension with "
                               f"repeating values, combine cannot be used: {repeating}")
        _check_channel_consistency(names_per_file, group, selection[group])
    return selection


def _source_name(ed):
    if "Provenance" in ed and "source_filenames" in ed["Provenance"]:
        return ed["Provenance"]["source_filenames"].values[0]
    return ed.source_file if ed.source_file is not None else ed.converted_raw_path


def _check_ascending_ds_times(ds_list, ed_group):
    """For every time dimension of the group: the FIRST time of a file must not lie before the first time of the file in
    front of it (``RuntimeError``).  A comparison with NaT never fails; all first times NaT skips the dimension."""
    for time in sorted(POSSIBLE_TIME_DIMS.intersection(ds_list[0].dims)):
        firsts = np.array([np.asarray(ds[time].values).reshape(-1)[0] for ds in ds_list])
        missing = np.isnat(firsts) if firsts.dtype.kind in "Mm" else np.isnan(firsts)
        if missing.all():
            continue
        if (firsts[1:] < firsts[:-1]).any():
            raise RuntimeError(f"The coordinate {time} is not in ascending order for group {ed_group}, combine cannot "
                               "be used!")


def _null(a):
    a = np.asarray(a)
    if a.dtype.kind in "fc":
        return np.isnan(a)
    if a.dtype.kind in "Mm":
        return np.isnat(a)
    if a.dtype.kind == "O":
        return np.array([x is None or (isinstance(x, float) and x != x) for x in a.reshape(-1)], dtype=bool).reshape(a.shape)
    return np.zeros(a.shape, dtype=bool)


def _same_values(a, b):
    """Equal where both hold a value and null in the same places (``Variable.identical`` on the data)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    na, nb = _null(a), _null(b)
    return bool(np.array_equal(na, nb) and np.all((a == b) | na))


def _check_no_append_vendor_params(ds_list, ed_group, ds_append_dims):
    """Every variable of ``Vendor_specific`` without an append dimension must be identical in all files -- names,
    dimensions, values, attributes (``RuntimeError``): each file is compared with the one in front of it."""
    if ed_group != "Vendor_specific":
        raise ValueError("Group must be `Vendor_specific`!")

    def fixed(ds):
        out = {k: v for k, v in ds.variables.items() if not set(v.dims) & set(ds_append_dims)}
        return out, dict(ds.attrs)

    kept = [fixed(ds) for ds in ds_list]
    for (vars_a, attrs_a), (vars_b, attrs_b) in zip(kept, kept[1:]):
        same = list(vars_a) == list(vars_b) and attrs_a == attrs_b and all(
            vars_a[k].dims == vars_b[k].dims and dict(vars_a[k].attrs) == dict(vars_b[k].attrs)
            and _same_values(vars_a[k].values, vars_b[k].values) for k in vars_a)
        if not same:
            raise RuntimeError(f"Non identical filter parameters in {ed_group} group. Objects cannot be merged!")


def _merge_attributes(attributes):
    """One dict from the files' attribute dicts: keys in the order they first appear, each with the first value that is
    not the empty string (the empty string itself when no file has another)."""
    merged = {}
    for attrs in attributes:
        for key, value in attrs.items():
            have = merged.get(key, "")
            if isinstance(have, str) and have == "":
                merged[key] = value
    return merged


# ---- one group ---------------------------------------------------------------------------------------------------------------
def _promoted(dtype):
    """The dtype that can hold a missing value (xarray's ``dtypes.maybe_promote``, from its documented behaviour)."""
    dtype = np.dtype(dtype)
    if dtype.kind in "fcMm":
        return dtype
    if dtype.kind in "iu":
        return np.dtype(np.float32) if dtype.itemsize <= 2 else np.dtype(np.float64)
    raise NotImplementedError(f"a variable of dtype {dtype} would have to be padded: only numbers and times are")


def _fill_of(dtype):
    return np.array("NaT", dtype=dtype) if dtype.kind in "Mm" else np.array(np.nan, dtype=dtype)


def _select(ds, order):
    """``ds`` with its channels in ``order`` (labels) -- ``ds.sel(channel=order)``; the same object when that is its order."""
    have = _channels(ds)
    if have == list(order):
        return ds
    idx = [have.index(c) for c in order]
    out = Dataset(attrs=dict(ds.attrs))
    for k, c in ds.coords.items():
        out.coords[k] = DataArray(c.values[idx], c.dims, attrs=c.attrs, name=k) if k == "channel" else c
    for k, v in ds.data_vars.items():
        if "channel" not in v.dims:
            out.data_vars[k] = v
            continue
        ax = v.dims.index("channel")
        if isinstance(v.data, DeviceArray):
            import torch

            t = v.data.tensor
            data = DeviceArray(t.index_select(ax, torch.as_tensor(idx, device=t.device)),
                               host=_readonly(np.take(np.asarray(v.data), idx, axis=ax)) if host_readable(v.data) else None)
        else:
            data = np.take(v.values, idx, axis=ax)
        out.data_vars[k] = DataArray(data, v.dims, attrs=v.attrs, name=k)
    return out


def _readonly(a):
    a = a.view()
    a.flags.writeable = False
    return a


def _aligned_host(v, sizes, chan_map, dtype, skip=None):
    """The host values of variable ``v`` brought to the combined sizes of its dimensions (``skip``: the append dimension,
    left as it is): channels in the combined order, ``range_sample`` padded with the fill value of ``dtype``."""
    a = np.asarray(v.values)
    if "channel" in v.dims and chan_map is not None and list(chan_map) != list(range(a.shape[v.dims.index("channel")])):
        a = np.take(a, chan_map, axis=v.dims.index("channel"))
    shape = tuple(a.shape[i] if d == skip else sizes.get(d, a.shape[i]) for i, d in enumerate(v.dims))
    if shape == a.shape:
        return a.astype(dtype, copy=False)
    out = np.full(shape, _fill_of(np.dtype(dtype)), dtype=dtype)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


def _uploadable(dtype):
    """Can a device tensor hold this dtype as it is?  (Times would become their int64 ticks, strings and objects cannot.)"""
    import torch

    if np.dtype(dtype).kind not in "fiucb":
        return False
    try:
        torch.from_numpy(np.empty(0, dtype=dtype))
    except TypeError:
        return False
    return True


def _is_padded(vs, sizes):
    """Does any file's variable fall short of the combined ``range_sample``?  It is the only dimension that is ever
    padded: a channel axis that a selection shortens is picked from, not filled, so integers keep their type."""
    want = sizes.get("range_sample")
    return any(d == "range_sample" and v.shape[i] != want for v in vs for i, d in enumerate(v.dims))


def _resident_rule(group, v):
    return group in RESIDENT_GROUPS and v.ndim >= 2 and np.dtype(v.dtype).kind == "f"


def _concat_variable(group, name, vs, dim, sizes, chan_maps):
    """The variable ``name`` of every file (``vs``) joined along ``dim``."""
    import torch

    from . import ops

    v0 = vs[0]
    for v in vs:
        if v.dims != v0.dims:
            raise ValueError(f"{group}: variable {name} has dimensions {v.dims} in one file and {v0.dims} in another")
    padded = _is_padded(vs, sizes)
    src_dtype = np.result_type(*[np.dtype(v.dtype) for v in vs]) if v0.dtype.kind not in "USO" else None
    out_dtype = (_promoted(src_dtype) if padded else src_dtype) if src_dtype is not None else None
    resident = any(isinstance(v.data, DeviceArray) for v in vs) or _resident_rule(group, v0)
    dims = v0.dims
    has_chan = bool(dims) and dims[0] == "channel"
    maps = chan_maps if has_chan and chan_maps is not None else None
    cube = (has_chan and len(dims) in (3, 4) and dims[1] == dim and dims[2] == "range_sample"
            and (len(dims) == 3 or dims[3] == "beam"))
    served = src_dtype is not None and (src_dtype.kind == "i" or src_dtype in (np.float32, np.float64)
                                        or (src_dtype == np.uint8 and not padded))
    if resident and served and (cube or (has_chan and len(dims) == 2 and dims[1] == dim)):
        want = torch.from_numpy(np.empty(0, dtype=src_dtype)).dtype
        ts = []
        for v in vs:  # file by file: what is on the host goes up as it is, the join and the pad happen in HBM
            t = v.data.tensor.contiguous() if isinstance(v.data, DeviceArray) else ops.to_device(np.asarray(v.data))
            ts.append(t if t.dtype == want else t.to(want))
        if cube:
            out_t = torch.from_numpy(np.empty(0, dtype=out_dtype)).dtype
            return DataArray(DeviceArray(ops.concat_rows(ts, maps, out_dtype=out_t)), dims, attrs=v0.attrs, name=name)
        if maps is not None:
            ts = [t if list(m) == list(range(t.shape[0])) else t.index_select(0, torch.as_tensor(list(m), device=t.device))
                  for t, m in zip(ts, maps)]
        mirror = None
        if all(host_readable(v.data) for v in vs):
            mirror = _readonly(np.concatenate([_aligned_host(v, {}, m, src_dtype, skip=dim)
                                               for v, m in zip(vs, maps or [None] * len(vs))], axis=1))
        return DataArray(DeviceArray(torch.cat(ts, dim=1), host=mirror), dims, attrs=v0.attrs, name=name)
    ax = dims.index(dim)
    parts = [_aligned_host(v, sizes, m if "channel" in dims else None,
                           out_dtype if out_dtype is not None else np.asarray(v.values).dtype, skip=dim)
             for v, m in zip(vs, chan_maps or [None] * len(vs))]
    joined = np.concatenate(parts, axis=ax)
    if resident and _uploadable(joined.dtype):
        # (a layout or type the device join does not serve -- an append dimension that is not the second, no leading
        # channel, float16, bool, complex, unsigned: joined in NumPy, and resident again like its inputs)
        return DataArray(DeviceArray(ops.to_device(joined), host=_readonly(joined)), dims, attrs=v0.attrs, name=name)
    return DataArray(joined, dims, attrs=v0.attrs, name=name)


def _merge_fixed(group, name, vs, sizes, chan_maps):
    """A variable without an append dimension: the files must agree where both hold a value (``no_conflicts``), the first
    value that is not null wins."""
    from . import ops

    v0 = vs[0]
    for v in vs:
        if v.dims != v0.dims:
            raise ValueError(f"{group}: variable {name} has dimensions {v.dims} in one file and {v0.dims} in another")
    padded = _is_padded(vs, sizes)
    if v0.dtype.kind in "USO":
        dtype = None
    else:
        dtype = np.result_type(*[np.dtype(v.dtype) for v in vs])
        dtype = _promoted(dtype) if padded else dtype
    parts = [_aligned_host(v, sizes, m, dtype if dtype is not None else np.asarray(v.values).dtype)
             for v, m in zip(vs, chan_maps or [None] * len(vs))]
    out = parts[0]
    for p in parts[1:]:
        if p.shape != out.shape:
            raise ValueError(f"{group}: variable {name} has shape {p.shape} in one file and {out.shape} in another")
        n_out, n_p = _null(out), _null(p)
        if not np.all((out == p) | n_out | n_p):
            raise ValueError(f"{group}: conflicting values for variable {name} on objects to be combined")
        if (n_out & ~n_p).any():
            out = np.where(n_out, p, out)
    unchanged = out is parts[0] and out is np.asarray(v0.values)
    if isinstance(v0.data, DeviceArray) and unchanged:
        return DataArray(v0.data, v0.dims, attrs=v0.attrs, name=name)
    if (any(isinstance(v.data, DeviceArray) for v in vs) or _resident_rule(group, v0)) and _uploadable(out.dtype):
        return DataArray(DeviceArray(ops.to_device(out), host=_readonly(out)), v0.dims, attrs=v0.attrs, name=name)
    return DataArray(out, v0.dims, attrs=v0.attrs, name=name)


def _combine_group(group, ds_list, selection):
    """One group of every file -> the combined dataset (attributes not yet set)."""
    first = ds_list[0]
    append_dims = set(first.dims).intersection(APPEND_DIMS)
    if len(append_dims) == 0:  # nothing is aligned: the first file's, in its own order unless channels are selected
        return first if selection is None or "channel" not in first.coords else _select(first, selection)
    # the combined channel order and, per file, combined position -> the file's position
    chan_maps, order = None, None
    if "channel" in first.coords:
        lists = [_channels(ds) for ds in ds_list]
        if selection is not None:
            order = list(selection)
        elif all(c == lists[0] for c in lists):
            order = lists[0]
        else:
            order = sorted(set(itertools.chain.from_iterable(lists)))
        chan_maps = [[c.index(x) for x in order] for c in lists]
    # the sizes of the dimensions that are not appended: range_sample is the union, the others must agree
    sizes = {}
    for ds in ds_list:
        for d, n in ds.sizes.items():
            if d in append_dims or d == "channel":
                continue
            if d == "range_sample":
                sizes[d] = max(sizes.get(d, 0), n)
            elif sizes.setdefault(d, n) != n:
                raise NotImplementedError(f"{group}: dimension {d} has {n} entries in one file and {sizes[d]} in another; only "
                                          "range_sample is padded")
    if order is not None:
        sizes["channel"] = len(order)
    out = Dataset()
    for k, c in first.coords.items():
        if k in append_dims:
            parts = [np.asarray(ds.coords[k].values) for ds in ds_list]
            out.coords[k] = DataArray(np.concatenate(parts), (k,), attrs=c.attrs, name=k)
        elif k == "channel":
            out.coords[k] = DataArray(np.asarray(c.values)[chan_maps[0]], (k,), attrs=c.attrs, name=k)
        elif k == "range_sample":
            longest = max((ds.coords[k].values for ds in ds_list if k in ds.coords), key=len)
            for ds in ds_list:
                if k in ds.coords and not np.array_equal(ds.coords[k].values, longest[:len(ds.coords[k].values)]):
                    raise NotImplementedError(f"{group}: the range_sample coordinates are not prefixes of the longest one")
            out.coords[k] = DataArray(np.asarray(longest), (k,), attrs=c.attrs, name=k)
        else:
            for ds in ds_list[1:]:
                if k not in ds.coords or not _same_values(ds.coords[k].values, c.values):
                    raise NotImplementedError(f"{group}: the coordinate {k} differs between the files; only channel and "
                                              "range_sample are aligned")
            out.coords[k] = c
    for name, v0 in first.data_vars.items():
        for ds in ds_list:
            if name not in ds.data_vars:
                raise ValueError(f"{group}: variable {name} is not found in all EchoData objects being combined")
        vs = [ds.data_vars[name] for ds in ds_list]
        mine = append_dims.intersection(v0.dims)
        if len(mine) > 1:
            continue  # (dropped by the reference's drop_dims in every pass)
        if len(mine) == 1:
            out.data_vars[name] = _concat_variable(group, name, vs, next(iter(mine)), sizes, chan_maps)
        else:
            out.data_vars[name] = _merge_fixed(group, name, vs, sizes, chan_maps if "channel" in v0.dims else None)
    return out


def _make_ping_time_resident(ds):
    """The combined ``ping_time`` goes up once; the verdict on it (sorted, no NaT) is the device's own."""
    from . import _lib, ops

    if "ping_time" not in ds.coords:
        return
    c = ds.coords["ping_time"]
    pt = c.values
    if not isinstance(pt, np.ndarray) or pt.dtype != np.dtype("datetime64[ns]") or pt.size == 0:
        return
    pt = np.ascontiguousarray(pt)
    t = ops.to_device(pt)
    facts, _ = ops.time_reversals(t)
    facts = facts.tolist()
    pt.flags.writeable = False
    ops.register_ping_time(pt, t, facts[_lib.QC_COUNT] == 0 and facts[_lib.QC_NAT] == 0)
    ds.coords["ping_time"] = DataArray(pt, ("ping_time",), attrs=c.attrs, name="ping_time")


def _is_scalar_attr(v):
    return isinstance(v, (str, bytes, bool, int, float, np.generic)) or v is None


def _capture_prov_attrs(attrs_dict, echodata_filenames):
    """Every scalar group attribute of every file as a string variable over ``echodata_filename`` carrying the attribute
    ``echodata_group``; a file without the attribute holds "" (combine.py:605-644)."""
    out = {}
    n = len(echodata_filenames)
    for group, attributes in attrs_dict.items():
        keys = list(dict.fromkeys(k for a in attributes for k, v in a.items() if _is_scalar_attr(v)))
        for k in keys:
            vals = [a.get(k) if _is_scalar_attr(a.get(k)) else None for a in attributes]
            if k in out:  # the same attribute name in two groups: merged, no_conflicts
                old = out[k][0]
                for i in range(n):
                    if old[i] is None:
                        old[i] = vals[i]
                    elif vals[i] is not None and str(vals[i]) != str(old[i]):
                        raise ValueError(f"conflicting values for the attribute {k} of two groups in file "
                                         f"{echodata_filenames[i]}")
            else:
                out[k] = (vals, group)
    return {k: DataArray(np.array(["" if x is None else str(x) for x in vals], dtype=str), (ED_FILENAME,),
                         attrs={ED_GROUP: group}, name=k) for k, (vals, group) in out.items()}


def _combine(sonar_model, eds, echodata_filenames, ed_group_chan_sel):
    group_order = []  # every group path of any file, in the order of first appearance
    for ed in eds:
        group_order += [path for path in ed.group_paths if path not in group_order]
    for ed in eds:
        if "Provenance" in ed and ed["Provenance"].attrs.get("is_combined", False):
            raise NotImplementedError("An input that is itself a combined EchoData object cannot be combined again")
    attrs_dict, tree = {}, {}
    for ed_group in group_order:
        missing = [i for i, ed in enumerate(eds) if ed_group not in ed]
        if missing:
            raise ValueError(f"The EchoData group {ed_group} is not found in all EchoData objects being combined "
                             f"(missing from {[echodata_filenames[i] for i in missing]})")
        ds_list = [ed[ed_group] for ed in eds]
        # (a selection is not applied to the files: it becomes the channel maps of the join, so that a resident cube is
        # read once, by the kernel that writes the combined one)
        selection = ed_group_chan_sel.get(ed_group)
        ds_attrs = [dict(ds.attrs) for ds in ds_list]
        attrs_dict[ed_group] = ds_attrs
        _check_ascending_ds_times(ds_list, ed_group)
        if ed_group == "Vendor_specific":
            vendor = ds_list
            if selection is not None and "channel" in ds_list[0].coords:
                vendor = [_select(ds, selection) for ds in ds_list]
            elif "channel" in ds_list[0].coords and any(_channels(ds) != _channels(ds_list[0]) for ds in ds_list):
                # (a deviation: compared channel by channel LABEL, where the reference's Dataset.identical refuses files
                # whose channels come in another order)
                vendor = [_select(ds, sorted(_channels(ds_list[0]))) for ds in ds_list]
            _check_no_append_vendor_params(vendor, ed_group, set(ds_list[0].dims).intersection(APPEND_DIMS))
        combined = _combine_group(ed_group, ds_list, selection).copy()
        group_attrs = _merge_attributes(ds_attrs)
        combined.attrs = group_attrs
        if ed_group in (BEAM1, BEAM2):
            _make_ping_time_resident(combined)
        tree[ed_group] = combined
    prov = tree.get("Provenance")
    if prov is None:
        prov = Dataset(coords={FILENAMES: np.arange(len(eds))})
        prov["source_filenames"] = ((FILENAMES,), np.array([str(_source_name(ed)) for ed in eds], dtype=str))
        attrs_dict["Provenance"] = [{} for _ in eds]
    prov.attrs["is_combined"] = True  # (the conversion_* attributes are the merged ones already)
    prov.attrs.update(echopype_prov_attrs(process_type="combination"))
    prov.coords[ED_FILENAME] = DataArray(np.array(echodata_filenames, dtype=str), (ED_FILENAME,), name=ED_FILENAME)
    for k, da in _capture_prov_attrs(attrs_dict, echodata_filenames).items():
        prov.data_vars[k] = da
    if FILENAMES in prov.coords:
        c = prov.coords[FILENAMES]
        prov.coords[FILENAMES] = DataArray(np.arange(*c.shape), (FILENAMES,), attrs=c.attrs, name=FILENAMES)
    tree["Provenance"] = prov
    return tree


def combine_echodata(echodata_list=None, channel_selection=None):
    """Combines multiple ``EchoData`` objects into a single ``EchoData`` object (the reference's signature,
    combine.py:860-976).

    ``echodata_list``: the ``EchoData`` objects, in time order.  ``channel_selection``: None, a list of channel names to
    keep in every group with a ``channel`` dimension, or a dict of beam group path -> list of names (the other groups
    then take the union).  Raises as the reference does: ``ValueError`` (sonar models, file names), ``TypeError`` (the
    form of ``channel_selection``), ``RuntimeError`` (channels that differ or repeat, first times that descend, filter
    parameters that differ), ``NotImplementedError`` (selected channels that some file lacks).  See the module docstring
    for what is concatenated how, where the result lives, and the deviations."""
    if echodata_list is None:
        warn("No EchoData objects were provided, returning an empty EchoData object.")
        return EchoData(None)
    sonar_model, echodata_filenames = check_eds(echodata_list)
    _check_channel_selection_form(channel_selection)
    ed_group_chan_sel = _check_echodata_channels(echodata_list, channel_selection)
    tree = _combine(sonar_model, echodata_list, echodata_filenames, ed_group_chan_sel)
    return EchoData(sonar_model, tree)


__all__ = ["combine_echodata"]
