"""NumPy restatement of ``combine_echodata`` (echopype echodata/combine.py: ``_combine`` and what it calls), on plain
dicts, written for the tests: slow, short, and independent of the package's code.

A *file* is ``dict(sonar_model=, source_file=, groups={path: group})``; a *group* is
``dict(coords={name: 1-D array}, vars={name: (dims, array, attrs)}, attrs={})``.  ``combine(files, channel_selection)``
returns the combined groups in the same form.

What is restated, per group: append dimensions are ``filenames`` and the seven time dimensions; a group without one is
the first file's (with the channel selection applied); a variable with exactly one append dimension is concatenated along
it, one with several is dropped, one without must agree where both files hold a value (``compat="no_conflicts"``) and the
first non-null value wins; ``range_sample`` is ``arange(max S_i)``, shorter files NaN-padded; variable attributes are the
first file's, group attributes the first non-empty value of every key.

Two rules are xarray's.  xarray is not installed where this was written, so they are stated here from its DOCUMENTED
behaviour and have not been executed against it:

* channel order: with a selection, the sorted selection; otherwise the first file's order if all files have the same
  order, else the sorted union (``join="outer"`` of unequal indexes returns a sorted union);
* dtype after a pad (``xarray.core.dtypes.maybe_promote``): floats, complex, datetime64 and timedelta64 keep their type
  (NaN / NaT fill), integers of at most 2 bytes become float32, wider integers float64; a variable none of whose files
  is padded keeps its type.

The reference's ``_combine`` itself cannot be executed here: it needs ``xr.concat`` with an outer join, which the stand-in
of the tests does not have."""
import itertools
from pathlib import Path

import numpy as np

TIME_DIMS = ("time1", "time2", "time3", "time4", "nmea_time", "ping_time", "filter_time")
APPEND = ("filenames",) + TIME_DIMS
EK80_LIKE = ("EK80", "ES80", "EA640")


# ---- the kernel's job -------------------------------------------------------------------------------------------------------
def promoted(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind in "iu":
        return np.dtype(np.float32 if dtype.itemsize <= 2 else np.float64)
    return dtype


def concat_rows(arrs, chan_maps=None, out_dtype=None):
    """(C_i, P_i, S_i[, B]) arrays -> (C, sum P_i, max S_i[, B]); ``chan_maps[i][c]`` = source channel of output channel c.
    Same-type joins move bytes (NaN payloads survive); a pad is NumPy's ``np.nan`` of the output type."""
    S = max(a.shape[2] for a in arrs)
    padded = any(a.shape[2] < S for a in arrs)
    src = arrs[0].dtype
    if out_dtype is None:
        out_dtype = promoted(src) if padded else src
    out_dtype = np.dtype(out_dtype)
    maps = chan_maps if chan_maps is not None else [list(range(a.shape[0])) for a in arrs]
    C = len(maps[0])
    P = sum(a.shape[1] for a in arrs)
    out = np.full((C, P, S) + arrs[0].shape[3:], np.nan if out_dtype.kind == "f" else 0, dtype=out_dtype)
    p0 = 0
    for a, m in zip(arrs, maps):
        part = a[list(m)]
        if out_dtype == src:  # bytes, not values: a signalling NaN stays what it is
            out.view(f"u{out_dtype.itemsize}")[:, p0:p0 + a.shape[1], :a.shape[2]] = part.view(f"u{src.itemsize}")
        else:
            out[:, p0:p0 + a.shape[1], :a.shape[2]] = part.astype(out_dtype)
        p0 += a.shape[1]
    return out


# ---- the checks (restated; the package's own are held to the reference's executed results) ------------------------------
def file_names(files):
    names = []
    for f in files:
        path = f.get("source_file") or f.get("converted_raw_path")
        name = Path(path).name if path is not None else "internal-memory"
        if path is not None and name in names:
            raise ValueError("EchoData objects have conflicting filenames")
        names.append(name)
    return names


def selection_dict(sonar_model, has_chan, sel):
    if sel is None:
        return {g: None for g in has_chan}
    union = sorted(sel) if isinstance(sel, list) else sorted(set(itertools.chain.from_iterable(sel.values())))
    out = {}
    for g, has in has_chan.items():
        if not has:
            out[g] = None
        elif isinstance(sel, dict) and sonar_model in EK80_LIKE and g not in ("Sonar", "Platform", "Vendor_specific"):
            out[g] = sorted(sel[g])
        else:
            out[g] = union
    return out


def merge_attributes(attrs):
    out = {}
    for a in attrs:
        for k, v in a.items():
            if k not in out or (isinstance(out[k], str) and out[k] == ""):
                out[k] = v
    return out


# ---- one group -----------------------------------------------------------------------------------------------------------------
def _isnull(a):
    if a.dtype.kind in "fc":
        return np.isnan(a)
    if a.dtype.kind in "Mm":
        return np.isnat(a)
    return np.zeros(a.shape, bool)


def _align(dims, a, positions, S, dtype, keep):
    """channels picked by position, range_sample padded to S with the missing value of ``dtype``; the dimension ``keep``
    is left alone."""
    a = np.asarray(a)
    if "channel" in dims and positions is not None:
        a = np.take(a, positions, axis=dims.index("channel"))
    a = a.astype(dtype) if dtype is not None else a
    if "range_sample" in dims and keep != "range_sample":
        ax = dims.index("range_sample")
        if a.shape[ax] < S:
            shape = list(a.shape)
            shape[ax] = S - a.shape[ax]
            fill = np.full(shape, np.datetime64("NaT") if a.dtype.kind == "M" else np.timedelta64("NaT") if a.dtype.kind == "m"
                           else np.nan, dtype=a.dtype)
            a = np.concatenate([a, fill], axis=ax)
    return a


def combine_group(group_list, selection=None):
    first = group_list[0]
    dims_of_first = set(first["coords"]) | {d for dims, _, _ in first["vars"].values() for d in dims}
    append = [d for d in APPEND if d in dims_of_first]
    order = positions = None
    if "channel" in first["coords"]:
        lists = [[str(c) for c in g["coords"]["channel"]] for g in group_list]
        if selection is not None:
            order = sorted(selection)
        elif all(c == lists[0] for c in lists):
            order = lists[0]
        else:
            order = sorted(set(itertools.chain.from_iterable(lists)))
        positions = [[c.index(x) for x in order] for c in lists]
    if not append:
        out = dict(coords=dict(first["coords"]), vars={}, attrs={})
        pick = positions[0] if selection is not None and order is not None else None  # (no alignment: the first file's order)
        if pick is not None:
            out["coords"]["channel"] = np.asarray(first["coords"]["channel"])[pick]
        for name, (dims, a, attrs) in first["vars"].items():
            out["vars"][name] = (dims, _align(dims, a, pick, 0, None, "range_sample"), dict(attrs))
        return out
    S = 0
    for g in group_list:
        if "range_sample" in g["coords"]:
            S = max(S, len(g["coords"]["range_sample"]))
        for dims, a, _ in g["vars"].values():
            if "range_sample" in dims:
                S = max(S, np.shape(a)[dims.index("range_sample")])
    out = dict(coords={}, vars={}, attrs={})
    for k, c in first["coords"].items():
        if k in append:
            out["coords"][k] = np.concatenate([np.asarray(g["coords"][k]) for g in group_list])
        elif k == "channel":
            out["coords"][k] = np.asarray(c)[positions[0]]
        elif k == "range_sample":
            out["coords"][k] = np.arange(S)
        else:
            for g in group_list[1:]:
                if not np.array_equal(np.asarray(g["coords"][k]), np.asarray(c)):
                    raise NotImplementedError(k)
            out["coords"][k] = np.asarray(c)
    for name, (dims, a0, attrs) in first["vars"].items():
        mine = [d for d in dims if d in append]
        if len(mine) > 1:
            continue
        arrs = [np.asarray(g["vars"][name][1]) for g in group_list]
        padded = "range_sample" in dims and any(a.shape[dims.index("range_sample")] < S for a in arrs)
        dtype = None
        if arrs[0].dtype.kind not in "USO":
            dtype = np.result_type(*[a.dtype for a in arrs])
            dtype = promoted(dtype) if padded else dtype
        parts = [_align(dims, a, p, S, dtype, mine[0] if mine else None)
                 for a, p in zip(arrs, positions or [None] * len(arrs))]
        if mine:
            val = np.concatenate(parts, axis=dims.index(mine[0]))
        else:
            val = parts[0]
            for p in parts[1:]:
                n_val, n_p = _isnull(val), _isnull(p)
                if not np.all((val == p) | n_val | n_p):
                    raise ValueError(f"conflicting values for variable {name}")
                val = np.where(n_val & ~n_p, p, val)
        out["vars"][name] = (dims, val, dict(attrs))
    return out


def combine(files, channel_selection=None, now=None):
    """-> (groups, file names).  The ``combination_time`` attribute of Provenance is whatever ``now`` says (None: absent;
    the comparison leaves it out)."""
    if len({f["sonar_model"] for f in files}) != 1:
        raise ValueError("all EchoData objects must have the same sonar_model value")
    names = file_names(files)
    paths = list(dict.fromkeys(itertools.chain.from_iterable(f["groups"] for f in files)))
    for f in files:
        if f["groups"].get("Provenance", {}).get("attrs", {}).get("is_combined"):
            raise NotImplementedError("combined input")
    g0 = files[0]["groups"]
    has_chan = {p: "channel" in g0[p]["coords"] for p in g0}
    sel = selection_dict(files[0]["sonar_model"], has_chan, channel_selection)
    out, attrs_dict = {}, {}
    for p in paths:
        if any(p not in f["groups"] for f in files):
            raise ValueError(f"group {p} is missing from a file")
        gl = [f["groups"][p] for f in files]
        if "channel" in gl[0]["coords"]:
            lists = [[str(c) for c in g["coords"]["channel"]] for g in gl]
            if any(len(set(c)) != len(c) for c in lists):
                raise RuntimeError("repeating channels")
            if sel.get(p) is None:
                if any(sorted(c) != sorted(lists[0]) for c in lists):
                    raise RuntimeError("channels differ")
            elif any(not set(sel[p]) <= set(c) for c in lists):
                raise NotImplementedError("selected channels missing")
            if sel.get(p) is not None:  # the selection comes first: what is compared and joined is the selected part
                gl = [combine_group([g], sel[p]) | {"attrs": g["attrs"]} for g in gl]
        for t in TIME_DIMS:
            if t in gl[0]["coords"]:
                firsts = np.array([np.asarray(g["coords"][t])[0] for g in gl])
                if not np.isnat(firsts).all() and (np.diff(firsts) < np.timedelta64(0, "ns")).any():
                    raise RuntimeError(f"The coordinate {t} is not in ascending order")
        if p == "Vendor_specific":
            vl = gl
            if "channel" in gl[0]["coords"]:  # compared channel by channel LABEL (a deviation: see the package's docstring)
                lists = [[str(c) for c in g["coords"]["channel"]] for g in gl]
                common = lists[0] if all(c == lists[0] for c in lists) else sorted(lists[0])
                vl = [combine_group([g], common) for g in gl]
            for g in vl[1:]:
                fixed = lambda grp: {k: v for k, v in grp["vars"].items() if not set(v[0]) & set(APPEND)}  # noqa: E731
                a, b = fixed(vl[0]), fixed(g)
                same = list(a) == list(b) and all(
                    a[k][0] == b[k][0] and np.shape(a[k][1]) == np.shape(b[k][1])
                    and np.array_equal(_isnull(np.asarray(a[k][1])), _isnull(np.asarray(b[k][1])))
                    and np.all((np.asarray(a[k][1]) == np.asarray(b[k][1])) | _isnull(np.asarray(a[k][1]))) for k in a)
                if not same:
                    raise RuntimeError("Non identical filter parameters")
        comb = combine_group(gl, sel.get(p))
        attrs_dict[p] = [dict(g["attrs"]) for g in gl]
        comb["attrs"] = merge_attributes(attrs_dict[p])
        out[p] = comb
    if "Provenance" not in out:
        out["Provenance"] = dict(coords={"filenames": np.arange(len(files))},
                                 vars={"source_filenames": (("filenames",), np.array([str(f["source_file"]) for f in files]), {})},
                                 attrs={})
        attrs_dict["Provenance"] = [{} for _ in files]
    prov = out["Provenance"]
    prov["attrs"]["is_combined"] = True
    prov["coords"]["echodata_filename"] = np.array(names, dtype=str)
    captured = {}  # attribute name -> [values per file (None: the file has none), the first group that has it]
    for p, attrs in attrs_dict.items():
        for k in dict.fromkeys(k for a in attrs for k, v in a.items() if v is not None and np.ndim(v) == 0 and not isinstance(v, (list, tuple, dict))):
            vals = [a[k] if k in a and a[k] is not None and np.ndim(a[k]) == 0 else None for a in attrs]
            if k not in captured:
                captured[k] = [vals, p]
            else:  # the same name in a later group: xr.merge, no_conflicts
                have = captured[k][0]
                for i, v in enumerate(vals):
                    if have[i] is None:
                        have[i] = v
                    elif v is not None and str(v) != str(have[i]):
                        raise ValueError(f"conflicting values for attribute {k}")
    for k, (vals, p) in captured.items():
        prov["vars"][k] = (("echodata_filename",), np.array(["" if v is None else str(v) for v in vals], dtype=str),
                           {"echodata_group": p})
    if "filenames" in prov["coords"]:
        prov["coords"]["filenames"] = np.arange(len(prov["coords"]["filenames"]))
    return out, names


# ---- EchoData <-> the plain form ---------------------------------------------------------------------------------------------
def from_echodata(ed):
    """The package's EchoData (host or resident) as a *file*."""
    groups = {}
    for p in ed.group_paths:
        ds = ed[p]
        groups[p] = dict(coords={k: np.asarray(c.values) for k, c in ds.coords.items()},
                         vars={k: (tuple(v.dims), np.asarray(v.values), dict(v.attrs)) for k, v in ds.data_vars.items()},
                         attrs=dict(ds.attrs))
    return dict(sonar_model=ed.sonar_model, source_file=ed.source_file, converted_raw_path=ed.converted_raw_path,
                groups=groups)


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind in "US" or b.dtype.kind in "US":
        return a.shape == b.shape and bool(np.all(a.astype(str) == b.astype(str)))
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


VOLATILE = ("combination_time",)


def assert_equal(ed, want, what=""):
    """The combined EchoData ``ed`` against the restated groups ``want``: group paths, coordinates, variables (order, dims,
    dtypes, bytes, attributes) and group attributes (the time stamp and software name of the combination aside)."""
    assert list(ed.group_paths) == list(want), (what, list(ed.group_paths), list(want))
    for p, g in want.items():
        ds = ed[p]
        assert list(ds.coords) == list(g["coords"]), (what, p, list(ds.coords), list(g["coords"]))
        for k, c in g["coords"].items():
            assert same_bytes(ds.coords[k].values, c), (what, p, k, ds.coords[k].values.dtype, np.asarray(c).dtype)
        assert list(ds.data_vars) == list(g["vars"]), (what, p, list(ds.data_vars), list(g["vars"]))
        for k, (dims, a, attrs) in g["vars"].items():
            v = ds.data_vars[k]
            assert tuple(v.dims) == tuple(dims), (what, p, k, v.dims, dims)
            assert np.dtype(v.dtype) == np.asarray(a).dtype or np.asarray(a).dtype.kind in "US", (what, p, k, v.dtype, a.dtype)
            assert same_bytes(v.values, a), (what, p, k)
            assert dict(v.attrs) == attrs, (what, p, k, dict(v.attrs), attrs)
        got = {k: v for k, v in ds.attrs.items() if not k.startswith("combination_")}
        assert got == g["attrs"], (what, p, got, g["attrs"])
