#!/usr/bin/env python3
"""Generate tests/golden/ref_location_goldens.npz and tests/golden/ref_location_signatures.json by EXECUTING THE
REFERENCE'S OWN utils/align.py, consolidate/loc_utils.py and consolidate/api.py::add_location over oracle/xr_shim.py.
Authoring machine only: needs the reference checkout.

The reference's modules are loaded as they are; what consolidate/api.py imports beside them (file opening, the EchoData
class, the calibration and split-beam modules, the processing-level decorator) is stood in for by empty modules, an
identity ``open_source`` and an identity decorator -- none of it takes part in add_location's arithmetic.  The shim's
``interp`` runs scipy's interp1d for ``method="linear"``; added here at run time (oracle/ is not edited): the same call
with ``kind="nearest"``, ``Dataset.get`` and ``Dataset.drop_vars``.

Stored, data only: the seeded inputs of tests/location_cases.py, what ``align_to_ping_time`` returned for them with both
methods, what ``add_location`` returned (latitude, longitude, the ``history`` attribute without its time stamp) or the
type and message of what it raised, the warnings it logged, and, in the JSON, the two signatures (read with ast).
Written with fixed zip timestamps: two runs give the same bytes."""
import ast
import io
import json
import logging
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_ref_signatures  # noqa: E402
import xr_shim  # noqa: E402
from gen_goldens import REF, _load  # noqa: E402

import location_cases as C  # noqa: E402
import location_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_location_goldens.npz")
OUT_SIG = os.path.join(ROOT, "tests", "golden", "ref_location_signatures.json")
DA, DS = xr_shim.DataArray, xr_shim.Dataset


def _extend_shim():
    linear = DA.interp

    def interp(self, coords=None, method="linear", kwargs=None, **kw):
        if method == "linear":
            return linear(self, coords, method, kwargs, **kw)
        from scipy.interpolate import interp1d

        assert method == "nearest" and self.ndim == 1
        (dim, new), = {**(coords or {}), **kw}.items()
        newv = np.asarray(new.data)
        x = np.asarray(self.coords[dim])
        x0 = x.min()  # datetimes: nanoseconds from the smallest label, as in the shim's linear branch
        xf = (x - x0).astype("timedelta64[ns]").astype(np.float64)
        qf = (newv.astype(x.dtype) - x0).astype("timedelta64[ns]").astype(np.float64)
        f = interp1d(xf, self.data.astype(np.float64), kind="nearest", axis=0, bounds_error=False, copy=False,
                     assume_sorted=False, **(kwargs or {}))
        return DA(f(qf), {new.dims[0]: newv, dim: newv}, (new.dims[0],), self.name, self.attrs)

    def get(self, name, default=None):
        return self[name] if name in self else default

    def drop_vars(self, names):
        names = [names] if isinstance(names, str) else list(names)
        out = DS(coords={k: v for k, v in self.coords.items() if k not in names}, attrs=self.attrs)
        for k, v in self.data_vars.items():
            if k not in names:
                out[k] = v
        return out

    DA.interp, DS.get, DS.drop_vars = interp, get, drop_vars


def load_reference():
    _extend_shim()
    xr = types.ModuleType("xarray")
    xr.DataArray, xr.Dataset = DA, DS
    sys.modules["xarray"] = xr

    def module(name, path=None, **members):
        m = types.ModuleType(name)
        if path:
            m.__path__ = [path]
        m.__dict__.update(members)
        sys.modules[name] = m
        return m

    module("echopype", REF)
    module("echopype.utils", f"{REF}/utils")
    module("echopype.consolidate", f"{REF}/consolidate")
    module("echopype.calibrate", f"{REF}/calibrate")
    module("echopype.calibrate.ek80_complex", get_filter_coeff=None)
    module("echopype.echodata", f"{REF}/echodata", EchoData=object)
    module("echopype.echodata.simrad", retrieve_correct_beam_group=None)
    module("echopype.utils.io", get_file_format=None, open_source=lambda obj, kind, opts: obj)
    module("echopype.utils.log", _init_logger=logging.getLogger)
    module("echopype.utils.prov", add_processing_level=lambda level: (lambda fn: fn))
    module("echopype.consolidate.ek_depth_utils", ek_use_beam_angles=None, ek_use_platform_angles=None,
           ek_use_platform_vertical_offsets=None)
    module("echopype.consolidate.split_beam_angle", get_angle_complex_samples=None, get_angle_power_samples=None)
    align = _load("echopype.utils.align", f"{REF}/utils/align.py")
    _load("echopype.consolidate.loc_utils", f"{REF}/consolidate/loc_utils.py")
    api = _load("echopype.consolidate.api", f"{REF}/consolidate/api.py")
    return align, api


class _EchoData:
    def __init__(self, sonar_model, platform):
        self.sonar_model, self._platform = sonar_model, platform

    def __getitem__(self, group):
        assert group == "Platform", group
        return self._platform


def _platform(spec):
    ds = DS()
    for name, (dim, t, v) in spec.items():
        ds[name] = DA(v, {dim: t}, [dim], name, {"long_name": name})
    return ds


class _Catch(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append([record.levelname, record.getMessage()])


def main():
    align, api = load_reference()
    g, align_recs, loc_recs = {}, [], []

    for name in C.ALIGN_CASES:
        if name in C.NOT_IN_GOLDENS:
            continue
        c = C.align_case(name)
        pt = DA(c["ping_time"], {"ping_time": c["ping_time"]}, ["ping_time"], "ping_time")
        for k, a in c.items():
            g[f"align/{name}/in/{k}"] = a
        for method in C.METHODS:
            rows = []
            for v in range(c["y"].shape[0]):
                da = DA(c["y"][v], {"time1": c["t_ext"]}, ["time1"], "latitude", {"units": "degrees"})
                with np.errstate(all="ignore"):
                    out = align.align_to_ping_time(da, "time1", pt, method)
                assert out.dims == ("ping_time",) and "time1" not in out.coords and out.attrs == da.attrs, name
                rows.append(np.asarray(out.data, dtype=np.float64))
            g[f"align/{name}/{method}"] = np.stack(rows)
        align_recs.append({"name": name, **{k: (list(v) if isinstance(v, tuple) else v)
                                            for k, v in C.ALIGN_CASES[name].items()}})

    catch = _Catch()
    logging.getLogger("echopype.consolidate.loc_utils").addHandler(catch)
    for name in C.LOCATION_CASES:
        c = C.location_case(name)
        ed = _EchoData(c["model"], _platform(c["platform"]))
        pt = c["ping_time"]
        ds = DS(coords={"ping_time": pt})
        ds["Sv"] = DA(np.zeros((len(pt), 2)), None, ["ping_time", "range_sample"], "Sv")
        catch.messages = []
        rec = {"name": name, "model": c["model"], "datagram_type": c["datagram_type"], "nmea_sentence": c["nmea_sentence"],
               "variables": sorted(c["platform"])}
        try:
            with np.errstate(all="ignore"):
                out = api.add_location(ds, ed, datagram_type=c["datagram_type"], nmea_sentence=c["nmea_sentence"])
        except ValueError as e:
            rec["raised"] = ["ValueError", str(e)]
        if name in C.ORDER_UNDEFINED:
            # the list in the message comes from a set: equal to the restatement's up to its order, nothing is stored
            with np.testing.assert_raises(ValueError) as r:
                R.add_location(pt, c["platform"], c["model"], c["datagram_type"], c["nmea_sentence"])
            head, ours = str(r.exception).split("[")
            head_ref, theirs = rec["raised"][1].split("[")
            assert head == head_ref and sorted(ours.split(", ")) != [] and \
                sorted(s.strip("].") for s in ours.split(", ")) == sorted(s.strip("].") for s in theirs.split(", ")), name
            continue
        rec["logged"] = catch.messages
        for k, (dim, t, v) in c["platform"].items():
            g[f"location/{name}/in/{k}"] = v
            g[f"location/{name}/in/{k}/time"] = t
        g[f"location/{name}/in/ping_time"] = pt
        if "raised" not in rec:
            assert "latitude" not in ds and not any(d in out for d in ("time1", "time3", "time4")), name
            for v in ("latitude", "longitude"):
                assert out[v].dims == ("ping_time",), name
                g[f"location/{name}/{v}"] = np.asarray(out[v].data, dtype=np.float64)
            stamp, _, rest = out["latitude"].attrs["history"].partition(". ")
            assert out["longitude"].attrs["history"] == out["latitude"].attrs["history"]
            rec["history"] = rest  # (the time stamp in front of it changes from run to run)
            rec["attrs"] = sorted(out["latitude"].attrs)
        loc_recs.append(rec)

    g["align_cases"] = np.array(json.dumps(align_recs, sort_keys=True))
    g["location_cases"] = np.array(json.dumps(loc_recs, sort_keys=True))
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(g):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(g[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, b.getvalue())
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes,", len(align_recs), "align cases,", len(loc_recs), "add_location cases")
    for r in loc_recs:
        print(" ", r["name"], r.get("raised") or r.get("logged") or "ok")

    sigs = {}
    for qual, rel, fname in (("consolidate.add_location", "consolidate/api.py", "add_location"),
                             ("utils.align_to_ping_time", "utils/align.py", "align_to_ping_time")):
        tree = ast.parse(open(os.path.join(REF, rel)).read())
        fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == fname)
        sigs[qual] = {"params": gen_ref_signatures.params(fn), "line": fn.lineno, "file": rel}
    with open(OUT_SIG, "w") as f:
        json.dump(sigs, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT_SIG, len(sigs), "signatures")


if __name__ == "__main__":
    main()
