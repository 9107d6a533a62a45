#!/usr/bin/env python3
"""Generate tests/golden/ref_metrics_goldens.npz and tests/golden/ref_metrics_signatures.json by EXECUTING THE REFERENCE'S
OWN metrics/summary_statistics.py over oracle/xr_shim.py.  Authoring machine only: needs the reference checkout.

The reference's module is loaded as it is.  The shim has ``diff``, ``where`` and the inner join of operands whose
``range_sample`` labels differ in number; what it lacks is ``sum``, added here at run time (oracle/ is not edited):
xarray's ``sum`` skips NaN for float data and has no ``min_count`` -- ``np.nansum`` for floats, ``np.sum`` otherwise.

Stored, data only: seeded inputs (float32 values; the float64 runs take the same values upcast), what the seven
functions returned for them in float64 and in float32 (or the type and message of what they raised), the five known
answers of the reference's own tests/metrics/test_metrics_summary_statistics.py (inputs, expected values, rtol, read
from that file with ast) and, in the JSON, the seven signatures (read with ast, as oracle/gen_ref_signatures.py does).
Written with fixed zip timestamps: two runs give the same bytes."""
import ast
import io
import json
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

import metrics_cases as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_metrics_goldens.npz")
OUT_SIG = os.path.join(ROOT, "tests", "golden", "ref_metrics_signatures.json")
REL = "metrics/summary_statistics.py"
REF_TEST = os.path.join(os.path.dirname(REF), "echopype", "tests", "metrics", "test_metrics_summary_statistics.py")
DA, DS = xr_shim.DataArray, xr_shim.Dataset
SEVEN = ("delta_z", "convert_to_linear", "abundance", "center_of_mass", "dispersion", "evenness", "aggregation")
STATS = SEVEN[2:]
SHAPE = (2, 5)


def load_reference():
    xr = types.ModuleType("xarray")
    xr.DataArray, xr.Dataset = DA, DS
    sys.modules["xarray"] = xr

    def _sum(self, dim=None, **kw):
        assert not kw, kw  # the reference passes dim only: skipna by dtype, no min_count
        return self._reduce(np.nansum if self.data.dtype.kind == "f" else np.sum, dim)

    DA.sum = _sum
    return _load("ref_metrics_summary_statistics", f"{REF}/{REL}")


def dataset(arrays, dims):
    """``arrays`` have range_sample last; the dataset's variables have their dimensions in the order ``dims``."""
    canon = [d for d in dims if d != "range_sample"] + ["range_sample"]
    perm = [canon.index(d) for d in dims]
    ds = DS(coords={d: np.arange(arrays["Sv"].shape[canon.index(d)]) for d in dims})
    for name, a in arrays.items():
        ds[name] = (dims, np.ascontiguousarray(np.transpose(a, perm))) if a.ndim == len(dims) else (("range_sample",), a)
    return ds


def known_answers():
    """The inputs and expected values of the reference's five tests, read from their source."""
    tree = ast.parse(open(REF_TEST).read())
    out = {}
    for fn in tree.body:
        if not (isinstance(fn, ast.FunctionDef) and fn.name.startswith("test_")):
            continue
        vals, called, rtol = {}, None, None
        for node in ast.walk(fn):
            if isinstance(node, ast.Assign) and isinstance(node.value, ast.Call) and \
                    ast.unparse(node.value.func) == "np.array":
                vals[node.targets[0].id] = ast.literal_eval(node.value.args[0])
            if isinstance(node, ast.Call) and ast.unparse(node.func) == "np.allclose":
                called = node.args[0].func.id
                rtol = next(ast.literal_eval(k.value) for k in node.keywords if k.arg == "rtol")
        sol = next(v for k, v in vals.items() if k.endswith("_SOL"))
        out[called] = {"Sv": vals["Sv"], "echo_range": vals["echo_range"], "expected": sol, "rtol": rtol}
    assert sorted(out) == sorted(STATS), sorted(out)
    return out


def main():
    ref = load_reference()
    g, cases = {}, []

    def case(tag, kind, S, dims=("channel", "ping_time", "range_sample"), label="echo_range", with_echo_range=True):
        sv, r = C.make(kind, SHAPE, S)
        inputs = {"Sv": sv}
        if with_echo_range:
            inputs["echo_range"] = r
        if label == "depth":
            inputs[label] = (r * np.float32(0.875) + np.float32(5.0)).astype(np.float32)
        for k, a in inputs.items():
            g[f"{tag}/in/{k}"] = a
        rec = {"tag": tag, "kind": kind, "S": S, "dims": list(dims), "label": label, "inputs": sorted(inputs),
               "results": {}}
        for dt, dn in ((np.float64, "f64"), (np.float32, "f32")):
            ds = dataset({k: a.astype(dt) for k, a in inputs.items()}, dims)
            for name in SEVEN:
                kw = {} if name == "convert_to_linear" else {"range_label": label}
                try:
                    with np.errstate(all="ignore"):
                        out = getattr(ref, name)(ds, **kw)
                except ValueError as e:
                    rec["results"][f"{dn}/{name}"] = ["ValueError", str(e)]
                    continue
                assert out.dtype == dt, (tag, name, out.dtype)  # the float32 run stays float32 throughout
                want_dims = [d for d in dims if d != "range_sample"] if name in STATS else None
                if want_dims is not None:
                    assert list(out.dims) == want_dims, (tag, name, out.dims)
                    g[f"{tag}/{dn}/{name}"] = np.asarray(out.data)
                elif dn == "f64" and S <= 5:  # the helpers' values: small cases only, they are not the hot path
                    g[f"{tag}/{dn}/{name}"] = np.asarray(out.data)
                    rec["results"][f"{dn}/{name}"] = list(out.dims)
        cases.append(rec)

    for kind in C.KINDS:
        case(f"{kind}_33", kind, 33)
    for S in (2, 3, 5, 130):
        case(f"clean_{S}", "clean", S)
        case(f"nan_tail_{S}", "nan_tail", S)
    case("frequency_33", "clean", 33, dims=("frequency", "ping_time", "range_sample"))
    case("sample_first_5", "sv_holes", 5, dims=("range_sample", "channel", "ping_time"))
    case("depth_33", "clean", 33, label="depth")
    case("depth_alone_33", "nan_tail", 33, label="depth", with_echo_range=False)
    case("missing_5", "clean", 5, label="nothing")

    known = known_answers()
    for name, k in known.items():  # the reference passes its own tests over the shim
        ds = dataset({"Sv": np.array(k["Sv"]), "echo_range": np.array(k["echo_range"])},
                     ("frequency", "ping_time", "range_sample"))
        assert np.allclose(getattr(ref, name)(ds).data, np.array(k["expected"]), rtol=k["rtol"]), name

    g["cases"] = np.array(json.dumps(cases, sort_keys=True))
    g["known"] = np.array(json.dumps(known, sort_keys=True))
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
    print(OUT, os.path.getsize(OUT), "bytes,", len(cases), "cases")

    tree = ast.parse(open(os.path.join(REF, REL)).read())
    fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    sigs = {f"metrics.{n}": {"params": gen_ref_signatures.params(fns[n]), "line": fns[n].lineno, "file": REL}
            for n in SEVEN}
    with open(OUT_SIG, "w") as f:
        json.dump(sigs, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT_SIG, len(sigs), "signatures")


if __name__ == "__main__":
    main()
