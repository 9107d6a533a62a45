#!/usr/bin/env python3
"""Generate tests/golden/qc_reversed_time.npz by EXECUTING THE REFERENCE'S OWN qc/api.py (``_clean_reversed`` and the
expression of ``exist_reversed_time``) on the cases of tests/qc_cases.py.  Authoring machine only: needs the reference
checkout.

The reference's module is loaded as it is; ``_clean_reversed`` needs NumPy alone, so ``xarray``, the EchoData class and
the logger factory it imports are stood in for by empty modules.  ``exist_reversed_time`` only indexes its dataset by
name: a dict serves.

Stored, data only: each case's input times (datetime64 in the case's own unit), ``win_len``, what ``_clean_reversed``
returned or the type of what it raised, and what ``exist_reversed_time`` answered -- also for the NaT cases, which have no
repair.  Written with fixed zip timestamps: two runs give the same bytes."""
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
from gen_goldens import REF, _load  # noqa: E402

import qc_cases as C  # noqa: E402
import qc_ref as R  # noqa: E402

OUT = C.GOLDEN


def load_reference():
    def module(name, path=None, **members):
        m = types.ModuleType(name)
        if path:
            m.__path__ = [path]
        m.__dict__.update(members)
        sys.modules[name] = m
        return m

    module("xarray", Dataset=object, DataArray=object)
    module("echopype", REF)
    module("echopype.qc", f"{REF}/qc")
    module("echopype.echodata", EchoData=object)
    module("echopype.utils", f"{REF}/utils")
    module("echopype.utils.log", _init_logger=logging.getLogger)
    return _load("echopype.qc.api", f"{REF}/qc/api.py")


def main():
    api = load_reference()
    g, recs = {}, []
    for name in C.FIXTURE_CASES + tuple(C.ERRORS):
        c = C.case(name)
        rec = {"name": name, "win_len": c["win_len"], "unit": np.datetime_data(c["t"].dtype)[0]}
        g[f"case/{name}/in"] = c["t"]
        rec["exists"] = bool(api.exist_reversed_time({"t": c["t"].copy()}, "t"))
        try:
            out = api._clean_reversed(c["t"].copy(), c["win_len"])
        except IndexError:
            rec["raised"] = "IndexError"
        else:
            assert out.dtype == c["t"].dtype and out.shape == c["t"].shape, name
            g[f"case/{name}/out"] = out
            rec["sorted"] = bool((np.diff(out.view(np.int64)) >= 0).all())
            # the restatement must say the same before anything is stored for it to be tested against
            assert np.array_equal(out.view(np.int64), R.clean_reversed(c["t"], c["win_len"])), name
        assert (name in C.ERRORS) == ("raised" in rec), name
        recs.append(rec)
    for name in C.NAT_CASES:
        t = C.nat_case(name)
        g[f"case/{name}/in"] = t
        recs.append({"name": name, "unit": "ns", "nat": True, "exists": bool(api.exist_reversed_time({"t": t.copy()}, "t"))})
    g["cases"] = np.array(json.dumps(recs, sort_keys=True))
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
    print(OUT, os.path.getsize(OUT), "bytes,", len(recs), "cases")
    for r in recs:
        print(" ", r)


if __name__ == "__main__":
    main()
