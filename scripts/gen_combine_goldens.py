#!/usr/bin/env python3
"""Generate tests/golden/combine_logic.json by EXECUTING THE REFERENCE'S OWN echodata/combine.py -- its
``_create_channel_selection_dict``, ``_check_channel_consistency``, ``_merge_attributes``, ``_check_ascending_ds_times`` and
``check_eds`` -- on the cases of tests/combine_cases.py.  Authoring machine only: needs the reference checkout.

The reference's module is loaded as it is.  The five functions need NumPy and the standard library alone, so what the
module imports besides (``fsspec``, ``pandas``, ``xarray``, the EchoData class, the logger factory, ``validate_output_path``,
``echopype_prov_attrs``) is stood in for by empty modules.  ``_check_ascending_ds_times`` reads ``.dims`` and
``ds[time].values`` of its datasets, ``check_eds`` three attributes of its EchoData objects: the small classes of the cases
file serve.  The reference's ``_combine`` itself is NOT run: it needs ``xr.concat`` with an outer join.

Stored, data only: per function and case, what the function returned (JSON) or the name of the exception type it raised."""
import copy
import json
import logging
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_goldens import REF, _load  # noqa: E402

import combine_cases as C  # noqa: E402


def load_reference():
    def module(name, path=None, **members):
        m = types.ModuleType(name)
        if path:
            m.__path__ = [path]
        m.__dict__.update(members)
        sys.modules[name] = m
        return m

    module("fsspec")
    module("pandas")
    module("xarray", Dataset=object, DataArray=object, DataTree=object)
    module("echopype", REF)
    module("echopype.echodata", f"{REF}/echodata")
    module("echopype.echodata.echodata", EchoData=C.FileStub)
    module("echopype.utils", f"{REF}/utils")
    module("echopype.utils.io", validate_output_path=None)
    module("echopype.utils.log", _init_logger=logging.getLogger)
    module("echopype.utils.prov", echopype_prov_attrs=None)
    return _load("echopype.echodata.combine", f"{REF}/echodata/combine.py")


def call(ref, fn, case):
    """The arguments of ``case`` (a fresh copy: two of the functions sort their inputs in place) -> the call's result."""
    case = copy.deepcopy(case)
    if fn == "_check_ascending_ds_times":
        return ref._check_ascending_ds_times(C.ascending_datasets(case), "test_group")
    if fn == "check_eds":
        model, names = ref.check_eds([C.FileStub(*e) for e in case["eds"]])
        return [model, names]
    return getattr(ref, fn)(**case)


def main():
    ref = load_reference()
    out = {}
    for fn, cases in C.LOGIC.items():
        out[fn] = {}
        for name, case in cases.items():
            try:
                rec = {"result": call(ref, fn, case)}
            except Exception as e:  # noqa: BLE001 - the type is the record
                rec = {"raised": type(e).__name__}
            json.dumps(rec)
            out[fn][name] = rec
            print(fn, name, rec)
    with open(C.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(C.GOLDEN, os.path.getsize(C.GOLDEN), "bytes,", sum(len(v) for v in out.values()), "cases")


if __name__ == "__main__":
    main()
