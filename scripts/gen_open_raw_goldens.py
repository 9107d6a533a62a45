#!/usr/bin/env python3
"""Generate tests/golden/open_raw_ek60.npz and tests/golden/open_raw_signature.json by EXECUTING THE REFERENCE'S OWN
datagram code on the cases of tests/raw_cases.py.  Authoring machine only: needs the reference checkout.

The reference ships no .raw file, but its parsers can write datagrams: ``SimradRawParser()._pack_contents(d, 0)`` and
``SimradConfigParser()._pack_contents(d, 0)`` followed by ``finalize_datagram`` give framed RAW0 / CON0 datagrams (the
public ``to_string`` compares a bytes type with a str under Python 3).  NME0 / TAG0 bodies are the 12-byte header and
the text, framed by the same ``finalize_datagram``: the reference's NMEA packer pads the text to a multiple of 4, and the
point of the sentences here is that they do not.  The bytes are then parsed back with the reference's ``from_string``,
padded per channel with ``ParseBase.pad_shorter_ping`` and timed with ``nt_to_unix``; a datagram whose time stamp is
(0, 0) is skipped as ``RawSimradFile._read_next_dgram`` skips it (ek_raw_io.py:267-275).

``ek_raw_parsers.py`` and ``parse_base.py`` are loaded as they are; what they import besides NumPy, pytz and the standard
library (the logger factory, dask, zarr, the file reader) is stood in for by empty modules: none of it is run.

Stored, data only: per case the file bytes, the offset / size / type / time of every datagram as laid down, per channel
the reference-parsed and reference-padded power and angle arrays (int16 coding, NaN as -32768), ping times, header
fields, the NME0 sentences and the parsed CON0 as JSON."""
import ast
import json
import logging
import os
import struct
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_goldens import REF, _load  # noqa: E402

import raw_cases as R  # noqa: E402


def load_reference():
    def module(name, path=None, **members):
        m = types.ModuleType(name)
        if path:
            m.__path__ = [path]
        m.__dict__.update(members)
        sys.modules[name] = m
        return m

    module("echopype", REF)
    module("echopype.utils", f"{REF}/utils")
    module("echopype.utils.log", _init_logger=logging.getLogger)
    module("echopype.utils.io", create_temp_zarr_store=None)
    _load("echopype.utils.misc", f"{REF}/utils/misc.py")
    module("echopype.convert", f"{REF}/convert")
    module("echopype.convert.utils", f"{REF}/convert/utils")
    dates = _load("echopype.convert.utils.ek_date_conversion", f"{REF}/convert/utils/ek_date_conversion.py")
    parsers = _load("echopype.convert.utils.ek_raw_parsers", f"{REF}/convert/utils/ek_raw_parsers.py")
    module("echopype.convert.utils.ek_raw_io", RawSimradFile=None, SimradEOF=Exception)
    module("echopype.convert.utils.ek_swap", calc_final_shapes=None)
    module("dask")
    module("dask.array", Array=object)
    module("dask.array.core", auto_chunks=None)
    sys.modules["dask"].array = sys.modules["dask.array"]
    module("zarr", Group=object)
    base = _load("echopype.convert.parse_base", f"{REF}/convert/parse_base.py")
    return parsers, dates, base


def pack(parsers, spec):
    """One datagram spec of raw_cases -> framed bytes."""
    d = {k: v for k, v in spec.items() if k != "kind"}
    if spec["kind"] == "RAW0":
        p = parsers.SimradRawParser()
        body = p._pack_contents(d, 0)
    elif spec["kind"] == "CON0":
        p = parsers.SimradConfigParser()
        d["transceivers"] = {k: dict(v) for k, v in d["transceivers"].items()}
        body = p._pack_contents(d, 0)
    else:  # NME0 / TAG0: header + text of any length
        p = parsers.SimradNMEAParser()
        text = d["text"].encode("ascii")
        body = struct.pack("=4sLL%ds" % len(text), d["type"], d["low_date"], d["high_date"], text)
    return p.finalize_datagram(body)


def code(a):
    """A padded array of the reference (integers, or float64 with NaN) -> int16 with NaN as -32768."""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        v = np.where(nan, 0, a)
        assert np.all(v == np.round(v)) and np.all(np.abs(v) < 32768)
        out = v.astype(np.int16)
        assert not np.any((out == R.SENTINEL) & ~nan)
        out[nan] = R.SENTINEL
        return out
    assert not np.any(a == R.SENTINEL)
    return a.astype(np.int16)


def ns(dates, low, high):
    return np.datetime64(dates.nt_to_unix((low, high)).replace(tzinfo=None), "ns")


def build_case(parsers, dates, base, name, out):
    specs = R.CASES[name]()
    blobs = [pack(parsers, s) for s in specs]
    data = b"".join(blobs)
    out[f"{name}/bytes"] = np.frombuffer(data, np.uint8)
    pos, off = 0, []
    for b in blobs:
        off.append(pos + 4)
        pos += len(b)
    out[f"{name}/rec_offset"] = np.array(off, np.int64)
    out[f"{name}/rec_size"] = np.array([len(b) - 8 for b in blobs], np.int32)
    out[f"{name}/rec_type"] = np.array([s["type"] for s in specs], "S4")
    out[f"{name}/rec_low"] = np.array([s["low_date"] for s in specs], np.uint32)
    out[f"{name}/rec_high"] = np.array([s["high_date"] for s in specs], np.uint32)
    out[f"{name}/rec_time"] = np.array([ns(dates, s["low_date"], s["high_date"]) for s in specs], "datetime64[ns]")
    if name not in R.GOOD:
        return
    # parse back with the reference's parsers
    raw_p, con_p, nme_p = parsers.SimradRawParser(), parsers.SimradConfigParser(), parsers.SimradNMEAParser()
    per, nmea_t, nmea_s, cfg = {}, [], [], None
    for s, b in zip(specs, blobs):
        body = b[4:-4]
        if (s["low_date"], s["high_date"]) == (0, 0):
            continue  # ek_raw_io.py:267-275
        if s["kind"] == "CON0":
            cfg = con_p.from_string(body, len(b))
        elif s["kind"] == "RAW0":
            d = raw_p.from_string(body, len(b))
            assert d["count"] == s["count"] and d["channel"] == s["channel"]
            if "power" in s and s["count"]:
                assert np.array_equal(d["power"], s["power"])
            per.setdefault(d["channel"], []).append(d)
        elif s["kind"] == "NME0":
            d = nme_p.from_string(body, len(b))
            nmea_t.append(np.datetime64(d["timestamp"].replace(tzinfo=None), "ns"))
            nmea_s.append(d["nmea_string"])
    pad = base.ParseEK.pad_shorter_ping
    out[f"{name}/channels"] = np.array(sorted(per), np.int64)
    p_res, a_res = set(), set()
    for k, dgs in per.items():
        out[f"{name}/ch{k}/power"] = code(pad([d["power"] for d in dgs]))
        if all(d["angle"] is not None for d in dgs):
            out[f"{name}/ch{k}/angle"] = code(pad([d["angle"] for d in dgs]))
        out[f"{name}/ch{k}/ping_time"] = np.array([np.datetime64(d["timestamp"].replace(tzinfo=None), "ns") for d in dgs],
                                                   "datetime64[ns]")
        for f in R.RAW0_FLOATS:
            out[f"{name}/ch{k}/hdr_{f}"] = np.array([d[f] for d in dgs], np.float64)
        for f in R.RAW0_INTS:
            out[f"{name}/ch{k}/hdr_{f}"] = np.array([d[f] for d in dgs], np.int64)
    for s, o in zip(specs, off):
        if s["kind"] == "RAW0" and s["count"]:
            p_res.add((o + 84) % 4)
            if s["mode"] & 2:
                a_res.add((o + 84 + 2 * s["count"]) % 4)
    if name == "ragged":
        assert p_res == {0, 1, 2, 3} and a_res == {0, 1, 2, 3}, (p_res, a_res)
    print(name, len(data), "bytes; power blocks start at offsets mod 4", sorted(p_res), "angle blocks", sorted(a_res))
    out[f"{name}/nmea_time"] = np.array(nmea_t, "datetime64[ns]")
    out[f"{name}/nmea_text"] = np.array(nmea_s, dtype=str)
    tx = {}
    for k, t in cfg["transceivers"].items():
        tx[str(k)] = {f: (v.tolist() if isinstance(v, np.ndarray) else v) for f, v in t.items()}
    head = {f: v for f, v in cfg.items() if f not in ("transceivers", "timestamp")}
    head["timestamp_ns"] = int(np.datetime64(cfg["timestamp"].replace(tzinfo=None), "ns").astype(np.int64))
    out[f"{name}/con0_json"] = np.array(json.dumps({**head, "transceivers": tx}, sort_keys=True))


def signature():
    tree = ast.parse(open(f"{REF}/convert/api.py").read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "open_raw")
    a = fn.args
    pos = a.posonlyargs + a.args
    defaults = [None] * (len(pos) - len(a.defaults)) + list(a.defaults)
    params = [[arg.arg, "positional_or_keyword", None if d is None else ast.unparse(d)] for arg, d in zip(pos, defaults)]
    assert not (a.vararg or a.kwonlyargs or a.kwarg)
    with open(R.SIGNATURE, "w") as f:
        json.dump({"convert.open_raw": {"params": params, "line": fn.lineno, "file": "convert/api.py"}}, f, indent=1)
        f.write("\n")


def main():
    parsers, dates, base = load_reference()
    out = {}
    for name in R.CASES:
        build_case(parsers, dates, base, name, out)
    np.savez_compressed(R.GOLDEN, **out)
    signature()
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
