#!/usr/bin/env python3
"""Generate tests/golden/open_raw_ek80.npz by EXECUTING THE REFERENCE'S OWN parsers on the cases of tests/raw3_cases.py.
Authoring machine only: needs the reference checkout.

The reference has no packer for RAW3, XML0 or FIL1 datagrams, so the file bytes come from the ``struct`` packers of
tests/raw3_cases.py.  They are parsed back the reference's way: ``ek_raw_parsers.py`` and ``parse_base.py`` are loaded as
they are over stand-in modules (``gen_open_raw_goldens.load_reference``), every datagram goes through the ``from_string``
of its parser class, the first one becomes ``config_datagram`` (its ``EC150`` channels removed as ``parse_raw`` removes
them), and the rest is fed to ``ParseEK._read_datagrams`` by an object whose ``read(1)`` hands out those parsed datagrams
and ends with ``SimradEOF``.  Then ``ParseEK._parse_and_pad_datagram`` pads power, angle and complex samples per channel.

One step needs help: a RAW3 with count 0 parses to a ONE-dimensional empty complex array, which ``pad_shorter_ping``
cannot concatenate with the two-dimensional arrays of the channel's other pings.  Such entries are reshaped to
``(0, sectors)`` before ``_parse_and_pad_datagram`` runs (case ``edges`` only); the padding itself is the reference's.

Stored, data only: per case the file bytes and the record list (offset, size, type, time stamps); per channel the
reference's padded real / imag (float32: the values are float32 numbers widened), power (float64) and angle arrays, its
ping times and the scalar fields of every ping's merged RAW3 + parameter dict (recorded where ``_read_datagrams`` hands it to
``_append_channel_ping_data``: the per-field lists of ``ping_data_dict`` lose the ping a value belongs to when a channel
alternates CW and LFM); the parsed configuration, environment,
FIL1 and MRU0 contents as JSON."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gen_open_raw_goldens import load_reference  # noqa: E402

import raw3_cases as R  # noqa: E402

SKIP = ("type", "spare", "timestamp", "bytes_read", "complex_dtype", "power", "angle", "complex", "low_date", "high_date")


def plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


def ns(t):
    return int(np.datetime64(t, "ns").astype(np.int64))


def build_case(parsers, base, name, out):
    data, off, size, specs = R.built(name)
    out[f"{name}/bytes"] = data
    out[f"{name}/rec_offset"], out[f"{name}/rec_size"] = off, size
    out[f"{name}/rec_type"] = np.array([d["kind"] for d in specs], "S4")
    out[f"{name}/rec_ticks"] = np.array([d["ticks"] for d in specs], np.uint64)
    by_type = {"RAW": parsers.SimradRawParser(), "XML": parsers.SimradXMLParser(), "FIL": parsers.SimradFILParser(),
               "NME": parsers.SimradNMEAParser(), "MRU": parsers.SimradMRUParser()}
    raw = data.tobytes()
    dgrams = [by_type[d["kind"][:3]].from_string(raw[int(o):int(o) + int(n)], int(n) + 8) for d, o, n in zip(specs, off, size)]
    for d in dgrams:
        if hasattr(d["timestamp"], "replace"):
            d["timestamp"] = d["timestamp"].replace(tzinfo=None)

    class Feed:
        def __init__(self, items):
            self.items = list(items)

        def read(self, n):
            if not self.items:
                raise sys.modules["echopype.convert.utils.ek_raw_io"].SimradEOF()
            return self.items.pop(0)

    class EndOfFile(Exception):
        pass

    sys.modules["echopype.convert.utils.ek_raw_io"].SimradEOF = EndOfFile
    base.SimradEOF = EndOfFile
    p = base.ParseEK(f"{name}.raw", "", "", None, "EK80")
    p.config_datagram = dgrams[0]
    p.config_datagram["timestamp"] = np.datetime64(p.config_datagram["timestamp"], "[ns]")
    for ch in [c for c in p.config_datagram["configuration"] if "EC150" in c]:  # (parse_base.py:369-374)
        p.config_datagram["configuration"].pop(ch)
    merged, append = {}, p._append_channel_ping_data

    def record(datagram, raw_type="receive"):  # the merged RAW3 + parameter dict of every ping, as the reference appends it
        if raw_type == "receive":
            merged.setdefault(datagram["channel_id"], []).append({f: plain(v) for f, v in datagram.items() if f not in SKIP})
        return append(datagram, raw_type)

    p._append_channel_ping_data = record
    p._read_datagrams(Feed(dgrams[1:]))
    for ch, lst in p.ping_data_dict["complex"].items():  # see the module docstring
        nb = max((a.shape[1] for a in lst if a is not None and a.ndim == 2), default=0)
        p.ping_data_dict["complex"][ch] = [a.reshape(0, nb) if a is not None and a.ndim == 1 and nb else a for a in lst]
    for dt in ("power", "angle", "complex"):
        p._parse_and_pad_datagram(dt, {dt: True})
    chans = list(p.ping_time)
    out[f"{name}/channels"] = np.array(chans, dtype=str)
    for k, ch in enumerate(chans):
        out[f"{name}/ch{k}/ping_time"] = np.array(p.ping_time[ch], dtype="datetime64[ns]")
        assert len(merged[ch]) == len(p.ping_time[ch])
        out[f"{name}/ch{k}/params_json"] = np.array(json.dumps(merged[ch], sort_keys=True))
        cx = p.ping_data_dict["complex"].get(ch)
        if cx is not None:
            for part in ("real", "imag"):
                a = cx[part]
                assert np.array_equal(a.astype(np.float32).astype(np.float64), a, equal_nan=True)
                out[f"{name}/ch{k}/{part}"] = a.astype(np.float32)
        pw = p.ping_data_dict["power"].get(ch)
        if pw is not None:
            out[f"{name}/ch{k}/power"] = np.asarray(pw, np.float64)
        an = p.ping_data_dict["angle"].get(ch)
        if an is not None:
            out[f"{name}/ch{k}/angle"] = np.asarray(an, np.float32)
    cfg = {ch: {f: plain(v) for f, v in d.items()} for ch, d in p.config_datagram["configuration"].items()}
    out[f"{name}/config_json"] = np.array(json.dumps(cfg, sort_keys=True))
    env = {f: (ns(v) if f == "timestamp" else plain(v)) for f, v in p.environment.items()}
    out[f"{name}/environment_json"] = np.array(json.dumps(env, sort_keys=True))
    fil = []
    for key, v in p.fil.items():
        if isinstance(key, tuple) and key[2] == "coeffs":
            fil.append({"channel_id": key[0], "stage": int(key[1]), "time_ns": ns(key[3]), "real": v.real.tolist(),
                        "imag": v.imag.tolist(), "decimation_factor": int(p.fil[(key[0], key[1], "deci_fac", key[3])])})
    out[f"{name}/fil_json"] = np.array(json.dumps(fil, sort_keys=True))
    mru = {f: ([ns(t) for t in v] if f == "timestamp" else plain(v)) for f, v in p.mru0.items()}
    out[f"{name}/mru0_json"] = np.array(json.dumps(mru, sort_keys=True))
    out[f"{name}/nmea_text"] = np.array(p.nmea["nmea_string"], dtype=str)
    out[f"{name}/nmea_time"] = np.array(p.nmea["timestamp"], dtype="datetime64[ns]")
    res = sorted({c % 4 for _, _, _, c in R.block_offsets(name) if c >= 0})
    if name in ("fm", "edges"):
        assert res == [0, 1, 2, 3], res
    print(name, data.size, "bytes; complex blocks start at offsets mod 4", res, "; channels", chans)


def check_float16(parsers):
    """The reference cannot read a float16 RAW3 either: its ``from_string`` fails."""
    data, exc, _ = R.bad_variants()["float16"]
    import struct

    pos = 0
    raw = data.tobytes()
    while pos < len(raw):
        n = struct.unpack_from("<l", raw, pos)[0]
        body = raw[pos + 4:pos + 4 + n]
        if body[:4] == b"RAW3":
            try:
                parsers.SimradRawParser().from_string(body, n + 8)
            except Exception as e:  # noqa: BLE001
                print("float16 RAW3: the reference raises", type(e).__name__, e)
                return
            raise AssertionError("the reference parsed a float16 RAW3")
        pos += n + 8


def main():
    parsers, _, base = load_reference()
    out = {}
    for name in R.CASES:
        build_case(parsers, base, name, out)
    check_float16(parsers)
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
