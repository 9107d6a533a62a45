#!/usr/bin/env python3
"""``open_raw`` at a survey file's size: an EK60 file of 4 channels x 30 000 pings x 2600 samples, mode 3 (int16 power and
int8 angle pairs, 4 B per sample), an NME0 sentence behind every ping whose length walks through all residues mod 4 --
so the sample blocks start at every byte offset mod 4 --, about 1.25 GB.  The file is written here with a few lines of
``struct`` and NumPy (scripts/raw_bench_file.py; sample values from a small random pool: the contents do not change what is
moved).

Per quantity the median, minimum and maximum of ``--reps`` (at least 7) timed runs after 2 warm-up runs:

1. the unpack KERNEL alone -- device events around ``epa_raw0_unpack`` with the file, the row table and the three outputs
   already in HBM; the host checks of the entry point run before the launch and are not in the window.  Bytes counted:
   the file's sample bytes read once plus the output bytes written once, against 8 TB/s; ``concat_rows_kernel`` measured
   0.74 of that on this card (profiles/combine_bench.json) -- a comparison, not a gate;
2. the host half: the framing walk, the header gather and the row table (``parse_ek60.plan``), host clock;
3. the upload of the file's bytes (``ops.to_device``), host clock ended by a device synchronise;
4. the whole ``open_raw`` call, file on disk (page cache) to resident EchoData, host clock ended by a synchronise;
5. the route a user has today, restated with NumPy in the same process: ``np.frombuffer`` per datagram, stacking (the
   pings here are all of one length, so the reference's ``pad_shorter_ping`` is ``np.array(list)``), ``astype(float32) *
   k``, the angle planes, then ``from_ek60_arrays(...).to_device()`` -- 4 B per sample and separate planes over PCIe.

The volumes of (4) are compared with those of (5) bit for bit before anything is timed.  Writes the JSON document to
``--out`` (default profiles/open_raw_bench.json) and prints it."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raw_bench_file  # noqa: E402
import echopype_amd as ep  # noqa: E402
from echopype_amd import _lib, ops  # noqa: E402
from echopype_amd.convert import api, parse_ek60  # noqa: E402
from echopype_amd.echodata import BEAM1  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=4)
ap.add_argument("--pings", type=int, default=30_000)
ap.add_argument("--samples", type=int, default=2600)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--baseline-reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_raw_bench.json"))
args = ap.parse_args()
if args.reps < 7 or args.baseline_reps < 7:
    ap.error("--reps and --baseline-reps must be at least 7: the spread is part of the result")
C, P, S, REPS = args.channels, args.pings, args.samples, args.reps
K = np.float32(10.0 * np.log10(2.0) / 256.0)
HBM_PEAK = 8.0e12


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts)), "runs": len(ts)}


# ---- the file (scripts/raw_bench_file.py, shared with bench_nmea.py) ------------------------------------------------------
NMEA = [b"$GPGLL,4704.12,N,12503.43,W,234911,A*2" + b"x" * r for r in range(4)]


def build_file(path):
    return raw_bench_file.build_file(path, C, P, S, lambda p: NMEA[p % 4], nme0_delay=5)[0]


# ---- the route of today, restated with NumPy ------------------------------------------------------------------------------
def numpy_route(path):
    data = open(path, "rb").read()
    pos, n = 0, len(data)
    power, angle, hdrs, times = [[] for _ in range(C)], [[] for _ in range(C)], [[] for _ in range(C)], [[] for _ in range(C)]
    while pos + 4 <= n:
        size = struct.unpack_from("<l", data, pos)[0]
        body = pos + 4
        if data[body:body + 4] == b"RAW0":
            h = struct.unpack_from("<4sLLhh13fh6sll", data, body)
            c, count = h[3] - 1, h[-1]
            power[c].append(np.frombuffer(data, "<i2", count, body + 84))
            angle[c].append(np.frombuffer(data, np.int8, 2 * count, body + 84 + 2 * count).reshape(-1, 2))
            hdrs[c].append(h)
            times[c].append((h[2] << 32) + h[1])
        pos += size + 8
    bs = np.stack([np.array(rows).astype("float32") * K for rows in power])
    an = np.stack([np.array(rows) for rows in angle])
    hd = np.array([[row[5:18] for row in ch] for ch in hdrs], dtype=np.float64)  # the 13 floats
    pt = parse_ek60.nt_to_ns(np.array(times[0]) & 0xFFFFFFFF, np.array(times[0]) >> 32)
    d = {"channel": [f"ch{c}" for c in range(C)], "ping_time": pt, "backscatter_r": bs,
         "angle_athwartship": np.ascontiguousarray(an[..., 0]), "angle_alongship": np.ascontiguousarray(an[..., 1]),
         "sample_interval": hd[:, :, 5], "transmit_duration_nominal": hd[:, :, 3], "transmit_power": hd[:, :, 2],
         "sound_speed_indicative": hd[:, :, 6], "absorption_indicative": hd[:, :, 7],
         "frequency_nominal": hd[:, 0, 1], "equivalent_beam_angle": np.full(C, -20.0), "beam_type": np.ones(C, np.int64),
         "pulse_length": np.tile([0.000256, 0.000512, 0.001024, 0.002048, 0.004096], (C, 1)),
         "gain_correction": np.full((C, 5), 25.0), "sa_correction": np.full((C, 5), -0.5)}
    ed = ep.echodata.from_ek60_arrays(d, source_file=path)
    ed.to_device()
    # (to_device leaves integer planes on the host: the angle planes go up as they are, 1 B per sample each)
    beam = ed[BEAM1]
    for name in ("angle_athwartship", "angle_alongship"):
        da = beam.data_vars[name]
        beam.data_vars[name] = ep.DataArray(ep.DeviceArray(ops.to_device(np.asarray(da.data))), da.dims, da.coords, da.attrs, name)
    return ed


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


tmp = tempfile.mkdtemp(prefix="open_raw_bench_")
path = os.path.join(tmp, "bench.raw")
file_bytes = build_file(path)
try:
    # correctness first: the kernel's volumes against the NumPy route's, bit for bit
    with _lib.launch_trace() as tr:
        ed = ep.open_raw(path, "EK60")
    assert tr.kernels.count("raw0_unpack_kernel<power, int8 angles>") == 1, tr.kernels
    ref = numpy_route(path)
    for name in ("backscatter_r", "angle_athwartship", "angle_alongship"):
        a, b = ed[BEAM1][name].data.tensor, ref[BEAM1][name].data.tensor
        assert a.dtype == b.dtype and a.shape == b.shape == (C, P, S), (name, a.dtype, a.shape, b.dtype, b.shape)
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), name
    assert np.array_equal(ed[BEAM1]["ping_time"].values, ref[BEAM1]["ping_time"].values)
    del ed, ref

    # (2) host half, (3) upload, (1) kernel alone
    buf, n_bytes = api.read_file(path)
    t_host = []
    for i in range(REPS + 2):
        t0 = time.perf_counter()
        pl = parse_ek60.plan(buf, n_bytes)
        if i >= 2:
            t_host.append((time.perf_counter() - t0) * 1e3)
    off = pl.table[:, 0]
    residues = sorted({int(v) % 4 for v in off[:64 * C]})
    t_up = []
    for i in range(REPS + 2):
        ms, dev = host_timed(lambda: ops.to_device(buf))
        if i >= 2:
            t_up.append(ms)
        if i < REPS + 1:
            del dev
    tab_dev = ops.to_device(pl.table)
    power = torch.empty((C, P, S), dtype=torch.float32, device=dev.device)
    athw = torch.empty((C, P, S), dtype=torch.int8, device=dev.device)
    along = torch.empty((C, P, S), dtype=torch.int8, device=dev.device)
    import ctypes

    def kernel():
        _lib.call("epa_raw0_unpack", ops._p(dev), n_bytes, dev.numel(), pl.table.ctypes.data_as(ctypes.c_void_p), ops._p(tab_dev),
                  C, P, S, _lib.RAW_ANGLE_I8, ops._p(power), ops._p(athw), ops._p(along), ops._stream())

    t_kernel = []
    for i in range(REPS + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        kernel()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            t_kernel.append(a.elapsed_time(b))
    del dev, power, athw, along, tab_dev, buf

    # (4) the whole call, (5) the NumPy route: alternating, both see the same machine
    t_api, t_np = [], []
    for i in range(max(REPS, args.baseline_reps) + 2):
        if i < REPS + 2:
            ms, out = host_timed(lambda: ep.open_raw(path, "EK60"))
            del out
            if i >= 2:
                t_api.append(ms)
        if i < args.baseline_reps + 2:
            ms, out = host_timed(lambda: numpy_route(path))
            del out
            if i >= 2:
                t_np.append(ms)
finally:
    os.remove(path)
    os.rmdir(tmp)

samples = C * P * S
need = samples * 4 + samples * 6  # 4 B of the file per sample read, float32 + 2 x int8 written
k = summary(t_kernel)
res = {
    "device": torch.cuda.get_device_name(0),
    "workload": {"channels": C, "pings": P, "range_samples": S, "mode": 3, "file_bytes": file_bytes,
                 "sample_block_offsets_mod_4": residues, "angles": "int8", "NME0_between_pings": True},
    "bit_equal_to_the_numpy_route": True,
    "tuning": "untuned, one run: one wavefront per row, aligned dword loads + byte shift, the loop over whole chunks unrolled four times",
    "bytes_counted": "file sample bytes (4 B per sample) + output bytes (float32 power, 2 x int8 angles), once each",
    "raw0_unpack_kernel_alone_by_device_events": {**k, "TB_per_s_median": need / (k["ms_median"] * 1e-3) / 1e12,
                                                  "fraction_of_8_TB_per_s": need / (k["ms_median"] * 1e-3) / HBM_PEAK,
                                                  "concat_rows_kernel_fraction_for_comparison": 0.74},
    "host_framing_walk_header_gather_row_table": summary(t_host),
    "upload_of_the_file_bytes": {**summary(t_up), "GB_per_s_median": file_bytes / (float(np.median(t_up)) * 1e-3) / 1e9},
    "open_raw_whole_call": summary(t_api),
    "numpy_route_then_to_device": summary(t_np),
    "numpy_route_over_open_raw_time_ratio_median": float(np.median(t_np)) / float(np.median(t_api)),
}
doc = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")
print(doc)
