#!/usr/bin/env python3
"""Positions from NMEA sentences at a survey file's size: the file of ``bench_open_raw.py`` (an EK60 file of 4 channels x
30 000 pings x 2600 samples, mode 3, an NME0 sentence behind every ping, about 1.25 GB) whose sentences are real GGA / GLL /
RMC text along a track, with valid checksums and lengths that walk through the residues mod 4.

Per quantity the median, minimum and maximum of ``--reps`` (at least 7) timed runs after 2 warm-up runs:

1. the positions KERNEL alone -- device events around ``epa_nmea_positions`` with the file, the table and the outputs
   already in HBM (the host checks of the entry point run before the launch and are not in the window);
2. the upload of the (n, 2) int64 table and the download of the 17 bytes per fix, each on its own, host clock ended by
   a device synchronise;
3. the whole ``open_raw`` call, file on disk (page cache) to resident EchoData with its positions, in this process and
   in a fresh child process;
4. the same call of the PARENT commit, in a child process of the same kind, when ``--parent DIR`` names a checkout of it
   with its library built (without it the entry is null); what ``open_raw`` gained is the difference of the two child
   processes' medians;
5. ``parse_nmea.parse_sentence`` over the same sentences on this machine's host: what the kernel replaces.

Before anything is timed, the positions ``open_raw`` returns are compared bit for bit with (5), and the share of sentences
the kernel left to the host is taken: it must be 0 for this file.  Writes the JSON document to ``--out`` (default
profiles/nmea_bench.json) and prints it."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time
from functools import reduce
from operator import xor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raw_bench_file  # noqa: E402
import echopype_amd as ep  # noqa: E402
from echopype_amd import _lib, ops  # noqa: E402
from echopype_amd.convert import api, parse_ek60, parse_nmea  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=4)
ap.add_argument("--pings", type=int, default=30_000)
ap.add_argument("--samples", type=int, default=2600)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmea_bench.json"))
args = ap.parse_args()
if args.reps < 7:
    ap.error("--reps must be at least 7: the spread is part of the result")
C, P, S, REPS = args.channels, args.pings, args.samples, args.reps


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts)), "runs": len(ts)}


# ---- the sentences (the file itself: scripts/raw_bench_file.py, shared with bench_open_raw.py) --------------------------------
def sentence(p):
    """The fix behind ping p: a vessel steaming north-west at about 5 m/s, the three sentence types in turn."""
    lat, lon = 47.0 + 4.5e-5 * p, -(125.0 + 1.5e-5 * p)
    la = f"{int(lat):02d}{(lat - int(lat)) * 60:0{7 + p % 3}.{4 + p % 3}f},N"
    lo = f"{int(-lon):03d}{(-lon - int(-lon)) * 60:0{7 + p // 3 % 2}.{4 + p // 3 % 2}f},W"
    hms = f"{p // 3600 % 24:02d}{p // 60 % 60:02d}{p % 60:02d}"
    body = (f"GPGGA,{hms}.00,{la},{lo},1,08,0.9,12.3,M,-20.1,M,,", f"GPGLL,{la},{lo},{hms},A",
            f"GPRMC,{hms},A,{la},{lo},9.7,315.0,120917,,")[p % 3]
    return f"${body}*{reduce(xor, body.encode(), 0):02X}".encode()


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


CHILD = """
import json, sys, time
sys.path.insert(0, sys.argv[1])
import torch
import echopype_amd as ep
ts = []
for i in range(int(sys.argv[3]) + 2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ed = ep.open_raw(sys.argv[2], "EK60")
    torch.cuda.synchronize()
    if i >= 2:
        ts.append((time.perf_counter() - t0) * 1e3)
    del ed
print(json.dumps({"ms": ts}))
"""


def child_open_raw(tree, path):
    """``open_raw`` of the package in ``tree`` on the same file, timed in a fresh child process: this tree and the parent
    commit's are measured the same way (the host buffer of 1.26 GB is new memory in both)."""
    env = {k: v for k, v in os.environ.items() if k != "ECHOPYPE_AMD_LIB"}
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(tree), path, str(REPS)], capture_output=True,
                       text=True, env=env, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"open_raw of {tree} failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms"]


tmp = tempfile.mkdtemp(prefix="nmea_bench_")
path = os.path.join(tmp, "bench.raw")
file_bytes, sentences = raw_bench_file.build_file(path, C, P, S, sentence, nme0_delay=50)
texts = [s.decode() for s in sentences]
try:
    # correctness first: open_raw's positions against parse_sentence over the same sentences, bit for bit
    with _lib.launch_trace() as tr:
        ed = ep.open_raw(path, "EK60")
    assert tr.kernels.count("nmea_positions_kernel") == 1, tr.kernels
    want = parse_nmea.positions_host(texts)
    plat = ed["Platform"]
    for got, ref in ((plat["latitude"].values, want[0]), (plat["longitude"].values, want[1])):
        assert got.shape == (P,) and np.array_equal(np.asarray(got).view(np.int64), ref.view(np.int64))
    assert list(plat["sentence_type"].values) == list(want[2]) and not np.isnan(want[0]).any()
    del ed

    buf, n_bytes = api.read_file(path)
    pl = parse_ek60.plan(buf, n_bytes)
    sel = pl.nmea_selected
    assert sel.size == P
    table = np.ascontiguousarray(np.stack([pl.nmea_offset[sel], pl.nmea_length[sel]], axis=1))
    residues = sorted({int(v) % 4 for v in table[:256, 0]})
    dev = ops.to_device(buf)
    n = int(sel.size)
    packed = torch.empty(17 * n, dtype=torch.uint8, device=dev.device)
    lat, lon, code = packed[:8 * n].view(torch.float64), packed[8 * n:16 * n].view(torch.float64), packed[16 * n:]
    t_up = []
    for i in range(REPS + 2):
        ms, tab_dev = host_timed(lambda: ops.to_device(table))
        if i >= 2:
            t_up.append(ms)

    def kernel():
        _lib.call("epa_nmea_positions", ops._p(dev), n_bytes, dev.numel(), table.ctypes.data_as(ctypes.c_void_p), ops._p(tab_dev),
                  n, ops._p(lat), ops._p(lon), ops._p(code), ops._stream())

    t_kernel, t_down = [], []
    for i in range(REPS + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        kernel()
        b.record()
        torch.cuda.synchronize()
        ms, host = host_timed(lambda: packed.cpu())
        if i >= 2:
            t_kernel.append(a.elapsed_time(b))
            t_down.append(ms)
    undecided = float((host.numpy()[16 * n:] == _lib.NMEA_UNDECIDED).mean())
    assert undecided == 0.0, undecided
    text_bytes = int(table[:, 1].sum())
    del dev, packed, lat, lon, code, tab_dev, buf

    t_api = []
    for i in range(REPS + 2):
        ms, out = host_timed(lambda: ep.open_raw(path, "EK60"))
        del out
        if i >= 2:
            t_api.append(ms)
    t_child = child_open_raw(ROOT, path)
    t_parent = child_open_raw(args.parent, path) if args.parent else None
    t_host = []
    for i in range(REPS + 2):
        t0 = time.perf_counter()
        parse_nmea.positions_host(texts)
        if i >= 2:
            t_host.append((time.perf_counter() - t0) * 1e3)
finally:
    os.remove(path)
    os.rmdir(tmp)

k = summary(t_kernel)
res = {
    "device": torch.cuda.get_device_name(0),
    "workload": {"channels": C, "pings": P, "range_samples": S, "file_bytes": file_bytes, "sentences": n,
                 "sentence_bytes": text_bytes, "types": ["GGA", "GLL", "RMC"], "valid_checksums": True,
                 "sentence_offsets_mod_4": residues},
    "bit_equal_to_parse_sentence": True,
    "share_of_sentences_left_to_the_host": undecided,
    "tuning": "untuned, one run: a wavefront per sentence, byte loads, ballot masks, digits read out of the lanes one by one",
    "nmea_positions_kernel_alone_by_device_events": {**k, "sentences_per_us_median": n / (k["ms_median"] * 1e3)},
    "upload_of_the_table": {**summary(t_up), "bytes": int(table.nbytes)},
    "download_of_17_bytes_per_fix": {**summary(t_down), "bytes": 17 * n},
    "open_raw_whole_call": summary(t_api),
    "open_raw_whole_call_in_a_child_process": summary(t_child),
    "open_raw_whole_call_parent_commit_no_positions_in_a_child_process": summary(t_parent) if t_parent else None,
    "open_raw_gained_over_parent_ms_median": (float(np.median(t_child)) - float(np.median(t_parent))) if t_parent else None,
    "parse_sentence_on_the_host_same_sentences": summary(t_host),
}
doc = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")
print(doc)
