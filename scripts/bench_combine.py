#!/usr/bin/env python3
"""``combine_echodata`` at a survey's size: 64 files of 4 x 30 000 x {2000 ... 2600} float32 samples, each already resident
(about 71 GB of sources, 80 GB of output: the card holds both, and one of the two outputs at a time).  Per run:

1. the ``ops.concat_rows`` CALL on the 64 tensors -- device events around the call.  The window holds the one launch of
   ``concat_rows_kernel`` and what the call does before it: the allocation of the output from torch's cache and the
   upload of the segment table (2.5 KB, new pointers' worth of content, staged and copied in every call; the 1 KB channel
   table is cached after the first call).  It is a call time, and so a lower bound on the kernel's rate;
2. the whole ``combine_echodata`` call on 64 resident ``EchoData`` objects -- host clock ended by a device synchronise;
3. the same volume built with ``torch.full(NaN)`` and one slice assignment per file on the device -- device events.

Each number is the median, minimum and maximum of ``--reps`` (at least 5) timed runs after 2 warm-up runs; (1) and (3)
alternate inside one process so that they see the same machine.  TB/s counts the source bytes plus the output bytes, once
each, over the time -- what the join needs, not what a method happens to move.  Both results are checked against the
sources slice by slice, bit for bit, and the pad against NumPy's NaN pattern, before anything is timed.

The KERNEL's own time comes from a run of its own under the profiler (tracing slows the host, so none of the numbers
above are taken there):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_combine.py --reps 5 --out /dev/null

``--kernel-stats DIR`` then reads the ``*kernel_stats.csv`` that run left under DIR and records the row of
``concat_rows_kernel`` next to the call times.  Writes the JSON document to ``--out`` (default
profiles/combine_bench.json) and prints it."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import echopype_amd as ep  # noqa: E402
from echopype_amd import _lib, ops  # noqa: E402
from echopype_amd.echodata import BEAM1  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--files", type=int, default=64)
ap.add_argument("--channels", type=int, default=4)
ap.add_argument("--pings", type=int, default=30_000)
ap.add_argument("--smin", type=int, default=2000)
ap.add_argument("--smax", type=int, default=2600)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this script")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine_bench.json"))
args = ap.parse_args()
if args.reps < 5:
    ap.error("--reps must be at least 5: the spread is part of the result")
F, C, P, REPS = args.files, args.channels, args.pings, args.reps
dev = torch.device("cuda", 0)
rng = np.random.default_rng(20261019)
widths = rng.integers(args.smin, args.smax + 1, F)
widths[rng.integers(0, F)] = args.smax
widths = [int(w) for w in widths]
W = max(widths)
NAN_WORD = 0x7FC00000


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts)), "runs": len(ts)}


srcs = []
for i, w in enumerate(widths):  # values and a NaN tail on every tenth ping, like the converter's padding inside a file
    t = torch.randn((C, P, w), dtype=torch.float32, device=dev)
    t[:, ::10, w - 50:] = float("nan")
    srcs.append(t)
src_bytes = sum(t.numel() * 4 for t in srcs)
out_bytes = C * P * F * W * 4
need = src_bytes + out_bytes


def check(out, what):
    p0 = 0
    for t, w in zip(srcs, widths):
        part = out[:, p0:p0 + P]
        assert torch.equal(part[:, :, :w].view(torch.int32), t.view(torch.int32)), (what, "file at ping", p0)
        assert bool((part[:, :, w:].view(torch.int32) == NAN_WORD).all()), (what, "pad at ping", p0)
        p0 += P


def kernel_call():
    return ops.concat_rows(srcs)


def torch_call():
    out = torch.full((C, F * P, W), float("nan"), dtype=torch.float32, device=dev)
    p0 = 0
    for t, w in zip(srcs, widths):
        out[:, p0:p0 + P, :w] = t
        p0 += P
    return out


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    del out
    return a.elapsed_time(b)


with _lib.launch_trace() as tr:
    out = kernel_call()
assert tr.kernels == ["concat_rows_kernel"], tr.kernels
check(out, "epa_concat_rows")
del out
out = torch_call()
check(out, "torch.full + slice assignments")
del out
for _ in range(2):
    events(kernel_call)
    events(torch_call)
t_kernel, t_torch = [], []
for _ in range(REPS):  # alternating: both see the same machine
    t_kernel.append(events(kernel_call))
    t_torch.append(events(torch_call))

# the whole call: 64 resident EchoData objects in, one out
t0 = np.datetime64("2026-03-01T00:00:00", "ns")
eds = []
for i, (t, w) in enumerate(zip(srcs, widths)):
    pt = t0 + ((i * P + np.arange(P)) * 1_000_000_000).astype("timedelta64[ns]")
    beam = ep.Dataset(coords={"channel": [f"ch{c}" for c in range(C)], "ping_time": pt, "range_sample": np.arange(w)})
    beam.data_vars["backscatter_r"] = ep.DataArray(ep.DeviceArray(t), ("channel", "ping_time", "range_sample"),
                                                   name="backscatter_r")
    eds.append(ep.EchoData("EK60", {BEAM1: beam}, source_file=f"file{i:03d}.raw"))


def api_call():
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    with _lib.launch_trace() as trace:
        ed = ep.combine_echodata(eds)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t_start) * 1e3
    assert trace.kernels.count("concat_rows_kernel") == 1, trace.kernels
    shape = ed[BEAM1]["backscatter_r"].shape
    del ed
    return ms, shape


for _ in range(2):
    api_call()
t_api = []
for _ in range(REPS):
    ms, shape = api_call()
    t_api.append(ms)
assert shape == (C, F * P, W), shape


def kernel_stats(folder):
    """The row of concat_rows_kernel in the profiler's kernel statistics (times in ns there, ms here)."""
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "concat_rows_kernel" not in row.get("Name", ""):
                    continue
                col = {key.lower(): key for key in row}  # Name, Calls, TotalDurationNs, AverageNs, Percentage, MinNs, MaxNs, StdDev
                avg = float(row[col["averagens"]])
                return {"source": "rocprofv3 --kernel-trace --stats, a run of its own; every launch of that run",
                        "launches": int(row[col["calls"]]), "ms_average": avg * 1e-6,
                        "ms_min": float(row[col["minns"]]) * 1e-6, "ms_max": float(row[col["maxns"]]) * 1e-6,
                        "TB_per_s_average": need / (avg * 1e-9) / 1e12}
    raise SystemExit(f"no concat_rows_kernel row in a *kernel_stats.csv under {folder}")


k, tt = summary(t_kernel), summary(t_torch)
res = {
    "device": torch.cuda.get_device_name(0),
    "workload": {"files": F, "channels": C, "pings_per_file": P, "range_samples": [min(widths), max(widths)],
                 "dtype": "float32", "source_bytes": src_bytes, "output_bytes": out_bytes, "resident": True},
    "bit_equal_to_the_sources_and_numpy_nan": True,
    "tuning": "untuned: the first version of the kernel, rows per workgroup and access scheme as first written",
    "bytes_counted": "source bytes + output bytes, once each",
    "concat_rows_kernel_alone": kernel_stats(args.kernel_stats) if args.kernel_stats else "not measured",
    "ops_concat_rows_call_by_device_events": {**k, "TB_per_s_median": need / (k["ms_median"] * 1e-3) / 1e12,
                                   "TB_per_s_range": [need / (k["ms_max"] * 1e-3) / 1e12, need / (k["ms_min"] * 1e-3) / 1e12]},
    "torch_full_plus_slice_assignments": {**tt, "launches": 1 + F,
                                          "TB_per_s_median_same_bytes": need / (tt["ms_median"] * 1e-3) / 1e12,
                                          "TB_per_s_range_same_bytes": [need / (tt["ms_max"] * 1e-3) / 1e12,
                                                                        need / (tt["ms_min"] * 1e-3) / 1e12]},
    "combine_echodata_whole_call": {**summary(t_api), "TB_per_s_median": need / (float(np.median(t_api)) * 1e-3) / 1e12},
    "call_over_torch_time_ratio_median": k["ms_median"] / tt["ms_median"],
}
doc = json.dumps(res, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(doc + "\n")
print(doc)
