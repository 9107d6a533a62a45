#!/usr/bin/env python3
"""``consolidate.add_location`` at a long deployment's size: P = 2 000 000 pings against a navigation track of
N = 100 000 fixes, latitude and longitude (V = 2), linear mode.  Four numbers from one run, each the median (and the
minimum) of 20 timed calls after 3 warm-up calls, as DESIGN.md section 6 takes them:

1. the kernel alone (``ops.align_to_ping_time`` on resident tensors; HIP events around the call);
2. the API call ``consolidate.add_location`` on a dataset whose ``ping_time`` lives on the host (host clock, ended by a
   device synchronise): the checks of the track, the upload of ``ping_time`` (16 MB) and of the track, the launch --
   with the upload of ``ping_time`` alone timed next to it, and the call again with ``ping_time`` resident;
3. the same formula as a torch expression on the device (``torch.searchsorted`` plus gathers; HIP events);
4. the reference's scipy call on the host, ``interp1d(kind="linear", fill_value="extrapolate")`` for the two variables
   (host clock; 5 calls).

The kernel's result is compared bit for bit with (3) and (4) first.  Bytes the kernel has to move: 8 P read + 16 P written
(the track stays in L2).  Writes the JSON document to ``--out`` (default profiles/location_bench.json) and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import echopype_amd as ep  # noqa: E402
from echopype_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pings", type=int, default=2_000_000)
ap.add_argument("--fixes", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "location_bench.json"))
args = ap.parse_args()
P, N, REPS = args.pings, args.fixes, args.reps


def med_min(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "calls": len(ts)}


def timed_events(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return med_min(ts)


def timed_host(fn, reps=REPS, warm=3, sync=True):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return med_min(ts)


rng = np.random.default_rng(20261019)
t0 = np.datetime64("2026-03-01T00:00:00", "ns").astype(np.int64)
t_ext = t0 + np.cumsum(rng.integers(500_000_000, 1_500_000_000, N, dtype=np.int64))  # a fix a second: 28 hours
y = np.stack([45.0 + np.cumsum(rng.normal(0, 1e-5, N)), -125.0 + np.cumsum(rng.normal(0, 1e-5, N))])
span = int(t_ext[-1] - t_ext[0])
pt = np.sort(t_ext[0] - span // 100 + rng.integers(0, span + span // 50, P, dtype=np.int64))  # both ends extrapolate

t_d, y_d, pt_d = ops.to_device(t_ext), ops.to_device(y), ops.to_device(pt)


def torch_linear():
    x = (t_d - t_d[0]).double()
    q = (pt_d - t_d[0]).double()
    k = torch.searchsorted(x, q).clamp(1, N - 1)
    xa = x[k - 1]
    slope = (y_d[:, k] - y_d[:, k - 1]) / (x[k] - xa)
    return slope * (q - xa) + y_d[:, k - 1]


x_h, q_h = (t_ext - t_ext[0]).astype(np.float64), (pt - t_ext[0]).astype(np.float64)


def scipy_linear():
    from scipy.interpolate import interp1d

    return np.stack([interp1d(x_h, y[v], kind="linear", bounds_error=False, copy=False, assume_sorted=False,
                              fill_value="extrapolate")(q_h) for v in range(2)])


got = ops.align_to_ping_time(t_d, y_d, pt_d, "linear").cpu().numpy()
ref = scipy_linear()
assert (got.view(np.int64) == ref.view(np.int64)).all(), "the kernel differs from scipy"
same_as_torch = bool((torch_linear().cpu().numpy().view(np.int64) == got.view(np.int64)).all())

plat = ep.Dataset()
tt = t_ext.astype("datetime64[ns]")
plat["latitude"] = ep.DataArray(y[0], ("time1",), {"time1": tt})
plat["longitude"] = ep.DataArray(y[1], ("time1",), {"time1": tt})
ed = ep.EchoData("EK60")
ed["Platform"] = plat
ds = ep.Dataset(coords={"ping_time": pt.astype("datetime64[ns]")})
ds_resident = ep.Dataset(coords={"ping_time": pt.astype("datetime64[ns]")})
ds_resident["ping_time"].values.flags.writeable = False  # (what EchoData.to_device does: the upload is paid once)
out = ep.consolidate.add_location(ds, ed)
assert (out["latitude"].values.view(np.int64) == ref[0].view(np.int64)).all()

res = {
    "shape": {"pings": P, "fixes": N, "rows": 2, "mode": "linear"},
    "device": torch.cuda.get_device_name(0),
    "bit_equal_to_scipy": True,
    "torch_expression_bit_equal_to_kernel": same_as_torch,
    "kernel_alone": timed_events(lambda: ops.align_to_ping_time(t_d, y_d, pt_d, "linear")),
    "kernel_alone_nearest": timed_events(lambda: ops.align_to_ping_time(t_d, y_d, pt_d, "nearest")),
    "api_add_location_ping_time_on_host": timed_host(lambda: ep.consolidate.add_location(ds, ed)),
    "api_add_location_ping_time_resident": timed_host(lambda: ep.consolidate.add_location(ds_resident, ed)),
    "upload_of_ping_time_alone": timed_host(lambda: ops.to_device(pt)),
    "torch_expression_on_device": timed_events(torch_linear),
    "scipy_interp1d_on_host": timed_host(scipy_linear, reps=5, warm=1, sync=False),
}
k = res["kernel_alone"]["ms_median"]
res["kernel_alone"]["bytes"] = 24 * P
res["kernel_alone"]["TB_per_s"] = 24 * P / k / 1e9
res["torch_over_kernel"] = res["torch_expression_on_device"]["ms_median"] / k
res["upload_share_of_api_call"] = (res["upload_of_ping_time_alone"]["ms_median"]
                                   / res["api_add_location_ping_time_on_host"]["ms_median"])
doc = json.dumps(res, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(doc + "\n")
print(doc)
