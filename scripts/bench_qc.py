#!/usr/bin/env python3
"""``qc.exist_reversed_time`` and ``qc.coerce_increasing_time`` at a long deployment's size: N = 2 000 000 times (16 MB)
with 0, 10 and 10 000 reversals, ``win_len`` = 100.  For each count, each number the median (and the minimum) of 20 timed
calls after 3 warm-up calls, host clock ended by a device synchronise:

1. ``exist_reversed_time`` on a coordinate that lives on the host (uploaded by the call) and on a resident one;
2. ``coerce_increasing_time`` likewise (every call on a fresh dataset around the same array: the repair replaces the
   coordinate) -- with 0 reversals this is the call that finds nothing to do;
3. the restated formula in NumPy on the same host (vectorised ``diff`` / ``cumsum``, a ``np.median`` per reversal), and
   its ``(diff < 0).any()`` alone;
4. ``torch.diff`` + ``any`` and ``torch.diff`` + ``torch.cumsum`` over resident ticks on the device (HIP events): the two
   sweeps of the repair without the medians, not a repair.

The repaired coordinate is compared bit for bit with (3) first.  Writes the JSON document to ``--out`` (default
profiles/qc_bench.json) and prints it."""
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
ap.add_argument("--times", type=int, default=2_000_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--win-len", type=int, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qc_bench.json"))
args = ap.parse_args()
N, REPS, WIN = args.times, args.reps, args.win_len


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


def numpy_exist(t):
    return bool((np.diff(t) < np.timedelta64(0, "ns")).any())


def numpy_repair(t, win_len):
    """The restated formula on int64 ticks: all medians from the original differences, then one cumulative sum."""
    ns = t.view(np.int64)
    d = np.diff(ns)
    neg = np.flatnonzero(d < 0)
    if neg.size == 0:
        return t
    sub = np.empty(neg.size, dtype=np.int64)
    for k, ni in enumerate(neg):
        w = np.sort(d[max(0, ni - win_len):ni])
        n = w.size
        s = w[(n - 1) // 2] + w[n // 2]
        sub[k] = w[n // 2] if n % 2 else (s + (s < 0)) >> 1  # truncation toward zero
    d[neg] = sub
    f = neg[0]
    out = ns.copy()
    out[f + 1:] = ns[f] + np.cumsum(d[f:])
    return out.view(t.dtype)


def coordinate(n_rev, rng):
    d = rng.integers(900_000_000, 1_100_000_000, N - 1, dtype=np.int64)  # a ping a second
    if n_rev:
        at = rng.choice(np.arange(1, N - 1), n_rev, replace=False)
        d[at] = -rng.integers(1, 3_000_000_000, n_rev, dtype=np.int64)
    t0 = np.datetime64("2026-03-01T00:00:00", "ns").astype(np.int64)
    return (t0 + np.concatenate([[0], np.cumsum(d)])).view("datetime64[ns]")


def api_calls(t, resident):
    arr = t.copy()
    if resident:
        arr.flags.writeable = False
        ops.ping_time_facts(arr)  # (what EchoData.to_device does: the upload is paid once)

    def exist():
        return ep.qc.exist_reversed_time(ep.Dataset(coords={"ping_time": arr}), "ping_time")

    def coerce():
        ep.qc.coerce_increasing_time(ep.Dataset(coords={"ping_time": arr}), "ping_time", WIN)

    return exist, coerce


rng = np.random.default_rng(20261019)
res = {"shape": {"times": N, "bytes": 8 * N, "win_len": WIN}, "device": torch.cuda.get_device_name(0), "reversals": {}}
for n_rev in (0, 10, 10_000):
    t = coordinate(n_rev, rng)
    ds = ep.Dataset(coords={"ping_time": t.copy()})
    assert ep.qc.exist_reversed_time(ds, "ping_time") == numpy_exist(t) == (n_rev > 0)
    ep.qc.coerce_increasing_time(ds, "ping_time", WIN)
    want = numpy_repair(t, WIN)
    assert np.array_equal(ds["ping_time"].values.view(np.int64), want.view(np.int64)), "the package differs from NumPy"
    t_d = ops.to_device(t)
    exist_h, coerce_h = api_calls(t, resident=False)
    exist_r, coerce_r = api_calls(t, resident=True)
    res["reversals"][str(n_rev)] = {
        "bit_equal_to_numpy": True,
        "still_reversed_after_repair": numpy_exist(want),
        "exist_reversed_time_host_coordinate": timed_host(exist_h),
        "exist_reversed_time_resident": timed_host(exist_r),
        "coerce_increasing_time_host_coordinate": timed_host(coerce_h),
        "coerce_increasing_time_resident": timed_host(coerce_r),
        "numpy_exist_on_host": timed_host(lambda: numpy_exist(t), sync=False),
        "numpy_repair_on_host": timed_host(lambda: numpy_repair(t, WIN), reps=5 if n_rev > 1000 else REPS, warm=1, sync=False),
        "torch_diff_any_on_device": timed_events(lambda: (torch.diff(t_d) < 0).any()),
        "torch_diff_cumsum_on_device": timed_events(lambda: t_d[0] + torch.cumsum(torch.diff(t_d), 0)),
    }
res["upload_of_the_times_alone"] = timed_host(lambda: ops.to_device(t))
res["download_of_the_times_alone"] = timed_host(lambda: t_d.cpu())
doc = json.dumps(res, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(doc + "\n")
print(doc)
