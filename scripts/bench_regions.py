"""Throughput of the region sweep (mask.region_statistics) at C=4, P=20000, S=4096, float32, on one GPU:
(1) ``ops.region_stats`` -- the two table memsets and ``region_stats_kernel`` -- by device events, and the GB/s that
    gives for 8 + C * (4 + 4) bytes per pixel (the codes, Sv and a full range cube, read once);
(2) ``mask.region_statistics`` end to end by the host clock, synchronised;
(3) the yardstick: the same six sums and two counts per channel as device torch expressions in float64, the foreground
    pixels selected first, ``index_add_`` on their labels.
Two masks: ``synth.shoal_scene()`` tiled over the plane, ``Sv > -70`` with gaps of up to 3 samples filled (a million
mostly tiny regions), and one region that covers a plane of a quarter of the pings (every update meets one entry; the
yardstick is timed once, on one channel, without a warm-up: it takes half a minute).  Writes the JSON document to
``--out`` (default ``profiles/regions_bench.json``) after every step."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import echopype_amd as ep  # noqa: E402
from echopype_amd import ops, synth  # noqa: E402
from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray  # noqa: E402

C, P, S = 4, 20000, 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.json"))
OUT = ap.parse_args().out
res = {"C": C, "P": P, "S": S, "dtype": "float32", "device": torch.cuda.get_device_name(0)}


def save():
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


def ev_time(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


base = torch.from_numpy(synth.shoal_scene().astype(np.float32)).cuda()
plane0 = base.repeat(-(-P // 90), -(-S // 120))[:P, :S].contiguous()
sv = torch.stack([plane0 + off for off in (0.0, -3.5, 1.25, -6.0)]).contiguous()
depth = (3.0 + 0.25 * torch.arange(S, device="cuda", dtype=torch.float32)[None, None, :]
         + 0.001 * torch.arange(P, device="cuda", dtype=torch.float32)[None, :, None]
         + 0.5 * torch.arange(C, device="cuda", dtype=torch.float32)[:, None, None]).contiguous()
del plane0


def yardstick(labels, n, reps, channels, warm):
    """The same six sums and two counts with torch: float64, NaN terms skipped, the foreground pixels selected first
    (index_add_ of 72M background pixels into one entry takes seconds per call), index_add_ on their labels."""
    lab = labels.reshape(-1)

    def one():
        sel = torch.nonzero(lab > 0).reshape(-1)
        idx = lab[sel].to(torch.int64) - 1
        out = torch.zeros((channels, 8, n), dtype=torch.float64, device="cuda")
        for c in range(channels):
            x = sv[c].reshape(-1)[sel].double()
            r = depth[c].double()
            dz = torch.empty_like(r)
            dz[:, 1:] = r[:, 1:] - r[:, :-1]
            dz[:, 0] = dz[:, 1]
            r, dz = r.reshape(-1)[sel], dz.reshape(-1)[sel]
            lin = torch.pow(10.0, x / 10.0)
            xv, rv, dv = ~torch.isnan(x), ~torch.isnan(r), ~torch.isnan(dz)
            zero = torch.zeros((), dtype=torch.float64, device="cuda")
            terms = (torch.where(xv, lin, zero), torch.where(rv, r, zero), torch.where(xv & rv, lin * r, zero),
                     torch.where(xv & rv, lin, zero), torch.where(dv, dz, zero), torch.where(xv & dv, lin * dz, zero),
                     xv.double(), rv.double())
            for j, t in enumerate(terms):
                out[c, j].index_add_(0, idx, t)
        return out

    if warm:
        one()
        torch.cuda.synchronize()
    return ev_time(one, reps)


def case(name, plane, reps, yard_reps, yard_channels, yard_warm):
    print(name, "labelling", flush=True)
    state = ops.shoal_state(plane.device)
    code, table = ops.shoal_label(plane, 8, state)
    err, n = (int(v) for v in state[:2].cpu())
    assert err == 0
    r = {"n_regions": n, "foreground_fraction": float(plane.float().mean())}
    ops.region_stats(code, n, state, sv, depth)
    torch.cuda.synchronize()
    ts = ev_time(lambda: ops.region_stats(code, n, state, sv, depth), reps)
    r["sweep_ms"] = {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "reps": reps,
                     "what": "ops.region_stats: two table memsets + region_stats_kernel, device events"}
    nbytes = P * S * (8 + C * (4 + 4))
    r["sweep_GBps_at_8_plus_8C_bytes_per_pixel"] = nbytes / (np.median(ts) * 1e-3) / 1e9
    assert int(state[0]) == 0
    res[name] = r
    save()
    ds = Dataset(coords={"channel": np.arange(C), "ping_time": np.arange(P), "range_sample": np.arange(S)})
    ds["Sv"] = DataArray(DeviceArray(sv), ("channel", "ping_time", "range_sample"))
    ds["depth"] = DataArray(DeviceArray(depth), ("channel", "ping_time", "range_sample"))
    m = DataArray(DeviceArray(plane), ("ping_time", "range_sample"))
    out = ep.mask.region_statistics(ds, m)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = ep.mask.region_statistics(ds, m)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    r["region_statistics_ms"] = {"median": float(np.median(ts)), "min": min(ts), "what": "end to end, host clock"}
    save()
    labels = out["region_label"].data.tensor
    del code, table
    print(name, "sweep and region_statistics timed, yardstick next", flush=True)
    ys = yardstick(labels, n, yard_reps, yard_channels, yard_warm)
    r["torch_index_add_ms"] = {"median": float(np.median(ys)), "min": min(ys), "reps": yard_reps, "channels": yard_channels,
                               "what": "six sums + two counts per channel, float64, foreground selected, index_add_"}
    r["sweep_speedup_over_torch_per_channel"] = float((np.median(ys) / yard_channels) / (r["sweep_ms"]["median"] / C))
    save()
    print(name, json.dumps(r), flush=True)


case("tiled_shoal_scene", ops.shoal_threshold_fill(sv[0], -70.0, maxvgap=3), 10, 3, C, True)
# one region that covers everything: a quarter of the pings (the labelling of one 82M-pixel component is not the subject)
P = 5000
sv, depth = sv[:, :P].contiguous(), depth[:, :P].contiguous()
res["one_big_region_P"] = P
case("one_big_region", torch.ones((P, S), dtype=torch.bool, device="cuda"), 5, 1, 1, False)
print("done", flush=True)
