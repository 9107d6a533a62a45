#!/usr/bin/env python3
"""Seafloor detection (mask.detect_seafloor) on one channel: one JSON line per measurement with the wall time of a
call (median of --steps timed calls after --warmup), the algorithmic bytes and their fraction of 8 TB/s.

  basic       epa_seafloor_basic over a no-detection f64 volume (every sample after bin_skip is read: 8 B/sample)
  blackwell   the whole API call, Sv / angles / depth f32 in HBM, and each stage at kernel level with its bytes per
              crop pixel: angle mask (4 + 4 read, 16 + 16 box sums written and read back, 1 mask written), median
              (4 radix passes of 1 B mask + 4 B Sv), components (init 4 + 8, merge 8 + neighbours, compress 8 + 8,
              seed 8 + 1), bottom (8 + the first kept sample's row)
  --ref-host  (authoring machine, needs the reference checkout) the reference's own bottom_blackwell over the xarray
              shim on the host at --ref-size, next to nothing: the GPU line at that size is the "blackwell_small" line

The planes are generated in HBM (no PCIe in the timed calls).  --scale shrinks the ping counts."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8.0e12
REF_SIZE = (2000, 600)


def timed(f, steps, warmup):
    import torch

    from echopype_amd import ops

    t = ops.Timer()
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t.start()
        f()
        t.stop()
        ms.append(t.elapsed_ms())
    return float(np.median(ms)), [round(m, 3) for m in ms]


def emit(out, **kw):
    s = json.dumps(kw)
    print(s, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(s + "\n")


def scene_device(P, S, dtype):
    """A seabed band (6 samples, exact angles) under a flat background, built in HBM; -> Dataset, top."""
    import torch

    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    p = torch.arange(P, device="cuda")
    top = (S * 3) // 5 + (p // 100) % (S // 5)
    sv = torch.full((1, P, S), -90.0, dtype=dtype, device="cuda")
    theta = torch.zeros((1, P, S), dtype=dtype, device="cuda")
    for j in range(6):
        sv[0, p, top + j] = -25.0
        theta[0, p, top + j] = 8.0
    depth = (torch.arange(S, dtype=dtype, device="cuda") * 0.25).expand(1, P, S).contiguous()
    ds = Dataset(coords={"channel": np.array(["c"]), "ping_time": np.arange(P), "range_sample": np.arange(S)})
    for k, t in (("Sv", sv), ("angle_alongship", theta), ("angle_athwartship", torch.zeros_like(theta)),
                 ("depth", depth)):
        ds[k] = DataArray(DeviceArray(t), ("channel", "ping_time", "range_sample"), name=k)
    return ds, top


def bench_basic(args):
    import torch

    from echopype_amd import ops

    P, S, skip = int(1_000_000 * args.scale), 4096, 200
    sv = torch.full((P, S), -120.0, dtype=torch.float64, device="cuda")
    d0 = torch.arange(S, dtype=torch.float64, device="cuda")
    ms, all_ms = timed(lambda: ops.seafloor_basic(sv, skip, -50.0, -40.0, d0, 0.5), args.steps, args.warmup)
    nbytes = P * (S - skip) * 8
    emit(args.out, method="basic", volume=[1, P, S], dtype="float64", ms=round(ms, 3), all_ms=all_ms,
         bytes=nbytes, bytes_per_sample=8, tb_s=round(nbytes / ms / 1e9, 3), frac_8tbs=round(nbytes / ms / 1e9 / 8, 3))


def bench_blackwell(args, P, S, label):
    import torch

    import echopype_amd as ep
    from echopype_amd import ops

    ds, _ = scene_device(P, S, torch.float32)
    prm = {"var_name": "Sv", "channel": "c", "threshold": (-75.0, 0.3001, 0.5), "r1": 1e6}
    ms, all_ms = timed(lambda: ep.mask.detect_seafloor(ds, "blackwell", prm), args.steps, args.warmup)
    n = P * S
    emit(args.out, method="blackwell", stage="api_call", label=label, volume=[1, P, S], dtype="float32",
         ms=round(ms, 3), all_ms=all_ms, ns_per_pixel=round(ms * 1e6 / n, 4))
    sv = ds["Sv"].data.tensor[0]
    th = ds["angle_alongship"].data.tensor[0]
    ph = ds["angle_athwartship"].data.tensor[0]
    d0 = torch.arange(S, dtype=torch.float64, device="cuda") * 0.25
    st = ops.seafloor_state(sv.device)
    stages = {}
    stages["angle_mask"] = (lambda: ops.seafloor_angle_mask(th, ph, 0, S, 28, 52, 0.3001, 0.5, st), 4 + 4 + 32 + 1)
    mask = ops.seafloor_angle_mask(th, ph, 0, S, 28, 52, 0.3001, 0.5, st)
    frac = float(mask.float().mean())
    stages["median"] = (lambda: ops.seafloor_median(sv, 0, S, mask, st), 4 * (1 + 4 * frac))
    stages["components"] = (lambda: ops.seafloor_components(sv, 0, S, -75.0, mask.clone(), st),
                            (4 + 8) + 8 + (8 + 8) + (8 + 1))
    parent = ops.seafloor_components(sv, 0, S, -75.0, mask, st)
    stages["bottom"] = (lambda: ops.seafloor_bottom(parent, mask, P, 0, d0, 0.3, torch.float32), None)
    for name, (f, bpp) in stages.items():
        ms, all_ms = timed(f, args.steps, args.warmup)
        line = dict(method="blackwell", stage=name, label=label, volume=[1, P, S], ms=round(ms, 3), all_ms=all_ms)
        if bpp is not None:
            line.update(bytes_per_pixel=round(bpp, 3), tb_s=round(bpp * n / ms / 1e9, 3),
                        frac_8tbs=round(bpp * n / ms / 1e9 / 8, 3))
        if name == "median":
            line["masked_fraction"] = round(frac, 4)
        emit(args.out, **line)


def ref_host(args):
    """The reference's own bottom_blackwell on the host (the shim + scipy), at REF_SIZE."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_seafloor_goldens as gen

    _, bottom_blackwell, _ = gen.load_reference_seafloor()
    P, S = REF_SIZE
    from echopype_amd.synth import seafloor_scene

    d = seafloor_scene(P=P, S=S, band_top=(S * 3) // 5, slope=0.0, thickness=6)
    ds = gen.make_ds(d["sv"].astype(np.float32), d["depth"].astype(np.float32), d["theta"].astype(np.float32),
                     d["phi"].astype(np.float32))
    t0 = time.perf_counter()
    bottom_blackwell(ds, "Sv", "chan1", threshold=(-75.0, 0.3001, 0.5), r1=1e6)
    s = time.perf_counter() - t0
    emit(args.out, method="blackwell", stage="reference_host", volume=[1, P, S], dtype="float32", s=round(s, 3),
         note="reference bottom_blackwell (scipy convolve2d + ndimage.label, one core) on the authoring host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref-host", action="store_true")
    args = ap.parse_args()
    if args.ref_host:
        ref_host(args)
        return
    bench_basic(args)
    bench_blackwell(args, *REF_SIZE, "blackwell_small")
    bench_blackwell(args, int(200_000 * args.scale), 2500, "blackwell_large")


if __name__ == "__main__":
    main()
