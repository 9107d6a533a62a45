#!/usr/bin/env python3
"""Transient-noise detection (clean.detect_transient), both methods with the reference's default parameters: one JSON
line per measurement with the time of an API call (median of --steps timed calls after --warmup, all of them listed),
the algorithmic bytes (one read of the layer / window rows plus one write of the mask) and their fraction of 8 TB/s.

  scenes      float32, 1 x 200 000 x 2500 on a 0.4 m range grid (2500 samples of a 0.19 m grid end at 475 m, above
              Fielding's default 900-1000 m layer: the call would return at once), built in HBM (no PCIe in the timed
              calls): background -78 dB with a spread of 2 dB; a share of the pings -- 0 %, 0.1 %, 5 % -- raised by
              15 dB from row 300 down, so both methods flag them (Fielding walks up 150 steps for each)
  small       1 x 2000 x 600 on a 1.7 m grid (synth.transient_scene): both API calls
  --ref-host  (authoring machine, needs the reference checkout) the reference's own detectors over the xarray shim
              on the host on that 2000 x 600 plane

--scale shrinks the ping counts."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF_SIZE = (2000, 600)
DIMS = ("channel", "ping_time", "range_sample")
PRM = {"range_var": "depth"}  # everything else: the reference's defaults


def timed(f, steps, warmup):
    """Median ms of ``f()`` by device events."""
    import torch

    from echopype_amd import ops

    t = ops.Timer()
    ms = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t.start()
        f()
        t.stop()
        if k >= warmup:
            ms.append(t.elapsed_ms())
    return float(np.median(ms)), [round(m, 3) for m in ms]


def emit(out, **kw):
    s = json.dumps(kw)
    print(s, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(s + "\n")


def small_scene():
    from echopype_amd.synth import transient_scene

    return transient_scene(P=REF_SIZE[0], S=REF_SIZE[1], seed=7, dtype=np.float32, dz=1.7, elevated=40,
                           bottom_frac=(1.1, 1.2))


def scene_device(share, P, S):
    import torch

    g = torch.Generator(device="cuda").manual_seed(5)
    sv = -78.0 + 2.0 * torch.randn((P, S), generator=g, device="cuda", dtype=torch.float32)
    if share > 0:
        step = max(int(round(1.0 / share)), 1)
        sv[step // 2::step, 300:] += 15.0
    return sv


def dataset(sv, r):
    import torch

    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    P, S = sv.shape
    ds = Dataset(coords={"channel": np.array(["c"]), "ping_time": np.arange(P), "range_sample": np.arange(S)})
    ds["Sv"] = DataArray(DeviceArray(sv[None]), DIMS, name="Sv")
    ds["depth"] = DataArray(DeviceArray(torch.from_numpy(r).cuda()[None, :].expand(P, S)), DIMS[1:])
    return ds


def window_rows(r):
    """Rows of the default Fielding layer and Matecho window of a range row (for the byte figures)."""
    lay = int(np.argmin(abs(r - 1000))) - int(np.argmin(abs(r - 900))) if r[-1] >= 900 else 0
    return {"fielding": lay, "matecho": int(((r >= 220) & (r <= 670)).sum())}


def bench_scene(args, kind, sv, r):
    import echopype_amd as ep

    P, S = sv.shape
    ds = dataset(sv, r)
    rows = window_rows(r)
    for method in ("fielding", "matecho"):
        out = ep.clean.detect_transient(ds, method, PRM)
        flagged = int((~out.data.tensor.all(dim=2)).sum())
        ms, all_ms = timed(lambda: ep.clean.detect_transient(ds, method, PRM), args.steps, args.warmup)
        nbytes = P * (4 * rows[method] + S)
        emit(args.out, scene=kind, stage=f"api_{method}", volume=[1, P, S], dtype="float32", ms=round(ms, 3),
             all_ms=all_ms, us_per_ping=round(ms * 1e3 / P, 4), flagged_pings=flagged, window_rows=rows[method],
             bytes=nbytes, tb_s=round(nbytes / ms / 1e9, 4), frac_8tbs=round(nbytes / ms / 8e9, 5))


def ref_host(args):
    """The reference's own detectors on the host (the shim, NumPy, scipy; one core), at REF_SIZE."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_transient_goldens as gen

    detect_transient, _, _ = gen.load_reference()
    sc = small_scene()
    P, S = sc["Sv"].shape
    ds = gen.make_ds(sc["Sv"][None], sc["depth"][None])
    for method in ("fielding", "matecho"):
        del gen.LOG[:]
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            out = detect_transient(ds, method, dict(PRM))
        s = time.perf_counter() - t0
        emit(args.out, scene="small", stage=f"reference_host_{method}", volume=[1, P, S], dtype="float32",
             s=round(s, 3), flagged_pings=int((~np.asarray(out.values).all(axis=2)).sum()),
             note="the reference's own code (NumPy, scipy, one core) on the authoring host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref-host", action="store_true")
    ap.add_argument("--scenes", default="small,0,0.001,0.05")
    args = ap.parse_args()
    if args.ref_host:
        ref_host(args)
        return
    import torch

    for kind in args.scenes.split(","):
        if kind == "small":
            sc = small_scene()
            bench_scene(args, kind, torch.from_numpy(sc["Sv"]).cuda(), sc["depth"].astype(np.float64))
        else:
            P = int(200_000 * args.scale)
            bench_scene(args, f"raised_{kind}", scene_device(float(kind), P, 2500), 0.4 * np.arange(2500, dtype=np.float64))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
