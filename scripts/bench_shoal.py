#!/usr/bin/env python3
"""Shoal detection (mask.detect_shoal) on one channel: one JSON line per measurement with the time of a call (median
of --steps timed calls after --warmup, all of them listed), the algorithmic bytes per pixel and their fraction of
8 TB/s.

  scenes      float32, 1 x 200 000 x 2500, built in HBM (no PCIe in the timed calls):
              sparse   eight large elliptical schools
              dense    speckle: about 10^6 single-pixel candidates
              huge     one school of 150 000 x 2000 pixels among 2.5 * 10^5 specks
  stages      threshold + fill (4 B read, 1 B written; the horizontal fill reads and rewrites the byte plane),
              labelling with boxes (init 1 + 8, merge 8 + neighbours, compress 8 + 8, number 8, boxes 8 + 8: about 57),
              weill filter (8 + 1), echoview link (candidates, both link scans, groups, 8 + 1 for the mask: the box
              areas are data, so no byte figure), and the two API calls
  small       1 x 2000 x 600 (synth.shoal_scene): both API calls
  --ref-host  (authoring machine, needs the reference checkout) the reference's own shoal_weill / shoal_echoview over
              the xarray shim on the host on that 2000 x 600 plane

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
WEILL = {"var_name": "Sv", "channel": "c", "maxvgap": 5, "maxhgap": 2, "minvlen": 3, "minhlen": 3}
SIZES = {"mincan": (3.0, 10.0), "maxlink": (3.0, 15.0), "minsho": (3.0, 15.0)}


def timed(f, steps, warmup, setup=None):
    """Median ms of ``f()`` by device events; ``setup()`` runs before every call, outside the timed window."""
    import torch

    from echopype_amd import ops

    t = ops.Timer()
    ms = []
    for k in range(warmup + steps):
        arg = setup() if setup else None
        torch.cuda.synchronize()
        t.start()
        f(arg) if setup else f()
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
    from echopype_amd.synth import shoal_scene

    return shoal_scene(P=REF_SIZE[0], S=REF_SIZE[1], seed=7, dtype=np.float32, schools=10, speckle=0.0005)


def scene_device(kind, P, S):
    import torch

    g = torch.Generator(device="cuda").manual_seed(5)
    sv = torch.full((P, S), -90.0, dtype=torch.float32, device="cuda")
    if kind == "sparse":
        pp = torch.arange(P, device="cuda", dtype=torch.float32)[:, None]
        ss = torch.arange(S, device="cuda", dtype=torch.float32)[None, :]
        for k in range(8):
            cp, cs = P * (k + 0.5) / 8, S * (0.25 + 0.5 * (k % 2))
            sv[((pp - cp) / (P / 20)) ** 2 + ((ss - cs) / (S / 5)) ** 2 < 1.0] = -50.0
    elif kind == "dense":
        sv[torch.rand((P, S), device="cuda", generator=g) < 0.002] = -60.0
    else:
        sv[torch.rand((P, S), device="cuda", generator=g) < 0.0005] = -60.0
        sv[P // 8:P // 8 + (3 * P) // 4, S // 10:S // 10 + (4 * S) // 5] = -50.0
    return sv


def dataset(sv):
    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    P, S = sv.shape
    ds = Dataset(coords={"channel": np.array(["c"]), "ping_time": np.arange(P), "range_sample": np.arange(S)})
    ds["Sv"] = DataArray(DeviceArray(sv[None]), ("channel", "ping_time", "range_sample"), name="Sv")
    return ds


def bench_scene(args, kind, sv, stages=True):
    import echopype_amd as ep
    from echopype_amd import ops

    P, S = sv.shape
    n = P * S
    ds = dataset(sv)
    idim, jdim = np.arange(S + 1) * 0.2, np.arange(P + 1) * 1.0
    ev = dict(var_name="Sv", channel="c", idim=idim, jdim=jdim, **SIZES)

    def line(stage, ms, all_ms, bpp=None, **kw):
        rec = dict(scene=kind, stage=stage, volume=[1, P, S], dtype="float32", ms=round(ms, 3), all_ms=all_ms,
                   ns_per_pixel=round(ms * 1e6 / n, 4), **kw)
        if bpp is not None:
            rec.update(bytes_per_pixel=bpp, tb_s=round(bpp * n / ms / 1e9, 3), frac_8tbs=round(bpp * n / ms / 8e9, 3))
        emit(args.out, **rec)

    line("api_weill", *timed(lambda: ep.mask.detect_shoal(ds, "weill", WEILL), args.steps, args.warmup))
    line("api_echoview", *timed(lambda: ep.mask.detect_shoal(ds, "echoview", ev), args.steps, args.warmup))
    if not stages:
        return
    line("threshold_vfill", *timed(lambda: ops.shoal_threshold_fill(sv, -70.0, 5, 0), args.steps, args.warmup), bpp=5)
    line("threshold_vfill_hfill", *timed(lambda: ops.shoal_threshold_fill(sv, -70.0, 5, 2), args.steps, args.warmup),
         bpp=7)
    plane = ops.shoal_threshold_fill(sv, -70.0)
    dev = sv.device
    for conn in (4, 8):
        line(f"label_{conn}", *timed(lambda: ops.shoal_label(plane, conn, ops.shoal_state(dev), conn == 8),
                                     args.steps, args.warmup), bpp=57)

    def labelled(conn):
        st = ops.shoal_state(dev)
        return (plane.clone(), *ops.shoal_label(plane, conn, st, conn == 8), st)

    line("weill_filter", *timed(lambda a: ops.shoal_weill_filter(a[0], a[1], a[2], 3, 3, a[3]), args.steps,
                                args.warmup, setup=lambda: labelled(4)), bpp=9)
    idim_d, jdim_d = ops.to_device(idim), ops.to_device(jdim)
    st = ops.shoal_state(dev)
    ops.shoal_label(plane, 8, st, True)
    line("echoview_link", *timed(lambda a: ops.shoal_echoview_link(a[0], a[1], a[2], idim_d, jdim_d, SIZES["mincan"],
                                                                  SIZES["maxlink"], SIZES["minsho"], a[3]),
                                 args.steps, args.warmup, setup=lambda: labelled(8)), components=int(st[1]))


def ref_host(args):
    """The reference's own detectors on the host (the shim + scipy + pandas), at REF_SIZE."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_shoal_goldens as gen

    detect_shoal = gen.load_reference_shoal()
    sv = small_scene()
    P, S = sv.shape
    ds = gen.make_ds(sv)
    calls = (("weill", dict(WEILL, channel="chan1")),
             ("echoview", dict(var_name="Sv", channel="chan1", idim=np.arange(S + 1) * 0.2,
                               jdim=np.arange(P + 1) * 1.0, **SIZES)))
    for method, prm in calls:
        t0 = time.perf_counter()
        out = detect_shoal(ds, method, prm)
        s = time.perf_counter() - t0
        emit(args.out, scene="small", stage=f"reference_host_{method}", volume=[1, P, S], dtype="float32",
             s=round(s, 3), kept=int(np.asarray(out.values).sum()),
             note="the reference's own code (scipy, pandas, one core) on the authoring host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref-host", action="store_true")
    ap.add_argument("--scenes", default="small,sparse,dense,huge")
    args = ap.parse_args()
    if args.ref_host:
        ref_host(args)
        return
    import torch

    for kind in args.scenes.split(","):
        if kind == "small":
            bench_scene(args, kind, torch.from_numpy(small_scene()).cuda(), stages=False)
        else:
            bench_scene(args, kind, scene_device(kind, int(200_000 * args.scale), 2500))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
