#!/usr/bin/env python3
"""Generate tests/golden/ref_shoal_goldens.npz by EXECUTING THE REFERENCE'S OWN shoal detectors
(mask/shoal_detection/shoal_weill.py, shoal_echoview.py and the dispatcher's check of mask/api.py) over
oracle/xr_shim.py.  Authoring machine only: needs the reference checkout.

The reference's modules are loaded as they are; what they ask of xarray beyond the shim is added here (oracle/ is not
edited): a scalar ``sel`` (drops the dimension).  scipy.ndimage and pandas are the real ones.  mask/api.py imports far
more than this package's fixtures can stand in for, so ``detect_shoal`` itself is not imported: its definition is taken
from the source by ast (the function alone, compiled against the two loaded detectors) and executed.

Also stored: the reference's signatures of detect_shoal, shoal_weill and shoal_echoview (ast of its sources).
Output = data only (seeded inputs, the reference's masks bit-packed, attributes, exception types and messages),
written with fixed zip timestamps: two runs give the same bytes."""
import ast
import hashlib
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import gen_ref_signatures  # noqa: E402
import xr_shim  # noqa: E402
from gen_goldens import REF, _load  # noqa: E402

from echopype_amd.synth import shoal_scene as _scene  # noqa: E402  (numpy only)

OUT = os.path.join(ROOT, "tests", "golden", "ref_shoal_goldens.npz")
DA, DS = xr_shim.DataArray, xr_shim.Dataset
DIMS = ("channel", "ping_time", "range_sample")


def scene(*a, **k):
    """synth.shoal_scene on a 2^-8 grid: the fixture compresses (a threshold needs no more precision)."""
    sv = _scene(*a, **k)
    return (np.round(sv.astype(np.float64) * 256) / 256).astype(sv.dtype)


def load_reference_shoal():
    xr = types.ModuleType("xarray")
    xr.DataArray, xr.Dataset = DA, DS
    sys.modules["xarray"] = xr
    shim_sel = DA.sel

    def sel(self, drop=False, **ix):
        scalar = {d: v for d, v in ix.items() if not isinstance(v, slice) and np.ndim(v) == 0}
        if not scalar:
            return shim_sel(self, drop=drop, **ix)
        pos = {}
        for d, v in scalar.items():
            hit = np.flatnonzero(np.asarray(self.coords[d]).astype(str) == str(v))
            if hit.size == 0:
                raise KeyError(v)
            pos[d] = int(hit[0])
        return self.isel(**pos)

    DA.sel = sel
    sd = f"{REF}/mask/shoal_detection"
    weill = _load("ref_shoal_weill", f"{sd}/shoal_weill.py").shoal_weill
    echoview = _load("ref_shoal_echoview", f"{sd}/shoal_echoview.py").shoal_echoview
    # detect_shoal: the dispatcher alone, cut out of mask/api.py
    tree = ast.parse(open(f"{REF}/mask/api.py").read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "detect_shoal")
    fn.returns = None
    for a in fn.args.args:
        a.annotation = None
    ns = {"METHODS_SHOAL": {"echoview": echoview, "weill": weill}}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "mask/api.py", "exec"), ns)
    return ns["detect_shoal"]


def reference_signatures():
    out = {}
    for file, name in (("mask/api.py", "detect_shoal"),
                       ("mask/shoal_detection/shoal_weill.py", "shoal_weill"),
                       ("mask/shoal_detection/shoal_echoview.py", "shoal_echoview")):
        tree = ast.parse(open(os.path.join(REF, file)).read())
        fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
        out[name] = {"params": gen_ref_signatures.params(fn), "line": fn.lineno, "file": file}
    return json.dumps(out, sort_keys=True)


def make_ds(sv, var="Sv", channel="chan1", layout="cps"):
    """layout: "cps" (channel, ping_time, range_sample), "ps" (no channel dimension), "p" / "s" (only that core
    dimension present: the plane's other axis is called "beam")."""
    P, S = sv.shape
    coords = {"channel": np.array([channel]), "ping_time": np.arange(P), "range_sample": np.arange(S),
              "beam": np.arange(S if layout == "p" else P)}
    dims = {"cps": DIMS, "ps": DIMS[1:], "p": ("channel", "ping_time", "beam"),
            "s": ("channel", "beam", "range_sample")}[layout]
    ds = DS(coords={k: coords[k] for k in DIMS})
    ds[var] = DA(sv if layout == "ps" else sv[None], {d: coords[d] for d in dims}, dims)
    return ds


def rect_plane(P, S, rects, dtype=np.float64, lo=-90.0, hi=-50.0):
    """Background ``lo`` with rectangles (p0, p1, s0, s1), ends included, at ``hi``."""
    sv = np.full((P, S), lo, dtype=dtype)
    for p0, p1, s0, s1 in rects:
        sv[p0:p1 + 1, s0:s1 + 1] = hi
    return sv


def uni(n, step=1.0):
    return np.arange(n + 1) * step


def main():
    detect_shoal = load_reference_shoal()
    g = {"signatures": np.array(reference_signatures())}
    cases = []

    def case(tag, method, sv, params, layout="cps", axes=None):
        """Run the reference on ``sv`` (P, S); store input, params and the mask (bit-packed) or the exception."""
        rec = {"tag": tag, "method": method, "params": dict(params), "layout": layout, "shape": list(sv.shape)}
        sv = np.ascontiguousarray(sv)
        key = "a_" + hashlib.sha256(sv.dtype.str.encode() + str(sv.shape).encode() + sv.tobytes()).hexdigest()[:16]
        g[key] = sv  # each distinct plane stored once
        rec["sv"] = key
        call = dict(params)
        if axes is not None:
            for name, a in zip(("idim", "jdim"), axes):
                a = np.asarray(a, dtype=np.float64)
                k = "x_" + hashlib.sha256(a.tobytes()).hexdigest()[:16]
                g[k] = a
                rec[name] = k
                call[name] = a
        for k in ("mincan", "maxlink", "minsho"):
            if k in call:
                call[k] = tuple(call[k])
        try:
            out = detect_shoal(make_ds(sv, layout=layout), method, call)
            m = np.asarray(out.values)
            assert m.dtype == np.bool_ and m.shape == sv.shape
            g[f"{tag}_out"] = np.packbits(m)
            rec["attrs"] = {k: v for k, v in out.attrs.items()}
            rec["name"], rec["dims"], rec["count"] = out.name, list(out.dims), int(m.sum())
        except Exception as e:  # noqa: BLE001 -- recorded: the tests expect the same type and message
            rec["error"] = [type(e).__name__, str(e)]
        cases.append(rec)

    W = {"var_name": "Sv", "channel": "chan1"}

    # ---- weill: scenes
    sc64 = scene(P=90, S=120, seed=1)
    sc32 = scene(P=70, S=130, seed=2, dtype=np.float32)
    case("w_default", "weill", sc64, W)
    case("w_default_f32", "weill", sc32, W)
    case("w_zeros", "weill", sc64, dict(W, maxvgap=0, maxhgap=0, minvlen=0, minhlen=0))
    case("w_all", "weill", sc64, dict(W, thr=-68.0, maxvgap=3, maxhgap=2, minvlen=4, minhlen=3))
    case("w_all_f32", "weill", sc32, dict(W, thr=-68.0, maxvgap=3, maxhgap=2, minvlen=4, minhlen=3))
    case("w_hgap_only", "weill", sc64, dict(W, maxvgap=0, maxhgap=4))
    case("w_len_only", "weill", sc64, dict(W, maxvgap=0, minvlen=3, minhlen=2))
    case("w_minv_only", "weill", sc32, dict(W, minvlen=6))
    case("w_minh_only", "weill", sc32, dict(W, minhlen=5))
    case("w_wide_gaps", "weill", scene(P=140, S=70, seed=3), dict(W, maxvgap=70, maxhgap=140, minvlen=2, minhlen=2))
    case("w_float_params", "weill", sc64, dict(W, maxvgap=2.5, maxhgap=1.5, minvlen=2.5, minhlen=1.5))
    # gaps of known length: 4 samples (vertical) at pings 2..5, 3 pings (horizontal) at samples 20..23
    gaps = rect_plane(12, 40, [(2, 5, 3, 6), (2, 5, 11, 14), (0, 2, 20, 23), (6, 9, 20, 23)])
    for v in (3, 4, 5):
        case(f"w_vgap_{v}", "weill", gaps, dict(W, maxvgap=v, maxhgap=0))
    for h in (2, 3, 4):
        case(f"w_hgap_{h}", "weill", gaps, dict(W, maxvgap=0, maxhgap=h))
    # gaps that touch each of the four borders stay, whatever the limits
    edge = np.full((10, 12), -50.0)
    edge[3, 0:3] = -90.0     # touches sample 0
    edge[5, 9:12] = -90.0    # touches sample S-1
    edge[0:2, 5] = -90.0     # touches ping 0
    edge[8:10, 7] = -90.0    # touches ping P-1
    edge[4:6, 4] = -90.0     # interior: filled
    case("w_borders", "weill", edge, dict(W, maxvgap=9, maxhgap=9))
    case("w_borders_v", "weill", edge, dict(W, maxvgap=9, maxhgap=0))
    case("w_borders_h", "weill", edge, dict(W, maxvgap=0, maxhgap=9))
    # runs longer than one 64-sample step, and runs that close across the steps' seams
    long = np.full((3, 200), -90.0)
    long[0, [10, 150]] = -50.0
    long[1, [63, 64, 130]] = -50.0
    long[2, [0, 127, 199]] = -50.0
    for v in (64, 65, 70, 71, 126, 138, 139, 200):
        case(f"w_long_{v}", "weill", long, dict(W, maxvgap=v))
    case("w_none", "weill", np.full((7, 9), -90.0), dict(W, maxvgap=3, maxhgap=3, minvlen=1, minhlen=1))
    case("w_full", "weill", np.full((7, 9), -50.0), dict(W, maxvgap=3, maxhgap=3, minvlen=9, minhlen=7))
    case("w_full_removed", "weill", np.full((7, 9), -50.0), dict(W, minvlen=10))
    case("w_allnan", "weill", np.full((5, 6), np.nan), W)
    case("w_one_ping", "weill", sc64[:1], dict(W, maxvgap=3, maxhgap=3, minvlen=2))
    case("w_one_sample", "weill", sc64[:, 17:18], dict(W, maxvgap=3, maxhgap=3, minhlen=2))
    case("w_one_pixel", "weill", np.array([[-50.0]]), dict(W, minvlen=1, minhlen=1))
    # a threshold float32 cannot hold: -70.1 rounds to -70.09999847...; samples on either side of the rounding
    t32 = np.float32(-70.1)
    near = np.array([[np.nextafter(t32, np.float32(-80)), t32, np.nextafter(t32, np.float32(0)), -70.125, -70.0625]],
                    dtype=np.float32)
    case("w_thr_f32", "weill", np.tile(near, (3, 1)), dict(W, thr=-70.1, maxvgap=0))
    case("w_thr_f64", "weill", np.tile(near.astype(np.float64), (3, 1)), dict(W, thr=-70.1, maxvgap=0))
    case("w_no_channel_dim", "weill", sc64, {"var_name": "Sv", "thr": -68.0, "maxvgap": 2, "minvlen": 3}, layout="ps")
    case("w_no_channel_dim_named", "weill", sc64, dict(W, minvlen=3), layout="ps")
    # diagonal-only checkerboard: one component per pixel under 4-connectivity
    chk = np.where((np.add.outer(np.arange(9), np.arange(11)) % 2) == 0, -50.0, -90.0)
    case("w_checker", "weill", chk, dict(W, maxvgap=0, minvlen=2))
    case("w_checker_keep", "weill", chk, dict(W, maxvgap=0, minvlen=1, minhlen=1))

    # ---- echoview
    E = {"var_name": "Sv", "channel": "chan1"}
    P, S = sc64.shape
    ax64 = (uni(S), uni(P))
    case("e_default", "echoview", sc64, E, axes=ax64)
    case("e_default_f32", "echoview", sc32, E, axes=(uni(sc32.shape[1]), uni(sc32.shape[0])))
    case("e_zeros", "echoview", sc64, dict(E, mincan=(0.0, 0.0), maxlink=(0.0, 0.0), minsho=(0.0, 0.0)), axes=ax64)
    case("e_metres", "echoview", sc64, dict(E, thr=-68.0, mincan=(1.0, 4.0), maxlink=(2.0, 6.0), minsho=(4.0, 12.0)),
         axes=(uni(S, 0.5), uni(P, 2.0)))
    rng = np.random.default_rng(7)
    irr = (np.concatenate([[0.0], np.cumsum(rng.uniform(0.2, 1.5, S))]),
           np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 4.0, P))]))
    case("e_irregular", "echoview", sc64, dict(E, mincan=(1.5, 3.0), maxlink=(2.0, 5.0), minsho=(3.0, 9.0)), axes=irr)
    case("e_irregular_f32", "echoview", sc32,
         dict(E, mincan=(1.5, 3.0), maxlink=(2.0, 5.0), minsho=(3.0, 9.0)),
         axes=(np.concatenate([[0.0], np.cumsum(rng.uniform(0.2, 1.5, sc32.shape[1]))]),
               np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 4.0, sc32.shape[0]))])))
    rep = np.repeat(np.arange(P // 3 + 2) * 3.0, 3)[:P + 1]  # every ping edge three times: zero-width pings
    case("e_repeated_jdim", "echoview", sc64, dict(E, mincan=(1.0, 3.0), maxlink=(1.0, 2.0), minsho=(2.0, 6.0)),
         axes=(uni(S), rep))
    case("e_repeated_jdim_neg", "echoview", sc64, dict(E, mincan=(1.0, 0.0), maxlink=(0.0, -1.0), minsho=(2.0, 6.0)),
         axes=(uni(S), rep))
    for ml in ((-1.0, -1.0), (-3.0, -2.0), (-1.5, 0.0), (0.0, 0.0)):
        case(f"e_maxlink_{ml[0]}_{ml[1]}", "echoview", sc64,
             dict(E, mincan=(1.0, 1.0), maxlink=ml, minsho=(4.0, 4.0)), axes=ax64)
    # three 2 x 2 squares in a row along pings, 4 background pings apart: the outer two meet only through the middle
    three = rect_plane(24, 12, [(2, 3, 5, 6), (8, 9, 5, 6), (14, 15, 5, 6)])
    ax3 = (uni(12), uni(24))
    for link, tag in (((0.0, 3.0), "short"), ((0.0, 4.0), "chain"), ((0.0, 10.0), "direct")):
        case(f"e_three_{tag}", "echoview", three, dict(E, mincan=(1.0, 1.0), maxlink=link, minsho=(1.0, 10.0)),
             axes=ax3)
    # two L shapes whose bounding boxes overlap in a corner that holds pixels of neither: boxes that meet are no link
    ell = rect_plane(30, 30, [(4, 16, 4, 4), (4, 4, 4, 16), (12, 24, 24, 24), (24, 24, 12, 24)])
    case("e_ell_bbox_only", "echoview", ell, dict(E, mincan=(1.0, 1.0), maxlink=(-1.0, -1.0), minsho=(14.0, 14.0)),
         axes=(uni(30), uni(30)))
    case("e_ell_linked", "echoview", ell, dict(E, mincan=(1.0, 1.0), maxlink=(8.0, 8.0), minsho=(14.0, 14.0)),
         axes=(uni(30), uni(30)))
    # a ring with a small square in its hole: inside the ring's box, linked by its pixels
    ring = rect_plane(30, 30, [(4, 5, 4, 24), (23, 24, 4, 24), (4, 24, 4, 5), (4, 24, 23, 24), (14, 15, 14, 15)])
    case("e_ring_bbox_only", "echoview", ring, dict(E, mincan=(1.0, 1.0), maxlink=(-1.0, -1.0), minsho=(5.0, 5.0)),
         axes=(uni(30), uni(30)))
    case("e_ring_linked", "echoview", ring, dict(E, mincan=(1.0, 1.0), maxlink=(8.0, 8.0), minsho=(5.0, 5.0)),
         axes=(uni(30), uni(30)))
    # a tie in an argmin: the target falls midway between two edges (maxlink + 1 = 1.5 on a unit grid): first index
    tie = rect_plane(20, 20, [(5, 6, 5, 6), (9, 10, 5, 6), (5, 6, 9, 10)])
    case("e_tie", "echoview", tie, dict(E, mincan=(1.0, 1.0), maxlink=(0.5, 0.5), minsho=(1.0, 5.0)),
         axes=(uni(20), uni(20)))
    case("e_tie_wider", "echoview", tie, dict(E, mincan=(1.0, 1.0), maxlink=(1.5, 1.5), minsho=(1.0, 5.0)),
         axes=(uni(20), uni(20)))
    # diagonal-only checkerboard: one component under 8-connectivity
    case("e_checker", "echoview", chk, dict(E, mincan=(9.0, 9.0), maxlink=(0.0, 0.0), minsho=(11.0, 9.0)),
         axes=(uni(11), uni(9)))
    case("e_checker_removed", "echoview", chk, dict(E, mincan=(9.0, 9.0), maxlink=(0.0, 0.0), minsho=(11.5, 9.0)),
         axes=(uni(11), uni(9)))
    case("e_none", "echoview", np.full((7, 9), -90.0), E, axes=(uni(9), uni(7)))
    case("e_full", "echoview", np.full((7, 9), -50.0), dict(E, mincan=(9.0, 7.0), minsho=(9.0, 7.0)),
         axes=(uni(9), uni(7)))
    case("e_full_removed", "echoview", np.full((7, 9), -50.0), dict(E, mincan=(9.0, 7.0), minsho=(9.5, 7.0)),
         axes=(uni(9), uni(7)))
    case("e_one_ping", "echoview", sc64[:1], dict(E, mincan=(2.0, 1.0), maxlink=(2.0, 1.0), minsho=(4.0, 1.0)),
         axes=(uni(S), uni(1)))
    case("e_one_sample", "echoview", sc64[:, 17:18], dict(E, mincan=(1.0, 2.0), maxlink=(1.0, 2.0), minsho=(1.0, 4.0)),
         axes=(uni(1), uni(P)))
    case("e_thr_f32", "echoview", np.tile(near, (3, 1)),
         dict(E, thr=-70.1, mincan=(0.0, 0.0), maxlink=(0.0, 0.0), minsho=(0.0, 0.0)), axes=(uni(5), uni(3)))
    case("e_no_channel_dim", "echoview", sc64, dict(E, channel=None), layout="ps", axes=ax64)

    # ---- host checks
    small = sc64[:6, :8]
    axs = (uni(8), uni(6))
    case("x_method", "otsu", small, W)
    case("x_w_var_name", "weill", small, dict(W, var_name="Sv_corrected"))
    case("x_w_channel_none", "weill", small, {"var_name": "Sv"})
    case("x_w_no_ping_time", "weill", small, W, layout="s")
    case("x_w_no_range_sample", "weill", small, W, layout="p")
    case("x_e_var_name", "echoview", small, dict(E, var_name="Sv_corrected"), axes=axs)
    case("x_e_channel_none", "echoview", small, dict(E, channel=None), axes=axs)
    bad = axs[0].copy()
    bad[3] = np.nan
    case("x_e_idim_nan", "echoview", small, E, axes=(bad, axs[1]))
    bad = axs[1].copy()
    bad[0] = np.nan
    case("x_e_jdim_nan", "echoview", small, E, axes=(axs[0], bad))

    g["cases"] = np.array(json.dumps(cases, sort_keys=True, default=float))
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(g):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(g[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, b.getvalue())
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
