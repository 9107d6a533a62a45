#!/usr/bin/env python3
"""Generate tests/golden/ref_transient_goldens.npz by EXECUTING THE REFERENCE'S OWN transient-noise detectors
(clean/transient_noise/transient_fielding.py, transient_matecho.py and the dispatcher of clean/api.py) over
oracle/xr_shim.py.  Authoring machine only: needs the reference checkout.

The reference's modules are loaded as they are; what they ask of xarray beyond the shim is added here (oracle/ is not
edited): ``isel`` with a positional dict, ``transpose`` with an Ellipsis, ``rename`` to a name, ``~`` on a DataArray, and an ``apply_ufunc``
that takes inputs of different core dims and returns several outputs (the shim's takes one output and equal dims).
dask is not needed by what is executed: an empty ``dask.array`` stands in for the import in utils/compute.py.
scipy.ndimage is the real one.  clean/api.py imports far more than this package's fixtures can stand in for, so
``detect_transient`` is not imported: its definition is taken from the source by ast and executed.

THE DECISION MARGINS are read off the reference while it runs, not recomputed: the detectors' ``_log2lin`` /
``_lin2log`` and the ``np`` they call are wrapped to note every median, percentile, mean and sample count they produce;
from those, per ping, the smallest |quantity - threshold| over the comparisons the reference evaluated (the definition
in tests/transient_ref.py).  The generator asserts that NO fixture ping is closer to a threshold than that file's
MARGIN for its dtype, so the GPU tests compare whole masks.

Also stored: the reference's signatures, and what its Fielding core does with ``start > 0`` for both shapes.
Output = data only (seeded inputs on a 2^-8 dB grid, the reference's masks bit-packed, margins, exception types and
messages), written with fixed zip timestamps: two runs give the same bytes."""
import ast
import hashlib
import io
import json
import os
import sys
import types
import warnings
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import gen_ref_signatures  # noqa: E402
import xr_shim  # noqa: E402
from gen_goldens import REF, _load  # noqa: E402

import transient_ref as R  # noqa: E402  (MARGIN, and the margin definition the numbers below follow)

OUT = os.path.join(ROOT, "tests", "golden", "ref_transient_goldens.npz")
DA, DS = xr_shim.DataArray, xr_shim.Dataset
DIMS = ("channel", "ping_time", "range_sample")

LOG = []  # what the running detector produced, in order: (kind, value)


class _NumpyTap:
    """The ``np`` of a reference module: numpy itself, with the calls whose results decide a ping noted."""

    def __init__(self, names):
        self._names = names

    def __getattr__(self, name):
        f = getattr(np, name)
        if name not in self._names:
            return f

        def tapped(*a, **k):
            out = f(*a, **k)
            LOG.append((name, out))
            return out

        return tapped


def apply_ufunc(func, *das, input_core_dims, output_core_dims, vectorize=True, kwargs=None, **_):
    """xarray.apply_ufunc(vectorize=True) for the two detectors: loops over the dimensions of the first input that are
    not core dimensions; an input without a loop dimension is handed over whole."""
    first = das[0]
    loop = [d for d in first.dims if d not in input_core_dims[0]]
    shape = [first.sizes[d] for d in loop]
    outs = [[] for _ in output_core_dims]
    for idx in np.ndindex(*shape):
        args = []
        for da, core in zip(das, input_core_dims):
            sel = {d: i for d, i in zip(loop, idx) if d in da.dims}
            sub = da.isel(**sel) if sel else da
            args.append(np.asarray(sub.transpose(*core).values))
        LOG.append(("call", idx))
        res = func(*args, **(kwargs or {}))
        for o, r, core in zip(outs, res, output_core_dims):
            want = tuple(first.sizes[d] for d in core)
            if np.shape(r) != want:
                raise ValueError(f"apply_ufunc: the function returned shape {np.shape(r)} for core dimensions {core} of "
                                 f"sizes {want}")
            o.append(np.asarray(r))
    coords = {d: first.coords[d] for d in first.dims if d in first.coords}
    return tuple(DA(np.stack(o).reshape(shape + list(o[0].shape)) if loop else o[0],
                    {d: coords[d] for d in loop + list(core) if d in coords}, loop + list(core))
                 for o, core in zip(outs, output_core_dims))


def load_reference():
    xr = types.ModuleType("xarray")
    xr.DataArray, xr.Dataset, xr.apply_ufunc = DA, DS, apply_ufunc
    sys.modules["xarray"] = xr
    shim_isel, shim_transpose = DA.isel, DA.transpose

    def isel(self, indexers=None, **ix):
        return shim_isel(self, **{**(indexers or {}), **ix})

    def transpose(self, *dims):
        if Ellipsis in dims:
            at = dims.index(Ellipsis)
            named = [d for d in dims if d is not Ellipsis]
            dims = list(dims[:at]) + [d for d in self.dims if d not in named] + list(dims[at + 1:])
        return shim_transpose(self, *dims)

    shim_rename = DA.rename

    def rename(self, new):
        return DA(self.data, dict(self.coords), self.dims, new, self.attrs) if isinstance(new, str) else shim_rename(self, new)

    DA.isel, DA.transpose, DA.rename = isel, transpose, rename
    DA.__invert__ = lambda self: self._like(~self.data)
    dask = types.ModuleType("dask")
    dask.array = types.ModuleType("dask.array")
    dask.array.Array = type("Array", (), {})
    sys.modules["dask"], sys.modules["dask.array"] = dask, dask.array
    for n, p in [("echopype", [REF]), ("echopype.utils", [f"{REF}/utils"])]:
        m = types.ModuleType(n)
        m.__path__ = p
        sys.modules[n] = m
    _load("echopype.utils.compute", f"{REF}/utils/compute.py")
    td = f"{REF}/clean/transient_noise"
    fm = _load("ref_transient_fielding", f"{td}/transient_fielding.py")
    mm = _load("ref_transient_matecho", f"{td}/transient_matecho.py")
    for mod, names in ((fm, ()), (mm, ("min", "sum", "percentile"))):
        l2l, lin2log = mod._log2lin, mod._lin2log
        mod._log2lin = lambda x, f=l2l: (LOG.append(("lin", np.ndim(x))), f(x))[1]
        mod._lin2log = lambda x, f=lin2log: (lambda out: (LOG.append(("db", out)), out)[1])(f(x))
        mod.np = _NumpyTap(names)
    tree = ast.parse(open(f"{REF}/clean/api.py").read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "detect_transient")
    fn.returns = None
    for a in fn.args.args:
        a.annotation = None
    ns = {"METHODS_TRANSIENT": {"fielding": fm.transient_noise_fielding, "matecho": mm.transient_noise_matecho}}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "clean/api.py", "exec"), ns)
    return ns["detect_transient"], fm, mm


def reference_signatures():
    out = {}
    for file, name in (("clean/api.py", "detect_transient"),
                       ("clean/transient_noise/transient_fielding.py", "transient_noise_fielding"),
                       ("clean/transient_noise/transient_matecho.py", "transient_noise_matecho")):
        tree = ast.parse(open(os.path.join(REF, file)).read())
        fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
        out[name] = {"params": gen_ref_signatures.params(fn), "line": fn.lineno, "file": file}
    return json.dumps(out, sort_keys=True)


# ---- margins from the log of a run -----------------------------------------------------------------------------------
def _channels(log):
    out = []
    for ev in log:
        if ev[0] == "call":
            out.append([])
        else:
            out[-1].append(ev)
    return out


def fielding_margins(log, P, n, thr, maxts, computable):
    """computable: (C, P) bool, from the auxiliary mask the core returns.  A computable ping logs lin(1) db lin(1) db
    lin(2) db (median, 75th percentile, block median), then lin(1) db lin(2) db per walk step."""
    mar = np.full(computable.shape, np.inf)
    for c, evs in enumerate(_channels(log)):
        toks = []  # (ndim of the window, dB value)
        for a, b in zip(evs[0::2], evs[1::2]):
            assert a[0] == "lin" and b[0] == "db", (a, b)
            toks.append((a[1], float(b[1])))
        i = 0
        if not toks:  # (the core returned early: its auxiliary mask is all-False although it looked at no ping)
            continue
        for j in np.flatnonzero(computable[c]):
            assert [t[0] for t in toks[i:i + 3]] == [1, 1, 2], (c, j, toks[i:i + 3])
            pm, p75, bm = (t[1] for t in toks[i:i + 3])
            i += 3
            m = R._gap(p75, maxts)
            if p75 < maxts:
                m = min(m, R._gap(pm - bm, thr[0]))
            while i + 1 < len(toks) and toks[i][0] == 1 and toks[i + 1][0] == 2:  # (a next ping starts 1, 1)
                m = min(m, R._gap(toks[i][1] - toks[i + 1][1], thr[1]))
                i += 2
            mar[c, j] = m
        assert i == len(toks), (c, i, len(toks))
    return mar


def matecho_margins(log, rows, P, delta_db, min_window, extend_ping):
    """Per ping: np.min (the local bottom: every ping), then np.sum (samples in the window), np.percentile, and the
    mean in dB, each only if the ping got that far."""
    chans = _channels(log)
    mar = np.full((len(chans), P), np.inf)
    for c, evs in enumerate(chans):
        r = rows[c]
        j = -1
        pctl = None
        for kind, val in evs:
            if kind == "min":
                j += 1
                pctl = None
            elif kind == "sum":
                mar[c, j] = R._gap((r[1] - r[0]) * val, min_window)
            elif kind == "percentile":
                pctl = val
            elif kind == "db":
                mar[c, j] = min(mar[c, j], R._gap(val, pctl + delta_db))
        assert j == P - 1, (c, j, P)
        mar[c] = R.dilate(np.zeros(P, dtype=bool), mar[c], extend_ping)[1]
    return mar


# ---- scenes --------------------------------------------------------------------------------------------------------
def plane(P, S, seed, dtype, pings, nan_frac=0.01, base=-80.0):
    """Background ``base`` dB with a spread of 1.5 dB on a 2^-8 dB grid; ``pings``: {ping: (first row, gain in dB)}
    raised from that row to the end of the column."""
    rng = np.random.default_rng(seed)
    sv = base + 1.5 * rng.standard_normal((P, S))
    for j, (top, gain) in pings.items():
        sv[j, top:] += gain
    sv[rng.random((P, S)) < nan_frac] = np.nan
    return (np.round(sv * 256) / 256).astype(dtype)


def make_ds(sv, rows, rlayout="cps", bottom=None, bdims=None, var="Sv", range_var="depth"):
    """sv (C, P, S); rows (C, S) range rows; rlayout: "cps" (broadcast over pings), "s" (the 1-D vector of channel 0),
    "cp" (a variable without range_sample)."""
    C, P, S = sv.shape
    coords = {"channel": np.array([f"chan{c + 1}" for c in range(C)]), "ping_time": np.arange(P),
              "range_sample": np.arange(S)}
    ds = DS(coords=coords)
    ds[var] = DA(sv, coords, DIMS)
    if rlayout == "cps":
        ds[range_var] = DA(np.ascontiguousarray(np.broadcast_to(rows[:, None, :], (C, P, S))), coords, DIMS)
    elif rlayout == "s":
        ds[range_var] = DA(rows[0], {"range_sample": coords["range_sample"]}, ("range_sample",))
    else:
        ds[range_var] = DA(np.zeros((C, P), dtype=rows.dtype), {k: coords[k] for k in DIMS[:2]}, DIMS[:2])
    if bottom is not None:
        ds["bottom_depth"] = DA(bottom, {k: coords[k] for k in bdims}, bdims)
    return ds


def main():
    detect_transient, fm, mm = load_reference()
    g = {"signatures": np.array(reference_signatures())}
    cases = []

    def store(prefix, a):
        a = np.ascontiguousarray(a)
        key = prefix + hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()[:16]
        g[key] = a
        return key

    def case(tag, method, sv, rows, params, rlayout="cps", bottom=None, drop=None):
        sv = sv if sv.ndim == 3 else sv[None]
        rows = np.asarray(rows)
        rows = rows if rows.ndim == 2 else rows[None]
        C, P, S = sv.shape
        rec = {"tag": tag, "method": method, "params": dict(params), "rlayout": rlayout, "shape": [C, P, S],
               "dtype": sv.dtype.name, "sv": store("a_", sv), "rows": store("r_", rows)}
        bdims = None
        if bottom is not None:
            bottom = np.asarray(bottom, dtype=np.float64)
            bdims = DIMS[1:2] if bottom.ndim == 1 else DIMS[:2]
            rec["bottom"], rec["bottom_dims"] = store("b_", bottom), list(bdims)
        if drop:
            rec["drop"] = drop
        ds = make_ds(sv, rows, rlayout, bottom, bdims)
        if drop:
            ds._vars.pop(drop)
        call = dict(params)
        if "thr" in call:
            call["thr"] = tuple(call["thr"])
        del LOG[:]
        try:
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore", RuntimeWarning)
                out = detect_transient(ds, method, call)
            m = np.asarray(out.values)
            assert m.dtype == np.bool_ and m.shape == sv.shape and tuple(out.dims) == DIMS
            g[f"{tag}_out"] = np.packbits(m)
            rec["name"], rec["dims"], rec["attrs"] = out.name, list(out.dims), dict(out.attrs)
            rec["masked"] = int((~m).sum())
            rec["masked_pings"] = int((~m).any(axis=2).sum())
            p = {**DEFAULTS[method], **params}
            if method == "fielding":
                # the auxiliary mask is dropped by the wrapper: the core once more, silently, for the computable pings
                log = list(LOG)
                aux = np.stack([fm._fielding_core_numpy(sv[c], rows[0 if rlayout == "s" else c], p["r0"], p["r1"], p["n"],
                                                        p["thr"], p["roff"], p["jumps"], p["maxts"], p["start"])[1][:, 0]
                                for c in range(C)]) if S else np.ones((C, P), dtype=bool)
                mar = fielding_margins(log, P, p["n"], p["thr"], p["maxts"], ~aux)
            else:
                mar = matecho_margins(LOG, rows, P, p["delta_db"], p["min_window"], p["extend_ping"])
            fin = mar[np.isfinite(mar)]
            assert fin.size == 0 or fin.min() >= R.MARGIN[sv.dtype.name], (tag, fin.min())
            g[f"{tag}_margin"] = mar
            rec["min_margin"] = float(fin.min()) if fin.size else None
        except AssertionError:
            raise
        except Exception as e:  # noqa: BLE001 -- recorded: the tests expect the same type and message
            rec["error"] = [type(e).__name__, str(e)]
        cases.append(rec)
        return rec

    F = {"var_name": "Sv", "range_var": "depth"}
    # ---- fielding: 2.5 m grid, 160 samples; layer 300-350 m = rows [120, 140), steps of 5 rows, stop row 20
    P, S = 40, 160
    r25 = 2.5 * np.arange(S)
    el = {3: (60, 10.0), 5: (60, 10.0), 12: (60, 10.0), 20: (100, 8.0), 27: (120, 9.0), 30: (10, 12.0), 34: (60, 10.0),
          37: (60, 10.0)}
    fp = dict(F, r0=300, r1=350, n=5, thr=(3.01, 1.01), roff=50, jumps=12.5)
    for dt in (np.float64, np.float32):
        sfx = "_f32" if dt == np.float32 else ""
        sv = plane(P, S, 1, dt, el)
        case("f_basic" + sfx, "fielding", sv, r25.astype(dt), fp)
        case("f_odd_layer" + sfx, "fielding", sv, r25.astype(dt), dict(fp, r1=347.5))
        case("f_n0" + sfx, "fielding", sv, r25.astype(dt), dict(fp, n=0))
        case("f_n1" + sfx, "fielding", sv, r25.astype(dt), dict(fp, n=1))
    sv64 = plane(P, S, 1, np.float64, el)
    case("f_range_1d", "fielding", sv64, r25, fp, rlayout="s")
    case("f_up_ge_lw", "fielding", sv64, r25, dict(fp, r1=300.5))
    case("f_r0_gt_r1", "fielding", sv64, r25, dict(fp, r0=350, r1=300))
    case("f_below_data", "fielding", sv64, r25, dict(fp, r0=500, r1=600))
    case("f_above_data", "fielding", sv64, r25, dict(fp, r0=-20, r1=-10))
    tail = r25.copy()
    tail[150:] = np.nan
    case("f_nan_tail", "fielding", sv64, tail, fp)
    holes = sv64.copy()
    holes[12, 120:140] = np.nan   # ping 12: its layer all NaN -> uncomputable although raised
    holes[19, :] = np.nan         # an all-NaN ping inside the block of ping 20 (and uncomputable itself)
    case("f_allnan_layer_and_ping", "fielding", holes, r25, fp)
    # a short layer (6 and 7 samples: the 75th percentile interpolates between two of them) and maxts BETWEEN those two
    # values for some raised pings: the interpolation in the linear domain decides p75 < maxts, both ways
    many = {j: (60, 10.0) for j in range(6, 74, 4)}  # (2 or 3 of the 10 pings of a block: its median stays quiet)
    for dt in (np.float64, np.float32):
        svp = plane(80, S, 6, dt, many, nan_frac=0.0)
        for r1_, name in ((315, "f_p75_across_maxts"), (317.5, "f_p75_across_maxts_7")):
            found = None
            for maxts in np.arange(-71.505, -67.5, 0.01):
                prm = dict(fp, r1=r1_, maxts=float(round(maxts, 3)))
                kw = {k: prm[k] for k in ("r0", "r1", "n", "thr", "roff", "jumps", "maxts")}
                br, _ = R.fielding_p75_bracket(svp, r25, **kw)
                valid, mar = R.fielding(svp, r25.astype(dt), **kw)
                hit = ~valid.all(axis=1)
                loud = ~R.fielding(svp, r25.astype(dt), **dict(kw, maxts=0.0))[0].all(axis=1)  # passes thr[0]
                br &= loud
                if (br & hit).any() and (br & ~hit).any() and mar.min() >= 10 * R.MARGIN[np.dtype(dt).name]:
                    found = prm
                    break
            assert found is not None, name
            rec = case(name + ("_f32" if dt == np.float32 else ""), "fielding", svp, r25.astype(dt), found)
            rec["bracket_pings"] = np.flatnonzero(br).tolist()
    case("f_defaults_no_layer", "fielding", sv64, r25, F)  # the default 900-1000 m layer lies below these 397.5 m
    # the negative-start walk: 400 rows of 2.5 m, up = 360, jumps = 950 m -> sf = 380, r0_ = -20
    neg = plane(24, 400, 2, np.float64, {8: (300, 10.0), 15: (200, 12.0)})
    case("f_negative_start", "fielding", neg, 2.5 * np.arange(400), dict(F, r0=900, r1=950, n=3, thr=(3.01, 1.01),
                                                                         roff=20, jumps=950))
    case("f_step_beyond_column", "fielding", neg, 2.5 * np.arange(400),
         dict(F, r0=900, r1=950, n=3, thr=(3.01, 1.01), roff=20, jumps=2500))
    # three channels, three range rows
    for dt in (np.float64, np.float32):
        sv3 = np.stack([plane(P, S, 10 + c, dt, el) for c in range(3)])
        r3 = np.stack([dz * np.arange(S) for dz in (2.5, 2.0, 3.0)]).astype(dt)
        case("f_three_channels" + ("_f32" if dt == np.float32 else ""), "fielding", sv3, r3,
             dict(fp, r0=250, r1=300, roff=40, jumps=10))
    # ---- fielding: what raises
    case("x_method", "ryan", sv64, r25, F)
    case("x_f_var_name", "fielding", sv64, r25, dict(F, var_name="Sv_corrected"))
    case("x_f_range_var", "fielding", sv64, r25, F, drop="depth")
    case("x_f_cannot_infer", "fielding", sv64, r25, F, rlayout="cp")
    case("x_f_dr_zero", "fielding", sv64, np.full(S, 320.0), fp)
    alt = r25.copy()
    alt[1::2] = np.nan
    case("x_f_dr_nan", "fielding", sv64[:, :159], alt[:159], fp)
    # start > 0: the reference's core on both shapes (S > P - start: vstack fails; otherwise P + start rows)
    starts = {}
    for tag, (p_, s_) in (("tall", (12, 30)), ("wide", (40, 8))):
        a = plane(p_, s_, 3, np.float64, {})
        try:
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore", RuntimeWarning)
                bad, _ = fm._fielding_core_numpy(a, 2.5 * np.arange(s_), 5, 15, 2, (3, 1), 0, 5, -35, start=4)
            starts[tag] = {"P": p_, "S": s_, "start": 4, "rows": int(bad.shape[0])}
        except Exception as e:  # noqa: BLE001
            starts[tag] = {"P": p_, "S": s_, "start": 4, "error": [type(e).__name__, str(e)[:80]]}
    g["fielding_start"] = np.array(json.dumps(starts, sort_keys=True))

    # ---- matecho: window 100-300 m = rows [40, 120], 10-ping windows
    M = {"var_name": "Sv", "range_var": "depth"}
    mp = dict(M, start_depth=100, window_meter=200, window_ping=10, delta_db=6.01, min_window=20)
    em = {0: (20, 10.0), 7: (20, 9.0), 20: (60, 14.0), 21: (20, 3.0), 39: (20, 10.0)}
    for dt in (np.float64, np.float32):
        sfx = "_f32" if dt == np.float32 else ""
        sv = plane(P, S, 4, dt, em)
        r = r25.astype(dt)
        case("m_basic" + sfx, "matecho", sv, r, mp)
        case("m_extend" + sfx, "matecho", sv, r, dict(mp, extend_ping=2))
        case("m_odd_window" + sfx, "matecho", sv, r, dict(mp, window_ping=7, percentile=40))
        slope = np.linspace(330.0, 180.0, P)
        case("m_bottom_slope" + sfx, "matecho", sv, r, dict(mp, bottom_var="bottom_depth"), bottom=slope)
    svm = plane(P, S, 4, np.float64, em)
    case("m_window_ping_1", "matecho", svm, r25, dict(mp, window_ping=1))
    case("m_window_ping_2", "matecho", svm, r25, dict(mp, window_ping=2))
    case("m_time_var_given", "matecho", svm, r25, dict(mp, time_var="ping_time"))
    case("m_bottom_none_named", "matecho", svm, r25, dict(mp, bottom_var="no_such_variable"))
    case("m_bottom_cuts", "matecho", svm, r25, dict(mp, bottom_var="bottom_depth"), bottom=np.full(P, 250.0))
    case("m_bottom_removes", "matecho", svm, r25, dict(mp, bottom_var="bottom_depth"), bottom=np.full(P, 90.0))
    case("m_bottom_min_window", "matecho", svm, r25, dict(mp, bottom_var="bottom_depth"), bottom=np.full(P, 110.0))
    bn = np.full(P, 250.0)
    bn[::3] = np.nan
    bn[15:32] = np.nan
    case("m_bottom_nan", "matecho", svm, r25, dict(mp, bottom_var="bottom_depth"), bottom=bn)
    case("m_window_outside", "matecho", svm, r25, dict(mp, start_depth=1000))
    case("m_defaults", "matecho", svm, r25, M)
    case("m_nan_tail", "matecho", svm, tail, mp)
    case("m_nan_tail_bottom", "matecho", svm, tail, dict(mp, bottom_var="bottom_depth"), bottom=np.full(P, 280.0))
    allnan = svm.copy()
    allnan[7, :] = np.nan
    allnan[:, 40:121][10:14] = np.nan
    case("m_allnan_ping", "matecho", allnan, r25, mp)
    for dt in (np.float64, np.float32):
        sv3 = np.stack([plane(P, S, 20 + c, dt, em) for c in range(3)])
        r3 = np.stack([dz * np.arange(S) for dz in (2.5, 2.0, 3.0)]).astype(dt)
        sfx = "_f32" if dt == np.float32 else ""
        case("m_three_channels" + sfx, "matecho", sv3, r3, mp)
        b3 = np.stack([np.full(P, 250.0), np.linspace(150.0, 320.0, P), np.full(P, np.nan)])
        case("m_bottom_per_channel" + sfx, "matecho", sv3, r3, dict(mp, bottom_var="bottom_depth"), bottom=b3)
    # the float32 limits: a 0.19 m grid in float32; start_depth a hair (in float64) above sample 40 -- rounded to
    # float32 it IS sample 40, which NumPy's comparison then includes; min_window sits between the heights with and
    # without that sample, so pings are flagged only if it was counted
    s32 = plane(P, S, 5, np.float32, em)
    r32 = (np.float32(0.19) * np.arange(S, dtype=np.float32)).astype(np.float32)
    dz = float(r32[1] - r32[0])
    lim = float(r32[40]) + 1e-9
    n_with = int(((r32 >= np.float32(lim)) & (r32 <= np.float32(lim + 12.0))).sum())
    case("m_f32_start_limit", "matecho", s32, r32, dict(M, start_depth=lim, window_meter=12.0, window_ping=10,
                                                        delta_db=6.01, min_window=dz * (n_with - 0.5)))
    # ... and the bottom, an np.float64 scalar: compared in float64, so a bottom a hair above sample 100 keeps it
    n_b = 100 - 40 + 1
    case("m_f32_bottom_limit", "matecho", s32, r32,
         dict(M, start_depth=float(r32[40]), window_meter=20.0, window_ping=10, delta_db=6.01,
              min_window=dz * (n_b - 0.5), bottom_var="bottom_depth"), bottom=np.full(P, float(r32[100]) + 1e-9))
    # a SMALL window (4 pings x 5 samples of a 10 m grid): the gap between two neighbouring order statistics is
    # decibels wide, the threshold mean_db - delta_db falls inside it for many pings, and the percentile itself --
    # selected and interpolated in dB -- decides.  delta_db is searched so that the case holds such pings with both
    # outcomes; the host test asserts from the oracle's replay of the device's counting sweep that they are there.
    r10 = 10.0 * np.arange(12)
    for dt in (np.float64, np.float32):
        svs = plane(60, 12, 7, dt, {}, nan_frac=0.02)
        for pct, name in ((25, "m_small_window_t75"), (22, "m_small_window_t18")):
            found = None
            for delta in np.arange(0.205, 3.0, 0.05):
                prm = dict(M, start_depth=30, window_meter=40, window_ping=4, percentile=pct,
                           delta_db=float(round(delta, 3)), min_window=5)
                kw = {k: prm[k] for k in ("start_depth", "window_meter", "window_ping", "percentile", "delta_db",
                                          "min_window")}
                route, frac = R.matecho_route(svs, r10.astype(dt), **kw)
                valid, mar = R.matecho(svs, r10.astype(dt), **kw)
                sel = route == 3
                if (sel & ~valid).sum() >= 2 and (sel & valid).sum() >= 2 and mar.min() >= 10 * R.MARGIN[np.dtype(dt).name]:
                    found = prm
                    break
            assert found is not None, name
            rec = case(name + ("_f32" if dt == np.float32 else ""), "matecho", svs, r10.astype(dt), found)
            rec["select_pings"] = np.flatnonzero(sel).tolist()
    # percentile outside [0, 100]: np.percentile raises when a ping reaches it ...
    case("x_m_percentile", "matecho", svm, r25, dict(mp, percentile=101))
    # ... and only then: with no ping that far (the window outside the data) the reference returns all-True.  This
    # package refuses the argument before any launch ("diverges": the tests expect its ValueError there)
    case("m_percentile_unreached", "matecho", svm, r25, dict(mp, percentile=101, start_depth=1000))["diverges"] = \
        ["ValueError", "Percentiles must be in the range [0, 100]"]
    # ---- matecho: what raises
    case("x_m_var_name", "matecho", svm, r25, dict(M, var_name="Sv_corrected"))
    case("x_m_range_var", "matecho", svm, r25, M, drop="depth")
    case("x_m_time_var", "matecho", svm, r25, dict(M, time_var="time1"))

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
    for c in cases:
        print(f"{c['tag']:28s}", c.get("error") or (c["masked_pings"], c["masked"], c["min_margin"]))
    print(json.dumps(starts))
    print(OUT, os.path.getsize(OUT), "bytes,", len(cases), "cases")


DEFAULTS = {
    "fielding": dict(r0=900, r1=1000, n=30, thr=(3, 1), roff=20, jumps=5, maxts=-35, start=0),
    "matecho": dict(start_depth=220, window_meter=450, window_ping=100, percentile=25, delta_db=12, extend_ping=0,
                    min_window=20),
}

if __name__ == "__main__":
    main()
