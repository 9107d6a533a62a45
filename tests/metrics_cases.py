"""Inputs of the metrics tests: seeded (Sv, range) pairs of every content the statistics treat differently.  All values
are float32 numbers, so the float64 cases are the same values upcast and a fixture stores float32 only."""
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_metrics_goldens.npz")
STATS = ("abundance", "center_of_mass", "dispersion", "evenness", "aggregation")


def load_fixture():
    """(cases, known, arrays) of tests/golden/ref_metrics_goldens.npz (scripts/gen_metrics_goldens.py): what the
    reference's own functions returned.  A case's inputs are ``arrays[f"{tag}/in/{name}"]`` (float32, range_sample
    last), its results ``arrays[f"{tag}/{f64|f32}/{function}"]`` or ``case["results"][f"{f64|f32}/{function}"]`` =
    [exception type, message]."""
    z = np.load(GOLDEN)
    return json.loads(z["cases"].item()), json.loads(z["known"].item()), z


def case_inputs(z, case, dtype):
    return {k: z[f"{case['tag']}/in/{k}"].astype(dtype) for k in case["inputs"]}


KINDS = ("clean", "nan_tail", "sv_holes", "range_nan", "repeats", "neg_inf", "all_neg_inf", "decreasing", "shared")


def make(kind, shape, S, dtype=np.float32, seed=0):
    """(Sv of shape + (S,), range of the same shape -- or (S,) for "shared") of ``dtype``.

    clean        increasing range (steps 0.1 .. 0.3 m from 2 .. 50 m), Sv in -90 .. -30 dB
    nan_tail     row i keeps its first i mod (S + 1) samples (0, 1, 2, ... valid samples), NaN in both arrays after them
    sv_holes     NaN in a tenth of Sv
    range_nan    one NaN in the middle of every range row: two dz are lost
    repeats      range values repeated (dz = 0) at every fifth sample
    neg_inf      -inf in a tenth of Sv
    all_neg_inf  every third row of Sv is -inf throughout
    decreasing   the range runs backwards: A < 0, abundance NaN
    shared       one range row for all"""
    assert kind in KINDS, kind
    rng = np.random.default_rng([seed, zlib.crc32(kind.encode()), S, *shape])
    R = int(np.prod(shape))
    sv = rng.uniform(-90.0, -30.0, (R, S)).astype(np.float32)
    step = rng.uniform(0.1, 0.3, (R, S)).astype(np.float32)
    r = (rng.uniform(2.0, 50.0, (R, 1)).astype(np.float32) + np.cumsum(step, axis=1, dtype=np.float32)).astype(np.float32)
    j = np.arange(S)
    if kind == "nan_tail":
        cut = j[None, :] >= (np.arange(R) % (S + 1))[:, None]
        sv[cut] = np.nan
        r[cut] = np.nan
    elif kind == "sv_holes":
        sv[rng.random((R, S)) < 0.1] = np.nan
    elif kind == "range_nan":
        r[:, S // 2] = np.nan
    elif kind == "repeats":
        for k in range(2, S, 5):
            r[:, k] = r[:, k - 1]
    elif kind == "neg_inf":
        sv[rng.random((R, S)) < 0.1] = -np.inf
    elif kind == "all_neg_inf":
        sv[::3] = -np.inf
    elif kind == "decreasing":
        r = np.ascontiguousarray(r[:, ::-1])
    if kind == "shared":
        return sv.reshape(*shape, S).astype(dtype), r[0].astype(dtype)
    return sv.reshape(*shape, S).astype(dtype), r.reshape(*shape, S).astype(dtype)


def thin_layer(S, dtype=np.float64):
    """The conditioning case: a 0.1 m layer at 10 000 m, S samples, two rows (a flat layer and a ramp of 30 dB).  The
    expanded form sum r^2 w - 2 cm sum r w + cm^2 sum w cancels eleven digits here (r^2 / I ~ 1e11)."""
    r = 10000.0 + 0.1 * np.arange(S, dtype=np.float64) / max(S - 1, 1)
    sv = np.stack([np.full(S, -60.0), -70.0 + 30.0 * np.arange(S) / max(S - 1, 1)])
    return sv.astype(dtype), np.stack([r, r]).astype(dtype)
