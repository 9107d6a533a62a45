"""The NumPy oracle of the echo summary statistics (tests/metrics_ref.py) against what the reference's own functions
returned (tests/golden/ref_metrics_goldens.npz, scripts/gen_metrics_goldens.py), the drop-in signatures and messages of
``echopype_amd.metrics``, and the conditioning of the case the GPU tests demand 1e-9 on.  No GPU."""
import inspect
import json
import os

import numpy as np
import pytest

import metrics_bounds as B
import metrics_cases as C
import metrics_ref as R
from test_signatures import ALLOWED_EXTRAS, KIND, _same_default

CASES, KNOWN, Z = C.load_fixture()
SIGS = json.load(open(os.path.join(os.path.dirname(C.GOLDEN), "ref_metrics_signatures.json")))


def assert_same_specials(got, want, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN pattern")
    inf = np.isinf(want)
    np.testing.assert_array_equal(np.isinf(got), inf, err_msg=f"{what}: inf pattern")
    np.testing.assert_array_equal(got[inf], want[inf], err_msg=f"{what}: inf sign")


def assert_rel(got, want, rtol, what, floor=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert_same_specials(got, want, what)
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    tol = rtol * np.abs(want[fin]) + np.broadcast_to(floor, want.shape)[fin]
    assert np.all(err <= tol), (what, float((err / np.maximum(np.abs(want[fin]), 1e-300)).max()))


@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_oracle_equals_the_reference_in_float64(case):
    ds = C.case_inputs(Z, case, np.float64)
    seen = 0
    for name in C.STATS:
        err = case["results"].get(f"f64/{name}")
        if err is not None:
            with pytest.raises(ValueError) as e:
                R.FUNCS[name](ds, range_label=case["label"])
            assert [type(e.value).__name__, str(e.value)] == err
            continue
        with np.errstate(all="ignore"):
            got = R.FUNCS[name](ds, range_label=case["label"])
        floor = 0.0
        if name == "dispersion":  # (see metrics_ref.dispersion_floor: a row of one term has I = 0 up to the rounding of cm)
            floor = R.dispersion_floor(R.center_of_mass(ds))
        assert_rel(got, Z[f"{case['tag']}/f64/{name}"], 1e-12, f"{case['tag']} {name}", floor)
        seen += 1
    assert seen or case["label"] == "nothing"


def test_fixture_holds_every_content_and_special_value():
    assert {c["kind"] for c in CASES} == set(C.KINDS)
    ab = Z["nan_tail_33/f64/abundance"].ravel()
    assert np.isneginf(ab[:2]).all() and np.isfinite(ab[2:]).all()  # 0 and 1 valid samples: no dz, the sum is 0
    assert np.isnan(Z["nan_tail_33/f64/center_of_mass"].ravel()[:2]).all()
    assert np.isnan(Z["decreasing_33/f64/abundance"]).all() and np.isfinite(Z["decreasing_33/f64/dispersion"]).all()
    assert np.isneginf(Z["all_neg_inf_33/f64/abundance"].ravel()[::3]).all()
    assert np.isnan(Z["all_neg_inf_33/f64/evenness"].ravel()[::3]).all()


@pytest.mark.parametrize("name", C.STATS)
def test_oracle_gives_the_known_answers_of_the_reference_tests(name):
    """Integer inputs, ``frequency`` as the first dimension; np.allclose with the reference's rtol, as its tests call it."""
    k = KNOWN[name]
    assert k["rtol"] == 1e-9
    got = R.FUNCS[name]({"Sv": np.array(k["Sv"]), "echo_range": np.array(k["echo_range"])})
    assert np.allclose(got, np.array(k["expected"]), rtol=k["rtol"]), (name, got)


def test_helpers_equal_the_reference():
    n = 0
    for case in CASES:
        ds = C.case_inputs(Z, case, np.float64)
        for name, f in (("delta_z", R.delta_z), ("convert_to_linear", R.convert_to_linear)):
            dims = case["results"].get(f"f64/{name}")
            if not isinstance(dims, list) or dims[0] == "ValueError":
                continue
            got = f(ds, case["label"]) if name == "delta_z" else f(ds)
            want = Z[f"{case['tag']}/f64/{name}"]
            canon = [d for d in case["dims"] if d != "range_sample"] + ["range_sample"]
            if got.ndim == len(canon):
                want = np.transpose(want, [dims.index(d) for d in canon])
            assert_rel(got, want, 1e-15, f"{case['tag']} {name}")
            n += 1
    assert n >= 8


def test_dispersion_takes_its_centre_from_echo_range():
    case = next(c for c in CASES if c["tag"] == "depth_33")
    ds = C.case_inputs(Z, case, np.float64)
    got = R.dispersion(ds, range_label="depth")
    assert_rel(got, Z["depth_33/f64/dispersion"], 1e-12, "depth")
    own = R.rows(ds["Sv"], ds["depth"])[0]["dispersion"]  # about depth's own centre: the least I there is, another number
    assert np.all(got >= own * (1 - 1e-12)) and np.any(got > 1.5 * own)
    alone = next(c for c in CASES if c["tag"] == "depth_alone_33")
    assert alone["results"]["f64/dispersion"] == ["ValueError", "echo_range not in the input Dataset!"]
    assert "f64/abundance" not in alone["results"]  # the other four do not need echo_range
    with pytest.raises(ValueError, match="^echo_range not in the input Dataset!$"):
        R.dispersion(C.case_inputs(Z, alone, np.float64), range_label="depth")


# ---- the package: signatures and messages (no device work is reached) -------------------------------------------------------
@pytest.mark.parametrize("qual", sorted(SIGS))
def test_signature_equals_the_reference(qual):
    import echopype_amd as ep

    mod, name = qual.split(".")
    fn = getattr(getattr(ep, mod), name)
    got = [(p.name, KIND[p.kind], p.default) for p in inspect.signature(fn).parameters.values()]
    ref = SIGS[qual]["params"]
    core = [g for g in got if not (g[0] in ALLOWED_EXTRAS or g[0].startswith("_"))]
    extras = [g for g in got if g[0] in ALLOWED_EXTRAS or g[0].startswith("_")]
    assert [g[0] for g in core] == [r[0] for r in ref], f"{qual}: parameter names / order"
    for (n, kind, default), (rn, rkind, rsrc) in zip(core, ref):
        assert kind == rkind, f"{qual}: {n} is {kind}, the reference's is {rkind}"
        assert _same_default(default, rsrc), f"{qual}: default of {n} is {default!r}, the reference's is {rsrc}"
    for n, kind, default in extras:
        assert kind == "keyword_only" and default is not inspect.Parameter.empty, f"{qual}: extra parameter {n}"


def test_the_seven_names_and_summary_are_exported():
    import echopype_amd as ep

    assert "metrics" in ep.__all__
    assert sorted(SIGS) == sorted(f"metrics.{n}" for n in ep.metrics.__all__ if n != "summary")
    assert "summary" in ep.metrics.__all__


def test_a_missing_range_variable_raises_the_reference_message():
    import echopype_amd as ep
    from echopype_amd.xr_lite import Dataset

    ds = Dataset(coords={"ping_time": np.arange(2), "range_sample": np.arange(3)})
    ds["Sv"] = (("ping_time", "range_sample"), np.zeros((2, 3)))
    ds["depth"] = (("ping_time", "range_sample"), np.ones((2, 3)))
    missing = next(c for c in CASES if c["tag"] == "missing_5")
    for name in ("delta_z",) + C.STATS + ("summary",):
        fn = getattr(ep.metrics, name)
        if name != "summary":
            assert missing["results"][f"f64/{name}"] == ["ValueError", "nothing not in the input Dataset!"]
        with pytest.raises(ValueError, match="^nothing not in the input Dataset!$"):
            fn(ds, range_label="nothing")
        with pytest.raises(ValueError, match="^echo_range not in the input Dataset!$"):
            fn(ds)
    # the quirk: dispersion needs echo_range whatever the label names, and says so with the default label
    for name in ("dispersion", "summary"):
        with pytest.raises(ValueError, match="^echo_range not in the input Dataset!$"):
            getattr(ep.metrics, name)(ds, range_label="depth")


# ---- conditioning ------------------------------------------------------------------------------------------------------
def _dispersion_longdouble(sv, r):
    L = np.longdouble
    sv, r = sv.astype(L), r.astype(L)
    dz = np.diff(r, axis=-1)
    rj, lin = r[..., 1:], L(10) ** (sv[..., 1:] / L(10))
    w = lin * dz
    A = w.sum(axis=-1)
    cm = (rj * w).sum(axis=-1) / A
    return (((rj - cm[..., None]) ** 2 * w).sum(axis=-1) / A)


@pytest.mark.parametrize("S", [64, 4097])
def test_thin_layer_far_away_is_well_conditioned_when_centred(S):
    """A 0.1 m layer at 10 000 m: the float64 oracle's dispersion agrees with an np.longdouble evaluation to 1e-10, which
    is what licenses demanding 1e-9 of the device on this case (tests/test_gpu_metrics.py).  The expanded form
    sum r^2 w - 2 cm sum r w + cm^2 sum w (terms 1e11 times the result) misses that bar even in float64."""
    assert np.finfo(np.longdouble).eps < 2.0**-60, "np.longdouble is no wider than double on this machine"
    sv, r = C.thin_layer(S)
    st, s = R.rows(sv, r)
    want = _dispersion_longdouble(sv, r).astype(np.float64)
    assert np.all(want > 1e-5) and np.all(want < 1e-2)
    assert np.all(np.abs(st["dispersion"] - want) <= 1e-10 * want), (st["dispersion"], want)
    dz = np.diff(r, axis=-1)
    lin = 10.0 ** (sv[..., 1:] / 10)
    w, rj = lin * dz, r[..., 1:]
    expanded = ((rj * rj * w).sum(-1) - 2 * s["cm"] * (rj * w).sum(-1) + s["cm"] ** 2 * w.sum(-1)) / w.sum(-1)
    assert np.all(np.abs(expanded - want) > 1e-8 * want)  # (measured here: 1e-5 and 3e-4 of the value)


# ---- the bounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c["label"] == "echo_range"], ids=lambda c: c["tag"])
def test_reference_float32_results_lie_within_their_derived_slack(case):
    """The reference's own float32 evaluation against the oracle on the same float32 values: the slack the GPU tests add
    when they compare with these results is a bound of them."""
    ds = C.case_inputs(Z, case, np.float32)
    with np.errstate(all="ignore"):
        st, s = R.rows(ds["Sv"], ds["echo_range"])
        slack = B.reference_f32_slack(st, s)
        kb = B.kernel_bounds(st, s)
    for name in C.STATS:
        ref32 = Z[f"{case['tag']}/f32/{name}"].astype(np.float64)
        assert ref32.shape == st[name].shape
        assert_same_specials(ref32, st[name], f"{case['tag']} {name}")
        fin = np.isfinite(st[name])
        assert np.all(np.isfinite(slack[name][fin])) and np.all(np.isfinite(kb[name][fin])), name
        with np.errstate(invalid="ignore"):
            err = np.abs(ref32 - st[name])
        assert np.all(err[fin] <= slack[name][fin]), (case["tag"], name)
        # the kernel's bound is a float32 bound: far inside the old 1e-3 bar on these inputs
        assert np.all(kb[name][fin] <= 1e-4 * np.maximum(np.abs(st[name][fin]), 1.0)), (case["tag"], name)
