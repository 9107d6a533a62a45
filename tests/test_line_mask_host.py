"""mask.line_mask without a GPU: the export and its signature, the NumPy restatement of its semantics
(tests/line_mask_ref.py) against answers written out by hand, every refusal of the public function (they all come before
any device work) and the refusals of the C entry."""
import inspect

import numpy as np
import pytest

from line_mask_ref import line_mask_ref

NAN, INF = np.nan, np.inf


def test_export_and_signature():
    import echopype_amd as ep
    from echopype_amd import _lib, ops

    assert "line_mask" in ep.mask.__all__ and callable(ops.line_mask)
    P = inspect.Parameter
    kw = P.POSITIONAL_OR_KEYWORD
    assert inspect.signature(ep.mask.line_mask) == inspect.Signature([
        P("ds", kw), P("upper", kw, default=None), P("lower", kw, default=None), P("range_var", kw, default="depth"),
        P("var_name", kw, default="Sv"), P("closed", kw, default="left"), P("nan_line", kw, default="exclude"),
        P("upper_offset", kw, default=0.0), P("lower_offset", kw, default=0.0), P("device", P.KEYWORD_ONLY, default=None)])
    assert len(_lib.SIGNATURES["epa_line_mask"]) == 23 and hasattr(_lib.lib, "epa_line_mask")
    assert (_lib.LINE_CLOSED_RIGHT, _lib.LINE_NAN_IGNORE) == (1, 2)
    assert _lib.lib.epa_version() == 104


def _row(r, **kw):
    return line_mask_ref(np.asarray(r, dtype=np.float64)[None, :], **kw)[0].tolist()


def test_restatement_ties_on_both_sides():
    r = [9.75, 10.0, 10.25, 19.75, 20.0, 20.25]
    assert _row(r, upper=10.0, lower=20.0) == [False, True, True, True, False, False]
    assert _row(r, upper=10.0, lower=20.0, closed="right") == [False, False, True, True, True, False]
    assert _row(r, upper=10.0) == [False, True, True, True, True, True]
    assert _row(r, upper=10.0, closed="right") == [False, False, True, True, True, True]
    assert _row(r, lower=20.0) == [True, True, True, True, False, False]
    assert _row(r, lower=20.0, closed="right") == [True, True, True, True, True, False]


def test_restatement_nan_sample_and_nan_line():
    assert _row([NAN, 15.0], upper=10.0) == [False, True]
    assert _row([NAN, 15.0], lower=20.0) == [False, True]
    r = np.array([[[5.0, 15.0], [5.0, 15.0]]])  # one channel, two pings
    up = np.array([NAN, 10.0])
    assert line_mask_ref(r, upper=up, lower=20.0).tolist() == [[[False, False], [False, True]]]
    assert line_mask_ref(r, upper=up, lower=20.0, nan_line="ignore").tolist() == [[[True, True], [False, True]]]
    assert line_mask_ref(r, upper=10.0, lower=up).tolist() == [[[False, False], [False, False]]]
    assert line_mask_ref(r, upper=10.0, lower=up, nan_line="ignore").tolist() == [[[False, True], [False, False]]]
    # both bounds NaN and ignored: nothing is tested, a NaN sample is still False
    assert _row([NAN, 1.0], upper=NAN, lower=NAN, nan_line="ignore") == [False, True]
    assert _row([NAN, 1.0], upper=NAN, lower=NAN) == [False, False]


def test_restatement_infinities_and_signed_zero():
    r = [-INF, 0.0, INF]
    assert _row(r, upper=-INF) == [True, True, True]
    assert _row(r, upper=-INF, closed="right") == [False, True, True]
    assert _row(r, lower=INF) == [True, True, False]
    assert _row(r, lower=INF, closed="right") == [True, True, True]
    assert _row(r, upper=INF) == [False, False, True]
    assert _row(r, lower=-INF, closed="right") == [True, False, False]
    assert _row([-0.0, 0.0], upper=0.0) == [True, True]
    assert _row([-0.0, 0.0], upper=0.0, closed="right") == [False, False]
    assert _row([0.0, -0.0], lower=-0.0) == [False, False]
    assert _row([0.0, -0.0], lower=-0.0, closed="right") == [True, True]


def test_restatement_offset_that_creates_a_tie_and_float32_promotion():
    assert _row([10.0], upper=10.25, upper_offset=-0.25) == [True]
    assert _row([10.0], upper=10.25, upper_offset=-0.25, closed="right") == [False]
    assert _row([10.0], lower=10.25, lower_offset=-0.25) == [False]
    assert _row([10.0], lower=10.25, lower_offset=-0.25, closed="right") == [True]
    # float32 samples are promoted, the line is not rounded to float32: fl32(0.1) > 0.1
    r32 = np.array([[0.1]], dtype=np.float32)
    assert line_mask_ref(r32, upper=0.1, closed="right").tolist() == [[True]]
    assert line_mask_ref(r32, lower=0.1, closed="right").tolist() == [[False]]
    assert line_mask_ref(r32.astype(np.float64) * 0 + 0.1, upper=0.1, closed="right").tolist() == [[False]]


# ---- the public function: refusals, all before any device work ----------------------------------------------------------
C_, P_, S_ = 2, 3, 4


def _ds(order=("channel", "ping_time", "range_sample")):
    from echopype_amd.xr_lite import Dataset

    sizes = {"channel": C_, "ping_time": P_, "range_sample": S_}
    ds = Dataset(coords={"channel": np.array(["a", "b"]), "range_sample": np.arange(S_),
                         "ping_time": np.datetime64("2026-01-01", "ns") + np.arange(P_) * np.timedelta64(1, "s")})
    shape = tuple(sizes[d] for d in order)
    ds["Sv"] = (order, np.zeros(shape))
    ds["depth"] = (order, np.zeros(shape))
    ds["bottom"] = (("ping_time",), np.array([50.0, NAN, 60.0]))
    return ds


def _line(dims, shape, **coords):
    from echopype_amd.xr_lite import DataArray

    return DataArray(np.zeros(shape), dims, coords=coords)


def test_refusals_of_the_public_function():
    import echopype_amd as ep
    from echopype_amd.xr_lite import DataArray

    lm = ep.mask.line_mask
    with pytest.raises(ValueError, match="not a valid option. Options are 'left' or 'right'"):
        lm(_ds(), upper=1.0, closed="both")
    with pytest.raises(ValueError, match="Options are 'exclude' or 'ignore'"):
        lm(_ds(), upper=1.0, nan_line="keep")
    with pytest.raises(ValueError, match="At least one of upper and lower"):
        lm(_ds())
    with pytest.raises(ValueError, match="lower_offset must be a finite number"):
        lm(_ds(), lower=1.0, lower_offset=NAN)
    with pytest.raises(ValueError, match="does not contain the variable Sv_corrected"):
        lm(_ds(), upper=1.0, var_name="Sv_corrected")
    with pytest.raises(ValueError, match="does not contain the variable echo_range"):
        lm(_ds(), upper=1.0, range_var="echo_range")
    # a DataArray bound: other dims, sizes, another dataset's ping_time
    with pytest.raises(ValueError, match="must have dimensions among"):
        lm(_ds(), upper=_line(("range_sample",), (S_,)))
    with pytest.raises(ValueError, match="must have dimensions among"):
        lm(_ds(), lower=_line(("channel", "ping_time", "range_sample"), (C_, P_, S_)))
    with pytest.raises(ValueError, match="dimension 'ping_time' has length 5, the dataset has 3"):
        lm(_ds(), lower=_line(("ping_time",), (5,)))
    with pytest.raises(ValueError, match="dimension 'channel' has length 3"):
        lm(_ds(), upper=_line(("ping_time", "channel"), (P_, 3)))
    with pytest.raises(ValueError, match="which the masked variable lacks"):
        lm(_ds(("ping_time", "range_sample")), upper=_line(("channel",), (C_,)))
    other = np.asarray(_ds()["ping_time"].values) + np.timedelta64(1, "ms")
    with pytest.raises(ValueError, match="a line from another dataset"):
        lm(_ds(), lower=_line(("ping_time",), (P_,), ping_time=other))
    with pytest.raises(TypeError, match="must hold real numbers"):
        lm(_ds(), lower=DataArray(np.zeros(P_, dtype=complex), ("ping_time",)))
    with pytest.raises(TypeError, match="must be a number, a string"):
        lm(_ds(), lower=[1.0, 2.0])
    # a string that is neither a variable nor "<number>m": the parser's own error
    with pytest.raises(ValueError, match="Range bin must be in meters"):
        lm(_ds(), upper="ten")
    # the dims of the masked variable and of the range
    for order in (("ping_time", "channel", "range_sample"), ("channel", "range_sample", "ping_time"),
                  ("range_sample", "ping_time")):
        with pytest.raises(NotImplementedError, match=r"must be \(channel, ping_time, X\) or \(ping_time, X\)"):
            lm(_ds(order), upper=1.0)
    ds = _ds()
    ds["depth"] = (("ping_time", "beam"), np.zeros((P_, 2)))
    with pytest.raises(ValueError, match="must be among those of Sv"):
        lm(ds, upper=1.0)
    ds = _ds()
    ds["tilt"] = (("ping_time",), np.zeros(P_, dtype=complex))
    with pytest.raises(TypeError, match="tilt must hold real numbers"):
        lm(ds, upper=1.0, range_var="tilt")


def test_forms_of_a_bound():
    from echopype_amd.mask.api import _check_bound

    ds = _ds()
    sizes = {"channel": C_, "ping_time": P_, "range_sample": S_}
    assert _check_bound(ds, None, "upper", sizes) is None
    for b in (250, 250.0, np.float32(250), np.int64(250), "250.0m", "250m", " 250 m"):
        got = _check_bound(ds, b, "upper", sizes)
        assert type(got) is float and got == 250.0, b
    got = _check_bound(ds, "bottom", "lower", sizes)  # the name of a variable comes first
    assert got.dims == ("ping_time",) and np.array_equal(got.values, [50.0, NAN, 60.0], equal_nan=True)
    ds["10m"] = (("ping_time",), np.arange(3.0))
    assert _check_bound(ds, "10m", "lower", sizes).dims == ("ping_time",)
    for dims in ((), ("ping_time",), ("channel",), ("channel", "ping_time"), ("ping_time", "channel")):
        line = _line(dims, tuple(sizes[d] for d in dims))
        assert _check_bound(ds, line, "upper", sizes) is line
    with pytest.raises(TypeError):
        _check_bound(ds, True, "upper", sizes)


# ---- the C entry -----------------------------------------------------------------------------------------------------------
def _call(range=8, coef=None, nan_raw=None, scale=None, offset=None, dtype=1, upper=8, lower=8, flags=0, out=8,
          strides=(0, 0, 1), shape=(0, 0, 0), upper_offset=0.0):
    from echopype_amd import _lib

    # (no launch can follow: every call here is refused, and the shape is empty besides)
    _lib.call("epa_line_mask", range, *strides, coef, nan_raw, scale, offset, dtype, upper, 0, 1, upper_offset, lower, 0, 1,
              0.0, flags, *shape, out, None)


def test_the_library_refuses_bad_arguments_before_any_hip_call():
    _call()  # an empty shape: nothing to do
    with pytest.raises(ValueError, match="epa_line_mask: out is NULL"):
        _call(out=None)
    with pytest.raises(ValueError, match="epa_line_mask: both lines are NULL"):
        _call(upper=None, lower=None)
    _call(upper=None)
    _call(lower=None)
    for bad in (-1, 2, 7):
        with pytest.raises(ValueError, match=f"epa_line_mask: bad dtype {bad}"):
            _call(dtype=bad)
    with pytest.raises(ValueError, match="as an array or as coefficient rows, one of the two"):
        _call(range=None)
    with pytest.raises(ValueError, match="as an array or as coefficient rows, one of the two"):
        _call(coef=8)
    with pytest.raises(ValueError, match="go with the coefficient rows"):
        _call(nan_raw=8)
    with pytest.raises(ValueError, match="scale and offset come together"):
        _call(range=None, coef=8, scale=8)
    with pytest.raises(ValueError, match="flags takes"):
        _call(flags=4)
    with pytest.raises(ValueError, match="bad shape"):
        _call(shape=(1, -1, 1))
    with pytest.raises(ValueError, match="bad shape"):
        _call(shape=(1, 1, (1 << 30) + 1))
    with pytest.raises(ValueError, match="strides must not be negative"):
        _call(strides=(0, -1, 1))
    with pytest.raises(ValueError, match="an offset is NaN"):
        _call(upper_offset=NAN)


def test_the_wrapper_refuses_before_it_calls():
    import torch

    from echopype_amd import ops

    with pytest.raises(ValueError, match="closed must be"):
        ops.line_mask((1, 1, 1), range=torch.zeros(1), upper=torch.zeros(1, 1), closed="both")
    with pytest.raises(ValueError, match="nan_line must be"):
        ops.line_mask((1, 1, 1), range=torch.zeros(1), upper=torch.zeros(1, 1), nan_line="keep")
    with pytest.raises(ValueError, match="at least one of upper and lower"):
        ops.line_mask((1, 1, 1), range=torch.zeros(1))
    with pytest.raises(ValueError, match="one of the two"):
        ops.line_mask((1, 1, 1), upper=torch.zeros(1, 1))
    with pytest.raises(ValueError, match="float32 / float64 device tensor"):
        ops.line_mask((1, 1, 1), range=torch.zeros(1), upper=torch.zeros(1, 1))
