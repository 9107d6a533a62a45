"""mask.frequency_differencing without a GPU: the criterion parser (accepted forms, every error with its type and
message), the dataset checks, the public signature, and the judge's own arithmetic rule."""
import inspect

import numpy as np
import pytest

import freq_diff_ref as R


def _parse(**kw):
    from echopype_amd.mask.freq_diff import _parse_freq_diff_eq

    return _parse_freq_diff_eq(**kw)


@pytest.mark.parametrize("eq, want", [
    ("38.0kHz - 120 kHz >= 10.0dB", [[38000.0, 120000.0], None, ">=", 10.0]),
    ("38kHz-120kHz>10dB", [[38000.0, 120000.0], None, ">", 10.0]),
    ("  ".join(["18000Hz", "-", "0.2MHz", "<", "5", "dB"]), [[18000.0, 200000.0], None, "<", 5.0]),
    ("1 GHz - .5GHz <= 0.25dB", [[1e9, 0.5e9], None, "<=", 0.25]),
    ("70 kHz - 38.5kHz == 3dB", [[70000.0, 38500.0], None, "==", 3.0]),
    ("200 Hz - 2 kHz<12.5 dB and more", [[200.0, 2000.0], None, "<", 12.5]),  # (match, not fullmatch: a tail is ignored)
])
def test_frequency_equations(eq, want):
    got = _parse(freqABEq=eq)
    assert got == want and isinstance(got[3], float)


@pytest.mark.parametrize("eq, want", [
    ('"chan1" - "chan2" < 5dB', [None, ["chan1", "chan2"], "<", 5.0]),
    ('"chan1"-"chan2">=10.0dB', [None, ["chan1", "chan2"], ">=", 10.0]),
    ('"GPT  38 kHz 009072058c8d 1-1 ES38B"  -  "GPT 120 kHz 00907205a6d0 4-1 ES120-7C" > 7 dB',
     [None, ["GPT  38 kHz 009072058c8d 1-1 ES38B", "GPT 120 kHz 00907205a6d0 4-1 ES120-7C"], ">", 7.0]),
    ('"a" - "b" == .5dB', [None, ["a", "b"], "==", 0.5]),
    ('"a" - "b" <= 12dB', [None, ["a", "b"], "<=", 12.0]),
])
def test_channel_equations(eq, want):
    got = _parse(chanABEq=eq)
    assert got == want and isinstance(got[3], float)


@pytest.mark.parametrize("kw, typ, msg", [
    ({}, ValueError, "Either freqAB or chanAB must be given!"),
    ({"freqABEq": "38kHz - 120kHz > 1dB", "chanABEq": '"a" - "b" > 1dB'}, ValueError,
     "Only one of freqAB or chanAB should be given, but not both!"),
    ({"freqABEq": "38kHz + 120kHz > 1dB"}, TypeError, "Invalid freqAB Equation!"),
    ({"freqABEq": "38k - 120kHz > 1dB"}, TypeError, "Invalid freqAB Equation!"),
    ({"freqABEq": "38kHz - 120kHz > 1"}, TypeError, "Invalid freqAB Equation!"),
    ({"freqABEq": '"a" - "b" > 1dB'}, TypeError, "Invalid freqAB Equation!"),
    ({"chanABEq": "chan1 - chan2 > 1dB"}, TypeError, "Invalid chanAB Equation!"),
    ({"chanABEq": '"a" - "b" > dB'}, TypeError, "Invalid chanAB Equation!"),
    ({"freqABEq": "38kHz - 120kHz => 1dB"}, ValueError, "Invalid operator!"),
    ({"freqABEq": "38kHz - 120kHz 1dB"}, ValueError, "Invalid operator!"),
    ({"freqABEq": "38kHz - 120kHz != 1dB"}, ValueError, "Invalid operator!"),
    ({"chanABEq": '"a" - "b" = 1dB'}, ValueError, "Invalid operator!"),
    ({"freqABEq": "38kHz - 38000Hz > 1dB"}, ValueError, "freqAB must be a list of length 2 with unique elements!"),
    ({"chanABEq": '"a" - "a" > 1dB'}, ValueError, "chanAB must be a list of length 2 with unique elements!"),
])
def test_equation_errors(kw, typ, msg):
    with pytest.raises(Exception) as ei:
        _parse(**kw)
    assert type(ei.value) is typ and str(ei.value) == msg


def _ds(channels=("chan1", "chan2", "chan3"), freqs=(38000.0, 120000.0, 200000.0), with_channel=True, with_freq=True):
    from echopype_amd.xr_lite import Dataset

    C = len(channels)
    ds = Dataset(coords={"channel": np.array(channels)} if with_channel else {})
    ds["Sv"] = (("channel", "ping_time", "range_sample") if with_channel else ("c", "ping_time", "range_sample"),
                np.zeros((C, 2, 3)))
    if with_freq:
        ds["frequency_nominal"] = (("channel",) if with_channel else ("c",), np.array(freqs))
    return ds


@pytest.mark.parametrize("ds_kw, freqAB, chanAB, msg", [
    ({"with_channel": False}, None, ["chan1", "chan2"], "The Dataset defined by source_Sv must have channel as a coordinate!"),
    ({"with_freq": False}, [38000.0, 120000.0], None,
     "The Dataset defined by source_Sv must have frequency_nominal as a variable!"),
    ({"channels": ("chan1", "chan2", "chan1")}, None, ["chan1", "chan2"],
     "The provided source_Sv contains repeated channel values, this is not allowed!"),
    ({}, None, ["chan1", "chan9"], "The provided list input chanAB contains values that are not in the channel coordinate!"),
    ({"freqs": (38000.0, 120000.0, 38000.0)}, [38000.0, 120000.0], None,
     "The provided source_Sv contains repeated frequency_nominal values, this is not allowed!"),
    ({}, [38000.0, 70000.0], None,
     "The provided list input freqAB contains values that are not in the frequency_nominal variable!"),
])
def test_dataset_errors(ds_kw, freqAB, chanAB, msg):
    from echopype_amd.mask.freq_diff import _check_freq_diff_source_Sv

    with pytest.raises(ValueError) as ei:
        _check_freq_diff_source_Sv(_ds(**ds_kw), freqAB, chanAB)
    assert str(ei.value) == msg
    assert _check_freq_diff_source_Sv(_ds(), [38000.0, 200000.0], None) is None
    assert _check_freq_diff_source_Sv(_ds(), None, ["chan3", "chan1"]) is None


def test_the_public_function_raises_them_before_any_device_work():
    import echopype_amd as ep

    with pytest.raises(ValueError, match="Either freqAB or chanAB must be given!"):
        ep.mask.frequency_differencing(_ds())
    with pytest.raises(TypeError, match="Invalid chanAB Equation!"):
        ep.mask.frequency_differencing(_ds(), chanABEq="chan1 - chan2 > 1dB")
    with pytest.raises(ValueError, match="not in the frequency_nominal variable"):
        ep.mask.frequency_differencing(_ds(), freqABEq="38kHz - 70kHz > 1dB")
    with pytest.raises(NotImplementedError):
        ep.mask.frequency_differencing("some/file.zarr", chanABEq='"chan1" - "chan2" > 1dB')


def test_signatures_and_exports():
    import echopype_amd as ep

    P = inspect.Parameter
    kw = P.POSITIONAL_OR_KEYWORD
    assert inspect.signature(ep.mask.frequency_differencing) == inspect.Signature([
        P("source_Sv", kw), P("storage_options", kw, default={}), P("freqABEq", kw, default=None),
        P("chanABEq", kw, default=None)])
    assert inspect.signature(ep.mask.regrid_mask) == inspect.Signature([
        P("mask_da", kw), P("range_da", kw), P("range_bin", kw, default="20m"), P("ping_time_bin", kw, default="20s"),
        P("third_dim", kw, default=None), P("func", kw, default="logical-AND"), P("method", kw, default="map-reduce"),
        P("reindex", kw, default=False), P("closed", kw, default="left"), P("range_var_max", kw, default=None),
        P("flox_kwargs", P.VAR_KEYWORD)])
    assert "frequency_differencing" in ep.mask.__all__ and "regrid_mask" in ep.mask.__all__
    assert {"apply_mask", "detect_seafloor", "detect_shoal"} <= set(ep.mask.__all__)


def test_the_judge_compares_in_the_type_of_the_array():
    """NumPy's rule for an array and a Python scalar, the one the reference runs into: float32 data is compared with
    fl32(diff).  With a - b == fl32(0.1) the float64 rule would call the difference greater than 0.1."""
    sv = np.zeros((2, 4), dtype=np.float32)
    sv[0] = [np.float32(0.1), 0.5, np.nan, 0.0]
    for op in R.OPS:
        np.testing.assert_array_equal(R.freq_diff(sv, 0, 1, op, 0.1), R.freq_diff_typed(sv, 0, 1, op, 0.1))
    assert not R.freq_diff(sv, 0, 1, ">", 0.1)[0] and R.freq_diff_in_double(sv, 0, 1, ">", 0.1)[0]
    assert R.freq_diff(sv, 0, 1, "==", 0.1)[0] and not R.freq_diff_in_double(sv, 0, 1, "==", 0.1)[0]
    assert not any(R.freq_diff(sv, 0, 1, op, 0.1)[2] for op in R.OPS)  # NaN: False for all five
