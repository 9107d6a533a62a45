"""Host-side checks of the reversed-time repair: the restatement tests/qc_ref.py against what the reference's own
``_clean_reversed`` and ``exist_reversed_time`` gave for the cases of tests/qc_cases.py (tests/golden/qc_reversed_time.npz,
written by scripts/gen_qc_goldens.py) bit for bit, the facts about ``np.median`` of timedelta64 the kernels reproduce, and
the three public signatures."""
import inspect

import numpy as np
import pytest

import qc_cases as C
import qc_ref as R

RECORDS, Z = C.load_fixture()
BY_NAME = {r["name"]: r for r in RECORDS}


def test_the_fixture_holds_the_cases_of_the_generator():
    assert sorted(BY_NAME) == sorted(C.FIXTURE_CASES + tuple(C.ERRORS) + tuple(C.NAT_CASES))
    for name in C.FIXTURE_CASES + tuple(C.ERRORS):
        c = C.case(name)
        stored = Z[f"case/{name}/in"]
        assert stored.dtype == c["t"].dtype and np.array_equal(stored.view(np.int64), c["t"].view(np.int64)), name
        assert BY_NAME[name]["win_len"] == c["win_len"] and stored.nbytes <= 4096, name
    for name in C.NAT_CASES:
        assert np.array_equal(Z[f"case/{name}/in"].view(np.int64), C.nat_case(name).view(np.int64)), name


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_restatement_equals_the_reference_executed_result(name):
    rec, t = BY_NAME[name], Z[f"case/{name}/in"]
    want = Z[f"case/{name}/out"]
    assert want.dtype == t.dtype
    got = R.clean_reversed(t, rec["win_len"])
    assert got.dtype == np.int64 and np.array_equal(got, want.view(np.int64)), name
    assert R.is_sorted_and_valid(got) == rec["sorted"]


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_exist_reversed_equals_the_reference(name):
    assert R.exist_reversed(Z[f"case/{name}/in"]) == BY_NAME[name]["exists"]
    if name in C.NAT_CASES:
        assert BY_NAME[name]["exists"] == C.NAT_CASES[name][1]


@pytest.mark.parametrize("name", sorted(C.ERRORS))
def test_the_reference_dies_with_index_error_and_so_does_the_restatement(name):
    assert BY_NAME[name]["raised"] == "IndexError"
    c = C.case(name)
    with pytest.raises(IndexError):
        R.clean_reversed(c["t"], c["win_len"])


@pytest.mark.parametrize("pair, want", [((3, 8), 5), ((-3, -8), -5), ((-3, 8), 2), ((-8, 3), -2)])
def test_median_of_an_even_window_truncates_toward_zero(pair, want):
    assert R.median(list(pair)) == want
    assert np.median(np.array(pair, dtype="timedelta64[ns]")).astype(np.int64) == want  # NumPy's own answer
    # ... and the wrapping sum: two values whose sum leaves int64
    big = (1 << 62) + 1
    assert R.median([big, big]) == -(1 << 62) + 1  # (2**63 + 2 wraps to -2**63 + 2)


@pytest.mark.parametrize("win_len", [100, 2])
def test_the_worked_example(win_len):
    t = np.array([0, 10, 20, 15, 25, 35, 30, 40], dtype=np.int64)
    want = [0, 10, 20, 30, 40, 50, 60, 70]
    assert R.clean_reversed(t, win_len).tolist() == want
    assert Z[f"case/worked_w{win_len}/out"].view(np.int64).tolist() == want
    assert np.array_equal(C.case(f"worked_w{win_len}")["t"].view(np.int64), t)


def test_nested_reversals_take_their_medians_from_the_original_differences():
    """The two nested cases are built so that a median taken AFTER the earlier substitution would differ."""
    for name, ni, original, substituted in (("nested_w4", 4, 14, 17), ("nested_w2", 3, 1, 11)):
        c = C.case(name)
        t = R.ticks(c["t"])
        d = [t[i + 1] - t[i] for i in range(len(t) - 1)]
        w = c["win_len"]
        assert R.median(d[ni - w:ni]) == original
        d[2] = R.median(d[max(0, 2 - w):2])
        assert R.median(d[ni - w:ni]) == substituted
        got = Z[f"case/{name}/out"].view(np.int64)
        assert got[ni + 1] - got[ni] == original


def test_the_microsecond_case_truncates_in_its_own_ticks():
    c = C.case("epoch_us")
    assert c["t"].dtype == np.dtype("datetime64[us]")
    t = R.ticks(c["t"])
    (ni,) = R.reversals(c["t"])
    win = sorted(t[i + 1] - t[i] for i in range(ni - c["win_len"], ni))
    assert len(win) % 2 == 0 and (win[len(win) // 2 - 1] + win[len(win) // 2]) % 2 == 1


# the reference's signatures (qc/api.py:38-40, 71, 88-90), written out: names, order and defaults
SIGNATURES = {
    "exist_reversed_time": "(ds, time_name)",
    "coerce_increasing_time": "(ds, time_name='ping_time', win_len=100)",
    "check_and_correct_reversed_time": "(combined_group, time_str, ed_group)",
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature_equals_the_reference(name):
    import echopype_amd as ep

    sig = inspect.signature(getattr(ep.qc, name))
    bare = sig.replace(parameters=[p.replace(annotation=inspect.Parameter.empty) for p in sig.parameters.values()],
                       return_annotation=inspect.Signature.empty)
    assert str(bare) == SIGNATURES[name]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    assert sorted(ep.qc.__all__) == sorted(SIGNATURES) and "qc" in ep.__all__


def test_argument_checks_need_no_gpu():
    """What coerce_increasing_time refuses before it touches the device."""
    import echopype_amd as ep

    ds = ep.Dataset(coords={"ping_time": C.case("worked_w2")["t"], "depth": np.arange(4.0)})
    with pytest.raises(ValueError, match="win_len must be at least 1"):
        ep.qc.coerce_increasing_time(ds, win_len=0)
    with pytest.raises(NotImplementedError, match=str(C.MAX_WIN)):
        ep.qc.coerce_increasing_time(ds, win_len=C.MAX_WIN + 1)
    with pytest.raises(TypeError, match="not a datetime64 coordinate"):
        ep.qc.coerce_increasing_time(ds, "depth")
    assert ep.ops.QC_MAX_WIN == C.MAX_WIN
    from echopype_amd import _lib

    assert (_lib.QC_SCAN_TILE, _lib.QC_MEDIAN_WAVES) == (C.SCAN_TILE, C.MEDIAN_WAVES)
    # the constants of the binding are the header's
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "echopype_amd.h")).read()
    for k in ("FACTS", "FIRST", "COUNT", "NAT", "SLOTS", "MAX_WIN", "MEDIAN_WAVES", "SCAN_TILE"):
        assert int(re.search(rf"#define EPA_QC_{k} (\d+)", hdr).group(1)) == getattr(_lib, f"QC_{k}"), k
