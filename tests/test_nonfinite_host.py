"""The +-inf cases of tests/nonfinite_cases.py do their job -- against the oracle alone, no GPU: the infinite samples sit
where the kernels' structure is at stake, and the oracle's outputs show the effect each case exists for."""
import numpy as np
import pytest

import nonfinite_cases as nc
from oracle import commongrid as ogrid


@pytest.mark.parametrize("key", nc.all_cases(), ids=nc.case_id)
def test_echo_range_is_nan_exactly_at_the_nan_samples(key):
    cs = nc.build(*key)
    sv, er = cs.sv_er()
    np.testing.assert_array_equal(np.isnan(er), np.isnan(cs.raw))
    assert np.isinf(cs.raw).any() or cs.name == "overflow"
    assert np.isfinite(er[np.isinf(cs.raw)]).all()
    assert cs.has_nan == (key[2] or cs.name == "bin_classes")
    # Sv is +-inf exactly where the raw sample is and R' > 0 (s >= 3 for these rows); NaN where R' <= 0
    np.testing.assert_array_equal(np.isinf(sv[:, :, 3:]), np.isinf(cs.raw[:, :, 3:]))
    np.testing.assert_array_equal(np.sign(sv[:, :, 3:][np.isinf(sv[:, :, 3:])]), np.sign(cs.raw[:, :, 3:][np.isinf(cs.raw[:, :, 3:])]))
    assert np.isnan(sv[:, :, :3]).all()
    assert cs.raw.size < 50_000


@pytest.mark.parametrize("S", nc.SIZES)
@pytest.mark.parametrize("with_nan", [False, True])
def test_last_column_sizes_the_grid(S, with_nan):
    cs = nc.build("last_column", S, with_nan)
    sv, er = cs.sv_er()
    mv, _, r_left = cs.mvbs()
    dropped = np.where(np.isinf(cs.raw), np.nan, er)         # what a kernel that masks inf like NaN would bin on
    n_dropped = len(ogrid.range_edges(dropped, ogrid.parse_range_bin(cs.range_bin))) - 1
    assert mv.shape[2] == len(r_left) == n_dropped + 1 == 41
    assert np.nanmax(er) == er[:, :, S - 1].max() and np.isinf(cs.raw[:, :, S - 1]).all()
    assert (nc.classes(mv[:, :, -1]) == 1).all()           # the last bin holds those samples alone: +inf


@pytest.mark.parametrize("S", nc.SIZES)
def test_first_columns_hold_the_range_minimum(S):
    cs = nc.build("first_columns", S)
    sv, er = cs.sv_er()
    assert np.nanmin(er) == 0.0 and (er[:, :, 0] == 0.0).all() and np.isneginf(cs.raw[:, :, :4]).all()
    assert np.isnan(sv[:, :, :3]).all() and np.isneginf(sv[:, :, 3]).all()     # R' <= 0 next to -inf
    with_nan = nc.build("first_columns", S, True)
    assert np.nanmin(with_nan.sv_er()[1]) == 0.0


@pytest.mark.parametrize("S", nc.SIZES)
def test_one_lane_positions(S):
    cs = nc.build("one_lane", S)
    m = cs.marks
    raw = cs.raw
    assert np.isinf(raw).sum() == 2 and raw[m["channel"], m["ping"], m["pos"]] == np.inf \
        and raw[m["channel"], m["ping"], m["neg"]] == -np.inf
    base = 256 * m["wavefront"]
    assert m["wavefront"] == (2 if S >= 768 else 0) and base + 256 <= S + 1
    a, b = m["pos"] - base, m["neg"] - base
    assert 0 <= a < 128 and a % 2 == 0            # pair A: base + 2l, the pair's first sample
    assert 128 <= b < 256 and (b - 128) % 2 == 1  # pair B: base + 128 + 2l, the pair's second sample
    assert a // 2 != (b - 128) // 2               # two different lanes
    # every other wavefront of that ping, and this one in every other ping, is all finite
    others = np.ones(raw.shape, bool)
    others[m["channel"], m["ping"], base:base + 256] = False
    assert np.isfinite(raw[others]).all()


@pytest.mark.parametrize("S", nc.SIZES)
def test_whole_ping(S):
    cs = nc.build("whole_ping", S)
    assert (cs.raw[:, cs.marks["pos_ping"]] == np.inf).all() and (cs.raw[:, cs.marks["neg_ping"]] == -np.inf).all()
    mv, _, _ = cs.mvbs()
    assert (nc.classes(mv[:, 0, 1:]) == 1).all()             # time bin 0 holds the +inf ping
    assert (nc.classes(mv[:, 2, 1:]) == 0).all()             # the -inf ping adds zeros to the means of time bin 2


@pytest.mark.parametrize("S", nc.SIZES)
def test_bin_classes_occur_in_the_expected_mvbs(S):
    cs = nc.build("bin_classes", S)
    m = cs.marks
    c, tb = m["channel"], m["time_bin"]
    mv, _, _ = cs.mvbs(skipna=True)
    mv_all, _, _ = cs.mvbs(skipna=False)
    assert mv[c, tb, m["only_neg"]] == -np.inf and mv_all[c, tb, m["only_neg"]] == -np.inf
    assert np.isfinite(mv[c, tb, m["neg_and_finite"]])
    assert mv[c, tb, m["pos_and_neg"]] == np.inf and mv_all[c, tb, m["pos_and_neg"]] == np.inf
    # (a NaN raw sample has a NaN echo_range: it is in no bin, whatever skipna says; the NaN Sv that skipna=False does
    # see are the R' <= 0 samples of range bin 0, whose range is a number)
    assert mv[c, tb, m["pos_and_nan"]] == np.inf and mv_all[c, tb, m["pos_and_nan"]] == np.inf
    assert np.isnan(mv_all[:, :, 0]).all() and np.isfinite(mv[:, :, 0]).all()
    # the zero terms of the -inf samples count in the mean: the same bin without them is higher by 10 log10(n / (n - 2))
    sv, er = cs.sv_er()
    finite_only, _, _ = ogrid.compute_MVBS(np.where(np.isneginf(sv), np.nan, sv), er, cs.d["ping_time"], cs.range_bin,
                                           cs.ping_time_bin)
    n = int((np.isfinite(sv[c]) & (ogrid.bin_index(er[c], ogrid.range_edges(er, 4.9)) == m["neg_and_finite"])
             & (np.arange(nc.P) // 6 == tb)[:, None]).sum())
    np.testing.assert_allclose(finite_only[c, tb, m["neg_and_finite"]] - mv[c, tb, m["neg_and_finite"]],
                               10 * np.log10((n + 2) / n), rtol=1e-9)


@pytest.mark.parametrize("S", nc.SIZES)
def test_overflow_targets(S):
    cs = nc.build("overflow", S)
    sv, _ = cs.sv_er()
    assert np.isfinite(cs.raw).all() and np.isfinite(sv[:, :, 3:]).all()
    for c, p, s, target in cs.marks["spots"]:
        assert abs(sv[c, p, s] - target) < 2e-4 * max(1.0, abs(target) / 385.0)   # float32 raw: half an ulp of ~3000
    with np.errstate(over="ignore"):
        lin64 = 10 ** (sv / 10)
        lin32 = np.float32(10) ** (sv.astype(np.float32) / np.float32(10))
    assert np.isinf(lin64).sum() == 3 and np.isinf(lin32[np.isfinite(lin64)]).sum() == 3 + 2 + 3   # (385.0 dB is below the float32 limit)
    mv, _, _ = cs.mvbs()
    assert (nc.classes(mv) == 1).sum() == 3 + 1      # three single terms, and one bin whose two terms overflow as a sum
    assert np.nanmax(np.where(np.isfinite(mv), mv, np.nan)) > 3050.0   # (a 3082 dB term in a mean of ~150: -22 dB)


def test_expectations_are_shared_and_read_only():
    cs = nc.build("one_lane", 1024)
    assert cs.sv_er()[0] is cs.sv_er()[0] and not cs.sv_er()[0].flags.writeable and not cs.raw.flags.writeable
    n, c = cs.clean()
    assert n.shape == c.shape == cs.raw.shape
    mvi, er_min = cs.mvbs_index()
    assert mvi.shape == (nc.C, 4, -(-1024 // nc.RSN))
