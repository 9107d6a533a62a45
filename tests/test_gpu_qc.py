"""``qc`` on a real MI355X: ``exist_reversed_time``, ``coerce_increasing_time`` and ``check_and_correct_reversed_time``
against the restatement tests/qc_ref.py (itself held to the reference's executed results by tests/test_qc_host.py), bit
for bit: everything is int64 arithmetic, there is no tolerance.  The shapes are the smallest at which each piece can go
wrong: windows clipped at the start of the file, nested reversals, even windows with odd sums, the seams of the scan's
tiles and of its carry loop, more reversals than the median launch has wavefronts."""
import logging

import numpy as np
import pytest

import qc_cases as C
import qc_ref as R

pytestmark = pytest.mark.gpu

REPAIR_KERNELS = ["time_reversals_kernel", "reversal_medians_kernel", "time_tile_sums_kernel", "time_tile_carry_kernel",
                  "time_rebuild_kernel"]
T = C.SCAN_TILE


@pytest.fixture(scope="module")
def ep():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    import echopype_amd

    return echopype_amd


def dataset(ep, t, name="ping_time", resident=False):
    t = t.copy()
    t.flags.writeable = not resident
    return ep.Dataset(coords={name: t})


def repair(ep, t, win_len, resident=False):
    """-> the coordinate after coerce_increasing_time, and the kernels it launched."""
    from echopype_amd import _lib

    ds = dataset(ep, t, resident=resident)
    with _lib.launch_trace() as tr:
        assert ep.qc.coerce_increasing_time(ds, "ping_time", win_len) is None
    return ds["ping_time"].values, tr.kernels


def assert_ticks(got, want, dtype, what):
    assert got.dtype == dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    same = got.view(np.int64) == np.asarray(want).view(np.int64)
    assert same.all(), (what, int((~same).sum()), np.flatnonzero(~same)[:4], got.view(np.int64)[~same][:4],
                        np.asarray(want).view(np.int64)[~same][:4])


def check_case(ep, c, what, repeat=1):
    want = R.clean_reversed(c["t"], c["win_len"])
    for _ in range(repeat):
        got, kernels = repair(ep, c["t"], c["win_len"])
        assert kernels == REPAIR_KERNELS, kernels
        assert_ticks(got, want, c["t"].dtype, what)
    return got


# ---- 1. the worked example and the reference's executed results, through the public API ----------------------------------------
@pytest.mark.parametrize("win_len", [100, 2])
def test_the_worked_example(ep, win_len):
    t = np.array([0, 10, 20, 15, 25, 35, 30, 40], dtype=np.int64).view("datetime64[ns]")
    got, _ = repair(ep, t, win_len)
    assert got.view(np.int64).tolist() == [0, 10, 20, 30, 40, 50, 60, 70]


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_repair_equals_the_reference_executed_result(ep, name):
    from echopype_amd import _lib

    records, z = C.load_fixture()
    rec = next(r for r in records if r["name"] == name)
    t = z[f"case/{name}/in"]
    ds = dataset(ep, t)
    with _lib.launch_trace() as tr:
        assert ep.qc.exist_reversed_time(ds, "ping_time") is rec["exists"] is True
    assert tr.kernels == ["time_reversals_kernel"], tr.kernels  # one launch
    got, kernels = repair(ep, t, rec["win_len"])
    assert kernels == REPAIR_KERNELS, kernels
    assert_ticks(got, z[f"case/{name}/out"], t.dtype, name)
    assert_ticks(got, R.clean_reversed(t, rec["win_len"]), t.dtype, name + " (restatement)")
    assert ep.qc.exist_reversed_time(dataset(ep, got), "ping_time") is (not rec["sorted"])


# ---- 2. the window clipped at the start of the file -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CLIP) + list(C.CLIP_CAP))
def test_window_clipping(ep, name):
    """A single reversal at ni = 1, win_len - 1, win_len, win_len + 1 for win_len = 1, an even, an odd one and the cap;
    the intervals before it are all different, so a window that starts one difference off gives another median."""
    c = C.case(name)
    ni, w = C.CLIP.get(name) or C.CLIP_CAP[name]
    assert R.reversals(c["t"]) == [ni] and c["win_len"] == w
    t = R.ticks(c["t"])
    d = [t[i + 1] - t[i] for i in range(ni)]
    if ni > w:  # (a window that reached one difference further back would give another value)
        assert R.median(d[ni - w:]) != R.median(d[ni - w - 1:])
    got = check_case(ep, c, name).view(np.int64)
    assert got[ni + 1] - got[ni] == R.median(d[max(0, ni - w):])


# ---- 3. reversals inside each other's windows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name, ni, original, substituted", [("nested_w4", 4, 14, 17), ("nested_w2", 3, 1, 11)])
def test_nested_reversals_use_the_original_differences(ep, name, ni, original, substituted):
    got = check_case(ep, C.case(name), name).view(np.int64)
    assert got[ni + 1] - got[ni] == original != substituted


# ---- 4. an even window whose middle pair has an odd sum -------------------------------------------------------------------------
@pytest.mark.parametrize("name, ni, want", [("even_odd_positive", 2, 5), ("even_odd_negative", 3, -5),
                                            ("even_mixed_positive", 3, 2), ("even_mixed_negative", 3, -2)])
def test_even_window_truncates_toward_zero(ep, name, ni, want):
    got = check_case(ep, C.case(name), name).view(np.int64)
    assert got[ni + 1] - got[ni] == want


# ---- 5. the seams of the scan ------------------------------------------------------------------------------------------------------
def _seam_case(D, first, more=()):
    """D differences, the first reversal at ``first``, further ones at ``more``; irregular positive intervals."""
    rng = np.random.default_rng(D * 7 + first)
    d = rng.integers(900, 1100, D, dtype=np.int64)
    for i in (first, *more):
        d[i] = -int(rng.integers(1, 5000))
    return dict(t=C.from_diffs(d, C.T0_NS), win_len=9)


@pytest.mark.parametrize("D, first, more", [
    (T - 1, 3, (T - 2,)),                # one tile, not full; the last difference is a reversal
    (T, T - 1, ()),                      # one full tile; the first reversal is its last difference
    (T + 1, T - 1, (T,)),                # ... and the next tile holds one difference, a reversal
    (T + 1, T, ()),                      # the first reversal is the first difference of the second tile
    (2 * T + 1, T - 1, (T + 5, 2 * T)),  # three tiles; reversals either side of both seams
    (2 * T + 1, T, (2 * T - 1,)),
    (2 * T + 1, 2 * T, ()),              # everything but the last time is a copy
])
def test_scan_seams(ep, D, first, more):
    c = _seam_case(D, first, more)
    assert R.reversals(c["t"]) == sorted((first, *more)) and len(c["t"]) == D + 1
    got = check_case(ep, c, f"D={D} first={first}")
    assert np.array_equal(got[:first + 1], c["t"][:first + 1])


def test_more_tiles_than_the_carry_workgroup_has_threads(ep):
    """The one large case (2 MB of times): 256 + 2 tiles, so the workgroup that scans the tile sums makes a second round,
    with two tiles; reversals in the first tile, either side of the seam between the two rounds and in the last tile."""
    D = (C.CARRY_THREADS + 1) * T + 17
    c = _seam_case(D, 700, (C.CARRY_THREADS * T - 1, C.CARRY_THREADS * T, C.CARRY_THREADS * T + 1, D - 1))
    assert (D + T - 1) // T == C.CARRY_THREADS + 2
    check_case(ep, c, "many tiles")


# ---- 6. more reversals than the median launch has wavefronts -------------------------------------------------------------------
def test_more_reversals_than_wavefronts(ep):
    """Every third difference is a reversal, win_len = 7: each window holds two other reversals, and there are two full
    rounds of the fixed grid's wavefronts plus a part of a third, in whatever order the list was filled.  Twice, with the
    same bits."""
    count = 2 * C.MEDIAN_WAVES + 100 + 3
    rng = np.random.default_rng(6)
    d = rng.integers(20, 90, 3 * count, dtype=np.int64)
    d[2::3] = -rng.integers(1, 15, count, dtype=np.int64)
    c = dict(t=C.from_diffs(d, C.T0_NS), win_len=7)
    assert len(R.reversals(c["t"])) == count
    check_case(ep, c, "every third", repeat=2)


# ---- 7. realistic magnitudes, 8. another unit -------------------------------------------------------------------------------------
def test_epoch_nanoseconds(ep):
    c = C.case("epoch_ns")
    assert c["t"].view(np.int64).min() > 1.69e18 and np.median(np.diff(c["t"].view(np.int64))) > 9e8
    got = check_case(ep, c, "epoch_ns")
    assert R.is_sorted_and_valid(got)


def test_microsecond_coordinate_keeps_its_unit(ep):
    c = C.case("epoch_us")
    assert c["t"].dtype == np.dtype("datetime64[us]")
    got = check_case(ep, c, "epoch_us")
    assert got.dtype == np.dtype("datetime64[us]")
    # the repaired step is a truncated half of an odd sum of microseconds: in nanoseconds the same file gives 500 ns more
    (ni,) = R.reversals(c["t"])
    as_ns = R.clean_reversed(c["t"].astype("datetime64[ns]"), c["win_len"])
    step = int(got.view(np.int64)[ni + 1] - got.view(np.int64)[ni])
    assert int(as_ns[ni + 1] - as_ns[ni]) == step * 1000 + 500


# ---- 9. errors and no-ops -----------------------------------------------------------------------------------------------------------
def test_no_reversal_and_short_coordinates_are_left_alone(ep):
    from echopype_amd import _lib

    for t in (C.case("no_reversal")["t"], C.case("no_reversal")["t"][:1], C.case("no_reversal")["t"][:0]):
        ds = dataset(ep, t)
        before_da, before = ds["ping_time"], ds["ping_time"].values
        with _lib.launch_trace() as tr:
            assert ep.qc.exist_reversed_time(ds, "ping_time") is False
            ep.qc.coerce_increasing_time(ds)
            assert ep.qc.check_and_correct_reversed_time(ds, "ping_time", "Sonar/Beam_group1") is None
        assert ds["ping_time"] is before_da and ds["ping_time"].values is before  # the same coordinate object
        assert tr.kernels == (["time_reversals_kernel"] * 3 if len(t) >= 2 else []), tr.kernels
    assert ep.qc.check_and_correct_reversed_time(ds, "time9", "Platform") is None  # no such coordinate


def test_reversed_first_difference_raises_index_error(ep):
    ds = dataset(ep, C.case("first_difference")["t"])
    assert ep.qc.exist_reversed_time(ds, "ping_time") is True
    before = ds["ping_time"].values
    with pytest.raises(IndexError, match="window before it is empty"):
        ep.qc.coerce_increasing_time(ds)
    assert ds["ping_time"].values is before


@pytest.mark.parametrize("name", sorted(C.NAT_CASES))
def test_nat(ep, name):
    t = C.nat_case(name)
    ds = dataset(ep, t)
    assert ep.qc.exist_reversed_time(ds, "ping_time") is R.exist_reversed(t) is C.NAT_CASES[name][1]
    with pytest.raises(ValueError, match="contains NaT"):
        ep.qc.coerce_increasing_time(ds)
    assert ds["ping_time"].values.view(np.int64).tolist() == t.view(np.int64).tolist()


def test_refused_arguments(ep):
    ds = dataset(ep, C.case("worked_w2")["t"])
    ds2 = ep.Dataset(coords={"ping_time": np.array([0.0, 2.0, 1.0])})
    with pytest.raises(ValueError, match="win_len must be at least 1"):
        ep.qc.coerce_increasing_time(ds, win_len=0)
    with pytest.raises(NotImplementedError, match=f"up to {C.MAX_WIN} "):
        ep.qc.coerce_increasing_time(ds, win_len=C.MAX_WIN + 1)
    for fn in (ep.qc.coerce_increasing_time, ep.qc.exist_reversed_time):
        with pytest.raises(TypeError, match="not a datetime64 coordinate"):
            fn(ds2, "ping_time")
    assert ds["ping_time"].values.view(np.int64).tolist() == [0, 10, 20, 15, 25, 35, 30, 40]


def test_ops_check_their_arguments(ep):
    import torch

    t = torch.tensor([0, 10, 5, 20], dtype=torch.int64, device="cuda")
    facts, lst = ep.ops.time_reversals(t, want_list=True)
    assert facts.tolist() == [1, 1, 0, 1] and lst[:1].tolist() == [1]
    assert ep.ops.time_reversals(t)[0].tolist() == [1, 1, 0, 0] and ep.ops.time_reversals(t)[1] is None
    assert ep.ops.time_reversals(t[:2])[0].tolist() == [-1, 0, 0, 0]
    with pytest.raises(ValueError, match="1-D int64"):
        ep.ops.time_reversals(t.double())
    with pytest.raises(ValueError, match=f"1 .. {C.MAX_WIN} are served"):
        ep.ops.reversal_medians(t, facts, lst, C.MAX_WIN + 1)
    with pytest.raises(ValueError, match="at least 2 are needed"):
        ep.ops.time_rebuild(t[:1], facts, lst)
    # without a reversal the rebuild is a copy
    sorted_t = torch.tensor([3, 4, 9], dtype=torch.int64, device="cuda")
    f2, l2 = ep.ops.time_reversals(sorted_t, want_list=True)
    assert ep.ops.time_rebuild(sorted_t, f2, ep.ops.reversal_medians(sorted_t, f2, l2, 5)).tolist() == [3, 4, 9]


# ---- 10. residency --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["worked_w2", "negative_median"])
def test_repaired_resident_coordinate_stays_resident(ep, name, monkeypatch):
    """A coordinate that cannot be written to (resident, EchoData.to_device): its device copy is the one ops already
    holds, the repaired array cannot be written to either and is known to ops.ping_time_facts with the rebuilt tensor --
    the very object -- and the device's verdict on it: sorted for the first case, not for the one whose median stays
    negative."""
    from echopype_amd import _lib, ops

    c = C.case(name)
    ds = dataset(ep, c["t"], resident=True)
    old = ds["ping_time"].values
    _, ok_old, dev_old = ops.ping_time_facts(old)
    assert not ok_old and not old.flags.writeable
    registered = []
    real_register, real_upload = ops.register_ping_time, ops.to_device
    monkeypatch.setattr(ops, "register_ping_time", lambda a, t, ok: (registered.append((a, t, ok)), real_register(a, t, ok))[1])
    monkeypatch.setattr(ops, "to_device", lambda *a, **k: pytest.fail("a resident coordinate was uploaded again"))
    with _lib.launch_trace() as tr:
        ep.qc.coerce_increasing_time(ds, "ping_time", c["win_len"])
    assert tr.kernels == REPAIR_KERNELS + ["time_reversals_kernel"], tr.kernels  # (the verdict: a second run on the result)
    new = ds["ping_time"].values
    assert new is not old and not new.flags.writeable and new.dtype == old.dtype
    want = R.clean_reversed(c["t"], c["win_len"])
    assert_ticks(new, want, c["t"].dtype, name)
    (arr, tensor, ok), = registered
    assert arr is new and ok is R.is_sorted_and_valid(want) is (name == "worked_w2")
    with _lib.launch_trace() as tr:
        ns, ok_new, dev_new = ops.ping_time_facts(new)  # (to_device still fails: nothing goes up)
    assert tr.kernels == [] and dev_new is tensor and dev_new is not dev_old and ok_new is ok
    assert np.array_equal(ns, want) and np.array_equal(dev_new.cpu().numpy(), want)
    monkeypatch.setattr(ops, "to_device", real_upload)
    # a coordinate that can be written to gives one that can, and ops looks at it like at any other
    got, _ = repair(ep, c["t"], c["win_len"])
    assert got.flags.writeable and bool(ops.ping_time_facts(got, want_device=False)[1]) is ok


# ---- 11. end to end -------------------------------------------------------------------------------------------------------------------
def test_repaired_echodata_goes_through_compute_Sv_and_compute_MVBS(ep, caplog):
    from echopype_amd import ops
    from echopype_amd.echodata import BEAM1, from_ek60_arrays

    d = ep.synth.ek60_numpy(C=2, P=300, S=64)
    bad = np.asarray(d["ping_time"], dtype="datetime64[ns]").copy()
    bad[150] -= np.timedelta64(2_500_000_000, "ns")  # one ping 2.5 s early: earlier than the two pings before it
    ed = from_ek60_arrays(dict(d, ping_time=bad)).to_device()
    assert ep.qc.exist_reversed_time(ed[BEAM1], "ping_time") is True
    assert not ops.ping_time_facts(ed[BEAM1]["ping_time"].values)[1]
    with caplog.at_level(logging.WARNING, logger="echopype_amd.qc"):
        old = ep.qc.check_and_correct_reversed_time(ed[BEAM1], "ping_time", BEAM1)
        old_env = ep.qc.check_and_correct_reversed_time(ed["Environment"], "time1", "Environment")
    messages = [r.getMessage() for r in caplog.records if r.name == "echopype_amd.qc"]
    assert len(messages) == 2 and messages[0].startswith(f"{BEAM1}: ping_time steps backwards"), messages
    assert np.array_equal(old.values, bad) and np.array_equal(old_env.values, bad) and old.dims == ("ping_time",)
    fixed = ed[BEAM1]["ping_time"].values
    want = R.clean_reversed(bad, 100)
    assert_ticks(fixed, want, bad.dtype, "ping_time")
    assert_ticks(ed["Environment"]["time1"].values, want, bad.dtype, "time1")
    assert R.is_sorted_and_valid(want) and ops.ping_time_facts(fixed)[1] and not fixed.flags.writeable
    assert ep.qc.exist_reversed_time(ed[BEAM1], "ping_time") is False

    direct = from_ek60_arrays(dict(d, ping_time=want.view("datetime64[ns]"))).to_device()
    results = []
    for e in (ed, direct):
        sv = ep.calibrate.compute_Sv(e)
        mvbs = ep.commongrid.compute_MVBS(sv, range_bin="2m", ping_time_bin="20s")
        results.append((sv, mvbs))
    (sv_a, mv_a), (sv_b, mv_b) = results
    for a, b in ((sv_a, sv_b), (mv_a, mv_b)):
        assert np.array_equal(a["ping_time"].values, b["ping_time"].values)
        for v in ("Sv", "echo_range"):
            x, y = np.asarray(a[v].values, np.float64), np.asarray(b[v].values, np.float64)
            assert x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64)), v
    assert np.isfinite(mv_a["Sv"].values).any() and mv_a["Sv"].shape[1] >= 10
