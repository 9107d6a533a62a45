"""commongrid.regrid_Sv without a GPU: the export and its signature, the properties of the NumPy restatement of its rule
(tests/regrid_ref.py, the oracle of the kernel) on small rows, the grid it shares with compute_MVBS, every refusal of the
public function (they all come before any device access) and the refusals of the C entry."""
import inspect

import numpy as np
import pytest

from regrid_cases import grid, ranges, volume
from regrid_ref import cell_bounds, conserved_sides, regrid_ref, regrid_row_ref

NAN, INF = np.nan, np.inf


def test_export_and_signature():
    import echopype_amd as ep
    from echopype_amd import _lib, ops

    assert "regrid_Sv" in ep.commongrid.__all__ and callable(ops.regrid_rows)
    P = inspect.Parameter
    kw = P.POSITIONAL_OR_KEYWORD
    assert inspect.signature(ep.commongrid.regrid_Sv) == inspect.Signature([
        P("ds_Sv", kw), P("range_var", kw, default="echo_range"), P("range_bin", kw, default="0.2m"),
        P("range_var_max", kw, default=None), P("with_coverage", kw, default=True), P("device", P.KEYWORD_ONLY, default=None)])
    assert len(_lib.SIGNATURES["epa_regrid_rows"]) == 17 and hasattr(_lib.lib, "epa_regrid_rows")
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "echopype_amd.h")).read()
    assert f"#define EPA_REGRID_TILE {_lib.REGRID_TILE} " in header
    assert "regrid_Sv" in ep.mask.frequency_differencing.__doc__


# ---- the oracle's own properties ---------------------------------------------------------------------------------------------
def test_identity_on_a_coinciding_power_of_two_grid():
    """Samples at (i + 1/2) / 4: their cells are [i / 4, (i + 1) / 4), the grid's own.  All arithmetic on the bounds is
    exact, so coverage is exactly 1 and Sv comes back to the rounding of 10^x and log10."""
    S = 64
    r = (np.arange(S) + 0.5) * 0.25
    v = np.random.default_rng(1).uniform(-90, -30, S)
    e = grid(r.max(), 0.25)
    assert len(e) - 1 == S
    sv, cov, bad = regrid_row_ref(r, v, e)
    assert not bad and (cov == 1.0).all()
    np.testing.assert_allclose(sv, v, rtol=0, atol=1e-12)
    # float32 input: the same after the one rounding
    sv32, cov32, _ = regrid_ref(v.astype(np.float32)[None, None], r.astype(np.float32), e)
    assert sv32.dtype == np.float32 and (cov32 == 1.0).all()
    np.testing.assert_array_equal(sv32[0, 0], v.astype(np.float32))


def test_a_source_cell_split_into_k_output_cells_gives_k_equal_values():
    r = np.array([0.5, 1.5, 2.5])
    v = np.array([-70.0, -50.0, -60.0])
    for k in (2, 4, 7):
        e = np.arange(3 * k + 1) / k  # k cells per source cell, exactly on its bounds for k a power of two
        sv, cov, _ = regrid_row_ref(r, v, e)
        np.testing.assert_allclose(cov, 1.0, rtol=0, atol=1e-14)
        for i in range(3):
            part = sv[i * k:(i + 1) * k]
            assert (part == part[0]).all(), (k, i)
            np.testing.assert_allclose(part[0], v[i], rtol=0, atol=1e-12)


def test_an_aligned_four_to_one_coarsening_is_the_mean_of_the_linear_values():
    S = 32
    r = (np.arange(S) + 0.5) * 0.125
    v = np.random.default_rng(2).uniform(-90, -30, S)
    sv, cov, _ = regrid_row_ref(r, v, grid(r.max(), 0.5))
    want = 10 * np.log10((10 ** (v / 10)).reshape(-1, 4).mean(axis=1))
    assert sv.size == S // 4 and (cov == 1.0).all()
    np.testing.assert_allclose(sv, want, rtol=0, atol=1e-12)
    # a NaN sample leaves the mean of the other three and a coverage of 3/4
    v[5] = NAN
    sv, cov, _ = regrid_row_ref(r, v, grid(r.max(), 0.5))
    assert cov[1] == 0.75 and np.isclose(sv[1], 10 * np.log10(np.mean(10 ** (v[[4, 6, 7]] / 10))), rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", ["irregular", "nan_runs", "cut_by_range_var_max", "one_cell", "fine"])
def test_the_echo_integral_is_conserved(case):
    sv, r = volume(7, 3, 2, 97, np.float64, np.float64)
    rmax = r.max()
    if case == "irregular":
        e = grid(rmax, 0.2)
    elif case == "nan_runs":  # a run that swallows whole cells and parts of their neighbours
        sv[:, :, 20:41] = NAN
        e = grid(rmax, 0.05)
    elif case == "cut_by_range_var_max":  # the last edge lies inside a sample's cell, in every channel
        e = grid(1.003 + 1e-8, 0.1)
        for c in range(3):
            _, m = cell_bounds(r[c])
            assert ((m[:-1] < e[-1]) & (e[-1] < m[1:])).any()
    elif case == "one_cell":
        e = grid(1e-3, 1000.0)
        assert len(e) == 2
    else:
        e = grid(rmax, 0.03)
    lhs, rhs = conserved_sides(sv, r, e)
    assert np.isfinite(rhs).all() and (rhs > 0).all()
    print(case, "largest relative difference", np.max(np.abs(lhs - rhs) / rhs))
    assert (np.abs(lhs - rhs) <= 1e-12 * rhs).all()
    got, cov, bad = regrid_ref(sv, r, e)
    assert bad == 0 and cov.max() <= 1 + 1e-12
    if case == "nan_runs":
        assert np.isnan(got).any() and ((cov > 0) & (cov < 0.999)).any()


def test_refused_rows_zero_width_cells_and_infinities():
    e = grid(3.0, 0.5)
    J = len(e) - 1
    for r in ([1.0, 2.0, 1.5, 3.0], [1.0, NAN, 2.0, 3.0], [NAN, 1.0, 2.0, 3.0], [INF, 1.0, 2.0, 3.0], [2.0, 1.0, NAN, 0.5]):
        sv, cov, bad = regrid_row_ref(r, [-50.0] * 4, e)
        assert bad and np.isnan(sv).all() and (cov == 0).all() and sv.size == J, r
    # a decrease behind the finite run does not count; equal ranges are in order
    sv, cov, bad = regrid_row_ref([1.0, 2.0, NAN, 0.5], [-50.0] * 4, e)
    assert not bad and cell_bounds([1.0, 2.0, NAN, 0.5])[0] == 2
    np.testing.assert_allclose(sv[1:5], -50.0, rtol=0, atol=1e-12)
    assert np.isnan(sv[0]) and np.isnan(sv[5]) and cov.tolist() == [0, 1, 1, 1, 1, 0]
    # three leading zeros: samples 0 and 1 have no width, sample 2 stands for [0, 0.25)
    n, m = cell_bounds([0.0, 0.0, 0.0, 0.5, 1.0])
    assert n == 5 and m.tolist() == [0.0, 0.0, 0.0, 0.25, 0.75, 1.25]
    sv, cov, bad = regrid_row_ref([0.0, 0.0, 0.0, 0.5, 1.0], [INF, NAN, -40.0, -50.0, -60.0], grid(1.0, 0.25))
    assert not bad and cov.tolist() == [1, 1, 1, 1]
    np.testing.assert_allclose(sv, [-40, -50, -50, -60], rtol=0, atol=1e-12)
    # -inf is a sample of linear value 0, +inf gives +inf; a cell of NaN samples alone is NaN with coverage 0
    r = (np.arange(6) + 0.5) * 0.5
    sv, cov, _ = regrid_row_ref(r, [-INF, -INF, -INF, -50.0, INF, NAN], grid(r.max(), 0.5))
    assert sv[0] == -INF and sv[4] == INF and np.isnan(sv[5]) and cov.tolist() == [1, 1, 1, 1, 1, 0]
    sv, cov, _ = regrid_row_ref(r, [-INF, -INF, -INF, -50.0, INF, NAN], grid(r.max(), 1.0))
    assert sv[0] == -INF and np.isclose(sv[1], -50 - 10 * np.log10(2)) and sv[2] == INF and cov.tolist() == [1, 1, 0.5]
    # the count of a volume
    sv, r3 = volume(3, 3, 2, 9, np.float32, np.float32, form="CPS")
    r3[1, 0, 3] = 0.0
    r3[2, 1, 1:] = NAN
    assert regrid_ref(sv, r3, grid(1.0, 0.1))[2] == 2


def test_the_grid_is_that_of_compute_MVBS():
    from echopype_amd.commongrid.deferred import n_range_bins, range_cap, range_edges

    for rmax, rb in ((93.97, 0.2), (250.0, 1.0), (0.0, 5.0), (17.3, 0.188), (1e-3, 1000.0)):
        e = range_edges(rmax, rb)
        np.testing.assert_array_equal(e, grid(rmax, rb))
        np.testing.assert_array_equal(e, np.arange(len(e)) * rb)  # what the kernel takes for the edges
        assert len(e) - 1 == n_range_bins(rmax, rb)
    assert range_cap("250m", None) == 250.0 + 1e-8 and range_cap(None, None) is None
    assert len(range_edges(NAN, 1.0)) == 1
    assert ranges(3, 5, 0).shape == (3, 5)


# ---- the public function: refusals, all before any device access ----------------------------------------------------------------
C_, P_, S_ = 2, 3, 4
DIMS = ("channel", "ping_time", "range_sample")


def _ds(order=DIMS, range_dims=None):
    from echopype_amd.xr_lite import Dataset

    sizes = dict(zip(DIMS, (C_, P_, S_)))
    ds = Dataset(coords={"channel": np.array(["a", "b"]), "range_sample": np.arange(S_),
                         "ping_time": np.datetime64("2026-01-01", "ns") + np.arange(P_) * np.timedelta64(1, "s")})
    ds["Sv"] = (order, np.zeros(tuple(sizes[d] for d in order)))
    rd = range_dims if range_dims is not None else order
    ds["echo_range"] = (rd, np.zeros(tuple(sizes.get(d, 2) for d in rd)))
    return ds


def test_refusals_of_the_public_function(monkeypatch):
    import torch

    import echopype_amd as ep
    from echopype_amd import ops
    from echopype_amd.xr_lite import DataArray

    def no_device(*a, **k):
        raise AssertionError("a refusal must come before any device access")

    monkeypatch.setattr(ops, "regrid_rows", no_device)
    monkeypatch.setattr(ops, "to_device", no_device)
    monkeypatch.setattr(ops, "nanminmax", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    rg = ep.commongrid.regrid_Sv
    with pytest.raises(TypeError, match="range_var must be a string"):
        rg(_ds(), range_var=3)
    with pytest.raises(ValueError, match="range_var must be one of 'echo_range' or 'depth'"):
        rg(_ds(), range_var="range_sample")
    with pytest.raises(ValueError, match="must contain all of the following variables"):
        rg(_ds(), range_var="depth")
    with pytest.raises(ValueError, match="must contain all of the following variables"):
        rg(_ds().drop_vars("Sv"))
    with pytest.raises(TypeError, match="range_bin must be a string"):
        rg(_ds(), range_bin=0.2)
    with pytest.raises(ValueError, match="Range bin must be in meters"):
        rg(_ds(), range_bin="0.2km")
    with pytest.raises(ValueError, match="Range bin must be in meters"):
        rg(_ds(), range_bin="-1m")
    for zero in ("0m", "0.0m"):
        with pytest.raises(ValueError, match="range_bin must be positive"):
            rg(_ds(), range_bin=zero)
    with pytest.raises(TypeError, match="must be a string"):
        rg(_ds(), range_var_max=250.0)
    with pytest.raises(ValueError, match="Range bin must be in meters"):
        rg(_ds(), range_var_max="far")
    for order in (("ping_time", "channel", "range_sample"), ("channel", "range_sample", "ping_time")):
        with pytest.raises(NotImplementedError, match="the dimensions of Sv must be"):
            rg(_ds(order))
    with pytest.raises(ValueError, match="and include 'range_sample'"):
        rg(_ds(range_dims=("channel", "ping_time")))
    with pytest.raises(ValueError, match="must be among those of Sv"):
        rg(_ds(range_dims=("beam", "range_sample")))
    ds = _ds()
    ds.data_vars["echo_range"] = DataArray(np.zeros(S_ + 1), ("range_sample",))  # (past the Dataset's own check)
    with pytest.raises(ValueError, match="does not match Sv"):
        rg(ds)
    ds = _ds()
    ds["echo_range"] = (("range_sample",), np.zeros(S_, dtype=complex))
    with pytest.raises(TypeError, match="echo_range must hold real numbers"):
        rg(ds)


# ---- the C entry and its wrapper ----------------------------------------------------------------------------------------------
def _call(sv=8, dtype=1, range=8, range_dtype=0, strides=(0, 0, 1), shape=(1, 1, 1), range_bin=0.2, n_rbins=1, sv_out=8,
          cov=None, counter=8, max_grid=0):
    from echopype_amd import _lib

    _lib.call("epa_regrid_rows", sv, dtype, range, range_dtype, *strides, *shape, range_bin, n_rbins, sv_out, cov, counter,
              max_grid, None)


def test_the_library_refuses_bad_arguments_before_any_hip_call():
    for bad in (-1, 2, 7):
        with pytest.raises(ValueError, match=f"epa_regrid_rows: bad dtype {bad}"):
            _call(dtype=bad)
        with pytest.raises(ValueError, match=f"epa_regrid_rows: bad range dtype {bad}"):
            _call(range_dtype=bad)
    for shape in ((1, -1, 1), (-1, 1, 1), (1, 1, (1 << 30) + 1)):
        with pytest.raises(ValueError, match="bad shape"):
            _call(shape=shape)
    for n in (-1, (1 << 30) + 1):
        with pytest.raises(ValueError, match="bad grid"):
            _call(n_rbins=n)
    for rb in (0.0, -0.2, NAN, INF):
        with pytest.raises(ValueError, match="range_bin must be positive and finite"):
            _call(range_bin=rb)
    with pytest.raises(ValueError, match="strides must not be negative"):
        _call(strides=(0, -1, 1))
    with pytest.raises(ValueError, match="max_grid must not be negative"):
        _call(max_grid=-1)
    with pytest.raises(ValueError, match="n_unordered_out is NULL"):
        _call(counter=None)
    with pytest.raises(ValueError, match="NULL array argument"):
        _call(sv=None)
    with pytest.raises(ValueError, match="NULL array argument"):
        _call(range=None)
    with pytest.raises(ValueError, match="sv_out is NULL"):
        _call(sv_out=None)


def test_the_wrapper_refuses_before_it_calls():
    import torch

    from echopype_amd import ops

    with pytest.raises(ValueError, match=r"sv must be float32 / float64 of shape \(C, P, S\)"):
        ops.regrid_rows(torch.zeros(2, 3), torch.zeros(3), 0.2, 1)
    with pytest.raises(ValueError, match=r"sv must be float32 / float64 of shape \(C, P, S\)"):
        ops.regrid_rows(torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(3), 0.2, 1)
    with pytest.raises(ValueError, match="range must be a float32 / float64 tensor on"):
        ops.regrid_rows(torch.zeros(1, 2, 3), torch.zeros(3, dtype=torch.int64), 0.2, 1)
