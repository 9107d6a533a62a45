""" "echo metrics" with the reference's signatures (echopype metrics/summary_statistics.py; Urmy et al. 2012, Measuring
the vertical distributional variability of pelagic fauna in Monterey Bay, ICES J. Mar. Sci. 69 (2): 184-196).

Per row -- every dimension of ``Sv`` but ``range_sample`` -- and for samples j = 1 .. S-1, with r = ``ds[range_label]``:
``dz_j = r_j - r_{j-1}`` in r's own type, a zero becoming NaN; ``sv_j = 10 ** (Sv_j / 10)``; ``w_j = sv_j dz_j``;
``A = sum w_j``, ``B = sum r_j w_j``, ``Q = sum sv_j**2 dz_j``, ``I = sum (r_j - cm)**2 w_j``, every sum skipping its
NaN terms (xarray's ``sum``: an all-NaN row sums to 0).  Sample 0 takes part in nothing: ``diff`` labels its result by the
upper sample and the products join on the labels.  +-inf, negative dz and 0/0 follow IEEE.

    abundance = 10 log10 A    center_of_mass = B / A    dispersion = I / A    evenness = A**2 / Q    aggregation = Q / A**2

The five statistics are one call of ``epa_echo_metrics`` each, asking for what they return; ``summary`` returns all five
from a single sweep over ``Sv`` and the range.  ``dispersion`` keeps the reference's quirk: its centre of mass is taken
on ``echo_range`` whatever ``range_label`` names (two calls then, and ``echo_range`` must be in the dataset).

Inputs: any dimensions as long as ``range_sample`` is one of them; it is moved last and the others are flattened to rows.
The range variable has the dimensions of ``Sv`` in any order, or ``range_sample`` alone (read as one row shared by all,
never expanded); any other subset of Sv's dimensions is expanded to the cube on the device first (one more write and
read of an Sv-sized array).  Anything but float32 / float64 becomes float64; ``Sv`` and a range of different float types
are both taken as float64.  A lazy ``echo_range`` left by ``compute_Sv`` is written once, by reading it.  Results are
DataArrays over the remaining dimensions with their coordinates, in the type of the inputs, and stay on the device.
Host synchronisations: none."""
from collections import namedtuple

import torch

from .. import ops
from ..device_view import device_view
from ..xr_lite import DataArray, Dataset, DeviceArray, xarray_io

_Rows = namedtuple("_Rows", "sv range dims shape coords")


def _range_var(ds, range_label):
    if range_label not in ds:
        raise ValueError(f"{range_label} not in the input Dataset!")
    return ds[range_label]


def _rows(ds, range_label, Sv_label="Sv"):
    """``Sv`` as (R, S) rows and the range as (R, S) or (S,), both on the device in one float type."""
    r_da = _range_var(ds, range_label)
    sv_da = ds[Sv_label]
    if "range_sample" not in sv_da.dims:
        raise ValueError(f"{Sv_label} must have the dimension 'range_sample', it has {sv_da.dims}")
    if "range_sample" not in r_da.dims or not set(r_da.dims) <= set(sv_da.dims):
        raise ValueError(f"{range_label} must have the dimension 'range_sample' and no dimension that {Sv_label} lacks: "
                         f"it has {r_da.dims}, {Sv_label} has {sv_da.dims}")
    rest = tuple(d for d in sv_da.dims if d != "range_sample")
    order = rest + ("range_sample",)
    sv = device_view(sv_da, order, floating=True)
    rg = device_view(r_da, order, device=sv.device, floating=True)
    if sv.dtype != rg.dtype:
        sv, rg = sv.double(), rg.double()
    shape = tuple(sv.shape[:-1])
    S = sv.shape[-1]
    if rg.dim() not in (1, sv.dim()):  # a subset of the dimensions: expanded to the cube
        have = [d for d in order if d in r_da.dims]
        rg = rg[tuple(slice(None) if d in have else None for d in order)].expand(sv.shape).contiguous()
    coords = {k: v for k, v in sv_da.coords.items() if k in rest}
    return _Rows(sv.reshape(-1, S), rg if rg.dim() == 1 else rg.reshape(-1, S), rest, shape, coords)


def _statistics(ds, range_label, want):
    # the reference's dispersion calls center_of_mass(ds) without its range_label
    two = "dispersion" in want and range_label != "echo_range"
    _range_var(ds, range_label)  # (what is missing is said before anything is sent to the device)
    if two:
        _range_var(ds, "echo_range")
    rows = _rows(ds, range_label)
    cm = None
    if two:
        base = _rows(ds, "echo_range")
        cm = ops.echo_metrics(base.sv, base.range, want=("center_of_mass",))["center_of_mass"].double()
    out = ops.echo_metrics(rows.sv, rows.range, cm=cm, want=want)
    return {w: DataArray(DeviceArray(out[w].reshape(rows.shape)), rows.dims, coords=rows.coords, name=w) for w in want}


@xarray_io()
def delta_z(ds, range_label="echo_range"):
    """Widths between range samples ``ds[range_label].diff("range_sample")`` with zeros as NaN, labelled by the upper
    sample.  A helper, not the hot path (a torch expression on the device): the statistics take dz inside their sweep."""
    r_da = _range_var(ds, range_label)
    t = device_view(r_da, r_da.dims, floating=True)
    dz = torch.diff(t, dim=r_da.dims.index("range_sample"))
    dz = torch.where(dz != 0, dz, torch.full_like(dz, float("nan")))
    coords = {k: (v[1:] if k == "range_sample" else v) for k, v in r_da.coords.items() if k in r_da.dims}
    return DataArray(DeviceArray(dz), r_da.dims, coords=coords, name=range_label)


@xarray_io()
def convert_to_linear(ds, Sv_label="Sv"):
    """``10 ** (ds[Sv_label] / 10)``: volume backscattering strength in the linear domain.  A helper, not the hot path
    (a torch expression on the device)."""
    sv_da = ds[Sv_label]
    t = device_view(sv_da, sv_da.dims, floating=True)
    coords = {k: v for k, v in sv_da.coords.items() if k in sv_da.dims}
    return DataArray(DeviceArray(torch.pow(10.0, t / 10)), sv_da.dims, coords=coords, name=Sv_label)


@xarray_io()
def abundance(ds, range_label="echo_range"):
    """Area backscattering strength Sa [dB re 1 m^2 m^-2]: ``10 log10 sum(sv dz)``, the integral of volume backscatter
    over range.  One sweep over ``Sv`` and the range."""
    return _statistics(ds, range_label, ("abundance",))["abundance"]


@xarray_io()
def center_of_mass(ds, range_label="echo_range"):
    """Mean backscatter location [m]: ``sum(r sv dz) / sum(sv dz)``.  One sweep over ``Sv`` and the range."""
    return _statistics(ds, range_label, ("center_of_mass",))["center_of_mass"]


@xarray_io()
def dispersion(ds, range_label="echo_range"):
    """Inertia [m^2]: ``sum((r - cm)**2 sv dz) / sum(sv dz)``, the spread of backscatter about the centre of mass, taken
    about the computed cm term by term (not from raw moments).  As in the reference, cm is ``center_of_mass(ds)`` on
    ``echo_range`` whatever ``range_label`` names: with another label this is two sweeps, and ``echo_range`` must be in
    the dataset."""
    return _statistics(ds, range_label, ("dispersion",))["dispersion"]


@xarray_io()
def evenness(ds, range_label="echo_range"):
    """Equivalent area EA [m]: ``sum(sv dz)**2 / sum(sv**2 dz)``, the area that would be occupied if all cells held the
    mean density.  One sweep over ``Sv`` and the range."""
    return _statistics(ds, range_label, ("evenness",))["evenness"]


@xarray_io()
def aggregation(ds, range_label="echo_range"):
    """Index of aggregation IA [m^-1]: ``1 / evenness``.  One sweep over ``Sv`` and the range."""
    return _statistics(ds, range_label, ("aggregation",))["aggregation"]


@xarray_io()
def summary(ds, range_label="echo_range"):
    """All five statistics as one Dataset (variables ``abundance``, ``center_of_mass``, ``dispersion``, ``evenness``,
    ``aggregation``) from a single sweep over ``Sv`` and the range -- bit for bit what the five functions return.  With
    ``range_label`` other than ``"echo_range"`` a second sweep takes the centre of mass ``dispersion`` is about."""
    out = _statistics(ds, range_label, ops.METRICS)
    res = Dataset()
    for w in ops.METRICS:
        res[w] = out[w]
    return res


__all__ = ["delta_z", "convert_to_linear", "abundance", "center_of_mass", "dispersion", "evenness", "aggregation", "summary"]
