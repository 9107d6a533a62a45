"""echopype_amd.device_view: the one place a dataset variable crosses to the device.

The helpers are checked on CPU tensors (``ops.to_device`` serves ``device="cpu"``, a ``DeviceArray`` can wrap a CPU
tensor); the ``gpu`` tests check what only a device shows -- no launch, no synchronisation, the current device -- and
every rewired entry point once: a variable in another dimension order, on the host or resident, gives exactly the
array the canonical order gives."""
import itertools

import numpy as np
import pytest

DIMS = ("channel", "ping_time", "range_sample")
SHAPE = (2, 3, 5)
PERMS = list(itertools.permutations(range(3)))
OTHER = (2, 0, 1)  # (range_sample, channel, ping_time)
DTYPES = ("float32", "float64", "int16")
INDEXES = (None, 1, [1, 0])


def _base(dtype):
    return (np.arange(30).reshape(SHAPE) * 3 - 40).astype(dtype)  # distinct values, exact in every dtype


def _var(a, perm, resident, device="cpu"):
    """The canonical (channel, ping_time, range_sample) array ``a`` stored in the dimension order ``perm``."""
    import torch

    from echopype_amd.xr_lite import DataArray, DeviceArray

    a = np.ascontiguousarray(a.transpose(perm))
    return DataArray(DeviceArray(torch.from_numpy(a).to(device)) if resident else a, tuple(DIMS[i] for i in perm))


def _indexed(a, index):
    return a if index is None else a[index]


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
@pytest.mark.parametrize("perm", PERMS, ids=lambda p: "".join(DIMS[i][0] for i in p))
def test_device_view_is_numpy_transpose_and_index(perm, resident):
    import torch

    from echopype_amd.device_view import device_view

    for dtype, index in itertools.product(DTYPES, INDEXES):
        base = _base(dtype)
        want = _indexed(base, index)
        t = device_view(_var(base, perm, resident), DIMS, device="cpu", index=index)
        assert t.is_contiguous() and t.dtype == getattr(torch, dtype)
        np.testing.assert_array_equal(t.numpy(), want)
        t = device_view(_var(base, perm, resident), DIMS, device="cpu", index=index, floating=True)
        assert t.is_contiguous() and t.dtype == (torch.float64 if dtype == "int16" else getattr(torch, dtype))
        np.testing.assert_array_equal(t.numpy(), want.astype(np.float64))
        for floating in (False, True):  # dtype= wins
            t = device_view(_var(base, perm, resident), DIMS, device="cpu", index=index, dtype=torch.float32,
                            floating=floating)
            assert t.is_contiguous() and t.dtype == torch.float32
            np.testing.assert_array_equal(t.numpy(), want.astype(np.float32))


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
def test_device_view_skips_the_dimensions_a_variable_lacks(resident):
    import torch

    from echopype_amd.device_view import device_view
    from echopype_amd.xr_lite import DataArray, DeviceArray

    for dtype in DTYPES:
        plane = _base(dtype)[0]  # (ping_time, range_sample)
        for dims, a in ((DIMS[1:], plane), (DIMS[:0:-1], np.ascontiguousarray(plane.T))):
            var = DataArray(DeviceArray(torch.from_numpy(a)) if resident else a, dims)
            t = device_view(var, DIMS, device="cpu", floating=True)
            assert t.is_contiguous() and t.dtype == (torch.float64 if dtype == "int16" else getattr(torch, dtype))
            np.testing.assert_array_equal(t.numpy(), plane)


def test_a_resident_variable_in_order_is_not_copied():
    import torch

    from echopype_amd.device_view import as_tensor, device_view
    from echopype_amd.xr_lite import DataArray, DeviceArray

    for dtype in ("float32", "float64"):
        t = torch.from_numpy(_base(dtype))
        var = DataArray(DeviceArray(t), DIMS)
        assert as_tensor(var) is t and as_tensor(var.data) is t and as_tensor(var, getattr(torch, dtype)) is t
        assert as_tensor(var, device=torch.device("cpu")) is t
        for kw in ({}, {"floating": True}, {"dtype": getattr(torch, dtype)}):
            v = device_view(var, DIMS, device="cpu", **kw)
            assert v.data_ptr() == t.data_ptr() and tuple(v.shape) == SHAPE
            s = device_view(var, DIMS, device="cpu", index=1, **kw)
            assert s.data_ptr() == t[1].data_ptr() and s.is_contiguous() and tuple(s.shape) == SHAPE[1:]
    # host data goes up once, converted on the way
    up = as_tensor(_base("int16"), torch.float64, device="cpu")
    assert up.dtype == torch.float64
    np.testing.assert_array_equal(up.numpy(), _base("float64"))


def test_a_lazy_variable_is_made_once():
    import torch

    from echopype_amd.device_view import device_view
    from echopype_amd.xr_lite import DataArray, LazyDeviceArray

    made = []

    def make():
        made.append(1)
        return torch.from_numpy(_base("float32").transpose(OTHER).copy())

    lazy = LazyDeviceArray(tuple(SHAPE[i] for i in OTHER), torch.float32, torch.device("cpu"), make)
    var = DataArray(lazy, tuple(DIMS[i] for i in OTHER))
    t = device_view(var, DIMS, device="cpu", index=1, floating=True)
    assert made == [1]
    np.testing.assert_array_equal(t.numpy(), _base("float32")[1])
    device_view(var, DIMS, device="cpu")
    assert made == [1]


def test_channel_position_compares_labels_as_strings():
    from echopype_amd.device_view import channel_position
    from echopype_amd.xr_lite import DataArray

    assert channel_position(np.array(["GPT 38", "GPT 120"]), "GPT 120") == 1  # np.str_ labels
    assert channel_position(["GPT 38", "GPT 120"], np.str_("GPT 38")) == 0   # plain str labels
    assert channel_position(np.array([38000, 120000]), "120000") == 1         # integer labels, by their str()
    assert channel_position(np.arange(3), 2) == 2
    assert channel_position(DataArray(np.array(["a", "b"]), ("channel",)), "b") == 1
    with pytest.raises(KeyError) as e:
        channel_position(np.array(["a", "b"]), "zz")
    assert e.value.args == ("zz",)


def test_broadcast_to_dims():
    from echopype_amd.device_view import broadcast_to_dims
    from echopype_amd.xr_lite import DataArray, Dataset

    ds = Dataset(coords={"channel": ["a", "b"], "ping_time": np.arange(3), "range_sample": np.arange(5)})
    full = DataArray(_base("float64"), DIMS)
    assert broadcast_to_dims(full, ds, DIMS) is full
    src = _base("float32")[:, 0, :]  # (channel, range_sample)
    out = broadcast_to_dims(DataArray(np.ascontiguousarray(src.T), ("range_sample", "channel")), ds, DIMS)
    assert tuple(out.dims) == DIMS and out.values.flags.c_contiguous
    np.testing.assert_array_equal(out.values, np.broadcast_to(src[:, None, :], SHAPE))
    out = broadcast_to_dims(DataArray(src[0], ("range_sample",)), ds, DIMS)
    np.testing.assert_array_equal(out.values, np.broadcast_to(src[0], SHAPE))
    swapped = np.ascontiguousarray(_base("float64").transpose(OTHER))
    out = broadcast_to_dims(DataArray(swapped, tuple(DIMS[i] for i in OTHER)), ds, DIMS)
    np.testing.assert_array_equal(out.values, _base("float64"))


# ---- on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_resident_variable_costs_no_launch_no_copy_no_synchronisation():
    import torch

    from echopype_amd import _lib
    from echopype_amd.device_view import as_tensor, device_view
    from echopype_amd.xr_lite import DataArray, DeviceArray

    cases = []
    for dtype in ("float32", "float64"):
        t = torch.from_numpy(_base(dtype)).cuda()
        cases.append((dtype, t, DataArray(DeviceArray(t), DIMS), _var(_base(dtype), OTHER, True, "cuda")))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with _lib.launch_trace() as trace:
            for dtype, t, var, swapped in cases:
                assert as_tensor(var) is t
                v, s = device_view(var, DIMS), device_view(var, DIMS, index=1)
                assert v.data_ptr() == t.data_ptr() and tuple(v.shape) == SHAPE
                assert s.data_ptr() == t[1].data_ptr() and s.is_contiguous()
                moved = device_view(swapped, DIMS, index=1, floating=True)  # a copy on the device: still no waiting
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert trace.kernels == []
    np.testing.assert_array_equal(moved.cpu().numpy(), _base("float64")[1])


@pytest.mark.gpu
def test_host_variable_arrives_on_the_current_device():
    import torch

    from echopype_amd.device_view import device_view, resolve_device

    here = torch.device("cuda", torch.cuda.current_device())
    assert resolve_device(None) == here and resolve_device("cpu") == torch.device("cpu")
    for index in INDEXES:
        t = device_view(_var(_base("int16"), OTHER, False), DIMS, index=index, floating=True)
        assert t.device == here and t.is_contiguous() and t.dtype == torch.float64
        np.testing.assert_array_equal(t.cpu().numpy(), _indexed(_base("float64"), index))


# ---- every rewired entry point: another dimension order, host or resident, gives the canonical order's array ---------
C, P, S = 2, 24, 40


def _scene(seed):
    """(C, P, S) float64 Sv with a bright band, a few raised pings and NaNs; depth 0.5 m per sample."""
    rng = np.random.default_rng(seed)
    sv = -80.0 + 3.0 * rng.standard_normal((C, P, S))
    sv[:, :, 28:32] = -30.0 + rng.standard_normal((C, P, 4))
    sv[:, 5:9, 10:16] = -55.0 + rng.standard_normal((C, 4, 6))
    sv[:, [7, 15], :] += 14.0
    sv[rng.random((C, P, S)) < 0.02] = np.nan
    depth = np.ascontiguousarray(np.broadcast_to(0.5 * np.arange(S), (C, P, S)))
    return sv, depth


def _dataset(arrays, perm, resident):
    from echopype_amd.xr_lite import Dataset

    ds = Dataset(coords={"channel": np.array(["chan1", "chan2"]), "ping_time": np.arange(P), "range_sample": np.arange(S)})
    for name, a in arrays.items():
        ds[name] = _var(a, perm, resident, "cuda")
    return ds


def _canonical(out):
    """The values of a result with its dimensions in (channel, ping_time, range_sample) order."""
    dims = list(out.dims)
    return np.asarray(out.values).transpose([dims.index(d) for d in DIMS if d in dims])


def _same_in_every_layout(run, arrays):
    want = _canonical(run(_dataset(arrays, (0, 1, 2), False)))
    for resident in (False, True):
        np.testing.assert_array_equal(_canonical(run(_dataset(arrays, OTHER, resident))), want)
    return want


@pytest.mark.gpu
def test_detect_seafloor_basic_in_another_dimension_order():
    import echopype_amd as ep

    sv, depth = _scene(1)
    prm = {"var_name": "Sv", "channel": "chan2", "threshold": (-40.0, -20.0), "bin_skip_from_surface": 4}
    want = _same_in_every_layout(lambda ds: ep.mask.detect_seafloor(ds, "basic", prm), {"Sv": sv, "depth": depth})
    assert want.shape == (P,) and np.isfinite(want).any()


@pytest.mark.gpu
def test_detect_shoal_weill_in_another_dimension_order():
    import echopype_amd as ep

    sv, _ = _scene(2)
    prm = {"var_name": "Sv", "channel": "chan2", "thr": -60.0, "maxvgap": 2, "maxhgap": 1, "minvlen": 2, "minhlen": 2}
    want = _same_in_every_layout(lambda ds: ep.mask.detect_shoal(ds, "weill", prm), {"Sv": sv})
    assert want.shape == (P, S) and want.any() and not want.all()


@pytest.mark.gpu
def test_detect_transient_fielding_in_another_dimension_order():
    import echopype_amd as ep

    sv, depth = _scene(3)
    prm = dict(range_var="depth", r0=4.0, r1=12.0, n=3, thr=(3, 1), roff=1.0, jumps=1.0, maxts=-35)
    want = _same_in_every_layout(lambda ds: ep.clean.detect_transient(ds, "fielding", prm), {"Sv": sv, "depth": depth})
    assert want.shape == (C, P, S) and want.any() and not want.all()


@pytest.mark.gpu
def test_mask_impulse_noise_in_another_dimension_order():
    import echopype_amd as ep

    sv, depth = _scene(4)
    want = _same_in_every_layout(lambda ds: ep.clean.mask_impulse_noise(ds, depth_bin="2m", num_side_pings=1,
                                                                        impulse_noise_threshold="8.0dB"),
                                 {"Sv": sv, "depth": depth})
    assert want.shape == (C, P, S) and want.any() and not want.all()


@pytest.mark.gpu
def test_add_splitbeam_angle_power_in_another_dimension_order():
    """The beam group's angle planes in another order (and a channel selection, so that they are gathered), the angle
    parameters as (ping_time, channel)."""
    import torch

    import echopype_amd as ep
    from echopype_amd import echodata, synth
    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    d = synth.ek60_splitbeam_numpy(C=2, P=6, S=50, nan_pad=True)  # float32 planes, NaN-padded
    names = ("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship",
             "angle_offset_athwartship")

    def run(perm, resident, flip):
        ed = echodata.from_ek60_arrays(d)
        beam = ed["Sonar/Beam_group1"]
        for k in ("angle_alongship", "angle_athwartship"):
            beam[k] = _var(np.asarray(d[k]), perm, resident, "cuda")
        ds = Dataset(coords={"channel": list(d["channel"])[::-1], "ping_time": d["ping_time"], "range_sample": np.arange(50)},
                     attrs={"processing_function": "calibrate.compute_Sv"})
        for k in names:
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(d[k], dtype=np.float64)[::-1, None], (2, 6)))
            a, dims = (np.ascontiguousarray(a.T), ("ping_time", "channel")) if flip else (a, ("channel", "ping_time"))
            ds[k] = DataArray(DeviceArray(torch.from_numpy(a).cuda()) if resident else a, dims)
        out = ep.consolidate.add_splitbeam_angle(ds, ed, "CW", "power", to_disk=False)
        return np.stack([out["angle_alongship"].values, out["angle_athwartship"].values])

    want = run((0, 1, 2), False, False)
    assert want.shape == (2, 2, 6, 50) and np.isfinite(want).any() and np.isnan(want).any()
    for resident in (False, True):
        np.testing.assert_array_equal(run(OTHER, resident, True), want)
