"""``combine_echodata`` on a real MI355X: the kernel ``epa_concat_rows`` through ``ops.concat_rows``, the public call, and
the chain behind it, all bit-equal (``tobytes()``) to the restatement tests/combine_ref.py -- copies, conversions of
integers that a float holds exactly or rounds to nearest even, and NumPy's own NaN pattern: there is no tolerance.

The shapes are the smallest at which the kernel can go wrong: rows of 1, 7, 64, 65 and 257 elements (shorter than a
16-byte chunk, odd, a whole number of chunks, one more, several chunks plus one) whose starts are only element-aligned in
the sources and in the output, files of 1, 5 and 70 pings (less than, and more than, the rows of one workgroup), more files
than a wavefront has lanes, and every served pair of element types."""
import copy
import ctypes
import logging

import numpy as np
import pytest

import combine_cases as C
import combine_ref as R

pytestmark = pytest.mark.gpu

KERNEL = "concat_rows_kernel"


@pytest.fixture(scope="module")
def ep():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    import echopype_amd

    return echopype_amd


def run(ep, arrs, maps=None, out_dtype=None):
    """-> the joined volume on the host; exactly one launch of the kernel."""
    import torch

    from echopype_amd import _lib

    ts = [torch.from_numpy(a.copy()).cuda() for a in arrs]
    tdt = None if out_dtype is None else torch.from_numpy(np.empty(0, dtype=out_dtype)).dtype
    with _lib.launch_trace() as tr:
        out = ep.ops.concat_rows(ts, maps, out_dtype=tdt)
    assert tr.kernels == [KERNEL], tr.kernels
    return out.cpu().numpy()


def check(ep, arrs, maps=None, out_dtype=None, what=""):
    want = R.concat_rows(arrs, maps, out_dtype)
    got = run(ep, arrs, maps, out_dtype)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(f"u{got.itemsize}") != want.reshape(-1).view(f"u{want.itemsize}"))
        pytest.fail(f"{what}: {bad.size} of {got.size} elements differ, first at {np.unravel_index(bad[0], got.shape)}: "
                    f"{got.reshape(-1)[bad[:4]]} for {want.reshape(-1)[bad[:4]]}")
    return got


def segments(dtype, P=C.P_LIST, W=C.W_LIST, Cn=3, seed=0, beam=None):
    return [C.fill((Cn, p, w) + ((beam,) if beam else ()), dtype, seed * 100 + i) for i, (p, w) in enumerate(zip(P, W))]


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src, out", [p for p in C.TYPE_PAIRS if p[1].startswith("float")])
def test_ragged_rows_every_padding_type_pair(ep, src, out):
    """P_i = 1, 5, 70, 1, 3 and W_i = 1, 7, 64, 65, 257: every row but the last file's is padded, W_out = 257 is odd, so
    output rows start at every element alignment."""
    arrs = segments(src, seed=1)
    got = check(ep, arrs, out_dtype=out, what=f"{src}->{out}")
    assert got.shape == (3, 80, 257)
    pad = got[:, :77, 65:]
    word = {4: 0x7FC00000, 8: 0x7FF8000000000000}[got.itemsize]
    assert (pad.view(f"u{got.itemsize}") == word).all()  # NumPy's np.nan, bit for bit
    if src == out:  # the NaN with a payload came through as it was
        assert got.view(f"u{got.itemsize}")[0, 6, 3] == arrs[2].view(f"u{got.itemsize}")[0, 0, 3] != word
        assert np.isposinf(got).any() and np.isneginf(got).any()


@pytest.mark.parametrize("src, out", C.TYPE_PAIRS)
@pytest.mark.parametrize("W", [65, 16])
def test_equal_widths_need_no_pad_and_integers_stay_integers(ep, src, out, W):
    arrs = segments(src, W=(W,) * 5, seed=2)
    got = check(ep, arrs, out_dtype=out, what=f"{src}->{out} W={W}")
    assert got.dtype == np.dtype(out) and got.shape == (3, 80, W)
    if src == out:
        assert check(ep, arrs, what=f"{src} default").dtype == np.dtype(src)  # no pad: the default keeps the type


@pytest.mark.parametrize("src, want", [("int8", "float32"), ("int16", "float32"), ("int32", "float64"), ("int64", "float64"),
                                       ("float32", "float32"), ("float64", "float64")])
def test_default_output_type_of_a_padded_join(ep, src, want):
    assert check(ep, segments(src, seed=3), what=src).dtype == np.dtype(want)


def test_int64_values_a_double_cannot_hold_round_to_nearest_even(ep):
    a = np.array([2**53 + 1, 2**53 + 3, -(2**53) - 1, 2**62 + 2**9 + 1, np.iinfo(np.int64).max, np.iinfo(np.int64).min],
                 dtype=np.int64).reshape(1, 2, 3)
    b = np.array([7], dtype=np.int64).reshape(1, 1, 1)
    got = check(ep, [a, b], what="int64 rounding")
    assert got[0, 0, 0] == 2.0**53 and got[0, 0, 1] == 2.0**53 + 4 and np.isnan(got[0, 2, 1:]).all()


def test_more_segments_than_lanes(ep):
    """130 files of one ping each, widths 1 .. 40 in a scrambled order: the search of the first-ping column goes past 64
    and past 128 entries, and every row belongs to another file than its neighbours."""
    rng = np.random.default_rng(4)
    widths = rng.integers(1, 41, 130)
    widths[rng.integers(0, 130)] = 40
    arrs = [C.fill((3, 1, int(w)), "float32", 400 + i) for i, w in enumerate(widths)]
    got = check(ep, arrs, what="130 segments")
    assert got.shape == (3, 130, 40)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_one_two_and_three_segments(ep, n):
    arrs = segments("float64", P=(5, 1, 70)[:n], W=(7, 257, 64)[:n], seed=5)
    check(ep, arrs, what=f"{n} segments")


@pytest.mark.parametrize("maps", [[[2, 0, 1], [0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 2, 1]],   # a permutation per file
                                  [[2, 0], [0, 1], [1, 2], [2, 1], [0, 2]]])                 # 2 of 3 channels
def test_channel_maps(ep, maps):
    arrs = segments("float32", seed=6)
    got = check(ep, arrs, maps, what=str(maps[0]))
    assert got.shape[0] == len(maps[0])
    assert got[0, 0, 0].tobytes() == arrs[0][maps[0][0], 0, 0].tobytes()


def test_files_with_different_channel_counts(ep):
    arrs = [C.fill((4, 3, 9), "float32", 70), C.fill((2, 5, 6), "float32", 71)]
    check(ep, arrs, [[3, 1], [0, 1]], what="4 and 2 channels")
    with pytest.raises(ValueError, match="need chan_maps"):
        run(ep, arrs)


@pytest.mark.parametrize("src", ["float32", "int16", "float64"])
def test_trailing_beam_dimension(ep, src):
    arrs = segments(src, P=(2, 5, 1), W=(3, 5, 3), seed=8, beam=4)
    got = check(ep, arrs, what=f"beam {src}")
    assert got.shape == (3, 8, 5, 4) and np.isnan(got[:, :2, 3:, :]).all() and not np.isnan(got[:, 2:7]).all()


def test_element_index_past_2_to_the_31(ep):
    """Two files of 1 x 1 100 000 x 1000 int8: the output holds 2.2e9 elements, so the last rows' element offsets do not
    fit 32 bits.  Equal widths make the join a plain concatenation; it is compared on the device with ``torch.cat`` (the
    NumPy restatement at this size would cost seconds of host time and 4 GB over PCIe), and the seam and the end are also
    compared with the sources on the host."""
    import torch

    from echopype_amd import _lib

    P, W = 1_100_000, 1000
    g = torch.Generator(device="cuda").manual_seed(31)
    ts = [torch.randint(-128, 128, (1, P, W), dtype=torch.int8, device="cuda", generator=g) for _ in range(2)]
    with _lib.launch_trace() as tr:
        out = ep.ops.concat_rows(ts)
    assert tr.kernels == [KERNEL] and out.numel() > 2**31 and out.dtype == torch.int8
    assert torch.equal(out, torch.cat(ts, dim=1))
    assert out[0, P - 1:P + 1].cpu().numpy().tobytes() == torch.stack([ts[0][0, -1], ts[1][0, 0]]).cpu().numpy().tobytes()
    assert out[0, -1].cpu().numpy().tobytes() == ts[1][0, -1].cpu().numpy().tobytes()


def _direct(ep, segs, chan, C_out, W_out, src_ct, out_ct, out_ptr):
    """The C entry point itself, with tables the wrapper would never build -> (status, kernels launched)."""
    from echopype_amd import _lib

    segs = np.ascontiguousarray(segs, dtype=np.int64)
    chan = np.ascontiguousarray(chan, dtype=np.int32)
    sd, cd = ep.ops.to_device(segs), ep.ops.to_device(chan)
    with _lib.launch_trace() as tr:
        rc = _lib.lib.epa_concat_rows(segs.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(sd.data_ptr()),
                                      chan.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(cd.data_ptr()), len(segs), C_out,
                                      W_out, src_ct, out_ct, ctypes.c_void_p(out_ptr), None)
    return rc, tr.kernels, _lib.last_error()


def test_refused_arguments_launch_nothing(ep):
    import torch

    from echopype_amd import _lib

    a = torch.zeros((3, 4, 8), dtype=torch.float32, device="cuda")
    b = torch.zeros((3, 2, 5), dtype=torch.float32, device="cuda")
    out = torch.zeros((3, 6, 8), dtype=torch.float32, device="cuda")
    ident = [[0, 1, 2], [0, 1, 2]]

    def seg(t, first, P=None, W=None):
        return [t.data_ptr(), t.shape[1] if P is None else P, t.shape[2] if W is None else W, first, t.shape[0]]

    F32, I16 = _lib.CT_F32, _lib.CT_I16
    rc, kernels, _ = _direct(ep, [seg(a, 0), seg(b, 4)], ident, 3, 8, F32, F32, out.data_ptr())
    assert (rc, kernels) == (_lib.EPA_OK, [KERNEL])  # the tables are sound: this one runs
    torch.cuda.synchronize()
    for what, args, message in [
        ("P_i == 0", ([seg(a, 0), seg(b, 4, P=0)], ident, 3, 8, F32, F32, out.data_ptr()), "P=0 pings"),
        ("W_i > W_out", ([seg(a, 0), seg(b, 4)], ident, 3, 7, F32, F32, out.data_ptr()), "W=8 elements"),
        ("padded integer", ([seg(a, 0), seg(b, 4)], ident, 3, 8, I16, I16, out.data_ptr()), "need a NaN pad"),
        ("integer from float", ([seg(a, 0), seg(b, 4)], ident, 3, 8, F32, I16, out.data_ptr()), "are served"),
        ("out is a source", ([seg(a, 0), seg(b, 4)], ident, 3, 8, F32, F32, a.data_ptr()), "overlaps the source of segment 0"),
        ("out ends inside a source", ([seg(a, 0), seg(b, 4)], ident, 3, 8, F32, F32, b.data_ptr() - 3 * 6 * 8 * 4 + 4),
         "overlaps the source of segment"),
        ("first ping", ([seg(a, 0), seg(b, 5)], ident, 3, 8, F32, F32, out.data_ptr()), "pings lie before it"),
        ("channel map", ([seg(a, 0), seg(b, 4)], [[0, 1, 2], [0, 1, 3]], 3, 8, F32, F32, out.data_ptr()), "source channel 3"),
        ("NULL out", ([seg(a, 0), seg(b, 4)], ident, 3, 8, F32, F32, 0), "out is NULL"),
    ]:
        rc, kernels, err = _direct(ep, *args)
        assert (rc, kernels) == (_lib.EPA_EINVAL, []) and message in err, (what, rc, kernels, err)
    # ... and through the wrapper
    with _lib.launch_trace() as tr:
        with pytest.raises(ValueError, match="P=0 pings"):
            ep.ops.concat_rows([a, torch.zeros((3, 0, 5), dtype=torch.float32, device="cuda")])
        with pytest.raises(ValueError, match="need a NaN pad"):
            ep.ops.concat_rows([a.to(torch.int16), b.to(torch.int16)], out_dtype=torch.int16)
        with pytest.raises(ValueError, match="f64 are served"):
            ep.ops.concat_rows([a, b], out_dtype=torch.float64)
        with pytest.raises(ValueError, match="must agree in dtype"):
            ep.ops.concat_rows([a, b.double()])
    assert tr.kernels == []


# ---- 2. the public call ---------------------------------------------------------------------------------------------------------
S_LIST, PINGS = (40, 64, 57), (30, 1, 45)
ORDERS = ((0, 1, 2), (2, 0, 1), (0, 1, 2))


def ek60_files(ep, starts=(0, 30, 31), S=S_LIST, P=PINGS, orders=ORDERS, angles=False):
    """Three synthetic EK60 files as host EchoData; file i starts ``starts[i]`` seconds after the first."""
    from echopype_amd.echodata import from_ek60_arrays

    eds = []
    for i, (s, p, order) in enumerate(zip(S, P, orders)):
        d = ep.synth.ek60_numpy(C=3, P=p, S=s, seed=900 + i)
        d["ping_time"] = np.asarray(d["ping_time"], dtype="datetime64[ns]") + np.timedelta64(starts[i], "s")
        if angles:
            rng = np.random.default_rng(i)
            d["angle_alongship"] = rng.integers(-128, 127, (3, p, s), dtype=np.int8)
            d["angle_athwartship"] = rng.integers(-128, 127, (3, p, s), dtype=np.int8)
        idx = list(order)
        for k, v in list(d.items()):
            if k == "channel":
                d[k] = [v[j] for j in idx]
            elif isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == 3 and k != "ping_time":
                d[k] = np.ascontiguousarray(v[idx])
        ed = from_ek60_arrays(d, source_file=f"/survey/leg{i}.raw")
        ed["Top-level"] = ep.Dataset(attrs={"title": f"leg {i}", "sonar_convention_version": "1.0"})
        ed["Sonar/Beam_group1"].attrs["beam_mode"] = "vertical"
        eds.append(ed)
    return eds


def restated(eds, sel=None):
    return R.combine([R.from_echodata(e) for e in eds], copy.deepcopy(sel))


@pytest.fixture(scope="module")
def ek60_want(ep):
    """The restatement of the three-file combination, computed once and left alone."""
    return restated(ek60_files(ep, angles=True))[0]


@pytest.mark.parametrize("where", ["host", "device", "mixed"])
def test_three_ek60_files(ep, where, ek60_want):
    from echopype_amd import _lib, ops
    from echopype_amd.echodata import BEAM1

    eds = ek60_files(ep, angles=True)
    for i, e in enumerate(eds):
        if where == "device" or (where == "mixed" and i == 1):
            e.to_device()
    with _lib.launch_trace() as tr:
        ed = ep.combine_echodata(eds)
    # one launch per (channel, ping_time, range_sample) variable that is resident, whatever the number of files; the int8
    # angle planes are not (EchoData.to_device leaves them on the host) and are joined in NumPy
    assert tr.kernels.count(KERNEL) == 1, tr.kernels
    R.assert_equal(ed, ek60_want, where)
    beam, env = ed[BEAM1], ed["Environment"]
    for name in ("backscatter_r", "sample_interval", "transmit_duration_nominal", "transmit_power"):
        assert isinstance(beam.data_vars[name].data, ep.DeviceArray), name
    for name in ("sound_speed_indicative", "absorption_indicative"):
        assert isinstance(env.data_vars[name].data, ep.DeviceArray), name
    assert beam["backscatter_r"].shape == (3, 76, 64) and beam["backscatter_r"].dtype == np.float32
    assert beam["angle_alongship"].dtype == np.float32 and isinstance(beam.data_vars["angle_alongship"].data, np.ndarray)
    assert beam["channel"].values.tolist() == sorted(eds[0][BEAM1]["channel"].values.tolist())
    assert beam["range_sample"].values.tolist() == list(range(64))
    # the parameters keep a host mirror that cannot be written to: looking at them costs no copy
    from echopype_amd.xr_lite import host_readable

    si = beam.data_vars["sample_interval"].data
    assert host_readable(si) and not np.asarray(si).flags.writeable
    assert np.array_equal(np.asarray(si), si.tensor.cpu().numpy())
    # ping_time is resident and known to be sorted: nothing scans or uploads it again
    pt = beam["ping_time"].values
    assert not pt.flags.writeable
    ns, ok, t = ops.ping_time_facts(pt)
    assert ok and np.array_equal(t.cpu().numpy(), pt.view(np.int64))
    assert ed["Provenance"]["title"].values.tolist() == ["leg 0", "leg 1", "leg 2"]
    assert ed["Provenance"]["beam_mode"].attrs == {"echodata_group": BEAM1}
    # the inputs are not consumed
    assert eds[0][BEAM1]["backscatter_r"].shape == (3, 30, 40)


@pytest.mark.parametrize("where", ["host", "device"])
def test_resident_int8_planes_go_through_the_converting_kernel(ep, where):
    from echopype_amd import _lib
    from echopype_amd.echodata import BEAM1

    eds = ek60_files(ep, angles=True)
    want = restated(eds)[0]
    for e in eds[: 3 if where == "device" else 1]:
        for k in ("angle_alongship", "angle_athwartship"):
            v = e[BEAM1].data_vars[k]
            e[BEAM1].data_vars[k] = ep.DataArray(ep.DeviceArray(ep.ops.to_device(v.values)), v.dims, attrs=v.attrs, name=k)
    with _lib.launch_trace() as tr:
        ed = ep.combine_echodata(eds)
    assert tr.kernels.count(KERNEL) == 3, tr.kernels
    R.assert_equal(ed, want, where)
    assert isinstance(ed[BEAM1].data_vars["angle_athwartship"].data, ep.DeviceArray)
    # all files of one width: the planes stay int8
    same = ek60_files(ep, S=(40, 40, 40), angles=True)
    ed = ep.combine_echodata(same)
    R.assert_equal(ed, restated(same)[0], "equal widths")
    assert ed[BEAM1]["angle_alongship"].dtype == np.int8


@pytest.mark.parametrize("where", ["host", "device"])
def test_channel_selection_as_a_list(ep, where, monkeypatch):
    """The selection reaches the kernel as its channel map: the files' own cubes are what it reads (no selected copy of
    a resident cube is made first), with two of their three channels mapped."""
    from echopype_amd import ops
    from echopype_amd.echodata import BEAM1

    eds = ek60_files(ep)
    if where == "device":
        for e in eds:
            e.to_device()
    chans = eds[0][BEAM1]["channel"].values.tolist()
    sel = [chans[2], chans[0]]
    want = restated(eds, sel)[0]
    calls = []
    real = ops.concat_rows
    monkeypatch.setattr(ops, "concat_rows", lambda ts, maps=None, **kw: (calls.append((ts, maps)), real(ts, maps, **kw))[1])
    ed = ep.combine_echodata(eds, channel_selection=list(sel))
    (ts, maps), = calls
    assert [tuple(t.shape) for t in ts] == [(3, 30, 40), (3, 1, 64), (3, 45, 57)]  # all three channels: nothing was selected yet
    order = [e[BEAM1]["channel"].values.tolist() for e in eds]
    assert [list(m) for m in maps] == [[o.index(c) for c in sorted(sel)] for o in order]
    if where == "device":
        assert [t.data_ptr() for t in ts] == [e[BEAM1].data_vars["backscatter_r"].data.tensor.data_ptr() for e in eds]
    R.assert_equal(ed, want, "list")
    assert ed[BEAM1]["channel"].values.tolist() == sorted(sel) and ed[BEAM1]["backscatter_r"].shape == (2, 76, 64)
    assert ed["Vendor_specific"]["channel"].values.tolist() == sorted(sel) and sel == [chans[2], chans[0]]


@pytest.mark.parametrize("dtype, dims", [("float64", ("ping_time", "channel")), ("float16", ("channel", "ping_time", "range_sample")),
                                         ("bool", ("channel", "ping_time"))])
def test_a_resident_variable_the_device_join_does_not_serve_comes_out_resident(ep, dtype, dims):
    """Joined in NumPy (another layout, or a type without a kernel) and uploaded again: resident in, resident out."""
    from echopype_amd import _lib
    from echopype_amd.echodata import BEAM1

    eds = ek60_files(ep)
    for i, e in enumerate(eds):
        b = e[BEAM1]
        shape = tuple(b.sizes[d] for d in dims)
        a = (np.random.default_rng(i).standard_normal(shape) > 0.3).astype(dtype) if dtype == "bool" else \
            np.random.default_rng(i).standard_normal(shape).astype(dtype)
        b["extra"] = (dims, a)
    want = restated(eds)[0]
    v = eds[1][BEAM1].data_vars["extra"]
    eds[1][BEAM1].data_vars["extra"] = ep.DataArray(ep.DeviceArray(ep.ops.to_device(v.values)), v.dims, name="extra")
    with _lib.launch_trace() as tr:
        ed = ep.combine_echodata(eds)
    assert tr.kernels.count(KERNEL) == 1, tr.kernels  # backscatter_r only
    R.assert_equal(ed, want, dtype)
    out = ed[BEAM1].data_vars["extra"].data
    assert isinstance(out, ep.DeviceArray) and out.dtype == np.dtype(dtype)
    assert out.tensor.cpu().numpy().tobytes() == np.asarray(want[BEAM1]["vars"]["extra"][1]).tobytes()


@pytest.mark.parametrize("where", ["host", "device"])
def test_selection_with_equal_widths_keeps_integer_planes_integer(ep, where):
    """Two of three channels, every file 40 samples wide: nothing is padded, so the int8 angle planes stay int8 -- host
    planes joined in NumPy, resident ones by the same-type kernel through the channel map, not the converting one."""
    from echopype_amd import _lib
    from echopype_amd.echodata import BEAM1

    eds = ek60_files(ep, S=(40, 40, 40), angles=True)
    chans = eds[0][BEAM1]["channel"].values.tolist()
    sel = [chans[2], chans[0]]
    want = restated(eds, sel)[0]
    if where == "device":
        for e in eds:
            for k in ("angle_alongship", "angle_athwartship"):
                v = e[BEAM1].data_vars[k]
                e[BEAM1].data_vars[k] = ep.DataArray(ep.DeviceArray(ep.ops.to_device(v.values)), v.dims, attrs=v.attrs, name=k)
    with _lib.launch_trace() as tr:
        ed = ep.combine_echodata(eds, channel_selection=list(sel))
    assert tr.kernels.count(KERNEL) == (3 if where == "device" else 1), tr.kernels
    R.assert_equal(ed, want, where)
    for k in ("angle_alongship", "angle_athwartship"):
        v = ed[BEAM1].data_vars[k]
        assert v.dtype == np.int8 and v.shape == (2, 76, 40) and isinstance(v.data, ep.DeviceArray) == (where == "device")
    assert ed[BEAM1]["backscatter_r"].dtype == np.float32 and not np.isnan(ed[BEAM1]["backscatter_r"].values[:, :, :38]).all()
    assert ed[BEAM1]["beam_type"].dtype == np.int64 if "beam_type" in ed[BEAM1] else True


def ek80_files(ep):
    from echopype_amd.echodata import from_ek80_arrays

    eds = []
    for i, (p, s) in enumerate(((4, 48), (3, 37))):
        d = ep.synth.ek80_numpy(C=2, P=p, S=s, B=4, seed=70 + i)
        d["ping_time"] = np.asarray(d["ping_time"], dtype="datetime64[ns]") + np.timedelta64(10 * i, "s")
        eds.append(from_ek80_arrays(d, ep.synth.ek80_filters(), source_file=f"bb{i}.raw"))
    return eds


@pytest.mark.parametrize("form", ["none", "list", "dict"])
def test_ek80_complex_with_a_beam_dimension(ep, form):
    from echopype_amd import _lib
    from echopype_amd.echodata import BEAM1

    eds = ek80_files(ep)
    chans = eds[0][BEAM1]["channel"].values.tolist()
    sel = {"none": None, "list": [chans[1]], "dict": {BEAM1: [chans[1]]}}[form]
    want = restated(eds, sel)[0]
    with _lib.launch_trace() as tr:
        ed = ep.combine_echodata(eds, channel_selection=copy.deepcopy(sel))
    assert tr.kernels.count(KERNEL) == 2, tr.kernels  # backscatter_r and backscatter_i
    R.assert_equal(ed, want, form)
    n = 2 if sel is None else 1
    assert ed[BEAM1]["backscatter_i"].shape == (n, 7, 48, 4) and isinstance(ed[BEAM1].data_vars["backscatter_i"].data, ep.DeviceArray)
    assert np.isnan(ed[BEAM1]["backscatter_r"].values[:, 4:, 37:, :]).all()
    assert ed["Vendor_specific"]["channel"].values.tolist() == (chans if sel is None else [chans[1]])
    assert ed[BEAM1]["transmit_type"].values.shape == (n, 7)


def test_error_paths_with_beam_groups(ep):
    from echopype_amd.echodata import BEAM1

    eds = ek60_files(ep)
    with pytest.raises(RuntimeError, match="ping_time is not in ascending order for group Sonar/Beam_group1"):
        ep.combine_echodata([eds[2], eds[0]])
    with pytest.raises(NotImplementedError, match="do not contain the selected channels"):
        ep.combine_echodata(eds, channel_selection=["no such channel"])
    with pytest.raises(ValueError, match="conflicting filenames"):
        ep.combine_echodata([eds[0], eds[0]])
    e80 = ek80_files(ep)
    with pytest.raises(ValueError, match="same sonar_model"):
        ep.combine_echodata([eds[0], e80[0]])
    b = e80[1][BEAM1]
    b.coords["beam"] = ep.DataArray(np.arange(4) + 1, ("beam",), name="beam")
    with pytest.raises(NotImplementedError, match="coordinate beam differs"):
        ep.combine_echodata(e80)
    with pytest.raises(KeyError):  # a dict without the group's entry, as in the reference
        ep.combine_echodata(ek80_files(ep), channel_selection={"Sonar/Beam_group2": ["x"]})


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(np.asarray(a))
    return a.dtype, a.shape, a.tobytes()


def _sv_mvbs(ep, ed):
    sv = ep.calibrate.compute_Sv(ed)
    return sv, ep.commongrid.compute_MVBS(sv, range_bin="1m", ping_time_bin="20s")


def test_chain_equals_the_chain_on_the_restated_volume_and_sees_across_the_seam(ep, ek60_want):
    """File 0 ends at second 29, file 1 is second 30, file 2 starts at second 31: the 20-second bin that starts at second
    20 holds pings of all three."""
    eds = ek60_files(ep, angles=True)
    combined = ep.combine_echodata([e.to_device() for e in eds])
    direct = C.as_echodata(ep, dict(sonar_model="EK60", source_file="restated.raw", groups=ek60_want))
    (sv_a, mv_a), (sv_b, mv_b) = _sv_mvbs(ep, combined), _sv_mvbs(ep, direct)
    for a, b in ((sv_a, sv_b), (mv_a, mv_b)):
        assert _bits(a["ping_time"].values) == _bits(b["ping_time"].values)
        for v in ("Sv", "echo_range"):
            assert _bits(a[v].values) == _bits(b[v].values), v
    assert np.isfinite(mv_a["Sv"].values).any()
    # the bin of the seam: each file alone gives a half-cell there, and neither is the value of the whole cell
    alone = [_sv_mvbs(ep, e)[1] for e in ek60_files(ep)[::2]]
    t_all = mv_a["ping_time"].values
    shared = [t for t in alone[0]["ping_time"].values if t in alone[1]["ping_time"].values]
    assert len(shared) == 1 and shared[0] in t_all
    whole = mv_a["Sv"].values[:, list(t_all).index(shared[0])]
    order = [list(mv_a["channel"].values).index(c) for c in alone[0]["channel"].values]
    for m in alone:
        half = m["Sv"].values[:, list(m["ping_time"].values).index(shared[0])]
        n = min(half.shape[-1], whole.shape[-1])
        both = np.isfinite(half[:, :n]) & np.isfinite(whole[order][:, :n])
        assert both.sum() > 10 and (half[:, :n][both] != whole[order][:, :n][both]).mean() > 0.9


def test_a_seam_that_steps_backwards_is_known_at_once_and_repaired_in_place(ep, monkeypatch, caplog):
    from echopype_amd import _lib, ops
    from echopype_amd.echodata import BEAM1

    eds = ek60_files(ep, starts=(0, 28, 30), P=(30, 2, 45))  # file 0 ends at second 29, file 1 starts at second 28
    combined = ep.combine_echodata(eds)
    beam = combined[BEAM1]
    bad = beam["ping_time"].values.copy()
    assert not ops.ping_time_facts(beam["ping_time"].values)[1]  # the verdict came with the combination
    assert ep.qc.exist_reversed_time(beam, "ping_time") is True
    real_upload = ops.to_device
    uploads = []

    def probe(a, *k, **kw):  # the residency probe of test_gpu_qc.py, recording instead of failing: (dtype kind, size)
        uploads.append((np.asarray(a).dtype.kind, np.asarray(a).size) if not hasattr(a, "is_cuda") else ("t", a.numel()))
        return real_upload(a, *k, **kw)

    monkeypatch.setattr(ops, "to_device", probe)
    with caplog.at_level(logging.WARNING, logger="echopype_amd.qc"):
        assert ep.qc.orchestrate_reverse_time_check(combined, None, ["ping_time"], {}) is None
    prov = combined["Provenance"]
    assert prov.attrs["reversed_ping_times"] == 1
    old = prov["sonar_beam_group1_old_ping_time"]
    assert old.dims == ("sonar_beam_group1_old_ping_time_dim",) and np.array_equal(old.values, bad)
    assert old.attrs["comment"] == "Uncorrected ping_time from the combined group Sonar/Beam_group1."
    import qc_ref

    want = qc_ref.clean_reversed(bad, 100)
    fixed = beam["ping_time"].values
    assert np.array_equal(fixed.view(np.int64), want) and qc_ref.is_sorted_and_valid(want)
    # the repaired coordinate is resident like the one it replaces: no time stamps went up for the repair, none go up later
    assert not fixed.flags.writeable and ops.ping_time_facts(fixed)[1] is True
    sv, mvbs = _sv_mvbs(ep, combined)
    times_up = [u for u in uploads if u[0] in "Mi" and u[1] == fixed.size]
    assert times_up == [], uploads
    monkeypatch.setattr(ops, "to_device", real_upload)
    assert np.isfinite(mvbs["Sv"].values).any() and np.array_equal(sv["ping_time"].values, fixed)
    # the Environment's time1 is the same clock; its old times go to Provenance under their own name
    ep.qc.orchestrate_reverse_time_check(combined, None, ["ping_time", "time1"], {})
    assert prov.attrs["reversed_ping_times"] == 1 and np.array_equal(prov["environment_old_time1"].values, bad)
    assert np.array_equal(combined["Environment"]["time1"].values.view(np.int64), want)
    # nothing reversed: the attribute says 0 and Provenance gains nothing
    clean = ep.combine_echodata(ek60_files(ep))
    ep.qc.orchestrate_reverse_time_check(clean, None, ["ping_time", "time1"], {})
    assert clean["Provenance"].attrs["reversed_ping_times"] == 0
    assert not any("_old_" in k for k in clean["Provenance"].data_vars)
