"""The echo summary statistics on the GPU (csrc/metrics.hip through ops.echo_metrics and the public functions of
echopype_amd.metrics) against the NumPy float64 oracle tests/metrics_ref.py, which runs on the values the kernel read.

Judging: NaN and +-inf where the oracle has them, nowhere else.  float64: 1e-9 relative, the project's float64 bar
(abundance is a logarithm: 1e-9 * 10 / ln 10 dB absolute; dispersion adds metrics_ref.dispersion_floor, the square of
cm's own rounding, without which a row whose mass sits in one sample -- dispersion 0 exactly -- compares noise with
noise).  float32: the derived per-row bounds of tests/metrics_bounds.py through f32_bounds.assert_f32_close, which also
asserts the old 1e-3 bar.

Row lengths: the issue's list, the sizes either side of where the code takes another form (one wave holds 2048 samples,
one workgroup 8192, longer rows are read in a loop), 8196 for the aligned looped form and 20 011 well past it."""
import numpy as np
import pytest

import f32_bounds as F
import metrics_bounds as B
import metrics_cases as C
import metrics_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 8191, 8192, 8193, 8196, 20011]
SHAPE = (3, 37)
DTYPES = [np.float32, np.float64]
F64_RTOL = 1e-9
LABELS = {"metrics_wave_kernel", "metrics_wave_kernel_unaligned", "metrics_block_kernel", "metrics_block_kernel_unaligned",
          "metrics_loop_kernel", "metrics_loop_kernel_unaligned"}

_CACHE = {}


def case(kind, S, dtype, shape=SHAPE):
    """(Sv, range, oracle statistics, oracle sums) of one seeded case; computed once, never written to."""
    key = (kind, S, np.dtype(dtype).name, shape)
    if key not in _CACHE:
        sv, r = C.make(kind, shape, S, dtype)
        st, s = R.rows(sv, r)
        for a in (sv, r, *st.values()):
            a.setflags(write=False)
        _CACHE[key] = (sv, r, st, s)
    return _CACHE[key]


def judge(got, st, s, dtype, what, given_cm=False, centre_err=0.0, extra=None):
    """``got`` {name: array} against the oracle's ``st`` for every name in ``got``."""
    bounds = B.kernel_bounds(st, s, given_cm, centre_err) if dtype == np.float32 else None
    for name, g in got.items():
        g = np.asarray(g)
        want = st[name]
        assert g.dtype == dtype and g.shape == want.shape, (what, name, g.dtype, g.shape)
        if dtype == np.float32:
            b = bounds[name] + (0.0 if extra is None else extra[name])
            F.assert_f32_close(g, want, b, f"{what} {name}")
            continue
        g = g.astype(np.float64)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(want), err_msg=f"{what} {name}: NaN pattern")
        inf = np.isinf(want)
        np.testing.assert_array_equal(np.isinf(g), inf, err_msg=f"{what} {name}: inf pattern")
        np.testing.assert_array_equal(g[inf], want[inf], err_msg=f"{what} {name}: inf sign")
        fin = np.isfinite(want)
        tol = np.full(want.shape, F64_RTOL * F.DB) if name == "abundance" else F64_RTOL * np.abs(want)
        if name == "dispersion" and not given_cm:
            tol = tol + R.dispersion_floor(st["center_of_mass"])
        if extra is not None:
            tol = tol + extra[name]
        with np.errstate(invalid="ignore"):
            err = np.abs(g - want)[fin]
        assert np.all(err <= tol[fin]), (what, name, float(err.max()), float((err / tol[fin]).max()))


def on_device(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cached cases are read-only)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def dataset(arrays, dims=("channel", "ping_time", "range_sample"), device=True):
    """A lite Dataset of ``arrays`` {name: array with range_sample LAST, or 1-D}, its variables laid out in ``dims``."""
    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    canon = [d for d in dims if d != "range_sample"] + ["range_sample"]
    shape = dict(zip(canon, arrays["Sv"].shape))
    ds = Dataset(coords={d: 100 + np.arange(shape[d]) for d in dims})
    for name, a in arrays.items():
        vd = tuple(dims) if a.ndim == len(dims) else ("range_sample",)
        if a.ndim == len(dims):
            a = np.ascontiguousarray(np.transpose(a, [canon.index(d) for d in dims]))
        ds[name] = DataArray(DeviceArray(on_device(a)) if device else a, vd, name=name)
    return ds


def public_five(ds, label="echo_range"):
    import echopype_amd as ep

    kw = {} if label == "echo_range" else {"range_label": label}
    return {name: getattr(ep.metrics, name)(ds, **kw) for name in C.STATS}


# ---- every length and content, through ops and through the public functions ------------------------------------------------
@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_every_length_and_content_through_ops(dtype, S):
    from echopype_amd import _lib, ops

    for kind in C.KINDS:
        sv, r, st, s = case(kind, S, dtype)
        with _lib.launch_trace() as tr:
            out = ops.echo_metrics(on_device(sv.reshape(-1, S)), on_device(r.reshape(-1, S) if r.ndim > 1 else r))
        assert len(tr.kernels) == 1 and tr.kernels[0] in LABELS
        form = "wave" if S <= 2048 else "block" if S <= 8192 else "loop"
        assert tr.kernels[0].startswith(f"metrics_{form}_kernel"), (S, tr.kernels)
        judge({k: v.reshape(SHAPE) for k, v in host(out).items()}, st, s, dtype, f"ops {kind} S={S}")
    if S == 1:  # no dz at all
        st = case("clean", 1, dtype)[2]
        assert np.isneginf(st["abundance"]).all() and all(np.isnan(st[k]).all() for k in C.STATS[1:])


@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_every_length_and_content_through_the_public_functions(dtype, S):
    """The five functions against the oracle, and ``summary`` equal to them bit for bit."""
    import torch

    import echopype_amd as ep

    for kind in C.KINDS:
        sv, r, st, s = case(kind, S, dtype)
        ds = dataset({"Sv": sv, "echo_range": r})
        five = public_five(ds)
        for name, da in five.items():
            assert da.dims == ("channel", "ping_time") and da.name == name and da.data.tensor.is_cuda
            np.testing.assert_array_equal(da.coords["ping_time"], 100 + np.arange(SHAPE[1]))
        judge({k: v.data.tensor.cpu().numpy() for k, v in five.items()}, st, s, dtype, f"public {kind} S={S}")
        both = ep.metrics.summary(ds)
        assert list(both.data_vars) == list(C.STATS)
        for name in C.STATS:
            a, b = both[name].data.tensor, five[name].data.tensor
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32 if dtype == np.float32 else torch.int64),
                                                      b.view(torch.int32 if dtype == np.float32 else torch.int64)), (kind, name)


# ---- rows: one, more than a grid's worth, row loops, views that start anywhere -----------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_single_row_and_views_offset_by_one_element(dtype):
    import torch

    from echopype_amd import _lib, ops

    for S in (5, 64, 2049, 8196):
        sv, r, st, s = case("sv_holes", S, dtype, shape=(1,))
        out = ops.echo_metrics(on_device(sv), on_device(r))
        judge(host(out), st, s, dtype, f"single row S={S}")
        # the same rows as views that start one element into their buffers: nothing is 16-byte aligned any more
        for shape in ((1,), (3,)):
            sv, r, st, s = case("sv_holes", S, dtype, shape=shape)
            bsv = torch.zeros(sv.size + 1, dtype=on_device(sv).dtype, device="cuda")
            brg = torch.zeros(r.size + 1, dtype=bsv.dtype, device="cuda")
            bsv[1:] = on_device(sv).reshape(-1)
            brg[1:] = on_device(r).reshape(-1)
            vsv, vrg = bsv[1:].view(-1, S), brg[1:].view(-1, S)
            assert vsv.data_ptr() % 16 != 0 and vsv.is_contiguous()
            with _lib.launch_trace() as tr:
                got = ops.echo_metrics(vsv, vrg)
            assert tr.kernels[0].endswith("_unaligned")
            judge(host(got), st, s, dtype, f"offset view S={S} rows={shape}")
            if shape == (1,):
                for k in out:  # alignment changes the loads, not the arithmetic
                    assert torch.equal(torch.nan_to_num(out[k], nan=7.0), torch.nan_to_num(got[k], nan=7.0)), (S, k)


def test_more_rows_than_one_grid_of_waves():
    """65 536 workgroups of four waves are the most a launch has: 262 144 + 5 rows make waves take a second row."""
    from echopype_amd import ops

    rows, S = 4 * 65536 + 5, 3
    sv, r, st, s = case("clean", S, np.float32, shape=(rows,))
    out = ops.echo_metrics(on_device(sv), on_device(r))
    judge(host(out), st, s, np.float32, "262149 rows")


@pytest.mark.parametrize("S", [257, 2049, 8193])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_row_loops_of_every_form_give_the_same_bits(dtype, S):
    """Two workgroups for 111 rows: every owner takes many rows in turn (the shared-memory slots of the sums alternate
    from row to row).  The rows do not know: bit for bit what one owner per row returns."""
    import torch

    from echopype_amd import ops

    sv, r, st, s = case("nan_tail", S, dtype)
    a, b = on_device(sv.reshape(-1, S)), on_device(r.reshape(-1, S))
    full = ops.echo_metrics(a, b)
    for want in (C.STATS, ("abundance",)):  # (abundance alone: one barrier per row)
        few = ops.echo_metrics(a, b, want=want, _max_grid=2)
        for k in few:
            assert torch.equal(torch.nan_to_num(few[k], nan=7.0), torch.nan_to_num(full[k], nan=7.0)), (S, k)
    judge({k: v.reshape(SHAPE) for k, v in host(full).items()}, st, s, dtype, f"row loop S={S}")


def test_every_launch_label_is_reached():
    from echopype_amd import _lib, ops

    seen = set()
    for S in (64, 65, 4096, 4097, 8196, 8193):
        sv, r, _, _ = case("clean", S, np.float32, shape=(2,))
        with _lib.launch_trace() as tr:
            ops.echo_metrics(on_device(sv), on_device(r), want=("abundance",))
        seen.update(tr.kernels)
    assert seen == LABELS


# ---- the centres handed in ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 257, 2049, 8193])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_dispersion_about_given_centres(dtype, S):
    from echopype_amd import ops

    sv, r, _, _ = case("sv_holes", S, dtype)
    cm = np.random.default_rng(S).uniform(0.0, 80.0, SHAPE)
    cm[0, 0], cm[0, 1] = np.nan, np.inf
    st, s = R.rows(sv, r, cm=cm)
    # a NaN centre makes every term NaN, all are skipped: 0 / A; an infinite one follows IEEE
    assert st["dispersion"][0, 0] == 0.0 and np.isposinf(st["dispersion"][0, 1])
    out = ops.echo_metrics(on_device(sv.reshape(-1, S)), on_device(r.reshape(-1, S)), cm=on_device(cm.reshape(-1)),
                           want=("dispersion", "center_of_mass", "abundance"))
    assert sorted(out) == ["abundance", "center_of_mass", "dispersion"]
    judge({k: v.reshape(SHAPE) for k, v in host(out).items()}, st, s, dtype, f"given cm S={S}", given_cm=True)


def test_bad_arguments_are_refused():
    import torch

    from echopype_amd import ops

    sv = torch.zeros((2, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="range must be"):
        ops.echo_metrics(sv, sv.double())
    with pytest.raises(ValueError, match="range must be"):
        ops.echo_metrics(sv, sv[:, :4].contiguous())
    with pytest.raises(ValueError, match="want must name"):
        ops.echo_metrics(sv, sv, want=("mean",))
    with pytest.raises(ValueError, match="cm must be float64"):
        ops.echo_metrics(sv, sv, cm=torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError, match="max_grid"):
        ops.echo_metrics(sv, sv, _max_grid=65537)
    assert ops.echo_metrics(sv[:0], sv[:0])["abundance"].shape == (0,)


# ---- the public functions: layouts, types, labels ---------------------------------------------------------------------------------
def test_the_known_answers_of_the_reference_tests():
    """Integer arrays on the host, ``frequency`` in place of ``channel``: np.allclose with rtol 1e-9 as the reference's
    tests call it, and the oracle at the float64 bar."""
    import echopype_amd as ep

    _, known, _ = C.load_fixture()
    for name in C.STATS:
        k = known[name]
        sv, r = np.array(k["Sv"]), np.array(k["echo_range"])
        assert sv.dtype.kind == "i" and r.dtype.kind == "i"
        ds = dataset({"Sv": sv, "echo_range": r}, dims=("frequency", "ping_time", "range_sample"), device=False)
        out = getattr(ep.metrics, name)(ds)
        assert out.dims == ("frequency", "ping_time") and out.data.tensor.dtype.is_floating_point
        got = out.data.tensor.cpu().numpy()
        assert got.dtype == np.float64 and np.allclose(got, np.array(k["expected"]), rtol=k["rtol"]), (name, got)
        st, s = R.rows(sv.astype(np.float64), r.astype(np.float64))
        judge({name: got}, st, s, np.float64, f"known {name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_any_layout_host_or_device_and_the_range_forms(dtype):
    import torch

    import echopype_amd as ep

    S = 65
    sv, r, st, s = case("range_nan", S, dtype)
    first = None
    for dims in (("channel", "ping_time", "range_sample"), ("range_sample", "ping_time", "channel"),
                 ("ping_time", "range_sample", "channel")):
        for device in (True, False):
            ds = dataset({"Sv": sv, "echo_range": r}, dims, device)
            out = ep.metrics.summary(ds)
            rest = tuple(d for d in dims if d != "range_sample")
            got = {}
            for name in C.STATS:
                assert out[name].dims == rest
                got[name] = out[name].data.tensor  # (dataset() lays the leading axes of the arrays out in the order of rest)
            judge(host(got), st, s, dtype, f"layout {dims} device={device}")
            first = got if first is None else first
            for name in C.STATS:  # the rows are the same rows: the same bits
                assert torch.equal(torch.nan_to_num(got[name], nan=7.0), torch.nan_to_num(first[name], nan=7.0))
    # the range laid out otherwise than Sv
    from echopype_amd.xr_lite import DataArray, DeviceArray

    ds = dataset({"Sv": sv, "echo_range": r})
    ds["echo_range"] = DataArray(DeviceArray(on_device(r.transpose(2, 0, 1))), ("range_sample", "channel", "ping_time"))
    judge({k: v.data.tensor.cpu().numpy() for k, v in public_five(ds).items()}, st, s, dtype, "range transposed")
    # one range row per channel: expanded to the cube on the device
    sub = np.ascontiguousarray(r[:, 0, :])
    st2, s2 = R.rows(sv, np.broadcast_to(sub[:, None, :], sv.shape))
    ds = dataset({"Sv": sv})
    ds["echo_range"] = DataArray(DeviceArray(on_device(sub)), ("channel", "range_sample"))
    judge({k: v.data.tensor.cpu().numpy() for k, v in public_five(ds).items()}, st2, s2, dtype, "range per channel")
    # range_sample alone: the shared row, read as it is
    sv, r1, st, s = case("shared", S, dtype)
    assert r1.ndim == 1
    ds = dataset({"Sv": sv, "echo_range": r1})
    assert ds["echo_range"].dims == ("range_sample",)
    judge({k: v.data.tensor.cpu().numpy() for k, v in public_five(ds).items()}, st, s, dtype, "shared range")


def test_mixed_float_types_are_taken_as_float64():
    import echopype_amd as ep

    sv, r, _, _ = case("clean", 65, np.float32)
    r64 = r.astype(np.float64) + 1e-9  # (not float32 numbers any more)
    st, s = R.rows(sv.astype(np.float64), r64)
    out = ep.metrics.summary(dataset({"Sv": sv, "echo_range": r64}))
    judge({k: out[k].data.tensor.cpu().numpy() for k in C.STATS}, st, s, np.float64, "mixed types")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_another_range_label_with_and_without_echo_range(dtype):
    """``range_label="depth"``: four statistics are depth's alone; dispersion is about the centre of mass on echo_range
    (the reference's quirk), so it needs echo_range and says so with the default label."""
    import echopype_amd as ep

    S = 257
    sv, r, _, _ = case("sv_holes", S, dtype)
    depth = (r * dtype(0.875) + dtype(5.0)).astype(dtype)
    ds = dataset({"Sv": sv, "echo_range": r, "depth": depth})
    cm_dev = ep.metrics.center_of_mass(ds).data.tensor.cpu().numpy()  # the centres the second sweep read
    st, s = R.rows(sv, depth, cm=cm_dev.astype(np.float64))
    got = public_five(ds, "depth")
    judge({k: v.data.tensor.cpu().numpy() for k, v in got.items()}, st, s, dtype, "depth", given_cm=True)
    own = R.rows(sv, depth)[0]["dispersion"]
    assert np.all(st["dispersion"] >= own * (1 - 1e-12)) and np.any(st["dispersion"] > 1.05 * own)
    both = ep.metrics.summary(ds, range_label="depth")
    for name in C.STATS:
        np.testing.assert_array_equal(both[name].data.tensor.cpu().numpy(), got[name].data.tensor.cpu().numpy())
    # the oracle's own route (its centres in float64) agrees too, with the error of the centres charged at first order
    ref = R.dispersion({"Sv": sv, "echo_range": r, "depth": depth}, range_label="depth")
    st_e, s_e = R.rows(sv, r)
    st_o, s_o = R.rows(sv, depth, cm=st_e["center_of_mass"])
    np.testing.assert_array_equal(ref, st_o["dispersion"])
    cerr = (B.kernel_bounds(st_e, s_e)["center_of_mass"] if dtype == np.float32
            else F64_RTOL * np.abs(st_e["center_of_mass"]))
    if dtype == np.float32:
        judge({"dispersion": got["dispersion"].data.tensor.cpu().numpy()}, st_o, s_o, dtype, "depth, oracle centres",
              given_cm=True, centre_err=cerr)
    else:
        with np.errstate(all="ignore"):
            slack = (2 * np.abs(s_o["B"] - s_o["cm"] * s_o["A"]) * cerr + cerr ** 2 * np.abs(s_o["A"])) / np.abs(s_o["A"])
        judge({"dispersion": got["dispersion"].data.tensor.cpu().numpy()}, st_o, s_o, dtype, "depth, oracle centres",
              given_cm=True, extra={"dispersion": slack})
    # without echo_range
    alone = dataset({"Sv": sv, "depth": depth})
    for name in ("abundance", "center_of_mass", "evenness", "aggregation"):
        judge({name: getattr(ep.metrics, name)(alone, range_label="depth").data.tensor.cpu().numpy()}, st, s, dtype,
              f"depth alone {name}")
    for fn in (ep.metrics.dispersion, ep.metrics.summary):
        with pytest.raises(ValueError, match="^echo_range not in the input Dataset!$"):
            fn(alone, range_label="depth")


def test_helpers_on_the_device():
    import echopype_amd as ep

    for dtype in DTYPES:
        sv, r, _, _ = case("repeats", 65, dtype)
        ds = dataset({"Sv": sv, "echo_range": r})
        dz = ep.metrics.delta_z(ds)
        assert dz.dims == ("channel", "ping_time", "range_sample") and dz.data.tensor.is_cuda
        np.testing.assert_array_equal(dz.coords["range_sample"], 100 + np.arange(1, 65))
        want = R.delta_z({"echo_range": r})
        assert np.isnan(want).any()
        np.testing.assert_array_equal(dz.values, want)
        lin = ep.metrics.convert_to_linear(ds)
        assert lin.dims == dz.dims and lin.values.dtype == dtype
        np.testing.assert_allclose(lin.values, R.convert_to_linear({"Sv": sv.astype(np.float64)}),
                                   rtol=1e-5 if dtype == np.float32 else 1e-13)
    ints = dataset({"Sv": np.array([[[20, 40, 60]]]), "echo_range": np.array([[[1, 1, 3]]])}, device=False)
    np.testing.assert_array_equal(ep.metrics.delta_z(ints).values, [[[np.nan, 2.0]]])


# ---- the reference's own results ------------------------------------------------------------------------------------------------
_CASES, _, _Z = C.load_fixture()


@pytest.mark.parametrize("c", [c for c in _CASES if c["label"] != "nothing"], ids=lambda c: c["tag"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_reference_executed_results(dtype, c):
    """What the reference's own functions returned for the fixture's inputs (executed over the xarray shim).  float64: the
    float64 bar.  float32: the reference's float32 evaluation has an error of its own -- float32 products and a float32
    sum of S terms, gamma(S) of sum |term| -- so the bar is the kernel's derived bound PLUS that
    (metrics_bounds.reference_f32_slack, which test_metrics_host.py holds the same results to)."""
    import echopype_amd as ep

    dn = "f32" if dtype == np.float32 else "f64"
    inputs = C.case_inputs(_Z, c, dtype)
    ds = dataset(inputs, tuple(c["dims"]))
    label = c["label"]
    for name in C.STATS:
        err = c["results"].get(f"{dn}/{name}")
        if err is not None:
            with pytest.raises(ValueError) as e:
                getattr(ep.metrics, name)(ds, range_label=label)
            assert [type(e.value).__name__, str(e.value)] == err
            continue
        got = getattr(ep.metrics, name)(ds, range_label=label).data.tensor.cpu().numpy()
        ref = _Z[f"{c['tag']}/{dn}/{name}"].astype(np.float64)
        given = name == "dispersion" and label != "echo_range"
        with np.errstate(all="ignore"):
            if given:
                st_e, s_e = R.rows(inputs["Sv"], inputs["echo_range"])
                st, s = R.rows(inputs["Sv"], inputs[label], cm=st_e["center_of_mass"])
            else:
                st, s = R.rows(inputs["Sv"], inputs[label])
        # the reference's results take the oracle's place; the oracle supplies sum |term| and the NaN / inf pattern
        np.testing.assert_array_equal(np.isnan(ref), np.isnan(st[name]))
        st_ref = dict(st, **{name: np.where(np.isfinite(ref), ref, st[name])})
        if dtype == np.float64:
            extra = None
            if given:
                cerr = 2 * F64_RTOL * np.abs(st_e["center_of_mass"])
                with np.errstate(all="ignore"):
                    extra = {name: (2 * np.abs(s["B"] - s["cm"] * s["A"]) * cerr + cerr ** 2 * np.abs(s["A"])) / np.abs(s["A"])}
            judge({name: got}, st_ref, s, dtype, f"fixture {c['tag']}", given_cm=given, extra=extra)
        else:
            cerr = 0.0
            if given:  # both sides took their own float32 centres
                cerr = B.kernel_bounds(st_e, s_e)["center_of_mass"] + B.reference_f32_slack(st_e, s_e)["center_of_mass"]
            slack = B.reference_f32_slack(st, s, given_cm=given)  # (the centres' difference is charged once, below)
            judge({name: got}, st_ref, s, dtype, f"fixture {c['tag']}", given_cm=given, centre_err=cerr if given else 0.0,
                  extra=slack)


# ---- conditioning -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 4097])
def test_a_thin_layer_far_away_in_float64(S):
    """The 0.1 m layer at 10 000 m of test_metrics_host.py, where the oracle is held to 1e-10 of an np.longdouble
    evaluation: the device at 1e-9, through ops and through the public function, in the register and the block form."""
    import echopype_amd as ep
    from echopype_amd import ops

    sv, r = C.thin_layer(S)
    st, s = R.rows(sv, r)
    out = host(ops.echo_metrics(on_device(sv), on_device(r)))
    judge(out, st, s, np.float64, f"thin layer S={S}")
    assert np.all(np.abs(out["dispersion"] - st["dispersion"]) <= F64_RTOL * st["dispersion"])  # (without the floor)
    ds = dataset({"Sv": sv[None], "echo_range": r[None]})
    got = ep.metrics.dispersion(ds).data.tensor.cpu().numpy()[0]
    assert np.all(np.abs(got - st["dispersion"]) <= F64_RTOL * st["dispersion"])


# ---- how the work is done -----------------------------------------------------------------------------------------------------
def test_a_public_call_only_enqueues_work(monkeypatch):
    import torch

    import echopype_amd as ep

    sv, r, st, s = case("sv_holes", 257, np.float32)
    depth = (r * np.float32(0.875) + np.float32(5.0)).astype(np.float32)
    ds = dataset({"Sv": sv, "echo_range": r, "depth": depth})
    ep.metrics.summary(ds)  # (warm: the library is loaded)

    def no(*a, **k):
        raise AssertionError("host synchronisation")

    for name in ("cpu", "item", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, no)
    monkeypatch.setattr(torch.cuda, "synchronize", no)
    out = ep.metrics.summary(ds)
    five = public_five(ds)
    deep = ep.metrics.dispersion(ds, range_label="depth")
    dz, lin = ep.metrics.delta_z(ds), ep.metrics.convert_to_linear(ds)
    monkeypatch.undo()
    judge({k: out[k].data.tensor.cpu().numpy() for k in C.STATS}, st, s, np.float32, "enqueue only")
    assert all(v.data.tensor.is_cuda for v in (*five.values(), deep, dz, lin))


def test_one_kernel_per_statistic_asking_for_what_it_needs():
    import echopype_amd as ep
    from echopype_amd import _lib

    sv, r, _, _ = case("clean", 257, np.float32)
    depth = (r * np.float32(0.875) + np.float32(5.0)).astype(np.float32)
    ds = dataset({"Sv": sv, "echo_range": r, "depth": depth})
    for fn in (ep.metrics.abundance, ep.metrics.center_of_mass, ep.metrics.dispersion, ep.metrics.evenness,
               ep.metrics.aggregation, ep.metrics.summary):
        with _lib.launch_trace() as tr:
            fn(ds)
        assert tr.kernels == ["metrics_wave_kernel_unaligned"], (fn.__name__, tr.kernels)
    for fn in (ep.metrics.dispersion, ep.metrics.summary):  # the quirk: one sweep for the centres, one for the rest
        with _lib.launch_trace() as tr:
            fn(ds, range_label="depth")
        assert tr.kernels == ["metrics_wave_kernel_unaligned"] * 2, (fn.__name__, tr.kernels)


def test_a_lazy_echo_range_is_written_once():
    import torch

    import echopype_amd as ep
    from echopype_amd.xr_lite import DataArray, LazyDeviceArray

    sv, r, st, s = case("clean", 65, np.float32)
    calls = []

    def make():
        calls.append(1)
        return on_device(r)

    lazy = LazyDeviceArray(r.shape, torch.float32, torch.device("cuda", torch.cuda.current_device()), make)
    ds = dataset({"Sv": sv})
    ds["echo_range"] = DataArray(lazy, ("channel", "ping_time", "range_sample"))
    assert not lazy.materialized
    out = ep.metrics.summary(ds)
    ep.metrics.abundance(ds)
    assert lazy.materialized and calls == [1]
    judge({k: out[k].data.tensor.cpu().numpy() for k in C.STATS}, st, s, np.float32, "lazy echo_range")
