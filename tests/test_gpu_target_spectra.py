"""targets.target_spectra on the GPU (csrc/target_spectrum.hip through ops.target_spectra and targets/spectra.py) against
the NumPy restatement tests/target_spectra_ref.py, on the fixtures of tests/target_spectra_cases.py: C = 2 (replicas of
177 and 113 taps), P = 3, S = 400, four and three sectors, float32 and float64 cubes.

What is compared how
- EQUAL: the NaN patterns of both spectra and ``n_window_samples``.
- 10^(TS/10) within 1e-9 relative of the oracle, the project's float64 bar.  tests/test_target_spectra_host.py holds the
  conditioning of the Fourier sums of these fixtures at kappa <= 10 on the signal rows and <= 100 on the edge rows: a
  sum of n <= 2h + L = 431 terms is off by about n 2**-53 kappa <= 5e-12 relative however it is ordered (the kernel adds
  the sectors first, splits the taps over lanes and evaluates the Fourier sum by Horner's rule; the oracle does none of
  these), and the chain after it is a dozen float64 operations.
- float32 output: the same after one rounding -- the value lies between the float32 roundings of the two ends of that
  interval about the oracle."""
import numpy as np
import pytest
import target_spectra_cases as K
import target_spectra_ref as R

pytestmark = pytest.mark.gpu

REL = 1e-9
DB = 10.0 * np.log10(1.0 + REL)  # what 1e-9 relative of 10^(TS/10) is in dB
COLS = ("channel_index", "ping_index", "range_sample", "target_range", "angle_alongship", "angle_athwartship")


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m 'not gpu' on CPU boxes)")
    from echopype_amd import ops

    return torch, ops


def _dev(torch, a):
    return torch.as_tensor(np.array(a)).cuda()  # (a copy: the fixtures are read-only)


def _run(env, B, dtype, h, F, two=False, channels=(0, 1), extra=True, out_dtype="float64", tab=None):
    torch, ops = env
    d, replicas, echoes = K.scene(B, dtype)
    fparams, pparams, rep_dt, reps, rid = K.params(d, F, replicas, two)
    tab = K.table(echoes, replicas, channels, extra) if tab is None else tab
    flat = np.concatenate(reps).astype(np.complex64)
    off = np.concatenate([[0], np.cumsum([r.size for r in reps])]).astype(np.int32)
    return ops.target_spectra(_dev(torch, d["backscatter_r"]), _dev(torch, d["backscatter_i"]),
                              _dev(torch, flat.view(np.float32)), _dev(torch, off), max(r.size for r in reps),
                              _dev(torch, rep_dt), _dev(torch, fparams), _dev(torch, pparams), h,
                              _dev(torch, np.asarray(channels, dtype=np.int32)), *(_dev(torch, tab[k]) for k in COLS),
                              replica_id=None if rid is None else _dev(torch, rid), dtype=out_dtype)


def _compare(got, want, out_dtype="float64"):
    ts, tu, nw = (t.cpu().numpy() for t in got)
    assert nw.dtype == np.int32 and np.array_equal(nw, want["n_window_samples"])
    worst = {}
    for name, g in (("TS_spectrum", ts), ("TS_spectrum_uncomp", tu)):
        ref = want[name]
        assert g.dtype == np.dtype(out_dtype) and g.shape == ref.shape
        assert np.array_equal(np.isnan(g), np.isnan(ref)), name
        f = ~np.isnan(ref)
        if out_dtype == "float64":
            worst[name] = float(np.max(np.abs(10.0 ** ((g[f] - ref[f]) / 10.0) - 1.0))) if f.any() else 0.0
        else:
            lo, hi = (ref[f] - DB).astype(np.float32), (ref[f] + DB).astype(np.float32)
            worst[name] = float(np.max(np.maximum(lo - g[f], g[f] - hi))) if f.any() else 0.0
    print("largest error (float64: relative, of 10^(TS/10); float32: dB outside the rounded interval):", worst)
    for name, e in worst.items():
        assert e <= (REL if out_dtype == "float64" else 0.0), (name, e)


@pytest.mark.parametrize("F", K.F_ALL)
@pytest.mark.parametrize("h", K.H_ALL)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("B", [4, 3])
def test_kernel_equals_the_restatement(env, B, dtype, h, F):
    """Every row kind of the fixture table: whole echoes (one at sample 0, one with the mixed-sector patch inside, one
    in front of the NaN tail, one ending with the row), the last sample S - 1 (the replica zero-fills past the row), a
    window inside the NaN tail, NaN angles, NaN and non-positive ranges, indices outside the cube."""
    want = K.reference(B, dtype, h, F)
    assert np.isfinite(want["TS_spectrum"]).all(axis=1).sum() >= 10 and (want["n_window_samples"] == 0).sum() >= 7
    assert np.isfinite(want["TS_spectrum_uncomp"]).all(axis=1).sum() >= 14  # (the rows with a NaN angle as well)
    _compare(_run(env, B, dtype, h, F), want)


@pytest.mark.parametrize("h,F", [(1, 41), (127, 257)])
def test_two_filter_intervals(env, h, F):
    """``replica_id``: the last ping of every channel is compressed with another, shorter replica."""
    want = K.reference(4, "float64", h, F, two_intervals=True)
    one = K.reference(4, "float64", h, F)
    assert not np.array_equal(want["TS_spectrum"], one["TS_spectrum"], equal_nan=True)
    _compare(_run(env, 4, "float64", h, F, two=True), want)


@pytest.mark.parametrize("channels", [(1,), (1, 0)])
def test_a_subset_of_channels_and_another_order(env, channels):
    want = K.reference(4, "float32", 16, 41, channels=channels)
    _compare(_run(env, 4, "float32", 16, 41, channels=channels), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float32_output_is_the_float64_result_rounded_once(env, dtype):
    want = K.reference(4, dtype, 16, 41)
    _compare(_run(env, 4, dtype, 16, 41, out_dtype="float32"), want, "float32")


def test_one_target_and_no_target(env):
    from echopype_amd import _lib

    torch, ops = env
    d, replicas, echoes = K.scene(4, "float64")
    full = K.table(echoes, replicas, extra=False)
    one = {k: v[1:2] for k, v in full.items()}
    want = K.reference(4, "float64", 16, 41, extra=False)
    got = _run(env, 4, "float64", 16, 41, tab=one)
    _compare(got, {k: v[1:2] for k, v in want.items()})
    none = {k: v[:0] for k, v in full.items()}
    with _lib.launch_trace() as tr:
        ts, tu, nw = _run(env, 4, "float64", 16, 41, tab=none)
    assert tr.kernels == [] and ts.shape == tu.shape == (0, 41) and nw.shape == (0,) and nw.dtype == torch.int32


def test_both_kernels_serve_a_call(env):
    from echopype_amd import _lib

    with _lib.launch_trace() as tr:
        _run(env, 4, "float64", 1, 1)
    assert tr.kernels == ["target_spectrum_replica_kernel", "target_spectrum_kernel"]


def test_arguments_are_checked_before_anything_is_launched(env):
    from echopype_amd import _lib

    torch, ops = env
    d, replicas, echoes = K.scene(4, "float64")
    fparams, pparams, rep_dt, reps, _ = K.params(d, 5, replicas)
    tab = K.table(echoes, replicas, extra=False)
    long = np.zeros(2049, dtype=np.complex64)
    off = np.array([0, 2049, 2049 + reps[1].size], dtype=np.int32)
    flat = np.concatenate([long, reps[1]])
    args = [_dev(torch, d["backscatter_r"]), _dev(torch, d["backscatter_i"]), _dev(torch, flat.view(np.float32)),
            _dev(torch, off), 2049, _dev(torch, rep_dt), _dev(torch, fparams), _dev(torch, pparams), 4,
            _dev(torch, np.arange(2, dtype=np.int32))] + [_dev(torch, tab[k]) for k in COLS]
    with _lib.launch_trace() as tr:
        with pytest.raises(ValueError, match="2048 taps"):
            ops.target_spectra(*args)
        args[4] = 177
        args[8] = 128
        with pytest.raises(ValueError, match="half_window"):
            ops.target_spectra(*args)
        args[8] = 4
        args[7] = _dev(torch, pparams[:2])
        with pytest.raises(ValueError, match="pparams"):
            ops.target_spectra(*args)
    assert tr.kernels == []
    # the library's own checks (the binding is bypassed): nothing is launched either
    with _lib.launch_trace() as tr:
        with pytest.raises(ValueError, match="2048 taps"):
            _lib.call("epa_target_spectra", None, None, _lib.F64, 2, 3, 400, 4, None, None, None, 2, 10, 4096, None, None, 5, 4,
                      None, None, 2, None, None, None, None, None, None, 1, None, None, None, _lib.F64, None, None)
        with pytest.raises(ValueError, match="NULL"):
            _lib.call("epa_target_spectra", None, None, _lib.F64, 2, 3, 400, 4, None, None, None, 2, 10, 100, None, None, 5, 4,
                      None, None, 2, None, None, None, None, None, None, 1, None, None, None, _lib.F64, None, None)
    assert tr.kernels == []


def test_guard_bands_behind_the_outputs_and_the_scratch_table_stay_untouched(env, monkeypatch):
    """The three outputs and the scratch table between bands of 0xA5: the kernels write what they own and nothing else,
    also for rows whose indices are outside the cube."""
    torch, ops = env
    band, fill = 4096, 0xA5
    bufs = []
    real_empty = torch.empty

    def banded(nbytes, dtype, device):
        raw = real_empty(band + nbytes + band, dtype=torch.uint8, device=device)
        raw[:band] = fill
        raw[band + nbytes:] = fill
        bufs.append((raw, nbytes))
        return raw[band:band + nbytes].view(dtype)

    def empty(shape, dtype=None, device=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape)) * dtype.itemsize
        return banded(-(-n // 256) * 256, dtype, device)[:int(np.prod(shape))].view(shape)

    want = K.reference(4, "float64", 16, 41)
    plain = [t.cpu().numpy() for t in _run(env, 4, "float64", 16, 41)]
    d, replicas, echoes = K.scene(4, "float64")
    fparams, pparams, rep_dt, reps, rid = K.params(d, 41, replicas)
    tab = K.table(echoes, replicas)
    flat = np.concatenate(reps).astype(np.complex64)
    off = np.concatenate([[0], np.cumsum([r.size for r in reps])]).astype(np.int32)
    args = [_dev(torch, d["backscatter_r"]), _dev(torch, d["backscatter_i"]), _dev(torch, flat.view(np.float32)),
            _dev(torch, off), 177, _dev(torch, rep_dt), _dev(torch, fparams), _dev(torch, pparams), 16,
            _dev(torch, np.arange(2, dtype=np.int32))] + [_dev(torch, tab[k]) for k in COLS]
    monkeypatch.setattr(ops, "_scratch_alloc", lambda nbytes, dtype, device, zero: banded(
        -(-nbytes // dtype.itemsize) * dtype.itemsize, dtype, device))
    monkeypatch.setattr(ops.torch, "empty", empty)
    got = ops.target_spectra(*args)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(bufs) == 4  # TS_spectrum, TS_spectrum_uncomp, n_window_samples, the table
    for raw, n in bufs:
        assert bool((raw[:band] == fill).all()) and bool((raw[band + n:] == fill).all())
    for a, b in zip(plain, got):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)
    _compare(got, want)


# ---- the public entry point -------------------------------------------------------------------------------------------
def _echodata(B=4, dtype="float64", noise=1e-4, echoes=None):
    from echopype_amd import echodata, synth

    d, replicas, echoes = synth.target_spectra_scene(B=B, dtype=np.dtype(dtype), noise=noise, echoes=echoes)
    return echodata.from_ek80_arrays(d, d["filters"]), d, replicas, echoes


def _oracle_for(ed, d, out, tab, h, F, params_extra=None):
    """The oracle fed with the arrays and parameter tables the entry point works from."""
    from echopype_amd.calibrate.calibrate_ek import CalibrateEK80
    from echopype_amd.targets import spectra

    cal = CalibrateEK80(ed, env_params=None, cal_params=None, ecs_file=None, waveform_mode="BB", encode_mode="complex")
    freq = R.grid(d["f_start"], d["f_stop"], F, **(params_extra or {}))
    fp = spectra.frequency_params(cal, freq)  # (8, C, F)
    _, tx = cal._transmit_replicas()
    reps = [np.asarray(tx[ch]).astype(np.complex64) for ch in cal.beam["channel"].values]
    Cn, Pn = d["backscatter_r"].shape[:2]
    pparams = np.stack([np.repeat(d["transmit_power"][:, None], Pn, axis=1),
                        np.broadcast_to(np.asarray(cal.env_params["sound_speed"].values
                                                   if hasattr(cal.env_params["sound_speed"], "values")
                                                   else cal.env_params["sound_speed"], dtype=np.float64), (Cn, Pn)),
                        np.repeat(d["z_er"][:, None], Pn, axis=1)])
    want = R.spectra(d["backscatter_r"], d["backscatter_i"], reps, None, np.full(Cn, K.DT), fp.transpose(1, 0, 2), pparams, h,
                     list(range(Cn)), tab)
    assert np.array_equal(out["frequency"].values, freq)
    return want


def _table_dataset(tab, channels):
    from echopype_amd.xr_lite import Dataset

    ds = Dataset(coords={"target": np.arange(len(tab["channel_index"])), "channel": np.asarray(channels)})
    for k in COLS:
        ds[k] = (("target",), tab[k])
    return ds


def test_whole_chain_from_ek80_fm_samples():
    """compute_TS -> add_splitbeam_angle -> detect_single_targets -> target_spectra on the scene equals the oracle fed
    with the same table."""
    import echopype_amd as ep

    ed, d, replicas, echoes = _echodata()
    ds = ep.calibrate.compute_TS(ed, waveform_mode="BB", encode_mode="complex")
    ds = ep.consolidate.add_splitbeam_angle(ds, ed, "BB", "complex", pulse_compression=True, to_disk=False)
    ts = np.asarray(ds["TS"].values)
    # (the echoes are 16 dB apart in strength and, 40 log r over 0.2 .. 1.7 m, 37 dB apart in range; the noise floor
    #  lies 80 dB below them)
    prm = {"TS_threshold": float(np.nanmax(ts)) - 55.0, "pldl": 6.0, "min_norm_pulse_length": 0.0,
           "max_norm_pulse_length": 2.0, "max_beam_compensation": 1e3, "max_std_alongship": 1e3,
           "max_std_athwartship": 1e3, "pulse_length_samples": d["tau"] / K.DT}
    targets = ep.targets.detect_single_targets(ds, "split_beam", prm)
    n = targets["target"].shape[0]
    assert n >= 4
    out = ep.targets.target_spectra(targets, ed, {"half_window": 8, "n_frequencies": 21})
    tab = {k: np.asarray(targets[k].values) for k in COLS}
    want = _oracle_for(ed, d, out, tab, 8, 21)
    assert out["TS_spectrum"].dims == ("target", "frequency_index") and out["TS_spectrum"].shape == (n, 21)
    assert [str(c) for c in out["channel"].values] == [str(c) for c in targets["channel"].values]
    assert np.isfinite(want["TS_spectrum_uncomp"]).all(axis=1).sum() >= 4
    _compare([out[k].data.tensor for k in ("TS_spectrum", "TS_spectrum_uncomp", "n_window_samples")], want)


def test_known_answer_on_the_device():
    """A noise-free point echo on the axis: Y / A = K at every f, so with parameters flat in frequency and zero offsets
    TS_uncomp(f) - TS_peak = 20 log10(f / f_c) + 2 (alpha(f) - alpha(f_c)) r."""
    import echopype_amd as ep
    from echopype_amd.utils.uwa import calc_absorption

    Kamp, s, r = 0.37, 150, 23.0
    # (pings whose samples are all valid: the NaN patches of the scene are on (0, 0), (1, 2) and ping 1)
    ed, d, replicas, _ = _echodata(noise=0.0, echoes=[(0, 2, s, Kamp, 0.0, 0.0), (1, 0, s, Kamp, 0.0, 0.0)])
    tab = dict(channel_index=np.array([0, 1], dtype=np.int32), ping_index=np.array([2, 0], dtype=np.int32),
               range_sample=np.full(2, s, dtype=np.int32), target_range=np.full(2, r), angle_alongship=np.zeros(2),
               angle_athwartship=np.zeros(2))
    F = 33
    cal = {"gain_correction": [26.0, 27.5], "impedance_transducer": [75.0, 75.0], "beamwidth_alongship": [7.0, 6.5],
           "beamwidth_athwartship": [7.0, 6.5], "angle_offset_alongship": [0.0, 0.0], "angle_offset_athwartship": [0.0, 0.0]}
    out = ep.targets.target_spectra(_table_dataset(tab, d["channel"]), ed, {"half_window": 12, "n_frequencies": F},
                                    cal_params=cal)
    got = out["TS_spectrum_uncomp"].values
    assert np.array_equal(out["TS_spectrum"].values, got)  # on the axis, zero offsets: no compensation
    freq = out["frequency"].values
    fc = (d["f_start"] + d["f_stop"]) / 2
    assert np.allclose(freq[:, F // 2], fc, rtol=1e-15)
    c_w = float(np.asarray(d["sound_speed"]).flat[0])
    for c in range(2):
        alpha, alpha_c = (np.asarray(calc_absorption(frequency=f, temperature=10.0, salinity=35.0, pressure=10.0, pH=8.0,
                                                     sound_speed=c_w, formula_source="FG")) for f in (freq[c], fc[c]))
        peak = R.ts_peak(Kamp, r, fc[c], float(alpha_c), cal["gain_correction"][c], 75.0, d["z_er"][c],
                         d["transmit_power"][c], c_w, 4)
        want = peak + 20 * np.log10(freq[c] / fc[c]) + 2 * (alpha - alpha_c) * r
        err = np.max(np.abs(10.0 ** ((got[c] - want) / 10.0) - 1.0))
        print("channel", c, "largest relative error of 10^(TS/10) against the known answer:", err)
        # the echo is K tx with tx rounded to complex64 and the cube float64: pc(s + n) = K a(n) up to float64 rounding
        assert err <= REL


def test_two_calls_agree_and_the_host_waits_once():
    import torch

    import echopype_amd as ep
    from echopype_amd.targets import spectra

    ed, d, replicas, echoes = _echodata()
    tab = K.table(echoes, replicas)
    ds = _table_dataset({k: v[:-1] for k, v in tab.items()}, d["channel"])  # (without the row of 2**31 - 1)
    reads = []
    real = spectra._to_host
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(spectra, "_to_host", lambda t: (reads.append(t.numel()), real(t))[1])
        mp.setattr(torch.cuda, "synchronize", lambda *a, **k: pytest.fail("synchronize"))
        a = ep.targets.target_spectra(ds, ed, {"half_window": 16, "n_frequencies": 41})
        assert len(reads) == 1
        b = ep.targets.target_spectra(ds, ed, {"half_window": 16, "n_frequencies": 41})
        assert len(reads) == 2
    for k in ("TS_spectrum", "TS_spectrum_uncomp", "n_window_samples", "frequency"):
        assert np.array_equal(a[k].values, b[k].values, equal_nan=True), k
    assert np.isfinite(a["TS_spectrum"].values).any()


def test_a_file_with_two_filter_intervals_equals_the_file_with_one():
    """The same filter set recorded at two filter_time stamps: four (channel, interval) replicas and a replica index
    per ping, picked as compute_TS picks them -- the same bits as the file with one interval."""
    import echopype_amd as ep
    from echopype_amd import echodata

    ed, d, replicas, echoes = _echodata()
    ed2 = echodata.from_ek80_arrays(d, d["filters"], filter_time_idx=[0, 2])
    tab = K.table(echoes, replicas)
    ds = _table_dataset({k: v[:-1] for k, v in tab.items()}, d["channel"])
    prm = {"half_window": 16, "n_frequencies": 41, "frequency_limits": [(50e3, 85e3), (95e3, 160e3)]}
    a, b = ep.targets.target_spectra(ds, ed, prm), ep.targets.target_spectra(ds, ed2, prm)
    assert a["frequency"].values[0, 0] == 50e3 and a["frequency"].values[1, -1] == 160e3
    for k in ("TS_spectrum", "TS_spectrum_uncomp", "n_window_samples", "frequency"):
        assert np.array_equal(a[k].values, b[k].values, equal_nan=True), k
    assert np.isfinite(a["TS_spectrum"].values).all(axis=1).sum() >= 10


def test_empty_table_gives_the_variables_without_a_launch():
    import echopype_amd as ep
    from echopype_amd import _lib
    from echopype_amd.targets import spectra

    ed, d, replicas, echoes = _echodata()
    tab = {k: v[:0] for k, v in K.table(echoes, replicas).items()}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(spectra, "_to_host", lambda t: pytest.fail("a synchronisation for an empty table"))
        with _lib.launch_trace() as tr:
            out = ep.targets.target_spectra(_table_dataset(tab, d["channel"]), ed, {"half_window": 3, "n_frequencies": 7})
    assert tr.kernels == []
    assert out["TS_spectrum"].shape == out["TS_spectrum_uncomp"].shape == (0, 7)
    assert out["n_window_samples"].shape == (0,) and out["frequency"].shape == (2, 7)


def test_device_errors_of_the_entry_point():
    """A sample interval that changes over the pings of a replica that hold targets."""
    import echopype_amd as ep
    from echopype_amd import echodata

    ed, d, replicas, echoes = _echodata()
    beam = ed[echodata.BEAM1]
    si = np.array(beam["sample_interval"].values)
    si[0, 2] *= 2
    beam["sample_interval"] = (("channel", "ping_time"), si)
    tab = K.table(echoes, replicas, extra=False)
    with pytest.raises(ValueError, match="sample_interval"):
        ep.targets.target_spectra(_table_dataset(tab, d["channel"]), ed, {"half_window": 3, "n_frequencies": 7})
    keep = tab["ping_index"] != 2  # no target on the ping that differs: served
    out = ep.targets.target_spectra(_table_dataset({k: v[keep] for k, v in tab.items()}, d["channel"]), ed,
                                    {"half_window": 3, "n_frequencies": 7})
    assert np.isfinite(out["TS_spectrum"].values).all()
