"""targets.target_spectra without a GPU: the rules' known answer (through the NumPy restatement), the frequency grid,
the parameters on the (channel, frequency) grid, every argument error raised before device work, and the conditioning of
the fixtures tests/test_gpu_target_spectra.py runs the kernel on."""
import numpy as np
import pytest
import target_spectra_cases as K
import target_spectra_ref as R


def _echodata(**kw):
    from echopype_amd import echodata, synth

    d, replicas, echoes = synth.target_spectra_scene(**kw)
    return echodata.from_ek80_arrays(d, d["filters"]), d, replicas, echoes


def _table(d, n=1, channels=None, **cols):
    from echopype_amd.xr_lite import Dataset

    d = d if channels is None else {"channel": channels}
    tab = dict(channel_index=np.zeros(n, dtype=np.int32), ping_index=np.zeros(n, dtype=np.int32),
               range_sample=np.full(n, 10, dtype=np.int32), target_range=np.full(n, 5.0), angle_alongship=np.zeros(n),
               angle_athwartship=np.zeros(n))
    tab.update(cols)
    ds = Dataset(coords={"target": np.arange(n), "channel": np.asarray(d["channel"])})
    for k, v in tab.items():
        if v is not None:
            ds[k] = (("target",), v)
    return ds


# ---- the scene -------------------------------------------------------------------------------------------------------
def test_scene_replicas_are_what_the_calibrator_builds():
    from echopype_amd.calibrate.calibrate_ek import CalibrateEK80

    ed, d, replicas, echoes = _echodata()
    assert [r.size for r in replicas] == [177, 113] and all(r.dtype == np.complex64 for r in replicas)
    cal = CalibrateEK80(ed, env_params=None, cal_params=None, ecs_file=None, waveform_mode="BB", encode_mode="complex")
    _, tx = cal._transmit_replicas()
    flat, off, max_taps = cal._replica_arrays(tx)
    assert max_taps == 177 and off.tolist() == [0, 177, 290]
    assert np.array_equal(flat, np.concatenate(replicas))
    # the stand-in filters pass the transmit band: |A| is within 3 dB of flat in band (ek80_filters(): 40 to 100 dB down)
    for c in range(2):
        f = R.grid(d["f_start"], d["f_stop"], 41)[c]
        A, kappa = R.replica_spectrum(replicas[c], K.DT, 127, f)
        assert np.ptp(20 * np.log10(np.abs(A))) < 6.0 and kappa.max() <= 10


# ---- known answer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0, 1, 12, 127])
def test_known_answer_of_an_ideal_point_echo(h):
    """Noise-free K tx on the axis: pc(s + n) = K a(n), so Y / A = K at every f, and with parameters flat in frequency
    and zero offsets  TS_uncomp(f) - TS_peak = 20 log10(f / f_c) + 2 (alpha(f) - alpha(f_c)) r."""
    from echopype_amd import synth

    Kamp, s, r, F = 0.37, 150, 23.0, 33
    d, replicas, _ = synth.target_spectra_scene(noise=0.0, echoes=[(0, 2, s, Kamp, 0.0, 0.0), (1, 0, s, Kamp, 0.0, 0.0)])
    freq = R.grid(d["f_start"], d["f_stop"], F)
    fc = (d["f_start"] + d["f_stop"]) / 2
    assert np.allclose(freq[:, F // 2], fc, rtol=1e-15)
    alpha = np.stack([np.asarray(synth.fg_absorption(freq[c])) for c in range(2)])
    flat = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64)[:, None], (2, F))  # noqa: E731
    fparams = np.stack([freq, alpha, flat([26.0, 27.5]), flat([75.0, 75.0]), flat([7.0, 6.5]), flat([7.0, 6.5]),
                        flat([0.0, 0.0]), flat([0.0, 0.0])]).transpose(1, 0, 2)
    pparams = np.stack([np.repeat(d["transmit_power"][:, None], 3, axis=1), np.asarray(d["sound_speed"]),
                        np.repeat(d["z_er"][:, None], 3, axis=1)])
    tab = dict(channel_index=np.array([0, 1]), ping_index=np.array([2, 0]), range_sample=np.array([s, s]),
               target_range=np.array([r, r]), angle_alongship=np.zeros(2), angle_athwartship=np.zeros(2))
    out = R.spectra(d["backscatter_r"], d["backscatter_i"], replicas, None, np.full(2, K.DT), fparams, pparams, h, [0, 1], tab)
    assert np.array_equal(out["TS_spectrum"], out["TS_spectrum_uncomp"])
    assert out["n_window_samples"].tolist() == [2 * h + 1] * 2
    for c in range(2):
        pc, _ = R.compress_window(d["backscatter_r"][c, tab["ping_index"][c]], d["backscatter_i"][c, tab["ping_index"][c]],
                                  replicas[c], s, 0)
        assert abs(pc[0] - Kamp) <= 1e-12 * Kamp
        alpha_c = float(synth.fg_absorption(fc[c]))
        peak = R.ts_peak(pc[0], r, fc[c], alpha_c, [26.0, 27.5][c], 75.0, d["z_er"][c], d["transmit_power"][c],
                         d["sound_speed"][c, tab["ping_index"][c]], 4)
        want = peak + 20 * np.log10(freq[c] / fc[c]) + 2 * (alpha[c] - alpha_c) * r
        assert np.max(np.abs(10.0 ** ((out["TS_spectrum_uncomp"][c] - want) / 10.0) - 1.0)) <= 1e-9


# ---- grid ------------------------------------------------------------------------------------------------------------
def test_frequency_grid():
    from echopype_amd.targets.spectra import frequency_grid

    f0, f1 = np.array([45e3, 90e3]), np.array([90e3, 170e3])
    g = frequency_grid(f0, f1, 41)
    assert g.shape == (2, 41) and np.array_equal(g, R.grid(f0, f1, 41))
    assert np.allclose(g[:, 0], f0 + 0.1 * (f1 - f0), rtol=1e-15) and np.allclose(g[:, -1], f1 - 0.1 * (f1 - f0), rtol=1e-15)
    assert np.all(np.diff(g, axis=1) > 0)
    g0 = frequency_grid(f0, f1, 2, band_margin=0.0)
    assert np.array_equal(g0, np.stack([f0, f1], axis=1))
    assert np.array_equal(frequency_grid(f0, f1, 1), ((f0 + f1) / 2)[:, None])  # F = 1: the centre, whatever the margin
    assert np.array_equal(frequency_grid(f0, f1, 1, 0.3), R.grid(f0, f1, 1, 0.3))
    one = frequency_grid(f0, f1, 5, 0.1, (50e3, 60e3))
    assert np.array_equal(one, R.grid(f0, f1, 5, 0.1, (50e3, 60e3))) and np.array_equal(one[0], one[1])
    assert one[0, 0] == 50e3 and one[0, -1] == 60e3
    pairs = [(50e3, 60e3), (100e3, 100e3)]
    per = frequency_grid(f0, f1, 1024, 0.1, pairs)
    assert per.shape == (2, 1024) and np.all(per[1] == 100e3) and np.array_equal(per, R.grid(f0, f1, 1024, 0.1, pairs))
    with pytest.raises(ValueError, match="pairs"):
        frequency_grid(f0, f1, 5, 0.1, [(1.0, 2.0)] * 3)


def test_parameters_on_the_grid_are_the_rules_of_the_centre_frequency():
    """Column j of the grid equals what get_cal_params_EK / get_env_params_EK give when f_j is the centre frequency."""
    from echopype_amd import _lib
    from echopype_amd.calibrate.cal_params import get_cal_params_EK
    from echopype_amd.calibrate.calibrate_ek import CalibrateEK80
    from echopype_amd.calibrate.env_params import get_env_params_EK
    from echopype_amd.targets.spectra import frequency_params
    from echopype_amd.xr_lite import DataArray

    ed, d, _, _ = _echodata()
    cal = CalibrateEK80(ed, env_params=None, cal_params=None, ecs_file=None, waveform_mode="BB", encode_mode="complex")
    freq = R.grid(d["f_start"], d["f_stop"], 5)
    fp = frequency_params(cal, freq)
    assert fp.shape == (8, 2, 5) and np.array_equal(fp[0], freq)
    names = _lib.TARGET_SPECTRA_FPARAM_NAMES
    for j in (0, 2, 4):
        fc = DataArray(freq[:, j].copy(), ("channel",))
        calp = get_cal_params_EK("BB", fc, cal.beam, cal.vend, {}, sonar_type="EK80")
        env = get_env_params_EK("EK80", cal.beam, ed["Environment"], {}, freq=fc)
        assert np.array_equal(fp[1, :, j], np.asarray(env["sound_absorption"].values))
        for k in range(2, 8):
            assert np.array_equal(fp[k, :, j], np.broadcast_to(np.asarray(calp[names[k]].values, dtype=np.float64), (2,))), names[k]
    # beamwidth x f_n / f; without a gain table the gain does not vary with f (the pulse-length table's value)
    assert np.allclose(fp[4], d["beamwidth_alongship"][:, None] * d["frequency_nominal"][:, None] / freq, rtol=1e-14)
    assert np.all(fp[2] == fp[2][:, :1]) and np.allclose(fp[2][:, 0], [d["gain"][0], d["gain"][1] - 0.5])
    # the user's dictionaries are the same rules
    fp2 = frequency_params(cal, freq, env_params={"sound_absorption": [0.01, 0.02]}, cal_params={"gain_correction": [20.0, 21.0]})
    assert np.array_equal(fp2[1], np.broadcast_to([[0.01], [0.02]], (2, 5))) and np.array_equal(fp2[2][:, 0], [20.0, 21.0])


# ---- arguments ---------------------------------------------------------------------------------------------------------
GOOD = {"half_window": 4, "n_frequencies": 9}


@pytest.mark.parametrize("params,match", [
    ("nope", "dict"), ({**GOOD, "window": 3}, "Unknown"), ({"half_window": 4}, "Missing"), ({"n_frequencies": 4}, "Missing"),
    ({**GOOD, "half_window": 128}, "half_window"), ({**GOOD, "half_window": -1}, "half_window"),
    ({**GOOD, "half_window": 2.5}, "half_window"), ({**GOOD, "half_window": "4"}, "half_window"),
    ({**GOOD, "half_window": True}, "half_window"), ({**GOOD, "n_frequencies": 0}, "n_frequencies"),
    ({**GOOD, "n_frequencies": 1025}, "n_frequencies"), ({**GOOD, "n_frequencies": None}, "n_frequencies"),
    ({**GOOD, "n_frequencies": float("nan")}, "n_frequencies"), ({**GOOD, "band_margin": 0.5}, "band_margin"),
    ({**GOOD, "band_margin": -0.1}, "band_margin"), ({**GOOD, "band_margin": "a"}, "band_margin"),
    ({**GOOD, "frequency_limits": (1.0,)}, "frequency_limits"), ({**GOOD, "frequency_limits": "ab"}, "frequency_limits"),
    ({**GOOD, "frequency_limits": (60e3, 50e3)}, "frequency_limits"),
    ({**GOOD, "frequency_limits": (float("nan"), 50e3)}, "frequency_limits"),
    ({**GOOD, "frequency_limits": [(50e3, 60e3)] * 3}, "frequency_limits"),
])
def test_parameter_errors_come_before_any_device_work(params, match, monkeypatch):
    import echopype_amd as ep
    from echopype_amd import ops

    ed, d, _, _ = _echodata()
    monkeypatch.setattr(ops, "to_device", lambda *a, **k: pytest.fail("device work"))
    monkeypatch.setattr(ops, "to_device_small", lambda *a, **k: pytest.fail("device work"))
    with pytest.raises(ValueError, match=match):
        ep.targets.target_spectra(_table(d), ed, params)


def test_table_and_file_errors(monkeypatch):
    import echopype_amd as ep
    from echopype_amd import echodata, ops, synth

    monkeypatch.setattr(ops, "to_device", lambda *a, **k: pytest.fail("device work"))
    monkeypatch.setattr(ops, "to_device_small", lambda *a, **k: pytest.fail("device work"))
    ed, d, _, _ = _echodata()
    with pytest.raises(ValueError, match="target_range"):
        ep.targets.target_spectra(_table(d, target_range=None), ed, GOOD)
    with pytest.raises(ValueError, match="ES333"):
        ep.targets.target_spectra(_table(d, channels=[d["channel"][0], "WBT 9-9 ES333"]), ed, GOOD)
    with pytest.raises(ValueError, match="holds"):
        ep.targets.target_spectra(_table(d, channel_index=np.zeros(1)), ed, GOOD)
    with pytest.raises(ValueError, match="dtype"):
        ep.targets.target_spectra(_table(d), ed, GOOD, dtype="int32")
    # files without BB complex samples: CW complex samples, and an EK60 file
    cw = synth.ek80_numpy(C=2, P=3, S=64, waveform="CW")
    with pytest.raises(TypeError, match="BB"):
        ep.targets.target_spectra(_table(cw), echodata.from_ek80_arrays(cw, synth.ek80_filters()), GOOD)
    e60 = synth.ek60_numpy(C=2, P=3, S=64)
    with pytest.raises(TypeError, match="EK60"):
        ep.targets.target_spectra(_table(e60), echodata.from_ek60_arrays(e60), GOOD)


def test_sample_interval_must_be_one_value_per_replica_over_the_pings_that_hold_targets():
    from echopype_amd.targets.spectra import replica_sample_interval

    rid = np.array([[0, 0, 2], [1, 1, -1]])
    si = np.array([[8e-6, 16e-6, 8e-6], [4e-6, 4e-6, 4e-6]])
    hold = np.array([[True, False, True], [False, True, True]])
    assert np.array_equal(replica_sample_interval(rid, si, hold), [8e-6, 4e-6, 8e-6])
    assert np.array_equal(replica_sample_interval(rid, si, np.zeros((2, 3), dtype=bool)), [8e-6, 4e-6, 8e-6])
    with pytest.raises(ValueError, match="sample_interval"):
        replica_sample_interval(rid, si, np.ones((2, 3), dtype=bool))


def test_library_checks_its_arguments_without_a_gpu():
    from echopype_amd import _lib, ops

    def call(**kw):
        a = dict(C=2, P=3, S=400, B=4, R=2, rep_len=10, max_taps=100, F=5, h=4, n_map=2, N=1)
        a.update(kw)
        _lib.call("epa_target_spectra", None, None, _lib.F64, a["C"], a["P"], a["S"], a["B"], None, None, None, a["R"],
                  a["rep_len"], a["max_taps"], None, None, a["F"], a["h"], None, None, a["n_map"], None, None, None, None,
                  None, None, a["N"], None, None, None, _lib.F64, None, None)

    for kw, match in ((dict(max_taps=2049), "2048 taps"), (dict(h=128), "half_window"), (dict(F=1025), "frequencies"),
                      (dict(B=9), "sectors"), (dict(S=0), "bad shape"), (dict(R=1), "replica_id"), (dict(), "NULL")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    call(N=0)  # no rows: nothing to do, nothing is dereferenced
    assert ops.scratch_bytes("target_spectra.table", 3, 41) == 3 * _lib.TARGET_SPECTRA_TABLE_ROWS * 41 * 8


# ---- conditioning of the GPU fixtures ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 3])
def test_conditioning_of_the_fixtures(B):
    """kappa = sum |terms| / |sum| of the Fourier sums the kernel test compares, with band_margin 0.1 and the band-pass
    stand-in filters: a CONDITION on the fixtures, not a measurement of the kernel.
    - A(f), every replica, and Y(f) on the signal rows (the peaks of whole echoes): kappa <= 10, for h in {1, 4, 16, 32,
      64, 127} and both bands.
    - Y(f) on the four edge rows (the last sample of a row, a sample inside the NaN tail): their windows hold the far
      side lobes of an echo or one the edge cuts off, which no choice of samples makes well conditioned at every
      frequency; kappa <= 100 at the window sizes the kernel test uses.  The rounding of a sum of n <= 2h + L = 431
      terms is about n 2**-53 kappa <= 5e-12 there, still 200 times inside the 1e-9 the kernel test asks."""
    d, replicas, echoes = K.scene(B, "float64")
    ns = K.n_signal(echoes, replicas)
    tab = K.table(echoes, replicas)
    assert ns == 10 and {0, K.S - K.TAIL - 178, K.S - 177, K.S // 2} <= set(tab["range_sample"][:ns].tolist())
    assert tab["range_sample"][ns:ns + 4].tolist() == [K.S - 1, K.S - K.TAIL + 12] * 2
    for h in (1, 4, 16, 32, 64, 127):
        for F in (1, 41, 257) if h in K.H_ALL else (41,):
            w = K.reference(B, "float64", h, F)
            fin = np.isfinite(w["TS_spectrum_uncomp"])
            assert fin[:ns].all()
            assert np.nanmax(w["kappa_A"]) <= 10 and w["kappa_Y"][:ns].max() <= 10, (h, F)
            if h in K.H_ALL:
                edge = np.where(fin[ns:ns + 4], w["kappa_Y"][ns:ns + 4], 0.0)
                assert edge.max() <= 100, (h, F, edge.max())
    for h in K.H_ALL:  # ... and with two filter intervals, on a subset of channels
        w = K.reference(B, "float64", h, 41, two_intervals=True)
        assert np.nanmax(w["kappa_A"]) <= 10 and w["kappa_Y"][:ns].max() <= 10
    w = K.reference(B, "float64", 16, 41, channels=(1,))
    assert w["kappa_Y"][:K.n_signal(echoes, replicas, (1,))].max() <= 10
