"""calibrate.compute_Sv_spectrum without a GPU: the NumPy restatement against a second formulation, its scaling
invariants, the cell centres and cell counts, every argument error raised before device work, and the conditioning of
the fixtures tests/test_gpu_sv_spectrum.py runs the kernel on."""
import numpy as np
import pytest
import sv_spectrum_cases as K
import sv_spectrum_ref as R


def _echodata(**kw):
    from echopype_amd import echodata, synth

    d, replicas, echoes = synth.target_spectra_scene(**kw)
    return echodata.from_ek80_arrays(d, d["filters"]), d, replicas, echoes


# ---- the oracle against a second formulation ---------------------------------------------------------------------------
NFFT = 500  # bins of 1 / (NFFT dt) = 250 Hz at dt = 8 us
# frequency_limits that put every frequency of the grid on a bin: channel 0 in the first Nyquist zone of the 125 kHz
# sample rate, channel 1 across 125 kHz (bins 400 .. 499, 0 .. 40 after aliasing)
LIMITS = [(50e3, 85e3), (100e3, 135e3)]
F_BINS = 141


def _second_formulation(re, im, tx, dt, c_w, Nw, hop, kind, f):
    """Sv-free half of the rules for one ping by other means: np.convolve for the compression of every sector, np.fft.fft
    of the zero-padded windowed cell for Y, np.fft.fft of the circularly placed lags for A.  -> |Y / A|^2 (M, F), NaN
    for cells that hold an invalid sample."""
    S, B = re.shape
    L = tx.size
    t = tx.astype(np.complex128)
    E = np.sum(np.abs(t) ** 2)
    ok = ~np.isnan(re) & ~np.isnan(im)
    z = np.where(ok, re.astype(np.float64) + 1j * im.astype(np.float64), 0.0)
    # sum_k z(n + k) conj(t(k)) = (z * reversed conj t)(n + L - 1)
    pcb = np.stack([np.convolve(z[:, b], np.conj(t)[::-1])[L - 1:L - 1 + S] for b in range(B)], axis=1) / E
    nv = ok.sum(axis=1)
    pc = np.where(nv > 0, (pcb * ok).sum(axis=1) / np.maximum(nv, 1), 0.0)
    ps = np.arange(S) * dt * c_w / 2 * pc
    q = np.rint(np.asarray(f) * dt * NFFT).astype(np.int64)
    assert np.array_equal(q / (dt * NFFT), f)  # on the bins, exactly
    q %= NFFT
    hh = min((Nw - 1) // 2, L - 1)
    lags = np.zeros(NFFT, dtype=np.complex128)
    ac = np.correlate(t, t, "full") / E  # ac[L - 1 + j] = sum_k t(k + j) conj(t(k))
    for j in range(-hh, hh + 1):
        lags[j % NFFT] = ac[L - 1 + j]
    A = np.fft.fft(lags)[q]
    wt = R.window(Nw, kind)
    M = R.n_cells(S, Nw, hop)
    out = np.full((M, len(f)), np.nan)
    for m in range(M):
        n0 = m * hop
        if not (nv[n0:n0 + Nw] > 0).all():
            continue
        Y = np.fft.fft(wt * ps[n0:n0 + Nw], NFFT)[q]
        out[m] = np.abs(Y / A) ** 2
    return out


@pytest.mark.parametrize("Nw,hop,kind", [(64, 32, "hann"), (255, 128, "hann"), (16, 23, "rectangular"), (400, 200, "hann")])
def test_oracle_equals_a_second_formulation_on_fft_bins(Nw, hop, kind):
    d, replicas, _ = K.scene(4, "float64")
    fparams, pparams, rep_dt, reps, rid = K.params(d, F_BINS, replicas)
    freq = _bin_grid()
    fparams = fparams.copy()
    fparams[:, 0] = freq
    want = R.sv_spectrum(d["backscatter_r"], d["backscatter_i"], reps, rid, rep_dt, fparams, pparams, Nw, hop, kind)
    worst, compared = 0.0, 0
    for c in range(K.C):
        f, alpha, G, z_et, psi = fparams[c]
        for p in range(K.P):
            p_t, c_w, z_er, dt = pparams[:, c, p]
            ya = _second_formulation(d["backscatter_r"][c, p], d["backscatter_i"][c, p], replicas[c], dt, c_w, Nw, hop, kind, f)
            prx = 4 * ya / 8 * (np.abs(z_er + z_et) / z_er) ** 2 / z_et
            r_m = want["echo_range"][c, p][:, None]
            lin = prx * 10 ** (2 * alpha * r_m / 10) / (p_t * (c_w / f) ** 2 * c_w / (32 * np.pi ** 2)) \
                / 10 ** (2 * G / 10) / (Nw * dt) / 10 ** (psi / 10)
            got = 10 ** (want["Sv_spectrum"][c, p] / 10)
            assert np.array_equal(np.isnan(got), np.isnan(lin) | ~(r_m > 0))
            fin = ~np.isnan(got)
            compared += int(fin.sum())
            if fin.any():
                worst = max(worst, float(np.max(np.abs(got[fin] / lin[fin] - 1.0))))
    assert compared >= 4 * F_BINS  # (N_w = S: one cell per ping, NaN on the ping with the NaN tail)
    print("largest relative difference of 10^(Sv/10) between the two formulations:", worst)
    assert worst <= 1e-10


def _bin_grid():
    from echopype_amd.targets.spectra import frequency_grid

    return frequency_grid([45e3, 90e3], [90e3, 170e3], F_BINS, 0.1, LIMITS)


# ---- scaling ---------------------------------------------------------------------------------------------------------
def test_scaling_invariants():
    """Samples doubled: + 20 log10 2 on every finite value.  Transmit power doubled: - 10 log10 2.  Within 1e-12 dB."""
    d, replicas, _ = K.scene(4, "float64")
    fparams, pparams, rep_dt, reps, rid = K.params(d, 41, replicas)
    base = K.reference(4, "float64", 64, None, 41)["Sv_spectrum"]
    twice = R.sv_spectrum(2 * d["backscatter_r"], 2 * d["backscatter_i"], reps, rid, rep_dt, fparams, pparams, 64, 32)
    pp2 = pparams.copy()
    pp2[0] *= 2
    power = R.sv_spectrum(d["backscatter_r"], d["backscatter_i"], reps, rid, rep_dt, fparams, pp2, 64, 32)
    fin = np.isfinite(base)
    assert fin.sum() > 2000
    for other, shift in ((twice, 20 * np.log10(2.0)), (power, -10 * np.log10(2.0))):
        assert np.array_equal(np.isfinite(other["Sv_spectrum"]), fin)
        assert np.max(np.abs(other["Sv_spectrum"][fin] - base[fin] - shift)) <= 1e-12


# ---- cells -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nw,hop", [(64, 32), (64, 64), (64, 71), (2, 1), (400, 7), (255, 128)])
def test_cell_centres_and_cell_count(Nw, hop):
    """echo_range = the mean of compute_Sv's BB echo_range (its restatement, oracle/calibrate.py) over the first and the
    last sample of the cell, to the bit; M = floor((S - N_w) / hop) + 1 for hop <, = and > N_w."""
    from oracle import calibrate as ocal

    from echopype_amd import ops

    d, replicas, _ = K.scene(4, "float64")
    fparams, pparams, rep_dt, reps, rid = K.params(d, 1, replicas)
    want = R.sv_spectrum(d["backscatter_r"], d["backscatter_i"], reps, rid, rep_dt, fparams, pparams, Nw, hop, "rectangular")
    M = len(range(0, K.S - Nw + 1, hop))
    assert want["echo_range"].shape == (K.C, K.P, M) and want["Sv_spectrum"].shape == (K.C, K.P, M, 1)
    assert ops.sv_spectrum_cells(K.S, Nw, hop) == M == R.n_cells(K.S, Nw, hop)
    rng = ocal.range_ek(np.zeros_like(d["backscatter_r"]), d["sample_interval"], d["sound_speed"])
    n0 = np.arange(M) * hop
    assert np.array_equal(want["echo_range"], (rng[:, :, n0] + rng[:, :, n0 + Nw - 1]) / 2)


def test_the_normalised_window():
    from echopype_amd.calibrate.sv_spectrum import normalised_window

    for n in (3, 16, 255, 1024):
        for kind in ("hann", "rectangular"):
            w = normalised_window(n, kind)
            assert w.dtype == np.float64 and w.shape == (n,) and abs(np.sum(w * w) - n) <= 1e-12 * n
            assert np.allclose(w, R.window(n, kind), rtol=1e-15, atol=0)
    assert np.array_equal(normalised_window(2, "rectangular"), [1.0, 1.0])


# ---- arguments ---------------------------------------------------------------------------------------------------------
GOOD = {"window_samples": 16, "n_frequencies": 9}


@pytest.mark.parametrize("params,match", [
    ("nope", "dict"), ({**GOOD, "half_window": 3}, "Unknown"), ({"window_samples": 4}, "Missing"),
    ({"n_frequencies": 4}, "Missing"), ({**GOOD, "window_samples": 1}, "window_samples"),
    ({**GOOD, "window_samples": 1025}, "window_samples"), ({**GOOD, "window_samples": 2.5}, "window_samples"),
    ({**GOOD, "window_samples": "4"}, "window_samples"), ({**GOOD, "window_samples": True}, "window_samples"),
    ({**GOOD, "n_frequencies": 0}, "n_frequencies"), ({**GOOD, "n_frequencies": 1025}, "n_frequencies"),
    ({**GOOD, "n_frequencies": None}, "n_frequencies"), ({**GOOD, "n_frequencies": float("nan")}, "n_frequencies"),
    ({**GOOD, "step_samples": 0}, "step_samples"), ({**GOOD, "step_samples": 1.5}, "step_samples"),
    ({**GOOD, "step_samples": None}, "step_samples"), ({**GOOD, "window": "hamming"}, "window"),
    ({**GOOD, "window": 3}, "window"), ({**GOOD, "window_samples": 2}, "hann"),
    ({**GOOD, "band_margin": 0.5}, "band_margin"), ({**GOOD, "band_margin": "a"}, "band_margin"),
    ({**GOOD, "frequency_limits": (1.0,)}, "frequency_limits"), ({**GOOD, "frequency_limits": (60e3, 50e3)}, "frequency_limits"),
    ({**GOOD, "frequency_limits": [(50e3, 60e3)] * 3}, "frequency_limits"),
    ({**GOOD, "window_samples": 401}, "401"),
])
def test_parameter_errors_come_before_any_device_work(params, match, monkeypatch):
    import echopype_amd as ep
    from echopype_amd import ops

    ed, d, _, _ = _echodata()
    monkeypatch.setattr(ops, "to_device", lambda *a, **k: pytest.fail("device work"))
    monkeypatch.setattr(ops, "to_device_small", lambda *a, **k: pytest.fail("device work"))
    with pytest.raises(ValueError, match=match):
        ep.calibrate.compute_Sv_spectrum(ed, params)


def test_file_errors_come_before_any_device_work(monkeypatch):
    import echopype_amd as ep
    from echopype_amd import echodata, ops, synth

    monkeypatch.setattr(ops, "to_device", lambda *a, **k: pytest.fail("device work"))
    monkeypatch.setattr(ops, "to_device_small", lambda *a, **k: pytest.fail("device work"))
    ed, d, _, _ = _echodata()
    with pytest.raises(ValueError, match="dtype"):
        ep.calibrate.compute_Sv_spectrum(ed, GOOD, dtype="int32")
    cw = synth.ek80_numpy(C=2, P=3, S=64, waveform="CW")
    with pytest.raises(TypeError, match="BB"):
        ep.calibrate.compute_Sv_spectrum(echodata.from_ek80_arrays(cw, synth.ek80_filters()), GOOD)
    e60 = synth.ek60_numpy(C=2, P=3, S=64)
    with pytest.raises(TypeError, match="EK60"):
        ep.calibrate.compute_Sv_spectrum(echodata.from_ek60_arrays(e60), GOOD)
    # a sample interval that changes over the pings a replica covers: there is no target table to narrow them down
    beam = ed[echodata.BEAM1]
    si = np.array(beam["sample_interval"].values)
    si[0, 2] *= 2
    beam["sample_interval"] = (("channel", "ping_time"), si)
    with pytest.raises(ValueError, match="sample_interval"):
        ep.calibrate.compute_Sv_spectrum(ed, GOOD)
    assert "compute_Sv_spectrum" in ep.calibrate.__all__


def test_library_checks_its_arguments_without_a_gpu():
    from echopype_amd import _lib, ops

    def call(**kw):
        a = dict(C=2, P=3, S=400, B=4, R=2, rep_len=10, max_taps=100, F=5, Nw=16, hop=8, M=49)
        a.update(kw)
        _lib.call("epa_sv_spectrum", None, None, _lib.F64, a["C"], a["P"], a["S"], a["B"], None, None, None, a["R"],
                  a["rep_len"], a["max_taps"], None, None, a["F"], None, None, a["Nw"], a["hop"], a["M"], None, None,
                  _lib.F64, None, None)

    for kw, match in ((dict(max_taps=2049), "2048 taps"), (dict(Nw=1025), "window_samples"), (dict(Nw=1), "window_samples"),
                      (dict(hop=0), "step_samples"), (dict(F=1025), "frequencies"), (dict(B=9), "sectors"),
                      (dict(S=0), "bad shape"), (dict(S=15), "window of 16"), (dict(M=48), "M=48"), (dict(R=1), "replica_id"),
                      (dict(), "NULL")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    assert ops.scratch_bytes("sv_spectrum.table", 3, 41) == 3 * _lib.SV_SPECTRUM_TABLE_ROWS * 41 * 8
    # the tile: at most SV_SPECTRUM_MAX_TILE_CELLS cells, evenly filled; the largest window with the largest replica fits
    assert ops.sv_spectrum_plan(177, 2, 1, 399)[:2] == (100, 4)
    t, n, lds = ops.sv_spectrum_plan(_lib.SV_SPECTRUM_MAX_TAPS, _lib.SV_SPECTRUM_MAX_WINDOW, 512, 3)
    assert (t, n) == (1, 3) and lds <= 160 * 1024
    t, n, lds = ops.sv_spectrum_plan(177, 256, 128, 18)
    assert t * n >= 18 and t <= _lib.SV_SPECTRUM_MAX_TILE_CELLS and lds <= 160 * 1024 // 3


# ---- conditioning of the GPU fixtures ----------------------------------------------------------------------------------
LIMIT = 1e-10


@pytest.mark.parametrize("case", K.SWEEP + (K.UNCOVERED_CASE + (True,),), ids=str)
def test_conditioning_of_the_fixtures(case):
    """kappa = sum |terms| / |sum| of the Fourier sums the kernel test compares: kappa (N_w + L) 2**-52 <= 1e-10 for Y at
    EVERY finite (cell, frequency) of every case of the sweep and for A at every (replica, frequency) -- a CONDITION on
    the fixtures, not a measurement of the kernel; the 1e-9 of the kernel test rests on it.  Met with the band margin of
    the fixtures widened from 0.1 to 0.25 (sv_spectrum_cases.MARGIN says why) and with the sweep as
    sv_spectrum_cases.SWEEP states it (hop = 1 at N_w = 2 only, and why)."""
    B, dtype, Nw, hop, F, kind, two = case[:7]
    w = K.reference(B, dtype, Nw, hop, F, kind, two, uncovered=len(case) > 7)
    fin = np.isfinite(w["Sv_spectrum"])
    assert fin.any() and np.array_equal(fin, np.isfinite(w["kappa_Y"]))
    n = Nw + 177
    worst_y, worst_a = float(w["kappa_Y"][fin].max()), float(np.nanmax(w["kappa_A"]))
    print("kappa_Y max", worst_y, "kappa_A max", worst_a, "bounds", worst_y * n * 2.0 ** -52, worst_a * n * 2.0 ** -52)
    assert worst_y * n * 2.0 ** -52 <= LIMIT and worst_a * n * 2.0 ** -52 <= LIMIT


@pytest.mark.parametrize("S,J", K.LONG)
def test_conditioning_of_the_long_pings(S, J):
    """The same bound on the longer pings, and that they reach the paths they are there for: one tile whose span makes a
    lane compress J samples side by side."""
    from echopype_amd import ops

    Nw, hop, F, kind = K.LONG_CASE
    w = K.long_reference(S)
    M = w["Sv_spectrum"].shape[2]
    cells, tiles, _ = ops.sv_spectrum_plan(177, Nw, K.hop_of(Nw, hop), M)
    assert tiles == 1 and cells == M and -(-((M - 1) * K.hop_of(Nw, hop) + Nw) // 256) == J
    fin = np.isfinite(w["Sv_spectrum"])
    assert fin.all()
    worst_y, worst_a = float(w["kappa_Y"].max()), float(np.nanmax(w["kappa_A"]))
    print("kappa_Y max", worst_y, "kappa_A max", worst_a)
    assert worst_y * (Nw + 177) * 2.0 ** -52 <= LIMIT and worst_a * (Nw + 177) * 2.0 ** -52 <= LIMIT
