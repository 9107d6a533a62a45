"""calibrate.compute_Sv_spectrum on the GPU (csrc/sv_spectrum.hip through ops.sv_spectrum and calibrate/sv_spectrum.py)
against the NumPy restatement tests/sv_spectrum_ref.py, on the fixtures of tests/sv_spectrum_cases.py: C = 2 (replicas of
177 and 113 taps), P = 3, S = 400, four and three sectors, float32 and float64 cubes.

What is compared how
- EQUAL: the NaN pattern of the spectra, and ``echo_range`` to the bit.
- 10^(Sv/10) within 1e-9 relative of the oracle, the project's float64 bar.  tests/test_sv_spectrum_host.py holds the
  conditioning of every compared Fourier sum at kappa (N_w + L) 2**-52 <= 1e-10: a sum of n <= N_w + L terms is off by
  about n 2**-53 kappa relative however it is ordered (the kernel adds the sectors first, runs the taps in order per
  sample and evaluates the Fourier sum by Horner's rule on a step from sincospi; the oracle does none of these), the
  phase k f dt of the last term is off by about N_w 2**-52 kappa in the same units, and the chain after the sums is a
  dozen float64 operations.
- float32 output: bit-equal to the float32 rounding of the same call's float64 output."""
import numpy as np
import pytest
import sv_spectrum_cases as K
import sv_spectrum_ref as R

pytestmark = pytest.mark.gpu

REL = 1e-9


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m 'not gpu' on CPU boxes)")
    from echopype_amd import ops

    return torch, ops


def _dev(torch, a):
    return torch.as_tensor(np.array(a)).cuda()  # (a copy: the fixtures are read-only)


def _args(env, B, dtype, Nw, hop, F, kind="hann", two=False, uncovered=False):
    torch, ops = env
    d, replicas, _ = K.scene(B, dtype)
    fparams, pparams, rep_dt, reps, rid = K.params(d, F, replicas, two, uncovered)
    flat = np.concatenate(reps).astype(np.complex64)
    off = np.concatenate([[0], np.cumsum([r.size for r in reps])]).astype(np.int32)
    args = [_dev(torch, d["backscatter_r"]), _dev(torch, d["backscatter_i"]), _dev(torch, flat.view(np.float32)),
            _dev(torch, off), max(r.size for r in reps), _dev(torch, rep_dt), _dev(torch, fparams), _dev(torch, pparams),
            _dev(torch, R.window(Nw, kind)), K.hop_of(Nw, hop)]
    return args, dict(replica_id=None if rid is None else _dev(torch, rid))


def _run(env, *case, out_dtype="float64", **kw):
    args, kwargs = _args(env, *case, **kw)
    return env[1].sv_spectrum(*args, dtype=out_dtype, **kwargs)


def _compare(got, want):
    sv, rng = (t.cpu().numpy() for t in got)
    ref = want["Sv_spectrum"]
    assert sv.dtype == np.float64 and sv.shape == ref.shape and rng.dtype == np.float64
    assert np.array_equal(rng, want["echo_range"])  # to the bit, NaN cells included
    assert np.array_equal(np.isnan(sv), np.isnan(ref))
    f = ~np.isnan(ref)
    worst = float(np.max(np.abs(10.0 ** ((sv[f] - ref[f]) / 10.0) - 1.0))) if f.any() else 0.0
    print("largest relative error of 10^(Sv/10):", worst, "over", int(f.sum()), "values")
    assert worst <= REL
    return sv


@pytest.mark.parametrize("case", K.SWEEP, ids=str)
def test_kernel_equals_the_restatement(env, case):
    """The sweep of sv_spectrum_cases.SWEEP: every N_w, hop, F, window, sector count and cube type the issue lists."""
    B, dtype, Nw, hop, F, kind, two = case
    want = K.reference(*case)
    M = R.n_cells(K.S, Nw, K.hop_of(Nw, hop))
    assert want["Sv_spectrum"].shape == (K.C, K.P, M, F) and np.isfinite(want["Sv_spectrum"]).all(axis=-1).sum() >= 4
    if two:
        assert not np.array_equal(want["Sv_spectrum"], K.reference(B, dtype, Nw, hop, F, kind)["Sv_spectrum"], equal_nan=True)
    _compare(_run(env, *case), want)


@pytest.mark.parametrize("S,J", K.LONG)
def test_longer_pings_reach_the_wider_compression_paths(env, S, J):
    """sv_spectrum_cases.LONG: one tile per ping whose span makes a lane compress J = 3, 4, 5 samples side by side
    (S = 400 reaches J <= 2), ping 0 on the per-sector path."""
    torch, ops = env
    Nw, hop, F, kind = K.LONG_CASE
    d, replicas = K.long_scene(S)
    fparams, pparams, rep_dt, reps, rid = K.params(d, F, replicas)
    flat = np.concatenate(reps).astype(np.complex64)
    off = np.concatenate([[0], np.cumsum([r.size for r in reps])]).astype(np.int32)
    got = ops.sv_spectrum(_dev(torch, d["backscatter_r"]), _dev(torch, d["backscatter_i"]), _dev(torch, flat.view(np.float32)),
                          _dev(torch, off), reps[0].size, _dev(torch, rep_dt), _dev(torch, fparams), _dev(torch, pparams),
                          _dev(torch, R.window(Nw, kind)), K.hop_of(Nw, hop))
    _compare(got, K.long_reference(S))


def test_seams_of_tiles_tails_and_sector_patches(env):
    torch, ops = env
    # hop = 1: more than two tiles per ping, and M no multiple of the tile
    case = K.SWEEP[0]
    M = R.n_cells(K.S, case[2], case[3])
    cells, tiles, _ = ops.sv_spectrum_plan(177, case[2], case[3], M)
    assert case[3] == 1 and tiles > 2 and M % cells != 0 and (tiles - 1) * cells < M <= tiles * cells
    sv = _compare(_run(env, *case), K.reference(*case))
    # ... the cell that ends on the last valid sample in front of the NaN tail is finite, the next one is NaN
    last = K.S - K.TAIL - case[2]
    assert np.isfinite(sv[:, 1, last]).all() and np.isnan(sv[:, 1, last + 1:]).all()
    # N_w = hop = 40: the same seam with a window that reaches over the tail with its taps
    sv = _compare(_run(env, *K.SEAM), K.reference(*K.SEAM))
    assert np.isfinite(sv[:, 1, 8]).all() and np.isnan(sv[:, 1, 9]).all() and np.isfinite(sv[:, 0, 9]).all()
    # the cells over the mixed-sector patch (sector 1 NaN at samples S/2 + 3 .. S/2 + 7 of (0, 0)): the per-sector path
    case = (4, "float32", 64, None, 257, "hann", False)
    assert case in K.SWEEP
    sv = _compare(_run(env, *case), K.reference(*case))
    over = [m for m in range(sv.shape[2]) if m * 32 <= K.S // 2 + 3 and K.S // 2 + 7 < m * 32 + 64]
    assert len(over) == 2 and np.isfinite(sv[0, 0, over]).all()
    d, _, _ = K.scene(4, "float64")
    whole = np.array(d["backscatter_r"])  # (the same patch in the float32 scene)
    assert np.isnan(whole[0, 0, K.S // 2 + 3:K.S // 2 + 8, 1]).all() and not np.isnan(whole[0, 0, K.S // 2 + 3, 0])
    # N_w = S: a single cell
    single = [c for c in K.SWEEP if c[2] == K.S][0]
    assert K.reference(*single)["Sv_spectrum"].shape[2] == 1


def test_a_ping_no_filter_interval_covers_gives_nan_cells_with_their_range(env):
    case = K.UNCOVERED_CASE
    want = K.reference(*case, uncovered=True)
    sv, rng = (t.cpu().numpy() for t in _run(env, *case, uncovered=True))
    c, p = K.UNCOVERED
    assert np.isnan(sv[c, p]).all() and np.isfinite(rng[c, p]).all() and np.isfinite(sv[c, p + 1]).any()
    _compare((env[0].as_tensor(sv), env[0].as_tensor(rng)), want)


def test_both_kernels_serve_a_call_and_arguments_are_checked_first(env):
    from echopype_amd import _lib

    torch, ops = env
    with _lib.launch_trace() as tr:
        _run(env, 4, "float64", 16, 23, 1)
    assert tr.kernels == ["sv_spectrum_replica_kernel", "sv_spectrum_kernel"]
    args, kw = _args(env, 4, "float64", 16, 23, 5)
    with _lib.launch_trace() as tr:
        long_window = torch.ones(1025, dtype=torch.float64).cuda()
        for i, bad, match in ((4, 2049, "2048 taps"), (9, 0, "step_samples"), (8, long_window, "window"),
                              (7, args[7][:3].contiguous(), "pparams"), (6, args[6][:, :4].contiguous(), "fparams")):
            broken = list(args)
            broken[i] = bad
            with pytest.raises(ValueError, match=match):
                ops.sv_spectrum(*broken, **kw)
        with pytest.raises(ValueError, match="NULL"):
            _lib.call("epa_sv_spectrum", None, None, _lib.F64, 2, 3, 400, 4, None, None, None, 2, 10, 100, None, None, 5,
                      None, None, 16, 8, 49, None, None, _lib.F64, None, None)
    assert tr.kernels == []


def test_guard_bands_stay_untouched_and_a_second_call_gives_the_same_bits(env, monkeypatch):
    """The two outputs and the scratch table between bands of 0xA5: the kernels write what they own and nothing else."""
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

    case = (4, "float32", 16, 23, 41, "rectangular", True)
    assert case in K.SWEEP
    want = K.reference(*case)
    plain = [t.cpu().numpy() for t in _run(env, *case)]
    args, kw = _args(env, *case)
    monkeypatch.setattr(ops, "_scratch_alloc", lambda nbytes, dtype, device, zero: banded(
        -(-nbytes // dtype.itemsize) * dtype.itemsize, dtype, device))
    monkeypatch.setattr(ops.torch, "empty", empty)
    got = ops.sv_spectrum(*args, **kw)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(bufs) == 3  # Sv_spectrum, echo_range, the table
    for raw, n in bufs:
        assert bool((raw[:band] == fill).all()) and bool((raw[band + n:] == fill).all())
    for a, b in zip(plain, got):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)  # the second call: identical bits
    _compare(got, want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float32_output_is_the_float64_output_rounded_once(env, dtype):
    case = (4, dtype, 64, None, 41, "hann", False)
    sv64, rng64 = _run(env, *case)
    sv32, rng32 = _run(env, *case, out_dtype="float32")
    assert sv32.dtype == env[0].float32 and rng32.dtype == env[0].float64
    assert np.array_equal(sv32.cpu().numpy(), sv64.cpu().numpy().astype(np.float32), equal_nan=True)
    assert np.array_equal(rng32.cpu().numpy(), rng64.cpu().numpy())
    assert np.isfinite(sv32.cpu().numpy()).any()


# ---- the public entry point -------------------------------------------------------------------------------------------
PRM = {"window_samples": 64, "n_frequencies": 41, "band_margin": K.MARGIN}


def _echodata(B=4, dtype="float64", **kw):
    from echopype_amd import echodata, synth

    d, replicas, _ = synth.target_spectra_scene(B=B, dtype=np.dtype(dtype))
    return echodata.from_ek80_arrays(d, d["filters"], **kw), d


def _oracle_for(ed, d, prm):
    """The oracle fed with the arrays and parameter tables the entry point works from."""
    import target_spectra_ref as TR

    from echopype_amd import _lib
    from echopype_amd.calibrate.calibrate_ek import CalibrateEK80
    from echopype_amd.calibrate.spectrum_common import frequency_params

    cal = CalibrateEK80(ed, env_params=None, cal_params=None, ecs_file=None, waveform_mode="BB", encode_mode="complex")
    F = prm["n_frequencies"]
    freq = TR.grid(d["f_start"], d["f_stop"], F, prm.get("band_margin", 0.1))
    fp = frequency_params(cal, freq, names=_lib.SV_SPECTRUM_FPARAM_NAMES)  # (5, C, F)
    assert fp.shape == (5, K.C, F)
    assert np.allclose(fp[4], d["psi"][:, None] + 20 * np.log10(d["frequency_nominal"][:, None] / freq), rtol=1e-14)
    _, tx = cal._transmit_replicas()
    reps = [np.asarray(tx[ch]).astype(np.complex64) for ch in cal.beam["channel"].values]
    ss = cal.env_params["sound_speed"]
    pparams = np.stack([np.repeat(d["transmit_power"][:, None], K.P, axis=1),
                        np.broadcast_to(np.asarray(getattr(ss, "values", ss), dtype=np.float64), (K.C, K.P)),
                        np.repeat(d["z_er"][:, None], K.P, axis=1), np.asarray(d["sample_interval"], dtype=np.float64)])
    Nw = prm["window_samples"]
    want = R.sv_spectrum(d["backscatter_r"], d["backscatter_i"], reps, None, np.full(K.C, K.DT), fp.transpose(1, 0, 2),
                         pparams, Nw, prm.get("step_samples", -(-Nw // 2)), prm.get("window", "hann"))
    return want, freq


def test_whole_chain_from_ek80_fm_samples_without_a_host_synchronisation():
    """from_ek80_arrays -> compute_Sv_spectrum equals the oracle; the call itself never waits for the device; its
    echo_range is the mean of compute_Sv's BB echo_range over the first and last sample of every cell."""
    import torch

    import echopype_amd as ep

    ed, d = _echodata()
    ep.calibrate.compute_Sv_spectrum(ed, PRM)  # (whatever is made once per process, before the calls that count)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", lambda *a, **k: pytest.fail("synchronize"))
        mp.setattr(torch.Tensor, "cpu", lambda *a, **k: pytest.fail(".cpu()"))
        mp.setattr(torch.Tensor, "item", lambda *a, **k: pytest.fail(".item()"))
        mp.setattr(torch.Tensor, "tolist", lambda *a, **k: pytest.fail(".tolist()"))
        out = ep.calibrate.compute_Sv_spectrum(ed, PRM)
        again = ep.calibrate.compute_Sv_spectrum(ed, PRM)
    want, freq = _oracle_for(ed, d, PRM)
    M = R.n_cells(K.S, 64, 32)
    assert out["Sv_spectrum"].dims == ("channel", "ping_time", "range_bin", "frequency_index")
    assert out["Sv_spectrum"].shape == (K.C, K.P, M, 41) and out["echo_range"].dims == ("channel", "ping_time", "range_bin")
    assert np.array_equal(out["frequency"].values, freq) and out.attrs["step_samples"] == 32 and out.attrs["window"] == "hann"
    _compare([out[k].data.tensor for k in ("Sv_spectrum", "echo_range")], want)
    for k in ("Sv_spectrum", "echo_range", "frequency"):
        assert np.array_equal(out[k].values, again[k].values, equal_nan=True), k
    rng = np.asarray(ep.calibrate.compute_Sv(ed, waveform_mode="BB", encode_mode="complex")["echo_range"].values)
    n0 = np.arange(M) * 32
    mean = (rng[:, :, n0] + rng[:, :, n0 + 63]) / 2
    ok = ~np.isnan(mean)  # (compute_Sv masks its echo_range where the samples are NaN; the cell centres are written)
    assert ok.sum() >= K.C * K.P * M - 4 and np.array_equal(out["echo_range"].values[ok], mean[ok])


def test_a_file_with_two_filter_intervals_equals_the_file_with_one_and_float32_rounds_once():
    import echopype_amd as ep

    ed, d = _echodata()
    ed2, _ = _echodata(filter_time_idx=[0, 2])
    prm = {"window_samples": 40, "n_frequencies": 21, "step_samples": 40, "window": "rectangular",
           "frequency_limits": [(55e3, 80e3), (110e3, 150e3)]}
    a, b = ep.calibrate.compute_Sv_spectrum(ed, prm), ep.calibrate.compute_Sv_spectrum(ed2, prm)
    assert a["frequency"].values[0, 0] == 55e3 and a["frequency"].values[1, -1] == 150e3
    for k in ("Sv_spectrum", "echo_range", "frequency"):
        assert np.array_equal(a[k].values, b[k].values, equal_nan=True), k
    assert np.isfinite(a["Sv_spectrum"].values).all(axis=-1).sum() >= 50
    c = ep.calibrate.compute_Sv_spectrum(ed, prm, dtype="float32")
    assert np.array_equal(c["Sv_spectrum"].values, a["Sv_spectrum"].values.astype(np.float32), equal_nan=True)
