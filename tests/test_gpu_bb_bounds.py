"""The EK80 broadband float32 routes against a float64 / longdouble NumPy correlation of exactly the float32 samples and
the complex64 replica the kernels read, with the bounds tests/f32_bounds.py derives from csrc/lds_fft.h, ek80_fft.hip and
ek80_complex.hip: the transform on its own (``epa_selftest_correlate``: norm and phase of its complex output), Sv / TS
of either form judged on its own -- every sample in linear amplitude, the dB value wherever its bound is finite -- and
the exact footprint of the FFT form's zero restoration.  No tolerance here is fitted; tests/bb_ref.py holds the oracle,
the inputs and the per-form amplitude bounds (shared with the CPU tests of the judge, tests/test_f32_bounds.py)."""
import numpy as np
import pytest

import bb_ref
import f32_bounds as fb

pytestmark = pytest.mark.gpu

PATH_SHAPES = [(177, 5000, False, 4), (64, 2048, True, 4), (16, 1873, False, 4), (1024, 3000, True, 4),
               (333, 8192, False, 4), (90, 2500, True, 3), (40, 1000, False, 1), (177, 2100, True, 4),
               (100, 1949, False, 4), (31, 300, True, 2)]   # those of test_sv_complex_fft_path_matches_direct


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m 'not gpu' on CPU boxes)")
    from echopype_amd import ops

    return torch, ops


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the transform on its own ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["complex64", "complex128"])
def test_transform_selftest_within_the_derived_norm_bound(env, precision):
    """``correlate<F>`` itself: per tile || got - exp ||_2 and max |got - exp| <= ``fft_tile_bound`` (complex128: the
    same derivation with u = 2^-53 against the longdouble sum).  Impulses at every register and wavefront edge, tones
    that single out every twiddle power of every pass, purely real / imaginary data and replicas, one-tap replicas (the
    output is the input times a constant: the phase is compared, not a magnitude), replicas of 1 .. 1024 taps with
    exact-zero ends, white and 140 dB tiles."""
    from echopype_amd import _lib

    torch, ops = env
    u = fb.U if precision == "complex64" else fb.U64
    with _lib.launch_trace() as tr:
        for name, tiles, h in bb_ref.transform_cases():
            x, exp, bound = bb_ref.transform_expected(tiles, h, u)
            got = ops.selftest_correlate(_dev(torch, x), _dev(torch, h)).cpu().numpy()
            assert got.dtype == x.dtype and got.shape == x.shape
            fb.assert_norm_close(got, exp, bound, f"correlate<{precision}> {name}")
    assert "selftest_correlate_kernel" in tr.kernels and "replica_prepare_kernel" in tr.kernels


def test_transform_selftest_refuses_what_it_cannot_take(env):
    torch, ops = env
    x = torch.zeros((1, 2048), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="tiles expected"):
        ops.selftest_correlate(x[:, :1024].contiguous(), x[0, :4].contiguous())
    with pytest.raises(ValueError, match="taps expected"):
        ops.selftest_correlate(x, torch.zeros(2049, dtype=torch.complex64, device="cuda"))


# ---- Sv / TS through ops.sv_complex --------------------------------------------------------------------------------
def _run_both(env, case, planes):
    """``ops.sv_complex`` direct and fft (complex64 transform), float32 output, on the case's float32 VALUES held in
    ``planes`` -> {form: (out, prx)}."""
    from echopype_amd import _lib

    torch, ops = env
    re, im, rep, lens, cc = case["inputs"]
    re, im = re.astype(np.float32).astype(planes), im.astype(np.float32).astype(planes)
    repf = _dev(torch, np.stack([rep.real, rep.imag], axis=1).astype(np.float32).reshape(-1))
    off = _dev(torch, np.cumsum([0] + list(lens)).astype(np.int32))
    kw = dict(replica=repf, replica_off=off, max_taps=lens[0], dtype=torch.float32, want_prx=True)
    args = (_dev(torch, re), _dev(torch, im), _dev(torch, cc))
    res = {}
    for form in ("direct", "fft"):
        with _lib.launch_trace() as tr:
            r = ops.sv_complex(*args, method=form, fft_dtype="float32" if form == "fft" else None, **kw)
        assert any("fft" in k for k in tr.kernels) == (form == "fft"), tr.kernels
        res[form] = (r["out"].cpu().numpy(), r["prx"].cpu().numpy())
    return res


@pytest.mark.parametrize("planes", ["float32", "float64"])
@pytest.mark.parametrize("taps,S,mixed,B", PATH_SHAPES)
def test_sv_complex_each_form_against_the_oracle(env, planes, taps, S, mixed, B):
    """Echoes over 140 dB (several tiles, ragged ends, two replica lengths, per-ping coefficients, partly-NaN sectors, a
    missing beam 0): the direct form against its per-sample bound, the FFT form against its tile bound, each on its
    own, every sample with a valid sector in linear amplitude and the dB value wherever ``bb_sample_bound`` is
    finite."""
    case = bb_ref.sv_case("path", taps, S, mixed, B)
    res = _run_both(env, case, planes)
    for form in ("direct", "fft"):
        r = bb_ref.judge_sv(*res[form], case, form, f"BB {form} {planes} planes taps={taps} S={S} B={B}")
        assert r["judged_db"] > 0.5, "most samples must be judged in dB"


@pytest.mark.parametrize("planes", ["float32", "float64"])
def test_sv_complex_flat_input_every_db_value_is_judged(env, planes):
    """Every finite sample within 40 dB of its tile's peak: the oracle alone gives every one of them a finite dB bound
    (asserted before the GPU is consulted), and all of them are compared."""
    case = bb_ref.sv_case("flat")
    o = case["o"]
    fin = np.isfinite(o["exp"])
    assert fin.mean() > 0.9
    for form in ("direct", "fft"):
        assert np.isfinite(case[form][1][fin]).all(), f"{form}: a finite sample without a finite dB bound"
    res = _run_both(env, case, planes)
    for form in ("direct", "fft"):
        r = bb_ref.judge_sv(*res[form], case, form, f"BB flat {form} {planes} planes")
        assert r["judged_db"] == 1.0


# ---- zero restoration: the exact footprint ------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [177, 1024, 16])
def test_zero_restoration_has_the_exact_footprint(env, taps):
    """Exact-zero runs inside strong data, their ends on / next to multiples of 64, 256 and the tile seams, single
    non-zero samples inside them, a replica with exact-zero first and last taps, a partly-NaN sector (the per-sector
    route).  Expected: the boolean correlation of the non-zero masks.  The direct form has that NaN pattern exactly;
    the FFT form is NaN wherever the window holds no product and a number wherever the oracle's amplitude exceeds the
    amplitude bound of its tile -- which (a condition on the input, checked on the oracle) is all but 1 % of the
    footprint at most."""
    case = bb_ref.sv_case("zeros", taps)
    has, sure = bb_ref.footprint(case)
    assert (~has & (case["o"]["nvalid"] > 0)).sum() > 1000 and sure.sum() >= 0.99 * has.sum()
    res = _run_both(env, case, "float32")
    for form in ("direct", "fft"):
        bb_ref.check_footprint(case, res[form][1], form)
        bb_ref.judge_sv(*res[form], case, form, f"BB zero runs {form} taps={taps}")
