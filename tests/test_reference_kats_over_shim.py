"""Stand-in + reference code == the numbers the reference's maintainers wrote down.

Every chain-level golden of this tree is reference arithmetic executed over oracle/xr_shim.py (xarray cannot be
installed here).  oracle/check_reference_kats.py runs the reference's OWN functions over that stand-in on the inputs of
the reference's OWN tests, asserts the expectations written in those test files, and stores the inputs and what the
reference returned (tests/golden/ref_kat_goldens.npz, ``--write``): 6 removed samples on the seed-1 noise data and NaN
noise points (tests/clean/test_noise.py:902-987), index-binned MVBS array_equal with the padded block mean
(tests/commongrid/test_commongrid_api.py:171-202), the four pulse-length tables incl. permuted channels
(tests/calibrate/test_cal_params.py:751-868), the 0.5 / [0.5, 2880.5] interpolations
(tests/calibrate/test_env_params.py:29-126).  Here the stored numbers are held to the same expectations, and this tree's
NumPy oracle to the stored numbers."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_kat_goldens.npz")

from oracle import calibrate as ocal  # noqa: E402
from oracle import clean as oclean  # noqa: E402
from oracle import commongrid as ogrid  # noqa: E402

VEND_CHANNELS = ["chA", "chB"]
VEND_PULSE_LENGTH = np.array([[64, 128, 256, 512], [128, 256, 512, 1024]], dtype=float)
VEND_SA = np.array([[10, 20, 30, 40], [110, 120, 130, 140]], dtype=float)
nan = np.nan
# (transmit_duration_nominal per beam channel, beam channel order, the expected sa_correction) of test_cal_params.py
VEND_CASES = [
    ([[64, 256, 128, 512], [512, 1024, 256, 128]], ["chA", "chB"], [[10, 30, 20, 40], [130, 140, 120, 110]]),
    ([[512, 1024, 256, 128], [64, 256, 128, 512]], ["chB", "chA"], [[130, 140, 120, 110], [10, 30, 20, 40]]),
    ([[64, nan, 128, 512], [512, 1024, 256, nan]], ["chA", "chB"], [[10, nan, 20, 40], [130, 140, 120, nan]]),
    ([[512, 1024, 256, nan], [64, nan, 128, 512]], ["chB", "chA"], [[130, 140, 120, nan], [10, nan, 20, 40]]),
]


def test_reference_functions_over_the_shim_meet_the_reference_tests_expectations():
    g = np.load(GOLDEN)
    # remove_background_noise (ping_num 2, range_sample_num 5, SNR 0 dB, sound_absorption 0.001)
    toy = g["noise_toy_Sv_corrected"]
    assert np.isnan(toy[0, 0, 30]) and np.isnan(toy[0, 0, 60])
    np.random.seed(1)
    seed1 = np.random.normal(loc=-100, scale=2, size=(1, 10, 100))
    assert np.array_equal(g["noise_seed1_Sv"], seed1)                  # the reference test's own input
    assert np.count_nonzero(np.isnan(g["noise_seed1_Sv_corrected"])[0, :, :50]) == 6
    for case in ("toy", "seed1"):
        sv, er = g[f"noise_{case}_Sv"], g[f"noise_{case}_echo_range"]
        _, corr = oclean.remove_background_noise(sv, er, 0.001, 2, 5, None, "0dB")
        ref = g[f"noise_{case}_Sv_corrected"]
        assert np.array_equal(np.isnan(corr), np.isnan(ref)), case
        np.testing.assert_allclose(corr, ref, rtol=1e-12, atol=1e-9, equal_nan=True)
    # compute_MVBS_index_binning (range_sample_num 7, ping_num 3): array_equal with the padded block mean
    sv, mv = g["ixbin_Sv"], g["ixbin_Sv_MVBS"]
    assert np.array_equal(sv, np.random.default_rng(0).uniform(-100, -20, (2, 120, 13)))
    assert mv.shape == (2, 40, 2)
    pad = np.full((2, 120, 14), np.nan)
    pad[:, :, :13] = 10 ** (sv / 10)
    assert np.array_equal(mv, 10 * np.log10(np.nanmean(pad.reshape(2, 40, 3, 2, 7), axis=(2, 4))))
    got, _ = ogrid.compute_MVBS_index_binning(sv, g["ixbin_echo_range"], range_sample_num=7, ping_num=3)
    np.testing.assert_allclose(got, mv, rtol=1e-12, atol=0)
    # get_vend_cal_params_power: the four pulse-length tables, channels in the beam group's order
    for i, (tdn, chans, exp) in enumerate(VEND_CASES):
        assert np.array_equal(g[f"vend_case{i}_transmit_duration_nominal"], np.array(tdn), equal_nan=True)
        ref = g[f"vend_case{i}_sa_correction"]
        np.testing.assert_array_equal(ref, np.array(exp, dtype=float))
        rows = [VEND_CHANNELS.index(c) for c in chans]
        got = ocal.vend_cal_params_power(np.array(tdn, dtype=float), VEND_PULSE_LENGTH[rows], VEND_SA[rows])
        np.testing.assert_array_equal(got, ref)
    # harmonize_env_param_time: 0.5 at 15 s into a 30-s series 0, 1, 2; [0.5, 2880.5] on the two-day series
    assert g["env_interp_one"].tolist() == [0.5] and g["env_interp_two"].tolist() == [0.5, 2880.5]
    t3 = np.arange("2017-06-20T01:00:00", "2017-06-20T01:01:30", np.timedelta64(30, "s"), dtype="datetime64[ns]")
    q = np.array(["2017-06-20T01:00:15"], dtype="datetime64[ns]")
    assert ocal.harmonize_time(np.array([0.0, 1.0, 2.0]), t3, q).tolist() == g["env_interp_one"].tolist()
    time1 = np.arange("2017-06-20T01:00:00", "2017-06-22T01:00:31", np.timedelta64(30, "s"), dtype="datetime64[ns]")
    q = np.array(["2017-06-20T01:00:15", "2017-06-21T01:00:15"], dtype="datetime64[ns]")
    assert ocal.harmonize_time(np.arange(len(time1), dtype=float), time1, q).tolist() == g["env_interp_two"].tolist()
