"""ctypes binding of libechopype_amd.so (the C ABI declared in include/echopype_amd.h).

The HIP library is the product: if it is missing, or fails to load, importing this module
raises -- there is NO CPU fallback anywhere in echopype_amd.

torch is imported first on purpose: PyTorch-ROCm bundles its own libamdhip64.so.7; loading it
before our library makes the dynamic linker resolve our DT_NEEDED libamdhip64.so.7 to the copy
already in the process, so torch tensors (device memory, streams, RCCL) and our kernels share one
HIP runtime.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# ECHOPYPE_AMD_LIB: alternative build of the same library (A/B tuning of kernel variants)
LIB_PATH = os.environ.get("ECHOPYPE_AMD_LIB") or os.path.join(_HERE, "lib", "libechopype_amd.so")

EPA_OK, EPA_EINVAL, EPA_EHIP, EPA_ENOMEM, EPA_EUNSUPPORTED = range(5)
F32, F64 = 0, 1
I8 = 2  # EPA_I8: int8 electrical-angle steps (epa_splitbeam_power only)
CAL_SV, CAL_TS = 0, 1
SONAR_EK60, SONAR_EK80 = 0, 1
PM_SCALAR, PM_CHANNEL, PM_CHANNEL_PING, PM_PULSE_TABLE = range(4)
NCOEF = 8
CF_RA, CF_RB, CF_R0, CF_SHIFT, CF_ALPHA2, CF_A0, CF_G, CF_D = range(8)
NCCOEF = 8
CC_RA, CC_RB, CC_SHIFT, CC_ALPHA2, CC_A, CC_PSCALE = range(6)
FLAG_GUARD_POS, FLAG_MASK_RANGE = 1, 2
BIN_SKIPNA, BIN_CLOSED_RIGHT, BIN_RANGE_AS_STORED = 1, 2, 4
POOL_NANMEAN, POOL_NANMEDIAN = 0, 1
CMP_GT, CMP_LT, CMP_LE, CMP_GE, CMP_EQ = range(5)  # enum epa_cmp
ALIGN_LINEAR, ALIGN_NEAREST = 0, 1  # epa_align_to_ping_time mode
LINE_CLOSED_RIGHT, LINE_NAN_IGNORE = 1, 2  # EPA_LINE_*: the flags of epa_line_mask
REGRID_TILE = 2048  # EPA_REGRID_TILE: source samples of a row that epa_regrid_rows keeps in LDS at a time
WINDOW_MEDIAN, WINDOW_MEAN, WINDOW_MIN, WINDOW_MAX = range(4)  # enum epa_window_method
WINDOW_METHODS = ("median", "mean", "min", "max")  # ... by name, in its order
WINDOW_FILTER_MAX = 15  # EPA_WINDOW_FILTER_MAX: the largest window size along either axis
WINDOW_FILTER_TP, WINDOW_FILTER_TS = 16, 64  # EPA_WINDOW_FILTER_TP, _TS: the pings x samples of a workgroup's tile
QC_FACTS = 4  # EPA_QC_FACTS
QC_FIRST, QC_COUNT, QC_NAT, QC_SLOTS = range(4)  # the words of the facts
QC_MAX_WIN = 1024  # EPA_QC_MAX_WIN
QC_MEDIAN_WAVES = 1024  # EPA_QC_MEDIAN_WAVES
QC_SCAN_TILE = 1024  # EPA_QC_SCAN_TILE
CT_I8, CT_I16, CT_I32, CT_I64, CT_F32, CT_F64 = range(6)  # enum epa_concat_type
CONCAT_SEG_WORDS = 5  # int64 words of an epa_concat_seg: base, P, W, first, C
RAW_ANGLE_NONE, RAW_ANGLE_I8, RAW_ANGLE_F32 = range(3)  # enum epa_raw_angle
RAW_ZERO_TIME = 1  # EPA_RAW_ZERO_TIME
NMEA_INVALID, NMEA_LAT_FAILED, NMEA_LON_FAILED, NMEA_UNDECIDED = 1, 2, 4, 64  # EPA_NMEA_*: the status byte
NMEA_TYPE_SHIFT, NMEA_TYPE_MASK = 3, 0x18  # ... and where it carries enum epa_nmea_type (GGA, GLL, RMC)
RAW_RECORD_BYTES = 32  # sizeof(epa_raw_record): offset i8, size i4, type u4, low_date u4, high_date u4, flags u4, reserved u4
CCP = ("sample_interval", "tau_nominal", "transmit_power", "sound_speed", "absorption", "gain", "freq_center", "psi",
       "sa_correction", "z_er", "z_et", "angle_offset_alongship", "angle_offset_athwartship", "beamwidth_alongship",
       "beamwidth_athwartship")  # enum epa_ccoef_param
EK80_NFFT = 2048
SEAFLOOR_STATE_WORDS = 16  # EPA_SEAFLOOR_STATE_WORDS
SHOAL_STATE_WORDS = 8  # EPA_SHOAL_STATE_WORDS
SHOAL_QUEUE_BOXES = 4096  # EPA_SHOAL_QUEUE_BOXES
SHOAL_STATE_ERROR, SHOAL_STATE_COUNT = 0, 1  # EPA_SHOAL_STATE_ERROR, EPA_SHOAL_STATE_COUNT
REGION_FIELDS = ("n_valid", "n_range", "sv_max", "range_min", "range_max", "sum_sv", "sum_range", "sum_sv_range",
                 "sum_sv_at_range", "sum_dz", "sum_sv_dz")  # enum epa_region_word, in its order
REGION_WORDS = 11  # EPA_REGION_WORDS
REGION_ID_SAMPLES, REGION_ID_FIRST, REGION_ID_WORDS = 0, 1, 2  # EPA_REGION_ID_*
SINGLE_TARGET_TILE = 1024  # EPA_SINGLE_TARGET_TILE
SINGLE_TARGET_ICOL_NAMES = ("channel_index", "ping_index", "range_sample", "sample_first", "sample_last")  # the rows of icols
SINGLE_TARGET_FCOL_NAMES = ("TS_uncomp", "TS_comp", "beam_compensation", "target_range", "angle_alongship", "angle_athwartship",
                            "std_angle_alongship", "std_angle_athwartship", "normalized_pulse_length")  # the rows of fcols
SINGLE_TARGET_ICOLS, SINGLE_TARGET_FCOLS, SINGLE_TARGET_PARAMS = 5, 9, 5  # EPA_SINGLE_TARGET_ICOLS, _FCOLS, _PARAMS
SINGLE_TARGET_LIMITS = ("TS_threshold", "pldl", "min_norm_pulse_length", "max_norm_pulse_length", "max_beam_compensation",
                        "max_std_alongship", "max_std_athwartship")  # the order of `limits`
TRACK_TILE = 128  # EPA_TRACK_TILE
TRACK_PARAMS, TRACK_ICOLS, TRACK_FCOLS = 11, 6, 13  # EPA_TRACK_PARAMS, _ICOLS, _FCOLS
TRACK_PARAM_NAMES = ("gate_alongship", "gate_athwartship", "gate_range", "max_ping_gap", "missed_ping_expansion",
                "weight_alongship", "weight_athwartship", "weight_range", "weight_TS", "weight_ping_gap",
                "max_TS_difference")  # the order of `params` (EPA_TRACK_PARAMS of them; max_TS_difference 0: no TS gate)
TRACK_ICOL_NAMES = ("channel_index", "n_targets", "ping_first", "ping_last", "target_first",
                    "target_last")  # the rows of a track's icols
TRACK_FCOL_NAMES = ("TS_mean", "TS_max", "range_mean", "x_first", "y_first", "z_first", "x_last", "y_last", "z_last",
                    "path_length", "displacement", "tortuosity", "delta_range")  # the rows of a track's fcols
TARGET_SPECTRA_MAX_HALF_WINDOW, TARGET_SPECTRA_MAX_FREQ, TARGET_SPECTRA_MAX_TAPS = 127, 1024, 2048  # EPA_TARGET_SPECTRA_MAX_*
TARGET_SPECTRA_FPARAMS, TARGET_SPECTRA_PPARAMS, TARGET_SPECTRA_TABLE_ROWS = 8, 3, 3  # EPA_TARGET_SPECTRA_FPARAMS, _PPARAMS, _TABLE_ROWS
TARGET_SPECTRA_FPARAM_NAMES = ("frequency", "sound_absorption", "gain_correction", "impedance_transducer", "beamwidth_alongship",
                               "beamwidth_athwartship", "angle_offset_alongship", "angle_offset_athwartship")  # the rows of fparams
TARGET_SPECTRA_PPARAM_NAMES = ("transmit_power", "sound_speed", "impedance_transceiver")  # the rows of pparams
SV_SPECTRUM_MAX_WINDOW, SV_SPECTRUM_MAX_FREQ, SV_SPECTRUM_MAX_TAPS = 1024, 1024, 2048  # EPA_SV_SPECTRUM_MAX_*
SV_SPECTRUM_MAX_TILE_CELLS = 128  # EPA_SV_SPECTRUM_MAX_TILE_CELLS
SV_SPECTRUM_FPARAMS, SV_SPECTRUM_PPARAMS, SV_SPECTRUM_TABLE_ROWS = 5, 4, 3  # EPA_SV_SPECTRUM_FPARAMS, _PPARAMS, _TABLE_ROWS
SV_SPECTRUM_FPARAM_NAMES = ("frequency", "sound_absorption", "gain_correction", "impedance_transducer",
                            "equivalent_beam_angle")  # the rows of its fparams
SV_SPECTRUM_PPARAM_NAMES = ("transmit_power", "sound_speed", "impedance_transceiver", "sample_interval")  # ... of its pparams


class EpaError(RuntimeError):
    """A C-ABI call returned a non-zero status."""


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python echopype_amd/build.py` "
            "(hipcc --offload-arch=gfx950).  echopype_amd has no CPU fallback."
        )
    return ctypes.CDLL(LIB_PATH)


lib = _load()

_vp, _i, _u, _d, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_double, ctypes.c_size_t
_i64 = ctypes.c_int64
_ll = ctypes.c_longlong

# name -> argtypes; every function returns int status except epa_version / epa_last_error
SIGNATURES = {
    "epa_version": [],
    "epa_source_digest": [],
    "epa_last_error": [],
    "epa_launch_trace": [_i],
    "epa_last_range_stats_filled": [],
    "epa_launch_seen": [],
    "epa_device_count": [ctypes.POINTER(_i)],
    "epa_set_device": [_i],
    "epa_device_name": [_i, ctypes.c_char_p, _sz],
    "epa_malloc": [ctypes.POINTER(_vp), _sz],
    "epa_free": [_vp],
    "epa_memset": [_vp, _i, _sz, _vp],
    "epa_memcpy_h2d": [_vp, _vp, _sz, _vp],
    "epa_memcpy_d2h": [_vp, _vp, _sz, _vp],
    "epa_stream_synchronize": [_vp],
    "epa_timer_create": [ctypes.POINTER(_vp)],
    "epa_timer_destroy": [_vp],
    "epa_timer_start": [_vp, _vp],
    "epa_timer_stop": [_vp, _vp],
    "epa_timer_elapsed_ms": [_vp, ctypes.POINTER(ctypes.c_float)],
    "epa_scratch_bytes": [ctypes.c_char_p, _ll, _ll, _ll, ctypes.POINTER(_sz)],
    "epa_mvbs_needs_partials": [_i, _i, _i, _i, ctypes.POINTER(_i)],
    "epa_regrid_needs_global_flags": [_i, ctypes.POINTER(_i)],
    "epa_sv_power_vectorized": [_vp, _i, _i, ctypes.POINTER(_i)],
    "epa_power_coef_ek": [_i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp,
                          _vp, _i, _vp, _i, _i, _vp, _vp],
    "epa_pulse_table_lookup": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    "epa_sv_power": [_vp, _vp, _i, _i, _i, _i, _u, _vp, _vp, _i, _vp],
    "epa_sv_power_stats": [_vp, _vp, _i, _i, _i, _i, _u, _vp, _vp, _i, _vp, _vp, _vp],
    "epa_range_power": [_vp, _vp, _i, _i, _i, _u, _vp, _i, _vp],
    "epa_range_complex": [_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp],
    "epa_sv_complex_cw_stats": [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp],
    "epa_time_bin_offsets": [_vp, _i, _i64, _i64, _i, _u, _vp, _vp],
    "epa_sv_mvbs_fused": [_vp, _vp, _i, _i, _i, _i, _u, _vp, _vp, _i, _d, _i, _u, _d, _vp, _vp, _vp,
                          _vp, _vp, _vp, _vp, _i, _vp],
    "epa_sv_mvbs_fused_i16": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _d, _i, _d, _vp, _vp, _vp, _vp, _vp, _i, _vp],
    "epa_sv_mvbs_fused_depth": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _d, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _i,
                                _vp],
    "epa_mvbs": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _d, _i, _u, _d, _vp, _vp, _vp, _i, _vp],
    "epa_selftest_lin_from_db": [_vp, _vp, _sz, _vp],
    "epa_selftest_log10": [_vp, _vp, _sz, _vp],
    "epa_selftest_log10_inline": [_vp, _vp, _sz, _vp],
    "epa_selftest_correlate": [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp],
    "epa_mvbs_finalize": [_vp, _vp, _sz, _d, _vp, _i, _vp],
    "epa_edge_pack": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp],
    "epa_edge_prepare_max": [_vp, _i, _vp],
    "epa_edge_gather": [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp],
    "epa_edge_finalize_mvbs": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _d, _i, _vp],
    "epa_affine_rows": [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp],
    "epa_depth_rows": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp],
    "epa_nanminmax": [_vp, _sz, _i, _vp, _vp, _vp],
    "epa_mvbs_index": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp],
    "epa_noise_estimate": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp, _i, _vp],
    "epa_noise_finalize": [_vp, _vp, _i, _i, _d, _vp, _vp],
    "epa_noise_apply": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp, _i, _vp],
    "epa_noise_apply_rows": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp, _i, _vp],
    "epa_complex_coef_ek80": [_i, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp],
    "epa_sv_complex": [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp],
    "epa_sv_complex_indexed": [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp],
    "epa_sv_complex_fft": [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp],
    "epa_sv_complex_fft_indexed": [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i,
                                   _vp, _vp, _vp],
    "epa_range_bin_smooth": [_vp, _vp, _i, _i, _i, _i, _d, _d, _i, _vp, _i, _vp],
    "epa_impulse_mask": [_vp, _i, _i, _i, _i, _d, _vp, _i, _vp],
    "epa_pool_sv": [_vp, _i, _i, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _i, _vp],
    "epa_attenuated_mask": [_vp, _vp, _i, _i, _i, _d, _d, _i, _d, _vp, _i, _vp],
    "epa_apply_mask": [_vp, _vp, _sz, _sz, _d, _vp, _sz, _vp, _i, _vp],
    "epa_apply_masks": [_vp, _vp, _vp, _i, _sz, _d, _vp, _sz, _vp, _vp, _vp, _i, _vp],
    "epa_mask_and": [_vp, _vp, _sz, _sz, _vp, _vp],
    "epa_range_step_mean": [_vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "epa_first_not_le": [_vp, _sz, _d, _i, _vp, _vp],
    "epa_range_rows_check": [_vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "epa_sv_noise_fused": [_vp, _vp, _vp, _i, _i, _i, _i, _u, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp],
    "epa_denoise_mvbs": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _vp, _vp, _i, _d, _i, _u, _d, _vp, _vp, _vp,
                         _vp, _vp, _i, _vp],
    "epa_sv_denoise_mvbs": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _u, _i, _i, _d, _vp, _vp, _i, _d, _i, _u, _d, _vp, _vp, _vp,
                            _vp, _vp, _vp, _vp, _i, _vp],
    "epa_geodesic_steps": [_vp, _vp, _i, _vp, _vp],
    "epa_nasc": [_vp, _vp, _i, _i, _i, _vp, _i, _d, _i, _u, _vp, _vp, _vp, _vp, _i, _vp],
    "epa_splitbeam_power": [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp],
    "epa_splitbeam_complex": [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp],
    "epa_splitbeam_complex_fft": [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _i,
                                  _vp, _vp],
    "epa_pool_sv_value": [_vp, _vp, _vp, _i, _i, _i, _d, _i, _d, _d, _d, _i, _d, _vp, _vp, _vp, _i, _vp],
    "epa_seafloor_depth_uniform": [_vp, _i, _i64, _i64, _vp, _vp],
    "epa_seafloor_basic": [_vp, _i, _i64, _i64, _i64, _d, _d, _vp, _d, _vp, _vp],
    "epa_seafloor_angle_mask": [_vp, _vp, _i, _i64, _i64, _i64, _i64, _i, _i, _d, _d, _vp, _vp, _vp, _vp],
    "epa_seafloor_median": [_vp, _i, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    "epa_seafloor_components": [_vp, _i, _i64, _i64, _i64, _i64, _d, _vp, _vp, _vp, _vp],
    "epa_seafloor_bottom": [_vp, _vp, _i64, _i64, _i64, _vp, _d, _vp, _i, _vp],
    "epa_shoal_threshold_fill": [_vp, _i, _i64, _i64, _d, _i64, _i64, _vp, _vp],
    "epa_shoal_label": [_vp, _i64, _i64, _i, _vp, _vp, _vp, _i64, _vp, _vp],
    "epa_shoal_weill_filter": [_vp, _i64, _i64, _vp, _vp, _i64, _d, _d, _vp, _vp, _vp],
    "epa_shoal_echoview_link": [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _d, _d, _d, _d, _d, _d, _vp,
                                _vp, _vp, _vp],
    "epa_transient_fielding": [_vp, _i, _i, _i, _i, _vp, _i, _i, _d, _d, _d, _vp, _vp, _vp, _vp],
    "epa_transient_matecho": [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _d, _d, _i, _d, _vp, _vp, _vp, _vp],
    "epa_freq_diff_mask": [_vp, _i, _sz, _i, _i, _i, _d, _vp, _i, _vp],
    "epa_regrid_mask": [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _d, _i, _u, _i, _vp, _vp, _vp],
    "epa_line_mask": [_vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _i, _vp, _ll, _ll, _d, _vp, _ll, _ll, _d, _u, _i, _i, _i, _vp,
                      _vp],
    "epa_regrid_rows": [_vp, _i, _vp, _i, _ll, _ll, _ll, _i, _i, _i, _d, _i, _vp, _vp, _vp, _i, _vp],
    "epa_window_filter": [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp],
    "epa_echo_metrics": [_vp, _vp, _i, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
    "epa_align_to_ping_time": [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp],
    "epa_time_reversals": [_vp, _ll, _vp, _vp, _vp],
    "epa_reversal_medians": [_vp, _ll, _i, _vp, _vp, _vp, _vp],
    "epa_time_rebuild": [_vp, _ll, _vp, _vp, _vp, _vp, _vp],
    "epa_concat_rows": [_vp, _vp, _vp, _vp, _i, _i, _ll, _i, _i, _vp, _vp],
    "epa_raw_index": [_vp, _ll, _vp, _ll, ctypes.POINTER(_ll), ctypes.POINTER(_ll)],
    "epa_raw0_unpack": [_vp, _ll, _ll, _vp, _vp, _i, _ll, _ll, _i, _vp, _vp, _vp, _vp],
    "epa_raw3_unpack": [_vp, _ll, _ll, _vp, _vp, _i, _ll, _ll, _i, _vp, _vp, _vp],
    "epa_nmea_positions": [_vp, _ll, _ll, _vp, _vp, _ll, _vp, _vp, _vp, _vp],
    "epa_region_stats": [_vp, _ll, _ll, _vp, _vp, _i, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp],
    "epa_region_labels": [_vp, _ll, _ll, _vp, _ll, _vp, _vp],
    "epa_single_target_count": [_vp, _vp, _vp, _vp, _i, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp],
    "epa_single_target_emit": [_vp, _vp, _vp, _vp, _i, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp],
    "epa_track_prepare": [_vp, _vp, _vp, _vp, _vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp],
    "epa_track_propose": [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp],
    "epa_track_accept": [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp],
    "epa_track_roots": [_vp, _ll, _i, _vp, _vp, _vp, _vp, _vp],
    "epa_track_chains": [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _vp, _vp],
    "epa_track_table": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp],
    "epa_target_spectra": [_vp, _vp, _i, _ll, _ll, _ll, _i, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _i, _i, _vp, _vp, _i,
                           _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp, _i, _vp, _vp],
    "epa_sv_spectrum": [_vp, _vp, _i, _ll, _ll, _ll, _i, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _i, _vp, _vp, _i, _ll, _ll,
                        _vp, _vp, _i, _vp, _vp],
    "epa_sv_spectrum_plan": [_i, _i, _ll, _ll, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_sz)],
}

for _name, _args in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = the .so does not export a declared symbol
    _fn.argtypes = _args
    _fn.restype = ctypes.c_char_p if _name in ("epa_last_error", "epa_launch_trace", "epa_launch_seen", "epa_source_digest") else _i


def _check_source_digest():
    """The library must have been built from the sources lying beside it (csrc/, include/): a stale binary raises here
    instead of answering for code it was not made from.  Skipped for an alternative build handed in through
    ECHOPYPE_AMD_LIB (A/B tuning: other flags on purpose) and when the sources are not there (an installed copy)."""
    if os.environ.get("ECHOPYPE_AMD_LIB"):
        return
    import importlib.util

    spec = importlib.util.spec_from_file_location("_epa_build", os.path.join(_HERE, "build.py"))
    if spec is None or not os.path.isdir(os.path.join(_HERE, "csrc")):
        return
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    want, got = b.source_digest(), lib.epa_source_digest().decode()
    if want != got:
        raise ImportError(f"{LIB_PATH} was built from other sources (digest {got}, the tree has {want}): "
                          "rebuild it with `python echopype_amd/build.py` (`--force` recompiles every translation unit)")


_check_source_digest()


class launch_trace:
    """``with launch_trace() as t: ...; t.kernels`` -- the names of the kernels the calls inside launched (tests)."""

    def __enter__(self):
        lib.epa_launch_trace(1)
        self.kernels = []
        return self

    def __exit__(self, *exc):
        self.kernels = [k for k in lib.epa_launch_trace(2).decode().split(";") if k]
        lib.epa_launch_trace(0)
        return False


def launched_kernels():
    """Names of every kernel this process has launched through the library so far."""
    return [k for k in lib.epa_launch_seen().decode().split(";") if k]


def last_error() -> str:
    msg = lib.epa_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(status: int, what: str = "") -> None:
    """Map a non-zero C status to a Python exception (SURVEY 8b error conventions)."""
    if status == EPA_OK:
        return
    msg = f"{what}: {last_error()}" if what else last_error()
    if status == EPA_EINVAL:
        raise ValueError(msg)
    if status == EPA_ENOMEM:
        raise MemoryError(msg)
    raise EpaError(f"[status {status}] {msg}")


def call(name: str, *args) -> None:
    check(getattr(lib, name)(*args), name)
