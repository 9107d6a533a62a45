"""echopype_amd -- MI355X (gfx950) native implementation of echopype's array-compute hot path

    calibrate.compute_Sv / compute_TS -> clean.remove_background_noise -> commongrid.compute_MVBS

behind echopype's own function signatures.  Host code is Python; the (channel, ping_time,
range_sample) arrays go through a C ABI (include/echopype_amd.h, loaded with ctypes) to hand-written
HIP kernels.  There is no CPU fallback: importing the package loads libechopype_amd.so and fails
loudly if it has not been built (``python echopype_amd/build.py``).
"""
# The HIP runtime maps a process's streams onto a fixed number of hardware queues (GPU_MAX_HW_QUEUES) when it
# initialises; streams that share a queue run one after the other.  The package leaves that number to the runtime and the
# user: ``pipeline`` keeps only side streams it has seen running side by side (``pipeline._runs_beside``).
from . import _lib  # noqa: F401,E402  (loads the HIP library; raises if missing)
from . import calibrate, clean, commongrid, consolidate, convert, mask, metrics, ops, pipeline, qc, synth, targets, utils  # noqa: F401,E402
from .combine import combine_echodata  # noqa: F401,E402
from .convert import open_raw, open_raw_ek80  # noqa: F401,E402
from .echodata import EchoData  # noqa: F401,E402
from .fused import compute_Sv_clean_MVBS, compute_Sv_MVBS  # noqa: F401,E402
from .xr_lite import DataArray, Dataset, DeviceArray  # noqa: F401,E402

__version__ = "0.1.0"
__all__ = ["calibrate", "clean", "commongrid", "consolidate", "convert", "open_raw", "open_raw_ek80", "mask", "metrics", "qc", "utils", "ops", "synth", "pipeline", "compute_Sv_MVBS", "compute_Sv_clean_MVBS", "combine_echodata",
           "EchoData", "Dataset", "DataArray",
           "DeviceArray", "targets"]
