from .api import (METHODS_TRANSIENT, detect_transient, estimate_background_noise, estimate_noise,  # noqa: F401
                  mask_attenuated_signal, mask_impulse_noise, mask_transient_noise, remove_background_noise,
                  remove_noise, window_filter)

__all__ = ["estimate_background_noise", "remove_background_noise", "estimate_noise", "remove_noise",
           "mask_transient_noise", "mask_impulse_noise", "mask_attenuated_signal", "detect_transient",
           "METHODS_TRANSIENT", "window_filter"]
