"""NumPy restatement of mask.line_mask: what the kernel must give, element for element."""
import numpy as np


def line_mask_ref(r, upper=None, lower=None, closed="left", nan_line="exclude", upper_offset=0.0, lower_offset=0.0):
    """bool array like ``r`` (..., S): True where ``upper + upper_offset <= r < lower + lower_offset`` (``closed="left"``)
    or ``upper + upper_offset < r <= lower + lower_offset`` (``"right"``).  ``r`` is compared as ``r.astype(float64)``;
    ``upper`` / ``lower``: None (not tested) or anything that broadcasts against ``r.shape[:-1]``, converted to float64
    and added to the offset in float64.  A NaN ``r`` is False; a NaN bound makes its whole row False (``"exclude"``:
    every comparison with NaN is) or is not tested in that row (``"ignore"``)."""
    assert closed in ("left", "right") and nan_line in ("exclude", "ignore") and not (upper is None and lower is None)
    r64 = np.asarray(r).astype(np.float64)
    ok = ~np.isnan(r64)
    for line, offset, is_upper in ((upper, upper_offset, True), (lower, lower_offset, False)):
        if line is None:
            continue
        with np.errstate(invalid="ignore"):
            b = np.broadcast_to(np.asarray(line, dtype=np.float64) + np.float64(offset), r64.shape[:-1])[..., None]
            if is_upper:
                t = (b <= r64) if closed == "left" else (b < r64)
            else:
                t = (r64 < b) if closed == "left" else (r64 <= b)
        if nan_line == "ignore":
            t = t | np.isnan(b)
        ok &= t
    return ok
