"""``qc``: a time coordinate that steps backwards, found and repaired on the GPU, with the reference's signatures
(echopype qc/api.py:12-128).

A file whose ``ping_time`` goes back for one ping while the pinging interval stays undisturbed is a known EK60/EK80
defect.  The repair is the reference's: with ``d = diff(time)``, every negative difference ``d[ni]`` is replaced by the
median of the ORIGINAL differences ``d[max(0, ni - win_len) : ni]`` -- all medians are taken before any substitution, a
negative difference inside another reversal's window enters that median as it is, a negative median stays negative, and
nothing is repeated --, and the times behind the first reversal ``f`` are rebuilt as ``time[f] + cumsum(d'[f:])``.
Everything is integer arithmetic on the int64 ticks of the coordinate's own datetime64 unit (the median of an even number
of differences is the wrapping sum of the two middle ones divided by 2, truncated toward zero, as ``np.median`` of
timedelta64 gives it), so the result is the reference's bit for bit.

Five launches for a repair: ``epa_time_reversals`` (count, first index, NaT count and the list of reversals),
``epa_reversal_medians`` (one wavefront per reversal, the window in LDS) and ``epa_time_rebuild`` (tile sums, carries,
apply).  The new host array is the download of the rebuilt tensor.  When the input could not be written to (resident
data, ``EchoData.to_device``) neither can the result, and it is made known to ``ops.ping_time_facts`` together with that
tensor and the verdict of ``epa_time_reversals`` run again on it -- the next ``compute_Sv`` / ``compute_MVBS`` /
``add_location`` neither looks at the times nor uploads them.

The three deviations of ``coerce_increasing_time``:

* no reversal leaves ``ds`` untouched, as the reference's docstring promises (its code raises ``IndexError``);
* a NaT anywhere in the coordinate raises ``ValueError`` (the reference's result is NaT from the first window or
  difference that holds one to the end);
* fewer than 2 times is a no-op.

A reversal in the very first difference has no window to take a median from: ``IndexError``, the reference's own type.
``create_old_time_array`` and ``orchestrate_reverse_time_check`` are the reference's Provenance plumbing for a combined
``EchoData`` (qc/api.py:131-267) without its zarr half: this package writes no files, ``zarr_store`` must be ``None``."""
import logging

import numpy as np

from .. import _lib, ops
from ..xr_lite import DataArray

logger = logging.getLogger("echopype_amd.qc")


def _ticks(ds, time_name):
    """(the coordinate's host array, its int64 device twin) -- the twin of a resident array (one that cannot be written
    to and that ``ops.ping_time_facts`` keeps by identity) is the one already in HBM."""
    values = ds[time_name].values
    if not isinstance(values, np.ndarray) or values.dtype.kind != "M":
        raise TypeError(f"{time_name} is not a datetime64 coordinate (dtype {getattr(values, 'dtype', type(values))})")
    if values.ndim != 1:
        raise ValueError(f"{time_name} must have one dimension, it has shape {values.shape}")
    if values.size == 0:
        return values, None
    if values.dtype == np.dtype("datetime64[ns]") and not values.flags.writeable:
        return values, ops.ping_time_facts(values)[2]
    return values, ops.to_device(values)


def exist_reversed_time(ds, time_name):
    """Test for occurrence of time reversal in the datetime coordinate ``time_name`` of ``ds``: ``True`` if at least one
    difference of consecutive times is negative (one launch of ``epa_time_reversals``, one read-back).  A difference
    that touches a NaT does not count, as in the reference; fewer than 2 times give ``False``."""
    values, t = _ticks(ds, time_name)
    if values.size < 2:
        return False
    facts, _ = ops.time_reversals(t)
    return bool(facts[_lib.QC_COUNT].item() != 0)


def coerce_increasing_time(ds, time_name="ping_time", win_len=100):
    """Coerce the time coordinate ``time_name`` so that it always flows forward; if coercion is necessary, ``ds`` (an
    ``xr_lite.Dataset``) is modified: ``ds[time_name] = (dims, values)``, in the coordinate's own datetime64 unit.

    ``win_len``: length of the window before a reversed time stamp within which the median pinging interval is used to
    infer the next ping time, 1 .. ``ops.QC_MAX_WIN`` (``ValueError`` below, ``NotImplementedError`` above: the window
    lives in LDS).  A coordinate that is not datetime64 raises ``TypeError``; a reversal in the first difference raises
    ``IndexError`` (the window is empty).

    Deviations from the reference: no reversal leaves ``ds`` untouched (the reference raises ``IndexError``); a NaT in the
    coordinate raises ``ValueError`` (the reference's result is a NaT tail); fewer than 2 times is a no-op."""
    if isinstance(win_len, bool) or not isinstance(win_len, (int, np.integer)):
        raise TypeError(f"win_len must be an integer, got {win_len!r}")
    if win_len < 1:
        raise ValueError(f"win_len must be at least 1, got {win_len}")
    if win_len > ops.QC_MAX_WIN:
        raise NotImplementedError(f"win_len={win_len}: windows of up to {ops.QC_MAX_WIN} differences are served")
    da = ds[time_name]
    values, t = _ticks(ds, time_name)
    if values.size < 2:
        return
    facts, lst = ops.time_reversals(t, want_list=True)
    first, count, nat, _ = facts.tolist()
    if nat:
        raise ValueError(f"{time_name} contains NaT ({nat} of {values.size}): the times must all be valid")
    if count == 0:
        return
    if first == 0:
        raise IndexError(f"{time_name} is reversed in its very first difference: the window before it is empty, there is "
                         "no interval to take a median from")
    new = ops.time_rebuild(t, facts, ops.reversal_medians(t, facts, lst, int(win_len)))
    resident = not values.flags.writeable and values.dtype == np.dtype("datetime64[ns]")
    if resident:  # (the verdict on the result comes from the device, like the result: a negative median keeps a reversal)
        again, _ = ops.time_reversals(new)
    host = new.cpu().numpy().view(values.dtype)
    host.flags.writeable = values.flags.writeable
    if resident:
        _, count2, nat2, _ = again.tolist()
        ops.register_ping_time(host, new, count2 == 0 and nat2 == 0)
    ds[time_name] = (da.dims, host)


def check_and_correct_reversed_time(combined_group, time_str, ed_group):
    """Repair the coordinate ``time_str`` of ``combined_group`` -- the dataset of the ``EchoData`` group ``ed_group`` -- in
    place when it steps backwards.  Returns a copy of the coordinate from before the repair, or ``None`` when the dataset
    has no such coordinate or it never steps backwards.  A repair is announced as a warning of the package's logger."""
    if time_str not in combined_group or not exist_reversed_time(combined_group, time_str):
        return None
    logger.warning("%s: %s steps backwards and is being repaired (the median pinging interval before each reversal "
                   "takes the place of the negative step)", ed_group, time_str)
    before = combined_group[time_str].copy()
    coerce_increasing_time(combined_group, time_name=time_str)
    return before


def create_old_time_array(group, old_time_in):
    """The uncorrected time ``old_time_in`` of the ``EchoData`` group ``group`` as the array that goes into the
    ``Provenance`` group: a copy of the values named ``<group>_old_<time>`` (the group path in lower case, ``-`` and ``/``
    written ``_``) on the dimension ``<that name>_dim``, with the input's attributes and a ``comment``.  The input is
    left as it is."""
    time_name = old_time_in.name
    name = f"{group.lower().translate(str.maketrans('-/', '__'))}_old_{time_name}"
    attrs = {**old_time_in.attrs, "comment": f"Uncorrected {time_name} from the combined group {group}."}
    return DataArray(np.array(old_time_in.values, copy=True), (f"{name}_dim",), attrs=attrs, name=name)


def orchestrate_reverse_time_check(ed_comb, zarr_store, possible_time_dims, storage_options, consolidated=True):
    """Checks every time dimension named in ``possible_time_dims`` of every group of the combined ``ed_comb`` --
    ``Platform/NMEA`` excepted, as in the reference: its sentences come out of order and are not meant to be repaired --
    and repairs in place those that step backwards (:func:`check_and_correct_reversed_time`: a resident coordinate stays
    resident).  The times from before each repair go into the ``Provenance`` group (:func:`create_old_time_array`), whose
    attribute ``reversed_ping_times`` ends as 1 if anything was repaired and 0 otherwise.  ``zarr_store`` must be ``None``
    (``NotImplementedError``): this package writes no files, so ``storage_options`` and ``consolidated`` have no effect."""
    if zarr_store is not None:
        raise NotImplementedError("orchestrate_reverse_time_check: zarr_store must be None, this package writes no files")
    provenance = ed_comb["Provenance"]
    wanted = set(possible_time_dims)
    repaired = 0
    for group in ed_comb.group_paths:
        if group == "Platform/NMEA":
            continue
        dataset = ed_comb[group]
        for time in sorted(wanted.intersection(dataset.dims)):
            before = check_and_correct_reversed_time(dataset, time, group)
            if before is None:
                continue
            kept = create_old_time_array(group, before)
            provenance[kept.name] = kept
            repaired += 1
    provenance.attrs["reversed_ping_times"] = 1 if repaired else 0


# (the two functions above are reached as qc.create_old_time_array / qc.orchestrate_reverse_time_check)
__all__ = ["exist_reversed_time", "coerce_increasing_time", "check_and_correct_reversed_time"]
