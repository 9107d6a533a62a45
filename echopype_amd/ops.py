"""Tensor-level wrappers of the C ABI: device buffers are torch CUDA tensors (plumbing only --
allocation, streams, RCCL), every computation is a call into libechopype_amd.so.

All functions run on the tensors' device and torch's current stream and return torch tensors.
"""
import ctypes
import functools
import threading
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import call

_DT = {torch.float32: _lib.F32, torch.float64: _lib.F64}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("echopype_amd kernels need device (HBM) buffers; got a CPU tensor")
    if not t.is_contiguous():
        raise ValueError("echopype_amd kernels need C-contiguous buffers")
    return ctypes.c_void_p(t.data_ptr())


def torch_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        td = dtype
    else:
        td = {"float32": torch.float32, "float64": torch.float64}.get(np.dtype(dtype).name)
    if td not in _DT:
        raise ValueError(f"dtype must be float32 or float64, got {dtype!r}")
    return td


# ---- scratch buffers: allocated here, sized by the library ----------------------------------------------------------------
@functools.lru_cache(maxsize=4096)
def _ask(name, *args, answer=ctypes.c_int):
    """A host-side question to the library, asked once per distinct arguments: the size of a scratch buffer, a yes / no
    about a call yet to be made."""
    ans = answer()
    _lib.check(getattr(_lib.lib, name)(*args, ctypes.byref(ans)), name)
    return ans.value


def scratch_bytes(what, a=0, b=0, c=0):
    """Bytes of the scratch buffer ``what`` ("<entry>.<parameter>", the table at ``epa_scratch_bytes`` in the header)."""
    return _ask("epa_scratch_bytes", what.encode(), int(a), int(b), int(c), answer=ctypes.c_size_t)


def _scratch_alloc(nbytes, dtype, device, zero):
    """A tensor of ``dtype`` that covers ``nbytes``: the one place scratch memory is allocated (tests wrap it)."""
    return (torch.zeros if zero else torch.empty)(-(-nbytes // dtype.itemsize), dtype=dtype, device=device)


def _scratch(what, device, a=0, b=0, c=0, dtype=torch.float64, zero=False):
    return _scratch_alloc(scratch_bytes(what, a, b, c), dtype, device, zero)


def _partials(want, C, n_tbins, n_rbins, dtype, dev, ask=True):
    """(sum, count) arrays of a binned reduction when asked for or (``ask``) when the library may need them."""
    if not (want or (ask and reduce_needs_workspace(C, n_tbins, n_rbins, dtype))):
        return None, None
    shape = (C, n_tbins, n_rbins)
    return torch.empty(shape, dtype=dtype, device=dev), torch.empty(shape, dtype=torch.int32, device=dev)


class _Uploader:
    """Host -> HBM copies that never make the HOST wait for the GPU.

    ``tensor.to(device)`` from pageable memory is a blocking copy on torch's current stream: it returns only after every
    kernel queued before it has finished -- a dozen small parameter uploads per API call then serialise the host with
    the previous call's 10-ms kernel.  Here the array is staged in a pinned buffer (a pool: hipHostMalloc is slow, the
    buffers are re-used once the copy that read them has completed), copied on a dedicated upload stream
    (``non_blocking``), and the CURRENT stream is made to wait for that copy ON THE DEVICE (an event): the host moves on
    at once, kernels launched afterwards see the data.  One instance per device."""

    _MAX_POOL = 64
    _MAX_BYTES = 256 << 20  # larger arrays (bulk sample data) take the plain blocking copy: staging them twice costs more

    def __init__(self, device):
        self.device = device
        self.stream = torch.cuda.Stream(device=device)
        self.pool = []  # [pinned uint8 tensor, event of the last copy that read it]
        self.lock = threading.Lock()  # picking a staging buffer and marking it busy is one step, also across threads

    def _staging(self, nbytes):
        best = None
        for slot in self.pool:
            buf, ev = slot
            if buf.numel() >= nbytes and (ev is None or ev.query()) and (best is None or buf.numel() < best[0].numel()):
                best = slot
        if best is None:
            if len(self.pool) >= self._MAX_POOL:  # drop the smallest idle buffer
                idle = [s_ for s_ in self.pool if s_[1] is None or s_[1].query()]
                if idle:
                    self.pool.remove(min(idle, key=lambda s_: s_[0].numel()))
            best = [torch.empty(max(4096, 1 << (int(nbytes) - 1).bit_length()), dtype=torch.uint8, pin_memory=True), None]
            self.pool.append(best)
        return best

    def upload(self, a):
        """C-contiguous numpy array -> device tensor of the same shape / dtype, ordered before whatever the current
        stream is given next."""
        nbytes = a.nbytes
        if nbytes == 0 or nbytes > self._MAX_BYTES:
            w = a if a.flags.writeable else a.copy()
            return torch.from_numpy(w).to(self.device)
        tdt = torch.from_numpy(np.empty(0, dtype=a.dtype)).dtype
        cur = torch.cuda.current_stream(self.device)
        with self.lock:
            slot = self._staging(nbytes)
            staged = slot[0][:nbytes]
            staged.numpy().view(np.uint8)[:] = a.reshape(-1).view(np.uint8)
            with torch.cuda.stream(self.stream):
                out = torch.empty(a.shape, dtype=tdt, device=self.device)
                out.view(-1).view(torch.uint8).copy_(staged, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.stream)
            slot[1] = ev
        cur.wait_event(ev)
        out.record_stream(cur)  # (allocated on the upload stream, used on the current one)
        out._epa_ready = ev  # (a holder that hands the tensor to ANOTHER stream later makes that stream wait for it)
        return out


class HostFuture:
    """A few numbers on their way from HBM to the host (``fetch_async``).  ``.cpu()`` waits for THAT copy only -- not
    for whatever was queued on the compute stream after it -- and returns the host tensor (so ``fut.cpu().tolist()``
    reads like the blocking ``tensor.cpu().tolist()`` it replaces)."""

    __slots__ = ("_slot", "_host", "_event", "_value")

    def __init__(self, slot, host, event):
        self._slot, self._host, self._event, self._value = slot, host, event, None

    def cpu(self):
        if self._value is None:
            self._event.synchronize()
            self._value = self._host.clone()
            self._slot[1] = None  # the staging buffer may be re-used
            self._slot = self._host = None
        return self._value

    def tolist(self):
        return self.cpu().tolist()

    def item(self):
        return self.cpu().item()

    def __del__(self):
        # never read: hand the staging buffer back (a later copy into it is queued on the same download stream behind
        # this one, so the two cannot overlap)
        slot = getattr(self, "_slot", None)
        if slot is not None:
            slot[1] = None


class _Downloader:
    """HBM -> host copies of kernel by-products (range statistics, a maximum) that do not queue behind later work.

    ``tensor.cpu()`` is a copy on the CURRENT stream: issued after the next file's 10-ms kernel has been launched it
    completes only when that kernel has.  Here an event marks the point of the current stream where the numbers are
    final, a dedicated download stream waits for that event and copies into a pinned buffer, and the reader waits for
    the copy's own event.  One instance per device; buffers come from a small pinned pool."""

    def __init__(self, device):
        self.device = device
        self.stream = torch.cuda.Stream(device=device)
        self.pool = []  # [pinned uint8 tensor, busy marker]
        self.lock = threading.Lock()

    def fetch(self, t):
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        with self.lock:
            slot = next((s_ for s_ in self.pool if s_[1] is None and s_[0].numel() >= nbytes), None)
            if slot is None:
                slot = [torch.empty(max(256, 1 << (int(nbytes) - 1).bit_length()), dtype=torch.uint8, pin_memory=True), None]
                self.pool.append(slot)
            slot[1] = True
        host = slot[0][:nbytes].view(t.dtype).view(t.shape)
        cur = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(cur)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            host.copy_(t, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        t.record_stream(self.stream)
        return HostFuture(slot, host, done)


_uploaders = {}
_downloaders = {}


def fetch_async(t):
    """Start copying a (small) device tensor to the host NOW, on a side stream, ordered after everything queued on the
    current stream so far; returns a :class:`HostFuture`."""
    dl = _downloaders.get(t.device)
    if dl is None:
        dl = _downloaders[t.device] = _Downloader(t.device)
    return dl.fetch(t)


def _uploader(dev):
    up = _uploaders.get(dev)
    if up is None:
        up = _uploaders[dev] = _Uploader(dev)
    return up


def to_device(a, dtype=None, device=None):
    """numpy / torch -> contiguous CUDA tensor.  Host arrays go up through :class:`_Uploader` (pinned staging, upload
    stream, a device-side wait): the call does not synchronise the host with the kernels already queued."""
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(dev)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if isinstance(a, torch.Tensor):
        t = a
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        if not t.is_cuda:
            t = _uploader(dev).upload(t.contiguous().numpy()) if dev.type == "cuda" else t.to(dev)
        return t.contiguous()
    a = np.ascontiguousarray(a)
    if dtype is not None:
        want = np.dtype(str(dtype).replace("torch.", ""))
        if a.dtype != want:
            a = a.astype(want)
    if a.dtype.kind == "M":  # datetime64 -> its int64 representation
        a = a.view(np.int64)
    if dev.type != "cuda":
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
    return _uploader(dev).upload(a)


# ---- what does not change from call to call stays in HBM ----------------------------------------------------------------
_SMALL = {}        # (device, dtype, shape, bytes) -> tensor: per-channel tables and vectors (<= 2 KiB), the same for every
_SMALL_MAX = 256   # file of a survey; read-only by contract (kernel inputs)


def to_device_small(a, dtype=None, device=None):
    """``to_device`` for a tiny parameter array (a (C,) vector, a (C, K) table): the device copy is kept, keyed on the
    CONTENT, and handed out again -- a call then uploads nothing for parameters it shares with the previous call (six
    staging copies and events per compute_Sv, a quarter of its host time).  Larger arrays take ``to_device``.  The
    tensors are shared: nobody writes to them."""
    a = np.ascontiguousarray(a)
    if dtype is not None:
        want = np.dtype(str(dtype).replace("torch.", ""))
        if a.dtype != want:
            a = a.astype(want)
    if a.nbytes > 2048 or a.nbytes == 0:
        return to_device(a, device=device)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (dev, a.dtype.str, a.shape, a.tobytes())
    ent = _SMALL.get(key)
    if ent is None:
        if len(_SMALL) >= _SMALL_MAX:
            _SMALL.clear()
        t = to_device(a, device=dev)
        ev = getattr(t, "_epa_ready", None)
        if ev is not None:
            ev.synchronize()  # (once per distinct content: afterwards the copy is there for every stream)
        _SMALL[key] = ent = t
    return ent


_PING_NS = {}  # id(ndarray) -> (weakref to it, int64 view, sorted and valid?, {device: tensor})


def ping_time_facts(ping_time, want_device=True):
    """(int64 ns view, sorted without NaT?, int64 device tensor | None) of a datetime64[ns] ping_time coordinate.  For an array
    that cannot be written to (``EchoData.to_device`` marks the beam groups' ping_time so -- resident data, like the
    samples) the three are kept with the ARRAY OBJECT: the O(P) look at the time stamps and their 8 P-byte upload are
    then paid once per file, not once per call.  A writeable array is looked at and uploaded every time."""
    pt = np.asarray(ping_time)
    if pt.dtype != np.dtype("datetime64[ns]"):
        pt = pt.astype("datetime64[ns]")
    dev = torch.device("cuda", torch.cuda.current_device())
    ent = _PING_NS.get(id(pt)) if not pt.flags.writeable else None
    if ent is not None and ent[0]() is pt:
        _, ns, ok, tens = ent
    else:
        ns = pt.view(np.int64)
        # unsorted, or NaT (INT64_MIN: the smallest value, so in a sorted array it could only be the first)
        ok = bool(ns.size) and not bool(np.any(ns[1:] < ns[:-1])) and ns[0] != np.iinfo(np.int64).min
        tens = {}
        if not pt.flags.writeable:
            key = id(pt)
            _PING_NS[key] = (weakref.ref(pt, lambda _r, k=key: _PING_NS.pop(k, None)), ns, ok, tens)
    if not want_device:
        return ns, ok, None
    t = tens.get(dev)
    if t is None:
        t = to_device(ns, device=dev)
        tens[dev] = t
    else:  # (uploaded under another call's stream: this one waits for that copy on the device)
        ev = getattr(t, "_epa_ready", None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
    return ns, ok, t


def register_ping_time(ping_time, tensor, sorted_and_valid):
    """Make a datetime64[ns] array that cannot be written to known to :func:`ping_time_facts` together with its int64
    device twin ``tensor`` and the verdict ``sorted_and_valid``, both computed on the device already (``qc``: the
    repaired coordinate is the download of ``tensor``).  The next ``ping_time_facts(ping_time)`` on that device then
    neither looks at the times nor uploads them.  The caller vouches for the three belonging together."""
    pt = ping_time
    if not isinstance(pt, np.ndarray) or pt.dtype != np.dtype("datetime64[ns]") or pt.flags.writeable:
        raise ValueError("register_ping_time: a datetime64[ns] ndarray that cannot be written to is needed")
    if tensor.dtype != torch.int64 or tuple(tensor.shape) != pt.shape or not tensor.is_cuda or not tensor.is_contiguous():
        raise ValueError(f"register_ping_time: the tensor must be contiguous int64 of shape {pt.shape} on a device, got "
                         f"{tensor.dtype} {tuple(tensor.shape)} on {tensor.device}")
    key = id(pt)
    _PING_NS[key] = (weakref.ref(pt, lambda _r, k=key, known=_PING_NS: known.pop(k, None)), pt.view(np.int64),
                     bool(sorted_and_valid), {tensor.device: tensor})


def _mode_of(t, C, P):
    n = t.numel()
    if n == 1:
        return _lib.PM_SCALAR
    if n == C and t.dim() <= 1:
        return _lib.PM_CHANNEL
    if n == C * P:
        return _lib.PM_CHANNEL_PING
    raise ValueError(f"parameter of shape {tuple(t.shape)} is not scalar, (C,) or (C,P) with C={C}, P={P}")


def _tau_mode(tau_eff, C, P):
    """tau_effective: (C,) per channel, or (C, P) -- an EK80 file with several filter_time intervals."""
    if tuple(tau_eff.shape) == (C,):
        return _lib.PM_CHANNEL
    if tuple(tau_eff.shape) == (C, P):
        return _lib.PM_CHANNEL_PING
    raise ValueError(f"tau_eff of shape {tuple(tau_eff.shape)}: expected ({C},) or ({C}, {P})")


def power_coef_ek(sample_interval, tau_nominal, transmit_power, sound_speed, absorption, gain, sa,
                  psi, f_nominal, tau_eff, *, sonar="EK60", cal_type="Sv", pulse_length=None,
                  gain_is_table=False, sa_is_table=False, gpt=None):
    """K0 -> coef (C, P, NCOEF) f64.  All inputs f64 CUDA tensors; ``psi`` scalar, (C,) or (C, P)."""
    C, P = sample_interval.shape
    coef = torch.empty((C, P, _lib.NCOEF), dtype=torch.float64, device=sample_interval.device)
    K = 0 if pulse_length is None else pulse_length.shape[1]
    gmode = _lib.PM_PULSE_TABLE if gain_is_table else _mode_of(gain, C, P)
    smode = _lib.PM_PULSE_TABLE if sa_is_table else _mode_of(sa, C, P)
    call("epa_power_coef_ek", C, P, _p(sample_interval), _p(tau_nominal), _p(transmit_power),
         _p(sound_speed), _mode_of(sound_speed, C, P), _p(absorption), _mode_of(absorption, C, P),
         _p(gain), gmode, _p(sa), smode, _p(pulse_length), K, _p(psi), _mode_of(psi, C, P), _p(f_nominal), _p(tau_eff),
         _tau_mode(tau_eff, C, P), _p(gpt), _lib.SONAR_EK60 if sonar in ("EK60", "ES70") else _lib.SONAR_EK80,
         _lib.CAL_SV if cal_type == "Sv" else _lib.CAL_TS, _p(coef), _stream())
    return coef


def pulse_table_lookup(tau_nominal, pulse_length, table):
    """(C, P) f64: table[c, argmin_k |tau[c,p] - pulse_length[c,k]|] (get_vend_cal_params_power on the device)."""
    C, P = tau_nominal.shape
    out = torch.empty((C, P), dtype=torch.float64, device=tau_nominal.device)
    call("epa_pulse_table_lookup", _p(tau_nominal), _p(pulse_length), _p(table), C, P, pulse_length.shape[1], _p(out),
         _stream())
    return out


def sv_power_vectorized(raw, S, dtype):
    """True when K1 takes its 16-byte path on these buffers (needed for range statistics without the range array)."""
    # (asked once per (alignment, S, dtype): the rule looks at the address's low four bits only)
    return _ask("epa_sv_power_vectorized", raw.data_ptr() % 16, int(S), _DT.get(dtype, _lib.F32)) != 0


def sv_power(raw, coef, *, cal_type="Sv", flags=_lib.FLAG_GUARD_POS | _lib.FLAG_MASK_RANGE,
             dtype=torch.float64, want_range=True, out=None, range_out=None, want_range_stats=False):
    """K1 -> (Sv|TS, echo_range|None), both (C,P,S) of dtype [, f64 device tensor {nanmin, nanmax, NaN count} of
    the echo_range, a by-product of the same pass].  ``want_range=False`` with ``want_range_stats=True``: the
    statistics of the echo_range that would be written, without the array (range_power writes it later if needed)."""
    C, P, S = raw.shape
    if raw.dtype != torch.float32:
        raise ValueError("raw power samples must be float32 (convert/parse_base.py:302)")
    if out is None:
        out = torch.empty((C, P, S), dtype=dtype, device=raw.device)
    if want_range and range_out is None:
        range_out = torch.empty((C, P, S), dtype=dtype, device=raw.device)
    ct = _lib.CAL_SV if cal_type == "Sv" else _lib.CAL_TS
    if want_range_stats:
        ws = _scratch("sv_power_stats.workspace", raw.device, S)
        stats = torch.empty(3, dtype=torch.float64, device=raw.device)
        call("epa_sv_power_stats", _p(raw), _p(coef), C, P, S, ct, flags, _p(out),
             _p(range_out) if want_range else None, _DT[out.dtype], _p(ws), _p(stats), _stream())
        return out, (range_out if want_range else None), stats
    call("epa_sv_power", _p(raw), _p(coef), C, P, S, ct, flags, _p(out), _p(range_out) if want_range else None,
         _DT[out.dtype], _stream())
    return out, (range_out if want_range else None)


def range_power(raw, coef, *, flags=_lib.FLAG_MASK_RANGE, dtype=torch.float64):
    """echo_range (C,P,S) of the power-sample coefficient rows alone (what K1 writes as range_out)."""
    C, P, S = raw.shape
    out = torch.empty((C, P, S), dtype=dtype, device=raw.device)
    call("epa_range_power", _p(raw), _p(coef), C, P, S, flags, _p(out), _DT[dtype], _stream())
    return out


def time_bin_offsets(ping_time_ns, t0, dt, n_bins, closed="left"):
    """CSR offsets (n_bins+1,) int32 of sorted int64-ns ping times against uniform edges."""
    P = ping_time_ns.numel()
    out = torch.empty(n_bins + 1, dtype=torch.int32, device=ping_time_ns.device)
    call("epa_time_bin_offsets", _p(ping_time_ns), P, int(t0), int(dt), int(n_bins),
         _lib.BIN_CLOSED_RIGHT if closed == "right" else 0, _p(out), _stream())
    return out


def _bin_flags(skipna, closed):
    return (_lib.BIN_SKIPNA if skipna else 0) | (_lib.BIN_CLOSED_RIGHT if closed == "right" else 0)


def reduce_needs_workspace(C, n_tbins, n_rbins, dtype):
    """Few ping bins, or a range grid too large for LDS, MAY need caller-provided sum / count arrays."""
    return _ask("epa_mvbs_needs_partials", int(C), int(n_tbins), int(n_rbins), _DT.get(dtype, _lib.F32)) != 0


def sv_mvbs_fused(raw, coef, bin_start, n_tbins, range_bin, n_rbins, *, cal_type="Sv",
                  cal_flags=_lib.FLAG_GUARD_POS | _lib.FLAG_MASK_RANGE, skipna=True, closed="left",
                  fill_value=float("nan"), dtype=torch.float64, want_sv=True, want_range=False,
                  want_partials=False, ping_perm=None, sv_out=None, range_out=None, mvbs_out=None,
                  want_range_max=False, want_range_stats=False):
    """K1+K5 -> dict(Sv, echo_range, MVBS, sum, cnt, range_max, range_stats).  ``want_range_stats``: f64 device tensor
    {nanmin, nanmax, NaN count} of the echo_range array that is NOT written (NaN count -1: the kernel that served the
    configuration leaves the maximum only)."""
    C, P, S = raw.shape
    dev = raw.device
    if want_sv and sv_out is None:
        sv_out = torch.empty((C, P, S), dtype=dtype, device=dev)
    if want_range and range_out is None:
        range_out = torch.empty((C, P, S), dtype=dtype, device=dev)
    if mvbs_out is None:
        mvbs_out = torch.empty((C, n_tbins, n_rbins), dtype=dtype, device=dev)
    ssum, cnt = _partials(want_partials, C, n_tbins, n_rbins, dtype, dev)
    rmax = torch.empty(1, dtype=torch.float64, device=dev) if want_range_max or want_range_stats else None
    rstats = torch.empty(3, dtype=torch.float64, device=dev) if want_range_stats else None
    call("epa_sv_mvbs_fused", _p(raw), _p(coef), C, P, S,
         _lib.CAL_SV if cal_type == "Sv" else _lib.CAL_TS, cal_flags, _p(bin_start), _p(ping_perm),
         int(n_tbins), float(range_bin), int(n_rbins), _bin_flags(skipna, closed), float(fill_value),
         _p(sv_out) if want_sv else None, _p(range_out) if want_range else None, _p(mvbs_out),
         _p(ssum), _p(cnt), _p(rmax), _p(rstats), _DT[dtype], _stream())
    return dict(Sv=sv_out if want_sv else None, echo_range=range_out if want_range else None,
                MVBS=mvbs_out, sum=ssum, cnt=cnt, range_max=rmax, range_stats=rstats,
                range_stats_filled=bool(_lib.lib.epa_last_range_stats_filled()) if want_range_stats else False)


def sv_mvbs_fused_depth(raw, coef, depth_scale, depth_offset, bin_start, n_tbins, range_bin, n_rbins, *, cal_type="Sv",
                        fill_value=float("nan"), dtype=torch.float64, want_sv=True, want_depth=False,
                        want_partials=False, sv_out=None, mvbs_out=None):
    """K1+K5 binned on depth = depth_offset[c,p] + depth_scale[c,p] * echo_range (add_depth fused into the pass) ->
    dict(Sv, depth, MVBS, sum, cnt, range_stats = f64 device tensor {nanmin, nanmax, NaN count} of the depth array).
    Raises EpaError (EPA_EUNSUPPORTED) for a configuration only the generic kernels serve."""
    C, P, S = raw.shape
    dev = raw.device
    if want_sv and sv_out is None:
        sv_out = torch.empty((C, P, S), dtype=dtype, device=dev)
    depth_out = torch.empty((C, P, S), dtype=dtype, device=dev) if want_depth else None
    if mvbs_out is None:
        mvbs_out = torch.empty((C, n_tbins, n_rbins), dtype=dtype, device=dev)
    ssum, cnt = _partials(want_partials, C, n_tbins, n_rbins, dtype, dev, ask=False)
    rstats = _scratch("sv_mvbs_fused_depth.depth_stats_out", dev)
    call("epa_sv_mvbs_fused_depth", _p(raw), _p(coef), _p(depth_scale), _p(depth_offset), C, P, S,
         _lib.CAL_SV if cal_type == "Sv" else _lib.CAL_TS, _p(bin_start), int(n_tbins), float(range_bin), int(n_rbins),
         float(fill_value), _p(sv_out) if want_sv else None, _p(depth_out), _p(mvbs_out), _p(ssum), _p(cnt), _p(rstats),
         _DT[dtype], _stream())
    return dict(Sv=sv_out if want_sv else None, depth=depth_out, MVBS=mvbs_out, sum=ssum, cnt=cnt,
                range_stats=rstats[:3], range_stats_filled=True)


def sv_mvbs_fused_i16(raw_i16, n_valid, coef, bin_start, n_tbins, range_bin, n_rbins, *, cal_type="Sv",
                      fill_value=float("nan"), dtype=torch.float64, want_sv=True, want_partials=False,
                      sv_out=None, mvbs_out=None, want_range_max=False):
    """K1+K5 fed with int16 instrument samples + per-ping recorded lengths."""
    C, P, S = raw_i16.shape
    if raw_i16.dtype != torch.int16 or n_valid.dtype != torch.int32:
        raise ValueError("raw_i16 must be int16 and n_valid int32")
    dev = raw_i16.device
    if want_sv and sv_out is None:
        sv_out = torch.empty((C, P, S), dtype=dtype, device=dev)
    if mvbs_out is None:
        mvbs_out = torch.empty((C, n_tbins, n_rbins), dtype=dtype, device=dev)
    ssum, cnt = _partials(want_partials, C, n_tbins, n_rbins, dtype, dev, ask=False)
    rmax = torch.empty(1, dtype=torch.float64, device=dev) if want_range_max else None
    call("epa_sv_mvbs_fused_i16", _p(raw_i16), _p(n_valid), _p(coef), C, P, S,
         _lib.CAL_SV if cal_type == "Sv" else _lib.CAL_TS, _p(bin_start), int(n_tbins), float(range_bin),
         int(n_rbins), float(fill_value), _p(sv_out) if want_sv else None, _p(mvbs_out), _p(ssum), _p(cnt),
         _p(rmax), _DT[dtype], _stream())
    return dict(Sv=sv_out if want_sv else None, MVBS=mvbs_out, sum=ssum, cnt=cnt, range_max=rmax)


def mvbs(sv, bin_start, n_tbins, range_bin, n_rbins, *, range=None, coef=None, skipna=True,
         closed="left", fill_value=float("nan"), want_partials=False, ping_perm=None, coef_as_stored=False):
    """K5 on an existing Sv -> dict(MVBS, sum, cnt).  ``coef`` (power-sample coefficient rows) in place of ``range``:
    the range is evaluated in the kernel; ``coef_as_stored`` rounds it to Sv's dtype first, i.e. bins exactly as on
    the echo_range array K1 would have written."""
    C, P, S = sv.shape
    dev, dtype = sv.device, sv.dtype
    if range is not None and range.dtype != dtype:
        range = range.to(dtype)
    out = torch.empty((C, n_tbins, n_rbins), dtype=dtype, device=dev)
    ssum, cnt = _partials(want_partials, C, n_tbins, n_rbins, dtype, dev)
    call("epa_mvbs", _p(sv), _p(range), _p(coef), C, P, S, _p(bin_start), _p(ping_perm), int(n_tbins),
         float(range_bin), int(n_rbins), _bin_flags(skipna, closed) | (_lib.BIN_RANGE_AS_STORED if coef_as_stored else 0),
         float(fill_value), _p(out), _p(ssum), _p(cnt), _DT[dtype], _stream())
    return dict(MVBS=out, sum=ssum, cnt=cnt)


def _selftest_f64(x, who):
    if x.dtype != torch.float64:  # (the entries take doubles and nothing else: another type would be read and written past its end)
        raise ValueError(f"{who}: a float64 tensor expected, got {x.dtype}")


def selftest_lin_from_db(u):
    """10^(u/10) through the fused kernel's table-driven f64 routine (accuracy self-test)."""
    _selftest_f64(u, "selftest_lin_from_db")
    out = torch.empty_like(u)
    call("epa_selftest_lin_from_db", _p(u), _p(out), u.numel(), _stream())
    return out


def selftest_log10(x, inline=False):
    _selftest_f64(x, "selftest_log10")
    out = torch.empty_like(x)
    call("epa_selftest_log10_inline" if inline else "epa_selftest_log10", _p(x), _p(out), x.numel(), _stream())
    return out


def selftest_correlate(x, replica, fft_dtype=None):
    """The raw output of the LDS transform's circular correlation (accuracy self-test): ``x`` (T, 2048) complex64 /
    complex128 tiles, ``replica`` complex64 (taps <= 2048) -> out[t, k] = sum_j x[t, (k + j) mod 2048] conj(replica[j])
    in ``x``'s precision, through the spectrum the replica preparation of sv_complex's fft form builds."""
    if x.dim() != 2 or x.shape[1] != _lib.EK80_NFFT or x.dtype not in (torch.complex64, torch.complex128):
        raise ValueError(f"x: (T, {_lib.EK80_NFFT}) complex64 / complex128 tiles expected")
    if replica.dtype != torch.complex64 or replica.dim() != 1 or not 1 <= replica.numel() <= _lib.EK80_NFFT:
        raise ValueError(f"replica: 1 .. {_lib.EK80_NFFT} complex64 taps expected")
    fdt = torch.float32 if x.dtype == torch.complex64 else torch.float64
    if fft_dtype is not None and torch_dtype(fft_dtype) != fdt:
        raise ValueError("fft_dtype is the precision of x")
    xr, rr = torch.view_as_real(x.contiguous()), torch.view_as_real(replica.contiguous())
    off = torch.tensor([0, replica.numel()], dtype=torch.int32, device=x.device)
    ws = _scratch("selftest_correlate.workspace", x.device, 1, 1, 1)
    out = torch.empty_like(xr)
    call("epa_selftest_correlate", _p(xr), x.shape[0], _p(rr), _p(off), _DT[fdt], _p(out), _p(ws), _stream())
    return torch.view_as_complex(out)


def mvbs_finalize(ssum, cnt, fill_value=float("nan")):
    out = torch.empty_like(ssum)
    call("epa_mvbs_finalize", _p(ssum), _p(cnt), ssum.numel(), float(fill_value), _p(out),
         _DT[ssum.dtype], _stream())
    return out


def affine_rows(x, scale, offset):
    """out[c,p,:] = offset[c,p] + scale[c,p] * x[c,p,:]  (add_depth)."""
    C, P, S = x.shape
    out = torch.empty_like(x)
    call("epa_affine_rows", _p(x), _p(scale), _p(offset), C, P, S, _p(out), _DT[x.dtype], _stream())
    return out


def depth_rows(scale, offset, *, range=None, coef=None, mask_raw=None, shape=None, dtype=None, want_stats=True):
    """depth = offset[c,p] + scale[c,p] * echo_range -> (depth (C,P,S), f64 device tensor {nanmin, nanmax, NaN count} of
    it, or None without ``want_stats``: from the coefficient rows that is the loop-free one-piece kernel).  echo_range as
    the array ``range`` or evaluated from the coefficient rows ``coef`` (+ ``mask_raw``: NaN where the raw power sample
    is), then ``shape`` = (C, P, S) and ``dtype`` say what to produce."""
    if range is not None:
        C, P, S = range.shape
        dtype, dev = range.dtype, range.device
    else:
        C, P, S = shape
        dev = coef.device
    out = torch.empty((C, P, S), dtype=dtype, device=dev)
    ws = _scratch("depth_rows.workspace", dev) if want_stats else None
    stats = torch.empty(3, dtype=torch.float64, device=dev) if want_stats else None
    call("epa_depth_rows", _p(range), _p(coef), _p(mask_raw), _p(scale), _p(offset), C, P, S, _p(out), _DT[dtype],
         _p(ws), _p(stats), _stream())
    return out, stats


def nanminmax(x, with_nan_count=False):
    """(nanmin, nanmax[, number of NaNs]) of a device tensor as Python floats (one 24-byte D2H copy)."""
    ws = _scratch("nanminmax.workspace", x.device)
    out = torch.empty(3, dtype=torch.float64, device=x.device)
    call("epa_nanminmax", _p(x), x.numel(), _DT[x.dtype], _p(ws), _p(out), _stream())
    lo, hi, nn = out.cpu().tolist()
    return (lo, hi, int(nn)) if with_nan_count else (lo, hi)


def mvbs_index(sv, ping_num, range_sample_num, range=None):
    """K5' -> (MVBS (C,Pb,Sb), echo_range block-min or None)."""
    C, P, S = sv.shape
    Pb, Sb = -(-P // ping_num), -(-S // range_sample_num)
    out = torch.empty((C, Pb, Sb), dtype=sv.dtype, device=sv.device)
    rmin = None
    if range is not None:
        if range.dtype != sv.dtype:
            range = range.to(sv.dtype)
        rmin = torch.empty((C, Pb, Sb), dtype=sv.dtype, device=sv.device)
    call("epa_mvbs_index", _p(sv), _p(range), C, P, S, int(ping_num), int(range_sample_num), _p(out),
         _p(rmin), _DT[sv.dtype], _stream())
    return out, rmin


def noise_estimate(sv, alpha2, ping_num, range_sample_num, *, range=None, coef=None,
                   noise_max=float("nan"), ping_phase=0, want_edges=False):
    """K6 -> noise (C, ceil((P + ping_phase) / ping_num)) f64 [, edge_sum f64 (2, C, Sb), edge_cnt int32 (2, C, Sb):
    raw (sum, count) per range block of the first / last ping block, for the cross-shard merge]."""
    C, P, S = sv.shape
    if range is not None and range.dtype != sv.dtype:
        range = range.to(sv.dtype)
    out = torch.empty((C, -(-(P + ping_phase) // ping_num)), dtype=torch.float64, device=sv.device)
    es = ec = None
    if want_edges:
        Sb = -(-S // range_sample_num)
        es = torch.zeros((2, C, Sb), dtype=torch.float64, device=sv.device)
        ec = torch.zeros((2, C, Sb), dtype=torch.int32, device=sv.device)
    call("epa_noise_estimate", _p(sv), _p(range), _p(coef), _p(alpha2), C, P, S, int(ping_num),
         int(range_sample_num), int(ping_phase), float(noise_max), _p(out), _p(es), _p(ec), _DT[sv.dtype], _stream())
    return (out, es, ec) if want_edges else out


def noise_finalize(ssum, cnt, noise_max=float("nan")):
    """Merged (sum, count) rows (rows, Sb) f64 -> noise per row (clean/api.py:402-422)."""
    rows, Sb = ssum.shape
    out = torch.empty(rows, dtype=torch.float64, device=ssum.device)
    call("epa_noise_finalize", _p(ssum), _p(cnt), rows, Sb, float(noise_max), _p(out), _stream())
    return out


def noise_apply(sv, alpha2, noise, ping_num, snr_threshold, *, range=None, coef=None, mask_raw=None,
                want_noise=True, want_corrected=True, want_minmax=False, ping_phase=0, minmax_async=False):
    """K7 -> (Sv_noise, Sv_corrected[, [min, max of Sv_noise, min, max of Sv_corrected]]).  ``coef`` + ``mask_raw``
    (the f32 power samples) in place of ``range``: the echo_range array evaluated in the kernel, NaN where the raw
    sample is.  ``minmax_async``: the four numbers as a ``HostFuture`` (the call does not wait for its kernel)."""
    C, P, S = sv.shape
    if range is not None and range.dtype != sv.dtype:
        range = range.to(sv.dtype)
    sn = torch.empty_like(sv) if want_noise else None
    sc = torch.empty_like(sv) if want_corrected else None
    mm = torch.empty(4, dtype=torch.float64, device=sv.device) if want_minmax else None
    if range is None and mask_raw is not None:
        call("epa_noise_apply_rows", _p(sv), _p(coef), _p(mask_raw), _p(alpha2), _p(noise), C, P, S, int(ping_num),
             int(ping_phase), float(snr_threshold), _p(sn), _p(sc), _p(mm), _DT[sv.dtype], _stream())
    else:
        call("epa_noise_apply", _p(sv), _p(range), _p(coef), _p(alpha2), _p(noise), C, P, S, int(ping_num),
             int(ping_phase), float(snr_threshold), _p(sn), _p(sc), _p(mm), _DT[sv.dtype], _stream())
    return (sn, sc, fetch_async(mm) if minmax_async else mm.cpu().tolist()) if want_minmax else (sn, sc)


def complex_coef_ek80(params, tau_eff, C, P, *, B, bb, cal_type="Sv", gpt=None):
    """EK80 complex-sample coefficient rows (C, P, NCCOEF) f64 on the device.  ``params``: name -> f64 device tensor of
    shape (), (C,) or (C, P) for the names of _lib.CCP (missing / None = unused by this mode)."""
    dev = tau_eff.device
    ptrs = (ctypes.c_void_p * len(_lib.CCP))()
    modes = (ctypes.c_int * len(_lib.CCP))()
    keep = []
    for k, name in enumerate(_lib.CCP):
        t = params.get(name)
        if t is None:
            ptrs[k], modes[k] = None, _lib.PM_SCALAR
            continue
        t = t.to(torch.float64).contiguous()
        keep.append(t)
        ptrs[k], modes[k] = t.data_ptr(), _mode_of(t, C, P)
    out = torch.empty((C, P, _lib.NCCOEF), dtype=torch.float64, device=dev)
    call("epa_complex_coef_ek80", C, P, ptrs, modes, _p(tau_eff), _tau_mode(tau_eff, C, P), _p(gpt), int(B), 1 if bb else 0,
         _lib.CAL_SV if cal_type == "Sv" else _lib.CAL_TS, _p(out), _stream())
    return out


def sv_complex_uses_fft(replica, max_taps, method="auto"):
    """The form sv_complex picks: LDS-FFT for replicas of 16 .. 1024 taps (or on request), direct otherwise / CW."""
    return replica is not None and (method == "fft" or (method == "auto" and 16 <= max_taps <= _lib.EK80_NFFT // 2))


def range_complex(re, ccoef, *, dtype=torch.float64):
    """echo_range (C,P,S) of complex samples alone (what the sample kernels write as range_out)."""
    C, P, S, B = re.shape
    out = torch.empty((C, P, S), dtype=dtype, device=re.device)
    call("epa_range_complex", _p(re), _DT[re.dtype], _p(ccoef), C, P, S, B, _p(out), _DT[dtype], _stream())
    return out


def power_rows_of_complex(ccoef):
    """(C, P, NCOEF) power-sample coefficient rows with the range terms of the complex-sample rows (range =
    (s * ra) * rb, nothing else set): what epa_mvbs takes in place of an echo_range array."""
    rows = torch.zeros(tuple(ccoef.shape[:2]) + (_lib.NCOEF,), dtype=torch.float64, device=ccoef.device)
    rows[..., 0] = ccoef[..., _lib.CC_RA]
    rows[..., 1] = ccoef[..., _lib.CC_RB]
    return rows


def sv_complex(re, im, ccoef, *, replica=None, replica_off=None, max_taps=0, cal_type="Sv",
               dtype=torch.float64, want_range=True, want_prx=False, method="auto", fft_dtype=None,
               want_range_stats=False, replica_id=None):
    """K3+K4 -> dict(out, echo_range, prx[, range_stats]).  ``method``: "direct" (sliding register window),
    "fft" (LDS-resident 2048-point FFT per tile) or "auto" (fft for replicas of 16 .. 1024 taps, where it is
    faster; direct otherwise and for CW).  ``fft_dtype``: arithmetic of the transform, default = ``dtype`` (float32
    output takes complex64 butterflies, as precise as that output; float64 output a complex128 transform).
    ``want_range_stats`` (fft form and CW): f64 device tensor {nanmin, nanmax, NaN count} of the echo_range as a by-product
    of the same pass -- with ``want_range=False`` of the array range_complex would write.
    ``replica_id`` (C, P) int32: one replica per (channel, filter interval) instead of one per channel
    (``replica_off`` then has one entry per replica + 1); -1 = a ping no interval covers (NaN coefficient row)."""
    C, P, S, B = re.shape
    n_rep = C if replica_id is None else int(replica_off.numel()) - 1
    if replica_id is not None and (replica is None or tuple(replica_id.shape) != (C, P) or replica_id.dtype != torch.int32):
        raise ValueError("replica_id: int32 (C, P) next to replica / replica_off")
    if re.dtype != im.dtype or re.dtype not in _DT:
        raise ValueError("backscatter_r / backscatter_i must both be float32 or float64")
    if method not in ("auto", "direct", "fft"):
        raise ValueError("method must be 'auto', 'direct' or 'fft'")
    dev = re.device
    out = torch.empty((C, P, S), dtype=dtype, device=dev)
    rng = torch.empty((C, P, S), dtype=dtype, device=dev) if want_range else None
    prx = torch.empty((C, P, S), dtype=dtype, device=dev) if want_prx else None
    cal = _lib.CAL_SV if cal_type == "Sv" else _lib.CAL_TS
    use_fft = sv_complex_uses_fft(replica, max_taps, method)
    stats = None
    if use_fft:
        ws = _scratch("sv_complex_fft.workspace", dev, max(C, n_rep), P, S)
        fdt = torch_dtype(fft_dtype) if fft_dtype is not None else dtype
        if want_range_stats:
            stats = torch.empty(3, dtype=torch.float64, device=dev)
        if replica_id is None:
            call("epa_sv_complex_fft", _p(re), _p(im), _DT[re.dtype], _p(replica), _p(replica_off), int(max_taps),
                 _p(ccoef), C, P, S, B, cal, _p(out), _p(rng), _p(prx), _DT[dtype], _DT[fdt], _p(ws), _p(stats),
                 _stream())
        else:
            call("epa_sv_complex_fft_indexed", _p(re), _p(im), _DT[re.dtype], _p(replica), _p(replica_off),
                 _p(replica_id), n_rep, int(max_taps), _p(ccoef), C, P, S, B, cal, _p(out), _p(rng), _p(prx),
                 _DT[dtype], _DT[fdt], _p(ws), _p(stats), _stream())
    elif replica is None and want_range_stats:  # CW: the streaming kernel leaves the statistics as well
        ws = _scratch("sv_complex_cw_stats.workspace", dev)
        stats = torch.empty(3, dtype=torch.float64, device=dev)
        call("epa_sv_complex_cw_stats", _p(re), _p(im), _DT[re.dtype], _p(ccoef), C, P, S, B, cal, _p(out), _p(rng),
             _p(prx), _DT[dtype], _p(ws), _p(stats), _stream())
    elif replica_id is not None:
        call("epa_sv_complex_indexed", _p(re), _p(im), _DT[re.dtype], _p(replica), _p(replica_off), _p(replica_id), n_rep,
             int(max_taps), _p(ccoef), C, P, S, B, cal, _p(out), _p(rng), _p(prx), _DT[dtype], _stream())
    else:
        call("epa_sv_complex", _p(re), _p(im), _DT[re.dtype], _p(replica), _p(replica_off), int(max_taps),
             _p(ccoef), C, P, S, B, cal, _p(out), _p(rng), _p(prx), _DT[dtype], _stream())
    return dict(out=out, echo_range=rng, prx=prx, range_stats=stats)


# ---- split-beam angles (consolidate.add_splitbeam_angle) ---------------------------------------------------------------
SPLITBEAM_PARAMS = ("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship",
                    "angle_offset_athwartship")
SPLITBEAM_BEAM_TYPES = (1, 17, 49, 65, 81)


def _angle_params(params, C, P):
    """The four angle parameters (f64 device tensors of shape (), (C,) or (C, P), in SPLITBEAM_PARAMS order) as the C
    ABI takes them: a host array of device pointers, one of epa_param_mode, and the tensors to keep alive."""
    if len(params) != 4:
        raise ValueError("four angle parameters: sensitivity along / athwart, offset along / athwart")
    keep = [t.to(torch.float64).contiguous() for t in params]
    ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in keep])
    modes = (ctypes.c_int * 4)(*[_mode_of(t, C, P) for t in keep])
    for t in keep:
        _p(t)  # (device and contiguous)
    return ptrs, modes, keep


def splitbeam_power(along, athw, params, *, dtype=torch.float64):
    """Split-beam angles of power/angle samples -> (theta, phi) (C, P, S).  ``along`` / ``athw``: the electrical angle
    planes, int8 steps as a file stores them or float32 / float64 (NaN padding stays NaN); ``params`` as
    _angle_params."""
    C, P, S = along.shape
    if athw.shape != along.shape or athw.dtype != along.dtype:
        raise ValueError("angle_alongship / angle_athwartship: same shape and dtype")
    codes = {torch.int8: _lib.I8, torch.float32: _lib.F32, torch.float64: _lib.F64}
    if along.dtype not in codes:
        raise ValueError(f"angle planes must be int8, float32 or float64 (got {along.dtype})")
    ptrs, modes, keep = _angle_params(params, C, P)
    theta = torch.empty((C, P, S), dtype=dtype, device=along.device)
    phi = torch.empty_like(theta)
    call("epa_splitbeam_power", _p(along), _p(athw), codes[along.dtype], ptrs, modes, C, P, S, _p(theta), _p(phi),
         _DT[dtype], _stream())
    return theta, phi


def splitbeam_uses_fft(replica, max_taps, method="auto"):
    """The form splitbeam_complex picks: the rule of sv_complex_uses_fft."""
    return sv_complex_uses_fft(replica, max_taps, method)


def splitbeam_complex(re, im, beam_type, params, *, replica=None, replica_off=None, max_taps=0, replica_id=None,
                      dtype=torch.float64, method="auto", fft_dtype=None):
    """Split-beam angles of complex samples -> (theta, phi) (C, P, S).  ``re`` / ``im`` (C, P, S, B), B = 3 or 4;
    ``beam_type``: host sequence of C ints (1, 17, 49, 65, 81; -1 = skip the channel: NaN rows).  With ``replica`` /
    ``replica_off`` (as sv_complex, ``replica_id`` too) the sector combinations are pulse-compressed first: "direct",
    "fft" or "auto" (fft for replicas of 16 .. 1024 taps).  ``fft_dtype``: arithmetic of the transform, default
    float64 whatever ``dtype`` is -- a phase needs the weak samples right, and complex64 butterflies err by ~3e-7 of
    the tile's strongest echo (~1e-2 deg at 1e-3 of a ping's RMS); float32 on request."""
    C, P, S, B = re.shape
    if re.dtype != im.dtype or re.dtype not in _DT or im.shape != re.shape:
        raise ValueError("backscatter_r / backscatter_i must both be float32 or float64 of one shape")
    if method not in ("auto", "direct", "fft"):
        raise ValueError("method must be 'auto', 'direct' or 'fft'")
    bt = np.ascontiguousarray(np.asarray(beam_type, dtype=np.int32).reshape(-1))
    if bt.size != C:
        raise ValueError(f"beam_type: {C} values expected, got {bt.size}")
    if replica_id is not None and (replica is None or tuple(replica_id.shape) != (C, P) or replica_id.dtype != torch.int32):
        raise ValueError("replica_id: int32 (C, P) next to replica / replica_off")
    n_rep = 0 if replica is None else (C if replica_id is None else int(replica_off.numel()) - 1)
    ptrs, modes, keep = _angle_params(params, C, P)
    dev = re.device
    theta = torch.empty((C, P, S), dtype=dtype, device=dev)
    phi = torch.empty_like(theta)
    bt_p = bt.ctypes.data_as(ctypes.c_void_p)
    if splitbeam_uses_fft(replica, max_taps, method):
        ws = _scratch("splitbeam_complex_fft.workspace", dev, n_rep)
        fdt = torch_dtype(fft_dtype) if fft_dtype is not None else torch.float64
        call("epa_splitbeam_complex_fft", _p(re), _p(im), _DT[re.dtype], bt_p, ptrs, modes, _p(replica),
             _p(replica_off), _p(replica_id), n_rep, int(max_taps), C, P, S, B, _p(theta), _p(phi), _DT[dtype],
             _DT[fdt], _p(ws), _stream())
    else:
        call("epa_splitbeam_complex", _p(re), _p(im), _DT[re.dtype], bt_p, ptrs, modes, _p(replica), _p(replica_off),
             _p(replica_id), n_rep, int(max_taps), C, P, S, B, _p(theta), _p(phi), _DT[dtype], _stream())
    return theta, phi

# ---- seafloor detection (mask.detect_seafloor) ------------------------------------------------------------------------
def _plane_dtype(t, what):
    if t.dim() != 2 or t.dtype not in _DT:
        raise ValueError(f"{what}: a (ping_time, range_sample) float32 / float64 plane expected, got {tuple(t.shape)} "
                         f"{t.dtype}")
    return _DT[t.dtype]


def seafloor_state(device):
    """The zeroed u64 state words of one Blackwell call (int64 tensor of EPA_SEAFLOOR_STATE_WORDS)."""
    return _scratch("seafloor.state", device, dtype=torch.int64, zero=True)


def seafloor_depth_uniform(depth):
    """-> int32 device tensor (1,): the pings of ``depth`` (P, S) whose grid differs from ping 0 (utils._check_inputs)."""
    bad = torch.zeros(1, dtype=torch.int32, device=depth.device)
    P, S = depth.shape
    call("epa_seafloor_depth_uniform", _p(depth), _plane_dtype(depth, "depth"), P, S, _p(bad), _stream())
    return bad


def seafloor_basic(sv, skip, tmin, tmax, depth0, offset):
    """bottom_basic on one channel: ``sv`` (P, S), ``depth0`` f64 (S,) -> f64 (P,) bottom depths."""
    P, S = sv.shape
    out = torch.empty(P, dtype=torch.float64, device=sv.device)
    call("epa_seafloor_basic", _p(sv), _plane_dtype(sv, "Sv"), P, S, int(skip), float(tmin), float(tmax),
         _p(depth0), float(offset), _p(out), _stream())
    return out


def seafloor_angle_mask(theta, phi, r0, R, wtheta, wphi, ttheta, tphi, state):
    """The Blackwell angle mask of the crop [r0, r0 + R) -> u8 (P, R); adds the masked count to ``state[0]``."""
    P, S = theta.shape
    if phi.shape != theta.shape or phi.dtype != theta.dtype:
        raise ValueError("angle_alongship / angle_athwartship: same shape and dtype")
    work = _scratch("seafloor_angle_mask.work", theta.device, P, R)
    mask = torch.empty((P, R), dtype=torch.uint8, device=theta.device)
    call("epa_seafloor_angle_mask", _p(theta), _p(phi), _plane_dtype(theta, "angles"), P, S, int(r0), int(R),
         int(wtheta), int(wphi), float(ttheta), float(tphi), _p(work), _p(mask), _p(state), _stream())
    return mask


def seafloor_median(sv, r0, R, mask, state):
    """Radix-select the one or two middle values of the non-NaN ``sv`` crop under ``mask`` into ``state``."""
    P, S = sv.shape
    hist = _scratch("seafloor_median.hist", sv.device, dtype=torch.int64)
    call("epa_seafloor_median", _p(sv), _plane_dtype(sv, "Sv"), P, S, int(r0), int(R), _p(mask), _p(state), _p(hist),
         _stream())


def seafloor_components(sv, r0, R, threshold, mask, state):
    """8-connected components of the ``sv`` crop above ``threshold``; marks the roots of those meeting the angle mask
    (bit 1 of ``mask``) -> int64 (P, R) roots, -1 for background."""
    P, S = sv.shape
    parent = torch.empty((P, R), dtype=torch.int64, device=sv.device)
    call("epa_seafloor_components", _p(sv), _plane_dtype(sv, "Sv"), P, S, int(r0), int(R), float(threshold),
         _p(mask), _p(parent), _p(state), _stream())
    return parent


def seafloor_bottom(parent, mask, P, r0, depth0, offset, dtype):
    """Per ping: depth0 of the first kept crop sample minus ``offset`` (depth0[0] - offset without one; ``parent`` None:
    nothing is kept) -> (P,) of ``dtype``."""
    out = torch.empty(P, dtype=dtype, device=depth0.device)
    R = 0 if parent is None else parent.shape[1]
    call("epa_seafloor_bottom", _p(parent), _p(mask), P, R, int(r0), _p(depth0), float(offset), _p(out), _DT[dtype],
         _stream())
    return out


# ---- shoal detection (mask.detect_shoal) -----------------------------------------------------------------------------
def shoal_table_capacity(P, S, connectivity):
    """The most components a (P, S) plane can hold (the size of the component table of the shoal detectors)."""
    return (P * S + 1) // 2 if connectivity == 4 else ((P + 1) // 2) * ((S + 1) // 2)


def shoal_state(device):
    """The zeroed u64 state words of one shoal call (int64 tensor of EPA_SHOAL_STATE_WORDS): [0] the error word."""
    return _scratch("shoal.state", device, dtype=torch.int64, zero=True)


def _gap(v, n):
    """A gap length as given (``run <= v`` for an integer run) -> the integer the kernels compare with."""
    v = float(v)
    return 0 if not v >= 0 else int(min(np.floor(v), n))


def shoal_threshold_fill(sv, thr, maxvgap=0, maxhgap=0):
    """``sv > thr`` on a (P, S) plane, background runs of at most ``maxvgap`` samples (then ``maxhgap`` pings) between
    foreground filled -> bool (P, S)."""
    dt = _plane_dtype(sv, "Sv")
    P, S = sv.shape
    plane = torch.empty((P, S), dtype=torch.bool, device=sv.device)
    call("epa_shoal_threshold_fill", _p(sv), dt, P, S, float(thr), _gap(maxvgap, S),
         _gap(maxhgap, P), _p(plane), _stream())
    return plane


def shoal_label(plane, connectivity, state, with_groups=False):
    """Connected components of a bool (P, S) plane -> (parent int64 (P, S): -(id + 2) on component id, -1 on
    background; table: dict of the int32 tensors ``box`` (4, cap), ``flag`` (cap) and, ``with_groups``, ``group``
    (cap))."""
    P, S = plane.shape
    cap = shoal_table_capacity(P, S, connectivity)
    dev = plane.device
    parent = torch.empty((P, S), dtype=torch.int64, device=dev)
    table = {"box": torch.empty((4, cap), dtype=torch.int32, device=dev),
             "flag": torch.empty(cap, dtype=torch.int32, device=dev), "cap": cap}
    if with_groups:
        table["group"] = torch.empty(cap, dtype=torch.int32, device=dev)
    call("epa_shoal_label", _p(plane), P, S, int(connectivity), _p(parent), _p(table["box"]), _p(table["flag"]), cap,
         _p(state), _stream())
    return parent, table


def shoal_weill_filter(plane, parent, table, minvlen, minhlen, state):
    """In place: ``plane`` keeps the components whose extents are not below ``minvlen`` samples / ``minhlen`` pings."""
    P, S = plane.shape
    call("epa_shoal_weill_filter", _p(parent), P, S, _p(table["box"]), _p(table["flag"]), table["cap"],
         float(minvlen), float(minhlen), _p(state), _p(plane), _stream())
    return plane


def shoal_echoview_link(plane, parent, table, idim, jdim, mincan, maxlink, minsho, state):
    """In place: Echoview's candidate filter, linking and shoal filter on a labelled plane; ``idim`` / ``jdim`` f64
    device vectors."""
    P, S = plane.shape
    queue = _scratch("shoal_echoview_link.queue", plane.device, dtype=torch.int32)
    call("epa_shoal_echoview_link", _p(parent), P, S, _p(table["box"]), _p(table["group"]), _p(table["flag"]),
         table["cap"], _p(idim), int(idim.numel()), _p(jdim), int(jdim.numel()), float(mincan[0]), float(mincan[1]),
         float(maxlink[0]), float(maxlink[1]), float(minsho[0]), float(minsho[1]), _p(queue), _p(state), _p(plane),
         _stream())
    return plane


# ---- region tables (mask.label_regions, mask.region_statistics) --------------------------------------------------------
def region_stats(code, n, state, sv=None, range=None):
    """One sweep over the code plane ``code`` (P, S) of ``shoal_label`` with ``n`` components, and over ``sv``
    (C, P, S) with its ``range`` (same float type, (C, P, S) or broadcasting to it: read through its strides, samples
    adjacent) -> (``stats`` int64 (C, n, 11), ``ids`` int64 (n, 2)), the zero-initialised tables of ``epa_region_stats``;
    ``region_tables`` names their words.  ``sv`` None: ``ids`` alone (``stats`` has C = 0).  A code that names no id
    below ``n`` counts into ``state[0]``."""
    P, S = code.shape
    n = int(n)
    dev = code.device
    if code.dtype != torch.int64:
        raise ValueError(f"region_stats: the code plane of shoal_label (int64) expected, got {code.dtype}")
    if sv is None:
        C, dt, sv_p, r_p, rs_c, rs_p = 0, _lib.F64, None, None, 0, 0
    else:
        if sv.dim() != 3 or tuple(sv.shape[1:]) != (P, S) or sv.dtype not in _DT:
            raise ValueError(f"region_stats: sv must be float32 / float64 of shape (C, {P}, {S}), got {sv.dtype} "
                             f"{tuple(sv.shape)}")
        if range is None or range.dtype != sv.dtype or not range.is_cuda:
            raise ValueError("region_stats: range must be a device tensor of sv's type")
        C = sv.shape[0]
        try:
            rv = range.expand(C, P, S)
        except RuntimeError:
            raise ValueError(f"region_stats: range of shape {tuple(range.shape)} does not broadcast to {(C, P, S)}") from None
        if S > 1 and rv.stride(2) != 1:  # (samples apart, or no sample axis: the one case copied)
            rv = rv.contiguous()
        dt, sv_p, r_p = _DT[sv.dtype], _p(sv), ctypes.c_void_p(rv.data_ptr())
        rs_c, rs_p = (rv.stride(0) if C > 1 else 0), (rv.stride(1) if P > 1 else 0)
    stats = torch.zeros((C, n, _lib.REGION_WORDS), dtype=torch.int64, device=dev)
    ids = torch.zeros((n, _lib.REGION_ID_WORDS), dtype=torch.int64, device=dev)
    call("epa_region_stats", _p(code), P, S, sv_p, r_p, dt, C, rs_c, rs_p, n, _p(stats) if C else None, _p(ids),
         _p(state), _stream())
    return stats, ids


def _unkey(k):
    """The float64 values of order-preserving u64 keys (``epa_region_word``); key 0 (nothing seen) -> NaN.  The host
    mirror of ``epa::key_value`` and ``epa::kKeyNoMax``: csrc/ordered_key.h is the definition and states the contract."""
    k = np.ascontiguousarray(k).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    bits = np.where(k & top, k & ~top, ~k)
    return np.where(k == 0, np.nan, bits.view(np.float64))


def region_tables(stats, ids, n_pix):
    """The downloaded tables of ``region_stats`` (int64 NumPy arrays (C, n, 11) and (n, 2)) by name -> dict: the
    int64 counts ``n_valid`` / ``n_range`` (C, n) and ``n_samples`` (n,), ``first`` (n,) the smallest linear pixel
    index, the float64 extrema ``sv_max`` / ``range_min`` / ``range_max`` (NaN: none seen) and the float64 raw sums
    ``sum_*`` (C, n)."""
    stats, ids = np.ascontiguousarray(stats), np.ascontiguousarray(ids)
    out = {"n_samples": ids[:, _lib.REGION_ID_SAMPLES].copy(), "first": int(n_pix) - ids[:, _lib.REGION_ID_FIRST]}
    for j, name in enumerate(_lib.REGION_FIELDS):
        w = np.ascontiguousarray(stats[:, :, j])
        if name.startswith("n_"):
            out[name] = w
        elif name.startswith("sum_"):
            out[name] = w.view(np.float64)
        else:
            out[name] = _unkey(w)
    out["range_min"] = -out["range_min"]
    return out


def region_labels(code, rank):
    """int32 (P, S): ``rank[id]`` on the pixels of component id of the code plane ``code``, 0 on background."""
    P, S = code.shape
    if rank.dtype != torch.int32 or rank.dim() != 1 or rank.numel() == 0:
        raise ValueError(f"region_labels: rank must be a non-empty int32 vector, got {rank.dtype} {tuple(rank.shape)}")
    labels = torch.empty((P, S), dtype=torch.int32, device=code.device)
    call("epa_region_labels", _p(code), P, S, _p(rank), rank.numel(), _p(labels), _stream())
    return labels


# ---- single targets, split beam (targets.detect_single_targets) -------------------------------------------------------
SINGLE_TARGET_TILE = _lib.SINGLE_TARGET_TILE  # samples of a row a workgroup holds at a time (EPA_SINGLE_TARGET_TILE)


def _single_target_args(who, ts, along, athw, range, prm, limits):
    """The arguments the two single-target entries share, checked: -> (tuple of C arguments, keep-alive list)."""
    if ts.dim() != 3 or ts.dtype not in _DT:
        raise ValueError(f"{who}: TS must be float32 / float64 of shape (C, P, S), got {ts.dtype} {tuple(ts.shape)}")
    C, P, S = ts.shape
    for name, t in (("angle_alongship", along), ("angle_athwartship", athw)):
        if t.dtype != ts.dtype or tuple(t.shape) != (C, P, S):
            raise ValueError(f"{who}: {name} must be {ts.dtype} of shape {(C, P, S)}, got {t.dtype} {tuple(t.shape)}")
    if range.dtype != ts.dtype or not range.is_cuda:
        raise ValueError(f"{who}: range must be a device tensor of TS's type")
    try:
        rv = range.expand(C, P, S)
    except RuntimeError:
        raise ValueError(f"{who}: range of shape {tuple(range.shape)} does not broadcast to {(C, P, S)}") from None
    if S > 1 and rv.stride(2) != 1:  # (samples apart, or no sample axis: the one case copied)
        rv = rv.contiguous()
    rs_c, rs_p = (rv.stride(0) if C > 1 else 0), (rv.stride(1) if P > 1 else 0)
    if prm.dtype != torch.float64 or tuple(prm.shape) != (5, C, P):
        raise ValueError(f"{who}: prm must be float64 of shape {(5, C, P)}, got {prm.dtype} {tuple(prm.shape)}")
    lim = np.ascontiguousarray(limits, dtype=np.float64)
    if lim.shape != (len(_lib.SINGLE_TARGET_LIMITS),):
        raise ValueError(f"{who}: {len(_lib.SINGLE_TARGET_LIMITS)} limits expected, got an array of shape {lim.shape}")
    args = (_p(ts), _p(along), _p(athw), ctypes.c_void_p(rv.data_ptr()), _DT[ts.dtype], C, P, S, rs_c, rs_p, _p(prm),
            lim.ctypes.data_as(ctypes.c_void_p))
    return args, (rv, lim)


def single_target_count(ts, along, athw, range, prm, limits):
    """The count pass of the single-target detection over a (C, P, S) cube ``ts`` with its angle cubes (same type and
    shape), its ``range`` ((C, P, S) or broadcasting to it: read through its strides, samples adjacent), ``prm`` f64
    (5, C, P) = samples per pulse, the two beamwidths, the two angle offsets, and the seven host ``limits`` in the
    order of ``_lib.SINGLE_TARGET_LIMITS`` -> (``n_targets`` int32 (C, P), ``n_candidates`` int64 (C,),
    ``n_rejected`` int64 (C, 4))."""
    args, keep = _single_target_args("single_target_count", ts, along, athw, range, prm, limits)
    C, P, _ = ts.shape
    dev = ts.device
    n_targets = torch.empty((C, P), dtype=torch.int32, device=dev)
    n_cand = torch.zeros(C, dtype=torch.int64, device=dev)
    n_rej = torch.zeros((C, 4), dtype=torch.int64, device=dev)
    call("epa_single_target_count", *args, _p(n_targets), _p(n_cand), _p(n_rej), _stream())
    del keep
    return n_targets, n_cand, n_rej


def single_target_emit(ts, along, athw, range, prm, limits, n_targets, offsets, n):
    """The emit pass: the inputs of ``single_target_count``, the ``n_targets`` it left, ``offsets`` int64 (C, P) their
    exclusive scan and ``n`` their sum -> (int32 (5, n), float64 (9, n)): the columns ``_lib.SINGLE_TARGET_ICOL_NAMES`` and
    ``_lib.SINGLE_TARGET_FCOL_NAMES``, ordered by (channel, ping, sample)."""
    args, keep = _single_target_args("single_target_emit", ts, along, athw, range, prm, limits)
    C, P, _ = ts.shape
    n = int(n)
    if n_targets.dtype != torch.int32 or tuple(n_targets.shape) != (C, P) or offsets.dtype != torch.int64 or \
            tuple(offsets.shape) != (C, P) or n <= 0:
        raise ValueError(f"single_target_emit: n_targets int32 and offsets int64 of shape {(C, P)} and n > 0 expected")
    icols = torch.empty((_lib.SINGLE_TARGET_ICOLS, n), dtype=torch.int32, device=ts.device)
    fcols = torch.empty((_lib.SINGLE_TARGET_FCOLS, n), dtype=torch.float64, device=ts.device)
    call("epa_single_target_emit", *args, _p(n_targets), _p(offsets), n, _p(icols), _p(fcols), _stream())
    del keep
    return icols, fcols


# ---- target strength spectra (targets.target_spectra) -----------------------------------------------------------------
def target_spectra(re, im, replica, replica_off, max_taps, rep_dt, fparams, pparams, half_window, chan_map, channel_index,
                   ping_index, range_sample, target_range, angle_alongship, angle_athwartship, *, replica_id=None,
                   dtype="float64"):
    """TS(f) of the rows of a single-target table (``epa_target_spectra``; targets/spectra.py states the rules).

    ``re``, ``im``: the sector samples (C, P, S, B), float32 or float64.  ``replica``: float32 (2 * n,) interleaved
    (re, im) of all replicas end to end; ``replica_off`` int32 (R + 1,); ``max_taps`` the most taps of one (at most
    ``_lib.TARGET_SPECTRA_MAX_TAPS``); ``replica_id`` int32 (C, P) or None (replica c for channel c).  ``rep_dt``
    float64 (R,): the sample interval of a replica's pings.  ``fparams`` float64 (R, 8, F) in the order of
    ``_lib.TARGET_SPECTRA_FPARAM_NAMES``; ``pparams`` float64 (3, C, P) in the order of
    ``_lib.TARGET_SPECTRA_PPARAM_NAMES``.  ``chan_map`` int32 (n,): the channel of the cubes behind every channel of the
    table.  The columns: int32 ``channel_index``, ``ping_index``, ``range_sample`` and float64 ``target_range``,
    ``angle_alongship``, ``angle_athwartship``, (N,) each.
    -> (``TS_spectrum`` (N, F), ``TS_spectrum_uncomp`` (N, F) of ``dtype``, ``n_window_samples`` int32 (N,)).  No rows:
    nothing is launched."""
    who = "target_spectra"
    td = torch_dtype(dtype)
    if re.dim() != 4 or re.dtype not in _DT or im.dtype != re.dtype or im.shape != re.shape:
        raise ValueError(f"{who}: re and im must be float32 / float64 of one shape (C, P, S, B), got {re.dtype} "
                         f"{tuple(re.shape)} and {im.dtype} {tuple(im.shape)}")
    C, P, S, B = re.shape
    max_taps, h = int(max_taps), int(half_window)
    if not 1 <= max_taps <= _lib.TARGET_SPECTRA_MAX_TAPS:
        raise ValueError(f"{who}: replicas of up to {_lib.TARGET_SPECTRA_MAX_TAPS} taps are served, got max_taps {max_taps}")
    if not 0 <= h <= _lib.TARGET_SPECTRA_MAX_HALF_WINDOW:
        raise ValueError(f"{who}: half_window {h} outside 0 .. {_lib.TARGET_SPECTRA_MAX_HALF_WINDOW}")
    if replica.dtype != torch.float32 or replica.dim() != 1 or replica.numel() % 2 or replica_off.dtype != torch.int32 \
            or replica_off.dim() != 1 or replica_off.numel() < 2:
        raise ValueError(f"{who}: replica float32 (2 n,) and replica_off int32 (R + 1,) expected")
    R = replica_off.numel() - 1
    if replica_id is not None and (replica_id.dtype != torch.int32 or tuple(replica_id.shape) != (C, P)):
        raise ValueError(f"{who}: replica_id must be int32 of shape {(C, P)}")
    if replica_id is None and R < C:
        raise ValueError(f"{who}: without replica_id every channel needs its replica ({R} replicas, {C} channels)")
    if fparams.dtype != torch.float64 or fparams.dim() != 3 or fparams.shape[:2] != (R, _lib.TARGET_SPECTRA_FPARAMS):
        raise ValueError(f"{who}: fparams must be float64 of shape ({R}, {_lib.TARGET_SPECTRA_FPARAMS}, F), got "
                         f"{fparams.dtype} {tuple(fparams.shape)}")
    F = fparams.shape[2]
    if not 1 <= F <= _lib.TARGET_SPECTRA_MAX_FREQ:
        raise ValueError(f"{who}: {F} frequencies outside 1 .. {_lib.TARGET_SPECTRA_MAX_FREQ}")
    if rep_dt.dtype != torch.float64 or tuple(rep_dt.shape) != (R,):
        raise ValueError(f"{who}: rep_dt must be float64 of shape ({R},)")
    if pparams.dtype != torch.float64 or tuple(pparams.shape) != (_lib.TARGET_SPECTRA_PPARAMS, C, P):
        raise ValueError(f"{who}: pparams must be float64 of shape {(_lib.TARGET_SPECTRA_PPARAMS, C, P)}")
    if chan_map.dtype != torch.int32 or chan_map.dim() != 1 or chan_map.numel() < 1:
        raise ValueError(f"{who}: chan_map must be int32 (n,), n >= 1")
    N = channel_index.numel()
    for name, t, want in (("channel_index", channel_index, torch.int32), ("ping_index", ping_index, torch.int32),
                          ("range_sample", range_sample, torch.int32), ("target_range", target_range, torch.float64),
                          ("angle_alongship", angle_alongship, torch.float64),
                          ("angle_athwartship", angle_athwartship, torch.float64)):
        if t.dtype != want or tuple(t.shape) != (N,):
            raise ValueError(f"{who}: {name} must be {want} of shape ({N},), got {t.dtype} {tuple(t.shape)}")
    dev = re.device
    ts = torch.empty((N, F), dtype=td, device=dev)
    ts_uncomp = torch.empty((N, F), dtype=td, device=dev)
    n_window = torch.empty(N, dtype=torch.int32, device=dev)
    if N == 0:
        return ts, ts_uncomp, n_window
    table = _scratch("target_spectra.table", dev, R, F)
    call("epa_target_spectra", _p(re), _p(im), _DT[re.dtype], C, P, S, B, _p(replica), _p(replica_off), _p(replica_id), R,
         replica.numel() // 2, max_taps, _p(rep_dt), _p(fparams), F, h, _p(pparams), _p(chan_map), chan_map.numel(),
         _p(channel_index), _p(ping_index), _p(range_sample), _p(target_range), _p(angle_alongship),
         _p(angle_athwartship), N, _p(table), _p(ts), _p(ts_uncomp), _DT[td], _p(n_window), _stream())
    return ts, ts_uncomp, n_window


# ---- volume backscattering spectra (calibrate.compute_Sv_spectrum) -------------------------------------------------------
def sv_spectrum_cells(S, window_samples, step_samples):
    """The cells of a ping of ``S`` samples: ``floor((S - window_samples) / step_samples) + 1``."""
    return (int(S) - int(window_samples)) // int(step_samples) + 1


def sv_spectrum_plan(max_taps, window_samples, step_samples, M):
    """The tile ``epa_sv_spectrum`` takes -> (cells of a tile, tiles of a ping, bytes of LDS of a workgroup)."""
    t, n, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    call("epa_sv_spectrum_plan", int(max_taps), int(window_samples), int(step_samples), int(M), ctypes.byref(t),
         ctypes.byref(n), ctypes.byref(b))
    return t.value, n.value, b.value


def sv_spectrum(re, im, replica, replica_off, max_taps, rep_dt, fparams, pparams, window, step_samples, *, replica_id=None,
                dtype="float64", out=None):
    """Sv(f) of the range cells of every ping (``epa_sv_spectrum``; calibrate/sv_spectrum.py states the rules).

    ``re``, ``im``, ``replica``, ``replica_off``, ``max_taps``, ``replica_id``, ``rep_dt``: as for ``target_spectra``
    (``max_taps`` at most ``_lib.SV_SPECTRUM_MAX_TAPS``).  ``fparams`` float64 (R, 5, F) in the order of
    ``_lib.SV_SPECTRUM_FPARAM_NAMES``; ``pparams`` float64 (4, C, P) in the order of ``_lib.SV_SPECTRUM_PPARAM_NAMES``.
    ``window`` float64 (N_w,): the normalised window; ``step_samples``: the hop.  ``out``: optionally the two results to
    write into.  -> (``Sv_spectrum`` (C, P, M, F) of ``dtype``, ``echo_range`` float64 (C, P, M)), M =
    ``sv_spectrum_cells(S, N_w, hop)``."""
    who = "sv_spectrum"
    td = torch_dtype(dtype)
    if re.dim() != 4 or re.dtype not in _DT or im.dtype != re.dtype or im.shape != re.shape:
        raise ValueError(f"{who}: re and im must be float32 / float64 of one shape (C, P, S, B), got {re.dtype} "
                         f"{tuple(re.shape)} and {im.dtype} {tuple(im.shape)}")
    C, P, S, B = re.shape
    max_taps, hop = int(max_taps), int(step_samples)
    if not 1 <= max_taps <= _lib.SV_SPECTRUM_MAX_TAPS:
        raise ValueError(f"{who}: replicas of up to {_lib.SV_SPECTRUM_MAX_TAPS} taps are served, got max_taps {max_taps}")
    if window.dtype != torch.float64 or window.dim() != 1 or not 2 <= window.numel() <= _lib.SV_SPECTRUM_MAX_WINDOW:
        raise ValueError(f"{who}: window must be float64 of 2 .. {_lib.SV_SPECTRUM_MAX_WINDOW} samples, got {window.dtype} "
                         f"{tuple(window.shape)}")
    Nw = window.numel()
    if not 1 <= hop < 2 ** 31 - 1:
        raise ValueError(f"{who}: step_samples {hop} outside 1 .. 2**31 - 2")
    if S < Nw:
        raise ValueError(f"{who}: a window of {Nw} samples on pings of {S}")
    if replica.dtype != torch.float32 or replica.dim() != 1 or replica.numel() % 2 or replica_off.dtype != torch.int32 \
            or replica_off.dim() != 1 or replica_off.numel() < 2:
        raise ValueError(f"{who}: replica float32 (2 n,) and replica_off int32 (R + 1,) expected")
    R = replica_off.numel() - 1
    if replica_id is not None and (replica_id.dtype != torch.int32 or tuple(replica_id.shape) != (C, P)):
        raise ValueError(f"{who}: replica_id must be int32 of shape {(C, P)}")
    if replica_id is None and R < C:
        raise ValueError(f"{who}: without replica_id every channel needs its replica ({R} replicas, {C} channels)")
    if fparams.dtype != torch.float64 or fparams.dim() != 3 or fparams.shape[:2] != (R, _lib.SV_SPECTRUM_FPARAMS):
        raise ValueError(f"{who}: fparams must be float64 of shape ({R}, {_lib.SV_SPECTRUM_FPARAMS}, F), got "
                         f"{fparams.dtype} {tuple(fparams.shape)}")
    F = fparams.shape[2]
    if not 1 <= F <= _lib.SV_SPECTRUM_MAX_FREQ:
        raise ValueError(f"{who}: {F} frequencies outside 1 .. {_lib.SV_SPECTRUM_MAX_FREQ}")
    if rep_dt.dtype != torch.float64 or tuple(rep_dt.shape) != (R,):
        raise ValueError(f"{who}: rep_dt must be float64 of shape ({R},)")
    if pparams.dtype != torch.float64 or tuple(pparams.shape) != (_lib.SV_SPECTRUM_PPARAMS, C, P):
        raise ValueError(f"{who}: pparams must be float64 of shape {(_lib.SV_SPECTRUM_PPARAMS, C, P)}")
    M = sv_spectrum_cells(S, Nw, hop)
    dev = re.device
    if out is None:
        sv = torch.empty((C, P, M, F), dtype=td, device=dev)
        rng = torch.empty((C, P, M), dtype=torch.float64, device=dev)
    else:
        sv, rng = out
        if sv.dtype != td or tuple(sv.shape) != (C, P, M, F) or rng.dtype != torch.float64 or tuple(rng.shape) != (C, P, M):
            raise ValueError(f"{who}: out must be ({td} {(C, P, M, F)}, float64 {(C, P, M)})")
    table = _scratch("sv_spectrum.table", dev, R, F)
    call("epa_sv_spectrum", _p(re), _p(im), _DT[re.dtype], C, P, S, B, _p(replica), _p(replica_off), _p(replica_id), R,
         replica.numel() // 2, max_taps, _p(rep_dt), _p(fparams), F, _p(pparams), _p(window), Nw, hop, M, _p(table), _p(sv),
         _DT[td], _p(rng), _stream())
    return sv, rng


# ---- target tracking (targets.track_targets) --------------------------------------------------------------------------
TRACK_TILE = _lib.TRACK_TILE  # rows of a run a workgroup of propose / accept stages in LDS at a time (EPA_TRACK_TILE)


def _track_params(params):
    prm = np.ascontiguousarray(params, dtype=np.float64)
    if prm.shape != (len(_lib.TRACK_PARAM_NAMES),):
        raise ValueError(f"track: {len(_lib.TRACK_PARAM_NAMES)} params expected, got an array of shape {prm.shape}")
    return prm


def _track_columns(who, n, **cols):
    for name, (t, dtype) in cols.items():
        if t.dtype != dtype or t.shape[-1] != n or not t.is_cuda:
            raise ValueError(f"{who}: {name} must be a device tensor of {dtype} with {n} rows, got {t.dtype} "
                             f"{tuple(t.shape)}")


def track_prepare(channel_index, ping_index, range, along, athw, C, P):
    """The first pass of the tracking over a table of n rows (int32 index columns, float64 ``range`` and angles) ->
    (``seg`` int32 (C * P + 1,): the first row of every (channel, ping) segment, ``xyz`` float64 (3, n), ``succ`` and
    ``pred`` int32 (n,) = -1, ``bad`` int32 (1,): 1 if the rows are not ordered by (channel, ping) or an index is outside
    [0, C) x [0, P))."""
    n = channel_index.numel()
    _track_columns("track_prepare", n, channel_index=(channel_index, torch.int32), ping_index=(ping_index, torch.int32),
                   range=(range, torch.float64), along=(along, torch.float64), athw=(athw, torch.float64))
    dev = channel_index.device
    seg = torch.empty(C * P + 1, dtype=torch.int32, device=dev)
    xyz = torch.empty((3, n), dtype=torch.float64, device=dev)
    succ = torch.empty(n, dtype=torch.int32, device=dev)
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    call("epa_track_prepare", _p(channel_index), _p(ping_index), _p(range), _p(along), _p(athw), n, C, P, _p(seg),
         _p(xyz), _p(succ), _p(pred), _p(bad), _stream())
    return seg, xyz, succ, pred, bad


def track_link_round(channel_index, ping_index, xyz, ts, C, P, seg, params, succ, pred, prop):
    """One propose / accept round, in place on ``succ`` and ``pred`` (``prop`` int32 (n,): the proposals of the round).
    ``params``: the host numbers in the order of ``_lib.TRACK_PARAM_NAMES``."""
    n = channel_index.numel()
    _track_columns("track_link_round", n, channel_index=(channel_index, torch.int32),
                   ping_index=(ping_index, torch.int32), xyz=(xyz, torch.float64), ts=(ts, torch.float64),
                   succ=(succ, torch.int32), pred=(pred, torch.int32), prop=(prop, torch.int32))
    if seg.dtype != torch.int32 or seg.numel() != C * P + 1:
        raise ValueError(f"track_link_round: seg must be int32 of {C * P + 1} entries")
    prm = _track_params(params)
    head = (_p(channel_index), _p(ping_index), _p(xyz), _p(ts), n, C, P, _p(seg), prm.ctypes.data_as(ctypes.c_void_p))
    call("epa_track_propose", *head, _p(succ), _p(pred), _p(prop), _stream())
    call("epa_track_accept", *head, _p(prop), _p(succ), _p(pred), _stream())


def track_roots(pred, passes):
    """``passes`` passes of pointer doubling over ``pred`` -> (``root``, ``rank``) int32 (n,): the first row of every
    row's chain and the row's position in it (chains of up to ``2 ** passes`` rows)."""
    n = pred.numel()
    _track_columns("track_roots", n, pred=(pred, torch.int32))
    bufs = torch.empty((4, n), dtype=torch.int32, device=pred.device)
    call("epa_track_roots", _p(pred), n, int(passes), _p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(bufs[3]), _stream())
    return (bufs[0], bufs[1]) if passes % 2 == 1 else (bufs[2], bufs[3])


def track_chains(ping_index, xyz, ts, succ, root, rank, min_targets, min_pings):
    """-> ``flag_len`` int32 (2, n): at the first row of every chain that is a track, 1 and the number of its rows."""
    n = ping_index.numel()
    _track_columns("track_chains", n, ping_index=(ping_index, torch.int32), xyz=(xyz, torch.float64),
                   ts=(ts, torch.float64), succ=(succ, torch.int32), root=(root, torch.int32), rank=(rank, torch.int32))
    flag_len = torch.zeros((2, n), dtype=torch.int32, device=ping_index.device)
    call("epa_track_chains", _p(ping_index), _p(xyz), _p(ts), _p(succ), _p(root), _p(rank), n, int(min_targets),
         int(min_pings), _p(flag_len), _stream())
    return flag_len


def track_table(channel_index, ping_index, range, ts, xyz, root, rank, flag_len, scans, T, M):
    """The track table: ``scans`` int64 (2, n) the inclusive scans of ``flag_len``'s rows, ``T >= 1`` and ``M`` their
    totals -> (``track_id`` int32 (n,), int32 (6, T), float64 (13, T)): the columns ``_lib.TRACK_ICOL_NAMES`` and
    ``_lib.TRACK_FCOL_NAMES``."""
    n = channel_index.numel()
    _track_columns("track_table", n, channel_index=(channel_index, torch.int32), ping_index=(ping_index, torch.int32),
                   range=(range, torch.float64), ts=(ts, torch.float64), xyz=(xyz, torch.float64),
                   root=(root, torch.int32), rank=(rank, torch.int32), flag_len=(flag_len, torch.int32),
                   scans=(scans, torch.int64))
    T, M = int(T), int(M)
    if not 1 <= T <= M <= n:
        raise ValueError(f"track_table: 1 <= T <= M <= n expected, got T={T} M={M} n={n}")
    dev = channel_index.device
    track_id = torch.empty(n, dtype=torch.int32, device=dev)
    order = torch.zeros(M, dtype=torch.int32, device=dev)  # (every entry is written; never a stray row number)
    start = torch.empty(T, dtype=torch.int32, device=dev)
    icols = torch.empty((len(_lib.TRACK_ICOL_NAMES), T), dtype=torch.int32, device=dev)
    fcols = torch.empty((len(_lib.TRACK_FCOL_NAMES), T), dtype=torch.float64, device=dev)
    call("epa_track_table", _p(channel_index), _p(ping_index), _p(range), _p(ts), _p(xyz), _p(root), _p(rank),
         _p(flag_len), _p(scans), n, T, M, _p(track_id), _p(order), _p(start), _p(icols), _p(fcols), _stream())
    return track_id, icols, fcols


# ---- transient-noise detectors (clean.detect_transient) --------------------------------------------------------------
def transient_fielding(sv, chan, n, thr0, thr1, maxts):
    """Fielding's transient-noise mask of a (C, P, S) cube -> bool (C, P, S), True = valid.  ``chan``: host int (C, 4)
    table of up, lw, rmin, sf per channel (``epa_transient_fielding``)."""
    C, P, S = sv.shape
    chan = np.ascontiguousarray(chan, dtype=np.int64).reshape(C, 4)
    up, lw, rmin, sf = chan.T
    if ((up < 0) | (up >= S) | (lw < 0) | (lw >= S) | (rmin < 0) | (rmin >= S) | (sf < 1)).any():
        raise ValueError(f"transient_fielding: window rows outside [0, {S}): {chan.tolist()}")
    chan[:, 3] = np.minimum(sf, 2 * S + 2)  # (a step beyond the column: no walk, a slice start below -S -- the same)
    max_rows = int(max(np.max(np.maximum(lw - up, 0)), np.max(np.where(chan[:, 3] < up, chan[:, 3], 0))))
    dev = sv.device
    mask = torch.empty((C, P, S), dtype=torch.bool, device=dev)
    todo = _scratch("transient_fielding.todo", dev, C, P, dtype=torch.int64)
    count = _scratch("transient_fielding.count", dev, dtype=torch.int32)
    call("epa_transient_fielding", _p(sv), _DT[sv.dtype], C, P, S, _p(to_device_small(chan.astype(np.int32), device=dev)),
         max_rows, int(n), float(thr0), float(thr1), float(maxts), _p(todo), _p(count), _p(mask), _stream())
    return mask


def transient_matecho(sv, range_rows, chan_i, chan_d, bottom, half_window, percentile, delta_db, extend_ping, min_window):
    """Matecho's transient-noise mask of a (C, P, S) cube -> bool (C, P, S), True = valid.  Host tables: ``range_rows``
    f64 (C, S), ``chan_i`` int (C, 2) = s_lo, s_top, ``chan_d`` f64 (C, 2) = r[1] - r[0], r[-1]; ``bottom``: f64 device
    tensor (P,) or (C, P), or None (``epa_transient_matecho``)."""
    C, P, S = sv.shape
    chan_i = np.ascontiguousarray(chan_i, dtype=np.int32).reshape(C, 2)
    if ((chan_i < 0) | (chan_i > S)).any() or (chan_i[:, 0] > chan_i[:, 1]).any():
        raise ValueError(f"transient_matecho: window rows outside [0, {S}]: {chan_i.tolist()}")
    dev = sv.device
    if bottom is not None:
        if bottom.dtype != torch.float64 or bottom.shape[-1] != P or bottom.numel() not in (P, C * P):
            raise ValueError(f"transient_matecho: bottom must be float64 of shape ({P},) or ({C}, {P}), got "
                             f"{bottom.dtype} {tuple(bottom.shape)}")
    mask = torch.empty((C, P, S), dtype=torch.bool, device=dev)
    s_hi = _scratch("transient_matecho.s_hi", dev, C, P, dtype=torch.int32)
    flag = _scratch("transient_matecho.flag", dev, C, P, dtype=torch.uint8)
    call("epa_transient_matecho", _p(sv), _DT[sv.dtype], C, P, S,
         _p(to_device(np.ascontiguousarray(range_rows, dtype=np.float64).reshape(C, S), device=dev)),
         _p(to_device_small(chan_i, device=dev)),
         _p(to_device_small(np.ascontiguousarray(chan_d, dtype=np.float64).reshape(C, 2), device=dev)),
         _p(bottom), 0 if bottom is None else bottom.numel() // P, int(half_window), float(percentile), float(delta_db),
         int(extend_ping), float(min_window), _p(s_hi), _p(flag), _p(mask), _stream())
    return mask


# ---- masks from Sv differences, masks on the MVBS grid (mask.frequency_differencing / mask.regrid_mask) ----------------
_CMP = {">": _lib.CMP_GT, "<": _lib.CMP_LT, "<=": _lib.CMP_LE, ">=": _lib.CMP_GE, "==": _lib.CMP_EQ}


def freq_diff_mask(sv, chan_a, chan_b, operator, diff):
    """(sv[chan_a] - sv[chan_b]) operator diff -> bool like ``sv[0]``; ``sv`` float32 / float64 with the channel axis
    first.  The difference and ``diff`` are rounded in sv's dtype, as NumPy does (``epa_freq_diff_mask``)."""
    if operator not in _CMP:
        raise ValueError(f"freq_diff_mask: operator must be one of {list(_CMP)}, got {operator!r}")
    C = sv.shape[0]
    out = torch.empty(tuple(sv.shape[1:]), dtype=torch.bool, device=sv.device)
    call("epa_freq_diff_mask", _p(sv), C, out.numel(), int(chan_a), int(chan_b), _CMP[operator], float(diff), _p(out),
         _DT[sv.dtype], _stream())
    return out


def regrid_needs_global_flags(n_rbins):
    """The flags of one time bin (4 bytes per range bin) do not fit in LDS (``epa_regrid_needs_global_flags``)."""
    return _ask("epa_regrid_needs_global_flags", int(n_rbins)) != 0


def regrid_mask(mask, range, bin_start, n_tbins, range_bin, n_rbins, *, group=None, n_groups=None, func="logical-AND",
                closed="left"):
    """``mask`` uint8 / bool (T, P, D) onto the (time bin, range bin) grid -> (uint8 (G, n_tbins, n_rbins), int32 (1,)
    device tensor that is non-zero when a mask byte is neither 0 nor 1).  ``range`` f64 (D,) or (P, D); ``group``
    int32 (T,) device tensor of output slices 0 .. n_groups-1 or None (identity, G = T) (``epa_regrid_mask``)."""
    T, P, D = mask.shape
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8:
        raise ValueError(f"regrid_mask: mask must be bool or uint8, got {mask.dtype}")
    if range.dtype != torch.float64 or tuple(range.shape) not in ((D,), (P, D)):
        raise ValueError(f"regrid_mask: range must be float64 of shape ({D},) or ({P}, {D}), got {range.dtype} "
                         f"{tuple(range.shape)}")
    G = T if group is None else int(n_groups)
    cells = G * n_tbins * n_rbins
    buf = _scratch("regrid_mask.out", mask.device, G, n_tbins, n_rbins, dtype=torch.uint8)  # (whole 32-bit words)
    nonbinary = torch.empty(1, dtype=torch.int32, device=mask.device)
    call("epa_regrid_mask", _p(mask), _p(group), T, P, D, _p(range), int(range.dim() == 2), _p(bin_start), int(n_tbins),
         float(range_bin), int(n_rbins), _lib.BIN_CLOSED_RIGHT if closed == "right" else 0,
         {"logical-AND": 0, "logical-OR": 1}[func], _p(buf), _p(nonbinary), _stream())
    return buf[:cells].view(G, n_tbins, n_rbins), nonbinary


def _line_of(line, C, P, dev, what):
    """A bound of ``line_mask`` as (pointer, channel stride, ping stride): a float64 device tensor of shape (C, P), or one
    that broadcasts to it -- expanded, not copied, so a broadcast dimension has stride 0."""
    if line is None:
        return None, 0, 0
    if line.dtype != torch.float64 or not line.is_cuda or line.device != dev:
        raise ValueError(f"line_mask: {what} must be a float64 tensor on {dev}, got {line.dtype} on {line.device}")
    try:
        v = line.expand(C, P)
    except RuntimeError:
        raise ValueError(f"line_mask: {what} of shape {tuple(line.shape)} does not broadcast to ({C}, {P})") from None
    return ctypes.c_void_p(v.data_ptr()), v.stride(0), v.stride(1)


def line_mask(shape, *, range=None, coef=None, nan_raw=None, scale=None, offset=None, dtype=None, upper=None, lower=None,
              upper_offset=0.0, lower_offset=0.0, closed="left", nan_line="exclude"):
    """bool (C, P, S) = ``shape``: True where ``upper + upper_offset <= r < lower + lower_offset`` (``closed="right"``:
    ``<`` and ``<=``), compared in float64 (``epa_line_mask``).  The range ``r`` is either the float32 / float64 tensor
    ``range``, of that shape or broadcasting to it (read through its strides: nothing is copied), or what a lazy array
    would hold: ``coef`` (C, P, 8) coefficient rows, NaN where ``nan_raw`` (C, P, S) float32 is, times ``scale`` plus
    ``offset`` (C, P) float64 for a depth, rounded to ``dtype``.  ``upper`` / ``lower``: float64 device tensors that
    broadcast to (C, P), or None (not tested).  ``nan_line``: a NaN bound empties its row ("exclude") or is not tested
    there ("ignore")."""
    C, P, S = (int(n) for n in shape)
    if closed not in ("left", "right"):
        raise ValueError(f"line_mask: closed must be 'left' or 'right', got {closed!r}")
    if nan_line not in ("exclude", "ignore"):
        raise ValueError(f"line_mask: nan_line must be 'exclude' or 'ignore', got {nan_line!r}")
    if upper is None and lower is None:
        raise ValueError("line_mask: at least one of upper and lower must be given")
    if (range is None) == (coef is None):
        raise ValueError("line_mask: the range comes as an array or as coefficient rows, one of the two")
    flags = (_lib.LINE_CLOSED_RIGHT if closed == "right" else 0) | (_lib.LINE_NAN_IGNORE if nan_line == "ignore" else 0)
    if range is not None:
        if range.dtype not in _DT or not range.is_cuda:
            raise ValueError(f"line_mask: range must be a float32 / float64 device tensor, got {range.dtype} on {range.device}")
        dev, dtype = range.device, range.dtype
        try:
            rv = range.expand(C, P, S)
        except RuntimeError:
            raise ValueError(f"line_mask: range of shape {tuple(range.shape)} does not broadcast to {(C, P, S)}") from None
        r_args = (ctypes.c_void_p(rv.data_ptr()), *rv.stride(), None, None, None, None)
    else:
        dev = coef.device
        if coef.dtype != torch.float64 or tuple(coef.shape) != (C, P, _lib.NCOEF):
            raise ValueError(f"line_mask: coef must be float64 of shape {(C, P, _lib.NCOEF)}, got {coef.dtype} "
                             f"{tuple(coef.shape)}")
        if nan_raw is not None and (nan_raw.dtype != torch.float32 or tuple(nan_raw.shape) != (C, P, S)):
            raise ValueError(f"line_mask: nan_raw must be float32 of shape {(C, P, S)}, got {nan_raw.dtype} "
                             f"{tuple(nan_raw.shape)}")
        if (scale is None) != (offset is None):
            raise ValueError("line_mask: scale and offset come together")
        for name, t in (("scale", scale), ("offset", offset)):
            if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != (C, P)):
                raise ValueError(f"line_mask: {name} must be float64 of shape {(C, P)}, got {t.dtype} {tuple(t.shape)}")
        dtype = torch_dtype(dtype)
        r_args = (None, 0, 0, 0, _p(coef), _p(nan_raw), _p(scale), _p(offset))
    up, up_c, up_p = _line_of(upper, C, P, dev, "upper")
    lo, lo_c, lo_p = _line_of(lower, C, P, dev, "lower")
    out = torch.empty((C, P, S), dtype=torch.bool, device=dev)
    if out.numel() == 0:
        return out
    call("epa_line_mask", *r_args, _DT[dtype], up, up_c, up_p, float(upper_offset), lo, lo_c, lo_p, float(lower_offset),
         flags, C, P, S, _p(out), _stream())
    return out


# ---- Sv onto one range grid, the echo integral kept (commongrid.regrid_Sv) ----------------------------------------------
def regrid_rows(sv, range, range_bin, n_rbins, *, with_coverage=True, out=None, _max_grid=0):
    """Every row of ``sv`` (C, P, S), float32 / float64, onto the cells ``[j * range_bin, (j + 1) * range_bin)``,
    ``j < n_rbins`` -> (Sv (C, P, n_rbins) of sv's dtype, coverage of the same shape and type or None, int32 (1,) device
    tensor: the rows refused because fewer than two leading ranges are finite or they decrease) (``epa_regrid_rows``: one
    launch, every output element written exactly once; the rule is in the header).  ``range``: a float32 / float64
    device tensor, of sv's dtype or not, of sv's shape or broadcasting to it (read through its strides: nothing is
    copied).  ``out``: the (Sv, coverage) tensors to write into instead of new ones, coverage None without
    ``with_coverage`` (tests: a pre-filled allocation shows that every element is written).  ``_max_grid``: the most
    workgroups to launch (tests: the row loop at small shapes)."""
    if sv.dim() != 3 or sv.dtype not in _DT:
        raise ValueError(f"regrid_rows: sv must be float32 / float64 of shape (C, P, S), got {sv.dtype} {tuple(sv.shape)}")
    C, P, S = sv.shape
    dev, n_rbins = sv.device, int(n_rbins)
    if range.dtype not in _DT or not range.is_cuda or range.device != dev:
        raise ValueError(f"regrid_rows: range must be a float32 / float64 tensor on {dev}, got {range.dtype} on {range.device}")
    try:
        rv = range.expand(C, P, S)
    except RuntimeError:
        raise ValueError(f"regrid_rows: range of shape {tuple(range.shape)} does not broadcast to {(C, P, S)}") from None
    if n_rbins < 0:
        raise ValueError(f"regrid_rows: n_rbins must not be negative, got {n_rbins}")
    shape = (C, P, n_rbins)
    if out is None:
        sv_out = torch.empty(shape, dtype=sv.dtype, device=dev)
        cov = torch.empty(shape, dtype=sv.dtype, device=dev) if with_coverage else None
    else:
        sv_out, cov = out
        for t, wanted in ((sv_out, True), (cov, bool(with_coverage))):
            if (t is not None) != wanted or (t is not None and (t.dtype != sv.dtype or tuple(t.shape) != shape
                                                                 or t.device != dev or not t.is_contiguous())):
                raise ValueError(f"regrid_rows: out must hold contiguous {shape} tensors of {sv.dtype} on {dev}, the second "
                                 "None without with_coverage")
    n_unordered = torch.empty(1, dtype=torch.int32, device=dev)
    call("epa_regrid_rows", _p(sv), _DT[sv.dtype], ctypes.c_void_p(rv.data_ptr()), _DT[range.dtype], *rv.stride(), C, P, S,
         float(range_bin), n_rbins, _p(sv_out), _p(cov), _p(n_unordered), int(_max_grid), _stream())
    return sv_out, cov, n_unordered


# ---- NaN-aware median, mean, min and max windows (clean.window_filter) ----------------------------------------------------
def window_filter_args(method, ping_num, range_sample_num, min_valid, who="window_filter"):
    """The checked (method code, ping_num, range_sample_num, min_valid) of a window filter; ValueError otherwise.  No
    device is touched."""
    if not isinstance(method, str) or method not in _lib.WINDOW_METHODS:
        raise ValueError(f"{who}: method must be one of {_lib.WINDOW_METHODS}, got {method!r}")
    sizes = []
    for name, n in (("ping_num", ping_num), ("range_sample_num", range_sample_num)):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n % 2 != 1 or not 1 <= n <= _lib.WINDOW_FILTER_MAX:
            raise ValueError(f"{who}: {name} must be an odd integer within 1 .. {_lib.WINDOW_FILTER_MAX}, got {n!r}")
        sizes.append(int(n))
    if isinstance(min_valid, bool) or not isinstance(min_valid, (int, np.integer)) or not 1 <= min_valid <= sizes[0] * sizes[1]:
        raise ValueError(f"{who}: min_valid must be an integer within 1 .. {sizes[0] * sizes[1]} (the window), got {min_valid!r}")
    return _lib.WINDOW_METHODS.index(method), sizes[0], sizes[1], int(min_valid)


def window_filter(x, method, ping_num, range_sample_num, *, min_valid=1, keep_nan=True, out=None, _max_grid=0):
    """``x`` (C, P, S) or (P, S), float32 / float64, contiguous, on the device -> the tensor of the same type and shape
    in which every sample is the ``method`` ("median", "mean", "min", "max") of the ``ping_num x range_sample_num``
    samples around it, both sizes odd and at most ``_lib.WINDOW_FILTER_MAX`` (``epa_window_filter``: one launch, every
    output element written exactly once; THE RULE is in the header and in ``clean.window_filter``).  The window is
    clipped to the array and never crosses channels; NaN is skipped, +-inf are values; fewer than ``min_valid`` valid
    values give NaN; with ``keep_nan`` a NaN sample stays NaN.  ``out``: the tensor to write into instead of a new one
    (it must not overlap ``x``; tests: a pre-filled allocation shows that every element is written).  ``_max_grid``:
    the most workgroups to launch (tests: the tile loop at small shapes).  No host synchronisation."""
    code, ping_num, range_sample_num, min_valid = window_filter_args(method, ping_num, range_sample_num, min_valid)
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or x.dtype not in _DT:
        raise ValueError("window_filter: x must be a float32 / float64 tensor of shape (C, P, S) or (P, S), got "
                         f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    if not x.is_cuda:
        raise ValueError(f"window_filter: x must be on the device, got a tensor on {x.device}")
    if not x.is_contiguous():
        raise ValueError("window_filter: x must be contiguous")
    if out is None:
        out = torch.empty_like(x)
    elif (not isinstance(out, torch.Tensor) or out.dtype != x.dtype or out.shape != x.shape or out.device != x.device
          or not out.is_contiguous()):
        raise ValueError(f"window_filter: out must be a contiguous {tuple(x.shape)} tensor of {x.dtype} on {x.device}")
    C = x.shape[0] if x.dim() == 3 else 1
    P, S = x.shape[-2:]
    call("epa_window_filter", _p(x), _DT[x.dtype], C, P, S, code, ping_num, range_sample_num, min_valid, int(bool(keep_nan)),
         _p(out), int(_max_grid), _stream())
    return out


# ---- echo summary statistics per row (metrics.*) ------------------------------------------------------------------------
METRICS =("abundance", "center_of_mass", "dispersion", "evenness", "aggregation")


def echo_metrics(sv, range, *, cm=None, want=METRICS, _max_grid=0):
    """The statistics named in ``want`` of every row of ``sv`` (R, S) -> {name: (R,) tensor of sv's dtype}, from one
    sweep over ``sv`` and ``range`` (``epa_echo_metrics``).  ``range``: sv's dtype, (R, S) or (S,) shared by all rows.
    ``cm``: float64 (R,) centres for ``dispersion``; None: the row's own centre of mass.  The arrays may start at any
    element (a contiguous view).  ``_max_grid``: the most workgroups to launch (tests: the row loops at small shapes)."""
    want = tuple(want)
    if not want or any(w not in METRICS for w in want):
        raise ValueError(f"echo_metrics: want must name some of {METRICS}, got {want!r}")
    if sv.dim() != 2 or sv.dtype not in _DT:
        raise ValueError(f"echo_metrics: sv must be float32 / float64 of shape (R, S), got {sv.dtype} {tuple(sv.shape)}")
    R, S = sv.shape
    if range.dtype != sv.dtype or tuple(range.shape) not in ((R, S), (S,)):
        raise ValueError(f"echo_metrics: range must be {sv.dtype} of shape ({R}, {S}) or ({S},), got {range.dtype} "
                         f"{tuple(range.shape)}")
    if cm is not None and (cm.dtype != torch.float64 or tuple(cm.shape) != (R,)):
        raise ValueError(f"echo_metrics: cm must be float64 of shape ({R},), got {cm.dtype} {tuple(cm.shape)}")
    out = {w: torch.empty(R, dtype=sv.dtype, device=sv.device) for w in METRICS if w in want}
    if R == 0:
        return out
    call("epa_echo_metrics", _p(sv), _p(range), int(range.dim() == 2), R, S, _p(cm), *(_p(out.get(w)) for w in METRICS),
         _DT[sv.dtype], int(_max_grid), _stream())
    return out


# ---- an external clock brought onto ping_time (utils.align.align_to_ping_time, consolidate.add_location) -------------------
ALIGN_MODES = {"linear": _lib.ALIGN_LINEAR, "nearest": _lib.ALIGN_NEAREST}


def align_to_ping_time(t_ext, y, ping_time, method="linear"):
    """``y`` (V, N) float64, recorded at the int64-ns times ``t_ext`` (N,) (strictly increasing, no NaT), on the int64-ns
    ``ping_time`` (P,) (any order, INT64_MIN = NaT -> NaN) -> (V, P) float64 (``epa_align_to_ping_time``): one launch,
    one search per ping for all V rows.  ``method``: "linear" (scipy's interp1d with extrapolation, bit for bit) or
    "nearest" (ties to the earlier sample, the end sample outside the track)."""
    if method not in ALIGN_MODES:
        raise ValueError(f"align_to_ping_time: method must be 'linear' or 'nearest', got {method!r}")
    if t_ext.dtype != torch.int64 or t_ext.dim() != 1 or ping_time.dtype != torch.int64 or ping_time.dim() != 1:
        raise ValueError(f"align_to_ping_time: t_ext and ping_time must be 1-D int64, got {t_ext.dtype} "
                         f"{tuple(t_ext.shape)} and {ping_time.dtype} {tuple(ping_time.shape)}")
    N, P = t_ext.numel(), ping_time.numel()
    if y.dtype != torch.float64 or y.dim() != 2 or y.shape[1] != N:
        raise ValueError(f"align_to_ping_time: y must be float64 of shape (V, {N}), got {y.dtype} {tuple(y.shape)}")
    if not (t_ext.device == y.device == ping_time.device):
        raise ValueError(f"align_to_ping_time: t_ext, y and ping_time must be on one device, got {t_ext.device}, "
                         f"{y.device} and {ping_time.device}")
    V = y.shape[0]
    out = torch.empty((V, P), dtype=torch.float64, device=y.device)
    call("epa_align_to_ping_time", _p(t_ext), N, _p(y), V, _p(ping_time), P, ALIGN_MODES[method], _p(out), _stream())
    return out


# ---- a time coordinate that steps backwards (qc.exist_reversed_time, qc.coerce_increasing_time) ----------------------------
QC_MAX_WIN = _lib.QC_MAX_WIN


def _qc_times(t, what):
    if t.dtype != torch.int64 or t.dim() != 1:
        raise ValueError(f"{what}: the times must be 1-D int64, got {t.dtype} {tuple(t.shape)}")
    return t.numel()


def time_reversals(t, want_list=False):
    """The facts of the int64 ticks ``t`` (N >= 1; INT64_MIN = NaT) -> (facts, list): ``facts`` int64 (4,) on the device
    -- the first reversal index (-1: none), the number of reversals, the number of NaT, the entries of the list
    (``_lib.QC_FIRST`` ...) --, ``list`` the (N - 1,) reversal indices in no particular order (the first ``count`` are
    meant) or None (``epa_time_reversals``, one launch).  A difference is a reversal when it is negative and touches no
    NaT."""
    N = _qc_times(t, "time_reversals")
    facts = torch.empty(_lib.QC_FACTS, dtype=torch.int64, device=t.device)
    lst = torch.empty(max(N - 1, 1), dtype=torch.int64, device=t.device) if want_list else None
    call("epa_time_reversals", _p(t), N, _p(facts), _p(lst), _stream())
    return facts, lst


def reversal_medians(t, facts, lst, win_len, sub=None):
    """``sub`` (N - 1,) int64 with, at every reversal ``ni`` of ``lst``, the median of the original differences
    ``d[max(0, ni - win_len) : ni]`` -- INT64_MIN (NaT) where that window is empty, a reversal in the first difference --
    (``epa_reversal_medians``; the other entries are not written).  ``facts`` and ``lst``
    as :func:`time_reversals` left them for the same ``t``, which must hold no NaT."""
    N = _qc_times(t, "reversal_medians")
    if sub is None:
        sub = torch.empty(N - 1, dtype=torch.int64, device=t.device)
    if lst.numel() < N - 1 or sub.numel() < N - 1 or facts.numel() != _lib.QC_FACTS:
        raise ValueError("reversal_medians: facts, list and sub must belong to the times")
    call("epa_reversal_medians", _p(t), N, int(win_len), _p(facts), _p(lst), _p(sub), _stream())
    return sub


def time_rebuild(t, facts, sub):
    """The times with the differences at the reversals replaced by ``sub`` (``epa_time_rebuild``: three launches, tile
    sums, carries, apply) -> a new (N,) int64 tensor; the times up to the first reversal are copies."""
    N = _qc_times(t, "time_rebuild")
    if sub.numel() < N - 1 or facts.numel() != _lib.QC_FACTS:
        raise ValueError("time_rebuild: facts and sub must belong to the times")
    out = torch.empty_like(t)
    work = _scratch("time_rebuild.tile_workspace", t.device, N, dtype=torch.int64)
    call("epa_time_rebuild", _p(t), N, _p(facts), _p(sub), _p(work), _p(out), _stream())
    return out


# ---- many files into one volume (combine_echodata) -----------------------------------------------------------------------
_CT = {torch.int8: _lib.CT_I8, torch.int16: _lib.CT_I16, torch.int32: _lib.CT_I32, torch.int64: _lib.CT_I64,
       torch.float32: _lib.CT_F32, torch.float64: _lib.CT_F64}
_CT_BITS = {1: _lib.CT_I8, 2: _lib.CT_I16, 4: _lib.CT_I32, 8: _lib.CT_I64}  # any other type, by its size: a bitwise copy
_CT_PROMOTED = {torch.int8: torch.float32, torch.int16: torch.float32, torch.int32: torch.float64,
                torch.int64: torch.float64}


def concat_rows(srcs, chan_maps=None, out_dtype=None):
    """The device tensors ``srcs[i]`` of shape (C_i, P_i, S_i) or (C_i, P_i, S_i, B), all of one dtype, joined along
    their second axis into ``out`` (C, sum P_i, max S_i[, B]); rows shorter than the longest are NaN-padded
    (``epa_concat_rows``: one launch however many tensors, every source byte read once, every output byte written once).
    ``chan_maps[i][c]``: the channel of ``srcs[i]`` that becomes output channel ``c`` (None: the tensors' own order, all
    C_i equal).  ``out_dtype`` None: the sources' own type, or, when a pad is needed and they are integers, the float
    type NumPy would promote them to for a NaN (int8 / int16 -> float32, int32 / int64 -> float64); otherwise the type
    asked for, which must be the sources' own or that promotion.  A same-type join is a bitwise copy."""
    srcs = list(srcs)
    if not srcs:
        raise ValueError("concat_rows: at least one tensor is needed")
    t0 = srcs[0]
    nd = t0.dim()
    if nd not in (3, 4):
        raise ValueError(f"concat_rows: tensors of 3 or 4 dimensions are served, got {tuple(t0.shape)}")
    for t in srcs:
        if t.dim() != nd or t.dtype != t0.dtype or t.device != t0.device or (nd == 4 and t.shape[3] != t0.shape[3]):
            raise ValueError(f"concat_rows: the tensors must agree in dtype, device, number of dimensions and trailing "
                             f"dimension, got {t.dtype} {tuple(t.shape)} on {t.device} next to {t0.dtype} "
                             f"{tuple(t0.shape)} on {t0.device}")
        if t.numel() and not (t.is_cuda and t.is_contiguous()):
            raise ValueError("concat_rows: C-contiguous device tensors are needed")
    B = int(t0.shape[3]) if nd == 4 else 1
    if chan_maps is None:
        if any(t.shape[0] != t0.shape[0] for t in srcs):
            raise ValueError("concat_rows: tensors with different numbers of channels need chan_maps")
        chan_maps = [range(int(t0.shape[0]))] * len(srcs)
    chan = np.ascontiguousarray(np.array([list(m) for m in chan_maps], dtype=np.int32).reshape(len(srcs), -1))
    if chan.shape[0] != len(srcs) or chan.shape[1] < 1:
        raise ValueError(f"concat_rows: chan_maps must hold one row of at least one channel per tensor, got {chan.shape}")
    C = chan.shape[1]
    S_out = max(int(t.shape[2]) for t in srcs)
    padded = any(int(t.shape[2]) < S_out for t in srcs)
    if out_dtype is None:
        out_dtype = _CT_PROMOTED.get(t0.dtype, t0.dtype) if padded else t0.dtype
    if out_dtype == t0.dtype:
        src_ct = out_ct = _CT.get(t0.dtype) if t0.dtype in (torch.float32, torch.float64) else _CT_BITS.get(t0.element_size())
    else:
        src_ct, out_ct = _CT.get(t0.dtype), _CT.get(out_dtype)
    if src_ct is None or out_ct is None:
        raise ValueError(f"concat_rows: {t0.dtype} -> {out_dtype} is not served")
    segs = np.zeros((len(srcs), _lib.CONCAT_SEG_WORDS), dtype=np.int64)
    first = 0
    for i, t in enumerate(srcs):
        segs[i] = (t.data_ptr(), t.shape[1], int(t.shape[2]) * B, first, t.shape[0])
        first += int(t.shape[1])
    shape = (C, first, S_out) + ((B,) if nd == 4 else ())
    out = torch.empty(shape, dtype=out_dtype, device=t0.device)
    # the segment table holds pointers, so its content is new with nearly every call: a plain upload, not the content-keyed
    # cache; the channel table is the same for every variable and file set of a survey
    seg_dev, chan_dev = to_device(segs, device=t0.device), to_device_small(chan, device=t0.device)
    call("epa_concat_rows", segs.ctypes.data_as(ctypes.c_void_p), _p(seg_dev), chan.ctypes.data_as(ctypes.c_void_p),
         _p(chan_dev), len(srcs), C, S_out * B, src_ct, out_ct, ctypes.c_void_p(out.data_ptr()), _stream())
    return out


def upload_file_bytes(data, device=None):
    """The bytes of a file (anything ``np.frombuffer`` takes) -> (uint8 device tensor padded with zeros to a multiple of
    16 bytes, the number of file bytes): what ``raw0_unpack`` reads.  One upload of the file as it is on disk."""
    host = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1).view(np.uint8)
    n = int(host.size)
    padded = np.zeros(max(16, -(-n // 16) * 16), dtype=np.uint8)
    padded[:n] = host
    return to_device(padded, device=device), n


_RAW_ANGLES = {None: _lib.RAW_ANGLE_NONE, "int8": _lib.RAW_ANGLE_I8, "float32": _lib.RAW_ANGLE_F32}


def raw0_unpack(file_bytes, table, C, P, S, angles="int8", *, n_bytes=None, out=None):
    """The RAW0 sample blocks of an EK60 .raw file -> (power, athwartship, alongship) device tensors of shape (C, P, S)
    (``epa_raw0_unpack``: one launch, every file sample byte read once, every output element written exactly once).

    ``file_bytes``: the file as it is on disk, a uint8 device tensor whose length is a multiple of 16 (``upload_file_bytes``
    pads it; ``n_bytes``: the file's own length, default all of it).  ``table``: int64 host array (C * P, 3), row
    ``(c, p)``: byte offset of the int16 power block, byte offset of the int8 (athwartship, alongship) pair block -- -1
    where the row has none -- and the sample count.  power = ``float32(int16) * float32(10 log10(2) / 256)``, NaN behind
    the count.  ``angles``: "int8" (every row must be full and have angles), "float32" (NaN-padded) or None (the two
    planes are returned as None).  ``out``: the three tensors to write into instead of new ones (tests: a pre-filled
    allocation shows that every element is written)."""
    if angles not in _RAW_ANGLES:
        raise ValueError(f"raw0_unpack: angles must be 'int8', 'float32' or None, got {angles!r}")
    if not (isinstance(file_bytes, torch.Tensor) and file_bytes.dtype == torch.uint8 and file_bytes.dim() == 1):
        raise ValueError("raw0_unpack: file_bytes must be a one-dimensional uint8 tensor")
    C, P, S = int(C), int(P), int(S)
    tab = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, 3))
    if tab.shape[0] != C * P:
        raise ValueError(f"raw0_unpack: the table has {tab.shape[0]} rows, C * P = {C * P} are needed")
    dev = file_bytes.device
    adt = {None: None, "int8": torch.int8, "float32": torch.float32}[angles]
    if out is None:
        power = torch.empty((C, P, S), dtype=torch.float32, device=dev)
        athw = torch.empty((C, P, S), dtype=adt, device=dev) if adt is not None else None
        along = torch.empty((C, P, S), dtype=adt, device=dev) if adt is not None else None
    else:
        power, athw, along = out
        for t, dt in ((power, torch.float32), (athw, adt), (along, adt)):
            if (t is None) != (dt is None) or (t is not None and (t.dtype != dt or tuple(t.shape) != (C, P, S))):
                raise ValueError("raw0_unpack: out must hold (C, P, S) tensors of the types asked for")
    tab_dev = to_device(tab, device=dev)
    call("epa_raw0_unpack", _p(file_bytes), int(file_bytes.numel() if n_bytes is None else n_bytes), int(file_bytes.numel()),
         tab.ctypes.data_as(ctypes.c_void_p), _p(tab_dev), C, P, S, _RAW_ANGLES[angles], _p(power), _p(athw), _p(along),
         _stream())
    return power, athw, along


def nmea_positions(file_bytes, table, *, n_bytes=None, out=None):
    """Latitude and longitude of NMEA sentences lying in the bytes of an EK60 .raw file -> (lat float64, lon float64,
    code uint8) device tensors of length n (``epa_nmea_positions``: one launch, a wavefront per sentence).

    ``file_bytes``: as for ``raw0_unpack``.  ``table``: int64 host array (n, 2), byte offset and length of each sentence's
    text, NULs stripped.  ``code``: 0 or the bits ``_lib.NMEA_LAT_FAILED`` / ``NMEA_LON_FAILED`` (that value is NaN) with
    the sentence type in ``_lib.NMEA_TYPE_MASK``; ``NMEA_INVALID`` (NaN, NaN); ``NMEA_UNDECIDED``: the kernel decides the
    plain form only (``convert.parse_nmea.plain_form``), the caller applies ``parse_nmea.parse_sentence`` to the rest.
    ``n == 0`` launches nothing.  ``out``: the three tensors to write into instead of new ones (tests)."""
    if not (isinstance(file_bytes, torch.Tensor) and file_bytes.dtype == torch.uint8 and file_bytes.dim() == 1):
        raise ValueError("nmea_positions: file_bytes must be a one-dimensional uint8 tensor")
    tab = np.asarray(table, dtype=np.int64)
    if tab.ndim != 2 or tab.shape[1] != 2:
        raise ValueError(f"nmea_positions: the table must have the shape (n, 2), got {tab.shape}")
    tab = np.ascontiguousarray(tab)
    n, dev = int(tab.shape[0]), file_bytes.device
    if out is None:
        lat = torch.empty(n, dtype=torch.float64, device=dev)
        lon = torch.empty(n, dtype=torch.float64, device=dev)
        code = torch.empty(n, dtype=torch.uint8, device=dev)
    else:
        lat, lon, code = out
        for t, dt in ((lat, torch.float64), (lon, torch.float64), (code, torch.uint8)):
            if t.dtype != dt or tuple(t.shape) != (n,) or t.device != dev or not t.is_contiguous():
                raise ValueError("nmea_positions: out must hold contiguous (n,) tensors of float64, float64 and uint8 on the "
                                 "file's device")
    tab_dev = to_device(tab, device=dev) if n else None
    call("epa_nmea_positions", _p(file_bytes), int(file_bytes.numel() if n_bytes is None else n_bytes), int(file_bytes.numel()),
         tab.ctypes.data_as(ctypes.c_void_p), _p(tab_dev), n, _p(lat), _p(lon), _p(code), _stream())
    return lat, lon, code


class Timer:
    """HIP-event timer on torch's current stream (epa_timer_*)."""

    def __init__(self):
        h = ctypes.c_void_p()
        _lib.check(_lib.lib.epa_timer_create(ctypes.byref(h)), "epa_timer_create")
        self._h = h

    def start(self):
        call("epa_timer_start", self._h, _stream())

    def stop(self):
        call("epa_timer_stop", self._h, _stream())

    def elapsed_ms(self):
        ms = ctypes.c_float()
        _lib.check(_lib.lib.epa_timer_elapsed_ms(self._h, ctypes.byref(ms)), "epa_timer_elapsed_ms")
        return float(ms.value)

    def __del__(self):
        try:
            _lib.lib.epa_timer_destroy(self._h)
        except Exception:
            pass


# ---- noise masks ------------------------------------------------------------------

def range_bin_smooth(sv, *, nper=None, range=None, r0=0.0, bin=0.0, nbins=0, out=None):
    """Depth-bin smoothing of mask_impulse_noise -> up-sampled Sv like ``sv``.
    Index mode: ``nper`` samples per bin (one value for all channels of ``sv``).
    Value mode: ``range`` array + bins np.arange(r0, max + bin, bin) (``nbins`` = len(edges) - 1)."""
    C, P, S = sv.shape
    if range is not None and range.dtype != sv.dtype:
        range = range.to(sv.dtype)
    if out is None:
        out = torch.empty_like(sv)
    call("epa_range_bin_smooth", _p(sv), _p(range), C, P, S, int(nper or 0), float(r0), float(bin),
         int(nbins), _p(out), _DT[sv.dtype], _stream())
    return out


def impulse_mask(up, num_side_pings, threshold):
    """Two-sided ping comparison -> uint8 (C,P,S)."""
    C, P, S = up.shape
    out = torch.empty((C, P, S), dtype=torch.uint8, device=up.device)
    call("epa_impulse_mask", _p(up), C, P, S, int(num_side_pings), float(threshold), _p(out),
         _DT[up.dtype], _stream())
    return out


def pool_sv(sv, first_sample, num_side_pings, num_side_samples, func="nanmean", threshold=0.0,
            want_pooled=True, want_mask=True, mask_out=None):
    """Index-binning pooled Sv (reflect window) and/or the mask Sv - pooled > threshold."""
    C, P, S = sv.shape
    f = {"nanmean": _lib.POOL_NANMEAN, "nanmedian": _lib.POOL_NANMEDIAN}[func]
    pooled = torch.empty_like(sv) if want_pooled else None
    mask = (mask_out if mask_out is not None else
            torch.empty((C, P, S), dtype=torch.uint8, device=sv.device)) if want_mask else None
    mean = f == _lib.POOL_NANMEAN
    ws = _scratch("pool_sv.sum_ws", sv.device, C, P, S) if mean else None
    wc = _scratch("pool_sv.cnt_ws", sv.device, C, P, S, dtype=torch.int32) if mean else None
    call("epa_pool_sv", _p(sv), C, P, S, int(first_sample), int(num_side_pings), int(num_side_samples),
         f, float(threshold), _p(pooled), _p(mask), _p(ws), _p(wc), _DT[sv.dtype], _stream())
    return pooled, mask


def attenuated_mask(sv, range, upper_limit, lower_limit, num_side_pings, threshold):
    C, P, S = sv.shape
    if range.dtype != sv.dtype:
        range = range.to(sv.dtype)
    out = torch.empty((C, P, S), dtype=torch.uint8, device=sv.device)
    call("epa_attenuated_mask", _p(sv), _p(range), C, P, S, float(upper_limit), float(lower_limit),
         int(num_side_pings), float(threshold), _p(out), _DT[sv.dtype], _stream())
    return out


def apply_mask(src, mask, fill_value=float("nan"), fill_array=None):
    """where(mask, src, fill); ``mask`` uint8 with src.numel() % mask.numel() == 0 (trailing-dims
    broadcast), ``fill_array`` likewise."""
    out = torch.empty_like(src)
    if fill_array is not None and fill_array.dtype != src.dtype:
        fill_array = fill_array.to(src.dtype)
    call("epa_apply_mask", _p(src), _p(mask), src.numel(), mask.numel(), float(fill_value),
         _p(fill_array), fill_array.numel() if fill_array is not None else 1, _p(out), _DT[src.dtype],
         _stream())
    return out


def apply_masks(src, masks, fill_value=float("nan"), fill_array=None, want_minmax=False):
    """where(AND of ``masks``, src, fill) in one sweep (1 to 4 uint8 masks, each tiling ``src`` over its leading dims)
    -> (out, f64 device tensor {nanmin, nanmax} of out | None)."""
    if not 1 <= len(masks) <= 4:
        raise ValueError("apply_masks takes 1 to 4 masks (AND further ones with mask_and first)")
    out = torch.empty_like(src)
    if fill_array is not None and fill_array.dtype != src.dtype:
        fill_array = fill_array.to(src.dtype)
    ptrs = (ctypes.c_void_p * len(masks))(*[m.data_ptr() for m in masks])
    periods = (ctypes.c_size_t * len(masks))(*[m.numel() for m in masks])
    ws = _scratch("apply_masks.workspace", src.device) if want_minmax else None
    mm = torch.empty(2, dtype=torch.float64, device=src.device) if want_minmax else None
    call("epa_apply_masks", _p(src), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(periods, ctypes.c_void_p), len(masks),
         src.numel(), float(fill_value), _p(fill_array), fill_array.numel() if fill_array is not None else 1, _p(out),
         _p(ws), _p(mm), _DT[src.dtype], _stream())
    return out, mm


def mask_and(a, b):
    """a & b, ``b`` broadcast over the leading dims of ``a``."""
    out = torch.empty_like(a)
    call("epa_mask_and", _p(a), _p(b), a.numel(), b.numel(), _p(out), _stream())
    return out


def range_step_mean(range):
    """Per-channel nanmean of the sample-to-sample range step -> numpy f64 [C]."""
    C, P, S = range.shape
    ws = _scratch("range_step_mean.workspace", range.device, C, P)
    out = torch.empty(C, dtype=torch.float64, device=range.device)
    call("epa_range_step_mean", _p(range), C, P, S, _DT[range.dtype], _p(ws), _p(out), _stream())
    return out.cpu().numpy()


def first_not_le(x, limit):
    """Flat index of the first element not <= limit (NaN counts); x.numel() if none."""
    out = torch.empty(1, dtype=torch.int64, device=x.device)
    call("epa_first_not_le", _p(x), x.numel(), float(limit), _DT[x.dtype], _p(out), _stream())
    return int(out.item())


def range_rows_check(range):
    """-> (nvalid int32 (C,P) device tensor, number of rows violating monotonicity / NaN-tail)."""
    C, P, S = range.shape
    nvalid = torch.empty((C, P), dtype=torch.int32, device=range.device)
    bad = torch.empty(1, dtype=torch.int32, device=range.device)
    call("epa_range_rows_check", _p(range), C, P, S, _DT[range.dtype], _p(nvalid), _p(bad), _stream())
    return nvalid, int(bad.item())


def pool_sv_value(sv, range, nvalid, depth_bin, num_side_pings, exclude_above, range_min, range_max,
                  func="nanmean", threshold=0.0, want_pooled=True, want_mask=True, running_sums=True):
    """Value-window pooled Sv (pool_Sv) and/or the mask Sv - pooled > threshold.  ``running_sums`` (nanmean):
    per-row double-double running sums and interval sums in a 40 B/sample workspace instead of summing every window;
    when that does not fit next to the arrays the workspace-free kernel runs
    (same results, every window summed value by value).  nanmedian: with ``running_sums`` the window is carried from
    ping to ping (a small workspace), without it every window is taken from memory."""
    C, P, S = sv.shape
    if range.dtype != sv.dtype:
        range = range.to(sv.dtype)
    f = {"nanmean": _lib.POOL_NANMEAN, "nanmedian": _lib.POOL_NANMEDIAN}[func]
    pooled = torch.empty_like(sv) if want_pooled else None
    mask = torch.empty((C, P, S), dtype=torch.uint8, device=sv.device) if want_mask else None
    ws = None
    if running_sums and func == "nanmean":
        try:
            ws = _scratch("pool_sv_value.ws_mean", sv.device, C, P, S)
        except torch.cuda.OutOfMemoryError:
            ws = None
    elif running_sums:  # nanmedian: the per-channel sample intervals
        ws = _scratch("pool_sv_value.ws_median", sv.device, C, S, dtype=torch.int32)
    call("epa_pool_sv_value", _p(sv), _p(range), _p(nvalid), C, P, S, float(depth_bin), int(num_side_pings),
         float(exclude_above), float(range_min), float(range_max), f, float(threshold), _p(pooled),
         _p(mask), _p(ws), _DT[sv.dtype], _stream())
    return pooled, mask


# ---- NASC ---------------------------------------------------------------------------

def geodesic_steps(lat, lon):
    """WGS-84 geodesic length in metres from every ping to the next (f64 device tensors (P,) in degrees; NaN for the
    last ping and NaN positions) -- commongrid/utils.py:208-231's geopy loop as one launch."""
    P = lat.numel()
    out = torch.empty(P, dtype=torch.float64, device=lat.device)
    call("epa_geodesic_steps", _p(lat), _p(lon), P, _p(out), _stream())
    return out


def nasc(sv, depth, bin_start, n_dbins, range_bin, n_rbins, skipna=True, closed="left", want_parts=False):
    """compute_raw_NASC -> NASC (C, n_dbins, n_rbins) [, sv_mean, h_mean]."""
    C, P, S = sv.shape
    if depth.dtype != sv.dtype:
        depth = depth.to(sv.dtype)
    ws = _scratch("nasc.workspace", sv.device, C, n_dbins, n_rbins)
    out = torch.empty((C, n_dbins, n_rbins), dtype=sv.dtype, device=sv.device)
    svm = torch.empty_like(out) if want_parts else None
    hm = torch.empty_like(out) if want_parts else None
    call("epa_nasc", _p(sv), _p(depth), C, P, S, _p(bin_start), int(n_dbins), float(range_bin), int(n_rbins),
         _bin_flags(skipna, closed), _p(ws), _p(out), _p(svm), _p(hm), _DT[sv.dtype], _stream())
    return (out, svm, hm) if want_parts else out


# ---- the whole chain in two passes ---------------------------------------------------------------------

def sv_noise_fused(raw, coef, alpha2, ping_num, range_sample_num, *, cal_type="Sv",
                   flags=_lib.FLAG_GUARD_POS | _lib.FLAG_MASK_RANGE, dtype=torch.float64,
                   noise_max=float("nan"), want_sv=True, want_range=False, want_range_max=False,
                   want_range_stats=False, ping_phase=0, want_edges=False):
    """K1+K6 -> (Sv|None, echo_range|None, noise (C, ceil((P + ping_phase)/ping_num)) f64[, nanmax(echo_range)]).
    ``want_range_stats``: the last element is instead the f64 device tensor {nanmin, nanmax, NaN count} of the echo_range
    (NaN count -1: the kernel that served the configuration leaves none; with ``want_range_max`` as well the maximum
    comes first, then the tensor).  ``ping_phase`` / ``want_edges``: a ping shard
    of a longer file, as ``noise_estimate`` -- with ``want_edges`` two more elements follow: edge_sum f64 (2, C, Sb),
    edge_cnt int32 (2, C, Sb), the raw (sum, count) rows of the shard's first / last ping block."""
    C, P, S = raw.shape
    if raw.dtype != torch.float32:
        raise ValueError("raw power samples must be float32 (convert/parse_base.py:302)")
    dev = raw.device
    sv = torch.empty((C, P, S), dtype=dtype, device=dev) if want_sv else None
    rng = torch.empty((C, P, S), dtype=dtype, device=dev) if want_range else None
    noise = torch.empty((C, -(-(P + ping_phase) // ping_num)), dtype=torch.float64, device=dev)
    rmax = torch.empty(1, dtype=torch.float64, device=dev) if want_range_max or want_range_stats else None
    rstats = torch.empty(3, dtype=torch.float64, device=dev) if want_range_stats else None
    es = ec = None
    if want_edges:
        Sb = -(-S // range_sample_num)
        es = torch.zeros((2, C, Sb), dtype=torch.float64, device=dev)
        ec = torch.zeros((2, C, Sb), dtype=torch.int32, device=dev)
    call("epa_sv_noise_fused", _p(raw), _p(coef), _p(alpha2), C, P, S,
         _lib.CAL_SV if cal_type == "Sv" else _lib.CAL_TS, flags, int(ping_num), int(range_sample_num), int(ping_phase),
         float(noise_max), _p(sv), _p(rng), _p(noise), _p(es), _p(ec), _p(rmax), _p(rstats), _DT[dtype], _stream())
    edges = (es, ec) if want_edges else ()
    if want_range_stats and want_range_max:  # both: the maximum (every kernel leaves it), then the statistics
        return (sv, rng, noise, float(rmax.item()), rstats) + edges
    if want_range_stats:
        return (sv, rng, noise, rstats) + edges
    return ((sv, rng, noise, float(rmax.item())) if want_range_max else (sv, rng, noise)) + edges


def denoise_mvbs(sv, alpha2, noise, ping_num, snr_threshold, bin_start, n_tbins, range_bin, n_rbins, *,
                 range=None, coef=None, skipna=True, closed="left", fill_value=float("nan"),
                 ping_perm=None, want_noise=False, want_corrected=True, want_partials=False):
    """K7+K5 -> dict(MVBS of the corrected Sv, Sv_noise, Sv_corrected, sum, cnt)."""
    C, P, S = sv.shape
    dev, dtype = sv.device, sv.dtype
    if range is not None and range.dtype != dtype:
        range = range.to(dtype)
    sn = torch.empty_like(sv) if want_noise else None
    sc = torch.empty_like(sv) if want_corrected else None
    out = torch.empty((C, n_tbins, n_rbins), dtype=dtype, device=dev)
    ssum, cnt = _partials(want_partials, C, n_tbins, n_rbins, dtype, dev)
    call("epa_denoise_mvbs", _p(sv), _p(range), _p(coef), _p(alpha2), _p(noise), C, P, S, int(ping_num),
         float(snr_threshold), _p(bin_start), _p(ping_perm), int(n_tbins), float(range_bin), int(n_rbins),
         _bin_flags(skipna, closed), float(fill_value), _p(sn), _p(sc), _p(out), _p(ssum), _p(cnt),
         _DT[dtype], _stream())
    return dict(MVBS=out, Sv_noise=sn, Sv_corrected=sc, sum=ssum, cnt=cnt)


def sv_denoise_mvbs(raw, coef, alpha2, noise, ping_num, snr_threshold, bin_start, n_tbins, range_bin, n_rbins,
                    *, cal_type="Sv", flags=_lib.FLAG_GUARD_POS | _lib.FLAG_MASK_RANGE, dtype=torch.float64,
                    skipna=True, closed="left", fill_value=float("nan"), ping_perm=None, want_noise=False,
                    want_corrected=True, want_range=False, want_partials=False, want_minmax=False,
                    minmax_async=False, ping_phase=0):
    """K1+K7+K5 from the raw power -> dict(MVBS of the corrected Sv, Sv_noise, Sv_corrected, echo_range, sum,
    cnt, minmax = [min, max of Sv_noise, min, max of Sv_corrected] (host floats) if asked; ``minmax_async``: a
    ``HostFuture`` of the four numbers instead -- the call then does not wait for its kernel)."""
    C, P, S = raw.shape
    dev = raw.device
    mk = lambda want: torch.empty((C, P, S), dtype=dtype, device=dev) if want else None  # noqa: E731
    sn, sc, rng = mk(want_noise), mk(want_corrected), mk(want_range)
    out = torch.empty((C, n_tbins, n_rbins), dtype=dtype, device=dev)
    ssum, cnt = _partials(want_partials, C, n_tbins, n_rbins, dtype, dev)
    mm = torch.empty(4, dtype=torch.float64, device=dev) if want_minmax else None
    call("epa_sv_denoise_mvbs", _p(raw), _p(coef), _p(alpha2), _p(noise), C, P, S,
         _lib.CAL_SV if cal_type == "Sv" else _lib.CAL_TS, flags, int(ping_num), int(ping_phase), float(snr_threshold),
         _p(bin_start), _p(ping_perm), int(n_tbins), float(range_bin), int(n_rbins), _bin_flags(skipna, closed),
         float(fill_value), _p(sn), _p(sc), _p(rng), _p(out), _p(ssum), _p(cnt), _p(mm), _DT[dtype], _stream())
    return dict(MVBS=out, Sv_noise=sn, Sv_corrected=sc, echo_range=rng, sum=ssum, cnt=cnt,
                minmax=(fetch_async(mm) if minmax_async else mm.cpu().tolist()) if want_minmax else None)


# ---- cross-shard edge exchange (pack -> all-reduce -> gather) ------------------------------------------------

def edge_pack(buf, rows, zero_first=True):
    """rows: [(slot, sum (C, R) f32/f64 view with unit inner stride, cnt (C, R) int32 view)] -> slots of ``buf``
    (n_slots, 2, C, R) f64, everything else zero."""
    n_slots, _, C, R = buf.shape
    n = len(rows)
    sums, cnts = (ctypes.c_void_p * max(n, 1))(), (ctypes.c_void_p * max(n, 1))()
    strides, slots = (ctypes.c_longlong * max(n, 1))(), (ctypes.c_int * max(n, 1))()
    dt = None
    for i, (slot, s, c) in enumerate(rows):
        if not (s.is_cuda and c.is_cuda) or tuple(s.shape) != (C, R) or tuple(c.shape) != (C, R):
            raise ValueError(f"edge_pack: row {i} must be a pair of ({C}, {R}) device tensors")
        if s.stride(1) != 1 or c.stride(1) != 1 or s.stride(0) != c.stride(0) or c.dtype != torch.int32 or s.dtype not in _DT:
            raise ValueError("edge_pack: rows need unit inner stride, equal channel strides, f32/f64 sums and int32 counts")
        if dt is not None and s.dtype != dt:
            raise ValueError("edge_pack: rows of mixed dtypes")
        dt = s.dtype
        sums[i], cnts[i], strides[i], slots[i] = s.data_ptr(), c.data_ptr(), s.stride(0), int(slot)
    call("epa_edge_pack", sums, cnts, strides, slots, n, _DT[dt if dt is not None else torch.float64], C, R, n_slots,
         1 if zero_first else 0, _p(buf), _stream())
    return buf


def edge_prepare_max(t):
    """NaN -> -inf in place on an f64 device tensor about to be all-reduced with MAX."""
    if t.dtype != torch.float64:
        raise ValueError("edge_prepare_max: f64 device tensor expected")
    call("epa_edge_prepare_max", _p(t), t.numel(), _stream())
    return t


def edge_gather(buf, group_off, group_slots, n_edges, *, typed=None):
    """Totals of the shared edges from the all-reduced buffer: (n_edges, 2, C, R) f64, or with ``typed`` (a torch
    dtype) the pair (sum (n_edges, C, R) of that dtype, count (n_edges, C, R) int32) that mvbs_finalize takes."""
    n_slots, _, C, R = buf.shape
    dev = buf.device
    if typed is None:
        tot = torch.empty((n_edges, 2, C, R), dtype=torch.float64, device=dev)
        call("epa_edge_gather", _p(buf), n_slots, _p(group_off), _p(group_slots), n_edges, C, R, _p(tot), None, None,
             _lib.F64, _stream())
        return tot
    s = torch.empty((n_edges, C, R), dtype=typed, device=dev)
    c = torch.empty((n_edges, C, R), dtype=torch.int32, device=dev)
    call("epa_edge_gather", _p(buf), n_slots, _p(group_off), _p(group_slots), n_edges, C, R, None, _p(s), _p(c),
         _DT[typed], _stream())
    return s, c


def edge_finalize_mvbs(buf, group_off, group_slots, rows, fill_value=float("nan")):
    """rows: [(edge index, dst (C, R) f32/f64 view with unit inner stride)]: the merged, finalised MVBS of those shared
    edges (10 log10(sum / count) of the all-reduced totals) written straight into the rows ``dst``."""
    n_slots, _, C, R = buf.shape
    n = len(rows)
    if n == 0:
        return
    edges, dsts, strides = (ctypes.c_int * n)(), (ctypes.c_void_p * n)(), (ctypes.c_longlong * n)()
    dt = rows[0][1].dtype
    for i, (e, d) in enumerate(rows):
        if not d.is_cuda or tuple(d.shape) != (C, R) or d.stride(1) != 1 or d.dtype != dt or dt not in _DT:
            raise ValueError(f"edge_finalize_mvbs: row {i} must be a ({C}, {R}) f32/f64 device view with unit inner stride")
        edges[i], dsts[i], strides[i] = int(e), d.data_ptr(), d.stride(0)
    call("epa_edge_finalize_mvbs", _p(buf), n_slots, _p(group_off), _p(group_slots), edges, dsts, strides, n, C, R,
         float(fill_value), _DT[dt], _stream())
