"""Every fresh device allocation of ``echopype_amd.ops`` between guard bands and pre-filled with one byte pattern.

What a call returns must be a function of its inputs alone.  ``torch.empty`` hands out whatever the caching allocator
freed last -- very often the right answer of an equal call a moment ago --, so a result element the library never wrote,
or a scratch word it read before writing it, goes unnoticed by a comparison with an oracle.  Under ``Poisoned`` each
such block is filled with a known byte first; the same call under two different bytes (``BYTES``) gives different bits
exactly where the library read memory it had not written.

``Poisoned(torch, ops, byte)`` generalises ``Guard`` of tests/test_gpu_scratch_guard.py (scratch buffers between bands)
and the ``banded`` / ``empty`` pair of the two spectrum tests (outputs between bands) -- it replaces, and puts back on
exit,

- ``ops._scratch_alloc`` (and wraps ``ops._scratch`` for the buffer's name), and
- ``torch.empty`` / ``torch.empty_like`` on the one ``torch`` module every file of the package shares.

A CUDA request becomes ``BAND`` bytes, the payload rounded up to 256 bytes, ``BAND`` bytes, all filled with ``byte``;
the payload starts 256-byte aligned, as torch's own allocations do, and everything behind its last byte -- the round-up
included -- is checked; a ``zero=True`` scratch request is zeroed afterwards
(the library's contract).  CPU and pinned requests, requests of no elements (torch gives those a NULL pointer, which the
library's argument checks see) and call shapes the package does not use (``out=``, a layout, a memory format) go to the
real functions.  Neither byte of ``BYTES`` makes a NaN of a float32 or float64 (0xA5A5A5A5 is about -2.9e-16, 0x5A5A5A5A
about 1.5e16), so an unwritten element shows where the oracle says NaN as well."""
import sys

BAND = 4096
ALIGN = 256
BYTES = (0xA5, 0x5A)


class Poisoned:
    """``with Poisoned(torch, ops, 0xA5) as p: ...; p.check()``."""

    def __init__(self, torch, ops, byte):
        if not 0 <= byte <= 255:
            raise ValueError("a byte is needed")
        self.torch, self.ops, self.byte = torch, ops, int(byte)
        self.bufs = []  # (name, raw uint8 tensor, payload bytes, "out" | "scratch")
        self.what = None
        self.callers = set()  # the functions of ops on the stack of any allocation request (zero-size ones included)

    # ---- the patch ------------------------------------------------------------------------------------------------------
    def __enter__(self):
        torch, ops = self.torch, self.ops
        assert ops.torch is torch, "the package and the test must share one torch module"
        self._saved = (torch.empty, torch.empty_like, ops._scratch_alloc, ops._scratch)
        self._empty, self._empty_like, _, scratch = self._saved

        def named_scratch(what, *args, **kw):
            self.what = what
            try:
                return scratch(what, *args, **kw)
            finally:
                self.what = None

        torch.empty, torch.empty_like = self.empty, self.empty_like
        ops._scratch_alloc, ops._scratch = self.scratch_alloc, named_scratch
        return self

    def __exit__(self, *exc):
        torch, ops = self.torch, self.ops
        torch.empty, torch.empty_like, ops._scratch_alloc, ops._scratch = self._saved
        return False

    def _banded(self, nbytes, device, name, kind):
        """``nbytes`` payload bytes (uint8 view) between two bands, everything filled with the byte."""
        padded = -(-nbytes // ALIGN) * ALIGN
        raw = self._empty(BAND + padded + BAND, dtype=self.torch.uint8, device=device)
        raw.fill_(self.byte)
        mid = raw[BAND:BAND + nbytes]
        assert mid.data_ptr() % ALIGN == 0
        self.bufs.append((name, raw, nbytes, kind))
        return mid

    def _note_callers(self):
        f = sys._getframe(2)
        while f is not None:
            if f.f_globals.get("__name__") == getattr(self.ops, "__name__", None):
                self.callers.add(f.f_code.co_name)
            f = f.f_back

    def _is_cuda(self, device):
        return device is not None and self.torch.device(device).type == "cuda"

    def empty(self, *size, **kw):
        torch = self.torch
        self._note_callers()
        if "size" in kw:
            size = (kw.pop("size"),)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        shape = tuple(int(n) for n in size)
        dtype, device = kw.get("dtype"), kw.get("device")
        numel = 1
        for n in shape:
            numel *= n
        if (not self._is_cuda(device) or kw.get("pin_memory") or numel == 0
                or set(kw) - {"dtype", "device", "pin_memory", "requires_grad"} or kw.get("requires_grad")):
            return self._empty(*size, **kw)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        name = f"{sys._getframe(1).f_code.co_name}: empty({shape}, {dtype})"
        return self._banded(numel * dtype.itemsize, device, name, "out").view(dtype).view(shape)

    def empty_like(self, t, **kw):
        self._note_callers()
        device = kw.get("device", t.device)
        if not self._is_cuda(device) or t.numel() == 0 or set(kw) - {"dtype", "device"} or not t.is_contiguous():
            return self._empty_like(t, **kw)
        dtype = kw.get("dtype") or t.dtype
        name = f"{sys._getframe(1).f_code.co_name}: empty_like({tuple(t.shape)}, {dtype})"
        return self._banded(t.numel() * dtype.itemsize, device, name, "out").view(dtype).view(t.shape)

    def scratch_alloc(self, nbytes, dtype, device, zero):
        self._note_callers()
        n = -(-nbytes // dtype.itemsize) * dtype.itemsize  # what ops._scratch_alloc hands out
        if n == 0:
            return self._saved[2](nbytes, dtype, device, zero)
        mid = self._banded(n, device, self.what or "scratch", "scratch")
        if zero:
            mid.zero_()
        return mid.view(dtype)

    # ---- the verdict ----------------------------------------------------------------------------------------------------
    def check(self):
        """Synchronise; every band intact, or the buffer is named -> (output allocations, scratch allocations)."""
        self.torch.cuda.synchronize()
        for name, raw, n, _ in self.bufs:
            for side, band in (("in front of", raw[:BAND]), ("behind", raw[BAND + n:])):
                bad = (band != self.byte).nonzero()
                assert bad.numel() == 0, (f"{name} ({n} bytes): {bad.numel()} bytes written {side} it, the first at band "
                                          f"offset {int(bad[0])}")
        kinds = [kind for _, _, _, kind in self.bufs]
        return kinds.count("out"), kinds.count("scratch")

    def scratch_names(self):
        return {name for name, _, _, kind in self.bufs if kind == "scratch"}


def pattern_values(np, dtype):
    """The values an element of ``dtype`` left at either byte pattern holds (for the cases that cannot compare bits)."""
    return [np.frombuffer(bytes([b]) * np.dtype(dtype).itemsize, dtype=dtype)[0] for b in BYTES]
