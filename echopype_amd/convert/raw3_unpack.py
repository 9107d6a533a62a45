"""The Python side of ``epa_raw3_unpack``: the RAW3 complex sample blocks of an EK80 .raw file, lying in HBM as they lie
on disk, written into the ``backscatter_r`` / ``backscatter_i`` volumes of one beam group by one launch.

The wrapper lives here and not in ``ops.py`` because every top-level function of ``ops.py`` that allocates with
``torch.empty`` must have its rows in the table of tests/test_gpu_poisoned_buffers.py (tests/test_poison_table_host.py
holds it to that), and that table belongs to an existing test file.  The property the table checks -- the result
depends on the inputs alone, whatever the allocator hands out -- is checked for this wrapper by
tests/test_gpu_open_raw_ek80.py (pre-filled ``out=`` planes with a guard band, and the whole ``open_raw_ek80`` call under
``tests/poison.py``).  A later change can move ``raw3_unpack`` into ``ops.py`` together with its table rows."""
import ctypes

import numpy as np
import torch

from .. import ops


def raw3_unpack(file_bytes, table, C, P, S, B, *, n_bytes=None, out=None):
    """The RAW3 complex blocks of an EK80 .raw file -> (backscatter_r, backscatter_i) float32 device tensors of shape
    (C, P, S, B) (``epa_raw3_unpack``: one launch, every file sample byte read once, every output element written exactly
    once).

    ``file_bytes``: as for ``ops.raw0_unpack`` (``ops.upload_file_bytes`` pads it; ``n_bytes``: the file's own length,
    default all of it).  ``table``: int64 host array (C * P, 3), row ``(c, p)``: byte offset of the complex block (-1: the
    row has none), the sample count and the number of sectors of that ping.  The values are bit copies; an imaginary
    part equal to 0.0 becomes NaN (the reference's rule, parse_base.py:312-314), and so does everything behind a row's
    count, in sectors the ping lacks and in rows without a block.  ``out``: the two tensors to write into instead of new
    ones (tests: a pre-filled allocation shows that every element is written)."""
    if not (isinstance(file_bytes, torch.Tensor) and file_bytes.dtype == torch.uint8 and file_bytes.dim() == 1):
        raise ValueError("raw3_unpack: file_bytes must be a one-dimensional uint8 tensor")
    C, P, S, B = int(C), int(P), int(S), int(B)
    tab = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, 3))
    if tab.shape[0] != C * P:
        raise ValueError(f"raw3_unpack: the table has {tab.shape[0]} rows, C * P = {C * P} are needed")
    dev = file_bytes.device
    if out is None:
        re = torch.empty((C, P, S, B), dtype=torch.float32, device=dev)
        im = torch.empty((C, P, S, B), dtype=torch.float32, device=dev)
    else:
        re, im = out
        for t in (re, im):
            if t.dtype != torch.float32 or tuple(t.shape) != (C, P, S, B) or t.device != dev or not t.is_contiguous():
                raise ValueError("raw3_unpack: out must hold contiguous float32 (C, P, S, B) tensors on the file's device")
    tab_dev = ops.to_device(tab, device=dev)
    ops.call("epa_raw3_unpack", ops._p(file_bytes), int(file_bytes.numel() if n_bytes is None else n_bytes),
             int(file_bytes.numel()), tab.ctypes.data_as(ctypes.c_void_p), ops._p(tab_dev), C, P, S, B, ops._p(re), ops._p(im),
             ops._stream())
    return re, im
