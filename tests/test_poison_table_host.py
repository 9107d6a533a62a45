"""The table of tests/test_gpu_poisoned_buffers.py is complete (no GPU needed): every top-level function of
``echopype_amd/ops.py`` that calls ``torch.empty``, ``torch.empty_like`` or ``_scratch(`` is named by a case of the table
or by ``EXEMPT`` with its reason -- a wrapper added later has to join the table (tests/test_zz_kernel_coverage.py holds the
kernels to the same idea with its ``ALLOWED``) -- and the scratch audit names every buffer ``epa_scratch_bytes`` knows.
``Poisoned``'s handling of the call shapes of ``torch.empty`` is checked on CPU tensors as far as that goes."""
import ast
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# allocating functions of ops.py that no case of the table calls, each with its reason
EXEMPT = {
}


def _allocating_functions():
    tree = ast.parse(open(os.path.join(ROOT, "echopype_amd", "ops.py")).read())
    out = {}
    for node in tree.body:
        if not isinstance(node, ast.FunctionDef):
            continue
        hits = []
        for call in ast.walk(node):
            if not isinstance(call, ast.Call):
                continue
            f = call.func
            if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id == "torch" and \
                    f.attr in ("empty", "empty_like"):
                hits.append(f"torch.{f.attr}")
            elif isinstance(f, ast.Name) and f.id == "_scratch":
                hits.append("_scratch")
        if hits:
            out[node.name] = hits
    return out


def test_every_allocating_wrapper_is_in_the_table_or_exempt():
    import test_gpu_poisoned_buffers as T

    allocating = _allocating_functions()
    assert len(allocating) >= 70 and "sv_power" in allocating and "nasc" in allocating  # (the parse found the wrappers)
    covered = {name for c in T.CASES for name in c.covers}
    unknown = covered - set(allocating)
    assert not unknown, f"the table names functions that allocate nothing (or do not exist): {sorted(unknown)}"
    missing = set(allocating) - covered - set(EXEMPT)
    assert not missing, (f"ops functions that allocate an output or scratch but have no case in "
                         f"tests/test_gpu_poisoned_buffers.py and no reason in EXEMPT: {sorted(missing)}")
    assert all(isinstance(r, str) and r for r in EXEMPT.values())
    both = (set(EXEMPT) & covered)
    assert not both, f"exempt and in the table: {sorted(both)}"


def test_the_table_is_well_formed():
    import test_gpu_poisoned_buffers as T

    names = [c.name for c in T.CASES]
    assert len(set(names)) == len(names)
    kinds = {k: sum(c.kind == k for c in T.CASES) for k in ("base", "degenerate", "zero")}
    print("cases:", len(names), kinds)
    assert kinds["degenerate"] >= 50 and kinds["zero"] >= 40
    assert {c.zero for c in T.CASES if c.kind == "zero"} == {"returns", "raises"}
    assert set(T.FALLBACK) <= set(names)


def test_the_audit_names_every_scratch_buffer_of_the_library():
    import test_gpu_poisoned_buffers as T

    src = open(os.path.join(ROOT, "echopype_amd", "csrc", "runtime.hip")).read()
    table = set(re.findall(r'\{"([a-z0-9_]+\.[a-z0-9_]+)", s::', src))
    assert len(table) >= 29
    assert set(T.AUDIT) == table, (sorted(table - set(T.AUDIT)), sorted(set(T.AUDIT) - table))
    for what, where in T.AUDIT.items():
        assert re.search(r"\.(hip|py)\b", where) or "same" in where, (what, where)


class _FakeOps:
    def __init__(self, torch):
        self.torch = torch
        self._scratch_alloc = lambda nbytes, dtype, device, zero: torch.zeros(-(-nbytes // dtype.itemsize), dtype=dtype,
                                                                                device=device)
        self._scratch = lambda what, device, *a, **k: self._scratch_alloc(16, torch.float64, device, False)


def test_poisoned_passes_cpu_pinned_and_empty_requests_through_and_puts_everything_back():
    import torch

    from poison import BYTES, Poisoned, pattern_values
    import numpy as np

    assert BYTES == (0xA5, 0x5A)
    for dt in (np.float32, np.float64):  # neither pattern is a NaN
        assert all(v == v for v in pattern_values(np, dt))
    assert abs(pattern_values(np, np.float32)[0] + 2.9e-16) < 1e-17 and abs(pattern_values(np, np.float32)[1] - 1.5e16) < 1e15
    ops = _FakeOps(torch)
    before = (torch.empty, torch.empty_like, ops._scratch_alloc, ops._scratch)
    with Poisoned(torch, ops, 0xA5) as p:
        assert torch.empty is not before[0] and ops._scratch_alloc is not before[2]
        for t, shape in ((torch.empty((2, 3), dtype=torch.float64), (2, 3)), (torch.empty(2, 3), (2, 3)),
                         (torch.empty(5, dtype=torch.int32, device="cpu"), (5,)), (torch.empty((0, 4)), (0, 4)),
                         (torch.empty(size=(3,), dtype=torch.uint8), (3,)),
                         (torch.empty_like(torch.zeros(4, 2)), (4, 2))):
            assert tuple(t.shape) == shape and not t.is_cuda
        assert p.bufs == []  # (nothing of it was a device allocation)
    assert (torch.empty, torch.empty_like, ops._scratch_alloc, ops._scratch) == before
    with pytest.raises(ValueError):
        Poisoned(torch, ops, 256)
