#!/usr/bin/env python
"""Compare the gfx950 device code of two source trees, function by function.

    python scripts/device_code_diff.py OLD_TREE NEW_TREE [file.hip ...]     (default: build.py's SOURCES)

Each file is compiled to device assembly with build.py's FLAGS of its own tree; every function body and every kernel
descriptor (registers, LDS, scratch, and with it the spill counts of the kernel's metadata and the occupancy the
compiler notes) is then compared as text.  Function-local labels carry the function's ordinal in
the file, which moves when the instantiation order does, so that ordinal is dropped first.  A body that differs is
reported with its instruction count on both sides and the opcodes whose number changed (none: registers renamed or
instructions reordered).  Exit status 1 when a symbol is missing, added or different.  Runs on the CPU: nothing is
launched.
"""
import collections
import os
import re
import runpy
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FUNC = re.compile(r"; -- Begin function (\S+)\n(.*?); -- End function", re.S)
DESC = re.compile(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", re.S)
LOCAL = re.compile(r"(\.LBB|\bBB|\.Lfunc_begin|\.Lfunc_end|\.LJTI)\d+")
BLANKS = re.compile(r"[ \t]+")  # a label's comment is aligned to a column: a longer ordinal moves it
SPILLS = re.compile(r"^    \.(name|sgpr_spill_count|vgpr_spill_count):\s+(\S+)$", re.M)  # of one amdhsa.kernels entry
OCCUPANCY = re.compile(r"\.set (\S+)\.has_indirect_call, \d+\n.*?; Occupancy: (\d+)", re.S)
OPCODE = re.compile(r"^ ([a-z][a-z0-9_]+)\b", re.M)  # (after BLANKS: an instruction line starts with one blank)


def opcode_delta(old_body, new_body):
    """'N -> M instructions' and the opcodes whose count changed, parent against branch."""
    a, b = (collections.Counter(OPCODE.findall(t)) for t in (old_body, new_body))
    moved = " ".join(f"{op}{b[op] - a[op]:+d}" for op in sorted(set(a) | set(b)) if a[op] != b[op])
    return f"{sum(a.values())} -> {sum(b.values())} instructions; {moved or 'same opcodes: registers renamed or reordered'}"


def device_symbols(tree, name):
    build = runpy.run_path(os.path.join(tree, "echopype_amd", "build.py"), run_name="build")
    cmd = [build["_hipcc"](), *build["FLAGS"], "--cuda-device-only", "-S", os.path.join(build["CSRC"], name), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"hipcc failed:\n{' '.join(cmd)}\n{r.stderr}")
    asm = r.stdout
    syms = {"func " + m.group(1): BLANKS.sub(" ", LOCAL.sub(r"\1", m.group(2))) for m in FUNC.finditer(asm)}
    syms.update({"desc " + m.group(1): m.group(2) for m in DESC.finditer(asm)})
    for entry in asm.split("\n  - ")[1:]:
        d = dict(SPILLS.findall(entry))
        if "desc " + d.get("name", "") in syms:
            syms["desc " + d["name"]] += f".sgpr_spill_count {d['sgpr_spill_count']}\n.vgpr_spill_count {d['vgpr_spill_count']}\n"
    for name, occ in OCCUPANCY.findall(asm):
        if "desc " + name in syms:
            syms["desc " + name] += f".occupancy {occ}\n"
    return syms


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    old, new = argv[1], argv[2]
    files = argv[3:] or runpy.run_path(os.path.join(new, "echopype_amd", "build.py"), run_name="build")["SOURCES"]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        olds = list(ex.map(lambda f: device_symbols(old, f), files))
        news = list(ex.map(lambda f: device_symbols(new, f), files))
    bad = bad_desc = 0
    for name, a, b in zip(files, olds, news):
        missing = sorted(set(a) - set(b))
        added = sorted(set(b) - set(a))
        differ = sorted(s for s in set(a) & set(b) if a[s] != b[s])
        for what, syms in (("missing", missing), ("added", added), ("differs", differ)):
            for s in syms:
                note = f": {opcode_delta(a[s], b[s])}" if what == "differs" and s.startswith("func ") else ""
                print(f"{name}: {what}: {s}{note}")
        bad += len(missing) + len(added) + len(differ)
        nfunc = sum(s.startswith("func ") for s in b)
        print(f"{name}: {nfunc} functions, {len(b) - nfunc} kernel descriptors: "
              f"{'identical' if not (missing or added or differ) else 'DIFFERENT'}")
        bad_desc += sum(s.startswith("desc ") for s in missing + added + differ)
    print(f"{bad} differences in {len(files)} files, {bad_desc} of them kernel descriptors")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
