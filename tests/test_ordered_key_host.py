"""The order-preserving keys of csrc/ordered_key.h (every min / max by-product of the library travels as one) as a
stand-alone host program under AddressSanitizer / UBSan: tools/ordered_key_check.cpp includes the header with a plain
C++ compiler and checks its contract for double and float -- exact round trip, strictly increasing over the non-NaN
values with -0.0 below +0.0, no number at a sentinel, +-inf strictly inside them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for cand in (shutil.which("clang++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_keys_keep_their_contract_as_a_stand_alone_program(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (clang++ / g++) for the stand-alone build")
    src = os.path.join(ROOT, "tools", "ordered_key_check.cpp")
    base = [cxx, "-std=c++17", "-O1", "-g", f"-I{os.path.join(ROOT, 'echopype_amd', 'csrc')}", src]
    exe = tmp_path / "ordered_key_check"
    built = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)],
                           capture_output=True, text=True)
    if built.returncode != 0 and any(w in built.stderr.lower() for w in ("asan", "ubsan", "sanitize")):
        # this compiler has no sanitizer runtime to link: the checks themselves still run
        built = subprocess.run(base + ["-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, f"tools/ordered_key_check.cpp does not compile:\n{built.stderr[-3000:]}"
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    out = run.stdout.splitlines()
    assert out[-1] == "ok" and out[0].startswith("double: 12 edge values, 100000 random values")
    assert out[1].startswith("float: 12 edge values, 100000 random values")
