"""csrc/bf16_split.h (the three-bf16-plane split of K1's plane k-step) as a stand-alone program,
tests/host/bf16_split_main.cpp, built with the host compiler under the undefined-behaviour and address
sanitizers.  No GPU and no libdmdx.so: the header compiles alone.

What it holds: h + m + l == x exactly over every normal binade (8, 16 and 24 significant bits), every plane a
bf16 value, the fast and the class-safe form equal on finite input, the class rule for +-Inf and every kind of
NaN, the detector firing exactly on non-finite input, 2^+-40 scaling, and an fp32 emulation of the six plane
products on a small Gram whose classes equal fp64's with the rule and do not with the plain split."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bf16_split_main.cpp")


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_bf16_split_program(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bf16_split")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address",
                            "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("0 failed")
