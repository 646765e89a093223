"""The host argument checks of the time-axis kernels (csrc/time_rows.h: check_block, check_ranges, chunks_of,
grid_rows) as a stand-alone program, tests/host/check_ranges_main.cpp, built with the host compiler under the
undefined-behaviour and address sanitizers.  No GPU and no libdmdx.so: the header's host half compiles alone.

What this holds that the GPU refusal tests cannot show: the extent arithmetic of the overlap test itself.  Sizes
below 2^31 give extents up to 2^62 elements, 4 times that wraps; a signed overflow anywhere in the check ends the
program here, a wrong verdict fails one of its cases."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "check_ranges_main.cpp")


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_check_ranges_program(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "check_ranges")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address",
                            "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("0 failed")
