"""The host argument checks of K23 (csrc/coarsen_geom.h: check_coarsen, the check_ranges for blocks of different
heights, coarsen_blocks) as a stand-alone program, tests/host/coarsen_checks_main.cpp, built with the host compiler
under the address and undefined-behaviour sanitizers.  No GPU and no libdmdx.so: the header's host half compiles alone.

What this holds that the refusal tests through the library cannot show: the extent arithmetic itself.  Sizes below 2^31
give planes of up to 2^62 points and extents beyond 2^60 elements; a signed overflow anywhere in the checks ends the
program here, a wrong verdict fails one of its cases."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "coarsen_checks_main.cpp")


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_coarsen_checks_program(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "coarsen_checks")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("0 failed")
