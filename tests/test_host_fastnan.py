"""The premise of K1's unit-end verdict (csrc/bf16_split.h, gemm_tn.hip) as a stand-alone program,
tests/host/bf16_fastnan_main.cpp, built with the host compiler under the undefined-behaviour and address sanitizers.
No GPU and no libdmdx.so: the header compiles alone.

What it holds: for all 2^24 fp32 patterns with an all-ones exponent the fast split leaves a bf16 NaN in the value's
half of the packed l plane and leaves the finite neighbour in the other half alone; the class rule of the rerun is
the identity on the fast planes of finite values."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bf16_fastnan_main.cpp")


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_bf16_fastnan_program(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bf16_fastnan")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address",
                            "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("0 failed")
    assert run.stdout.startswith("16777216 non-finite patterns")
