"""csrc/plane_image.h (the bf16 plane images of K1, dmdx_syrk_blocks_planes_f32) as a stand-alone program,
tests/host/plane_image_main.cpp, built with the host compiler under the undefined-behaviour and address sanitizers.
No GPU: the header compiles alone.

What it holds: the piece index is a bijection onto the 1536 pieces of an image and puts the 64 pieces of an operand read
in lane order; the slot formula gives the four dwords the in-kernel split packs (a literal transcription of
DMDX_SPLIT_GROUP); the byte counts of (K, n) = (31, 100), (32, 128), (20 481, 312) and the cfg2 block (129 780, 8760)
by hand; the count saturates near 2^63.  The second test holds the library's dmdx_syrk_planes_bytes to the same
numbers, and the refusals of dmdx_syrk_blocks_planes_f32 that need no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "plane_image_main.cpp")
IMAGE = 24576
SIZE_MAX = (1 << 64) - 1


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_plane_image_program(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "plane_image")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address",
                            "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("plane_image: 0 failed")


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "dmd_era5_amd", "libdmdx.so")
    if not os.path.exists(so):
        import __graft_entry__

        __graft_entry__.build()
    from dmd_era5_amd import _lib

    return _lib.load()


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def test_planes_bytes_of_the_library(lib):
    for K, n, want in [(31, 100, IMAGE), (32, 128, IMAGE), (20481, 312, 3 * 641 * IMAGE), (129780, 8760, 69 * 4056 * IMAGE)]:
        assert lib.dmdx_syrk_planes_bytes(_i64([K]), 1, n) == want
    assert lib.dmdx_syrk_planes_bytes(_i64([129780] * 8), 8, 8760) == 8 * 69 * 4056 * IMAGE == 55023501312
    assert lib.dmdx_syrk_planes_bytes(_i64([20481, 4097, 31]), 3, 312) == 3 * (641 + 129 + 1) * IMAGE
    assert lib.dmdx_syrk_planes_bytes(None, 1, 8) == 0
    assert lib.dmdx_syrk_planes_bytes(_i64([5]), 0, 8) == 0
    assert lib.dmdx_syrk_planes_bytes(_i64([5, 0]), 2, 8) == 0
    assert lib.dmdx_syrk_planes_bytes(_i64([(1 << 63) - 1]), 1, (1 << 62)) == SIZE_MAX
    assert lib.dmdx_syrk_planes_bytes(_i64([1 << 40] * 32), 32, 128000) == SIZE_MAX
    # the entry points and queries that were there keep their numbers
    assert lib.dmdx_version() == 110


def test_refusals_need_no_gpu(lib):
    """Every refusal comes before the first HIP call: made-up device addresses are enough.  X at 2^32, G behind it,
    the workspace and the planes further up."""
    K, n = 4099, 312
    ld = 4100
    X, G, WS, PL = 1 << 32, 1 << 33, 1 << 34, 1 << 35
    ms, lds, ptrs = _i64([K]), _i64([ld]), (C.c_void_p * 1)(X)
    ws_need = lib.dmdx_syrk_blocks_workspace_bytes(ms, 1, n)
    need = lib.dmdx_syrk_planes_bytes(ms, 1, n)
    assert ws_need > 0 and need == 3 * 129 * IMAGE

    def call(planes=PL, planes_bytes=need, nblocks=1, ws=WS, ws_bytes=ws_need, g=G):
        return lib.dmdx_syrk_blocks_planes_f32(ptrs, ms, lds, nblocks, n, g, n, None, 0, 0, ws, ws_bytes, planes,
                                               planes_bytes, None)

    assert call(planes=None) == -1001 and b"plane buffer" in lib.dmdx_last_error()
    assert call(planes_bytes=need - 1) == -1001 and b"plane buffer" in lib.dmdx_last_error()
    assert call(planes_bytes=0) == -1001
    assert call(nblocks=0) == -1000 and b"no blocks" in lib.dmdx_last_error()
    assert call(ws_bytes=ws_need - 1) == -1001 and b"workspace" in lib.dmdx_last_error()
    assert call(planes=PL + 8) == -1000 and b"aligned" in lib.dmdx_last_error()
    x_bytes = 4 * ((n - 1) * ld + K)
    for planes in (X, (X + x_bytes - 16) & ~15, X - need + 16, X + 4096):
        assert call(planes=planes) == -1000 and b"overlaps" in lib.dmdx_last_error(), hex(planes)
    assert call(planes=G + 8 * n * n - 16) == -1000 and b"overlaps" in lib.dmdx_last_error()
    assert call(planes=WS + ws_need - 16) == -1000 and b"overlaps" in lib.dmdx_last_error()
    assert call(planes=WS - need + 16) == -1000 and b"overlaps" in lib.dmdx_last_error()
