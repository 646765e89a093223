"""Ingest of one field stored twice: as CF-packed int16 codes and as the decoded float32 values.

file -> centred X in HBM (``era5_svd._upload_variable`` with mean_center, i.e. read + staging + PCIe +
unpack or copy + K5), no SVD, for
  resident   the whole variable in one call (pad4 as main() asks for it);
  streamed   latitude sub-bands of `--piece-gib` each, one call per piece, blocks dropped after each: one
             pass of the forced-streaming path of main() (svd_snapshots_streaming makes 2 to 9 of them).
The two files alternate, `--reps` times after one warm-up call each; every time is a host clock around
work that ends in a device synchronise.  The files were just written, so they are read from the page cache
(as DESIGN section 4's 20-28 GB/s are): what is compared is staging + PCIe + device work, not a disk.

`DMDX_PKG_ROOT=<tree>` times another checkout of the package (the parent commit) on the same files: a tree
without the packed route moves the packed file's bytes through the host cast (and gets wrong values:
`values_ok`, checked by the run that wrote the files, is then false; a run that reuses `--dir` reports null).  One JSON line per (file, path).
"""
import argparse
import datetime
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

PKG_ROOT = os.environ.get("DMDX_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, PKG_ROOT)
os.environ["DMDX_NETCDF_BACKEND"] = "hdf5"

import torch  # noqa: E402

from dmd_era5_amd import era5_svd, hdf5_lite, io_netcdf  # noqa: E402
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000, help="hourly snapshots (1000 of one 0.25-degree level: 4.15 GB as float32)")
ap.add_argument("--nlev", type=int, default=1)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--piece-gib", type=float, default=1.0)
ap.add_argument("--dir", default=None, help="where the two files go (default: a temporary directory, removed afterwards)")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_ingest_packed: no GPU visible (a CPU run measures nothing)")

nlat, nlon, n, nlev = 721, 1440, a.n, a.nlev
root = a.dir or tempfile.mkdtemp(prefix="dmdx_ingest_packed_")
os.makedirs(root, exist_ok=True)
paths = {"packed": os.path.join(root, "packed.nc"), "float32": os.path.join(root, "float32.nc")}
SF, AO, FILL = 0.0018501293483403683, 271.93247, -32767

t0 = time.perf_counter()
if not all(os.path.exists(p) for p in paths.values()):
    rs = np.random.RandomState(0)
    base = rs.standard_normal((8, nlev * nlat * nlon)).astype(np.float32)
    coef = rs.standard_normal((n, 8)).astype(np.float32) * (0.8 ** np.arange(8, dtype=np.float32))
    q = np.empty((n, nlev, nlat, nlon), dtype=np.int16)
    x = np.empty((n, nlev, nlat, nlon), dtype=np.float32)
    for j0 in range(0, n, 50):                                 # (in slabs: the fp64 temporaries of the decode stay small)
        f = (coef[j0:j0 + 50] @ base).astype(np.float64) * 4.0 + AO
        qq = np.clip(np.rint((f - AO) / SF), -32766, 32767).astype(np.int16).reshape(-1, nlev, nlat, nlon)
        q[j0:j0 + 50] = qq
        x[j0:j0 + 50] = (qq.astype(np.float64) * SF + AO).astype(np.float32)
    times = np.datetime64("2019-01-01T00", "ns") + np.arange(n) * np.timedelta64(1, "h")
    hours = ((times - np.datetime64("1970-01-01T00", "ns")) / np.timedelta64(1, "h")).astype(np.int64)
    for kind, arr, attrs in (("packed", q, {"scale_factor": np.float64(SF), "add_offset": np.float64(AO),
                                            "_FillValue": np.int16(FILL)}),
                            ("float32", x, {"_FillValue": np.float32(np.nan)})):   # (as xarray writes every float variable)
        with hdf5_lite.Writer(paths[kind]) as w:
            w.dataset("time", hours, ("time",), {"units": io_netcdf.TIME_UNITS, "calendar": "proleptic_gregorian"})
            w.dataset("level", np.arange(1000, 1000 - 50 * nlev, -50, dtype=np.int64), ("level",))
            w.dataset("latitude", np.linspace(90, -90, nlat), ("latitude",))
            w.dataset("longitude", np.linspace(0, 359.75, nlon), ("longitude",))
            w.dataset("temperature", arr, ("time", "level", "latitude", "longitude"), attrs)
            w.attrs(None, {"source_path": "synthetic", "variables": ["temperature"], "levels": [1000]})
    check = torch.from_numpy(x[7, 0].reshape(-1).copy())
    del q, x, base
else:
    check = None
print(f"# package {PKG_ROOT}; files in {root}: " + ", ".join(f"{k} {os.path.getsize(p) / 1e9:.2f} GB" for k, p in paths.items())
      + f" ({time.perf_counter() - t0:.1f} s)", flush=True)

kern = default_kernels()
dev = torch.device("cuda", torch.cuda.current_device())
has_k14 = hasattr(kern, "unpack_i16_")
dss = {k: io_netcdf.open_dataset(p) for k, p in paths.items()}
lvl, _, take, _ = era5_svd.plan_selection(dss["float32"], None, datetime.timedelta(hours=1))
h = max(1, int(a.piece_gib * (1 << 30)) // (4 * n * nlev * nlon))
pieces = [(j, min(nlat, j + h)) for j in range(0, nlat, h)]


def ingest(kind, streamed):
    """-> (seconds, bytes reported, snapshot 7 as centred + mean, for the value check)."""
    da = dss[kind]["temperature"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    moved, row = 0, None
    for band in (pieces if streamed else [None]):
        st = {"mean": [], "std": []}
        blocks, m_v, nb = era5_svd._upload_variable(da, lvl, take, dev, kern, True, False, st, band, pad4=not streamed)
        moved += nb
        if band is None:
            row = (torch.cat([b[7] for b in blocks])[:m_v] + torch.cat(st["mean"])).cpu()
        del blocks
    torch.cuda.synchronize()
    return time.perf_counter() - t0, moved, row


lines = []
for streamed in (False, True):
    secs = {k: [] for k in paths}
    info = {}
    for rep in range(a.reps + 1):
        for kind in paths:                                     # alternating; rep 0 is the warm-up
            dt, moved, row = ingest(kind, streamed)
            if rep:
                secs[kind].append(dt)
            ok = None
            if row is not None and check is not None:
                ok = bool(torch.allclose(row[: check.numel()], check, rtol=0, atol=2e-3))
            info[kind] = (moved, ok if ok is not None else info.get(kind, (0, None))[1])
    for kind in paths:
        med = statistics.median(secs[kind])
        line = {"bench": "ingest_packed", "file": kind, "path": "streamed" if streamed else "resident",
                "package_has_k14": has_k14, "n": n, "nlev": nlev, "pieces": len(pieces) if streamed else 1,
                "values_GB": 4 * n * nlev * nlat * nlon / 1e9, "reported_GB": info[kind][0] / 1e9,
                "median_s": med, "min_s": min(secs[kind]), "max_s": max(secs[kind]),
                "values_GBps": 4 * n * nlev * nlat * nlon / med / 1e9, "values_ok": info[kind][1]}
        lines.append(line)
        print(json.dumps(line), flush=True)
    print(f"# {'streamed' if streamed else 'resident'}: packed / float32 = "
          f"{statistics.median(secs['packed']) / statistics.median(secs['float32']):.2f}", flush=True)
if a.out:
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
if not a.dir:
    shutil.rmtree(root, ignore_errors=True)
