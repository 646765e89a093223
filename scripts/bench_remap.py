"""K28 (dmdx_remap_f32) alone, on one row block of cfg2's size, against K23 and a torch composition.

X is one resident row block of the size of cfg2's (4.25 GB fp32): one plane of the whole 0.25 degree ERA5 grid, 721 x 1440
points, ``--T`` = 1024 snapshots -- a remapping onto a global grid needs the poles and the wrap, so the block is a whole
plane and fewer snapshots, not a latitude band and a year.  Variants, in ONE process, alternating:
  k28-1deg       (a) Remap.regular(lat, lon, 1, 1): 181 x 360, spans of 5 x 5, half cells, the wrap, the pole caps
  k28-blocks     (b) Remap.blocks(lat, lon, 4, 4): the tables of K23's 4 x 4 blocks (180 x 360)
  k23            (c) kern.coarsen at 4 x 4, the product build (16-byte loads)
  k23-NAME       (c) the same entry point of another build (``--alt-lib generic=PATH``: the element-by-element walk alone,
                 ``make -C dmd_era5_amd/csrc coarsen-generic``): the yardstick of (b), which does the same loads plus one
                 fp64 multiply per element
  torch          (d) the remapping of (a) by torch operators, ``--chunk`` snapshots at a time: an fp64 copy, two dense
                 products with the weight matrices (181 x 721 and 1440 x 360), a divide and a cast
Conditions, asserted before anything is timed: on the first ``--check-snapshots`` snapshots (a) and (b) give the bits of
tests/remap_ref.py; (b) gives the bits of (c) on the whole block, and so does every other build of (c); (d), which sums in
another order, agrees with (a) within 2^-22 |y|.  Times are HIP events around batches of calls on the current stream
(>= ``--sample-ms`` of device time per sample), ``--reps`` samples after ``--warmup`` calls; medians, minimum and maximum,
with GB/s of the X that is read (4 T nlat nlon bytes for (a) and (d), 4 T 720 x 1440 for (b) and (c)), the fraction of the
6.3 TB/s HBM figure of DESIGN.md that is, and the ratios (a) / (d) and (b) / (c).  One JSON line per variant, also appended
to profiles/k28_bench_remap.jsonl.  The only condition on the rates is that (a) beats (d).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import remap_ref  # noqa: E402
from dmd_era5_amd import _lib  # noqa: E402
from dmd_era5_amd.kernels import default_kernels  # noqa: E402
from dmd_era5_amd.regrid import Remap  # noqa: E402

HBM_TBS = 6.3
T_START = time.time()


def note(msg):
    print(f"# [{time.time() - T_START:7.1f} s] {msg}", file=sys.stderr, flush=True)


ap = argparse.ArgumentParser()
ap.add_argument("--T", type=int, default=1024)
ap.add_argument("--chunk", type=int, default=64, help="snapshots per step of the torch composition")
ap.add_argument("--alt-lib", nargs="*", default=[], metavar="NAME=PATH",
                help="other builds of libdmdx.so whose dmdx_coarsen_f32 is timed beside the product's")
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--check-snapshots", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--tag", default="", help="copied into every line (the build that was measured)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k28_bench_remap.jsonl"),
                help="the JSON lines are appended to this file too ('' switches that off)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_remap: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
nlat, nlon, T, fy, fx = 721, 1440, a.T, 4, 4
m = nlat * nlon
lat, lon = 90.0 - 0.25 * np.arange(nlat), 0.25 * np.arange(nlon)
one = Remap.regular(lat, lon, 1.0, 1.0)
blk = Remap.blocks(lat, lon, fy, fx, weights="band")
alts = {}
for item in a.alt_lib:
    alt_name, alt_path = item.split("=", 1)
    alts[alt_name] = ctypes.CDLL(os.path.abspath(alt_path))
    alts[alt_name].dmdx_coarsen_f32.restype, alts[alt_name].dmdx_coarsen_f32.argtypes = _lib.SIGNATURES["dmdx_coarsen_f32"]

X = torch.empty((T, m), dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(28)
for t0 in range(0, T, 128):                                      # positive values, a few hundred: temperatures
    X[t0:t0 + 128].normal_(270.0, 15.0, generator=gen)


def tables_of(rm):
    return [torch.from_numpy(v).to(dev) for v in (rm.iy0, rm.ny, rm.wy, rm.jx0, rm.nx, rm.wx)]


def dense(first, count, w, n_src):
    M = np.zeros((first.shape[0], n_src))
    for c in range(first.shape[0]):
        for k in range(int(count[c])):
            M[c, (int(first[c]) + k) % n_src] += w[c, k]
    return M


def batch_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(fns):
    calls = {}
    for name, fn in fns.items():
        for _ in range(a.warmup):
            fn()
        calls[name] = max(1, int(a.sample_ms / max(batch_ms(fn, 1), 1e-3)))
    ms = {name: [] for name in fns}
    for _ in range(a.reps):                                      # alternating: all see the same machine
        for name, fn in fns.items():
            ms[name].append(batch_ms(fn, calls[name]))
    return ms, calls


t_one, t_blk = tables_of(one), tables_of(blk)
w_blk = torch.zeros(nlat, dtype=torch.float64, device=dev)       # K23's row weights: those of the blocks, in order; row 720 is dropped
w_blk[:blk.wy.size] = torch.from_numpy(blk.wy.reshape(-1).copy()).to(dev)
Y1 = torch.empty((T, one.rows_out(1)), dtype=torch.float32, device=dev)
Yb = torch.empty((T, blk.rows_out(1)), dtype=torch.float32, device=dev)
Yc = torch.empty_like(Yb)
NLATb, NLONb = blk.shape_out


def k28_one():
    return K.remap(X, 1, nlat, nlon, *t_one, out=Y1)


def k28_blocks():
    return K.remap(X, 1, nlat, nlon, *t_blk, out=Yb)


def k23():
    return K.coarsen(X, 1, nlat, nlon, w_blk, fy, fx, n_lat_out=NLATb, n_lon_out=NLONb, out=Yc)


note("first launches and the checks")
k28_one(), k28_blocks(), k23()
torch.cuda.synchronize()
n = a.check_snapshots
for name, rm, Y in (("k28-1deg", one, Y1), ("k28-blocks", blk, Yb)):
    want = remap_ref.remap(X[:n].cpu().numpy(), 1, nlat, nlon, rm.iy0, rm.ny, rm.wy, rm.jx0, rm.nx, rm.wx)
    assert np.array_equal(Y[:n].cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{name}: not the bits of tests/remap_ref.py"
assert torch.equal(Yb.view(torch.int32), Yc.view(torch.int32)), "k28-blocks: not the bits of K23"
fns, errs = {"k28-1deg": k28_one, "k28-blocks": k28_blocks, "k23": k23}, {}
st = torch.cuda.current_stream().cuda_stream
for alt_name, alt in alts.items():
    Yalt = torch.empty_like(Yc)

    def k23_alt(alt=alt, Yalt=Yalt):
        rc = alt.dmdx_coarsen_f32(X.data_ptr(), T, m, 1, m, nlat, nlon, w_blk.data_ptr(), fy, fx, 0, 0, NLATb, NLONb, 0, 0.0,
                                  Yalt.data_ptr(), NLATb * NLONb, NLATb * NLONb, st)
        assert rc == 0, rc

    k23_alt()
    assert torch.equal(Yalt.view(torch.int32), Yc.view(torch.int32)), f"the build {alt_name} differs"
    fns[f"k23-{alt_name}"] = k23_alt
if not a.no_torch:
    A = torch.from_numpy(dense(one.iy0, one.ny, one.wy, nlat)).to(dev)            # (181, 721)
    Bt = torch.from_numpy(dense(one.jx0, one.nx, one.wx, nlon).T.copy()).to(dev)   # (1440, 360)
    den = torch.outer(A.sum(dim=1), Bt.sum(dim=0))
    Yt = torch.empty_like(Y1)

    def t_comp():
        for t0 in range(0, T, a.chunk):
            x = X[t0:t0 + a.chunk].double().view(-1, nlat, nlon)
            Yt[t0:t0 + a.chunk] = (torch.matmul(A, torch.matmul(x, Bt)) / den).float().view(x.shape[0], -1)
        return Yt

    note("the torch composition")
    t_comp()
    d = (Yt - Y1).abs() / Y1.abs().clamp_min(1e-30)
    errs["torch"] = float(d.max()) / 2.0 ** -22
    assert errs["torch"] <= 1.0, f"torch is {errs['torch']:.3g} of the bound away from the kernel"
    fns["torch"] = t_comp
    del d

note(f"timing {list(fns)}")
ms, calls = measure(fns)
med = {name: statistics.median(v) for name, v in ms.items()}
read = {name: 4 * T * (m if name in ("k28-1deg", "torch") else NLATb * fy * NLONb * fx) for name in fns}
rate = {name: read[name] / med[name] / 1e6 for name in fns}
yard = "k23-generic" if "k23-generic" in fns else "k23"
lines = []
for name in fns:
    line = {"bench": "remap", "variant": name, "nlat": nlat, "nlon": nlon, "T": T, "bits_equal_ref_snapshots": n,
            "err_of_bound": errs.get(name), "calls_per_sample": calls[name], "samples": len(ms[name]), "median_ms": med[name],
            "min_ms": min(ms[name]), "max_ms": max(ms[name]), "GBps_X_read": rate[name], "of_hbm_peak": rate[name] / 1e3 / HBM_TBS,
            "a_over_d": rate["k28-1deg"] / rate["torch"] if "torch" in fns else None,
            "b_over_c": rate["k28-blocks"] / rate[yard], "c_is": yard, "tag": a.tag}
    lines.append(line)
    print(json.dumps(line), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
if "torch" in fns:
    assert rate["k28-1deg"] > rate["torch"], "K28 loses to the torch composition"
