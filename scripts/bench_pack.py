"""K17 (forecast fields -> CF-packed int16 codes on the device) on one cfg2 row block against what a user of the
library had before it.

For k in {10, 50, 200}, m = 129 780 rows, T = 256 snapshots, mean and std given, in ONE process and alternating:
  range_pack  kern.expand_range(...) then kern.expand_pack(...)     (a) the chain twice, 2 m T bytes written, the
                                                                        packing taken from a range known on the host
  pack        kern.expand_pack(...) with the packing given          (b) the chain once
  old         P = kern.expand(...) (K12) into a (T, m) fp32 buffer, then torch: isfinite / amin / amax, the fp64
              (x - o) / s, round, clamp, where, to(int16)           (c) what the parent commit's entry points allow
Before anything is timed the codes of the three ways are compared: (a) and (b) must be EQUAL to the composition
(the field is K12's bit for bit and the composition's arithmetic is the contract's).
Times are HIP events around batches of calls (>= `--sample-ms` of device time each, per call reported) on the
current stream, `--reps` samples after `--warmup` calls; the minimum, the median and the spread (min .. max) of
each are printed, with the GB/s of the codes (2 m T bytes per call), the algorithmic TFLOP/s (2 m k T per chain, the
unpadded k) and the ratios old / range_pack and old / pack on the medians, on the minima, and the one that cannot
be a timing accident: the composition's fastest sample against K17's slowest.  One JSON line per k.

`--file N` adds the end-to-end comparison: era5_svd.write_forecast_slice of N daily fields of the block against
fields() -> host -> numpy encode -> Writer.dataset, both into files under `--dir` (in the page cache), with the
bytes each moves over PCIe.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd.kernels import default_kernels  # noqa: E402
from dmd_era5_amd.labeled import Packing  # noqa: E402

MFMA_TFLOPS = 157.3

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780)
ap.add_argument("--T", type=int, default=256)
ap.add_argument("--ks", type=int, nargs="+", default=[10, 50, 200])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sample-ms", type=float, default=20.0, help="device time one timed sample should cover")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
ap.add_argument("--file", type=int, default=0, help="snapshots of the end-to-end file comparison (0: skip; 365: a year)")
ap.add_argument("--dir", default="data/bench_pack", help="where the end-to-end files go")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_pack: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
g = torch.Generator(device="cuda").manual_seed(17)
m, T = a.m, a.T
F64 = torch.float64


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    return e0, e1, r


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def torch_range(P):
    fin = torch.isfinite(P)
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=P.device)
    return torch.where(fin, P, inf).amin(), torch.where(fin, P, -inf).amax(), (~fin).sum()


def torch_encode(P, sf, ao):
    fin = torch.isfinite(P)
    r = torch.round((P.to(F64) - ao) / sf)
    sat = fin & ((r < -32767) | (r > 32767))
    q = torch.where(fin, r.clamp(-32767, 32767), torch.tensor(-32768.0, dtype=F64, device=P.device)).to(torch.int16)
    return q, (~fin).sum(), sat.sum()


lines = []
mean = torch.randn(m, generator=g, device=dev, dtype=torch.float32).mul_(10.0).add_(250.0)
std = torch.rand(m, generator=g, device=dev, dtype=torch.float32).mul_(10.0).add_(5.0)
for k in a.ks:
    Ut = torch.randn((k, m), generator=g, device=dev, dtype=torch.float32).mul_(m ** -0.5)
    kp = (k + 3) // 4 * 4                    # every k-vector on a 16-byte boundary: nobody re-pitches while timed
    Ct = torch.randn((T, kp), generator=g, device=dev, dtype=torch.float32).mul_(m ** 0.5)[:, :k]
    P = torch.empty((T, m), dtype=torch.float32, device=dev)
    Q = torch.empty((T, m), dtype=torch.int16, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    rng0, _ = K.expand_range(Ut, Ct, mean, std)
    pk = Packing.for_range(*rng0.tolist())

    def range_pack():
        K.expand_range(Ut, Ct, mean, std)
        return K.expand_pack(Ut, Ct, mean, std, pk, out=Q, counts=counts)[0]

    def pack():
        return K.expand_pack(Ut, Ct, mean, std, pk, out=Q, counts=counts)[0]

    def old():
        K.expand(Ut, Ct, mean, std, out=P)
        torch_range(P)
        return torch_encode(P, pk.scale_factor, pk.add_offset)[0]

    fns = {"range_pack": range_pack, "pack": pack, "old": old}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    want = old().clone()
    lo, hi, _ = torch_range(P)
    same = {"range_equal": bool(lo == rng0[0]) and bool(hi == rng0[1]),
            "range_pack_codes_equal": bool(torch.equal(range_pack(), want)), "pack_codes_equal": bool(torch.equal(pack(), want))}
    torch.cuda.synchronize()
    if not all(same.values()):
        sys.exit(f"bench_pack: the three ways do not give the same codes: {same}")
    del want
    batch = {}
    for name, fn in fns.items():
        e0, e1, _ = timed(fn)
        torch.cuda.synchronize()
        batch[name] = max(1, min(500, int(a.sample_ms / max(e0.elapsed_time(e1), 1e-3)) + 1))

    def many(fn, nb):
        for _ in range(nb):
            fn()

    ev = {name: [] for name in fns}
    for _ in range(a.reps):                 # alternating, in the same process
        for name, fn in fns.items():
            ev[name].append(timed(lambda fn=fn, name=name: many(fn, batch[name]))[:2])
    torch.cuda.synchronize()
    res = {name: stats([e0.elapsed_time(e1) / batch[name] for e0, e1 in ev[name]]) for name in ev}
    line = {"entry": "pack", "m": m, "k": k, "T": T, "reps": a.reps, "calls_per_sample": batch}
    chains = {"range_pack": 2, "pack": 1, "old": 1}
    for name in fns:
        sec = res[name]["median_ms"] * 1e-3
        tf = chains[name] * 2.0 * m * k * T / sec / 1e12
        line[name] = dict(res[name], codes_gbs=2.0 * m * T / sec / 1e9, tflops=tf, fraction_of_mfma_peak=tf / MFMA_TFLOPS)
    line.update({
        "old_over_range_pack_median": res["old"]["median_ms"] / res["range_pack"]["median_ms"],
        "old_over_range_pack_min": res["old"]["min_ms"] / res["range_pack"]["min_ms"],
        "old_min_over_range_pack_max": res["old"]["min_ms"] / res["range_pack"]["max_ms"],
        "old_over_pack_median": res["old"]["median_ms"] / res["pack"]["median_ms"],
        "old_min_over_pack_max": res["old"]["min_ms"] / res["pack"]["max_ms"],
        "same_codes": same,
    })
    print(json.dumps(line), flush=True)
    lines.append(line)
    del Ut, Ct, P, Q

if a.file:
    from dmd_era5_amd import era5_svd, hdf5_lite
    from dmd_era5_amd.bopdmd import OptDMDResult
    from dmd_era5_amd.forecast import DmdForecast

    # one cfg2 row block as a (1 variable, 1 level, 180 x 721) grid; a planted real model of 6 modes at k = 50
    k, n, nlat, nlon = 50, a.file, 180, 721
    assert nlat * nlon == m, "the end-to-end comparison is written for the default block of 129 780 rows"
    rs = np.random.RandomState(17)
    half = np.array([-0.001 + 0.05j, -0.002 + 0.11j, -0.0005 + 0.017j])
    mh = rs.standard_normal((k, 3)) + 1j * rs.standard_normal((k, 3))
    res = OptDMDResult(eigs=torch.from_numpy(np.concatenate([half, half.conj()])).to(dev),
                       modes=torch.from_numpy(np.concatenate([mh, mh.conj()], axis=1)).to(dev),
                       amplitudes=torch.full((6,), float(m) ** 0.5, dtype=F64, device=dev), rel_error=0.0, n_iter=0,
                       converged=True)
    Ut = torch.randn((k, m), generator=g, device=dev, dtype=torch.float32).mul_(m ** -0.5)
    f = DmdForecast([Ut], res, means=[mean], stds=[std])
    t = np.arange(n, dtype=np.float64)
    stamps = np.datetime64("2020-01-01T00", "ns") + np.arange(n) * np.timedelta64(24, "h")
    grid = dict(levels=[1000], latitude=np.linspace(89.5, -89.5, nlat), longitude=np.arange(nlon) * 0.5)
    os.makedirs(a.dir, exist_ok=True)
    new_path, old_path = os.path.join(a.dir, "k17_new.nc"), os.path.join(a.dir, "k17_old.nc")

    def new_way():
        return era5_svd.write_forecast_slice(new_path, f, t, stamps, ["temperature"], **grid)

    def old_way():
        X = f.fields(torch.from_numpy(t))[0].cpu().numpy()                        # 4 m n bytes over PCIe
        fin = np.isfinite(X)
        pk = Packing.for_range(X[fin].min(), X[fin].max())
        q = pk.encode(X).reshape(n, 1, nlat, nlon)
        with hdf5_lite.Writer(old_path) as w:
            w.dataset("time", np.arange(n, dtype=np.int64), ("time",))
            w.dataset("temperature", q, ("time", "level", "latitude", "longitude"),
                      {"scale_factor": np.float64(pk.scale_factor), "add_offset": np.float64(pk.add_offset),
                       "_FillValue": np.int16(-32768)})
        return pk

    wall = {"new": [], "old": []}
    for rep in range(3):
        for name, fn in (("new", new_way), ("old", old_way)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    rn, ro = hdf5_lite.Reader(new_path), hdf5_lite.Reader(old_path)
    equal = bool(np.array_equal(rn.read("temperature"), ro.read("temperature")))
    rn.close()
    ro.close()
    line = {"entry": "write_forecast_slice", "m": m, "k": k, "snapshots": n, "new_s": wall["new"], "old_s": wall["old"],
            "new_pcie_bytes": 2 * m * n, "old_pcie_bytes": 4 * m * n, "file_bytes": os.path.getsize(new_path),
            "codes_equal": equal}
    print(json.dumps(line), flush=True)
    lines.append(line)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
