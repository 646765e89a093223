"""K14 (dmdx_unpack_i16_f32) alone, on a time slab for one cfg2 row block, against the torch composition.

A slab of T snapshots of one 721 x 1440 level of int16 codes sits in HBM as the ingest puts it there
(snapshot stride = the whole level); the row block is 129 780 of its space points, `--row0` into the level.
In ONE process and alternating:
  k14    kern.unpack_i16_(codes, lds, 1, block, row0, plane, [0], sf, ao, fills, counter)
  torch  block.copy_((codes[:, row0:row0 + m].to(float64) * sf + ao).to(float32))        (no fill handling)
Both give the same bits (checked once).  Times are HIP events around batches of calls on the current
stream (>= `--sample-ms` of device time per sample), `--reps` samples after `--warmup` calls; median and
spread are printed with GB/s of the bytes the operation needs (2 read + 4 written per element) and the
fraction of the 6.3 TB/s HBM figure of DESIGN.md that is.  `--tstep 3` times the strided gather of a resampling.
One JSON line per variant.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

HBM_TBS = 6.3
SF, AO = 0.0018501293483403683, 271.93247

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--plane", type=int, default=721 * 1440)
ap.add_argument("--row0", type=int, nargs="+", default=[0, 4 * 129780, 4 * 129780 + 3],
                help="first row of the block inside the level (the last default: a source that is not 16-byte aligned)")
ap.add_argument("--T", type=int, default=128, help="snapshots of the slab")
ap.add_argument("--tstep", type=int, default=1)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_unpack: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
m, T, plane = a.m, a.T, a.plane
nsrc = (T - 1) * a.tstep + 1
codes = torch.randint(-32766, 32767, (nsrc, plane), dtype=torch.int16, device=dev)
counter = torch.zeros(1, dtype=torch.int64, device=dev)
block = torch.empty((T, m), dtype=torch.float32, device=dev)
other = torch.empty_like(block)
nbytes = 6 * m * T


def batch_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


lines = []
for row0 in a.row0:
    def k14():
        K.unpack_i16_(codes.reshape(-1), plane, a.tstep, block, row0, plane, [0], SF, AO, (-32767,), counter)

    def composed():
        other.copy_((codes[::a.tstep, row0:row0 + m].to(torch.float64) * SF + AO).to(torch.float32))

    k14()
    composed()
    torch.cuda.synchronize()
    same = bool(torch.equal(block.view(torch.int32), other.view(torch.int32)))
    fns = {"k14": k14, "torch": composed}
    calls = {}
    for name, fn in fns.items():
        for _ in range(a.warmup):
            fn()
        calls[name] = max(1, int(a.sample_ms / max(batch_ms(fn, 3), 1e-3)))
    ms = {name: [] for name in fns}
    for _ in range(a.reps):                      # alternating: both see the same machine
        for name, fn in fns.items():
            ms[name].append(batch_ms(fn, calls[name]))
    for name in fns:
        med = statistics.median(ms[name])
        line = {"bench": "unpack", "variant": name, "m": m, "T": T, "tstep": a.tstep, "row0": row0,
                "source_16B_aligned": (row0 * 2) % 16 == 0, "bit_equal": same, "calls_per_sample": calls[name],
                "median_ms": med, "min_ms": min(ms[name]), "max_ms": max(ms[name]),
                "GBps": nbytes / med / 1e6, "of_hbm_peak": nbytes / med / 1e6 / (HBM_TBS * 1e3)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    print(f"# row0 {row0}: K14 is {statistics.median(ms['torch']) / statistics.median(ms['k14']):.2f}x the torch "
          f"composition; fills counted so far {int(counter.item())}", flush=True)
if a.out:
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
