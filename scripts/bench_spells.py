"""K27 (dmdx_spell_f32) alone, on one cfg2 row block, against the torch composition and the one-read stream next door.

X is one resident row block, 129 780 rows x 8760 hourly snapshots (4.55 GB fp32), one period (the year).  In ONE process
and alternating:
  split-J{1,2,4}-S366   kern.spells with J thresholds in day-of-year slots (the slot changes every 24 snapshots): time
                        split into pieces of SEGMENT snapshots through the workspace, records merged in order
  split-J1-S1           one slot: the thresholds are loaded once per piece
  split-J1-S8784        day-of-year x hour slots: the thresholds change with every snapshot (a second X of traffic)
  walk-J1-S366          workspace == NULL: one lane walks the year of its rows (one workgroup row)
  k20-count             kern.row_missing_count(X): the project's one-read stream over the same block
  torch                 (``--torch``) gather thr[slot] to a (T, m) field, compare, cumsum with resets through cummax,
                        reductions: n_event, n_spell, n_in_spell and longest of ONE threshold (13.7 GB of temporaries)
Conditions, asserted before anything is timed: split and walk give equal planes, every seg of (64, SEGMENT, T) gives
equal planes, and with ``--torch`` the four planes of the composition equal the kernel's.  Times are HIP events around
batches of calls on the current stream (>= ``--sample-ms`` of device time per sample), ``--reps`` samples after
``--warmup`` calls; medians, minimum and maximum, with GB/s of one read of X, the fraction of the 6.3 TB/s HBM figure
of DESIGN.md that is, and the ratio to K20's rate in the same run.  One JSON line per variant; ``--out FILE`` appends
them to a file too (profiles/k27_bench_spells.jsonl holds the run MEASUREMENTS.md cites and is not written by default).
No bar is set: nobody has measured this kernel before.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd import _lib  # noqa: E402
from dmd_era5_amd.climatology import slots_of  # noqa: E402
from dmd_era5_amd.kernels import default_kernels  # noqa: E402
from dmd_era5_amd.spells import SEGMENT  # noqa: E402

HBM_TBS = 6.3

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--T", type=int, default=8760, help="hourly snapshots from 2019-01-01T00")
ap.add_argument("--min-len", type=int, default=6)
ap.add_argument("--torch", action="store_true", help="time the torch composition too (three (T, m) temporaries)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--out", default="", help="append the JSON lines to this file too (default: print only)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_spells: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
m, T, ML = a.m, a.T, a.min_len
X = torch.empty((T, m), dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(27)
X[0].normal_(0.0, 1.0, generator=gen)
for t in range(1, T):                                            # AR(1), phi = 0.9: runs of many lengths
    X[t].normal_(0.0, 0.436, generator=gen).add_(X[t - 1], alpha=0.9)
times = np.datetime64("2019-01-01T00", "h") + np.arange(T) * np.timedelta64(1, "h")
bounds = [0, T]
levels = torch.tensor([1.2816, -1.2816, 0.0, 0.6745], device=dev)        # the 90th, 10th, 50th and 75th percentile
above = [True, False, True, True]


def table(J, S):
    g = torch.Generator(device=dev).manual_seed(S)
    return (levels[:J, None, None] + 0.05 * torch.randn((J, S, m), generator=g, device=dev)).contiguous()


def labels(kind):
    return None if kind is None else torch.from_numpy(slots_of(times, kind)[0]).to(dev)


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


def walk(thr, slot, out):
    """The C entry point with workspace == NULL (the wrapper always splits a year)."""
    J, S = int(thr.shape[0]), int(thr.shape[1])
    rc = K._lib.dmdx_spell_f32(X.data_ptr(), m, T, m, thr.data_ptr(), m, J, S, None if slot is None else slot.data_ptr(),
                               sum(1 << j for j in range(J) if above[j]), (ctypes.c_int32 * J)(*([ML] * J)),
                               (ctypes.c_int32 * 2)(0, T), 1, SEGMENT, out.data_ptr(), m, 0, None, 0,
                               torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "dmdx_spell_f32")
    return out


def composition(thr1, slot):
    """n_event, n_spell, n_in_spell, longest of threshold 0 (above) over the one period, in torch."""
    h = thr1[0] if slot is None else thr1[slot.long()]           # (T, m): a second X
    e = torch.isfinite(X) & (X > h)
    del h
    c = e.to(torch.int32).cumsum(dim=0, dtype=torch.int32)
    run = c - torch.where(e, torch.zeros_like(c), c).cummax(dim=0).values          # the length of the run that ends at t
    del c
    ends = e.clone()
    ends[:-1] &= ~e[1:]
    q = ends & (run >= ML)
    return torch.stack([e.sum(dim=0, dtype=torch.int32), q.sum(dim=0, dtype=torch.int32),
                        torch.where(q, run, torch.zeros_like(run)).sum(dim=0, dtype=torch.int32), run.max(dim=0).values])


doy, doyh = labels("dayofyear"), labels("dayofyear_hour")
cases = {"split-J1-S366": (table(1, 366), doy), "split-J2-S366": (table(2, 366), doy), "split-J4-S366": (table(4, 366), doy),
         "split-J1-S1": (table(1, 1), None), "split-J1-S8784": (table(1, 8784), doyh)}
outs = {name: torch.empty((thr.shape[0], 7, 1, m), dtype=torch.int32, device=dev) for name, (thr, _) in cases.items()}
fns = {}
for name, (thr, slot) in cases.items():
    J = int(thr.shape[0])
    fns[name] = (lambda thr=thr, slot=slot, J=J, name=name:
                 K.spells(X, thr, bounds, ML, above[:J], slot=slot, seg=SEGMENT, out=outs[name]))
thr1, out_walk = cases["split-J1-S366"][0], torch.empty((1, 7, 1, m), dtype=torch.int32, device=dev)
fns["walk-J1-S366"] = lambda: walk(thr1, doy, out_walk)
count = torch.zeros(m, dtype=torch.int32, device=dev)
fns["k20-count"] = lambda: K.row_missing_count(X, out=count)

ref = fns["split-J1-S366"]().clone()
assert torch.equal(ref, walk(thr1, doy, out_walk)), "split and walk differ"
for seg in (64, T):
    assert torch.equal(ref, K.spells(X, thr1, bounds, ML, True, slot=doy, seg=seg)), f"seg = {seg} differs"
four = fns["split-J4-S366"]()
assert torch.equal(four[0], K.spells(X, cases["split-J4-S366"][0][:1].contiguous(), bounds, ML, True, slot=doy)[0])
torch_equal = None
if a.torch:
    got = composition(thr1[0], doy)
    torch_equal = bool(torch.equal(got, ref[0, 1:5, 0]))
    assert torch_equal, "the torch composition and the kernel differ"
    del got
    fns["torch"] = lambda: composition(thr1[0], doy)
spell_rows = {"rows_with_a_spell": int((ref[0, 2, 0] > 0).sum()), "longest": int(ref[0, 4, 0].max()),
              "mean_n_event": float(ref[0, 1, 0].double().mean())}

ms, calls = measure(fns)
med = {name: statistics.median(v) for name, v in ms.items()}
nbytes = 4 * m * T
lines = []
for name in fns:
    thr, slot = cases.get(name, (thr1 if name.startswith("walk") else None, None))
    line = {"bench": "spells", "variant": name, "m": m, "T": T, "seg": SEGMENT, "min_len": ML,
            "J": None if thr is None else int(thr.shape[0]), "S": None if thr is None else int(thr.shape[1]),
            "split_walk_seg_equal": True, "torch_equal": torch_equal, **spell_rows,
            "calls_per_sample": calls[name], "median_ms": med[name], "min_ms": min(ms[name]), "max_ms": max(ms[name]),
            "GBps": nbytes / med[name] / 1e6, "of_hbm_peak": nbytes / med[name] / 1e9 / HBM_TBS,
            "of_k20_rate": med["k20-count"] / med[name],
            "speedup_vs_torch": med["torch"] / med[name] if "torch" in med else None}
    lines.append(line)
    print(json.dumps(line), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
