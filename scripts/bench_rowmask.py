"""K20 (dmdx_row_missing_count_f32 / dmdx_row_mask_apply_f32) alone, on one cfg2 row block, against the torch
compositions.

X is one resident row block, 129 780 rows x 8760 snapshots (4.55 GB fp32), with `--masked` (30 %) of the rows NaN in
every snapshot: a static land mask, in runs of neighbouring rows as a coast line cuts them (`--scatter`: every row
drawn on its own, the worst case for the stores of apply).  In ONE process and alternating:
  count  k20    kern.row_missing_count(X)                          one read of X, m ints
         torch  torch.isfinite(X).logical_not().sum(0)            two n x m bool temporaries, two more passes
  apply  k20    kern.row_mask_apply_(X, count, 0.0)               the stores of the masked rows
         torch  X[:, mask] = 0                                    an index kernel, a host round trip for the indices
Conditions, asserted before anything is timed: equal counts; equal bits of X after apply.  Times are HIP events around
batches of calls on the current stream (>= `--sample-ms` of device time per sample), `--reps` samples after `--warmup`
calls; medians, with GB/s of the bytes the operation needs (count: one read of X; apply: one store of the masked
rows) and the peak memory each variant allocates beyond what is resident (torch.cuda.max_memory_allocated).  One JSON
line per variant (`--out FILE` appends them to a file as well); the process fails when K20 is slower than the
composition measured in the same run, or allocates anything that grows with n x m.
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

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--n", type=int, default=8760, help="snapshots")
ap.add_argument("--masked", type=float, default=0.3, help="share of the rows that is missing")
ap.add_argument("--run", type=int, default=40, help="mean length of a run of masked rows")
ap.add_argument("--scatter", action="store_true", help="mask every row on its own instead of in runs")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--out", default="", help="append the JSON lines to this file too")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_rowmask: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
m, n = a.m, a.n
gen = torch.Generator(device=dev).manual_seed(20)
X = torch.empty((n, m), dtype=torch.float32, device=dev)
for t0 in range(0, n, 1024):
    X[t0:t0 + 1024].normal_(285.0, 10.0, generator=gen)
if a.scatter:
    mask = torch.rand(m, generator=gen, device=dev) < a.masked
else:                                                            # runs: a two-state chain with the asked share and run length
    u = torch.rand(m, generator=gen, device=dev).cpu().tolist()
    leave, enter = 1.0 / a.run, a.masked / (1.0 - a.masked) / a.run
    state, on = [], bool(u[0] < a.masked)
    for i in range(m):
        on = (u[i] >= leave) if on else (u[i] < enter)
        state.append(bool(on))
    mask = torch.tensor(state, device=dev)
X[:, mask] = float("nan")
n_masked = int(mask.sum())
Xk, Xt = X.clone(), X.clone()
torch.cuda.synchronize()


def batch_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def peak_extra_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def measure(fns):
    calls = {}
    for name, fn in fns.items():
        for _ in range(a.warmup):
            fn()
        calls[name] = max(1, int(a.sample_ms / max(batch_ms(fn, 1), 1e-3)))
    ms = {name: [] for name in fns}
    for _ in range(a.reps):                                      # alternating: both see the same machine
        for name, fn in fns.items():
            ms[name].append(batch_ms(fn, calls[name]))
    return ms, calls


def k_count():
    return K.row_missing_count(X)


def t_count():
    return torch.isfinite(X).logical_not().sum(0)


count = k_count()
assert torch.equal(count.long(), t_count()), "the counts differ"
assert torch.equal(count != 0, mask) and int(count.max()) == n


def k_apply():
    return K.row_mask_apply_(Xk, count, 0.0)


def t_apply():
    Xt[:, mask] = 0.0


k_apply()
t_apply()
torch.cuda.synchronize()
same = bool(torch.equal(Xk.view(torch.int32), Xt.view(torch.int32)))
assert same, "apply does not give the bits of X[:, mask] = 0"

lines, missed = [], []
for op, fns, nbytes in (("count", {"k20": k_count, "torch": t_count}, 4 * m * n),
                        ("apply", {"k20": k_apply, "torch": t_apply}, 4 * n_masked * n)):
    extra = {name: peak_extra_bytes(fn) for name, fn in fns.items()}
    ms, calls = measure(fns)
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name in fns:
        line = {"bench": "rowmask", "op": op, "variant": name, "m": m, "n": n, "masked_rows": n_masked,
                "runs": not a.scatter, "apply_bit_equal": same, "calls_per_sample": calls[name], "median_ms": med[name],
                "min_ms": min(ms[name]), "max_ms": max(ms[name]), "GBps": nbytes / med[name] / 1e6,
                "of_hbm_peak": nbytes / med[name] / 1e9 / HBM_TBS, "peak_extra_bytes": extra[name],
                "speedup_vs_torch": med["torch"] / med[name]}
        lines.append(line)
        print(json.dumps(line), flush=True)
    ratio = med["torch"] / med["k20"]
    print(f"# {op}: K20 is {ratio:.2f}x the torch composition; extra memory {extra['k20']} B against {extra['torch']} B",
          flush=True)
    if ratio < 1.0:
        missed.append(f"{op}: {ratio:.2f}x the torch composition")
    if extra["k20"] > 8 * m + (1 << 20):
        missed.append(f"{op}: K20 allocated {extra['k20']} bytes")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
if missed:
    sys.exit("bench_rowmask: the acceptance is missed: " + "; ".join(missed))
