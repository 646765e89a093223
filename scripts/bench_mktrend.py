"""K32 (dmdx_mk_stats_f32, dmdx_sen_slopes_f32) alone, on one cfg2 row block of index series, against the torch
composition and against K20's one-read rate.

Y is one resident block of series, n time points x 129 780 rows (fp32, finite: normal noise on a trend per row), for
n = 40, 85 and 128 (780, 3570 and 8128 pairs per row).  In ONE process and alternating:
  mk_stats     kern.mk_stats(Y)                                   the integer planes v, S, E, G
  sen_slopes   kern.sen_slopes(Y, years, ranks), J = 4            the four order statistics a fit asks for
  fit          MannKendall.fit([Y], years)                        both kernels and the fp64 torch operations between them
  torch        chunked to fit: the pairwise fp64 slopes -> fp32 -> torch.sort -> gather of the four ranks, and the sum
               of the signs of the differences (S); the (pairs, rows) temporaries of a chunk stay below `--chunk-mb`
  row_missing  kern.row_missing_count(Y)                          K20: the one-read floor of the same block
Conditions, asserted before anything is timed: sen_slopes gives the bits of the composition (finite data: a zero
slope is +0.0, and the float order is the key order) and mk_stats its S.  Times are HIP events around batches of calls on the
current stream (>= `--sample-ms` of device time per sample), `--reps` samples after `--warmup` calls; medians with
min .. max.  One JSON line per variant, also appended to profiles/k32_bench_mktrend.jsonl.  No ratio is asked for: the
lines say what it is.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd import mktrend  # noqa: E402
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780, help="rows of the block")
ap.add_argument("--n", type=int, nargs="+", default=[40, 85, 128], help="time points of a series")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--chunk-mb", type=float, default=1024.0, help="the fp64 slopes of one chunk of the composition")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                             "k32_bench_mktrend.jsonl"),
                help="the JSON lines are appended to this file too ('' switches that off)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_mktrend: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
m = a.m


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


def composition(Y, h, ia, ib, ranks, chunk):
    """-> (slopes (J, m) fp32, S (m,) fp64) by the pairwise slopes, a full sort and a gather, `chunk` rows at a time."""
    out = torch.empty((ranks.shape[0], m), dtype=torch.float32, device=dev)
    S = torch.empty(m, dtype=torch.float64, device=dev)
    for r0 in range(0, m, chunk):
        y = Y[:, r0:r0 + chunk].double()
        d = y[ib] - y[ia]                                        # (pairs, rows)
        S[r0:r0 + chunk] = torch.sign(d).sum(dim=0)
        srt = torch.sort((d / h).float(), dim=0).values
        out[:, r0:r0 + chunk] = torch.gather(srt, 0, ranks[:, r0:r0 + chunk].long())
    return out, S


lines = []
for n in a.n:
    years = 1940.0 + np.arange(n)
    gen = torch.Generator(device=dev).manual_seed(32 + n)
    Y = torch.empty((n, m), dtype=torch.float32, device=dev).normal_(0.0, 1.0, generator=gen)
    Y += torch.empty(m, dtype=torch.float32, device=dev).uniform_(-0.02, 0.04, generator=gen) * \
        torch.arange(n, dtype=torch.float32, device=dev)[:, None]
    N = n * (n - 1) // 2
    ia_h, ib_h = np.triu_indices(n, k=1)
    ia, ib = torch.from_numpy(ia_h).to(dev), torch.from_numpy(ib_h).to(dev)
    h = torch.from_numpy(years[ib_h] - years[ia_h]).to(dev)[:, None]
    chunk = max(1, min(m, int(a.chunk_mb * 2 ** 20 / (8 * N))))
    fit = mktrend.MannKendall.fit([Y], years)
    ranks = mktrend.interval_ranks(fit.stats[0], 0.05).contiguous()
    fns = {"mk_stats": lambda: K.mk_stats(Y),
           "sen_slopes": lambda: K.sen_slopes(Y, years, ranks),
           "fit": lambda: mktrend.MannKendall.fit([Y], years),
           "torch": lambda: composition(Y, h, ia, ib, ranks, chunk),
           "row_missing": lambda: K.row_missing_count(Y)}
    ref, S = fns["torch"]()
    assert torch.equal(fns["sen_slopes"]().view(torch.int32), ref.view(torch.int32)), f"n={n}: not the composition's bits"
    assert torch.equal(fns["mk_stats"]()[1].double(), S), f"n={n}: S is not the composition's"
    del ref, S
    ms, calls = measure(fns)
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name in fns:
        line = {"bench": "mktrend", "variant": name, "n": n, "pairs": N, "m": m, "J": 4, "chunk_rows": chunk,
                "bit_equal_to_composition": True, "median_ms": med[name], "min_ms": min(ms[name]), "max_ms": max(ms[name]),
                "calls_per_sample": calls[name], "x_row_missing": med[name] / med["row_missing"],
                "speedup_vs_torch": med["torch"] / med[name]}
        lines.append(line)
        print(json.dumps(line), flush=True)
    print(f"# n={n}: sen_slopes {med['sen_slopes']:.3f} ms, mk_stats {med['mk_stats']:.3f} ms, fit {med['fit']:.3f} ms, the "
          f"composition {min(ms['torch']):.2f} .. {max(ms['torch']):.2f} ms, row_missing {med['row_missing']:.3f} ms", flush=True)
    del Y, fit, ranks
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
