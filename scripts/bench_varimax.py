"""K30 (varimax_step) on a U of cfg2's size against the torch composition and against a plain one-read kernel.

For k in {10, 20, 32, 50, 64}, m = 1 038 240 rows, in ONE process and alternating:
  new    kern.varimax_step(Ut, Rt)                                U read once, L never stored, k^2 + 2 k numbers out
  old    L = R^T U^T; G = (L L L) U; q = sum L L; f = sum (L L)(L L)   torch: L and its powers are temporaries of U's
         size, U is read twice, the products go through the BLAS library
  read   kern.row_missing_count(Ut)                               K20: one read of the same bytes, nothing else
Times are HIP events around batches of calls (>= `--sample-ms` of device time each, per call reported), `--reps`
samples after `--warmup` calls; median and the spread (min .. max) are printed, with the fraction of
max(bytes / 6.3 TB/s, flops / 157.3 TFLOP/s) the new kernel reaches (bytes: 4 m k; flops: 4 m k_pad^2, k_pad = k rounded
up to 32).  One JSON line per k.

Then a whole rotation to convergence (`orthomax_blocks`, structured loadings with noise, k = `--rot-k`), with the
parts of a step shown separately: the kernel (HIP events of the provider), the k x k host SVD and the device-to-host copy
of the k^2 + 2 k doubles (both timed on their own, per step).
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
from dmd_era5_amd.rotation import orthomax_blocks  # noqa: E402

HBM_TBS, MFMA_TFLOPS = 6.3, 157.3

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=1038240)
ap.add_argument("--ks", type=int, nargs="+", default=[10, 20, 32, 50, 64])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sample-ms", type=float, default=20.0, help="device time one timed sample should cover")
ap.add_argument("--rot-k", type=int, default=20)
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_varimax: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
g = torch.Generator(device="cuda").manual_seed(30)
m = a.m


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    return e0, e1, r


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


lines = []
for k in a.ks:
    Ut = torch.randn((k, m), generator=g, device=dev, dtype=torch.float32).mul_(m ** -0.5)
    Rt = torch.linalg.qr(torch.randn((k, k), generator=g, device=dev, dtype=torch.float32))[0].contiguous()

    def new():
        return K.varimax_step(Ut, Rt)

    def old():
        L = Rt @ Ut                      # (k, m): row c = column c of L = U R
        L2 = L * L
        return ((L2 * L) @ Ut.T).double(), L2.sum(dim=1, dtype=torch.float64), (L2 * L2).sum(dim=1, dtype=torch.float64)

    def read():
        return K.row_missing_count(Ut)

    fns = {"new": new, "old": old, "read": read}
    kp = (k + 31) // 32 * 32
    flops, nbytes = 4.0 * m * kp * kp, 4.0 * m * k
    bound_ms = max(nbytes / (HBM_TBS * 1e12), flops / (MFMA_TFLOPS * 1e12)) * 1e3
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    (Gn, qn, fn_), (Go, qo, fo) = new(), old()
    torch.cuda.synchronize()
    dev_rel = {"G": float((Gn - Go).abs().max() / Go.abs().max()), "q": float(((qn - qo).abs() / qo).max()),
               "f": float(((fn_ - fo).abs() / fo).max())}
    del Gn, qn, fn_, Go, qo, fo
    batch = {}
    for w, fn in fns.items():
        e0, e1, _ = timed(fn)
        torch.cuda.synchronize()
        batch[w] = max(1, min(500, int(a.sample_ms / max(e0.elapsed_time(e1), 1e-3)) + 1))

    def many(fn, nb):
        for _ in range(nb):
            fn()

    ev = {w: [] for w in fns}
    for _ in range(a.reps):                 # alternating, in the same process
        for w, fn in fns.items():
            ev[w].append(timed(lambda: many(fn, batch[w]))[:2])
    torch.cuda.synchronize()
    res = {w: stats([e0.elapsed_time(e1) / batch[w] for e0, e1 in ev[w]]) for w in ev}
    line = {
        "entry": "varimax_step", "m": m, "k": k, "reps": a.reps, "calls_per_sample": batch,
        "new": res["new"], "old": res["old"], "read": res["read"],
        "bound_ms": bound_ms, "bound_by": "bytes" if nbytes / HBM_TBS / 1e12 >= flops / MFMA_TFLOPS / 1e12 else "flops",
        "new_fraction_of_bound": bound_ms / res["new"]["median_ms"],
        "new_tb_per_s": nbytes / res["new"]["median_ms"] / 1e9, "read_tb_per_s": nbytes / res["read"]["median_ms"] / 1e9,
        "new_over_read": res["new"]["median_ms"] / res["read"]["median_ms"],
        "speedup_median": res["old"]["median_ms"] / res["new"]["median_ms"],
        # the condition of the measurement: faster by more than the spread of the composition's own timings
        "faster_beyond_old_spread": res["old"]["min_ms"] - res["new"]["max_ms"] > 0
        and res["old"]["median_ms"] - res["new"]["median_ms"] > res["old"]["max_ms"] - res["old"]["min_ms"],
        "max_rel_difference_new_vs_old": dev_rel,
        "workspace_bytes": int(K._lib.dmdx_varimax_workspace_bytes(m, k)),
    }
    print(json.dumps(line), flush=True)
    lines.append(line)
    del Ut
    torch.cuda.empty_cache()

# ---- a whole rotation to convergence
k = a.rot_k
simple = torch.zeros((m, k), device=dev, dtype=torch.float32)
col = torch.randint(0, k, (m, 1), generator=g, device=dev)
simple.scatter_(1, col, torch.rand((m, 1), generator=g, device=dev, dtype=torch.float32).add_(0.5))
simple.add_(torch.randn((m, k), generator=g, device=dev, dtype=torch.float32), alpha=0.02)
Q = torch.linalg.qr(torch.randn((k, k), generator=g, device=dev, dtype=torch.float32))[0]
Ut = (Q @ simple.T).mul_(m ** -0.5).contiguous()
del simple, col
for normalize in (False, True):
    orthomax_blocks([Ut], normalize=normalize, max_iter=3, tol=0, kern=K)          # warm: workspaces, libraries
    torch.cuda.synchronize()
    K.events = []
    t0 = time.perf_counter()
    rot = orthomax_blocks([Ut], normalize=normalize, kern=K)
    torch.cuda.synchronize()
    total_ms = (time.perf_counter() - t0) * 1e3
    kernel_ms = {}
    for name, _, e0, e1 in K.events:
        kernel_ms[name] = kernel_ms.get(name, 0.0) + e0.elapsed_time(e1)
    K.events = None
    B = np.random.default_rng(0).standard_normal((k, k))
    t0 = time.perf_counter()
    for _ in range(50):
        u, sig, vh = np.linalg.svd(B)
        u @ vh
    svd_ms = (time.perf_counter() - t0) * 1e3 / 50
    v = torch.zeros(k * k + 2 * k, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        v.cpu()
    d2h_ms = (time.perf_counter() - t0) * 1e3 / 50
    evals = rot.iterations + 1
    line = {"entry": "orthomax_blocks", "m": m, "k": k, "normalize": normalize, "iterations": rot.iterations,
            "converged": rot.converged, "total_ms": total_ms, "kernel_ms_total": kernel_ms,
            "step_kernel_ms_each": kernel_ms.get("varimax_step", 0.0) / evals, "host_svd_ms_each": svd_ms,
            "d2h_copy_ms_each": d2h_ms, "ms_per_step_all_in": total_ms / evals,
            "criterion_first_last": [float(rot.criterion[0]), float(rot.criterion[-1])]}
    print(json.dumps(line), flush=True)
    lines.append(line)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
