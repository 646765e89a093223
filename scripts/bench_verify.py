"""K16 (area-weighted verification) on one cfg2 row block against what a user of the library had before it.

For k in {10, 50, 200}, m = 129 780 rows, T = 256 snapshots, weights and a climatology given, in ONE process and
alternating:
  verify  kern.verify(Ut, Ct, Xt, mean, std, w, clim)       one launch, X read once, nothing of size m x T stored
  score   kern.expand_score(Ut, Ct, Xt, mean, std)          K12's two unweighted sums at the same shape
  old     P = kern.expand(Ut, Ct, mean, std) (K12) into a (T, m) buffer, then the torch expressions of the six
          weighted sums on it: e = P - X, f = P - clim, a = X - clim in fp32, (w * q).sum(dtype=float64)
Before anything is timed both ways are compared with the fp64 evaluation of the same fp32 inputs, within the
bounds of tests/verify_ref.py (re-derived here in torch: the script does not import the tests).
Times are HIP events around batches of calls (>= `--sample-ms` of device time each, per call reported) on the
current stream, `--reps` samples after `--warmup` calls; the minimum, the median and the spread (min .. max) of
each are printed, with the GB/s of X (4 m T bytes per call), the algorithmic TFLOP/s (2 m k T, the unpadded k) and
its fraction of the 157.3 TFLOP/s fp32 MFMA peak, and the ratios old / verify and verify / score on the medians
and on the minima.  One JSON line per k.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

MFMA_TFLOPS = 157.3
U24 = 2.0 ** -24

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780)
ap.add_argument("--T", type=int, default=256)
ap.add_argument("--ks", type=int, nargs="+", default=[10, 50, 200])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sample-ms", type=float, default=20.0, help="device time one timed sample should cover")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_verify: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
g = torch.Generator(device="cuda").manual_seed(16)
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


def reference(Ut, Ct, Xt, mean, std, w, clim):
    """fp64 sums (6, T) of the fp32 inputs and their bound (tests/verify_ref.py, column sums, R = 128)."""
    k = Ut.shape[0]
    Xh = (Ct.to(F64) @ Ut.to(F64)) * std.to(F64) + mean.to(F64)
    el = (k + 2) * U24 * ((Ct.abs().to(F64) @ Ut.abs().to(F64)) * std.abs().to(F64) + mean.abs().to(F64))
    x, cl, ww = Xt.to(F64), clim.to(F64), w.to(F64)
    e, f, q = (Xh - x).abs(), (Xh - cl).abs(), (x - cl).abs()
    de, df, da = el + U24 * x.abs(), el + U24 * f, U24 * q
    dQ = (2 * e * de + de * de, de, da, 2 * f * df + df * df, 2 * q * da + da * da, f * da + q * df + df * da)
    Qa = (e * e, e, q, f * f, q * q, f * q)
    bound = torch.stack([(ww * d).sum(dim=1) + (128 + 3) * U24 * (ww * v).sum(dim=1) for d, v in zip(dQ, Qa)])
    e, f, q = Xh - x, Xh - cl, x - cl
    sums = torch.stack([(ww * v).sum(dim=1) for v in (e * e, e, q, f * f, q * q, f * q)])
    return sums, bound


lines = []
mean = torch.randn(m, generator=g, device=dev, dtype=torch.float32).mul_(10.0)
std = torch.rand(m, generator=g, device=dev, dtype=torch.float32).mul_(10.0).add_(5.0)
clim = mean + torch.randn(m, generator=g, device=dev, dtype=torch.float32)
w = torch.rand(m, generator=g, device=dev, dtype=torch.float32).mul_(0.95).add_(0.05)       # cos(lat)-like, none masked
for k in a.ks:
    Ut = torch.randn((k, m), generator=g, device=dev, dtype=torch.float32).mul_(m ** -0.5)
    # (T, k) with every k-vector on a 16-byte boundary, as forecast.verify_blocks hands it over, so that neither
    # side re-pitches inside the timed region
    kp = (k + 3) // 4 * 4
    Ct = torch.randn((T, kp), generator=g, device=dev, dtype=torch.float32).mul_(m ** 0.5)[:, :k]
    Xt = K.expand(Ut, Ct, mean, std).add_(torch.randn((T, m), generator=g, device=dev, dtype=torch.float32).mul_(3.0))
    P = torch.empty((T, m), dtype=torch.float32, device=dev)

    def verify():
        return K.verify(Ut, Ct, Xt, mean, std, w, clim)[0]

    def score():
        return K.expand_score(Ut, Ct, Xt, mean, std)[0]

    def old():
        K.expand(Ut, Ct, mean, std, out=P)
        e, f, q = P - Xt, P - clim, Xt - clim
        return torch.stack([(w * v).sum(dim=1, dtype=F64) for v in (e * e, e, q, f * f, q * q, f * q)])

    fns = {"verify": verify, "score": score, "old": old}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    want, bound = reference(Ut, Ct, Xt, mean, std, w, clim)
    vn, on = verify().clone(), old().clone()
    torch.cuda.synchronize()
    agree = {"verify_err_over_bound": float(((vn - want).abs() / bound).max()),
             "old_err_over_bound": float(((on - want).abs() / bound).max())}
    if not (agree["verify_err_over_bound"] <= 1.0 and agree["old_err_over_bound"] <= 1.0):
        sys.exit(f"bench_verify: the two ways do not compute the same sums within the bounds: {agree}")
    del want, bound, vn, on
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
    line = {"entry": "verify", "m": m, "k": k, "T": T, "reps": a.reps, "calls_per_sample": batch}
    for name in fns:
        sec = res[name]["median_ms"] * 1e-3
        tf = 2.0 * m * k * T / sec / 1e12
        line[name] = dict(res[name], x_gbs=4.0 * m * T / sec / 1e9, tflops=tf, fraction_of_mfma_peak=tf / MFMA_TFLOPS)
    line.update({
        "old_over_verify_median": res["old"]["median_ms"] / res["verify"]["median_ms"],
        "old_over_verify_min": res["old"]["min_ms"] / res["verify"]["min_ms"],
        # the comparison that cannot be a timing accident: the composition's fastest sample against K16's slowest
        "old_min_over_verify_max": res["old"]["min_ms"] / res["verify"]["max_ms"],
        "verify_over_score_median": res["verify"]["median_ms"] / res["score"]["median_ms"],
        "verify_over_score_min": res["verify"]["min_ms"] / res["score"]["min_ms"],
        "err_over_bound": agree,
    })
    print(json.dumps(line), flush=True)
    lines.append(line)
    del Ut, Ct, Xt, P

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
