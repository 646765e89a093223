"""K24 (exceedance probability, Brier sums and counts) on one cfg2 row block against what it replaces and against
its natural bound.

For k in {20, 50, 200}, B in {16, 100} and J in {1, 4} thresholds (S = 4 slots), m = 129 780 rows, T = 32 lead times,
in ONE process and alternating:
  k24     kern.exceed_score(Ut, Cm, Xt, thr, slot, True, mean, std, w)   one launch (+ three small reduce kernels),
          no member field stored
  prob    kern.exceed_prob(Ut, Cm, thr, slot, True, mean, std, out=P)    the J probability planes
  old     the composition on the entry points that existed before: B x kern.expand (K12) into a (B, T, m) stack, and
          per threshold (stack > thr).sum(members), X > thr, p = c / B, the four quantities, (w * q).sum(float64) per
          lead time and a bincount of (o, c) over the selected elements (the per-element thresholds thr[j, slot] are
          gathered once, outside the timed region)
  k15     kern.spread_score(Ut, Cm, std) at the same (k, B): the same B chains per tile and one quantity, K24's bound
The expectation to test: k24 at J = 4 ~ k24 at J = 1 ~ k15.  Nothing is asserted; the ratios are recorded.
k24 and old are first compared with each other: the counts must be equal (both count the fp32 fields of K12) and the
largest relative difference of the column sums is reported.
Times are HIP events around batches of calls (>= `--sample-ms` of device time each, per call reported) on the
current stream, `--reps` samples after `--warmup` calls, alternating; the median and the spread (min .. max) of each
are printed.  One JSON line per (k, B, J).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=129780)
ap.add_argument("--T", type=int, default=32)
ap.add_argument("--S", type=int, default=4)
ap.add_argument("--Js", type=int, nargs="+", default=[1, 4])
ap.add_argument("--Bs", type=int, nargs="+", default=[16, 100])
ap.add_argument("--ks", type=int, nargs="+", default=[20, 50, 200])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sample-ms", type=float, default=20.0, help="device time one timed sample should cover")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_exceed: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
g = torch.Generator(device="cuda").manual_seed(24)
m, T, S = a.m, a.T, a.S
Z = (-1.0, 0.0, 0.5, 1.2816)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    return e0, e1, r


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


lines = []
std = torch.rand(m, generator=g, device=dev, dtype=torch.float32).mul_(10.0).add_(5.0)
mean = torch.randn(m, generator=g, device=dev, dtype=torch.float32).mul_(30.0)
w = torch.rand(m, generator=g, device=dev, dtype=torch.float32)
w[torch.rand(m, generator=g, device=dev) < 0.1] = 0.0          # a mask
slot = torch.randint(0, S, (T,), generator=g, device=dev).to(torch.int32)
sel = w != 0
wsel = w[sel]
for k in a.ks:
    for B in a.Bs:
        Ut = torch.randn((k, m), generator=g, device=dev, dtype=torch.float32).mul_(m ** -0.5)
        # (B, T, k) with every k-vector on a 16-byte boundary, as forecast.exceed_blocks hands it over
        kp = (k + 3) // 4 * 4
        common = torch.randn((1, T, kp), generator=g, device=dev, dtype=torch.float32).mul_(m ** 0.5)
        Cm = (common + 0.3 * m ** 0.5 * torch.randn((B, T, kp), generator=g, device=dev, dtype=torch.float32))[:, :, :k]
        Xt = mean + std * (common[0, :, :k] @ Ut) + 0.5 * k ** 0.5 * std * torch.randn((T, m), generator=g, device=dev,
                                                                                      dtype=torch.float32)
        stack = torch.empty((B, T, m), dtype=torch.float32, device=dev)
        for J in a.Js:
            zj = torch.tensor(Z[:J], device=dev, dtype=torch.float32)[:, None, None]
            thr = (mean + zj * std * k ** 0.5 * (1.0 + 0.1 * torch.randn((J, S, m), generator=g, device=dev,
                                                                        dtype=torch.float32))).contiguous()
            th = thr[:, slot.long()].contiguous()                        # (J, T, m): the threshold of every element
            P = torch.empty((J, T, m), dtype=torch.float32, device=dev)

            def k24():
                cols, _, cnt = K.exceed_score(Ut, Cm, Xt, thr, slot, True, mean, std, w)
                return cols, cnt

            def prob():
                return K.exceed_prob(Ut, Cm, thr, slot, True, mean, std, out=P)

            def old():
                for b in range(B):
                    K.expand(Ut, Cm[b], mean, std, out=stack[b])
                cols, cnts = [], []
                fin = torch.isfinite(stack).all(dim=0) & torch.isfinite(Xt)
                for j in range(J):
                    c = (stack > th[j]).sum(dim=0)
                    o = Xt > th[j]
                    p = c.to(torch.float32) / B
                    of = o.to(torch.float32)
                    d = p - of
                    cols.append(torch.stack([((q[:, sel] * wsel).sum(dim=1, dtype=torch.float64))
                                             for q in (d * d, of, p, p * p)]))
                    key = (o.to(torch.int64) * (B + 1) + c)[:, sel][fin[:, sel]]
                    cnts.append(torch.bincount(key, minlength=2 * (B + 1)).reshape(2, B + 1))
                return torch.stack(cols), torch.stack(cnts)

            def k15():
                return K.spread_score(Ut, Cm, std)

            fns = {"k24": k24, "prob": prob, "old": old, "k15": k15}
            for _ in range(a.warmup):
                for fn in fns.values():
                    fn()
            (cn, hn), (co, ho) = k24(), old()
            torch.cuda.synchronize()
            mixed = float(hn[:, :, 1:B].sum()) / float(hn.sum())
            agree = {"counts_k24_equal_old": bool(torch.equal(hn, ho)), "counts_total": int(hn.sum()),
                     "share_of_mixed_counts": mixed, "base_rate": [float(v) for v in hn[:, 1].sum(dim=1) / hn.sum(dim=(1, 2))],
                     "cols_k24_vs_old_max_rel": float(((cn - co).abs() / co.abs().clamp_min(1e-300)).max())}
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
            line = {"entry": "exceed", "m": m, "k": k, "T": T, "B": B, "J": J, "S": S, "reps": a.reps,
                    "calls_per_sample": batch, **res,
                    "old_over_k24_median": res["old"]["median_ms"] / res["k24"]["median_ms"],
                    # the comparison that cannot be a timing accident: the composition's fastest sample against K24's slowest
                    "old_min_over_k24_max": res["old"]["min_ms"] / res["k24"]["max_ms"],
                    "k24_over_k15_median": res["k24"]["median_ms"] / res["k15"]["median_ms"],
                    "prob_over_k15_median": res["prob"]["median_ms"] / res["k15"]["median_ms"],
                    "agreement": agree}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del thr, th, P
        del Ut, Cm, Xt, stack

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
