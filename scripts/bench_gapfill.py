"""K31 (dmdx_gap_fill_f32 / dmdx_gap_mask_f32) alone, on one cfg2 row block, against the torch compositions.

X is one resident row block, 129 780 rows x 8760 snapshots (4.55 GB fp32); the factors are k = 20 random modes.  Gap shares
of 1 %, 10 % and 50 %, each SCATTERED (every element drawn on its own: nearly every tile of the fill holds a gap) and
CLUSTERED in boxes of 128 rows x 32 snapshots on the tile grid of the fill (a share of the tiles is all gaps, the rest has
none: the case the skip is for).  In ONE process and alternating, per mask:
  fill   k31         kern.gap_fill_(U, C, W, X, mean, std)                 change_row wanted
         k31_plain   the same with want_change=False                      (old is never loaded)
         torch       kern.expand(U, C, mean, std, out=tmp); torch.where(mask, tmp, X, out=X)
                     a second X-sized buffer, a boolean mask of X's shape, three more X-sized streams
  mask   k31         kern.gap_mask(X)                                      words, counts and fp64 sums in one read
         k31_walk    the same with split=False
         k20         kern.row_missing_count(X)                             K20's one read of the same bytes
Conditions, asserted before anything is timed: the words of gap_mask hold exactly the planted gaps; the fill and the
composition leave the same bits in X.  Times are HIP events around batches of calls on the current stream (>=
`--sample-ms` of device time per sample), `--reps` samples after `--warmup` calls; medians, and the peak memory each
variant allocates beyond what is resident.  One JSON line per variant (`--out FILE` appends them to a file as well).
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
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--shares", default="0.01,0.1,0.5")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--out", default="", help="append the JSON lines to this file too")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_gapfill: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
m, n, k = a.m, a.n, a.k
gen = torch.Generator(device=dev).manual_seed(31)
X0 = torch.empty((n, m), dtype=torch.float32, device=dev)
for t0 in range(0, n, 1024):
    X0[t0:t0 + 1024].normal_(0.0, 1.0, generator=gen)
Ut = torch.randn((k, m), generator=gen, device=dev)
Ct = torch.randn((n, k), generator=gen, device=dev)
mean = torch.randn(m, generator=gen, device=dev)
std = 0.5 + torch.rand(m, generator=gen, device=dev)
tmp = torch.empty_like(X0)


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
    for _ in range(a.reps):                                      # alternating: all see the same machine
        for name, fn in fns.items():
            ms[name].append(batch_ms(fn, calls[name]))
    return ms, calls


def planted(share, clustered):
    """The boolean (n, m) mask: every element on its own, or whole boxes of 128 rows x 32 snapshots."""
    if not clustered:
        G = torch.empty((n, m), dtype=torch.bool, device=dev)
        for t0 in range(0, n, 1024):
            G[t0:t0 + 1024] = torch.rand((min(1024, n - t0), m), generator=gen, device=dev) < share
        return G
    cells = torch.rand((-(-n // 32), -(-m // 128)), generator=gen, device=dev) < share
    return cells.repeat_interleave(32, dim=0)[:n].repeat_interleave(128, dim=1)[:, :m].contiguous()


lines = []
out_f = open(a.out, "a") if a.out else None


def emit(line):
    lines.append(line)
    print(json.dumps(line), flush=True)
    if out_f:
        out_f.write(json.dumps(line) + "\n")


for share in [float(s) for s in a.shares.split(",")]:
    for clustered in (False, True):
        G = planted(share, clustered)
        n_gaps = int(G.sum())
        Xk = X0.clone()
        Xk.masked_fill_(G, float("nan"))
        W, nmiss, sums = K.gap_mask(Xk)
        assert int(nmiss.sum(dtype=torch.int64)) == n_gaps, "gap_mask counts other gaps than were planted"
        probe = torch.randint(0, n, (4096,), device=dev), torch.randint(0, m, (4096,), device=dev)
        assert torch.equal(((W[probe[0] >> 5, probe[1]] >> (probe[0] & 31)) & 1) != 0, G[probe]), "the words are wrong"

        # the same bits from the kernel and from the composition, from the same start
        Xt = Xk.clone()
        K.gap_fill_(Ut, Ct, W, Xk, mean, std)
        K.expand(Ut, Ct, mean, std, out=tmp)
        torch.where(G, tmp, Xt, out=Xt)
        torch.cuda.synchronize()
        same = bool(torch.equal(Xk.view(torch.int32), Xt.view(torch.int32)))
        assert same, "gap_fill_ does not give the bits of expand + torch.where"

        def k_fill():
            return K.gap_fill_(Ut, Ct, W, Xk, mean, std)

        def k_plain():
            return K.gap_fill_(Ut, Ct, W, Xk, mean, std, want_change=False)

        def t_fill():
            K.expand(Ut, Ct, mean, std, out=tmp)
            return torch.where(G, tmp, Xt, out=Xt)

        fns = {"k31": k_fill, "k31_plain": k_plain, "torch": t_fill}
        extra = {name: peak_extra_bytes(fn) for name, fn in fns.items()}
        ms, calls = measure(fns)
        med = {name: statistics.median(v) for name, v in ms.items()}
        for name in fns:
            # the bytes the operation needs: the words, and the gaps written (k31: and read)
            need = 4 * W.numel() + 4 * n_gaps * (2 if name == "k31" else 1)
            emit({"bench": "gapfill", "op": "fill", "variant": name, "m": m, "n": n, "k": k, "share": share,
                  "clustered": clustered, "gaps": n_gaps, "bit_equal": same, "calls_per_sample": calls[name],
                  "median_ms": med[name], "min_ms": min(ms[name]), "max_ms": max(ms[name]),
                  "needed_GBps": need / med[name] / 1e6, "peak_extra_bytes": extra[name],
                  "resident_extra_bytes": (tmp.numel() * 4 + G.numel()) if name == "torch" else W.numel() * 4,
                  "speedup_vs_torch": med["torch"] / med[name]})
        print(f"# fill, share {share}, {'clustered' if clustered else 'scattered'}: K31 {med['k31']:.3f} ms "
              f"({med['k31_plain']:.3f} ms without change_row), expand + where {med['torch']:.3f} ms", flush=True)
        del Xt, G

# the mask against K20's read of the same bytes, 10 % scattered gaps
Xk = X0.clone()
Xk.masked_fill_(planted(0.1, False), float("nan"))
fns = {"k31": lambda: K.gap_mask(Xk), "k31_walk": lambda: K.gap_mask(Xk, split=False), "k20": lambda: K.row_missing_count(Xk)}
extra = {name: peak_extra_bytes(fn) for name, fn in fns.items()}
ms, calls = measure(fns)
med = {name: statistics.median(v) for name, v in ms.items()}
for name in fns:
    emit({"bench": "gapfill", "op": "mask", "variant": name, "m": m, "n": n, "calls_per_sample": calls[name],
          "median_ms": med[name], "min_ms": min(ms[name]), "max_ms": max(ms[name]), "GBps": 4 * m * n / med[name] / 1e6,
          "of_hbm_peak": 4 * m * n / med[name] / 1e9 / HBM_TBS, "peak_extra_bytes": extra[name],
          "speed_vs_k20": med["k20"] / med[name]})
print(f"# mask: K31 {med['k31']:.3f} ms split, {med['k31_walk']:.3f} ms walk; K20's count {med['k20']:.3f} ms", flush=True)
if out_f:
    out_f.close()
