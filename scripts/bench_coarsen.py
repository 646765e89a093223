"""K23 (dmdx_coarsen_f32) alone, on one cfg2 row block, against the torch compositions.

X is one resident row block of the size of cfg2's, 129 600 rows x 8760 hourly snapshots (4.54 GB fp32): one plane of a
latitude band of the ERA5 grid, 90 latitudes (90 N .. 67.75 N) x 1440 longitudes, with cos-latitude weights.  Cases:
(fy, fx) in {(2, 2), (4, 4), (8, 8), (3, 5)} with skipna off and on (1 % of the values missing), in ONE process, the
variants of a case alternating:
  k23            kern.coarsen(X, 1, 90, 1440, w, fy, fx, ...)
  k23-NAME       the same entry point of another build of the library (``--alt-lib NAME=PATH``; ``generic``: the
                 element-by-element walk alone, ``make -C dmd_era5_amd/csrc coarsen-generic``), called through ctypes on
                 the same operands; its results must equal the product's bit for bit
  torch          the cells as a (T, NLAT, fy, NLON, fx) view, ``.double()``, times w, summed over the two cell axes, divided
                 and ``.float()`` (an fp64 copy of the cells: 9.1 GB, and as much again for the product)
  torch-chunked  the same over ``--chunk`` snapshots at a time, which bounds the fp64 temporaries
  k20-count      kern.row_missing_count(X): the project's read-only streaming yardstick, one read of the same block
Conditions, asserted before anything is timed: on the first ``--check-snapshots`` snapshots the kernel gives the bits of
tests/coarsen_ref.py; against the torch results, which sum in another order, it agrees within 2^-22 |y| (one rounding to
fp32 each; the fp64 sums of at most 64 terms are far below that) and has its NaNs in the same cells.  Times are HIP
events around batches of calls on the current stream (>= ``--sample-ms`` of device time per sample), ``--reps`` samples
after ``--warmup`` calls; medians, minimum and maximum, with GB/s of the algorithmic traffic 4 T P (NLAT fy NLON fx + NLAT
NLON) bytes (4 T m for k20-count), the fraction of the 6.3 TB/s HBM figure of DESIGN.md that is, the ratio to the faster
torch composition and the fraction of the k20-count rate.  One JSON line per variant, also appended to
profiles/k23_bench_coarsen.jsonl.  No bar is set: nobody has measured this kernel before.
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
import coarsen_ref  # noqa: E402
from dmd_era5_amd import _lib  # noqa: E402
from dmd_era5_amd.kernels import default_kernels  # noqa: E402
from dmd_era5_amd.regrid import lat_weights  # noqa: E402

HBM_TBS = 6.3
T_START = time.time()


def note(msg):
    print(f"# [{time.time() - T_START:7.1f} s] {msg}", file=sys.stderr, flush=True)


def factors(text):
    fy, fx = text.lower().split("x")
    return int(fy), int(fx)


ap = argparse.ArgumentParser()
ap.add_argument("--nlat", type=int, default=90)
ap.add_argument("--nlon", type=int, default=1440)
ap.add_argument("--planes", type=int, default=1)
ap.add_argument("--T", type=int, default=8760)
ap.add_argument("--factors", nargs="+", type=factors, default=[(2, 2), (4, 4), (8, 8), (3, 5)], help="fy x fx, e.g. 4x4")
ap.add_argument("--skipna", nargs="+", type=int, default=[0, 1], choices=[0, 1])
ap.add_argument("--missing", type=float, default=0.01, help="fraction of NaN in the block of the skipna cases")
ap.add_argument("--min-frac", type=float, default=0.5)
ap.add_argument("--chunk", type=int, default=256, help="snapshots per step of the chunked composition")
ap.add_argument("--alt-lib", nargs="*", default=[], metavar="NAME=PATH",
                help="other builds of libdmdx.so whose dmdx_coarsen_f32 is timed beside the product's")
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--check-snapshots", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sample-ms", type=float, default=20.0)
ap.add_argument("--tag", default="", help="copied into every line (the build that was measured)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k23_bench_coarsen.jsonl"),
                help="the JSON lines are appended to this file too ('' switches that off)")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_coarsen: no GPU visible (a CPU run measures nothing)")
K = default_kernels()
dev = torch.device("cuda")
P, nlat, nlon, T = a.planes, a.nlat, a.nlon, a.T
m = P * nlat * nlon
alts = {}
for item in a.alt_lib:
    alt_name, alt_path = item.split("=", 1)
    alts[alt_name] = ctypes.CDLL(os.path.abspath(alt_path))
    alts[alt_name].dmdx_coarsen_f32.restype, alts[alt_name].dmdx_coarsen_f32.argtypes = _lib.SIGNATURES["dmdx_coarsen_f32"]

w_host = lat_weights(np.clip(90.0 - 0.25 * np.arange(nlat), -90.0, 90.0), "cos")
w = torch.from_numpy(w_host).to(dev)
X = torch.empty((T, m), dtype=torch.float32, device=dev)
gen = torch.Generator(device=dev).manual_seed(23)
for t0 in range(0, T, 1024):                                     # positive values, a few hundred: temperatures
    X[t0:t0 + 1024].normal_(270.0, 15.0, generator=gen)
Xnan = None


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


def torch_cells(Xs, fy, fx, NLAT, NLON, skipna, least_frac):
    """(T', P NLAT NLON) fp32 of the snapshots Xs by torch operators."""
    Tn = Xs.shape[0]
    x = Xs.view(Tn, P, nlat, nlon)[:, :, :NLAT * fy, :NLON * fx].double().reshape(Tn, P, NLAT, fy, NLON, fx)
    wv = w[:NLAT * fy].view(1, 1, NLAT, fy, 1, 1)
    if not skipna:
        y = (x * wv).sum(dim=(3, 5)) / (wv.sum(dim=3, keepdim=True) * fx).view(1, 1, NLAT, 1)
        return y.float().view(Tn, -1)
    ok = torch.isfinite(x)
    num = (torch.where(ok, x, torch.zeros((), dtype=x.dtype, device=x.device)) * wv).sum(dim=(3, 5))
    den = (ok * wv).sum(dim=(3, 5))
    full = (wv.sum(dim=3, keepdim=True) * fx).view(1, 1, NLAT, 1)
    y = torch.where((den == 0) | (den < least_frac * full), torch.full((), float("nan"), dtype=x.dtype, device=x.device), num / den)
    return y.float().view(Tn, -1)


lines = []
count = torch.zeros(m, dtype=torch.int32, device=dev)
for skipna in a.skipna:
    if skipna and Xnan is None:
        Xnan = X.clone()
        for t0 in range(0, T, 1024):
            part = Xnan[t0:t0 + 1024]
            part[torch.rand(part.shape, device=dev, generator=gen) < a.missing] = float("nan")
    Xc = Xnan if skipna else X
    for fy, fx in a.factors:
        NLAT, NLON = nlat // fy, nlon // fx
        case = f"{fy}x{fx}{'-skipna' if skipna else ''}"
        Y = torch.empty((T, P * NLAT * NLON), dtype=torch.float32, device=dev)
        kw = dict(skipna=bool(skipna), min_frac=a.min_frac)

        def k23():
            return K.coarsen(Xc, P, nlat, nlon, w, fy, fx, out=Y, **kw)

        note(f"{case}: {NLAT} x {NLON} cells; first launch")
        k23()
        torch.cuda.synchronize()
        n = a.check_snapshots
        want = coarsen_ref.coarsen(Xc[:n].cpu().numpy(), P, nlat, nlon, w_host, fy, fx, **kw)
        got = Y[:n].cpu().numpy()
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), f"{case}: not the bits of tests/coarsen_ref.py"
        fns, errs = {"k23": k23}, {}
        st = torch.cuda.current_stream().cuda_stream
        for alt_name, alt in alts.items():
            Yalt = torch.empty_like(Y)

            def k23_alt(alt=alt, Yalt=Yalt):
                rc = alt.dmdx_coarsen_f32(Xc.data_ptr(), T, m, P, nlat * nlon, nlat, nlon, w.data_ptr(), fy, fx, 0, 0, NLAT, NLON,
                                          int(skipna), a.min_frac, Yalt.data_ptr(), P * NLAT * NLON, NLAT * NLON, st)
                assert rc == 0, rc

            k23_alt()
            assert torch.equal(Yalt.view(torch.int32), Y.view(torch.int32)), f"{case}: the build {alt_name} differs"
            fns[f"k23-{alt_name}"] = k23_alt
        if not a.no_torch:
            def t_full():
                return torch_cells(Xc, fy, fx, NLAT, NLON, skipna, a.min_frac)

            Yc = torch.empty_like(Y)

            def t_chunked():
                for t0 in range(0, T, a.chunk):
                    Yc[t0:t0 + a.chunk] = torch_cells(Xc[t0:t0 + a.chunk], fy, fx, NLAT, NLON, skipna, a.min_frac)
                return Yc

            for name, fn in (("torch", t_full), ("torch-chunked", t_chunked)):
                note(f"{case}: the {name} composition")
                Yt = fn()
                assert torch.equal(torch.isnan(Yt), torch.isnan(Y)), f"{case}: {name} has its NaNs elsewhere"
                d = torch.nan_to_num(Yt - Y).abs() / torch.nan_to_num(Y).abs().clamp_min(1e-30)
                errs[name] = float(d.max()) / 2.0 ** -22
                assert errs[name] <= 1.0, f"{case}: {name} is {errs[name]:.3g} of the bound away from the kernel"
                fns[name] = fn
                del Yt, d
        fns["k20-count"] = lambda: K.row_missing_count(Xc, out=count)

        note(f"{case}: timing {list(fns)}")
        ms, calls = measure(fns)
        med = {name: statistics.median(v) for name, v in ms.items()}
        base = min((med[nm] for nm in med if nm.startswith("torch")), default=None)
        nbytes = 4 * T * P * (NLAT * fy * NLON * fx + NLAT * NLON)
        rate = {name: (4 * T * m if name == "k20-count" else nbytes) / med[name] / 1e6 for name in fns}
        for name in fns:
            line = {"bench": "coarsen", "case": case, "variant": name, "fy": fy, "fx": fx, "skipna": int(skipna), "planes": P,
                    "nlat": nlat, "nlon": nlon, "T": T, "NLAT": NLAT, "NLON": NLON, "bits_equal_ref_snapshots": n,
                    "err_of_bound": errs.get(name), "calls_per_sample": calls[name], "samples": len(ms[name]),
                    "median_ms": med[name], "min_ms": min(ms[name]), "max_ms": max(ms[name]), "GBps": rate[name],
                    "of_hbm_peak": rate[name] / 1e3 / HBM_TBS,
                    "speedup_vs_torch": None if base is None else base / med[name],
                    "of_k20_rate": rate[name] / rate["k20-count"], "tag": a.tag}
            lines.append(line)
            print(json.dumps(line), flush=True)
        del Y, fns
        torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
