"""What K1's unit rerun costs on data with Inf / NaN in it: the Gram launch of cfg2's row blocks
(bench.py's generator), timed with HIP events around dmdx_syrk_blocks_f32, on

  clean    the blocks as the benchmark feeds them;
  one      one NaN planted in one element: the tiles of one tile row / column of one K-split run twice;
  column   one NaN every --stride rows of one column, in every block: every unit that the column feeds runs twice
           (units are at most 65 536 rows long; cfg2's are 64 896).

The same script under DMDX_LIB_PATH=<another build> gives that build's times (MEASUREMENTS.md pairs them).
Results are correct in every case; nothing is asserted here beyond the class of the planted column."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import WORKLOADS, make_snapshot_blocks  # noqa: E402
from dmd_era5_amd.kernels import default_kernels  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--column", type=int, default=100)
ap.add_argument("--stride", type=int, default=32768)
a = ap.parse_args()

dev = torch.device("cuda", 0)
kern = default_kernels()
m, n, _, _ = WORKLOADS[a.workload]
blocks = make_snapshot_blocks(m, n, 1234, dev)
for Xb in blocks:
    kern.row_center_scale_(Xb, False)
torch.cuda.synchronize()


def launch_ms():
    kern.syrk_blocks(blocks)
    torch.cuda.synchronize()
    out = []
    for _ in range(a.reps):
        kern.events = []
        G = kern.syrk_blocks(blocks)
        torch.cuda.synchronize()
        out.append(sum(e0.elapsed_time(e1) for _, _, e0, e1 in kern.events))
        kern.events = None
    return out, G


res = {"lib": os.environ.get("DMDX_LIB_PATH", "product"), "workload": a.workload, "blocks": len(blocks),
       "rows_per_block": [int(b.shape[1]) for b in blocks]}
ms, G = launch_ms()
assert bool(torch.isfinite(G).all())
res["clean_ms"] = ms
nan = float("nan")
blocks[0][a.column, 5] = nan
ms, G = launch_ms()
assert bool(torch.isnan(G[a.column]).all()) and int(torch.isnan(G).sum()) == 2 * n - 1
res["one_nan_ms"] = ms
planted = 1
for Xb in blocks:
    Xb[a.column, 5::a.stride] = nan
    planted += len(range(5, Xb.shape[1], a.stride))
ms, G = launch_ms()
assert int(torch.isnan(G).sum()) == 2 * n - 1
res["column_nan_ms"] = ms
res["column_nans_planted"] = planted - 1
print(json.dumps(res))
