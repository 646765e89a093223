import numpy as np, os, torch, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from dmd_era5_amd.engine import svd_numpy
from parity_utils import load_golden
g = load_golden(os.path.join(ROOT, "tests", "golden"), "conditioning_2048x160")
for tag in ("raw", "cen"):
    X = g[f"{tag}_X"]; k = int(g["k"])
    for typ in ("standard", "randomized"):
        U, s, V = svd_numpy(X, typ, k, device="cuda:0", **({"random_state": 0} if typ == "randomized" else {}))
        rel = np.abs(s / g[f"{tag}_s64"] - 1)
        print(tag, typ, "max rel err of s", rel.max(), "numpy fp32:", np.abs(g[f"{tag}_s32"] / g[f"{tag}_s64"] - 1).max(), "s[:3]", s[:3])
