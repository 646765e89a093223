"""Host definitions for the K20 tests (row mask: count of missing values per row, one value for the masked rows)
and the reference decomposition of a slice with masked grid points.  Plain numpy; no GPU, no test in here.

Layout as in the package: a block is ``(n snapshots, m rows)``, one snapshot per row of the array.
"""
import numpy as np

from oracle import era5_oracle as orc

EXP_MASK = 0x7F800000


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def not_finite(X) -> np.ndarray:
    """The bit-pattern definition: exponent all ones (every NaN, +Inf, -Inf)."""
    return (bits(X) & EXP_MASK) == EXP_MASK


def count(X) -> np.ndarray:
    """(n, m) fp32 -> int32 (m,): the number of snapshots of every row that are not finite."""
    X = np.asarray(X, dtype=np.float32)
    return not_finite(X).sum(axis=0).astype(np.int32).reshape(X.shape[1])


def apply(X, cnt, value) -> np.ndarray:
    """A copy of X (as uint32 bit patterns) with every row whose count is not 0 set to the bits of ``value``."""
    out = bits(X).copy()
    out[:, np.asarray(cnt) != 0] = np.float32(value).view(np.uint32)
    return out


# ---- patterns of missing values ------------------------------------------------------------------------------
NAN_PAYLOADS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FC0DEAD, 0x7FA5A5A5)
MISSING = NAN_PAYLOADS + (0x7F800000, 0xFF800000)                      # ... and +Inf, -Inf
FINITE_EDGES = (0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000000)   # -0, denormals, +-FLT_MAX, +0
PATTERNS = ("scattered", "first", "last", "row0", "rowlast", "ragged", "allrow", "none")


def planted(n: int, m: int, pattern: str, seed: int = 0):
    """-> (X (n, m) fp32, where (n, m) bool): finite data with the finite edge values sprinkled in and missing values
    (all payloads, both infinities) planted by ``pattern``."""
    rs = np.random.RandomState(1000 * n + m + seed)
    X = (280.0 + 20.0 * rs.standard_normal((n, m))).astype(np.float32)
    b = X.view(np.uint32)
    edge = rs.rand(n, m) < 0.1
    b[edge] = np.asarray(FINITE_EDGES, dtype=np.uint32)[rs.randint(0, len(FINITE_EDGES), int(edge.sum()))]
    where = np.zeros((n, m), dtype=bool)
    some_rows, some_times = rs.rand(m) < 0.3, rs.rand(n) < 0.4
    if pattern == "scattered":
        where = rs.rand(n, m) < 0.05
    elif pattern == "first":
        where[0] = some_rows
        where[0, m // 2] = True
    elif pattern == "last":
        where[n - 1] = some_rows
        where[n - 1, m // 2] = True
    elif pattern == "row0":
        where[:, 0] = some_times
        where[n // 2, 0] = True
    elif pattern == "rowlast":
        where[:, m - 1] = some_times
        where[n // 2, m - 1] = True
    elif pattern == "ragged":                                          # the last (partial) quad of rows
        q = (m - 1) // 4 * 4
        where[:, q:] = rs.rand(n, m - q) < 0.5
        where[n - 1, m - 1] = True
    elif pattern == "allrow":
        where[:, m // 2] = True
    elif pattern != "none":
        raise ValueError(pattern)
    k = int(where.sum())
    b[where] = np.asarray(MISSING, dtype=np.uint32)[np.arange(k) % len(MISSING)]
    assert np.array_equal(not_finite(X), where)
    return X, where


# ---- the reference decomposition -----------------------------------------------------------------------------
def point_mask(variables: dict) -> np.ndarray:
    """(time, level, lat, lon) arrays in dict order -> bool over the physical space points in flatten order:
    True = used (finite in every snapshot)."""
    X, _ = orc.flatten({k: np.asarray(v) for k, v in variables.items()})
    return np.isfinite(X).all(axis=1)


def masked_svd(variables: dict, mean_center: bool, scale: bool, d: int, k: int):
    """Drop the masked space points, centre / scale like ``oracle.standardize``, embed, ``np.linalg.svd`` in fp64.
    -> dict: used (M,) bool; U (d * M_used, k), s, V of the compacted matrix; X the compacted embedded matrix;
    mean / std (M_used,) or None."""
    used = point_mask(variables)
    X, _ = orc.flatten({key: np.asarray(v, dtype=np.float64) for key, v in variables.items()})
    X = X[used]
    mean = std = None
    if mean_center:
        Xt, mean, std = orc.standardize(np.ascontiguousarray(X.T), 0, scale=scale)
        X = Xt.T
    E = orc.delay_embed(np.ascontiguousarray(X), d)
    U, s, V = orc.svd_standard(E, k)
    return {"used": used, "U": U, "s": s, "V": V, "X": E, "mean": mean, "std": std}
