"""numpy doubles of the CF decode (io_netcdf) and of K14 (dmdx_unpack_i16_f32).

The arithmetic is the contract of both: an fp64 multiply, an fp64 add, one rounding to fp32,
``(q.astype(float64) * scale_factor + add_offset).astype(float32)``, and the quiet NaN numpy itself
produces (0x7FC00000) where the code equals a fill code.  Plain helpers, no fixtures.
"""
from __future__ import annotations

import numpy as np


def decode(q, scale_factor=1.0, add_offset=0.0, fills=()) -> np.ndarray:
    """Packed codes (any integer dtype) -> float32 physical values, NaN at the fill codes."""
    q = np.asarray(q)
    with np.errstate(over="ignore"):
        x = (q.astype(np.float64) * np.float64(scale_factor) + np.float64(add_offset)).astype(np.float32)
    for f in fills:
        x[q == f] = np.float32(np.nan)
    return x


def row_index(row0: int, rows: int, plane: int, seg_offset) -> np.ndarray:
    """Source element (inside one snapshot) of the rows row0 .. row0 + rows - 1 of the variable."""
    g = row0 + np.arange(rows, dtype=np.int64)
    return np.asarray(seg_offset, dtype=np.int64)[g // plane] + g % plane


def unpack_i16(S, lds, T, tstep, rows, row0, plane, seg_offset, scale_factor, add_offset, fills=()):
    """K14 on a flat int16 host array ``S`` -> ((rows, T) float32, number of fill codes met)."""
    S = np.asarray(S).reshape(-1)
    src = row_index(row0, rows, plane, seg_offset)
    q = np.stack([S[j * tstep * lds + src] for j in range(T)], axis=1) if T else np.zeros((rows, 0), np.int16)
    nfill = int(sum(int((q == f).sum()) for f in dict.fromkeys(fills)))
    return decode(q, scale_factor, add_offset, fills), nfill


def addressed(size, lds, T, tstep, rows, row0, plane, seg_offset) -> np.ndarray:
    """Boolean mask over a flat source of ``size`` elements: the codes the call may read."""
    mask = np.zeros(size, dtype=bool)
    src = row_index(row0, rows, plane, seg_offset)
    for j in range(T):
        mask[j * tstep * lds + src] = True
    return mask


def pack(x, scale_factor, add_offset, fill=None, dtype=np.int16) -> np.ndarray:
    """Physical values -> codes (round to nearest), NaN -> ``fill``: how the fixtures are made."""
    x = np.asarray(x, dtype=np.float64)
    info = np.iinfo(dtype)
    q = np.rint((np.nan_to_num(x, nan=add_offset) - add_offset) / scale_factor)
    q = np.clip(q, info.min + 1, info.max).astype(dtype)
    if fill is not None:
        q[np.isnan(x)] = fill
    return q
