"""What :mod:`climatology` (K18), :mod:`trend` (K21) and :mod:`timefilter` (K22) share on the host: the check of the
time stamps, a host table on the devices of the blocks, and the pieces of ``to_dataset`` / ``from_dataset``."""
from __future__ import annotations

import numpy as np
import torch

from .labeled import Coord


def stamps(times, who: str, wrong_type=ValueError) -> np.ndarray:
    """``times`` as a 1-D datetime64 array without NaT, in its own unit; else a ValueError (``wrong_type``: the dtype)."""
    t = np.atleast_1d(np.asarray(times))
    if not np.issubdtype(t.dtype, np.datetime64):
        raise wrong_type(f"{who}: times must be numpy.datetime64, got {t.dtype}")
    if t.ndim != 1:
        raise ValueError(f"{who}: times must be one-dimensional, got {t.shape}")
    if np.isnat(t).any():
        raise ValueError(f"{who}: times holds NaT")
    return t


class OnDevices:
    """A host array as a tensor on every device that asks for it, uploaded once per device."""

    def __init__(self, host: np.ndarray):
        self.host = torch.from_numpy(host)
        self._copies = {}

    def on(self, device) -> torch.Tensor:
        if device not in self._copies:
            self._copies[device] = self.host.to(device)
        return self._copies[device]


def attr_int(v) -> int:
    return int(np.asarray(v).reshape(-1)[0])


def attr_str(v) -> str:
    v = np.asarray(v).reshape(-1)[0] if not isinstance(v, (str, bytes)) else v
    return v.decode() if isinstance(v, bytes) else str(v)


def row_coords(coords) -> dict:
    """The per-row coordinates among ``coords`` (``space`` and what lives on it), as :class:`Coord`, as they are."""
    row = {}
    for name, c in (coords or {}).items():
        c = c if isinstance(c, Coord) else Coord(name, c)
        if set(c.dims) <= {"space"} or name == "space":
            row[name] = c
    return row


def cut_rows(field: np.ndarray, rows, device, kern, who: str) -> list:
    """A stored ``(n, M)`` field as one contiguous ``(n, rows[b])`` tensor per block (``rows`` None: one block) on
    ``device`` (None: the GPU for the HIP provider ``kern``)."""
    if device is None:
        device = torch.device("cuda" if getattr(kern, "name", "") == "hip" else "cpu")
    M = int(field.shape[1])
    rows = [M] if rows is None else [int(r) for r in rows]
    if sum(rows) != M:
        raise ValueError(f"{who}: rows sum to {sum(rows)}, the file holds {M}")
    edges = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return [torch.from_numpy(np.ascontiguousarray(field[:, i:j])).to(device) for i, j in zip(edges[:-1], edges[1:])]
