"""Minimal labelled arrays for the host side of the path.

The reference passes ``xarray`` objects between its stages; xarray is not available
in this image, and the engine only ever needs four things from them: the values, the
dimension names, 1-D coordinate arrays and an attribute dict.  ``DataArray`` /
``Dataset`` below carry exactly that, with the attribute names xarray uses
(``.values .dims .coords .attrs .sizes .data_vars``), so the mirrored functions read
like the reference's.  Any object with ``.values`` (a real ``xr.DataArray`` included)
is accepted at the SVD boundary.

The ``space`` coordinate: the reference stores one Python tuple ``(level, lat, lon)``
per row (slice_tools.py:323,346); at 10^6-10^7 rows that is minutes of interpreter
time, so here it is an ``(m, 3)`` float64 array with the same three numbers per row.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np


class Coord:
    """A coordinate: values indexed by one named dimension (or several for `space`)."""

    __slots__ = ("dims", "values")

    def __init__(self, dims, values):
        self.dims = (dims,) if isinstance(dims, str) else tuple(dims)
        self.values = np.asarray(values)

    @property
    def data(self):
        return self.values

    @property
    def shape(self):
        return self.values.shape

    def __len__(self):
        return len(self.values)

    def __getitem__(self, idx):
        return Coord(self.dims, self.values[idx])


def _as_coords(coords) -> "OrderedDict[str, Coord]":
    out: OrderedDict[str, Coord] = OrderedDict()
    for name, c in (coords or {}).items():
        if isinstance(c, Coord):
            out[name] = c
        elif isinstance(c, tuple) and len(c) == 2 and isinstance(c[0], (str, tuple, list)):
            out[name] = Coord(c[0], c[1])
        else:
            out[name] = Coord(name, c)
    return out


PACKING_ATTRS = ("scale_factor", "add_offset", "_FillValue", "missing_value")


class Packing:
    """The CF packing of a variable: physical value = code * scale_factor + add_offset, NaN where the
    code equals ``_FillValue`` / ``missing_value`` (``fills``: at most two distinct codes).

    ``decode`` is the one arithmetic of the package for it (kernel K14 does the same on the device,
    bit for bit): an fp64 multiply, an fp64 add, one rounding to float32.  float64 variables stay
    float64; a variable with fill values only keeps its float dtype (integers become float32)."""

    __slots__ = ("scale_factor", "add_offset", "fills")

    def __init__(self, scale_factor=1.0, add_offset=0.0, fills=()):
        self.scale_factor, self.add_offset = float(scale_factor), float(add_offset)
        self.fills = tuple(dict.fromkeys(fills))

    @property
    def affine(self) -> bool:
        return self.scale_factor != 1.0 or self.add_offset != 0.0

    def out_dtype(self, dtype) -> np.dtype:
        return np.dtype(np.float64) if np.dtype(dtype) == np.float64 else np.dtype(np.float32)

    def decode(self, q) -> np.ndarray:
        q = np.asarray(q)
        out = self.out_dtype(q.dtype)
        if self.affine or q.dtype.kind != "f":
            with np.errstate(over="ignore", invalid="ignore"):
                x = (q.astype(np.float64) * np.float64(self.scale_factor) + np.float64(self.add_offset)).astype(out)
        else:
            x = q.astype(out, copy=True)
        for f in self.fills:
            x[q == f] = np.nan
        return x

    FILL_I16 = -32768       # the fill code of a packing made by for_range; the live codes are -32767 .. 32767
    MAX_I16 = 32767

    @classmethod
    def for_range(cls, vmin, vmax) -> "Packing":
        """The int16 packing of the values ``vmin .. vmax`` (fp64): ``vmin`` encodes to -32767 and ``vmax`` to 32767,
        -32768 is the fill code.  A single value packs with scale 1 and itself as the offset; no finite value at
        all -- the range (+inf, -inf) the kernels return for an all-missing group -- with scale 1 and offset 0."""
        vmin, vmax = float(vmin), float(vmax)
        if np.isfinite(vmin) and np.isfinite(vmax) and vmin < vmax:
            sf, ao = (vmax - vmin) / 65534.0, (vmax + vmin) / 2.0
        elif np.isfinite(vmin) and vmin == vmax:
            sf, ao = 1.0, vmin
        elif vmin == np.inf and vmax == -np.inf:
            sf, ao = 1.0, 0.0
        else:
            raise ValueError(f"Packing.for_range: ({vmin}, {vmax}) is no range")
        return cls(sf, ao, (cls.FILL_I16,))

    def encode(self, x, counts: bool = False):
        """float32 values -> int16 codes, the inverse of :meth:`decode` and the one arithmetic of the package for it
        (kernel K17 does the same on the device, bit for bit): a non-finite value becomes the fill code -32768
        (*filled*); any other ``rint((float64(x) - add_offset) / scale_factor)`` -- an fp64 subtract, an fp64 divide,
        round half to even -- clamped to -32767 .. 32767 (*saturated* where the clamp was needed).
        ``counts=True`` returns ``(codes, filled, saturated)``."""
        x = np.asarray(x, dtype=np.float32)
        fin = np.isfinite(x)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            r = np.rint((np.where(fin, x, np.float32(0)).astype(np.float64) - np.float64(self.add_offset))
                        / np.float64(self.scale_factor))
        sat = fin & ((r < -self.MAX_I16) | (r > self.MAX_I16))
        q = np.where(fin, np.clip(r, -self.MAX_I16, self.MAX_I16), self.FILL_I16).astype(np.int16)
        return (q, int((~fin).sum()), int(sat.sum())) if counts else q

    def __repr__(self):
        return f"Packing(scale_factor={self.scale_factor!r}, add_offset={self.add_offset!r}, fills={self.fills!r})"


class LazyArray:
    """A file-backed array (like xarray's lazily opened variables): shape / dtype are known,
    the data are read on first use, or in slabs along the first axis by the streaming ingest.

    ``dtype`` is the FILE's: ``read_slab`` / ``read_box`` deliver what is stored (the ingest moves
    packed codes as they are).  ``packing`` (a :class:`Packing`, or None) says how stored values
    become physical ones; ``np.asarray(lazy)`` applies it."""

    def __init__(self, shape, dtype, read_all, read_slab, read_box=None, packing=None):
        self.shape, self.dtype, self.ndim = tuple(shape), np.dtype(dtype), len(shape)
        self._read_all, self.read_slab = read_all, read_slab
        self.packing = packing
        # read_box(starts, counts, out=None): a hyperslab (one rank's latitude band of a time slab)
        self.read_box = read_box or self._box_from_slab

    def _box_from_slab(self, starts, counts, out=None):
        slab = self.read_slab(starts[0], starts[0] + counts[0])
        box = slab[(slice(None),) + tuple(slice(a, a + c) for a, c in zip(starts[1:], counts[1:]))]
        if out is None:
            return np.ascontiguousarray(box)
        out[...] = box
        return out

    @property
    def decoded_dtype(self) -> np.dtype:
        return self.dtype if self.packing is None else self.packing.out_dtype(self.dtype)

    def __array__(self, dtype=None, copy=None):
        a = self._read_all()
        if self.packing is not None:
            a = self.packing.decode(a)
        return a.astype(dtype) if dtype is not None else a


class DataArray:
    def __init__(self, values, dims, coords=None, attrs=None, name=None):
        self._values = values if hasattr(values, "shape") else np.asarray(values)
        self.dims = tuple(dims)
        if len(self.dims) != self._values.ndim:
            raise ValueError(f"dims {self.dims} do not match a {self._values.ndim}-D array")
        self.coords = _as_coords(coords)
        self.attrs = dict(attrs or {})
        self.name = name
        # how the variable was stored in the file it came from (xarray's .encoding): the reader puts
        # the CF packing attributes here after decoding; nothing reads it when writing
        self.encoding: dict = {}

    @property
    def values(self):
        if isinstance(self._values, LazyArray):
            self._values = np.asarray(self._values)
        return self._values

    @values.setter
    def values(self, v):
        self._values = v

    @property
    def lazy(self) -> "LazyArray | None":
        """The file-backed array if the data have not been loaded yet, else None."""
        return self._values if isinstance(self._values, LazyArray) else None

    @property
    def shape(self):
        return tuple(self._values.shape)

    @property
    def ndim(self):
        return self._values.ndim

    @property
    def dtype(self):
        """dtype of ``.values`` (a packed file-backed variable: the decoded one, not the file's)."""
        if isinstance(self._values, LazyArray):
            return self._values.decoded_dtype
        return self._values.dtype

    @property
    def sizes(self):
        return dict(zip(self.dims, self._values.shape))

    def __repr__(self):
        return f"<DataArray {self.name or ''} {self.sizes} coords={list(self.coords)}>"


class Dataset:
    def __init__(self, data_vars=None, coords=None, attrs=None):
        self.data_vars: OrderedDict[str, DataArray] = OrderedDict()
        self.coords = _as_coords(coords)
        self.attrs = dict(attrs or {})
        for name, da in (data_vars or {}).items():
            self[name] = da

    def __setitem__(self, name, da):
        if not isinstance(da, DataArray):
            raise TypeError("Dataset variables must be DataArray")
        da.name = name
        self.data_vars[name] = da
        for cn, c in da.coords.items():
            self.coords.setdefault(cn, c)

    def __getitem__(self, key):
        if isinstance(key, (list, tuple)):
            missing = [k for k in key if k not in self.data_vars]
            if missing:
                raise KeyError(f"variables not in dataset: {missing}")
            return Dataset({k: self.data_vars[k] for k in key}, self.coords, self.attrs)
        return self.data_vars[key]

    def __contains__(self, key):
        return key in self.data_vars

    @property
    def sizes(self):
        out = {}
        for da in self.data_vars.values():
            out.update(da.sizes)
        for name, c in self.coords.items():
            if c.dims == (name,):
                out.setdefault(name, len(c))
        return out

    def __repr__(self):
        return f"<Dataset vars={list(self.data_vars)} sizes={self.sizes}>"
