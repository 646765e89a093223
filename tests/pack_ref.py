"""numpy reference of K17 (dmdx_expand_range_f32 / dmdx_expand_pack_i16 / dmdx_range_f32 / dmdx_pack_f32_i16) and a
CPU double of the four provider methods.

TEST INFRASTRUCTURE, like tests/unpack_ref.py: written out on its own here, independent of labeled.Packing.encode
(which the tests compare with it).  The arithmetic of a code (include/dmdx.h, K17):
  non-finite x  -> -32768 (the fill code), counted as filled
  otherwise     rint((float64(x) - add_offset) / scale_factor): an fp64 subtract, an IEEE fp64 divide, round half to
                even; clamped to -32767 .. 32767, an element that needed the clamp counted as saturated.
Everything is exact: the tests that use it are equalities.
"""
import numpy as np

FILL = -32768
QMAX = 32767
U24 = 2.0 ** -24


def for_range(vmin, vmax):
    """-> (scale_factor, add_offset) of the packing of the values vmin .. vmax (python floats are fp64)."""
    vmin, vmax = float(vmin), float(vmax)
    if vmin == np.inf and vmax == -np.inf:          # no finite value at all
        return 1.0, 0.0
    assert np.isfinite(vmin) and np.isfinite(vmax) and vmin <= vmax
    if vmin == vmax:
        return 1.0, vmin
    return (vmax - vmin) / 65534.0, (vmax + vmin) / 2.0


def encode(x, scale_factor, add_offset):
    """-> (codes int16, filled, saturated) of the float32 array x."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    sf, ao = np.float64(scale_factor), np.float64(add_offset)
    q = np.full(x.shape, FILL, dtype=np.int16)
    fin = np.isfinite(x)
    with np.errstate(all="ignore"):
        r = np.rint((x[fin].astype(np.float64) - ao) / sf)
    sat = (r < -QMAX) | (r > QMAX)
    q[fin] = np.minimum(np.maximum(r, -QMAX), QMAX).astype(np.int16)
    return q, int((~fin).sum()), int(sat.sum())


def decode(q, scale_factor, add_offset):
    """K14's arithmetic (tests/unpack_ref.py): fp64 multiply, fp64 add, one rounding to float32; fill -> NaN."""
    q = np.asarray(q)
    x = (q.astype(np.float64) * np.float64(scale_factor) + np.float64(add_offset)).astype(np.float32)
    x[q == FILL] = np.nan
    return x


def finite_range(x):
    """-> (min, max as float32, number of non-finite values); (+inf, -inf) without a finite value."""
    x = np.asarray(x, dtype=np.float32)
    fin = np.isfinite(x)
    if not fin.any():
        return np.float32(np.inf), np.float32(-np.inf), int(x.size)
    return x[fin].min(), x[fin].max(), int((~fin).sum())


def ulp32(x):
    """One float32 unit in the last place of |x| (of the smallest normal below it)."""
    return np.spacing(np.maximum(np.abs(np.asarray(x, dtype=np.float32)), np.float32(2.0 ** -126))).astype(np.float64)


class PackDouble:
    """The four K17 methods of a kernel provider on the CPU, for the host-layer tests: this file's numpy on the
    provider's own ``expand``; mixed into tests/kernel_double.CpuKernelDouble next to expand_ref.ExpandDouble."""

    pack_max_k = 256

    @staticmethod
    def _merge(x, out):
        import torch

        lo, hi, n = finite_range(x)
        if out is None:
            return torch.tensor([lo, hi], dtype=torch.float32), torch.tensor([n], dtype=torch.int64)
        rng, cnt = out
        rng[0], rng[1] = min(float(rng[0]), float(lo)), max(float(rng[1]), float(hi))
        cnt += n
        return rng, cnt

    @staticmethod
    def _codes(x, packing, out, counts):
        import torch

        q, filled, saturated = encode(x, packing.scale_factor, packing.add_offset)
        Q = torch.from_numpy(q)
        if out is not None:
            out.copy_(Q)
            Q = out
        add = torch.tensor([filled, saturated], dtype=torch.int64)
        if counts is None:
            return Q, add
        counts += add
        return Q, counts

    def expand_range(self, Ut, Ct, mean=None, std=None, out=None):
        return self._merge(self.expand(Ut, Ct, mean, std).numpy(), out)

    def expand_pack(self, Ut, Ct, mean, std, packing, out=None, counts=None):
        return self._codes(self.expand(Ut, Ct, mean, std).numpy(), packing, out, counts)

    def field_range(self, Xt, out=None):
        return self._merge(Xt.detach().cpu().numpy(), out)

    def pack(self, Xt, packing, out=None, counts=None):
        return self._codes(np.ascontiguousarray(Xt.detach().cpu().numpy()), packing, out, counts)
