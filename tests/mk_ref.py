"""The definition of K32 (dmdx_mk_stats_f32, dmdx_sen_slopes_f32) in plain numpy over the pairs -- the kernel is never
its own reference -- and ``MkDouble``, a CPU stand-in with the two ``HipKernels`` methods, so that
``dmd_era5_amd.mktrend`` is tested without a GPU.

Y is (m, n) fp32 here (rows first), tc the n fp64 time coordinates.  A point is valid iff it is finite.  The slopes are
ordered by K25's key of the bit pattern, which separates -0.0 from +0.0; ``np.sort`` does not.
"""
import numpy as np
import torch

QUIET_NAN = 0x7FC00000
NO_PAIR = np.uint64(1) << np.uint64(32)          # above every key: the place of a pair with a missing point


def key_of(bits):
    """The order-preserving key of fp32 bit patterns (uint32 -> uint32)."""
    u = np.asarray(bits, dtype=np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def bits_of(key):
    k = np.asarray(key, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)


def pairs_of(n):
    """All a < b of n points -> (a, b), each (n (n - 1) / 2,)."""
    a, b = np.triu_indices(n, k=1)
    return a, b


def mk_stats(Y):
    """-> (4, m) int32: v, S, E, G."""
    Y = np.asarray(Y, dtype=np.float32)
    m, n = Y.shape
    ok = np.isfinite(Y)
    a, b = pairs_of(n)
    both = ok[:, a] & ok[:, b]
    ya, yb = Y[:, a], Y[:, b]
    with np.errstate(invalid="ignore"):
        S = (both & (yb > ya)).sum(axis=1).astype(np.int64) - (both & (yb < ya)).sum(axis=1)
        E = (both & (yb == ya)).sum(axis=1).astype(np.int64)
        G = np.zeros(m, dtype=np.int64)
        for i0 in range(0, m, 256):                                   # (rows, n, n) booleans, a slab of rows at a time
            y, k = Y[i0:i0 + 256], ok[i0:i0 + 256]
            c = ((y[:, :, None] == y[:, None, :]) & k[:, None, :]).sum(axis=2).astype(np.int64)
            G[i0:i0 + 256] = np.where(k, (c - 1) * (2 * c + 5), 0).sum(axis=1)
    return np.stack([ok.sum(axis=1), S, E, G]).astype(np.int32)


def slope_keys(Y, tc):
    """-> (keys, N): the keys of the fp32 slopes of every row, (m, n (n - 1) / 2) uint64 sorted ascending with the pairs
    that hold a missing point last (``NO_PAIR``); N (m,) the number of pairs of valid points."""
    Y = np.asarray(Y, dtype=np.float32)
    tc = np.asarray(tc, dtype=np.float64)
    ok = np.isfinite(Y)
    a, b = pairs_of(Y.shape[1])
    both = ok[:, a] & ok[:, b]
    y64 = Y.astype(np.float64)
    with np.errstate(all="ignore"):
        d = y64[:, b] - y64[:, a]
        h = tc[b] - tc[a]
        e = (d / h[None, :]).astype(np.float32)
    keys = np.where(both, key_of(e.view(np.uint32)).astype(np.uint64), NO_PAIR)
    keys.sort(axis=1)
    v = ok.sum(axis=1).astype(np.int64)
    return keys, v * (v - 1) // 2


def select(keys, N, rank):
    """The bits of the order statistics: ``rank`` (J, m) -> (J, m) uint32, the quiet NaN where rank is outside 0 .. N - 1."""
    rank = np.asarray(rank, dtype=np.int64)
    out = np.full(rank.shape, QUIET_NAN, dtype=np.uint32)
    if keys.shape[1] == 0:
        return out
    rows = np.arange(keys.shape[0])
    for j in range(rank.shape[0]):
        inside = (rank[j] >= 0) & (rank[j] < N)
        k = keys[rows, np.where(inside, rank[j], 0)]
        out[j] = np.where(inside, bits_of((k & np.uint64(0xFFFFFFFF)).astype(np.uint32)), np.uint32(QUIET_NAN))
    return out


def sen_slopes(Y, tc, rank):
    """-> (J, m) uint32: the bits dmdx_sen_slopes_f32 writes."""
    keys, N = slope_keys(Y, tc)
    return select(keys, N, rank)


class MkDouble:
    """A kernel double: ``mk_stats`` and ``sen_slopes`` of HipKernels on CPU tensors, computed by the functions above."""

    name = "cpu-double+mk"
    mk_max_n = 128
    sen_max_ranks = 4
    calls = 0

    def mk_stats(self, Yt, out=None):
        type(self).calls += 1
        Q = torch.from_numpy(mk_stats(Yt.numpy().T))
        if out is None:
            return Q
        out.copy_(Q)
        return out

    def sen_slopes(self, Yt, coord, ranks, out=None):
        type(self).calls += 1
        bits = sen_slopes(Yt.numpy().T, np.asarray(coord, dtype=np.float64), ranks.numpy())
        E = torch.from_numpy(bits.view(np.float32).copy())
        if out is None:
            return E
        out.copy_(E)
        return out
