"""Host definition of K27 (csrc/spell.hip) in numpy: spell and exceedance-count indices of every row, per threshold and
period.

This file IS the contract the kernel is held to element for element (tests/test_gpu_spell.py); the kernel is never its
own reference.  :func:`spells` is a plain loop over the snapshots of a period with no pieces and no merge.  X is a
(rows, snapshots) host array, the C ABI's logical view; ``thr`` the (J, S, rows) table (the C ABI's column j S + s is
``thr[j, s]``), ``slot`` (T,) integers or None (every snapshot in slot 0).

    valid  v_t = x_t is finite (bit pattern: the exponent is not all ones)  and  0 <= slot[t] < S  and  h is not NaN,
                 h = thr[j, slot[t], i]
    event  e_t = v_t and (x_t > h if above[j] else x_t < h)            strict: a tie is no event, +-Inf is a threshold
    run    a maximal set of consecutive t inside one period [b_p, b_{p+1}) with e_t; it qualifies with >= min_len[j]

    plane 0 n_valid   1 n_event   2 n_spell (qualifying runs)   3 n_in_spell (their lengths, summed)
          4 longest (any run; 0 if none)   5 first   6 last  (t - b_p of the first snapshot of the first / the last
          snapshot of the last qualifying run; -1 if none)

:func:`spells_by_pieces` restates the same results the way the split form of the kernel reaches them -- a record per
piece of ``seg`` snapshots, merged in order -- and tests/test_spells.py holds the two against each other.
"""
import numpy as np
import torch

NQ = 7
WS_WORDS = 9


def finite_bits(X):
    return (np.ascontiguousarray(X, dtype=np.float32).view(np.uint32) & 0x7F800000) != 0x7F800000


def _above_list(above, J):
    a = [bool(v) for v in np.atleast_1d(np.asarray(above)).reshape(-1)]
    return a * J if len(a) == 1 else a


def _min_list(min_len, J):
    a = [int(v) for v in np.atleast_1d(np.asarray(min_len)).reshape(-1)]
    return a * J if len(a) == 1 else a


def valid_and_event(X, thr, slot, above):
    """-> (V, E), (J, m, T) booleans: the valid snapshots and the events of every threshold."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    m, T = X.shape
    J, S = thr.shape[:2]
    assert thr.shape == (J, S, m)
    sl = np.zeros(T, dtype=np.int64) if slot is None else np.asarray(slot, dtype=np.int64).reshape(-1)
    assert sl.shape == (T,)
    inside = (sl >= 0) & (sl < S)
    fin = finite_bits(X)
    V, E = np.empty((J, m, T), dtype=bool), np.empty((J, m, T), dtype=bool)
    with np.errstate(invalid="ignore"):
        for j in range(J):
            h = thr[j][np.where(inside, sl, 0)].T                     # (m, T): the threshold of every element
            V[j] = fin & inside[None] & ~np.isnan(h)
            E[j] = V[j] & ((X > h) if above[j] else (X < h))
    return V, E


def _close(q, length, end, min_len, mask):
    """A run of ``length`` snapshots whose last one is ``end`` has ended in the rows of ``mask``."""
    mask = mask & (length > 0)
    q[4] = np.where(mask, np.maximum(q[4], length), q[4])
    ok = mask & (length >= min_len)
    q[2] += ok
    q[3] += np.where(ok, length, 0)
    q[5] = np.where(ok & (q[5] < 0), end - length + 1, q[5])
    q[6] = np.where(ok, end, q[6])


def tally(V, E, min_len):
    """The 7 planes (7, m) of one threshold and one period: V, E (m, n) are its snapshots.  The plain loop."""
    m, n = E.shape
    q = np.zeros((NQ, m), dtype=np.int64)
    q[5:] = -1
    run = np.zeros(m, dtype=np.int64)
    for t in range(n):
        e = E[:, t]
        q[0] += V[:, t]
        q[1] += e
        _close(q, run, t - 1, min_len, ~e)
        run = np.where(e, run + 1, 0)
    _close(q, run, n - 1, min_len, np.ones(m, dtype=bool))
    return q


def _check(bounds, T, J, min_len):
    b = [int(v) for v in np.asarray(bounds).reshape(-1)]
    assert len(b) >= 2 and b[0] >= 0 and b[-1] <= T and all(x < y for x, y in zip(b, b[1:])), b
    assert 1 <= J <= 4 and len(min_len) == J and all(v >= 1 for v in min_len)
    return b


def spells(X, thr, bounds, min_len=1, above=True, slot=None):
    """(J, 7, P, m) int32 of the (m, T) fp32 matrix X."""
    thr = np.asarray(thr, dtype=np.float32)
    J = thr.shape[0]
    above, min_len = _above_list(above, J), _min_list(min_len, J)
    b = _check(bounds, np.shape(X)[1], J, min_len)
    V, E = valid_and_event(X, thr, slot, above)
    out = np.empty((J, NQ, len(b) - 1, V.shape[1]), dtype=np.int32)
    for j in range(J):
        for p, (lo, hi) in enumerate(zip(b[:-1], b[1:])):
            out[j, :, p] = tally(V[j][:, lo:hi], E[j][:, lo:hi], min_len[j])
    return out


# ---------------------------------------------------------------- the same through pieces and an ordered merge
def piece_record(V, E, min_len, off):
    """The record (9, m) of one piece -- snapshots V, E (m, n), the first of them ``off`` after the period's start:
    valid, events, head run, tail run, and count / snapshots / longest / first / last of the runs strictly inside."""
    m, n = E.shape
    rec = np.zeros((WS_WORDS, m), dtype=np.int64)
    rec[0], rec[1] = V.sum(axis=1), E.sum(axis=1)
    for i in range(m):
        e = E[i]
        gaps = np.flatnonzero(~e)
        if gaps.size == 0:
            rec[2:4, i], rec[7:, i] = n, -1
            continue
        head, tail = int(gaps[0]), n - 1 - int(gaps[-1])
        inner = tally(np.zeros((1, n), dtype=bool), (e & (np.arange(n) > head) & (np.arange(n) < n - tail))[None], min_len)
        rec[2, i], rec[3, i] = head, tail
        rec[4:7, i] = inner[2:5, 0]
        rec[7, i] = inner[5, 0] + off if inner[5, 0] >= 0 else -1
        rec[8, i] = inner[6, 0] + off if inner[6, 0] >= 0 else -1
    return rec


def merge_records(records, lengths, seg, plen, min_len):
    """The 7 planes (7, m) of a period from the records of its pieces, in ascending order: a piece of events only
    extends the carry; otherwise carry + head is closed, the interior added and the carry becomes the tail; the carry
    is closed at the period's end."""
    m = records[0].shape[1]
    q = np.zeros((NQ, m), dtype=np.int64)
    q[5:] = -1
    carry = np.zeros(m, dtype=np.int64)
    every = np.ones(m, dtype=bool)
    for k, (rec, n) in enumerate(zip(records, lengths)):
        q[0] += rec[0]
        q[1] += rec[1]
        full = rec[1] == n
        _close(q, carry + rec[2], k * seg + rec[2] - 1, min_len, ~full)
        q[2] += np.where(full, 0, rec[4])
        q[3] += np.where(full, 0, rec[5])
        q[4] = np.where(full, q[4], np.maximum(q[4], rec[6]))
        q[5] = np.where(~full & (q[5] < 0), rec[7], q[5])
        q[6] = np.where(~full & (rec[8] >= 0), rec[8], q[6])
        carry = np.where(full, carry + n, rec[3])
    _close(q, carry, plen - 1, min_len, every)
    return q


def spells_by_pieces(X, thr, bounds, min_len=1, above=True, slot=None, seg=4):
    """:func:`spells` through records of pieces of ``seg`` snapshots, every period cut from its own start."""
    thr = np.asarray(thr, dtype=np.float32)
    J = thr.shape[0]
    above, min_len = _above_list(above, J), _min_list(min_len, J)
    b = _check(bounds, np.shape(X)[1], J, min_len)
    V, E = valid_and_event(X, thr, slot, above)
    out = np.empty((J, NQ, len(b) - 1, V.shape[1]), dtype=np.int32)
    for j in range(J):
        for p, (lo, hi) in enumerate(zip(b[:-1], b[1:])):
            cuts = list(range(lo, hi, seg))
            recs = [piece_record(V[j][:, a:min(a + seg, hi)], E[j][:, a:min(a + seg, hi)], min_len[j], a - lo) for a in cuts]
            out[j, :, p] = merge_records(recs, [min(a + seg, hi) - a for a in cuts], seg, hi - lo, min_len[j])
    return out


def n_pieces(bounds, seg):
    b = [int(v) for v in bounds]
    return sum(-(-(y - x) // seg) for x, y in zip(b[:-1], b[1:]))


class SpellDouble:
    """A kernel double: ``spells`` of HipKernels on CPU tensors, computed by :func:`spells`."""

    name = "cpu-double+spell"
    spell_max_thresholds = 4
    spell_max_periods = 128
    spell_calls = 0

    def spells(self, Xt, thr, bounds, min_len=1, above=True, slot=None, seg=512, out=None):
        type(self).spell_calls += 1
        th = thr.numpy() if thr.dim() == 3 else thr.numpy()[:, None]
        P = torch.from_numpy(spells(Xt.numpy().T, th, bounds, min_len, above, None if slot is None else slot.numpy()))
        if out is None:
            return P
        out.copy_(P)
        return out
