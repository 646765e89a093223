"""numpy double of K24 (dmdx_exceed_prob_f32, dmdx_exceed_score_f32) and the error bounds its tests use.

TEST INFRASTRUCTURE, like tests/crps_ref.py.  Matrices are the LOGICAL column-major ones of include/dmdx.h: member
fields F (B, m, T) fp32, X (m, T), thr (m, J S) with column j S + s = threshold j of every row for slot s, slot (T,)
int or None (all 0), w (m,) or None.

Everything per element is EXACT: given the fp32 member fields (dmdx_expand_f32's, on the GPU) the count c, the
outcome o, p = fp32(c / B) and the four quantities d^2, o, p, p^2 (d = fl(p - o), each rounded once in fp32) are
formed here in the same fp32 operations the kernel uses, so P, the counts and every term of a sum have no error at
all.  What is left is the summation.  The terms are non-negative (and <= 1 before the weight), the kernel adds at most
R of them in fp32 in some fixed order and the partial results in fp64, so (u = 2^-24, derived, not measured)
  |d col_q| <= (R + 3) u sum_i fl(w_i q)      R = DMDX_EXCEED_FP32_ROWS = 128
  |d row_q| <= (R + 3) u sum_t q              R = 16 (the fp32 part of a row sum)
the form of verify_ref / crps_ref: (R - 1) u for the fp32 chain in any order to first order, the rest for its second
order and the fp64 additions.
"""
import numpy as np

import expand_ref as er

U24 = 2.0 ** -24
FP32_ROWS = 128           # DMDX_EXCEED_FP32_ROWS of include/dmdx.h
FP32_COLS = 16
NQ = 4                    # DMDX_EXCEED_NQ
MAX_B = 256               # DMDX_EXCEED_MAX_B
MAX_THR = 4               # DMDX_EXCEED_MAX_THR


def thresholds_of(thr, J, S, T, slot=None):
    """-> (J, m, T) fp32: the threshold of every element."""
    sl = np.zeros(T, dtype=np.int64) if slot is None else np.asarray(slot, dtype=np.int64)
    assert sl.shape == (T,) and sl.min() >= 0 and sl.max() < S and thr.shape[1] == J * S
    return np.stack([thr[:, j * S + sl] for j in range(J)]).astype(np.float32)


def elements(F, X, thr, J, S, slot=None, above=True):
    """-> (c (J, m, T) int32, o (J, m, T) bool or None, p (J, m, T) fp32, finite (m, T) bool): the count of members
    in the event, the outcome of X (None without X), p = fp32(c / B); `finite` is whether every member (and X) is."""
    B, m, T = F.shape
    assert F.dtype == np.float32 and thr.dtype == np.float32
    th = thresholds_of(thr, J, S, T, slot)
    cmp = np.greater if above else np.less
    with np.errstate(invalid="ignore"):
        c = np.zeros((J, m, T), dtype=np.int32)
        for b in range(B):
            c += cmp(F[b][None], th)
        o = None if X is None else cmp(X[None], th)
    p = (np.arange(B + 1, dtype=np.float64) / B).astype(np.float32)[c]
    finite = np.isfinite(F).all(axis=0)
    if X is not None:
        finite &= np.isfinite(X)
    return c, o, p, finite


def prob(F, thr, J, S, slot=None, above=True, el=None):
    """-> P (J, m, T) fp32, NaN where a member is not finite: what dmdx_exceed_prob_f32 writes, bit for bit.  ``el``:
    elements(...) of the same operands (with or without X), to save forming them again."""
    p = (elements(F, None, thr, J, S, slot, above) if el is None else el)[2]
    return np.where(np.isfinite(F).all(axis=0)[None], p, np.float32(np.nan)).astype(np.float32)


def quantities(o, p, finite):
    """-> the four (J, m, T) fp32 quantities d^2, o, p, p^2 in fp32 operations, NaN where the element is not finite."""
    of = o.astype(np.float32)
    d = p - of
    nan = np.float32(np.nan)
    return [np.where(finite[None], q, nan).astype(np.float32) for q in (d * d, of, p, p * p)]


def score(F, X, thr, J, S, slot=None, above=True, w=None, el=None):
    """-> (col (J, 4, T) fp64, row (J, 4, m) fp64, cnt (J, 2, B + 1) int64); rows with w == 0 are selected out of col
    and cnt, non-finite elements enter no bin.  The terms of col are fl(w q) in fp32, added in fp64."""
    B, m, T = F.shape
    c, o, p, finite = elements(F, X, thr, J, S, slot, above) if el is None else el
    keep = np.ones(m, dtype=bool) if w is None else w != 0
    col, row = np.empty((J, NQ, T)), np.empty((J, NQ, m))
    with np.errstate(invalid="ignore"):
        for q, Q in enumerate(quantities(o, p, finite)):
            assert Q.dtype == np.float32
            row[:, q] = Q.sum(axis=2, dtype=np.float64)
            terms = Q[:, keep] if w is None else Q[:, keep] * w[keep].astype(np.float32)[None, :, None]
            assert terms.dtype == np.float32
            col[:, q] = terms.sum(axis=1, dtype=np.float64)
    sel = finite & keep[:, None]
    cnt = np.stack([np.bincount((o[j][sel] * np.int32(B + 1) + c[j][sel]), minlength=2 * (B + 1)) for j in range(J)])
    return col, row, cnt.reshape(J, 2, B + 1).astype(np.int64)


def bounds_of(col, row):
    """The bounds of the sums (col, row) of score(): every term is non-negative, so the sum of the terms is the sum."""
    return (FP32_ROWS + 3) * U24 * col, (FP32_COLS + 3) * U24 * row


def score_bounds(F, X, thr, J, S, slot=None, above=True, w=None, el=None):
    """-> bounds of (col (J, 4, T), row (J, 4, m)).  Every operand must be finite here."""
    return bounds_of(*score(F, X, thr, J, S, slot, above, w, el)[:2])


def scores(S, W, B):
    """The scores of forecast.exceed_blocks from sums S (..., 4, n) and W (broadcast against S[..., 0, :])."""
    S0, S1, S2, S3 = (S[..., q, :] for q in range(4))
    with np.errstate(all="ignore"):
        brier, base = S0 / W, S1 / W
        fair = brier - (S2 - S3) / ((B - 1) * W) if B > 1 else np.full_like(brier, np.nan)
        return {"brier": brier, "brier_fair": fair, "base_rate": base, "forecast_rate": S2 / W,
                "brier_skill": 1.0 - brier / (base * (1.0 - base))}


def roc_area(cnt):
    """The area under the ROC curve of counts (..., 2, B + 1): the decision "at least c members" for c = B + 1 .. 0
    gives (false alarm rate, hit rate) from (0, 0) to (1, 1), joined by trapezoids; NaN without both outcomes."""
    n0, n1 = cnt[..., 0, :].astype(np.float64), cnt[..., 1, :].astype(np.float64)
    with np.errstate(all="ignore"):
        far = np.cumsum(n0[..., ::-1], axis=-1) / n0.sum(axis=-1, keepdims=True)
        hit = np.cumsum(n1[..., ::-1], axis=-1) / n1.sum(axis=-1, keepdims=True)
    z = np.zeros(far.shape[:-1] + (1,))
    far, hit = np.concatenate([z, far], axis=-1), np.concatenate([z, hit], axis=-1)
    return (0.5 * (hit[..., 1:] + hit[..., :-1]) * (far[..., 1:] - far[..., :-1])).sum(axis=-1)


def murphy(cnt):
    """-> (reliability_term, resolution_term, uncertainty) of counts (..., 2, B + 1), unweighted:
    sum_c N_c (p_c - O_c / N_c)^2 / N, sum_c N_c (O_c / N_c - O / N)^2 / N, (O / N)(1 - O / N), p_c = c / B."""
    B = cnt.shape[-1] - 1
    Nc = cnt.sum(axis=-2).astype(np.float64)
    Oc = cnt[..., 1, :].astype(np.float64)
    N = Nc.sum(axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        obar = Oc.sum(axis=-1, keepdims=True) / N
        freq = np.where(Nc > 0, Oc / np.where(Nc > 0, Nc, 1.0), 0.0)
        pc = np.arange(B + 1) / B
        rel = (Nc * (pc - freq) ** 2).sum(axis=-1) / N[..., 0]
        res = (Nc * (freq - obar) ** 2).sum(axis=-1) / N[..., 0]
    return rel, res, (obar * (1.0 - obar))[..., 0]


class ExceedDouble:
    """K24's methods of a kernel provider on the CPU, for the host-layer tests: numpy through the functions above
    (independent of forecast.py's torch fallback), mixed into tests/kernel_double.CpuKernelDouble.  The member fields
    are the fp64 products rounded to fp32."""

    exceed_max_k = 256
    exceed_max_members = MAX_B
    exceed_max_thresholds = MAX_THR

    @staticmethod
    def _ops(Ut, Cm, thr, slot, mean, std):
        def _np(t):
            return None if t is None else t.detach().cpu().numpy()

        B, T, k = Cm.shape
        C = _np(Cm).reshape(B * T, k).T
        U = _np(Ut).T
        F = np.stack([er.expand64(U, C[:, b * T:(b + 1) * T], _np(mean), _np(std)) for b in range(B)]).astype(np.float32)
        th = _np(thr)
        th = th[:, None, :] if th.ndim == 2 else th
        J, S, m = th.shape
        assert m == U.shape[0] and 1 <= J <= MAX_THR
        return F, np.ascontiguousarray(th.reshape(J * S, m).T), J, S, _np(slot)

    def exceed_prob(self, Ut, Cm, thr, slot=None, above=True, mean=None, std=None, out=None):
        import torch

        F, th, J, S, sl = self._ops(Ut, Cm, thr, slot, mean, std)
        P = torch.from_numpy(np.ascontiguousarray(prob(F, th, J, S, sl, above).transpose(0, 2, 1)))
        if out is not None:
            out.copy_(P)
            return out
        return P

    def exceed_score(self, Ut, Cm, Xt, thr, slot=None, above=True, mean=None, std=None, weight=None, out=None,
                     counts=None, want_rows=False):
        import torch

        F, th, J, S, sl = self._ops(Ut, Cm, thr, slot, mean, std)
        w = None if weight is None else weight.detach().cpu().numpy()
        col, row, cnt = score(F, Xt.detach().cpu().numpy().T, th, J, S, sl, above, w)
        cols, cnt = torch.from_numpy(col), torch.from_numpy(cnt)
        assert (out is None) == (counts is None)
        if out is not None:
            out += cols
            counts += cnt
            cols, cnt = out, counts
        return cols, (torch.from_numpy(row) if want_rows else None), cnt
