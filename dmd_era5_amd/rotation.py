"""Varimax / orthomax rotation of the leading k modes to simple structure, iterated on the device (K30,
csrc/varimax.hip): rotated EOFs and rotated PCs.

The unrotated EOFs of a global field are domain-shaped dipoles and quadrupoles; the published regional patterns are
rotated ones.  The loadings are ``A = U diag(s)`` (or ``U`` itself), ``U`` the resident ``(k, rows)`` blocks of the left
singular vectors.  An orthogonal ``R`` (k, k) is sought that maximises the orthomax criterion of ``L = A R``,

    sum_c ( sum_i L[i, c]^4 / m  -  gamma (sum_i L[i, c]^2 / m)^2 ),        gamma = 1: varimax, 0: quartimax.

One step reads every block of U once (``HipKernels.varimax_step``: ``G = A^T L^3``, ``q = colsum(L^2)``,
``f = colsum(L^4)``, L never stored) and moves ``k^2 + 2 k`` doubles to the host, where, in fp64,

    B = G - (gamma / m) (A^T A R) diag(q),     u, sigma, vh = svd(B),     R = u vh.

The scaling never touches U: the kernel gets ``diag(s) R`` rounded to fp32, the host forms ``G = diag(s) G'``, and
``A^T A`` comes once from K3 (``gemm_tn_blocks``).  Kaiser's normalisation divides every row of A by its norm ``h``
(``HipKernels.row_norms``); a row of zeros gets the weight 0 and takes no part.  Its Gram ``U^T W^2 U`` is the one place
where weighted rows exist in memory: K3 takes no row weights, so they are formed ``GRAM_SLICE`` rows at a time, once,
before the iteration.

    rot = orthomax_blocks(res.Ublocks, s=res.s)            # varimax with Kaiser's normalisation
    reofs = rot.loadings_blocks(res.Ublocks, s=res.s)      # (k, rows) fp32 per block, through K12
    rpcs = rot.coefficients(res.Vh)                        # R^T Vh: the rotated PCs

Row shards: one all-reduce of ``A^T A`` before the iteration and one packed all-reduce of ``k^2 + 2 k`` doubles per
step.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _timeaxis as ta
from . import io_netcdf
from .labeled import Coord, DataArray, Dataset
from .svd import Comm, _kern

__all__ = ["Rotation", "orthomax_blocks", "GRAM_SLICE"]

# rows of the one temporary of a normalised rotation: 256 MB at k = 64; a cfg2 block is one slice, cfg4's 15.6 M rows 15
GRAM_SLICE = 1 << 20


def _vec64(s, k: int, who: str):
    if s is None:
        return None
    v = s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else np.asarray(s)
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    if v.shape[0] != k:
        raise ValueError(f"{who}: s holds {v.shape[0]} values, the blocks hold {k} modes")
    if not np.isfinite(v).all():
        raise ValueError(f"{who}: s must be finite")
    return v


def _factors(R: np.ndarray, s, device) -> torch.Tensor:
    """``diag(s) R`` rounded to fp32, as the (k, k) tensor of the column-major matrix (row c = column c)."""
    C = R if s is None else s[:, None] * R
    return torch.from_numpy(np.ascontiguousarray(C.T.astype(np.float32))).to(device)


@dataclass
class Rotation:
    """An orthogonal rotation of k modes: ``R`` (k, k) fp64, columns ordered by descending variance of the rotated
    loadings and signed so that the largest entry of every column is positive.  ``criterion`` holds the orthomax
    criterion before every step and after the last one (``iterations + 1`` values); ``variance`` is
    ``colsum((U diag(s) R)^2)``; ``communality`` (normalised rotations only) per block the (rows,) fp32 row norms of
    ``U diag(s)``."""

    R: np.ndarray
    gamma: float
    normalized: bool
    iterations: int
    converged: bool
    criterion: np.ndarray
    variance: np.ndarray
    communality: list | None = None
    kern: object = field(default=None, repr=False)

    @property
    def k(self) -> int:
        return int(self.R.shape[0])

    def loadings_blocks(self, Ublocks, s=None, out=None) -> list:
        """The rotated patterns ``U diag(s) R`` of every block as a (k, rows) fp32 tensor: K12's ``expand`` with the
        k columns of ``diag(s) R`` as coefficients, U resident.  ``out``: a list of (k, rows) fp32 views."""
        kern = _kern(self.kern)
        s64 = _vec64(s, self.k, "Rotation.loadings_blocks")
        res = []
        for b, U in enumerate(Ublocks):
            if int(U.shape[0]) != self.k:
                raise ValueError(f"Rotation.loadings_blocks: block {b} holds {int(U.shape[0])} modes, R rotates {self.k}")
            res.append(kern.expand(U, _factors(self.R, s64, U.device), out=None if out is None else out[b]))
        return res

    def coefficients(self, C):
        """``R^T C``: the rotated PCs of ``C`` = Vh, S Vh or DMD coefficients, (k, T); a tensor gives a tensor."""
        if isinstance(C, torch.Tensor):
            if int(C.shape[0]) != self.k:
                raise ValueError(f"Rotation.coefficients: C holds {int(C.shape[0])} rows, R rotates {self.k}")
            return torch.from_numpy(np.ascontiguousarray(self.R.T)).to(device=C.device, dtype=C.dtype) @ C
        C = np.asarray(C)
        if C.shape[0] != self.k:
            raise ValueError(f"Rotation.coefficients: C holds {C.shape[0]} rows, R rotates {self.k}")
        return self.R.T @ C

    # -- persistence ----------------------------------------------------------------------------------------------
    def to_dataset(self, coords=None) -> Dataset:
        """``rotation(mode, rotated_mode)``, ``rotated_variance(rotated_mode)``, ``criterion(step)`` in fp64 and, of a
        normalised rotation, ``communality(space)``; ``gamma`` (``repr`` of the fp64), ``normalized``, ``iterations``
        and ``converged`` as attributes.  ``coords``: the per-row coordinates of the decomposed array."""
        k = self.k
        cds = {"mode": Coord("mode", np.arange(k, dtype=np.int64)),
               "rotated_mode": Coord("rotated_mode", np.arange(k, dtype=np.int64)),
               "step": Coord("step", np.arange(len(self.criterion), dtype=np.int64))}
        if self.communality is not None:
            cds.update(ta.row_coords(coords))
        ds = Dataset(coords=cds, attrs={"gamma": repr(float(self.gamma)), "normalized": int(self.normalized),
                                        "iterations": int(self.iterations), "converged": int(self.converged)})
        ds["rotation"] = DataArray(np.array(self.R, dtype=np.float64), ("mode", "rotated_mode"),
                                   {"mode": cds["mode"], "rotated_mode": cds["rotated_mode"]})
        ds["rotated_variance"] = DataArray(np.array(self.variance, dtype=np.float64), ("rotated_mode",),
                                           {"rotated_mode": cds["rotated_mode"]})
        ds["criterion"] = DataArray(np.array(self.criterion, dtype=np.float64), ("step",), {"step": cds["step"]})
        if self.communality is not None:
            row = {n: c for n, c in cds.items() if n not in ("mode", "rotated_mode", "step")}
            h = np.concatenate([v.detach().cpu().numpy() for v in self.communality])
            ds["communality"] = DataArray(h, ("space",), row)
        return ds

    @classmethod
    def from_dataset(cls, ds: Dataset, rows=None, device=None, kern=None) -> "Rotation":
        """The rotation :meth:`to_dataset` stored.  ``rows``: the row counts of the blocks to cut the communalities
        into (default: one block); ``device``: where they go (default: the GPU for the HIP provider)."""
        a = ds.attrs
        comm = None
        if "communality" in ds:
            kern = _kern(kern)
            h = np.ascontiguousarray(np.asarray(ds["communality"].values), dtype=np.float32).reshape(1, -1)
            comm = [v.reshape(-1) for v in ta.cut_rows(h, rows, device, kern, "Rotation.from_dataset")]
        R = np.ascontiguousarray(np.asarray(ds["rotation"].values), dtype=np.float64)
        if R.ndim != 2 or R.shape[0] != R.shape[1]:
            raise ValueError(f"Rotation.from_dataset: rotation is {R.shape}, a square matrix asked for")
        return cls(R, float(ta.attr_str(a["gamma"])), bool(ta.attr_int(a["normalized"])), ta.attr_int(a["iterations"]),
                   bool(ta.attr_int(a["converged"])), np.asarray(ds["criterion"].values, dtype=np.float64).reshape(-1),
                   np.asarray(ds["rotated_variance"].values, dtype=np.float64).reshape(-1), comm, kern)

    def to_netcdf(self, path: str, coords=None) -> str:
        return io_netcdf.to_netcdf(self.to_dataset(coords), path)

    @classmethod
    def from_netcdf(cls, path: str, rows=None, device=None, kern=None) -> "Rotation":
        return cls.from_dataset(io_netcdf.open_dataset(path), rows, device, kern)


def _polar(B: np.ndarray):
    """-> (u vh, sum of the singular values) of a small fp64 matrix."""
    u, sig, vh = np.linalg.svd(B)
    return u @ vh, float(sig.sum())


def orthomax_blocks(Ublocks, s=None, gamma: float = 1.0, normalize: bool = True, max_iter: int = 100, tol: float = 1e-6,
                    comm: Comm | None = None, kern=None, n_rows: int | None = None) -> Rotation:
    """The orthomax rotation of the loadings ``U diag(s)`` (``s`` None: of U) held as (k, rows) fp32 blocks.

    ``gamma``: 1 varimax, 0 quartimax, k / 2 equamax.  ``normalize``: Kaiser's normalisation, every row of the
    loadings divided by its norm for the iteration (a row of zeros keeps the weight 0).  The iteration stops after
    ``max_iter`` steps, or -- with ``tol`` > 0 -- once the sum of the singular values of B grew by no more than
    ``tol`` times itself; ``tol`` <= 0 runs exactly ``max_iter`` steps.  ``m`` of the formulas is the row count
    over all blocks and ranks, or ``n_rows`` when given (the unmasked grid points of a masked decomposition).
    ``comm``: the row shards' communicator (:class:`svd.Comm`)."""
    kern = _kern(kern)
    comm = comm or Comm()
    Ublocks = list(Ublocks)
    if not Ublocks:
        raise ValueError("orthomax_blocks: no blocks")
    k, dev = int(Ublocks[0].shape[0]), Ublocks[0].device
    for b, U in enumerate(Ublocks):
        if U.dim() != 2 or int(U.shape[0]) != k:
            raise ValueError(f"orthomax_blocks: block {b} is {tuple(U.shape)}, ({k}, rows) asked for")
    max_k = int(kern.varimax_max_k)
    if k > max_k:
        raise ValueError(f"orthomax_blocks: {k} modes, at most {max_k} are rotated at once: rotate fewer modes "
                         f"(the leading ones: Ublocks of U[:{max_k}])")
    if int(max_iter) < 1:
        raise ValueError(f"orthomax_blocks: max_iter = {max_iter} must be >= 1")
    gamma = float(gamma)
    s64 = _vec64(s, k, "orthomax_blocks")
    sv = np.ones(k) if s64 is None else s64

    # A^T A of the loadings the criterion sees (normalised or not) and of the plain ones (the variances), once
    weights, communality = [None] * len(Ublocks), None
    plain = kern.gemm_tn_blocks(Ublocks, Ublocks)
    if normalize:
        cs = None if s64 is None else torch.from_numpy(s64.astype(np.float32)).to(dev)
        communality, seen = [], None
        for b, U in enumerate(Ublocks):
            h = kern.row_norms(U, None if cs is None else cs.to(U.device))
            weights[b] = torch.where(h > 0, 1.0 / torch.where(h > 0, h, torch.ones_like(h)), torch.zeros_like(h))
            communality.append(h)
            # the normalised Gram needs the weighted rows once, before the iteration: slices of GRAM_SLICE rows, so that
            # the temporary is k x GRAM_SLICE floats whatever the block is, never a second U
            for r0 in range(0, int(U.shape[1]), GRAM_SLICE):
                Uw = U[:, r0:r0 + GRAM_SLICE] * weights[b][r0:r0 + GRAM_SLICE]
                seen = kern.gemm_tn_blocks([Uw], [Uw], out=seen)
                del Uw
    else:
        seen = plain
    rows_local = sum(int(U.shape[1]) for U in Ublocks)
    flat = torch.cat([seen.reshape(-1).to(torch.float64), plain.reshape(-1).to(torch.float64),
                      torch.tensor([float(rows_local)], dtype=torch.float64, device=seen.device)])
    flat = comm.allreduce_sum_(flat, tag="orthomax_gram_allreduce").cpu().numpy()
    AtA = sv[:, None] * flat[:k * k].reshape(k, k) * sv[None, :]
    AtA_plain = sv[:, None] * flat[k * k:2 * k * k].reshape(k, k) * sv[None, :]
    m = float(n_rows) if n_rows is not None else float(flat[2 * k * k])
    if not m >= 1:
        raise ValueError(f"orthomax_blocks: {m} rows")

    def sums(R):
        acc, Rt = None, {}
        for U, w in zip(Ublocks, weights):
            if U.device not in Rt:
                Rt[U.device] = _factors(R, s64, U.device)
            acc = kern.varimax_step(U, Rt[U.device], w, out=acc)
        Gt, q, f = acc
        v = comm.allreduce_sum_(torch.cat([Gt.reshape(-1), q, f]), tag="orthomax_allreduce").cpu().numpy()
        G = sv[:, None] * v[:k * k].reshape(k, k).T
        q, f = v[k * k:k * k + k], v[k * k + k:]
        return G, q, float((f / m - gamma * (q / m) ** 2).sum())

    R, d_old, crit, converged, it = np.eye(k), 0.0, [], False, 0
    for it in range(1, int(max_iter) + 1):
        G, q, c = sums(R)
        crit.append(c)
        if not np.isfinite(G).all() or not np.isfinite(q).all():
            raise ValueError("orthomax_blocks: the sums of a step are not finite (a NaN or Inf in U or s; rows masked "
                             "out of the decomposition must be zeros)")
        R, d = _polar(G - (gamma / m) * (AtA @ R) * q[None, :])
        if tol > 0 and it > 1 and d - d_old <= tol * d:
            converged = True
            break
        d_old = d
    crit.append(sums(R)[2])

    variance = np.einsum("jc,jl,lc->c", R, AtA_plain, R)
    order = np.argsort(-variance, kind="stable")
    R, variance = R[:, order], variance[order]
    top = np.abs(R).argmax(axis=0)
    R = R * np.where(R[top, np.arange(k)] < 0, -1.0, 1.0)[None, :]
    return Rotation(np.ascontiguousarray(R), gamma, bool(normalize), it, converged, np.asarray(crit), variance, communality,
                    kern)
