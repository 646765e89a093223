"""Optimized DMD (variable projection) on the reduced coordinates of the snapshot SVD.

The reference only *announces* this step ("makes use of the optimized DMD algorithm",
/root/reference/README.md:85, citation :139 -- Askham & Kutz, "Variable projection methods for an
optimized dynamic mode decomposition", SIADS 2018); it contains no code for it and pydmd is not a
dependency (SURVEY.md header table).  BASELINE config 5 asks for it on the rank-r reduced
coordinates H = (U_r^T X)^T = V_r S  (n snapshots x r), which is what this module fits:

        min over alpha in C^r, B in C^{r x r}   || H - Phi(alpha) B ||_F ,   Phi_ij = exp(alpha_j t_i)

by variable projection: B = Phi^+ H is eliminated, the residual R(alpha) = (I - Phi Phi^+) H is
minimised over alpha with Levenberg-Marquardt.  With Phi = U S V^H, W = diag(t) Phi, C = W^H R,
the Gauss-Newton matrix and gradient of the full Golub-Pereyra Jacobian reduce to r x r pieces
(the cross terms vanish because U^H R = 0):

        J^H J = [(P W)^H (P W)] o [conj(B) B^T]  +  [V S^-2 V^H]^T-type term o [conj(C) C^T]
        J^H rho = -g ,   g_j = sum_s C[j, s] conj(B[j, s]) ,        P = I - U U^H

so one iteration costs an orthonormal basis of the n x r matrix Phi (CholeskyQR2; the economy SVD
only when Phi is too ill-conditioned for it) and a handful of (n x r)^H (n x r) products -- all
dense torch ops on whatever device H lives on (complex128 by default; launch-bound small dense
work at n = 8760, r = 200, not a roofline kernel).
Initial eigenvalues come from the trapezoidal-rule DMD of the same data (Askham & Kutz section 3.3).
``num_trials > 0`` adds the bagging of BOP-DMD (Sashidhar & Kutz 2022): refits on random subsets
of the snapshots, eigenvalue mean / std over the trials.

Parity: **unpinned** (no pydmd, no reference code, no reference fixtures).  The tests pin it on
known answers instead: planted damped complex exponentials, uneven sampling, noise.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

__all__ = ["OptDMDResult", "trapezoidal_dmd_eigs", "exact_dmd_eigs", "initial_eigs", "optdmd", "bopdmd",
           "reduced_coordinates"]


@dataclass
class OptDMDResult:
    eigs: torch.Tensor          # (r,) continuous-time eigenvalues alpha
    modes: torch.Tensor         # (n_s, r) unit-norm modes in the coordinates of H's columns
    amplitudes: torch.Tensor    # (r,) b_j >= 0, H ~ Phi(alpha) diag(b) modes^T
    rel_error: float
    n_iter: int
    converged: bool
    eigs_std: torch.Tensor | None = None   # bagging only
    info: dict = field(default_factory=dict)
    trials: list["OptDMDResult"] | None = None   # bopdmd(keep_trials=True): every trial's own fit

    def reconstruct(self, t: torch.Tensor) -> torch.Tensor:
        """(len(t), n_s) = Phi(alpha) diag(b) modes^T."""
        phi = torch.exp(t.to(self.eigs.real.dtype)[:, None].to(self.eigs.dtype) * self.eigs[None, :])
        return (phi * self.amplitudes.to(self.eigs.dtype)) @ self.modes.T


def reduced_coordinates(s: torch.Tensor, Vh: torch.Tensor) -> torch.Tensor:
    """H = (U_r^T X)^T = V_r S from the SVD factors: (n, r), row i = snapshot i in the U_r basis."""
    return (Vh * s[:, None].to(Vh.dtype)).T.contiguous()


def _phi(alpha: torch.Tensor, t: torch.Tensor, dtype: torch.dtype | None = None) -> torch.Tensor:
    """Phi_ij = exp(alpha_j t_i).  The exponent is always formed in complex128 -- |alpha| t reaches
    ~1.4e4 rad over a year of hourly snapshots at 6 cycles / day, which fp32 would carry to 1e-3 rad
    only -- and the result rounded once to the working dtype."""
    out = dtype or alpha.dtype
    a = alpha.to(torch.complex128)
    tt = (t.real if t.is_complex() else t).to(torch.float64)
    if a.is_cuda and out in (torch.complex64, torch.complex128):
        # one launch of the HIP kernel (dmdx_exp_basis) instead of the outer product / exp / cast chain
        from .kernels import default_kernels

        return default_kernels().exp_basis(a, tt.to(a.device), out, want_w=False)[0]
    return torch.exp(tt[:, None] * a[None, :]).to(out)


def trapezoidal_dmd_eigs(H: torch.Tensor, t: torch.Tensor, r: int) -> torch.Tensor:
    """Initial guess: eigenvalues of the rank-r operator fitted to the trapezoidal rule
    (h_{i+1} - h_i) / dt_i ~ A (h_i + h_{i+1}) / 2   (works for uneven sampling)."""
    X1, X2 = H[:-1].T, H[1:].T                        # (n_s, m-1)
    dt = (t[1:] - t[:-1]).to(H.dtype)
    dX = (X2 - X1) / dt[None, :]
    Xm = 0.5 * (X1 + X2)
    U, S, Vh = torch.linalg.svd(Xm, full_matrices=False)
    r = min(r, int((S > S[0] * 1e-12).sum()))
    U, S, Vh = U[:, :r], S[:r], Vh[:r]
    At = U.conj().T @ dX @ Vh.conj().T / S[None, :]
    return torch.linalg.eigvals(At)


def exact_dmd_eigs(H: torch.Tensor, dt: float, r: int) -> torch.Tensor:
    """Continuous-time eigenvalues log(mu) / dt of the rank-r exact DMD operator h_{i+1} = A h_i
    (uniform sampling).  The trapezoidal rule sees mu through the bilinear map
    lambda = (2 / dt) (mu - 1) / (mu + 1): at omega dt = pi / 2 (6 cycles / day, hourly data) that
    is 27 % off in frequency, far outside the basin of the optimisation (its width is ~1 / T), so
    on uniformly sampled data the one-step operator itself is used."""
    X1, X2 = H[:-1].T, H[1:].T
    U, S, Vh = torch.linalg.svd(X1, full_matrices=False)
    r = min(r, int((S > S[0] * 1e-12).sum()))
    U, S, Vh = U[:, :r], S[:r], Vh[:r]
    At = U.conj().T @ X2 @ Vh.conj().T / S[None, :]
    mu = torch.linalg.eigvals(At)
    return torch.log(mu) / dt


def initial_eigs(H: torch.Tensor, t: torch.Tensor, r: int) -> torch.Tensor:
    """Cold-start eigenvalues (complex128): exact DMD when the sampling is uniform, the
    trapezoidal-rule DMD of Askham & Kutz (section 3.3) otherwise."""
    tr = (t.real if t.is_complex() else t).to(torch.float64)
    dts = tr[1:] - tr[:-1]
    dt = float(dts.mean())
    H128 = H.to(torch.complex128)
    if float((dts - dt).abs().max()) <= 1e-9 * abs(dt):
        return exact_dmd_eigs(H128, dt, r)
    return trapezoidal_dmd_eigs(H128, tr.to(torch.complex128), r)


def _project(alpha, t, H, rank_tol=None, use_qr: bool = True):
    """Variable projection at alpha: (Phi, Q, Ginv, B, R) with Q an orthonormal basis of
    range(Phi), Ginv = (Phi^H Phi)^-1, B = Phi^+ H and R = H - Phi B -- all in H's dtype (alpha
    complex128).  Returns None when Phi is not finite (a trial step into Re(alpha) t > the dtype's
    range).

    Route (round 2): CholeskyQR2 of Phi -- two r x r Grams accumulated in complex128, two
    Cholesky factorisations, two triangular solves: ~10 small launches, ~2 ms at n = 8760,
    r = 200 -- instead of the economy SVD (rocSOLVER gesvd of the 8760 x 200 matrix: ~90 ms of
    launch-bound time per evaluation, i.e. the whole iteration).  Exponentials whose frequencies
    are separated by more than ~1 / T are nearly orthogonal, which is the regime of the fit; when
    the basis is too ill-conditioned for the Gram route (Cholesky fails, or the factor's diagonal
    spans more than 1 / rank_tol) the SVD route takes over, with its truncation of the null
    directions."""
    Phi = _phi(alpha, t, H.dtype)
    if not bool(torch.isfinite(Phi.real).all() and torch.isfinite(Phi.imag).all()):
        return None
    if rank_tol is None:
        rank_tol = 1e-12 if H.dtype == torch.complex128 else 1e-6
    if use_qr:
        Q, Rt = Phi, None
        ok = True
        for _ in range(2):
            Qd = Q.to(torch.complex128)          # the r x r Gram in complex128 whatever the working dtype:
            G = Qd.conj().T @ Qd                  # fp32 sums would cap the usable cond(Phi) at ~3e3
            L, err = torch.linalg.cholesky_ex(G)
            d = torch.diagonal(L).real
            if int(err) != 0 or not bool(torch.isfinite(d).all()) or float(d.min()) < math.sqrt(rank_tol) * float(d.max()):
                ok = False
                break
            Rk = L.conj().T                                           # Q_old = Q_new Rk
            Q = torch.linalg.solve_triangular(Rk.to(H.dtype), Q, upper=True, left=False)
            Rt = Rk if Rt is None else Rk @ Rt
        if ok:
            Rinv = torch.linalg.solve_triangular(Rt, torch.eye(Rt.shape[0], dtype=Rt.dtype, device=Rt.device), upper=True)
            QhH = Q.conj().T @ H
            B = Rinv.to(H.dtype) @ QhH
            R = H - Q @ QhH
            Ginv = (Rinv @ Rinv.conj().T).to(H.dtype)
            return Phi, Q, Ginv, B, R
    U, S, Vh = torch.linalg.svd(Phi, full_matrices=False)
    keep = int((S > S[0] * rank_tol).sum())
    U, S, Vh = U[:, :keep], S[:keep], Vh[:keep]
    UhH = U.conj().T @ H
    B = Vh.conj().T @ (UhH / S[:, None].to(H.dtype))
    R = H - U @ UhH
    Ginv = Vh.conj().T @ (Vh / (S[:, None].to(H.dtype) ** 2))
    return Phi, U, Ginv, B, R


class _GramEval:
    """One evaluation of the variable projection at alpha on the GPU, from ONE pass over the tall
    matrices (round 3; replaces CholeskyQR2 of Phi through rocSOLVER / rocBLAS trsm + six tall complex
    GEMMs per Levenberg-Marquardt iteration, ~35 library launches of 8-18 ms in all):

    * Phi = exp(t alpha^T) and W = diag(t) Phi: one launch of ``dmdx_exp_basis`` (complex128);
    * the complex Gram block  [Phi W]^H [Phi W H]  as the REAL product of the interleaved
      (re, im) views -- a complex n x c matrix is a real n x 2c matrix in memory -- on the fp64 MFMA
      kernel K9 (``gemm_tn64``: one launch + its reduce); the four real blocks (rr, ri, ir, ii) of
      every complex entry are recombined on the small result:  A^H B = (rr + ii) + i (ri - ir);
    * G = Phi^H Phi = L L^H through K10 on the real embedding [[Gr, -Gi], [Gi, Gr]] (symmetric
      positive definite, order 2r <= 1024): one launch gives the factor's inverse, hence
      G^-1 and B = G^-1 Phi^H H;  the Levenberg-Marquardt system (J^H J + lambda D) delta = g is
      Hermitian positive definite and solved the same way (was an LU through rocSOLVER);
    * the residual R = H - Phi B explicitly (its norm decides acceptance and convergence: formed
      from Gram pieces it would lose everything below 1e-8 ||H||), as the real product
      [Phi_r Phi_i] M on K11;  C = W^H R, P W and the Gauss-Newton pieces from the Gram blocks:
      (P W)^H (P W) = W^H W - (W^H Phi) G^-1 (Phi^H W),   C = W^H H - (W^H Phi) B.

    Everything is complex128 whatever H's dtype (complex64 input is cast once: the n x r basis is
    28 MB).  A basis too ill-conditioned for the normal equations (K10 reports a failed
    factorisation or a diagonal spread beyond 1 / sqrt(rank_tol)) makes ``evaluate`` return False:
    the caller switches to the library route (economy SVD with truncation) for good."""

    def __init__(self, H: torch.Tensor, t: torch.Tensor, kern):
        self.kern = kern
        self.H = H.to(torch.complex128).contiguous()
        self.t = t
        n, ns = self.H.shape
        self.n, self.ns = n, ns
        self.normH2 = float((self.H.real ** 2 + self.H.imag ** 2).sum())
        self.buf = None

    @staticmethod
    def _cplx(Cm: torch.Tensor, a: int, b: int) -> torch.Tensor:
        """Real product of interleaved views (2a x 2b) -> complex A^H B (a x b)."""
        v = Cm.view(a, 2, b, 2)
        return torch.complex(v[:, 0, :, 0] + v[:, 1, :, 1], v[:, 0, :, 1] - v[:, 1, :, 0])

    @staticmethod
    def _embed(G: torch.Tensor) -> torch.Tensor:
        """Hermitian G (r x r complex) -> the real symmetric [[Gr, -Gi], [Gi, Gr]] (2r x 2r)."""
        Gr, Gi = G.real, G.imag
        return torch.cat([torch.cat([Gr, -Gi], dim=1), torch.cat([Gi, Gr], dim=1)], dim=0).contiguous()

    def _solve_hpd(self, G: torch.Tensor, Y: torch.Tensor, rank_tol: float | None):
        """G^-1 Y and G^-1 for Hermitian positive definite G: K10 on the real embedding."""
        r = G.shape[0]
        if 2 * r > getattr(self.kern, "chol_max_n", 0):
            return None
        L, Linv, info = self.kern.chol_inv(self._embed(G))
        st, dmin, dmax = info.tolist()
        if st != 0.0 or not (math.isfinite(dmin) and math.isfinite(dmax)) or dmin <= 0.0:
            return None
        if rank_tol is not None and dmin < math.sqrt(rank_tol) * dmax:
            return None
        Ginv_e = Linv.T @ Linv                                   # (2r, 2r) = embedding of G^-1
        Ginv = torch.complex(Ginv_e[:r, :r], Ginv_e[r:, :r])
        return Ginv @ Y, Ginv

    def evaluate(self, alpha: torch.Tensor, rank_tol: float = 1e-12):
        """-> dict of the pieces at alpha, None when exp(alpha t) is not finite, False when the basis
        is too ill-conditioned for this route."""
        kern, n, ns = self.kern, self.n, self.ns
        r = alpha.numel()
        Phi, W = kern.exp_basis(alpha, self.t, torch.complex128, want_w=True)
        if self.buf is None or self.buf.shape[1] != 2 * r + ns:
            self.buf = torch.empty((n, 2 * r + ns), dtype=torch.complex128, device=self.H.device)
            self.buf[:, 2 * r:] = self.H
        self.buf[:, :r] = Phi
        self.buf[:, r:2 * r] = W
        F = torch.view_as_real(self.buf).reshape(n, 2 * (2 * r + ns))     # interleaved (re, im) columns
        Cm = kern.gemm_tn64(F[:, :4 * r], F)                               # (4r, 4r + 2 ns) real
        S = self._cplx(Cm, 2 * r, 2 * r + ns)                              # [Phi W]^H [Phi W H]
        if not bool(torch.isfinite(torch.diagonal(S[:r, :r]).real).all()):
            return None
        PhP, PhW, PhH = S[:r, :r], S[:r, r:2 * r], S[:r, 2 * r:]
        WhW, WhH = S[r:, r:2 * r], S[r:, 2 * r:]
        PhP = 0.5 * (PhP + PhP.conj().T)
        sol = self._solve_hpd(PhP, torch.cat([PhH, PhW], dim=1), rank_tol)
        if sol is None:
            return False
        X, Ginv = sol
        B, GiPhW = X[:, :ns], X[:, ns:]                                   # B = G^-1 Phi^H H ; G^-1 Phi^H W
        # R = H - Phi B as a real product on K11: [Phi_r | Phi_i interleaved] (n x 2r) times the real
        # (2r x 2 ns) image of B, given transposed
        Bt = torch.view_as_real(B.T.contiguous())                          # (ns, r, 2): [j][c] -> (Br, Bi)
        Mt = torch.stack([torch.stack([Bt[..., 0], -Bt[..., 1]], dim=-1).reshape(ns, 2 * r),
                          torch.stack([Bt[..., 1], Bt[..., 0]], dim=-1).reshape(ns, 2 * r)], dim=1).reshape(2 * ns, 2 * r)
        PB = kern.gemm_nt64(F[:, :2 * r], Mt.contiguous())                 # (n, 2 ns) = interleaved Phi B
        R = self.H - torch.view_as_complex(PB.view(n, ns, 2))
        res2 = float((R.real ** 2 + R.imag ** 2).sum())
        return {"Phi": Phi, "B": B, "R": R, "err": math.sqrt(max(res2, 0.0) / max(self.normH2, 1e-300)), "Ginv": Ginv,
                "WhH": WhH, "WhW": WhW, "PhW": PhW, "GiPhW": GiPhW}

    def normal_matrix(self, pc: dict):
        """(J^H J, g) of the variable-projection functional from the pieces of ``evaluate``."""
        B, Ginv = pc["B"], pc["Ginv"]
        WhP = pc["PhW"].conj().T
        PWhPW = pc["WhW"] - WhP @ pc["GiPhW"]                              # (P W)^H (P W), P = I - Phi G^-1 Phi^H
        PWhPW = 0.5 * (PWhPW + PWhPW.conj().T)
        C = pc["WhH"] - WhP @ B                                            # W^H R
        JtJ = PWhPW * (B.conj() @ B.T) + Ginv * (C.conj() @ C.T)
        g = (C * B.conj()).sum(dim=1)
        return 0.5 * (JtJ + JtJ.conj().T), g

    def lm_step(self, JtJ: torch.Tensor, g: torch.Tensor, dg: torch.Tensor, lmb: float):
        sol = self._solve_hpd(JtJ + lmb * torch.diag(dg), g[:, None], None)
        if sol is None:
            return torch.linalg.solve(JtJ + lmb * torch.diag(dg), g)
        return sol[0][:, 0]


def _gram_route(H: torch.Tensor):
    """The HIP kernel provider when H lives on a GPU with libdmdx (else None: library route)."""
    if not H.is_cuda:
        return None
    try:
        from .kernels import default_kernels

        kern = default_kernels()
    except Exception:
        return None
    return kern if all(hasattr(kern, f) for f in ("gemm_tn64", "chol_inv", "gemm_nt64", "exp_basis")) else None


def optdmd(H: torch.Tensor, t: torch.Tensor, r: int, alpha0: torch.Tensor | None = None,
           maxiter: int = 30, tol: float = 1e-6, eps_stall: float | None = None, init_lambda: float = 1.0,
           lamup: float = 2.0, maxlam: int = 52) -> OptDMDResult:
    """Optimized DMD of the rows of H (snapshots at times t) with r exponentials.

    Defaults (maxiter 30, tol 1e-6, eps_stall 1e-12, lambda 1, x2 up to 52 times) are the ones
    commonly used for this algorithm; tol is on the relative residual ||R||_F / ||H||_F.
    ``eps_stall`` (relative gain below which the iteration counts as stalled): None = 1e-12 in
    complex128 and 1e-6 in complex64 -- there the residual norm itself carries ~1e-7 of rounding,
    and a tighter test makes every late iteration walk lambda through all its 52 doublings (one
    projection each) before it gives up: measured 59 instead of 9 ms per iteration at cfg5."""
    cdtype = torch.complex128 if H.dtype in (torch.float64, torch.complex128) else torch.complex64
    rdtype = torch.float64 if cdtype == torch.complex128 else torch.float32
    if eps_stall is None:
        eps_stall = 1e-12 if cdtype == torch.complex128 else 1e-6
    H = H.to(cdtype)
    t = (t.real if t.is_complex() else t).to(device=H.device, dtype=torch.float64)
    # the parameters stay complex128 whatever the working dtype of the n x r matrices is
    alpha = (initial_eigs(H, t, r) if alpha0 is None else alpha0).to(device=H.device, dtype=torch.complex128)
    r = alpha.numel()
    tw = t.to(rdtype).to(cdtype)
    normH = torch.linalg.norm(H)
    lam = float(init_lambda)

    # Two routes to the same pieces (B, the residual norm, J^H J and g): the Gram route on our own
    # kernels (_GramEval: GPU, complex128 inside) and the library route (_project: CholeskyQR2 / SVD
    # of Phi through torch -- the CPU path, and the fallback for ill-conditioned bases).
    kern = _gram_route(H)
    ge = _GramEval(H, t, kern) if kern is not None else None
    route = {"gram": ge is not None}

    def evaluate(a):
        """-> (err, B, normal) with normal() -> (JtJ, g) in complex128, or None (not finite)."""
        if route["gram"]:
            pc = ge.evaluate(a)
            if pc is None:
                return None
            if pc is not False:
                return pc["err"], pc["B"], (lambda pc=pc: ge.normal_matrix(pc))
            route["gram"] = False                                   # ill-conditioned basis: library route from here on
        pieces = _project(a, t, H)
        if pieces is None or not bool(torch.isfinite(pieces[4].real).all()):
            return None
        Phi, U, Ginv, B, R = pieces

        def normal():
            W = tw[:, None] * Phi
            PW = W - U @ (U.conj().T @ W)
            C = W.conj().T @ R                                           # (r, n_s)
            A1 = (PW.conj().T @ PW) * (B.conj() @ B.T)
            A2 = Ginv * (C.conj() @ C.T)                                  # (Phi^H Phi)^-1 = V S^-2 V^H
            return (A1 + A2).to(torch.complex128), (C * B.conj()).sum(dim=1).to(torch.complex128)

        return float(torch.linalg.norm(R) / normH), B, normal

    state = evaluate(alpha)
    if state is None:
        raise ValueError("optdmd: exp(alpha0 * t) is not finite in the working dtype")
    err, B, normal = state
    n_iter, converged = 0, err < tol
    errs = [err]
    n_proj = 1
    while n_iter < maxiter and not converged:
        n_iter += 1
        JtJ, g = normal()
        dg = torch.diagonal(JtJ).real.clamp_min(1e-300).to(torch.complex128)

        def trial(lmb):
            if route["gram"]:
                delta = ge.lm_step(JtJ, g, dg, lmb)
            else:
                delta = torch.linalg.solve(JtJ + lmb * torch.diag(dg), g)
            a_new = alpha + delta
            st = evaluate(a_new)
            nonlocal n_proj
            n_proj += 1
            if st is None:
                return a_new, None, math.inf
            return a_new, st, st[0]

        a_new, st, e_new = trial(lam)
        if e_new < err:
            lam = max(lam / lamup, 1e-12)
        else:
            improved = False
            for _ in range(maxlam):
                lam *= lamup
                a_new, st, e_new = trial(lam)
                if e_new < err:
                    improved = True
                    break
            if not improved:
                break                                               # stalled: keep the current alpha
        gain = err - e_new
        alpha, err = a_new, e_new
        _, B, normal = st
        errs.append(err)
        if err < tol:
            converged = True
        elif gain < eps_stall * max(err, 1e-300):
            break
    B = B.to(cdtype)
    alpha = alpha.to(cdtype)
    amp = torch.linalg.norm(B, dim=1)
    modes = (B / amp[:, None].clamp_min(1e-300).to(cdtype)).T.contiguous()
    order = torch.argsort(-amp)
    return OptDMDResult(eigs=alpha[order], modes=modes[:, order], amplitudes=amp[order].to(rdtype),
                        rel_error=err, n_iter=n_iter, converged=converged,
                        info={"errors": errs, "lambda": lam, "projections": n_proj,
                              "route": "gram (K9 / K10 / K11)" if route["gram"] else "library"})


def _match(reference: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """Greedy nearest-neighbour assignment of ``values`` to ``reference`` (both (r,))."""
    out = torch.empty_like(reference)
    free = list(range(values.numel()))
    for i in torch.argsort(-reference.abs()).tolist():
        d = (values[free] - reference[i]).abs()
        j = int(torch.argmin(d))
        out[i] = values[free[j]]
        free.pop(j)
    return out


def bopdmd(H: torch.Tensor, t: torch.Tensor, r: int, num_trials: int = 0, trial_size: float = 0.6,
           seed: int = 0, keep_trials: bool = False, **kwargs) -> OptDMDResult:
    """Optimized DMD with optional bagging: ``num_trials`` refits on random subsets
    (``trial_size`` of the snapshots, without replacement, kept in time order) started from the
    full-data eigenvalues; the reported eigenvalues are the trial mean, ``eigs_std`` their spread,
    modes / amplitudes come from the projection of the full data on the averaged eigenvalues.

    ``keep_trials=True`` keeps what the bag knows beyond the eigenvalues: ``trials`` holds the untouched
    ``optdmd`` result of every trial (an ensemble of models: forecast.ensemble_coefficients,
    DmdForecast.ensemble_fields / ensemble_score) and ``info["trial_indices"]`` the sorted snapshot indices
    each was fitted on.  Every other field is the same, bit for bit, as without it."""
    base = optdmd(H, t, r, **kwargs)
    if num_trials <= 0:
        return base
    rs = np.random.RandomState(seed)
    m = H.shape[0]
    size = max(2 * r, int(round(trial_size * m))) if trial_size <= 1 else int(trial_size)
    size = min(size, m)
    trials, kept, kept_idx = [], [], []
    for _ in range(num_trials):
        idx = torch.from_numpy(np.sort(rs.choice(m, size=size, replace=False))).to(H.device)
        res = optdmd(H[idx], t[idx], r, alpha0=base.eigs, **kwargs)
        trials.append(_match(base.eigs, res.eigs))
        if keep_trials:
            kept.append(res)
            kept_idx.append(idx.cpu())
    A = torch.stack(trials)
    mean = A.mean(dim=0)
    std = torch.sqrt(((A - mean).abs() ** 2).mean(dim=0))
    cdtype = mean.dtype
    _, _, _, B, R = _project(mean.to(torch.complex128), t.to(H.device), H.to(cdtype))
    amp = torch.linalg.norm(B, dim=1)
    modes = (B / amp[:, None].clamp_min(1e-300).to(cdtype)).T.contiguous()
    order = torch.argsort(-amp)
    info = {"num_trials": num_trials, "trial_size": size, "base_error": base.rel_error}
    if keep_trials:
        info["trial_indices"] = kept_idx
    return OptDMDResult(eigs=mean[order], modes=modes[:, order], amplitudes=amp[order].to(std.dtype),
                        rel_error=float(torch.linalg.norm(R) / torch.linalg.norm(H)),
                        n_iter=base.n_iter, converged=base.converged, eigs_std=std[order],
                        info=info, trials=kept if keep_trials else None)
