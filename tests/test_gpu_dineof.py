"""DINEOF end to end on the GPU (dmd_era5_amd/gapfill.py over HipKernels) against the plain fp64 DINEOF of
tests/gap_ref.py, run in the test on the same field.

Field: m = 300, T = 96 fp32, per-row offset ~ 280, three temporal modes (periods 24, 37, 11; amplitudes 3, 2, 1.2), white
noise 0.05.  Gaps: 8 % scattered, a box of 80 rows x 30 snapshots, 30 rows half missing, one snapshot missing everywhere,
one row missing everywhere.  max_rank = 8, cv_fraction = 0.03.  The reference chooses rank 4: the three modes and the
rank-one offset that the gappy row means leave.

The tolerance g is half the reference's own relative distance between its best and its second-best rank (0.00719
here: cv_error 0.05375153 at rank 4, 0.05452463 at rank 5), computed in the test: an engine whose cross-validation error is within g of the reference's minimum cannot have
preferred a rank the reference separates from its best by 2 g.  Measured on an MI355X (MEASUREMENTS.md "K31"): the
engine's cv_error at its rank over the reference's minimum, and the same ratio of the rms error at the true gaps, both
printed below before they are asserted.
"""
import numpy as np
import pytest
import torch

import gap_ref as gr

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def problem():
    truth, X = gr.synthetic(0)
    return truth, X, gr.dineof64(X, 8, cv_fraction=0.03, seed=0)


def _run(X, cuts, **kw):
    from dmd_era5_amd.gapfill import dineof_blocks

    edges = [0, *cuts, X.shape[0]]
    blocks = [torch.from_numpy(np.ascontiguousarray(X[a:b].T)).to(DEV) for a, b in zip(edges[:-1], edges[1:])]
    fit = dineof_blocks(blocks, 8, cv_fraction=0.03, seed=0, **kw)
    return fit, torch.cat(blocks, dim=1).cpu().numpy().T


@pytest.mark.parametrize("svd", ["snapshots", "randomized"])
def test_engine_matches_the_fp64_reference(problem, svd):
    truth, X, ref = problem
    fit, F = _run(X, [130], svd=svd)
    e_ref = ref["cv_error"][1:]
    best, second = np.sort(e_ref)[:2]
    g = 0.5 * (second - best) / best
    gaps = ref["gaps"] & ~ref["row_mask"][:, None]
    rms_ref = np.sqrt(((ref["filled"] - truth)[gaps] ** 2).mean())
    rms = np.sqrt(((F.astype(np.float64) - truth)[gaps] ** 2).mean())
    print(f"{svd}: g = {g:.5f}; reference rank {ref['rank']} cv_error {e_ref}; engine rank {fit.rank} cv_error "
          f"{fit.cv_error[1:]}; ratio of the minima {fit.cv_error[fit.rank] / best:.6f}; rms at the gaps {rms:.6f} against "
          f"{rms_ref:.6f}, ratio {rms / rms_ref:.6f}; iterations {fit.iterations} against {ref['iterations']}")
    assert ref["rank"] == 4 and 0.001 < g < 0.05
    assert e_ref[fit.rank - 1] <= best * (1 + g)
    assert fit.cv_error[fit.rank] <= best * (1 + g)
    assert rms <= rms_ref * (1 + g)
    assert fit.converged and (fit.n_missing, fit.n_cv) == (ref["n_missing"], ref["n_cv"])
    assert fit.expected_error == fit.cv_error[fit.rank]

    # the masked row is NaN, the all-missing snapshot is finite, every observed element is unchanged to the round trip
    # of standardize (one rounding of x - mean, one of z + mean at values below 512: 2^-15)
    rowm = np.concatenate([r.cpu().numpy() for r in fit.row_mask])
    assert rowm.tolist() == [i == 17 for i in range(300)]
    assert np.isnan(F[17]).all() and np.isfinite(F[~rowm]).all() and np.isfinite(F[~rowm, 55]).all()
    seen = ~gr.gap_bits(X)
    assert np.abs(F[seen].astype(np.float64) - X[seen]).max() <= 2.0 ** -15
    bits = gr.unpack_bits(np.concatenate([w.cpu().numpy().view(np.uint32) for w in fit.masks], axis=1), 96)
    assert np.array_equal(bits[~rowm], gr.gap_bits(X)[~rowm]) and bits[rowm].all()

    # fit.svd reconstructs the filled Z to within its own truncation: it is the SVD of the field before the last fill,
    # which moved the gaps by no more than tol scale0 in the rms (0.01 in the norm below covers that and the 2^-16 per
    # element of forming Z from the stored field); the best rank-r approximation leaves the tail of the spectrum
    mean = np.concatenate([v.cpu().numpy() for v in fit.mean]).astype(np.float64)
    Z = (F.astype(np.float64) - mean[:, None])[~rowm]
    U = fit.svd.Ut.cpu().numpy().astype(np.float64).T[~rowm]
    R = (U * fit.svd.s.cpu().numpy()[None, :]) @ fit.svd.Vh.cpu().numpy()
    tail = np.sqrt((np.linalg.svd(Z, compute_uv=False)[fit.rank:] ** 2).sum())
    err = np.sqrt(((Z - R) ** 2).sum())
    print(f"|Z - U S Vh| = {err:.5f}, tail of the spectrum {tail:.5f}")
    assert fit.svd.Ut.shape == (fit.rank, 300) and err <= 1.001 * tail + 0.01


def test_blocks_and_scale(problem):
    """Three blocks instead of two give the same decisions; with scale the data come back in raw units."""
    truth, X, ref = problem
    fit2, F2 = _run(X, [130])
    fit3, F3 = _run(X, [77, 200])
    assert fit3.rank == fit2.rank and fit3.n_cv == fit2.n_cv
    n = min(len(fit2.cv_error), len(fit3.cv_error))
    assert np.allclose(fit3.cv_error[1:n], fit2.cv_error[1:n], rtol=1e-2)       # (the block sums of the Gram in another order)
    fits, Fs = _run(X, [130], scale=True)
    rowm = np.concatenate([r.cpu().numpy() for r in fits.row_mask])
    gaps = ref["gaps"] & ~rowm[:, None]
    rms = np.sqrt(((Fs.astype(np.float64) - truth)[gaps] ** 2).mean())
    rms_ref = np.sqrt(((ref["filled"] - truth)[gaps] ** 2).mean())
    print(f"scale: rank {fits.rank}, cv_error {fits.cv_error[1:]}, rms at the gaps {rms:.5f} (unscaled reference {rms_ref:.5f})")
    assert fits.scaled and fits.scale0 == pytest.approx(1.0, rel=1e-9) and rowm.sum() == 1 and np.isnan(Fs[17]).all()
    seen = ~gr.gap_bits(X)
    assert np.abs(Fs[seen].astype(np.float64) - X[seen]).max() <= 2.0 ** -14     # a rounded product more than without scale
