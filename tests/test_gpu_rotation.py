"""The rotation of dmd_era5_amd/rotation.py on the device against the fp64 reference of tests/varimax_ref.py.

Both sides run a fixed number of steps (``tol=0, max_iter=30``): stopping rules are not compared, fp32 and fp64 stop
one step apart on some inputs.  The tolerance on the matched loadings is measured here, not chosen: 8 times the
deviation the float32 restatement of the step (varimax_ref.step32: the same unit roundoff, another summation order)
shows against fp64 on the same input.  The inputs are structured loadings WITH noise (0.02): on noise-free structure
the criterion is flat in some directions and the restatement itself deviates by 2e-5.
"""
import numpy as np
import pytest
import torch

import varimax_ref as vr

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 30


@pytest.fixture(scope="module")
def KERN():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _blocks(A, cuts):
    edges = [0, *cuts, A.shape[0]]
    return [_t(A[a:b].T) for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("m,k,cuts,normalize,with_s", [(4200, 6, [1801], False, False), (4200, 6, [1801], True, True),
                                                       (9000, 17, [], False, False), (9000, 17, [], True, True)])
def test_orthomax_blocks_against_the_fp64_reference(KERN, m, k, cuts, normalize, with_s):
    from dmd_era5_amd.rotation import orthomax_blocks

    rng = np.random.default_rng(3200 + k)
    A = vr.structured(rng, m, k)[0]
    s = np.linspace(7.0, 1.0, k) if with_s else None
    ref = vr.orthomax(A, s=s, normalize=normalize, tol=0, max_iter=STEPS)
    r32 = vr.orthomax(A, s=s, normalize=normalize, tol=0, max_iter=STEPS, step=vr.step32)
    dev32 = float(np.abs(vr.match_columns(r32["loadings"], ref["loadings"]) - ref["loadings"]).max())
    blocks = _blocks(A, cuts)
    rot = orthomax_blocks(blocks, s=s, normalize=normalize, tol=0, max_iter=STEPS, kern=KERN)
    assert rot.iterations == STEPS and len(rot.criterion) == STEPS + 1 and not rot.converged
    assert np.abs(rot.R.T @ rot.R - np.eye(k)).max() <= 1e-12
    sv = np.ones(k) if s is None else s
    loadings = (A.astype(np.float64) * sv[None, :]) @ rot.R
    err = float(np.abs(vr.match_columns(loadings, ref["loadings"]) - ref["loadings"]).max())
    print(f"rotation m={m} k={k} normalize={normalize}: loadings off by {err:.3e}, float32 restatement by {dev32:.3e}")
    assert err <= 8 * dev32
    c = rot.criterion
    drop = float((-np.diff(c) / np.abs(c[:-1])).max())
    print(f"  criterion {c[0]:.6g} -> {c[-1]:.6g}, largest relative drop between steps {drop:.3e}")
    assert drop <= 1e-6
    assert c[-1] == pytest.approx(ref["criterion"][-1], rel=1e-5)
    assert (np.diff(rot.variance) <= 0).all()
    assert np.allclose(rot.variance, (loadings ** 2).sum(axis=0), rtol=1e-5)
    if normalize:
        h = torch.cat(rot.communality).cpu().numpy()
        assert np.array_equal(h, vr.row_norms(A, None if s is None else s.astype(np.float32)))

    # the rotated patterns: K12's expand of diag(s) R, bit for bit
    P = rot.loadings_blocks(blocks, s=s)
    Ct = _t((sv[:, None] * rot.R).T.astype(np.float32))
    for U, p in zip(blocks, P):
        assert p.shape == U.shape and p.dtype == torch.float32
        assert torch.equal(p, KERN.expand(U, Ct))
    got = torch.cat(P, dim=1).cpu().numpy().T
    assert np.abs(got - loadings).max() <= (k + 2) * 2.0 ** -24 * (np.abs(A).astype(np.float64) @ np.abs(sv[:, None] * rot.R)).max()


def test_masked_rows_stay_zero_and_finite(KERN):
    """The zero rows a masked decomposition leaves in U: weight 0 under Kaiser's normalisation, no NaN anywhere, the
    rotation of the other rows, zero rows in the rotated patterns."""
    from dmd_era5_amd.rotation import orthomax_blocks

    rng = np.random.default_rng(3201)
    m, k, extra = 3000, 5, 333
    A = vr.structured(rng, m, k)[0]
    Z = np.zeros((m + extra, k), dtype=np.float32)
    keep = np.sort(rng.choice(m + extra, m, replace=False))
    gone = np.setdiff1d(np.arange(m + extra), keep)
    Z[keep] = A
    blocks = _blocks(Z, [1203])
    rot = orthomax_blocks(blocks, normalize=True, tol=0, max_iter=STEPS, kern=KERN, n_rows=m)
    ref = vr.orthomax(A, normalize=True, tol=0, max_iter=STEPS)
    r32 = vr.orthomax(A, normalize=True, tol=0, max_iter=STEPS, step=vr.step32)
    dev32 = float(np.abs(vr.match_columns(r32["loadings"], ref["loadings"]) - ref["loadings"]).max())
    assert np.isfinite(rot.R).all() and np.isfinite(rot.criterion).all() and np.isfinite(rot.variance).all()
    loadings = A.astype(np.float64) @ rot.R
    err = float(np.abs(vr.match_columns(loadings, ref["loadings"]) - ref["loadings"]).max())
    print(f"rotation with {extra} zero rows: loadings off by {err:.3e}, float32 restatement by {dev32:.3e}")
    assert err <= 8 * dev32
    h = torch.cat(rot.communality).cpu().numpy()
    assert (h[gone] == 0).all() and (h[keep] > 0).all()
    P = torch.cat(rot.loadings_blocks(blocks), dim=1).cpu().numpy()
    assert np.isfinite(P).all() and (P[:, gone] == 0).all()


def test_refusals(KERN):
    from dmd_era5_amd.rotation import orthomax_blocks

    with pytest.raises(ValueError, match="rotate fewer modes"):
        orthomax_blocks([torch.zeros((KERN.varimax_max_k + 1, 100), device=DEV)], kern=KERN)
