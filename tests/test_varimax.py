"""K30 without a GPU: the numpy reference of the step (tests/varimax_ref.py) against values worked out by hand, the
iteration against the closed-form k = 2 angle and a planted simple structure, and the host layer
(dmd_era5_amd/rotation.py) over the CPU double of the kernels."""
import numpy as np
import pytest
import torch

import varimax_ref as vr
from expand_ref import ExpandDouble
from kernel_double import CpuKernelDouble


class Double(vr.VarimaxDouble, ExpandDouble, CpuKernelDouble):
    pass


class CountingComm:
    """A one-rank communicator that records what it is asked to reduce."""

    world_size, rank, exchanges = 1, 0, True

    def __init__(self):
        self.calls = []

    def allreduce_sum_(self, t, tag="allreduce"):
        self.calls.append((tag, int(t.numel()), t.dtype))
        return t


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _blocks(A, cuts):
    edges = [0, *cuts, A.shape[0]]
    return [_t(A[a:b].T) for a, b in zip(edges[:-1], edges[1:])]


def test_reference_step_by_hand():
    U = np.array([[1, 2], [0, 1], [-1, 1]], dtype=np.float32)
    R = np.array([[1, 1], [0, 2]], dtype=np.float32)
    # L = [[1, 5], [0, 2], [-1, 1]]
    G, q, f = vr.step64(U, R)
    assert np.array_equal(G, [[2, 124], [1, 259]]) and np.array_equal(q, [2, 30]) and np.array_equal(f, [2, 642])
    # w = (2, 1, 1/2): a = [[2, 4], [0, 1], [-.5, .5]], L = [[2, 10], [0, 2], [-.5, .5]]
    G, q, f = vr.step64(U, R, np.array([2, 1, 0.5], dtype=np.float32))
    assert np.array_equal(G, [[16.0625, 1999.9375], [31.9375, 4008.0625]])
    assert np.array_equal(q, [4.25, 104.25]) and np.array_equal(f, [16.0625, 10016.0625])
    for got, want in zip(vr.step32(U, R), vr.step64(U, R)):
        assert np.array_equal(got, want)                      # small integers: fp32 is exact
    bG, bq, bf = vr.step_bounds(U, R)
    assert np.allclose(bG, (4096 + 14) * vr.U24 * np.array([[2, 152], [3, 285]]))   # Labs = [[1, 5], [0, 2], [1, 3]]
    assert np.allclose(bq, (4096 + 10) * vr.U24 * np.array([2, 38])) and np.allclose(bf, (4096 + 16) * vr.U24 * np.array([2, 722]))
    assert np.array_equal(vr.row_norms(np.array([[3, 4], [0, 0]], dtype=np.float32)), np.array([5, 0], dtype=np.float32))
    assert np.array_equal(vr.row_norms(np.array([[3, 2]], dtype=np.float32), np.array([1, 2], dtype=np.float32)), [5])


def test_iteration_reaches_the_closed_form_angle_of_two_columns():
    rng = np.random.default_rng(3001)
    for trial in range(4):
        A = vr.structured(rng, 400, 2, noise=0.1, dtype=np.float64)[0].astype(np.float32)
        res = vr.orthomax(A, normalize=False, max_iter=300, tol=0, round_R=False)   # (a fixed point of R, not a line search)
        theta = np.arctan2(res["R"][1, 0], res["R"][0, 0])
        diff = (theta - vr.varimax_angle_k2(A) + np.pi / 4) % (np.pi / 2) - np.pi / 4
        print("k = 2 angle: iteration - closed form =", diff)
        assert abs(diff) < 1e-8, (trial, diff)


def _criterion(L, gamma=1.0):
    m = L.shape[0]
    return float(((L ** 4).sum(axis=0) / m - gamma * ((L ** 2).sum(axis=0) / m) ** 2).sum())


@pytest.mark.parametrize("m,k,gamma", [(600, 3, 1.0), (1500, 6, 1.0), (900, 5, 0.0), (900, 4, 0.5)])
def test_recovers_simple_structure_and_stays_orthogonal(m, k, gamma):
    rng = np.random.default_rng(3002 + k)
    A, simple, _ = vr.structured(rng, m, k)
    res = vr.orthomax(A, gamma=gamma, normalize=False, max_iter=200, tol=1e-10, round_R=False)
    assert res["converged"]
    R = res["R"]
    assert np.abs(R.T @ R - np.eye(k)).max() <= 1e-12
    got = vr.match_columns(res["loadings"], simple)
    assert np.abs(got - simple).max() < 0.05              # the noise is 0.02 per element; 1e-2 of the structure moves
    c = res["criterion"]
    assert (np.diff(c) >= -1e-12 * np.abs(c[:-1])).all()
    assert c[-1] == pytest.approx(_criterion(A.astype(np.float64) @ R, gamma), rel=1e-12)
    assert c[-1] >= _criterion(simple, gamma) * (1 - 1e-3)
    v = res["variance"]
    assert (np.diff(v) <= 0).all() and np.allclose(v, (res["loadings"] ** 2).sum(axis=0), rtol=1e-12)
    assert (R[np.abs(R).argmax(axis=0), np.arange(k)] > 0).all()


def test_product_iteration_is_the_reference_iteration():
    """orthomax_blocks over the double, two row blocks, against the reference on the stacked rows: the same fp64
    arithmetic up to the order of the block sums."""
    from dmd_era5_amd.rotation import orthomax_blocks

    rng = np.random.default_rng(3003)
    m, k = 700, 5
    A = vr.structured(rng, m, k)[0]
    s = np.linspace(9.0, 1.0, k)
    for normalize, sv in ((False, None), (True, None), (True, s), (False, s)):
        comm = CountingComm()
        rot = orthomax_blocks(_blocks(A, [301]), s=sv, normalize=normalize, kern=Double(), comm=comm, tol=1e-9)
        ref = vr.orthomax(A, s=sv, normalize=normalize, tol=1e-9)
        assert rot.iterations == ref["iterations"] and rot.converged and ref["converged"]
        assert np.abs(rot.R - ref["R"]).max() < 1e-9
        assert np.allclose(rot.criterion, ref["criterion"], rtol=1e-10) and np.allclose(rot.variance, ref["variance"], rtol=1e-10)
        assert np.abs(rot.R.T @ rot.R - np.eye(k)).max() <= 1e-12
        assert rot.normalized == normalize and rot.gamma == 1.0 and len(rot.criterion) == rot.iterations + 1
        # one all-reduce of the two Gram matrices and the row count, then k^2 + 2 k doubles per evaluation
        assert comm.calls[0] == ("orthomax_gram_allreduce", 2 * k * k + 1, torch.float64)
        assert [c[1:] for c in comm.calls[1:]] == [(k * k + 2 * k, torch.float64)] * (rot.iterations + 1)
        assert (rot.communality is not None) == normalize
        if normalize:
            h = np.concatenate([v.numpy() for v in rot.communality])
            assert np.array_equal(h, vr.row_norms(A, None if sv is None else sv.astype(np.float32)))


def test_algebra_of_s_and_normalize():
    """s: rotating U with s equals rotating the matrix U diag(s) (s powers of two: the same fp32 products).  normalize:
    equals the plain rotation of the matrix with unit rows, and a positive scale per row changes nothing."""
    rng = np.random.default_rng(3004)
    m, k = 500, 4
    A = vr.structured(rng, m, k)[0]
    s = np.array([8.0, 4.0, 2.0, 0.5])
    a = vr.orthomax(A, s=s, normalize=False, tol=1e-10)
    b = vr.orthomax((A * s.astype(np.float32)[None, :]).astype(np.float32), normalize=False, tol=1e-10)
    assert np.abs(a["R"] - b["R"]).max() < 1e-9 and np.abs(a["loadings"] - b["loadings"]).max() < 1e-8
    h = vr.row_norms(A).astype(np.float64)
    unit = (A / h[:, None]).astype(np.float32)
    c = vr.orthomax(A, normalize=True, tol=1e-10)
    d = vr.orthomax(unit, normalize=False, tol=1e-10)
    # fl(A / h) against fl(A fl(1 / h)): fp32 roundings of the input; the variances that order the columns are others
    assert np.abs(c["R"] - vr.match_columns(d["R"], c["R"])).max() < 1e-5
    scale = (2.0 ** rng.integers(-3, 4, m)).astype(np.float32)
    e = vr.orthomax(A * scale[:, None], normalize=True, tol=1e-10)
    assert np.abs(c["R"] - vr.match_columns(e["R"], c["R"])).max() < 1e-6


def test_zero_rows_contribute_nothing_under_normalisation():
    from dmd_era5_amd.rotation import orthomax_blocks

    rng = np.random.default_rng(3005)
    m, k = 400, 3
    A = vr.structured(rng, m, k)[0]
    Z = np.zeros((m + 50, k), dtype=np.float32)
    keep = np.sort(rng.choice(m + 50, m, replace=False))
    Z[keep] = A
    with np.errstate(all="raise"):
        rot = orthomax_blocks(_blocks(Z, [123]), normalize=True, kern=Double(), n_rows=m, tol=1e-10)
    ref = vr.orthomax(A, normalize=True, tol=1e-10)
    assert np.isfinite(rot.R).all() and np.isfinite(rot.criterion).all()
    assert np.abs(rot.R - ref["R"]).max() < 1e-9
    h = np.concatenate([v.numpy() for v in rot.communality])
    assert (h[np.setdiff1d(np.arange(m + 50), keep)] == 0).all()
    P = torch.cat(rot.loadings_blocks(_blocks(Z, [123])), dim=1).numpy()
    assert (P[:, np.setdiff1d(np.arange(m + 50), keep)] == 0).all()


def test_loadings_coefficients_and_refusals():
    from dmd_era5_amd.rotation import orthomax_blocks

    rng = np.random.default_rng(3006)
    m, k, T = 300, 4, 7
    A = vr.structured(rng, m, k)[0]
    s = np.array([5.0, 3.0, 2.0, 1.0])
    kern = Double()
    rot = orthomax_blocks(_blocks(A, [100]), s=s, kern=kern)
    P = torch.cat(rot.loadings_blocks(_blocks(A, [100]), s=s), dim=1).numpy().T
    want = (A.astype(np.float64) * s[None, :]) @ rot.R
    assert np.abs(P - want).max() < 1e-5
    assert (np.diff((want ** 2).sum(axis=0)) <= 0).all() and np.allclose(rot.variance, (want ** 2).sum(axis=0), rtol=1e-10)
    C = rng.standard_normal((k, T))
    assert np.array_equal(rot.coefficients(C), rot.R.T @ C)
    Ct = rot.coefficients(_t(C, torch.float64))
    assert isinstance(Ct, torch.Tensor) and np.allclose(Ct.numpy(), rot.R.T @ C, rtol=1e-14, atol=1e-14)
    # the rotated patterns times the rotated coefficients are the unrotated product
    assert np.allclose(want @ rot.coefficients(C), (A.astype(np.float64) * s[None, :]) @ C, atol=1e-12)
    with pytest.raises(ValueError, match="rotate fewer modes"):
        orthomax_blocks([torch.zeros((kern.varimax_max_k + 1, 10))], kern=kern)
    with pytest.raises(ValueError):
        orthomax_blocks(_blocks(A, [100]), s=s[:3], kern=kern)
    with pytest.raises(ValueError):
        orthomax_blocks([], kern=kern)
    with pytest.raises(ValueError):
        rot.coefficients(C[:3])
    bad = A.copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        orthomax_blocks(_blocks(bad, [100]), normalize=False, kern=kern)


def test_fixed_step_count_and_quartimax():
    from dmd_era5_amd.rotation import orthomax_blocks

    A = vr.structured(np.random.default_rng(3007), 300, 3)[0]
    rot = orthomax_blocks(_blocks(A, []), gamma=0.0, normalize=False, tol=0, max_iter=12, kern=Double())
    assert rot.iterations == 12 and not rot.converged and len(rot.criterion) == 13 and rot.gamma == 0.0
    ref = vr.orthomax(A, gamma=0.0, normalize=False, tol=0, max_iter=12)
    assert np.abs(rot.R - ref["R"]).max() < 1e-9


@pytest.mark.parametrize("normalize", [False, True])
def test_netcdf_round_trip(tmp_path, normalize):
    from dmd_era5_amd.rotation import Rotation, orthomax_blocks

    A = vr.structured(np.random.default_rng(3008), 200, 3)[0]
    kern = Double()
    rot = orthomax_blocks(_blocks(A, [77]), normalize=normalize, kern=kern)
    path = str(tmp_path / "rot.nc")
    rot.to_netcdf(path)
    back = Rotation.from_netcdf(path, rows=[77, 123], device="cpu", kern=kern)
    assert np.array_equal(back.R, rot.R) and np.array_equal(back.variance, rot.variance)
    assert np.array_equal(back.criterion, rot.criterion)
    assert (back.gamma, back.normalized, back.iterations, back.converged) == (rot.gamma, rot.normalized, rot.iterations,
                                                                              rot.converged)
    if normalize:
        assert [tuple(v.shape) for v in back.communality] == [(77,), (123,)]
        assert all(torch.equal(a, b) for a, b in zip(back.communality, rot.communality))
    else:
        assert back.communality is None
    C = np.arange(6.0).reshape(3, 2)
    assert np.array_equal(back.coefficients(C), rot.coefficients(C))


def test_normalised_gram_in_row_slices(monkeypatch):
    """The weighted rows of the normalised Gram are formed GRAM_SLICE rows at a time: slices that cut the blocks
    anywhere give the rotation of one slice per block."""
    import dmd_era5_amd.rotation as rotation

    A = vr.structured(np.random.default_rng(3009), 500, 4)[0]
    whole = rotation.orthomax_blocks(_blocks(A, [210]), s=np.array([4.0, 3.0, 2.0, 1.0]), kern=Double(), tol=1e-10)
    monkeypatch.setattr(rotation, "GRAM_SLICE", 64)
    cut = rotation.orthomax_blocks(_blocks(A, [210]), s=np.array([4.0, 3.0, 2.0, 1.0]), kern=Double(), tol=1e-10)
    assert cut.iterations == whole.iterations and np.abs(cut.R - whole.R).max() < 1e-10


def test_alias_module():
    import dmd_era5.rotation as alias
    import dmd_era5_amd.rotation as rotation

    assert alias.orthomax_blocks is rotation.orthomax_blocks and alias.Rotation is rotation.Rotation
