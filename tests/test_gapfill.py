"""K31 without a GPU: the numpy definitions (tests/gap_ref.py) against values worked out by hand, and the host layer
(dmd_era5_amd/gapfill.py) over the CPU double of the three kernels against the plain fp64 DINEOF of gap_ref."""
import numpy as np
import pytest
import torch

import gap_ref as gr


class CountingComm:
    """A one-rank communicator that records what it is asked to reduce."""

    world_size, rank, exchanges = 1, 0, False

    def __init__(self):
        self.calls = []

    def allreduce_sum_(self, t, tag="allreduce"):
        self.calls.append((tag, int(t.numel()), t.dtype))
        return t

    def allgather(self, t, tag="allgather"):
        return [t]

    def broadcast_(self, *tensors, tag="broadcast"):
        return tensors if len(tensors) != 1 else tensors[0]


def _blocks(X, cuts):
    edges = [0, *cuts, X.shape[0]]
    return [torch.from_numpy(np.ascontiguousarray(X[a:b].T)) for a, b in zip(edges[:-1], edges[1:])]


def _field(blocks):
    return torch.cat(blocks, dim=1).numpy().T


@pytest.fixture(scope="module")
def synth():
    truth, X = gr.synthetic(0)
    return truth, X, gr.dineof64(X, 8, cv_fraction=0.03, seed=0)


def test_reference_definitions_by_hand():
    X = np.zeros((2, 35), dtype=np.float32)
    X[0, :] = np.arange(35)
    X[0, [0, 31, 33]] = [np.nan, np.inf, -np.inf]
    X[1, 34] = np.float32(np.nan)
    X[1, 3] = np.finfo(np.float32).max
    X[1, 4] = np.float32(1e-45)                            # a denormal is finite
    W, nmiss, sums = gr.mask(X)
    assert W.dtype == np.uint32 and W.shape == (2, 2)
    assert W[0, 0] == (1 | 1 << 31) and W[1, 0] == 2 and W[0, 1] == 0 and W[1, 1] == 4
    assert nmiss.tolist() == [3, 1]
    assert sums[0, 0] == sum(range(35)) - 31 - 33 and sums[1, 0] == sum(t * t for t in range(35)) - 31 ** 2 - 33 ** 2
    assert np.array_equal(gr.unpack_bits(W, 35), gr.gap_bits(X))
    assert np.array_equal(gr.pack_bits(gr.gap_bits(X)), W)
    mu, sg = np.array([1, 0], dtype=np.float32), np.array([2, 1], dtype=np.float32)
    Z = gr.standardize(X, W, mu, sg)
    assert Z[0, 0] == 0 and not np.signbit(Z[0, 0]) and Z[0, 5] == 2 and Z[0, 31] == 0 and Z[1, 34] == 0
    assert np.array_equal(gr.standardize_back(Z, mu, sg)[0, 1:31], X[0, 1:31])
    new, old = np.array([[3, 5, 1]], dtype=np.float32), np.array([[1, 5, 4]], dtype=np.float32)
    assert gr.change64(new, old, np.array([[True, True, False]])).tolist() == [4.0]
    assert gr.change_bound(np.array([4.0]))[0] == 19 * 4.0 * 2.0 ** -24
    # the module's updates of these words, as the CV set goes in and out: two bits of one word, bit 31, a set neighbour
    from dmd_era5_amd.gapfill import _bits_at, _flip_bits_

    Wt = torch.from_numpy(W.view(np.int32).copy())
    rows, ts = torch.tensor([0, 0, 1, 1, 0]), torch.tensor([1, 30, 31, 2, 34])
    assert _bits_at(Wt, rows, ts).tolist() == [0] * 5 and _bits_at(Wt, rows[:2], ts[:2] + 1).tolist() == [0, 1]
    _flip_bits_(Wt, rows, ts, True)
    bits = gr.gap_bits(X)
    bits[rows.numpy(), ts.numpy()] = True
    assert np.array_equal(Wt.numpy().view(np.uint32), gr.pack_bits(bits)) and _bits_at(Wt, rows, ts).tolist() == [1] * 5
    _flip_bits_(Wt, rows, ts, False)
    _flip_bits_(Wt, rows[:0], ts[:0], True)
    assert np.array_equal(Wt.numpy().view(np.uint32), W)


def test_cv_set_is_disjoint_from_the_gaps_and_reproducible():
    from dmd_era5_amd.gapfill import dineof_blocks, draw_cv

    _, X = gr.synthetic(1)
    G = gr.gap_bits(X)
    a = draw_cv(np.random.default_rng(5), 300, 96, 500, lambda f: ~G.reshape(-1)[f])
    b = draw_cv(np.random.default_rng(5), 300, 96, 500, lambda f: ~G.reshape(-1)[f])
    c = draw_cv(np.random.default_rng(6), 300, 96, 500, lambda f: ~G.reshape(-1)[f])
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert len(np.unique(a)) == 500 and not G.reshape(-1)[a].any()
    assert np.array_equal(a, gr.draw_cv(np.random.default_rng(5), 300, 96, 500, ~G))     # the reference draws the same
    with pytest.raises(ValueError, match="too few present"):
        draw_cv(np.random.default_rng(0), 4, 4, 3, lambda f: f == 0)
    # through the module: the masks of a run with CV points differ from the gaps nowhere after the final pass, and the
    # observed values come back (here: to the rounding of standardize there and back)
    fits = [dineof_blocks(_blocks(X, [130]), 3, cv_fraction=0.02, seed=s, max_iter=3, kern=gr.GapKernelDouble())
            for s in (4, 4, 5)]
    assert np.array_equal(fits[0].cv_error, fits[1].cv_error, equal_nan=True)
    assert not np.array_equal(fits[0].cv_error, fits[2].cv_error, equal_nan=True)
    Wcat = np.concatenate([w.numpy().view(np.uint32) for w in fits[0].masks], axis=1)
    bits = gr.unpack_bits(Wcat, 96)
    rowm = np.concatenate([r.numpy() for r in fits[0].row_mask])
    assert np.array_equal(bits[~rowm], G[~rowm]) and bits[rowm].all()
    assert fits[0].n_cv == max(30, int(0.02 * (~G[~rowm]).sum())) and fits[0].n_missing == G[~rowm].sum()


def test_masked_rows_and_exact_round_trip_of_the_observed_values():
    """Integer data with a power-of-two spread per row: standardize there and back is exact, so every observed element
    comes back bit for bit; a row with one present value (min_valid = 2) and a constant row under scale are masked."""
    from dmd_era5_amd.gapfill import dineof_blocks

    rng = np.random.default_rng(11)
    m, T = 40, 64
    # rows of +-2^e around an integer mean: mean = c exactly (as many + as -), std = 2^e exactly
    e = rng.integers(0, 4, m)
    sign = np.stack([rng.permutation(np.repeat([1.0, -1.0], T // 2)) for _ in range(m)])
    c = rng.integers(-50, 50, m).astype(np.float64)
    X = (c[:, None] + sign * 2.0 ** e[:, None]).astype(np.float32)
    X[9, :], c[9] = 5.0, 5.0                               # a constant row
    X0 = X.copy()
    # gaps in balanced pairs (one +, one -), so that mean and std stay exact
    for i in range(m):
        p, q = np.nonzero(sign[i] > 0)[0], np.nonzero(sign[i] < 0)[0]
        X[i, p[:3]] = np.nan
        X[i, q[:3]] = np.nan
    X[7, 1:] = np.nan                                      # one present value
    for scale in (False, True):
        blocks = _blocks(X, [13])
        fit = dineof_blocks(blocks, 2, cv_fraction=0.0, min_cv=10, scale=scale, max_iter=5, kern=gr.GapKernelDouble())
        F = _field(blocks)
        rowm = np.concatenate([r.numpy() for r in fit.row_mask])
        assert rowm.tolist() == [i == 7 or (scale and i == 9) for i in range(m)]
        assert np.isnan(F[rowm]).all() and np.isfinite(F[~rowm]).all()
        seen = ~np.isnan(X) & ~rowm[:, None]
        assert np.array_equal(F[seen].view(np.uint32), X0[seen].view(np.uint32))
        mean = np.concatenate([v.numpy() for v in fit.mean])
        std = np.concatenate([v.numpy() for v in fit.std])
        keep = ~rowm & (np.arange(m) != 9)
        assert np.array_equal(mean[keep], c[keep].astype(np.float32)) and (mean[rowm] == 0).all() and (std[rowm] == 1).all()
        assert np.array_equal(std[keep], (2.0 ** e[keep]).astype(np.float32) if scale else np.ones(keep.sum(), np.float32))
        assert fit.scaled == scale and fit.scale0 == pytest.approx(1.0 if scale else np.sqrt(
            ((X0 - c[:, None]) ** 2)[seen].sum() / seen.sum()), rel=1e-12)


def test_warm_start_and_patience(synth):
    from dmd_era5_amd.gapfill import dineof_blocks

    _, X, ref = synth
    kern = gr.GapKernelDouble()
    # warm start: every rank continues from the fill of the rank before it.  The iteration counts of the warm-started
    # reference are reproduced exactly, and a rank-4 fill of the same field that starts from zeros at the gaps needs
    # more iterations than the final pass, which starts from the last fill
    fit = dineof_blocks(_blocks(X, [130]), 8, cv_fraction=0.03, seed=0, kern=kern)
    assert fit.iterations.tolist() == ref["iterations"].tolist()
    Zc = gr.standardize(X, gr.pack_bits(gr.gap_bits(X)), ref["mean"], None).astype(np.float64)
    G = gr.gap_bits(X)
    G[ref["row_mask"]] = True
    n_cold = 0
    for n_cold in range(1, 500):
        u, s, vh = np.linalg.svd(Zc, full_matrices=False)
        R = (u[:, :4] * s[:4]) @ vh[:4]
        ch = np.sqrt(((R - Zc)[G] ** 2).sum() / ref["n_missing"])
        Zc[G] = R[G]
        if ch <= 1e-4 * ref["scale0"]:
            break
    assert n_cold > fit.iterations[0]
    # patience: the errors rise after rank 4, so rank 4 + patience is the last one tried
    for patience in (1, 2, 3):
        f = dineof_blocks(_blocks(X, [130]), 8, cv_fraction=0.03, seed=0, patience=patience, kern=kern)
        assert f.rank == 4 and len(f.cv_error) == 1 + min(8, 4 + patience), (patience, f.cv_error)
        assert np.nanargmin(f.cv_error) == 4
    f = dineof_blocks(_blocks(X, [130]), 3, cv_fraction=0.03, seed=0, kern=kern)
    assert f.rank == 3 and len(f.cv_error) == 4            # max_rank ends the search first


def test_module_reproduces_the_fp64_reference(synth):
    """Same chosen rank, cv_error equal to what fp32 factors allow: U and C go to the fill rounded to fp32 (relative
    2^-24 each on values of order 1, against cv errors of 0.05 and more), everything else is fp64 on both sides."""
    from dmd_era5_amd.gapfill import dineof_blocks

    truth, X, ref = synth
    comm = CountingComm()
    blocks = _blocks(X, [77, 200])
    fit = dineof_blocks(blocks, 8, cv_fraction=0.03, seed=0, kern=gr.GapKernelDouble(), comm=comm)
    print("cv_error module", fit.cv_error, "reference", ref["cv_error"])
    assert fit.rank == ref["rank"] == 4 and fit.converged and ref["converged"]
    assert fit.iterations.tolist() == ref["iterations"].tolist()
    assert np.allclose(fit.cv_error[1:], ref["cv_error"][1:], rtol=1e-5, atol=0)
    assert (fit.n_missing, fit.n_cv) == (ref["n_missing"], ref["n_cv"])
    assert fit.scale0 == pytest.approx(ref["scale0"], rel=1e-12) and fit.expected_error == fit.cv_error[4]
    F = _field(blocks).astype(np.float64)
    rowm = np.concatenate([r.numpy() for r in fit.row_mask])
    assert rowm.tolist() == ref["row_mask"].tolist() == [i == 17 for i in range(300)]
    assert np.isnan(F[17]).all() and np.isfinite(F[~rowm]).all() and np.isfinite(F[~rowm, 55]).all()
    assert np.abs(F[~rowm] - ref["filled"][~rowm]).max() < 2e-4          # fp32 storage of values near 290: 3e-5 an ulp
    seen = ~gr.gap_bits(X)
    assert np.abs(F[seen] - X[seen]).max() <= 2.0 ** -15                  # one rounding there, one back, at < 512
    assert np.allclose(fit.svd.s.numpy(), ref["s"], rtol=1e-5)
    # one packed all-reduce at the start and one per iteration: two doubles
    assert comm.calls[0] == ("dineof_setup_allreduce", 4, torch.float64)
    per_iter = [c for c in comm.calls if c[0] == "dineof_allreduce"]
    assert len(per_iter) == int(fit.iterations.sum()) and all(c[1:] == (2, torch.float64) for c in per_iter)


def test_netcdf_round_trip_and_alias(tmp_path):
    import dmd_era5.gapfill as alias
    import dmd_era5_amd.gapfill as gapfill

    assert alias.dineof_blocks is gapfill.dineof_blocks and alias.GapFill is gapfill.GapFill
    _, X = gr.synthetic(2, m=90, T=40)
    kern = gr.GapKernelDouble()
    fit = gapfill.dineof_blocks(_blocks(X, [33]), 3, max_iter=4, kern=kern)
    path = str(tmp_path / "fill.nc")
    fit.to_netcdf(path)
    back = gapfill.GapFill.from_netcdf(path, rows=[33, 57], device="cpu", kern=kern)
    assert (back.rank, back.converged, back.n_missing, back.n_cv, back.scale0, back.tol, back.scaled) == (
        fit.rank, fit.converged, fit.n_missing, fit.n_cv, fit.scale0, fit.tol, fit.scaled)
    assert np.array_equal(back.cv_error, fit.cv_error, equal_nan=True) and np.array_equal(back.iterations, fit.iterations)
    assert back.expected_error == fit.expected_error and back.masks is None
    for name in ("mean", "std", "row_mask"):
        assert [tuple(v.shape) for v in getattr(back, name)] == [(33,), (57,)]
        assert all(torch.equal(a, b) for a, b in zip(getattr(back, name), getattr(fit, name)))
    assert torch.equal(back.svd.s, fit.svd.s) and torch.equal(back.svd.Vh, fit.svd.Vh) and torch.equal(back.svd.Ut, fit.svd.Ut)


def test_refusals():
    from dmd_era5_amd.gapfill import dineof_blocks

    _, X = gr.synthetic(3, m=60, T=40)
    kern = gr.GapKernelDouble()
    for kw in (dict(max_rank=0), dict(max_rank=41), dict(max_rank=2, max_iter=0), dict(max_rank=2, patience=0),
               dict(max_rank=2, cv_fraction=0.6), dict(max_rank=2, svd="lanczos")):
        with pytest.raises(ValueError):
            dineof_blocks(_blocks(X, [20]), kern=kern, **kw)
    with pytest.raises(ValueError):
        dineof_blocks([], 2, kern=kern)
    with pytest.raises(ValueError):
        dineof_blocks([torch.zeros((40, 5)), torch.zeros((39, 5))], 2, kern=kern)
    with pytest.raises(ValueError, match="no row"):
        dineof_blocks([torch.full((40, 5), float("nan"))], 2, kern=kern)
