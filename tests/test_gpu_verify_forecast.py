"""DmdForecast.verify on the HIP provider (K16) against the CPU kernel double and the direct numpy evaluation of
tests/test_verify.py: two row blocks, groups that end off the 128-row boundary of the kernel's workgroups, a
delay embedding, a masked row whose X holds the NaN K14 makes of a fill value, and the per-row scores."""
import numpy as np
import pytest
import torch

import verify_ref as vr
from test_ensemble import _members
from test_verify import DoubleWithVerify, KEYS, _t, compare, reference

pytestmark = pytest.mark.gpu

DELAY, K, T = 2, 7, 21
ROWS = (300, 211)
LABELS = ([0] * 150 + [1] * 150, [1] * 61 + [2] * 150)          # runs of 150, 150 | 61, 150 rows
MASKED = ((7, 128, 299), (60,))


def _problem():
    from dmd_era5_amd.bopdmd import OptDMDResult

    rs = np.random.RandomState(163)
    members = _members(4, K, seed=8)
    base = members[0]
    result = OptDMDResult(eigs=base.eigs, modes=base.modes, amplitudes=base.amplitudes, rel_error=0.0, n_iter=0,
                          converged=True, trials=members)
    blocks = []
    for mb, lab, masked in zip(ROWS, LABELS, MASKED):
        w = (0.05 + rs.rand(mb)).astype(np.float32)
        w[list(masked)] = 0.0
        mu = (3.0 * rs.standard_normal(mb)).astype(np.float32)
        X = (mu + 2.0 * rs.standard_normal((T + DELAY - 1, mb))).astype(np.float32)
        X[:, list(masked)] = np.nan
        blocks.append(dict(U=(rs.standard_normal((K, DELAY * mb)) / np.sqrt(K)).astype(np.float32), X=X, mu=mu,
                           sd=(0.5 + rs.rand(mb)).astype(np.float32), w=w,
                           clim=(mu + 0.5 * rs.standard_normal(mb)).astype(np.float32), lab=np.asarray(lab, dtype=np.int64)))
    return result, blocks


def _forecast(result, blocks, device, kern):
    from dmd_era5_amd.forecast import DmdForecast

    dev = (lambda key: [_t(B[key]).to(device) for B in blocks])
    return DmdForecast(dev("U"), result, dev("mu"), dev("sd"), delay=DELAY, kern=kern)


@pytest.mark.parametrize("ensemble", [False, True])
def test_forecast_verify_on_the_device_equals_the_cpu_double(ensemble):
    result, blocks = _problem()
    t = torch.from_numpy(np.linspace(0.0, 3.0, T))
    kw = dict(weights=[_t(B["w"]) for B in blocks], clims=[_t(B["clim"]) for B in blocks],
              groups=[torch.from_numpy(B["lab"]) for B in blocks], want_rows=True, ensemble=ensemble)
    gpu = _forecast(result, blocks, "cuda", None)
    got = gpu.verify([_t(B["X"]).cuda() for B in blocks], t, **kw)
    torch.cuda.synchronize()
    cpu = _forecast(result, blocks, "cpu", DoubleWithVerify())
    want = cpu.verify([_t(B["X"]) for B in blocks], t, **kw)
    assert got["imag_ratio"] == want["imag_ratio"]
    host = {key: ([x.cpu() for x in v] if isinstance(v, list) else v.cpu() if isinstance(v, torch.Tensor) else v)
            for key, v in got.items()}
    C = (gpu.ensemble_coefficients(t)[0] if ensemble else gpu.coefficients(t)[0]).cpu().numpy()
    ref = reference(C, blocks, DELAY, 3)
    compare(host, ref)          # the device result within the kernel's bounds of the fp64 evaluation, scores included
    compare(want, ref)
    assert torch.equal(host["rows"], want["rows"]) and torch.equal(host["masked_rows"], want["masked_rows"])
    assert int(host["masked_rows"].sum()) == 4 * DELAY and torch.equal(host["weight"], want["weight"])
    for key in KEYS:
        sb = np.stack([vr.score_bounds(col, bound, W)[key] for col, bound, W, _, _ in ref])
        assert (np.abs(host[key].numpy() - want[key].numpy()) <= sb + 1e-13).all(), key
    for key in ("row_rmse", "row_bias", "row_acc"):
        for B, g, w_ in zip(blocks, host[key], want[key]):
            fin = np.tile(B["w"], DELAY) != 0
            assert g.shape == w_.shape == (DELAY * B["X"].shape[1],)
            assert np.isnan(g.numpy()[~fin]).all() and np.isfinite(g.numpy()[fin]).all()
            assert np.allclose(g.numpy()[fin], w_.numpy()[fin], rtol=1e-4, atol=1e-5), key
