"""K31 on the GPU through the ctypes table: dmdx_gap_mask_f32 and dmdx_gap_standardize_f32 against the numpy definitions
of tests/gap_ref.py, bit for bit; every operand lives in a guarded allocation (tests/memguard.py)."""
import itertools

import numpy as np
import pytest
import torch

import gap_ref as gr
import memguard as mg

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
MS = [1, 3, 4, 255, 257, 1025]
TS = [1, 31, 32, 33, 1023, 1025, 2100]


@pytest.fixture(scope="module")
def L():
    from dmd_era5_amd.kernels import default_kernels

    return default_kernels()._lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _x_guard(m, T, layout):
    """layout 0: a 16-byte aligned base with ldx % 4 == 0 (the 16-byte loads), 1: an odd base, 2: ldx % 4 != 0"""
    ldx = {0: (m + 3) // 4 * 4 + 4, 1: m + 4, 2: (m + 3) // 4 * 4 + 1}[layout]
    return mg.Guarded(m, T, ldx, F32, {0: 0, 1: 1 + m % 3, 2: 0}[layout], DEV)


def _special_field(rng, m, T):
    """Normal values with NaN of several payloads, +-Inf, denormals, -0 and +-FLT_MAX planted in a fifth of the places."""
    X = rng.standard_normal((m, T)).astype(np.float32)
    bits = X.view(np.uint32)
    special = np.array([0x7FC00000, 0x7FC0DEAD, 0xFFC00001, 0x7F800001, 0xFF812345, 0x7F800000, 0xFF800000,   # gaps
                        0x00000001, 0x807FFFFF, 0x80000000, 0x00000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000], dtype=np.uint32)
    where = rng.random((m, T)) < 0.2
    bits[where] = special[rng.integers(0, len(special), int(where.sum()))]
    return X


def _mask_call(L, gX, m, T, gW, gN, gS, ws):
    rc = L.dmdx_gap_mask_f32(gX.ptr, m, T, gX.ld, gW.ptr, gW.ld, None if gN is None else gN.ptr,
                             None if gS is None else gS.ptr, 0 if gS is None else gS.ld, None if ws is None else ws.ptr,
                             0 if ws is None else ws.nbytes, _stream())
    torch.cuda.synchronize()
    return rc


def test_mask_counts_and_sums_are_the_reference_bit_for_bit_in_both_launch_forms(L):
    rng = np.random.default_rng(3101)
    assert L.dmdx_gap_mask_segment() == gr.SEGMENT
    for (im, m), (it, T) in itertools.product(enumerate(MS), enumerate(TS)):
        layout = (im + it) % 3
        X = _special_field(rng, m, T)
        W, nmiss, sums = gr.mask(X)
        nw = -(-T // 32)
        got = []
        for split in (True, False):
            gX = _x_guard(m, T, layout).fill(X)
            gX.iview.copy_(torch.from_numpy(np.ascontiguousarray(X.T).view(np.int32)).to(DEV))   # (the payloads as they are)
            gX.snapshot()
            gW = mg.Guarded(m, nw, m + (layout > 0) * 3, F32, layout, DEV)
            gN = mg.Guarded(m, 1, m, F32, 0, DEV)
            gS = mg.Guarded(m, 2, m + (layout > 0) * 5, F64, 0, DEV)
            ws = mg.exact_workspace(L.dmdx_gap_mask_workspace_bytes(m, T), DEV) if split else None
            assert _mask_call(L, gX, m, T, gW, gN, gS, ws) == 0, L.dmdx_last_error()
            for g, name in ((gW, "W"), (gN, "nmiss"), (gS, "sums")):
                g.check_untouched(name)
            gW.check_fully_written("W")
            gX.check_untouched("X")
            gX.check_unchanged("X")
            if ws is not None:
                ws.check_untouched()
            w = gW.iview.cpu().numpy().view(np.uint32)
            n = gN.iview.cpu().numpy().reshape(-1)
            s = gS.view.cpu().numpy()
            assert np.array_equal(w, W), (m, T, layout, split)
            assert np.array_equal(n, nmiss), (m, T, layout, split)
            assert np.array_equal(s.view(np.uint64), sums.view(np.uint64)), (m, T, layout, split)
            if T % 32:
                assert (w[-1] >> np.uint32(T % 32) == 0).all()                 # the bits past T are zero
            got.append((w, n, s))
        for a, b in zip(*got):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (m, T, layout)


def test_mask_without_the_optional_outputs(L):
    rng = np.random.default_rng(3102)
    m, T = 257, 1100
    X = _special_field(rng, m, T)
    W, nmiss, sums = gr.mask(X)
    for want_n, want_s, split in ((False, False, True), (True, False, False), (False, True, True), (False, False, False)):
        gX = _x_guard(m, T, 0).fill(X)
        gX.iview.copy_(torch.from_numpy(np.ascontiguousarray(X.T).view(np.int32)).to(DEV))
        gW = mg.Guarded(m, -(-T // 32), m, F32, 0, DEV)
        gN = mg.Guarded(m, 1, m, F32, 0, DEV) if want_n else None
        gS = mg.Guarded(m, 2, m, F64, 0, DEV) if want_s else None
        ws = mg.exact_workspace(L.dmdx_gap_mask_workspace_bytes(m, T), DEV) if split else None
        assert _mask_call(L, gX, m, T, gW, gN, gS, ws) == 0, L.dmdx_last_error()
        assert np.array_equal(gW.iview.cpu().numpy().view(np.uint32), W)
        if want_n:
            assert np.array_equal(gN.iview.cpu().numpy().reshape(-1), nmiss)
        if want_s:
            assert np.array_equal(gS.view.cpu().numpy().view(np.uint64), sums.view(np.uint64))
        if ws is not None:
            ws.check_untouched()


def _same_class_or_bits(got, want, what):
    """Finite and infinite results bit for bit; a NaN where the reference has a NaN (K13's contract: the class)."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


def test_standardize_forward_and_back_are_the_reference_bit_for_bit(L):
    rng = np.random.default_rng(3103)
    for (im, m), (it, T) in itertools.product(enumerate(MS), enumerate([1, 31, 32, 33, 100])):
        layout = (im + it) % 3
        X = (280.0 + 10.0 * rng.standard_normal((m, T))).astype(np.float32)
        X[rng.random((m, T)) < 0.2] = np.nan
        X[m // 2, :] = 7.0                                  # with sigma = 0 below: 0 / 0 and x / 0
        X[m // 2, T // 2] = 9.0
        mu = (280.0 + rng.standard_normal(m)).astype(np.float32)
        sigma = (0.5 + rng.random(m)).astype(np.float32)
        mu[m // 2], sigma[m // 2] = 7.0, 0.0
        W = gr.pack_bits(gr.gap_bits(X))
        for use_w, use_mu, use_sigma in ((True, True, True), (True, True, False), (True, False, True), (False, True, True)):
            X1 = X if use_w else np.where(np.isnan(X), np.float32(1.5), X)
            gX = _x_guard(m, T, layout).fill(X1)
            gW = mg.Guarded(m, W.shape[0], m + (layout > 0) * 3, F32, 0, DEV)
            gW.iview.copy_(torch.from_numpy(W.view(np.int32)).to(DEV))
            gW.snapshot()
            gmu = mg.Guarded(m, 1, m, F32, layout, DEV).fill(mu).snapshot()
            gsg = mg.Guarded(m, 1, m, F32, 0, DEV).fill(sigma).snapshot()
            args = (gW.ptr if use_w else None, gW.ld, gmu.ptr if use_mu else None, gsg.ptr if use_sigma else None)
            assert L.dmdx_gap_standardize_f32(gX.ptr, m, T, gX.ld, *args, 0, _stream()) == 0, L.dmdx_last_error()
            torch.cuda.synchronize()
            Z = gX.logical()
            want = gr.standardize(X1, W if use_w else None, mu if use_mu else None, sigma if use_sigma else None)
            _same_class_or_bits(Z, want, (m, T, layout, use_w, use_mu, use_sigma))
            if use_w:
                assert (Z.view(np.uint32)[np.isnan(X)] == 0).all()               # +0.0 at the gaps, whatever was there
            # back: W is ignored, every element moves (the non-finite ones of the sigma = 0 row are left out of the input)
            Zf = np.where(np.isfinite(Z), Z, np.float32(2.0))
            gX.fill(Zf)
            assert L.dmdx_gap_standardize_f32(gX.ptr, m, T, gX.ld, *args, 1, _stream()) == 0, L.dmdx_last_error()
            torch.cuda.synchronize()
            back = gr.standardize_back(Zf, mu if use_mu else None, sigma if use_sigma else None)
            assert np.array_equal(gX.logical().view(np.uint32), back.view(np.uint32)), (m, T, layout)
            for g, name in ((gX, "X"), (gW, "W"), (gmu, "mu"), (gsg, "sigma")):
                g.check_untouched(name)
            for g in (gW, gmu, gsg):
                g.check_unchanged("input")


def test_wrappers_give_the_same_words(L):
    """HipKernels.gap_mask / gap_standardize_ on plain tensors: shapes, dtypes and the two launch forms."""
    from dmd_era5_amd.kernels import default_kernels

    kern = default_kernels()
    rng = np.random.default_rng(3104)
    m, T = 515, 2100
    X = _special_field(rng, m, T)
    W, nmiss, sums = gr.mask(X)
    Xt = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV)
    for split in (True, False):
        Wd, nd, sd = kern.gap_mask(Xt, split=split)
        assert Wd.shape == (66, m) and Wd.dtype == torch.int32 and nd.dtype == torch.int32 and sd.shape == (2, m)
        assert np.array_equal(Wd.cpu().numpy().view(np.uint32), W) and np.array_equal(nd.cpu().numpy(), nmiss)
        assert np.array_equal(sd.cpu().numpy().view(np.uint64), sums.view(np.uint64))
    assert kern.gap_mask(Xt, want_sums=False)[2] is None
    mu = torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(DEV)
    sg = torch.from_numpy((0.5 + rng.random(m)).astype(np.float32)).to(DEV)
    fin = np.where(gr.gap_bits(X), np.float32(0), np.clip(X, -100, 100))          # (no overflow of x - mu)
    Xt = torch.from_numpy(np.ascontiguousarray(np.where(gr.gap_bits(X), X, fin).T)).to(DEV)
    kern.gap_standardize_(Xt, Wd, mu, sg)
    want = gr.standardize(np.where(gr.gap_bits(X), X, fin), W, mu.cpu().numpy(), sg.cpu().numpy())
    assert np.array_equal(Xt.cpu().numpy().T.view(np.uint32), want.view(np.uint32))
    kern.gap_standardize_(Xt, None, mu, sg, back=True)
    assert np.array_equal(Xt.cpu().numpy().T.view(np.uint32),
                          gr.standardize_back(want, mu.cpu().numpy(), sg.cpu().numpy()).view(np.uint32))
