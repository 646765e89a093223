"""Python face of the C ABI (include/dmdx.h): torch tensors in, torch tensors out.

Layout convention used everywhere in this package
-------------------------------------------------
The C ABI is column-major ``(ptr, rows, cols, ld)``.  A column-major matrix
``M`` (rows x cols) is held on the device as the torch tensor ``Mt`` of shape
``(cols, rows)`` with strides ``(ld, 1)`` -- i.e. the row-major transpose, so
``Mt[j, i] == M[i, j]``.  The snapshot matrix X (space x time) is therefore a
``(time, space)`` tensor: one snapshot per row, exactly the order an ERA5
NetCDF slice is stored in.  The delay-embedded matrix (reference
slice_tools.py:207-211) is the overlapping view
``Xt.as_strided((n-d+1, d*m), (m, 1))`` -- zero copy.

PyTorch is plumbing here (device memory, streams); the arithmetic is in
libdmdx.so.  There is no CPU fallback: every method raises if the library or
the GPU is missing.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _check_mat(t: torch.Tensor, dtype, name: str) -> tuple[int, int, int]:
    """-> (rows, cols, ld) of the column-major matrix a (cols, rows) tensor holds."""
    if not t.is_cuda:
        raise _lib.DmdxError(f"{name}: expected a device tensor (no CPU fallback exists)")
    if t.dtype != dtype or t.dim() != 2:
        raise _lib.DmdxError(f"{name}: expected 2-D {dtype}, got {t.dtype} {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise _lib.DmdxError(f"{name}: inner stride must be 1, got {t.stride()}")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
    return t.shape[1], t.shape[0], ld


def _check_vec(v: torch.Tensor | None, m: int, device, who: str, name: str) -> None:
    """An optional per-row vector: None, or (m,) contiguous fp32 on `device`."""
    if v is not None and (v.dtype != torch.float32 or v.shape != (m,) or v.device != device or not v.is_contiguous()):
        raise _lib.DmdxError(f"{who}: {name} must be a contiguous fp32 vector of length {m} on {device}")


def _check_ivec(v, device, who: str, name: str, n: int | None = None) -> int:
    """A device int32 vector (contiguous; ``n`` entries if given) -> its length."""
    if (not isinstance(v, torch.Tensor) or v.dtype != torch.int32 or v.dim() != 1 or v.device != device
            or not v.is_contiguous() or (n is not None and v.numel() != n)):
        raise _lib.DmdxError(f"{who}: {name} must be a contiguous int32 vector"
                             f"{'' if n is None else f' of length {n}'} on {device}")
    return int(v.numel())


def _check_field(t: torch.Tensor, m: int, T: int, dtype, device, who: str, name: str, kind: str = "") -> int:
    """A (T, m) field on `device` (inner stride 1, any row stride) -> its leading dimension.  ``kind``: what the
    message adds to the shape (" int16")."""
    mt, Tt, ld = _check_mat(t, dtype, f"{who} {name}")
    if (mt, Tt) != (m, T) or t.device != device:
        raise _lib.DmdxError(f"{who}: {name} must be ({T}, {m}){kind} on {device}, got {tuple(t.shape)}")
    return ld


def _check_snapshots(Xt: torch.Tensor, m: int, T: int, device, who: str) -> int:
    """The snapshots a kernel reads: (T, m) fp32 on `device` (any row stride) -> ldx."""
    return _check_field(Xt, m, T, torch.float32, device, who, "X")


def _out_view(out: torch.Tensor | None, m: int, T: int, dtype, device, who: str, kind: str = ""):
    """The (T, m) field a kernel writes: ``out`` (as :func:`_check_field`) or a fresh tensor -> (tensor, ld)."""
    if out is None:
        return torch.empty((T, m), dtype=dtype, device=device), m
    return out, _check_field(out, m, T, dtype, device, who, "out", kind)


_DTYPE_NAME = {torch.float64: "fp64", torch.float32: "fp32", torch.int64: "int64", torch.int32: "int32"}
DMDX_SPELL_NQ = 7                        # the planes of K27 (include/dmdx.h)
DMDX_PSTAT_NQ = 8                        # the planes of K29
PSTAT_INNER = ("sum", "mean", "max", "min", "range")      # DMDX_PSTAT_SUM .. DMDX_PSTAT_RANGE


def _accumulator(out: torch.Tensor | None, shape: tuple, dtype, device, who: str, name: str = "out") -> torch.Tensor:
    """The sums a kernel writes or adds to: ``out``, contiguous with this shape and dtype on `device`, or a fresh
    (uninitialised) tensor."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.shape != shape or out.dtype != dtype or not out.is_contiguous() or out.device != device:
        raise _lib.DmdxError(f"{who}: {name} must be a contiguous {shape} {_DTYPE_NAME[dtype]} tensor on {device}")
    return out


def _check_bounds(bounds, T: int, who: str) -> list[int]:
    """The P + 1 positions of the periods of a (T, m) block, as integers."""
    b = [int(v) for v in np.asarray(bounds).reshape(-1)]
    # here and not only in C: the int32 array of a launch would wrap what does not fit it
    if len(b) < 2 or b[0] < 0 or b[-1] > T or any(y <= x for x, y in zip(b, b[1:])):
        raise _lib.DmdxError(f"{who}: bounds must be at least 2 strictly ascending integers in 0 .. T = {T}")
    return b


def _check_threshold_table(thr, slot, m: int, T: int, device, max_thr: int, who: str, check_labels: bool):
    """-> (thr3, J, S): ``thr`` as the contiguous (J, S, m) fp32 table of K24 and K27, J <= ``max_thr``; ``slot`` the
    (T,) int32 labels on ``device``, or None for S = 1.  ``check_labels``: a device read, the labels must lie in
    0 .. S - 1."""
    if (not isinstance(thr, torch.Tensor) or thr.dtype != torch.float32 or thr.dim() not in (2, 3)
            or thr.device != device or thr.shape[-1] != m or not thr.is_contiguous()):
        raise _lib.DmdxError(f"{who}: thr must be a contiguous (J, S, {m}) or (J, {m}) fp32 tensor on {device}")
    thr3 = thr if thr.dim() == 3 else thr.unsqueeze(1)
    J, S = int(thr3.shape[0]), int(thr3.shape[1])
    if not 1 <= J <= max_thr or S < 1:
        raise _lib.DmdxError(f"{who}: {J} thresholds in {S} slots; 1 .. {max_thr} thresholds and at least one slot "
                             f"asked for")
    if slot is None:
        if S != 1:
            raise _lib.DmdxError(f"{who}: thr has {S} slots, so slot must name one per snapshot")
    else:
        _check_ivec(slot, device, who, "slot", T)
        if check_labels:
            lo, hi = int(slot.min()), int(slot.max())
            if lo < 0 or hi >= S:
                raise _lib.DmdxError(f"{who}: slot labels {lo} .. {hi} outside 0 .. {S - 1}")
    return thr3, J, S


class HipKernels:
    """The product kernel provider (libdmdx.so on the current CUDA/HIP device)."""

    name = "hip"

    def __init__(self, lib=None):
        # lib: another build of the library with its signatures set (the A/B builds of the measurement scripts);
        # workspaces and events are per object, nothing is shared with the default provider
        self._lib = _lib.load() if lib is None else lib
        if not torch.cuda.is_available():
            raise _lib.DmdxError("no HIP device visible: the dmdx kernels have no CPU fallback")
        self._ws: dict[int, torch.Tensor] = {}
        self._planes: dict[int, torch.Tensor] = {}   # K1's bf16 planes (_plane_groups), cached like the workspaces
        # when set to a list, every launch is bracketed by HIP events on the launch
        # stream and (name, shape, start, stop) is appended (bench.py reads these)
        self.events: list | None = None

    # -- plumbing ---------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream().cuda_stream

    def _timed(self, name: str, shape: tuple, fn):
        if self.events is None:
            return fn()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        self.events.append((name, shape, e0, e1))
        return rc

    def _ws_key(self, device: torch.device) -> tuple:
        # one scratch buffer per (device, stream): launches on different streams may overlap
        idx = device.index if device.index is not None else torch.cuda.current_device()
        return (idx, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)

    def _workspace(self, device: torch.device, nbytes: int) -> torch.Tensor:
        key = self._ws_key(device)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            self._ws[key] = ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        return ws

    def _per_period(self, name: str, entry: str, planes: torch.Tensor, paxis: int, b: list, maxp: int, mid: tuple,
                    pieces_of, workspace_bytes, call) -> torch.Tensor:
        """A per-period kernel (K27, K29) over the periods ``b`` in launches of at most ``maxp``, their bounds by value:
        fills ``planes`` (periods along ``paxis``, rows last) and returns it.  ``pieces_of(length)``: the pieces of one
        period; time is split, and ``workspace_bytes(host_b, n)`` asked for, only where a launch has more than one.
        ``call(host_b, n, part, ws, nbytes)``: the C call ``entry`` for n periods into ``part``."""
        P, m = len(b) - 1, int(planes.shape[-1])
        for p0 in range(0, P, maxp):
            n = min(maxp, P - p0)
            cut = b[p0:p0 + n + 1]
            part = planes if n == P else torch.empty(planes.shape[:paxis] + (n,) + planes.shape[paxis + 1:],
                                                     dtype=planes.dtype, device=planes.device)
            host_b = (ctypes.c_int32 * (n + 1))(*cut)
            split = sum(pieces_of(y - x) for x, y in zip(cut, cut[1:])) > 1
            nbytes = int(workspace_bytes(host_b, n)) if split else 0
            ws = self._workspace(planes.device, nbytes) if split else None
            rc = self._timed(name, (m, cut[-1] - cut[0], *mid, n), lambda: call(host_b, n, part, ws, nbytes))
            _lib.check(rc, entry)
            if part is not planes:
                planes.narrow(paxis, p0, n).copy_(part)
        return planes

    def release_workspace(self) -> int:
        """Drop the cached partial-tile workspaces and K1's bf16 planes (K1 / K3: 128 KB per (row block, K-split, tile)
        of a launch -- 5.1 GB for cfg2's Gram, 9.5 GB for a cfg3 shard; they are kept between calls
        because re-allocating them costs more than the eigen stage).  Callers that are about to
        fill the HBM with something else (main() before a larger slice, the 227 GB cfg4 matrix)
        call this first.  Returns the number of bytes released."""
        n = sum(int(w.numel()) for w in self._ws.values()) + sum(int(w.numel()) for w in self._planes.values())
        self._ws.clear()
        self._planes.clear()
        return n

    # -- K1 -----------------------------------------------------------------
    # HBM left free next to the plane buffer of a Gram call (the allocator's slack and whatever the caller allocates
    # between the Gram and the next release_workspace()); the buffer also never takes more than half of what is free
    PLANE_RESERVE_BYTES = 16 << 30

    def _plane_groups(self, dev: torch.device, ms: list, n: int):
        """The memory policy of K1's bf16 planes (6 bytes per value of X, made once per call, cached like the
        workspaces): the groups [(a, b), ...] of whole row blocks that each run as one dmdx_syrk_blocks_planes_f32 call --
        one group where the planes of the whole call fit half of what torch.cuda.mem_get_info reports free and leave
        PLANE_RESERVE_BYTES of it (a cached buffer counts as free), else as few groups as fit, summed with ``accumulate`` --
        or None for the entry without planes: a Gram of n <= 96 columns (the library runs those without planes), not one
        block fits, or DMDX_K1_PLANES=0 (A/B knob, results unchanged)."""
        if n <= 96 or os.environ.get("DMDX_K1_PLANES") == "0":
            return None

        # (the library's count of one block; a call's planes are the sum over its blocks)
        per_block = [int(self._lib.dmdx_syrk_planes_bytes((ctypes.c_int64 * 1)(m), 1, n)) for m in ms]
        have = self._planes.get(self._ws_key(dev))
        have = int(have.numel()) if have is not None else 0
        free = int(torch.cuda.mem_get_info(dev)[0]) + have
        room = max(have, min(free - self.PLANE_RESERVE_BYTES, free // 2))
        groups, a, held = [], 0, 0
        for b, nbytes in enumerate(per_block):
            if nbytes <= 0 or nbytes > room:
                return None
            if held + nbytes > room:
                groups.append((a, b))
                a, held = b, 0
            held += nbytes
        groups.append((a, len(ms)))
        return groups

    def _plane_buffer(self, dev: torch.device, nbytes: int) -> torch.Tensor:
        key = self._ws_key(dev)
        buf = self._planes.get(key)
        if buf is None or buf.numel() < nbytes:
            # The smaller buffer goes back to the DEVICE before the larger one is asked for, not into torch's cache:
            # _plane_groups has counted it as free, and a block of this size that stays reserved next to its
            # successor (55 GB next to 102 GB, cfg2 then a cfg3 shard) is of no use to any later allocation.
            # Side effects, only on a call whose planes outgrow the cached buffer: empty_cache() hands EVERY unused
            # cached block of the process back, so the allocations that follow pay the device allocator once more, and
            # the call itself -- inside its event pair when events are recorded -- pays the release and the new buffer.
            if self._planes.pop(key, None) is not None:
                buf = None
                torch.cuda.empty_cache()
            self._planes[key] = buf = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        return buf

    def _gram(self, dev, ptr_list, ms, ld_list, n, G64, G32, accumulate: bool, without_planes):
        """G64 (+)= sum_j X_j^T X_j [, G32] through dmdx_syrk_blocks_planes_f32 in the groups of _plane_groups;
        ``without_planes()``: the call of the entry that takes none, where the policy says so.  -> (rc, entry)."""
        groups = self._plane_groups(dev, ms, n) if max(ld_list) < (1 << 24) else None
        if groups is None:
            return without_planes()
        L = self._lib
        calls = []
        for a, b in groups:
            nb = b - a
            m_arr = (ctypes.c_int64 * nb)(*ms[a:b])
            calls.append((nb, (ctypes.c_void_p * nb)(*ptr_list[a:b]), m_arr, (ctypes.c_int64 * nb)(*ld_list[a:b]),
                          int(L.dmdx_syrk_blocks_workspace_bytes(m_arr, nb, n)), int(L.dmdx_syrk_planes_bytes(m_arr, nb, n))))
        ws = self._workspace(dev, max(c[4] for c in calls))
        planes = self._plane_buffer(dev, max(c[5] for c in calls))
        rc = 0
        for i, (nb, p_arr, m_arr, ld_arr, _, _) in enumerate(calls):
            rc = L.dmdx_syrk_blocks_planes_f32(p_arr, m_arr, ld_arr, nb, n, _ptr(G64), n, _ptr(G32), n,
                                               int(accumulate or i > 0), _ptr(ws), ws.numel(), _ptr(planes),
                                               planes.numel(), self._stream())
            if rc:
                break
        return rc, "dmdx_syrk_blocks_planes_f32"

    def syrk(self, Xt: torch.Tensor, want32: bool = False, out: torch.Tensor | None = None):
        """G = X^T X (fp64, both triangles).  Xt: (n, m) fp32.  -> G64 [, G32].

        ``out``: an (n, n) fp64 tensor to accumulate into (G64 = out += X^T X): the
        Gram of a row-blocked snapshot matrix is the sum over its blocks.  A batch of one block through the
        entry of ``syrk_blocks`` (same arithmetic as dmdx_syrk_f32, which still takes what that entry does not)."""
        m, n, ld = _check_mat(Xt, torch.float32, "syrk X")
        if out is not None:
            if out.shape != (n, n) or out.dtype != torch.float64 or not out.is_contiguous():
                raise _lib.DmdxError("syrk: out must be a contiguous (n, n) fp64 tensor")
            G64 = out
        else:
            G64 = torch.empty((n, n), dtype=torch.float64, device=Xt.device)
        G32 = torch.empty((n, n), dtype=torch.float32, device=Xt.device) if want32 else None

        def without_planes():
            ws = self._workspace(Xt.device, self._lib.dmdx_syrk_workspace_bytes(m, n))
            return self._lib.dmdx_syrk_f32(_ptr(Xt), m, n, ld, _ptr(G64), n, _ptr(G32), n, int(out is not None), _ptr(ws),
                                           ws.numel(), self._stream()), "dmdx_syrk_f32"

        rc, entry = self._timed("syrk", (m, n), lambda: self._gram(
            Xt.device, [Xt.data_ptr()], [m], [ld], n, G64, G32, out is not None, without_planes))
        _lib.check(rc, entry)
        return (G64, G32) if want32 else G64

    def syrk_blocks(self, blocks, out: torch.Tensor | None = None) -> torch.Tensor:
        """G (+)= sum_j X_j^T X_j over a list of (n, m_j) fp32 row blocks, 16 blocks per launch."""
        import ctypes as C

        shapes = [_check_mat(B, torch.float32, "syrk_blocks X") for B in blocks]
        n = shapes[0][1]
        if any(s[1] != n for s in shapes):
            raise _lib.DmdxError("syrk_blocks: the blocks must have the same number of columns")
        dev = blocks[0].device
        if out is not None:
            if out.shape != (n, n) or out.dtype != torch.float64 or not out.is_contiguous():
                raise _lib.DmdxError("syrk_blocks: out must be a contiguous (n, n) fp64 tensor")
            G64 = out
        else:
            G64 = torch.empty((n, n), dtype=torch.float64, device=dev)
        nb = len(blocks)

        def without_planes():
            ptrs = (C.c_void_p * nb)(*[B.data_ptr() for B in blocks])
            ms = (C.c_int64 * nb)(*[s[0] for s in shapes])
            lds = (C.c_int64 * nb)(*[s[2] for s in shapes])
            ws = self._workspace(dev, self._lib.dmdx_syrk_blocks_workspace_bytes(ms, nb, n))
            return self._lib.dmdx_syrk_blocks_f32(ptrs, ms, lds, nb, n, _ptr(G64), n, None, 0, int(out is not None),
                                                  _ptr(ws), ws.numel(), self._stream()), "dmdx_syrk_blocks_f32"

        # (the pre-split of the planes is part of the call: inside the event pair)
        rc, entry = self._timed("syrk_blocks", (sum(s[0] for s in shapes), n, nb), lambda: self._gram(
            dev, [B.data_ptr() for B in blocks], [s[0] for s in shapes], [s[2] for s in shapes], n, G64, None,
            out is not None, without_planes))
        _lib.check(rc, entry)
        return G64

    # -- K3 -----------------------------------------------------------------
    def gemm_tn(self, At: torch.Tensor, Bt: torch.Tensor, want32: bool = False,
                out: torch.Tensor | None = None):
        """C = A^T B for K-contiguous A (K x na), B (K x nb).

        At: (na, K), Bt: (nb, K) fp32.  Returns Ct of shape (nb, na) (the
        column-major na x nb C), fp64 [and fp32]."""
        Ka, na, lda = _check_mat(At, torch.float32, "gemm_tn A")
        Kb, nb, ldb = _check_mat(Bt, torch.float32, "gemm_tn B")
        if Ka != Kb:
            raise _lib.DmdxError(f"gemm_tn: K mismatch {Ka} vs {Kb}")
        if out is not None:
            if out.shape != (nb, na) or out.dtype != torch.float64 or not out.is_contiguous():
                raise _lib.DmdxError("gemm_tn: out must be a contiguous (nb, na) fp64 tensor")
            C64 = out
        else:
            C64 = torch.empty((nb, na), dtype=torch.float64, device=At.device)
        C32 = torch.empty((nb, na), dtype=torch.float32, device=At.device) if want32 else None
        nbytes = self._lib.dmdx_gemm_tn_workspace_bytes(Ka, na, nb)
        ws = self._workspace(At.device, nbytes)
        rc = self._timed("gemm_tn", (Ka, na, nb), lambda: self._lib.dmdx_gemm_tn_f32(
            _ptr(At), lda, _ptr(Bt), ldb, Ka, na, nb, _ptr(C64), na, _ptr(C32), na,
            int(out is not None), _ptr(ws), ws.numel(), self._stream(),
        ))
        _lib.check(rc, "dmdx_gemm_tn_f32")
        return (C64, C32) if want32 else C64

    def gemm_tn_blocks(self, Ablocks, Bblocks, out: torch.Tensor | None = None) -> torch.Tensor:
        """C (+)= sum_j A_j^T B_j over lists of K-contiguous row blocks (At_j: (na, K_j), Bt_j:
        (nb, K_j) fp32), 16 blocks per launch.  Returns Ct (nb, na) fp64."""
        import ctypes as C

        if len(Ablocks) != len(Bblocks) or not Ablocks:
            raise _lib.DmdxError("gemm_tn_blocks: two equally long, non-empty lists of blocks")
        sa = [_check_mat(A, torch.float32, "gemm_tn_blocks A") for A in Ablocks]
        sb = [_check_mat(B, torch.float32, "gemm_tn_blocks B") for B in Bblocks]
        na, nb_ = sa[0][1], sb[0][1]
        if any(x[1] != na for x in sa) or any(x[1] != nb_ for x in sb) or any(x[0] != y[0] for x, y in zip(sa, sb)):
            raise _lib.DmdxError("gemm_tn_blocks: inconsistent block shapes")
        dev = Ablocks[0].device
        if out is not None:
            if out.shape != (nb_, na) or out.dtype != torch.float64 or not out.is_contiguous():
                raise _lib.DmdxError("gemm_tn_blocks: out must be a contiguous (nb, na) fp64 tensor")
            C64 = out
        else:
            C64 = torch.empty((nb_, na), dtype=torch.float64, device=dev)
        n = len(Ablocks)
        pa = (C.c_void_p * n)(*[A.data_ptr() for A in Ablocks])
        pb = (C.c_void_p * n)(*[B.data_ptr() for B in Bblocks])
        la = (C.c_int64 * n)(*[x[2] for x in sa])
        lb = (C.c_int64 * n)(*[x[2] for x in sb])
        ks = (C.c_int64 * n)(*[x[0] for x in sa])
        ws = self._workspace(dev, self._lib.dmdx_gemm_tn_blocks_workspace_bytes(ks, n, na, nb_))
        rc = self._timed("gemm_tn_blocks", (sum(x[0] for x in sa), na, nb_, n), lambda: self._lib.dmdx_gemm_tn_blocks_f32(
            pa, la, pb, lb, ks, n, na, nb_, _ptr(C64), na, None, 0, int(out is not None), _ptr(ws), ws.numel(),
            self._stream()
        ))
        _lib.check(rc, "dmdx_gemm_tn_blocks_f32")
        return C64

    # -- K2 -----------------------------------------------------------------
    @staticmethod
    def pitch(Wt: torch.Tensor) -> torch.Tensor:
        """A view of the small operand W (l, n) whose rows start on 16-byte boundaries (a padded
        copy unless it already is one).  K2's 16-byte load path needs that of X, Y *and* W; W is
        small and X is not, so W is re-pitched rather than X sent down the scalar-load path
        (n = 3653, cfg4: 1.6 -> 2.9 TB/s of X).  Callers that loop over row blocks do it once."""
        l, n = Wt.shape
        if l <= 1 or not (Wt.stride(0) % 4 or Wt.data_ptr() % 16 or Wt.stride(1) != 1):
            return Wt
        Wp = torch.zeros((l, (n + 3) // 4 * 4), dtype=Wt.dtype, device=Wt.device)
        Wp[:, :n] = Wt
        return Wp[:, :n]

    @property
    def skinny_gram_max_l(self) -> int:
        return int(self._lib.dmdx_gemm_nn_skinny_gram_max_l())

    def skinny(self, Xt: torch.Tensor, Wt: torch.Tensor, out: torch.Tensor | None = None,
               gram: torch.Tensor | None = None) -> torch.Tensor:
        """Y = X W.  Xt: (n, m), Wt: (l, n) fp32 -> Yt: (l, m) fp32.

        ``out``: an (l, m) fp32 view to write into (inner stride 1, any row stride >= m) -- a
        column slice of the (l, M) result of all row blocks, so that no concatenation follows.
        ``gram``: an (l, l) fp64 tensor (l <= skinny_gram_max_l) that Y^T Y is ADDED to, formed from
        the accumulators inside the same launch (the Gram of the CholeskyQR round that follows)."""
        m, n, ldx = _check_mat(Xt, torch.float32, "skinny X")
        nw, l, ldw = _check_mat(Wt, torch.float32, "skinny W")
        if nw != n:
            raise _lib.DmdxError(f"skinny: W has {nw} rows, X has {n} columns")
        Wt = self.pitch(Wt)
        ldw = _check_mat(Wt, torch.float32, "skinny W")[2]
        if out is not None:
            mo, lo, ldy = _check_mat(out, torch.float32, "skinny out")
            if (mo, lo) != (m, l) or out.device != Xt.device:
                raise _lib.DmdxError(f"skinny: out must be ({l}, {m}) on {Xt.device}, got {tuple(out.shape)}")
            Yt = out
        else:
            Yt, ldy = torch.empty((l, m), dtype=torch.float32, device=Xt.device), m
        if gram is not None:
            if gram.shape != (l, l) or gram.dtype != torch.float64 or not gram.is_contiguous() or gram.device != Xt.device \
                    or l > self.skinny_gram_max_l:
                raise _lib.DmdxError(f"skinny: gram must be a contiguous ({l}, {l}) fp64 tensor on {Xt.device}, "
                                     f"l <= {self.skinny_gram_max_l}")
            ws = self._workspace(Xt.device, self._lib.dmdx_gemm_nn_skinny_gram_workspace_bytes(m, l))
            rc = self._timed("skinny_gram", (m, n, l), lambda: self._lib.dmdx_gemm_nn_skinny_gram_f32(
                _ptr(Xt), m, n, ldx, _ptr(Wt), ldw, l, _ptr(Yt), ldy, _ptr(gram), l, 1, _ptr(ws), ws.numel(),
                self._stream()
            ))
            _lib.check(rc, "dmdx_gemm_nn_skinny_gram_f32")
            return Yt
        rc = self._timed("skinny", (m, n, l), lambda: self._lib.dmdx_gemm_nn_skinny_f32(
            _ptr(Xt), m, n, ldx, _ptr(Wt), ldw, l, _ptr(Yt), ldy, self._stream()
        ))
        _lib.check(rc, "dmdx_gemm_nn_skinny_f32")
        return Yt

    # -- K12 ----------------------------------------------------------------
    @property
    def expand_max_k(self) -> int:
        return int(self._lib.dmdx_expand_max_k())

    def _expand_args(self, Ut, Ct, mean, std, who):
        m, k, ldu = _check_mat(Ut, torch.float32, f"{who} U")
        kc, T, _ = _check_mat(Ct, torch.float32, f"{who} C")
        if kc != k:
            raise _lib.DmdxError(f"{who}: C has {kc} rows, U has {k} columns")
        Ct = self.pitch(Ct)
        ldc = _check_mat(Ct, torch.float32, f"{who} C")[2]
        for v, name in ((mean, "mean"), (std, "std")):
            _check_vec(v, m, Ut.device, who, name)
        return m, k, ldu, T, Ct, ldc

    def expand(self, Ut: torch.Tensor, Ct: torch.Tensor, mean: torch.Tensor | None = None,
               std: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """Xhat = mean + std * (U C).  Ut: (k, m), Ct: (T, k) fp32, mean / std: (m,) fp32 or None
        -> Xt: (T, m) fp32, the layout of a snapshot block.

        ``out``: a (T, m) fp32 view to write into (inner stride 1, any row stride >= m)."""
        m, k, ldu, T, Ct, ldc = self._expand_args(Ut, Ct, mean, std, "expand")
        Xt, ldxh = _out_view(out, m, T, torch.float32, Ut.device, "expand")
        rc = self._timed("expand", (m, k, T), lambda: self._lib.dmdx_expand_f32(
            _ptr(Ut), m, k, ldu, _ptr(Ct), ldc, T, _ptr(mean), _ptr(std), _ptr(Xt), ldxh, self._stream()
        ))
        _lib.check(rc, "dmdx_expand_f32")
        return Xt

    def expand_score(self, Ut: torch.Tensor, Ct: torch.Tensor, Xt: torch.Tensor, mean: torch.Tensor | None = None,
                     std: torch.Tensor | None = None, out: torch.Tensor | None = None, want_rows: bool = False):
        """Squared error of Xhat = mean + std * (U C) against X, Xhat never stored.  Ut: (k, m),
        Ct: (T, k), Xt: (T, m) fp32 (the delay view included) -> (cols, rows): ``cols`` a (2, T) fp64
        tensor, row 0 = sum_i (X - Xhat)^2, row 1 = sum_i (X - mean)^2 per snapshot; ``rows`` the (m,)
        fp64 sum_t (X - Xhat)^2 per space point, or None.

        ``out``: a contiguous (2, T) fp64 tensor the column sums are ADDED to (row blocks of X)."""
        m, k, ldu, T, Ct, ldc = self._expand_args(Ut, Ct, mean, std, "expand_score")
        ldx = _check_snapshots(Xt, m, T, Ut.device, "expand_score")
        cols = _accumulator(out, (2, T), torch.float64, Ut.device, "expand_score")
        rows = torch.empty(m, dtype=torch.float64, device=Ut.device) if want_rows else None
        ws = self._workspace(Ut.device, self._lib.dmdx_expand_score_workspace_bytes(m, k, T))
        rc = self._timed("expand_score", (m, k, T), lambda: self._lib.dmdx_expand_score_f32(
            _ptr(Ut), m, k, ldu, _ptr(Ct), ldc, T, _ptr(mean), _ptr(std), _ptr(Xt), ldx, cols[0].data_ptr(),
            cols[1].data_ptr(), _ptr(rows), int(out is not None), _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_expand_score_f32")
        return cols, rows

    # -- K16 ----------------------------------------------------------------
    @property
    def verify_max_k(self) -> int:
        return int(self._lib.dmdx_verify_max_k())

    def verify(self, Ut: torch.Tensor, Ct: torch.Tensor, Xt: torch.Tensor, mean: torch.Tensor | None = None,
               std: torch.Tensor | None = None, weight: torch.Tensor | None = None, clim: torch.Tensor | None = None,
               out: torch.Tensor | None = None, want_rows: bool = False):
        """The six weighted sums behind RMSE, bias and ACC of Xhat = mean + std * (U C) against X and a
        climatology, Xhat never stored.  Ut: (k, m), Ct: (T, k), Xt: (T, m) fp32 (the delay view included),
        mean / std / weight / clim: (m,) fp32 or None (0 / 1 / 1 / mean) -> (cols, rows): ``cols`` a (6, T) fp64
        tensor of sum_i w (e^2, e, a, f^2, a^2, f a) with e = Xhat - X, f = Xhat - clim, a = X - clim over the
        rows with w != 0 (a row with weight 0 is left out whatever it holds); ``rows`` the (6, m) fp64 sums of
        the same quantities over t, unweighted, or None.

        ``out``: a contiguous (6, T) fp64 tensor the column sums are ADDED to (row blocks, groups of rows)."""
        m, k, ldu, T, Ct, ldc = self._expand_args(Ut, Ct, mean, std, "verify")
        ldx = _check_snapshots(Xt, m, T, Ut.device, "verify")
        for v, name in ((weight, "weight"), (clim, "clim")):
            _check_vec(v, m, Ut.device, "verify", name)
        cols = _accumulator(out, (6, T), torch.float64, Ut.device, "verify")
        rows = torch.empty((6, m), dtype=torch.float64, device=Ut.device) if want_rows else None
        ws = self._workspace(Ut.device, self._lib.dmdx_verify_workspace_bytes(m, k, T))
        rc = self._timed("verify", (m, k, T), lambda: self._lib.dmdx_verify_f32(
            _ptr(Ut), m, k, ldu, _ptr(Ct), ldc, T, _ptr(mean), _ptr(std), _ptr(Xt), ldx, _ptr(weight), _ptr(clim),
            _ptr(cols), T, _ptr(rows), m, int(out is not None), _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_verify_f32")
        return cols, rows

    # -- K15 ----------------------------------------------------------------
    @property
    def spread_max_k(self) -> int:
        return int(self._lib.dmdx_spread_max_k())

    def _spread_args(self, Ut, Dev, std, who):
        m, k, ldu = _check_mat(Ut, torch.float32, f"{who} U")
        if not Dev.is_cuda or Dev.dtype != torch.float32 or Dev.dim() != 3 or Dev.device != Ut.device:
            raise _lib.DmdxError(f"{who}: Dev must be a 3-D (B, T, k) fp32 tensor on {Ut.device}, got {Dev.dtype} "
                                 f"{tuple(Dev.shape)} on {Dev.device}")
        B, T, kd = Dev.shape
        if kd != k or B < 1 or T < 1:
            raise _lib.DmdxError(f"{who}: Dev is {tuple(Dev.shape)}, U has {k} columns; (B >= 1, T >= 1, {k}) asked for")
        # the (B T, ldd) row-major image of the k x (B T) column-major D, rows on 16-byte boundaries
        # (a Dev that already is such an image -- forecast._pitched_dev -- is taken as it is)
        if (k == 1 or Dev.stride(2) == 1) and Dev.stride(1) >= k and Dev.stride(0) == T * Dev.stride(1):
            Dt = Dev.as_strided((B * T, k), (Dev.stride(1), 1))
        else:
            Dt = Dev.reshape(B * T, k)
        Dt = self.pitch(Dt)
        ldd = _check_mat(Dt, torch.float32, f"{who} Dev")[2]
        _check_vec(std, m, Ut.device, who, "std")
        return m, k, ldu, int(T), int(B), Dt, ldd

    def spread(self, Ut: torch.Tensor, Dev: torch.Tensor, std: torch.Tensor | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
        """S = |std| * sqrt(sum_b (U d_b)^2): the spread of B member fields whose scaled deviations from the
        ensemble mean are ``Dev``.  Ut: (k, m), Dev: (B, T, k) fp32, std: (m,) fp32 or None -> St: (T, m)
        fp32.  No member field is stored.

        ``out``: a (T, m) fp32 view to write into (inner stride 1, any row stride >= m)."""
        m, k, ldu, T, B, Dt, ldd = self._spread_args(Ut, Dev, std, "spread")
        St, lds = _out_view(out, m, T, torch.float32, Ut.device, "spread")
        rc = self._timed("spread", (m, k, T, B), lambda: self._lib.dmdx_spread_f32(
            _ptr(Ut), m, k, ldu, _ptr(Dt), ldd, T, B, _ptr(std), _ptr(St), lds, self._stream()
        ))
        _lib.check(rc, "dmdx_spread_f32")
        return St

    def spread_score(self, Ut: torch.Tensor, Dev: torch.Tensor, std: torch.Tensor | None = None,
                     out: torch.Tensor | None = None, want_rows: bool = False):
        """The sums of the squared spread, S never stored.  Ut: (k, m), Dev: (B, T, k) fp32 -> (var, rows):
        ``var`` the (T,) fp64 sum_i S[i, t]^2 per snapshot, ``rows`` the (m,) fp64 sum_t S[i, t]^2 per space
        point, or None.

        ``out``: a contiguous (T,) fp64 tensor the snapshot sums are ADDED to (row blocks of U)."""
        m, k, ldu, T, B, Dt, ldd = self._spread_args(Ut, Dev, std, "spread_score")
        var = _accumulator(out, (T,), torch.float64, Ut.device, "spread_score")
        rows = torch.empty(m, dtype=torch.float64, device=Ut.device) if want_rows else None
        ws = self._workspace(Ut.device, self._lib.dmdx_spread_score_workspace_bytes(m, k, T, B))
        rc = self._timed("spread_score", (m, k, T, B), lambda: self._lib.dmdx_spread_score_f32(
            _ptr(Ut), m, k, ldu, _ptr(Dt), ldd, T, B, _ptr(std), _ptr(var), _ptr(rows), int(out is not None),
            _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_spread_score_f32")
        return var, rows

    # -- K19 ----------------------------------------------------------------
    @property
    def crps_max_k(self) -> int:
        return int(self._lib.dmdx_crps_max_k())

    @property
    def crps_max_members(self) -> int:
        return int(self._lib.dmdx_crps_max_members())

    def crps(self, Ut: torch.Tensor, Cm: torch.Tensor, Xt: torch.Tensor, mean: torch.Tensor | None = None,
             std: torch.Tensor | None = None, weight: torch.Tensor | None = None, out: torch.Tensor | None = None,
             hist: torch.Tensor | None = None, want_rows: bool = False):
        """The sums behind the CRPS and the rank counts of the B member fields x_b = mean + std * (U c_b) against
        X, no member field stored.  Ut: (k, m), Cm: (B, T, k) fp32 (the members' coefficients, pitched like
        ``forecast._pitched_dev`` or not), Xt: (T, m) fp32 (the delay view included), mean / std / weight: (m,)
        fp32 or None (0 / 1 / 1) -> (cols, rows, hist): ``cols`` a (2, T) fp64 tensor of sum_i w sum_b |x_b - x|
        and sum_i w sum_{b < b'} |x_b - x_b'| over the rows with w != 0; ``rows`` the (2, m) fp64 sums of the same
        two quantities over t, unweighted, or None; ``hist`` the (B + 1,) int64 counts of the rank
        #{b : x_b < x} over the selected, finite elements.

        ``out`` / ``hist``: a contiguous (2, T) fp64 and a contiguous (B + 1,) int64 tensor the sums and the counts
        are ADDED to (row blocks, groups of rows); both or neither."""
        m, k, ldu, T, B, Dt, ldc = self._spread_args(Ut, Cm, std, "crps")
        if B > self.crps_max_members:
            raise _lib.DmdxError(f"crps: {B} members, at most {self.crps_max_members}")
        ldx = _check_snapshots(Xt, m, T, Ut.device, "crps")
        for v, name in ((mean, "mean"), (weight, "weight")):
            _check_vec(v, m, Ut.device, "crps", name)
        if (out is None) != (hist is None):
            raise _lib.DmdxError("crps: out and hist are accumulated into together: pass both or neither")
        cols = _accumulator(out, (2, T), torch.float64, Ut.device, "crps")
        counts = _accumulator(hist, (B + 1,), torch.int64, Ut.device, "crps", "hist")
        rows = torch.empty((2, m), dtype=torch.float64, device=Ut.device) if want_rows else None
        ws = self._workspace(Ut.device, self._lib.dmdx_crps_workspace_bytes(m, k, T, B))
        rc = self._timed("crps", (m, k, T, B), lambda: self._lib.dmdx_crps_f32(
            _ptr(Ut), m, k, ldu, _ptr(Dt), ldc, T, B, _ptr(mean), _ptr(std), _ptr(Xt), ldx, _ptr(weight),
            _ptr(cols), T, _ptr(rows), m, _ptr(counts), int(out is not None), _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_crps_f32")
        return cols, rows, counts

    # -- K24 ----------------------------------------------------------------
    @property
    def exceed_max_k(self) -> int:
        return int(self._lib.dmdx_exceed_max_k())

    @property
    def exceed_max_members(self) -> int:
        return int(self._lib.dmdx_exceed_max_members())

    @property
    def exceed_max_thresholds(self) -> int:
        return int(self._lib.dmdx_exceed_max_thresholds())

    def _exceed_args(self, Ut, Cm, thr, slot, mean, std, who):
        """-> (m, k, ldu, T, B, Dt, ldc, thr3, J, S): the members as :meth:`crps` takes them, ``thr`` as the
        contiguous (J, S, m) table, ``slot`` checked against it (a device read: the labels must lie in 0 .. S - 1)."""
        m, k, ldu, T, B, Dt, ldc = self._spread_args(Ut, Cm, std, who)
        if B > self.exceed_max_members:
            raise _lib.DmdxError(f"{who}: {B} members, at most {self.exceed_max_members}")
        _check_vec(mean, m, Ut.device, who, "mean")
        thr3, J, S = _check_threshold_table(thr, slot, m, T, Ut.device, self.exceed_max_thresholds, who, True)
        return m, k, ldu, T, B, Dt, ldc, thr3, J, S

    def exceed_prob(self, Ut: torch.Tensor, Cm: torch.Tensor, thr: torch.Tensor, slot: torch.Tensor | None = None,
                    above: bool = True, mean: torch.Tensor | None = None, std: torch.Tensor | None = None,
                    out: torch.Tensor | None = None) -> torch.Tensor:
        """The share of the B member fields x_b = mean + std * (U c_b) beyond a threshold, no member field stored.
        Ut: (k, m), Cm: (B, T, k) fp32 (as :meth:`crps`), thr: (J, S, m) or (J, m) fp32, threshold j of every row for
        slot s, J <= ``exceed_max_thresholds``; slot: (T,) device int32 labels in 0 .. S - 1, or None (S = 1);
        ``above``: the event is x > thr, otherwise x < thr (strict: a tie is no event, a NaN threshold gives none)
        -> P (J, T, m) fp32: the fp32 nearest to c / B with c the number of members in the event, NaN where a member
        is not finite.

        ``out``: a contiguous (J, T, m) fp32 tensor to write into."""
        m, k, ldu, T, B, Dt, ldc, thr3, J, S = self._exceed_args(Ut, Cm, thr, slot, mean, std, "exceed_prob")
        if out is not None and (out.shape != (J, T, m) or out.dtype != torch.float32 or not out.is_contiguous()
                                or out.device != Ut.device):
            raise _lib.DmdxError(f"exceed_prob: out must be a contiguous ({J}, {T}, {m}) fp32 tensor on {Ut.device}")
        P = torch.empty((J, T, m), dtype=torch.float32, device=Ut.device) if out is None else out
        rc = self._timed("exceed_prob", (m, k, T, B, J), lambda: self._lib.dmdx_exceed_prob_f32(
            _ptr(Ut), m, k, ldu, _ptr(Dt), ldc, T, B, _ptr(mean), _ptr(std), _ptr(thr3), m, J, S, _ptr(slot),
            int(bool(above)), _ptr(P), m, T * m, self._stream()
        ))
        _lib.check(rc, "dmdx_exceed_prob_f32")
        return P

    def exceed_score(self, Ut: torch.Tensor, Cm: torch.Tensor, Xt: torch.Tensor, thr: torch.Tensor,
                     slot: torch.Tensor | None = None, above: bool = True, mean: torch.Tensor | None = None,
                     std: torch.Tensor | None = None, weight: torch.Tensor | None = None,
                     out: torch.Tensor | None = None, counts: torch.Tensor | None = None, want_rows: bool = False):
        """The sums behind the Brier score and the counts behind the reliability diagram and the ROC curve of the
        exceedance probability p of :meth:`exceed_prob` against X, nothing stored.  Operands as :meth:`exceed_prob`,
        Xt: (T, m) fp32 (the delay view included), weight: (m,) fp32 or None (1).  With o = 1 where X is in the event
        and 0 otherwise -> (cols, rows, counts): ``cols`` a (J, 4, T) fp64 tensor of sum_i w ((p - o)^2, o, p, p^2)
        over the rows with w != 0 (a row with weight 0 is left out whatever it holds); ``rows`` the (J, 4, m) fp64
        sums of the same quantities over t, unweighted, or None; ``counts`` the (J, 2, B + 1) int64 numbers of
        selected, finite elements with outcome o and c members in the event.  An element with a non-finite member
        or X makes its sums NaN and enters no count.

        ``out`` / ``counts``: a contiguous (J, 4, T) fp64 and a contiguous (J, 2, B + 1) int64 tensor the sums and
        the counts are ADDED to (row blocks, groups of rows); both or neither."""
        m, k, ldu, T, B, Dt, ldc, thr3, J, S = self._exceed_args(Ut, Cm, thr, slot, mean, std, "exceed_score")
        ldx = _check_snapshots(Xt, m, T, Ut.device, "exceed_score")
        _check_vec(weight, m, Ut.device, "exceed_score", "weight")
        if (out is None) != (counts is None):
            raise _lib.DmdxError("exceed_score: out and counts are accumulated into together: pass both or neither")
        cols = _accumulator(out, (J, 4, T), torch.float64, Ut.device, "exceed_score")
        cnt = _accumulator(counts, (J, 2, B + 1), torch.int64, Ut.device, "exceed_score", "counts")
        rows = torch.empty((J, 4, m), dtype=torch.float64, device=Ut.device) if want_rows else None
        ws = self._workspace(Ut.device, self._lib.dmdx_exceed_score_workspace_bytes(m, k, T, B, J))
        rc = self._timed("exceed_score", (m, k, T, B, J), lambda: self._lib.dmdx_exceed_score_f32(
            _ptr(Ut), m, k, ldu, _ptr(Dt), ldc, T, B, _ptr(mean), _ptr(std), _ptr(thr3), m, J, S, _ptr(slot),
            int(bool(above)), _ptr(Xt), ldx, _ptr(weight), _ptr(cols), T, _ptr(rows), m, _ptr(cnt),
            int(out is not None), _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_exceed_score_f32")
        return cols, rows, cnt

    # -- K13 ----------------------------------------------------------------
    @property
    def project_max_k(self) -> int:
        return int(self._lib.dmdx_project_max_k())

    def project(self, Ut: torch.Tensor, Xt: torch.Tensor, mean: torch.Tensor | None = None,
                std: torch.Tensor | None = None, out=None, want_energy: bool = True):
        """C = U^T ((X - mean) / std) and the energy sum_i ((x - mean) / std)^2 of every snapshot, X read once
        and no standardised copy made.  Ut: (k, m), Xt: (T, m) fp32 (the delay view included), mean / std:
        (m,) fp32 or None -> (Ct (T, k) fp64, energy (T,) fp64 or None).

        ``out``: the pair (Ct, energy) of an earlier call -- contiguous (T, k) / (T,) fp64 -- that this
        block's sums are ADDED to (row blocks of X and U); its energy is None iff ``want_energy`` is false."""
        m, k, ldu = _check_mat(Ut, torch.float32, "project U")
        mx, T, ldx = _check_mat(Xt, torch.float32, "project X")
        if mx != m or Xt.device != Ut.device:
            raise _lib.DmdxError(f"project: X must be (T, {m}) on {Ut.device}, got {tuple(Xt.shape)} on {Xt.device}")
        for v, name in ((mean, "mean"), (std, "std")):
            _check_vec(v, m, Ut.device, "project", name)
        if out is not None:
            Ct, energy = out
            _accumulator(Ct, (T, k), torch.float64, Ut.device, "project", "out[0]")
            if (energy is not None) != bool(want_energy) or (energy is not None and (
                    energy.shape != (T,) or energy.dtype != torch.float64 or not energy.is_contiguous()
                    or energy.device != Ut.device)):
                raise _lib.DmdxError(f"project: out[1] must be a contiguous ({T},) fp64 tensor on {Ut.device} "
                                     "when the energy is wanted, and None otherwise")
        else:
            Ct = torch.empty((T, k), dtype=torch.float64, device=Ut.device)
            energy = torch.empty(T, dtype=torch.float64, device=Ut.device) if want_energy else None
        ws = self._workspace(Ut.device, self._lib.dmdx_project_workspace_bytes(m, k, T))
        rc = self._timed("project", (m, k, T), lambda: self._lib.dmdx_project_f32(
            _ptr(Ut), m, k, ldu, _ptr(Xt), ldx, T, _ptr(mean), _ptr(std), _ptr(Ct), k, _ptr(energy),
            int(out is not None), _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_project_f32")
        return Ct, energy

    # -- K30 ----------------------------------------------------------------
    @property
    def varimax_max_k(self) -> int:
        return int(self._lib.dmdx_varimax_max_k())

    def varimax_step(self, Ut: torch.Tensor, Rt: torch.Tensor, w: torch.Tensor | None = None, out=None,
                     want_f: bool = True):
        """The sums of one orthomax step in one read of U: with ``a = U`` (or ``fl(U w)``, one weight per row) and
        ``L = a R``, ``G = a^T L^3``, ``q = colsum(L^2)``, ``f = colsum(L^4)``; L is never stored.  Ut: (k, m) fp32,
        Rt: (k, k) fp32 holding the column-major R (``Rt[c, j] = R[j, c]``, any row stride), w: (m,) fp32 or None
        -> (Gt (k, k) fp64 with ``Gt[c, j] = G[j, c]``, q (k,) fp64, f (k,) fp64 or None).

        ``out``: the triple (Gt, q, f) of an earlier call -- contiguous fp64 -- that this block's sums are ADDED to
        (row blocks of U); its f is None iff ``want_f`` is false."""
        m, k, ldu = _check_mat(Ut, torch.float32, "varimax_step U")
        kr, kc, ldr = _check_mat(Rt, torch.float32, "varimax_step R")
        if (kr, kc) != (k, k) or Rt.device != Ut.device:
            raise _lib.DmdxError(f"varimax_step: R must be ({k}, {k}) on {Ut.device}, got {tuple(Rt.shape)} on {Rt.device}")
        _check_vec(w, m, Ut.device, "varimax_step", "w")
        if out is not None:
            Gt, q, f = out
            _accumulator(Gt, (k, k), torch.float64, Ut.device, "varimax_step", "out[0]")
            _accumulator(q, (k,), torch.float64, Ut.device, "varimax_step", "out[1]")
            if (f is not None) != bool(want_f):
                raise _lib.DmdxError("varimax_step: out[2] must be given when f is wanted, and None otherwise")
            if f is not None:
                _accumulator(f, (k,), torch.float64, Ut.device, "varimax_step", "out[2]")
        else:
            Gt = torch.empty((k, k), dtype=torch.float64, device=Ut.device)
            q = torch.empty(k, dtype=torch.float64, device=Ut.device)
            f = torch.empty(k, dtype=torch.float64, device=Ut.device) if want_f else None
        ws = self._workspace(Ut.device, self._lib.dmdx_varimax_workspace_bytes(m, k))
        rc = self._timed("varimax_step", (m, k), lambda: self._lib.dmdx_varimax_step_f32(
            _ptr(Ut), m, k, ldu, _ptr(Rt), ldr, _ptr(w), _ptr(Gt), k, _ptr(q), _ptr(f), int(out is not None),
            _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_varimax_step_f32")
        return Gt, q, f

    def row_norms(self, Ut: torch.Tensor, cscale: torch.Tensor | None = None, out: torch.Tensor | None = None):
        """``h[i] = fp32(sqrt(sum_j fp64(fl(U[i, j] cscale[j]))^2))``: the communalities of Kaiser's normalisation, how
        much of a grid point the k modes explain.  Ut: (k, m) fp32 (any row stride), cscale: (k,) fp32 or None
        -> h (m,) fp32 (``out`` if given).  One read of Ut."""
        m, k, ldu = _check_mat(Ut, torch.float32, "row_norms U")
        _check_vec(cscale, k, Ut.device, "row_norms", "cscale")
        h = _accumulator(out, (m,), torch.float32, Ut.device, "row_norms") if out is not None else \
            torch.empty(m, dtype=torch.float32, device=Ut.device)
        rc = self._timed("row_norms", (m, k), lambda: self._lib.dmdx_row_norms_f32(
            _ptr(Ut), m, k, ldu, _ptr(cscale), _ptr(h), self._stream()
        ))
        _lib.check(rc, "dmdx_row_norms_f32")
        return h

    # -- K5 -----------------------------------------------------------------
    def row_center_scale_(self, Xt: torch.Tensor, scale: bool):
        """In place: subtract the per-space-point mean over time (and divide by the
        std, ddof 0).  Xt: (n, m).  -> (mean (m,), std (m,) or None)."""
        m, n, ldx = _check_mat(Xt, torch.float32, "row_center_scale X")
        mean = torch.empty(m, dtype=torch.float32, device=Xt.device)
        std = torch.empty(m, dtype=torch.float32, device=Xt.device) if scale else None
        rc = self._timed("row_center_scale", (m, n), lambda: self._lib.dmdx_row_center_scale_f32(
            _ptr(Xt), m, n, ldx, _ptr(mean), _ptr(std), int(bool(scale)), self._stream()
        ))
        _lib.check(rc, "dmdx_row_center_scale_f32")
        return mean, std

    # -- K14 ----------------------------------------------------------------
    def unpack_i16_(self, codes: torch.Tensor, lds: int, tstep: int, Xt: torch.Tensor, row0: int, plane: int,
                    seg_offset, scale_factor: float, add_offset: float, fills=(),
                    fill_count: torch.Tensor | None = None) -> torch.Tensor:
        """CF-packed int16 codes -> the snapshots ``Xt`` ((T, rows) fp32 view of a row block), in place.
        ``codes``: device int16, the time slab as the file holds it (snapshot stride ``lds`` elements,
        starting at the first snapshot to take); snapshot j of Xt is source snapshot j * tstep; row
        row0 + r of the variable is element seg_offset[(row0 + r) // plane] + (row0 + r) % plane.
        ``fills``: up to two fill codes (-> NaN); ``fill_count``: one device int64 that accumulates."""
        if not codes.is_cuda or codes.dtype != torch.int16 or not codes.is_contiguous():
            raise _lib.DmdxError("unpack_i16: codes must be a contiguous device int16 tensor")
        if fill_count is not None and (not fill_count.is_cuda or fill_count.dtype != torch.int64 or fill_count.numel() != 1):
            raise _lib.DmdxError("unpack_i16: fill_count must be one device int64")
        rows, T, ldx = _check_mat(Xt, torch.float32, "unpack_i16 X")
        segs = [int(o) for o in seg_offset]
        fills = [int(f) for f in fills]
        if not 1 <= len(segs) <= 64 or len(fills) > 2:
            raise _lib.DmdxError(f"unpack_i16: {len(segs)} segments (1..64), {len(fills)} fill codes (0..2)")
        need, plane, row0 = 0, int(plane), int(row0)
        if T and rows and plane >= 1 and row0 >= 0 and row0 + rows <= len(segs) * plane:
            last = row0 + rows - 1                       # the last code a snapshot addresses, per segment touched
            need = (T - 1) * int(tstep) * int(lds) + max(
                segs[s] + (plane if s < last // plane else last % plane + 1) for s in range(row0 // plane, last // plane + 1))
        if codes.numel() < need:
            raise _lib.DmdxError(f"unpack_i16: the call addresses {need} codes, the slab holds {codes.numel()}")
        import ctypes as C

        table = (C.c_int64 * len(segs))(*segs)
        f = fills + [0, 0]
        rc = self._timed("unpack_i16", (rows, T), lambda: self._lib.dmdx_unpack_i16_f32(
            _ptr(codes), int(lds), T, int(tstep), rows, int(row0), int(plane), len(segs), table, float(scale_factor),
            float(add_offset), len(fills), f[0], f[1], _ptr(Xt), ldx, _ptr(fill_count), self._stream()
        ))
        _lib.check(rc, "dmdx_unpack_i16_f32")
        return Xt

    # -- K17 ----------------------------------------------------------------
    @property
    def pack_max_k(self) -> int:
        return int(self._lib.dmdx_pack_max_k())

    @staticmethod
    def _range_out(out, device, who):
        """-> (range (2,) fp32, count (1,) int64, accumulate) of a range call; ``out`` is the pair of an earlier one."""
        if out is None:
            return (torch.empty(2, dtype=torch.float32, device=device), torch.empty(1, dtype=torch.int64, device=device), 0)
        rng, cnt = out
        if (rng.shape != (2,) or rng.dtype != torch.float32 or not rng.is_contiguous() or rng.device != device
                or cnt.shape != (1,) or cnt.dtype != torch.int64 or cnt.device != device):
            raise _lib.DmdxError(f"{who}: out must be the pair ((2,) fp32, (1,) int64) on {device}")
        return rng, cnt, 1

    @staticmethod
    def _pack_out(out, counts, m, T, device, who):
        """-> (Qt (T, m) int16, ldq, counts (2,) int64) of a pack call; a given ``counts`` accumulates."""
        Qt, ldq = _out_view(out, m, T, torch.int16, device, who, " int16")
        if counts is None:
            counts = torch.zeros(2, dtype=torch.int64, device=device)
        return Qt, ldq, _accumulator(counts, (2,), torch.int64, device, who, "counts")

    def expand_range(self, Ut: torch.Tensor, Ct: torch.Tensor, mean: torch.Tensor | None = None,
                     std: torch.Tensor | None = None, out=None):
        """The range of Xhat = mean + std * (U C), Xhat never stored (operands as :meth:`expand`) -> (range, count):
        ``range`` the (2,) fp32 minimum and maximum of the finite values -- exactly those of ``expand(...)``;
        (+inf, -inf) without one -- and ``count`` the (1,) int64 number of non-finite ones.

        ``out``: the pair of an earlier call, which this block is MERGED into (row blocks, the runs of a group)."""
        m, k, ldu, T, Ct, ldc = self._expand_args(Ut, Ct, mean, std, "expand_range")
        rng, cnt, acc = self._range_out(out, Ut.device, "expand_range")
        ws = self._workspace(Ut.device, self._lib.dmdx_expand_range_workspace_bytes(m, k, T))
        rc = self._timed("expand_range", (m, k, T), lambda: self._lib.dmdx_expand_range_f32(
            _ptr(Ut), m, k, ldu, _ptr(Ct), ldc, T, _ptr(mean), _ptr(std), _ptr(rng), _ptr(cnt), acc, _ptr(ws),
            ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_expand_range_f32")
        return rng, cnt

    def expand_pack(self, Ut: torch.Tensor, Ct: torch.Tensor, mean: torch.Tensor | None, std: torch.Tensor | None,
                    packing, out: torch.Tensor | None = None, counts: torch.Tensor | None = None):
        """``packing.encode`` of Xhat = mean + std * (U C), Xhat never stored (operands as :meth:`expand`; ``packing``
        a :class:`labeled.Packing`) -> (Qt, counts): ``Qt`` the (T, m) int16 codes, the layout of a time slab of a
        file, ``counts`` the (2,) int64 [filled, saturated].

        ``out``: a (T, m) int16 view to write into (inner stride 1, any row stride >= m, any 2-byte aligned base);
        ``counts``: a (2,) int64 tensor that ACCUMULATES (zero it once per variable)."""
        m, k, ldu, T, Ct, ldc = self._expand_args(Ut, Ct, mean, std, "expand_pack")
        Qt, ldq, counts = self._pack_out(out, counts, m, T, Ut.device, "expand_pack")
        sf, ao = float(packing.scale_factor), float(packing.add_offset)
        rc = self._timed("expand_pack", (m, k, T), lambda: self._lib.dmdx_expand_pack_i16(
            _ptr(Ut), m, k, ldu, _ptr(Ct), ldc, T, _ptr(mean), _ptr(std), sf, ao, _ptr(Qt), ldq, _ptr(counts),
            self._stream()
        ))
        _lib.check(rc, "dmdx_expand_pack_i16")
        return Qt, counts

    def field_range(self, Xt: torch.Tensor, out=None):
        """:meth:`expand_range` of a field that exists.  Xt: (T, m) fp32 (any row stride) -> (range, count)."""
        m, T, ldx = _check_mat(Xt, torch.float32, "field_range X")
        rng, cnt, acc = self._range_out(out, Xt.device, "field_range")
        ws = self._workspace(Xt.device, self._lib.dmdx_range_workspace_bytes(m, T))
        rc = self._timed("field_range", (m, T), lambda: self._lib.dmdx_range_f32(
            _ptr(Xt), m, T, ldx, _ptr(rng), _ptr(cnt), acc, _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_range_f32")
        return rng, cnt

    def pack(self, Xt: torch.Tensor, packing, out: torch.Tensor | None = None, counts: torch.Tensor | None = None):
        """:meth:`expand_pack` of a field that exists.  Xt: (T, m) fp32 (any row stride) -> (Qt (T, m) int16, counts)."""
        m, T, ldx = _check_mat(Xt, torch.float32, "pack X")
        Qt, ldq, counts = self._pack_out(out, counts, m, T, Xt.device, "pack")
        sf, ao = float(packing.scale_factor), float(packing.add_offset)
        rc = self._timed("pack", (m, T), lambda: self._lib.dmdx_pack_f32_i16(
            _ptr(Xt), m, T, ldx, sf, ao, _ptr(Qt), ldq, _ptr(counts), self._stream()
        ))
        _lib.check(rc, "dmdx_pack_f32_i16")
        return Qt, counts

    # -- K18 ----------------------------------------------------------------
    @staticmethod
    def _clim_lists(Xt, order, start, who: str):
        """X and the CSR slot lists of clim_mean / clim_std -> (m, T, ldx, n_order, S)."""
        m, T, ldx = _check_mat(Xt, torch.float32, f"{who} X")
        n_order = _check_ivec(order, Xt.device, who, "order")
        S = _check_ivec(start, Xt.device, who, "start") - 1
        if S < 1:
            raise _lib.DmdxError(f"{who}: start must hold S + 1 >= 2 offsets")
        return m, T, ldx, n_order, S

    def clim_mean(self, Xt: torch.Tensor, order: torch.Tensor, start: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
        """The slot means of the snapshots of a row block.  Xt: (T, m) fp32 (any row stride); ``order`` / ``start``:
        device int32, the CSR list of :func:`climatology.slots_of` (slot s owns ``order[start[s]:start[s + 1]]``,
        ``start`` has S + 1 entries) -> mean (S, m) fp32: the fp64 sum over the list, in its order, divided by the
        number of entries inside [0, T) and rounded once; NaN for a slot without one.  ``out``: an (S, m) fp32 view
        to write into (inner stride 1)."""
        m, T, ldx, n_order, S = self._clim_lists(Xt, order, start, "clim_mean")
        mean, ldc = _out_view(out, m, S, torch.float32, Xt.device, "clim_mean")
        rc = self._timed("clim_mean", (m, T, S), lambda: self._lib.dmdx_clim_mean_f32(
            _ptr(Xt), m, T, ldx, _ptr(order), n_order, _ptr(start), S, _ptr(mean), ldc, self._stream()
        ))
        _lib.check(rc, "dmdx_clim_mean_f32")
        return mean

    def clim_std(self, Xt: torch.Tensor, order: torch.Tensor, start: torch.Tensor, mean: torch.Tensor, ddof: int = 0,
                 out: torch.Tensor | None = None) -> torch.Tensor:
        """The slot standard deviations about ``mean`` ((S, m) fp32 of :meth:`clim_mean`): the fp64 sum of the
        squared fp64 differences in the order of the list, divided by n_s - ddof, the correctly rounded root, one
        rounding to fp32; NaN where n_s - ddof <= 0.  Operands and ``out`` as :meth:`clim_mean`."""
        m, T, ldx, n_order, S = self._clim_lists(Xt, order, start, "clim_std")
        ldc = _check_field(mean, m, S, torch.float32, Xt.device, "clim_std", "mean")
        sd, lds = _out_view(out, m, S, torch.float32, Xt.device, "clim_std")
        rc = self._timed("clim_std", (m, T, S), lambda: self._lib.dmdx_clim_std_f32(
            _ptr(Xt), m, T, ldx, _ptr(order), n_order, _ptr(start), S, _ptr(mean), ldc, int(ddof), _ptr(sd), lds,
            self._stream()
        ))
        _lib.check(rc, "dmdx_clim_std_f32")
        return sd

    def clim_apply_(self, Xt: torch.Tensor, slot: torch.Tensor, mean: torch.Tensor, sd: torch.Tensor | None = None,
                    restore: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
        """Anomalies against a slot climatology, or back: snapshot t of Xt ((T, m) fp32) takes row ``slot[t]``
        (device int32, T labels) of ``mean`` / ``sd`` ((S, m) fp32): ``(x - mean) [/ sd]``, or with ``restore``
        ``x [* sd] + mean`` (two roundings).  A label outside 0 .. S - 1 (-1) leaves its snapshot as it is.  In
        place by default; ``out``: a (T, m) fp32 view that does not overlap Xt.  -> the tensor written."""
        m, T, ldx = _check_mat(Xt, torch.float32, "clim_apply X")
        _check_ivec(slot, Xt.device, "clim_apply", "slot", T)
        if mean.dim() != 2:
            raise _lib.DmdxError(f"clim_apply: mean must be (S, {m}) fp32, got {tuple(mean.shape)}")
        S = int(mean.shape[0])
        ldc = _check_field(mean, m, S, torch.float32, Xt.device, "clim_apply", "mean")
        lds = 0 if sd is None else _check_field(sd, m, S, torch.float32, Xt.device, "clim_apply", "sd")
        Yt, ldy = (Xt, ldx) if out is None else _out_view(out, m, T, torch.float32, Xt.device, "clim_apply")
        rc = self._timed("clim_apply", (m, T, S), lambda: self._lib.dmdx_clim_apply_f32(
            _ptr(Xt), m, T, ldx, _ptr(slot), S, _ptr(mean), ldc, _ptr(sd), lds, int(bool(restore)), _ptr(Yt), ldy,
            self._stream()
        ))
        _lib.check(rc, "dmdx_clim_apply_f32")
        return Yt

    # -- K25 ----------------------------------------------------------------
    QUANTILE_METHODS = {"linear": 0, "lower": 1, "higher": 2}

    @property
    def clim_quantile_max_q(self) -> int:
        return int(self._lib.dmdx_clim_quantile_max_q())

    @property
    def clim_quantile_max_staged(self) -> int:
        """The longest slot list whose members are staged in LDS (one read of X); longer ones are re-read per step."""
        return int(self._lib.dmdx_clim_quantile_max_staged())

    def clim_quantile(self, Xt: torch.Tensor, order: torch.Tensor, start: torch.Tensor, q, method: str = "linear",
                      out: torch.Tensor | None = None, streamed: bool = False) -> torch.Tensor:
        """The empirical quantiles of the snapshots of a row block per slot.  Xt, ``order``, ``start`` as
        :meth:`clim_mean`; ``q``: 1 .. ``clim_quantile_max_q`` values in [0, 1]; ``method``: ``"linear"`` (numpy's
        default), ``"lower"`` or ``"higher"`` -> (J, S, m) fp32, the ``thr`` of :meth:`exceed_prob`: order statistics
        with their bits, the linear interpolation in fp64 rounded once; NaN for a slot without a counted snapshot
        and where a member is NaN.  ``out``: a (J, S, m) fp32 view to write into (inner stride 1, the planes one
        uniform row stride apart).  ``streamed``: re-read the members in every step of the selection instead of
        staging them in LDS (the route of lists beyond ``clim_quantile_max_staged``; the same bits)."""
        m, T, ldx, n_order, S = self._clim_lists(Xt, order, start, "clim_quantile")
        qs = [float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1)]
        J = len(qs)
        if not 1 <= J <= self.clim_quantile_max_q or not all(0.0 <= v <= 1.0 for v in qs):
            raise _lib.DmdxError(f"clim_quantile: q must hold 1 .. {self.clim_quantile_max_q} values in [0, 1], got {q!r}")
        if method not in self.QUANTILE_METHODS:
            raise _lib.DmdxError(f"clim_quantile: method = {method!r}, expected one of {sorted(self.QUANTILE_METHODS)}")
        if out is None:
            res = torch.empty((J, S, m), dtype=torch.float32, device=Xt.device)
        else:
            if (not isinstance(out, torch.Tensor) or out.dim() != 3 or tuple(out.shape) != (J, S, m)
                    or (J > 1 and S > 1 and out.stride(0) != S * out.stride(1))):
                raise _lib.DmdxError(f"clim_quantile: out must be a ({J}, {S}, {m}) fp32 view whose planes lie one uniform "
                                     f"row stride apart")
            res = out
        row = res.stride(0) if S == 1 else res.stride(1)
        flat, ldo = _out_view(res.as_strided((J * S, m), (row, res.stride(2))), m, J * S, torch.float32, Xt.device,
                              "clim_quantile")
        qa = (ctypes.c_double * J)(*qs)
        rc = self._timed("clim_quantile", (m, T, S, J), lambda: self._lib.dmdx_clim_quantile_f32(
            _ptr(Xt), m, T, ldx, _ptr(order), n_order, _ptr(start), S, qa, J, self.QUANTILE_METHODS[method],
            int(bool(streamed)), _ptr(flat), ldo, self._stream()
        ))
        _lib.check(rc, "dmdx_clim_quantile_f32")
        return res

    # -- K21 ----------------------------------------------------------------
    # the fit cuts time over workgroups (a workspace of segment sums, added in order by a second kernel) whenever
    # there is more than one segment: rows alone fill half of the chip on a 129 780-row block (MEASUREMENTS.md K21).
    # False walks the segments in one lane; the bits are the same.
    treg_split = True

    @property
    def treg_max_p(self) -> int:
        return int(self._lib.dmdx_treg_max_p())

    def treg_fit(self, Xt: torch.Tensor, W: torch.Tensor, seg: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """The regression coefficients of every row of a block on a temporal design.  Xt: (T, m) fp32 (any row
        stride); W: (p, T) fp64 contiguous, ``(D^T D)^-1 D^T`` of the (T, p) design (:func:`trend.weights`), p <= 8;
        ``seg``: the segment length of the fp64 sums (part of the result: :data:`trend.SEGMENT`) -> coef (p, m)
        fp32: per segment the sum of ``fp64(x) * W[j, t]`` in ascending t, the segment sums added in ascending
        order, one rounding.  ``out``: a (p, m) fp32 view to write into (inner stride 1).  One read of Xt."""
        if not isinstance(W, torch.Tensor) or W.dim() != 2:
            raise _lib.DmdxError("treg_fit: W must be a (p, T) fp64 tensor")
        p, T = int(W.shape[0]), int(W.shape[1])
        if not 1 <= p <= self.treg_max_p or int(seg) < 1:
            raise _lib.DmdxError(f"treg_fit: p = {p} outside 1..{self.treg_max_p} or seg = {seg} < 1")
        m = int(Xt.shape[1]) if Xt.dim() == 2 else -1
        ldx = _check_snapshots(Xt, m, T, Xt.device, "treg_fit")
        _accumulator(W, (p, T), torch.float64, Xt.device, "treg_fit", "W")
        coef, ldc = _out_view(out, m, p, torch.float32, Xt.device, "treg_fit")
        split = self.treg_split and T > int(seg)
        nbytes = int(self._lib.dmdx_treg_fit_workspace_bytes(m, T, p, int(seg))) if split else 0
        ws = self._workspace(Xt.device, nbytes) if split else None
        rc = self._timed("treg_fit", (m, T, p), lambda: self._lib.dmdx_treg_fit_f32(
            _ptr(Xt), m, T, ldx, _ptr(W), p, T, int(seg), _ptr(coef), ldc, _ptr(ws), nbytes, self._stream()
        ))
        _lib.check(rc, "dmdx_treg_fit_f32")
        return coef

    def treg_apply_(self, Xt: torch.Tensor, D: torch.Tensor, coef: torch.Tensor, restore: bool = False,
                    out: torch.Tensor | None = None) -> torch.Tensor:
        """The fitted regression removed from the snapshots, or put back: ``y = fp32(fp64(x) -+ f)`` with
        ``f = sum over j of fp64(coef[j, i]) * D[t, j]`` in ascending j (fp64, products rounded), + with
        ``restore``.  Xt: (T, m) fp32; D: (T, p) fp64 contiguous, the design at the times of the snapshots; coef:
        (p, m) fp32 (inner stride 1).  In place by default; ``out``: a (T, m) fp32 view that does not overlap Xt.
        -> the tensor written.  One read and one write."""
        if not isinstance(D, torch.Tensor) or D.dim() != 2:
            raise _lib.DmdxError("treg_apply: D must be a (T, p) fp64 tensor")
        T, p = int(D.shape[0]), int(D.shape[1])
        if not 1 <= p <= self.treg_max_p:
            raise _lib.DmdxError(f"treg_apply: p = {p} outside 1..{self.treg_max_p}")
        m = int(Xt.shape[1]) if Xt.dim() == 2 else -1
        ldx = _check_snapshots(Xt, m, T, Xt.device, "treg_apply")
        _accumulator(D, (T, p), torch.float64, Xt.device, "treg_apply", "D")
        ldc = _check_field(coef, m, p, torch.float32, Xt.device, "treg_apply", "coef")
        Yt, ldy = (Xt, ldx) if out is None else _out_view(out, m, T, torch.float32, Xt.device, "treg_apply")
        rc = self._timed("treg_apply", (m, T, p), lambda: self._lib.dmdx_treg_apply_f32(
            _ptr(Xt), m, T, ldx, _ptr(D), p, p, _ptr(coef), ldc, int(bool(restore)), _ptr(Yt), ldy, self._stream()
        ))
        _lib.check(rc, "dmdx_treg_apply_f32")
        return Yt

    # -- K26 ----------------------------------------------------------------
    @property
    def lag_max_lags(self) -> int:
        return int(self._lib.dmdx_lag_moments_max_lags())

    @property
    def lag_ring(self) -> int:
        """The largest lag whose earlier member a lane keeps in LDS; beyond it the member is loaded again."""
        return int(self._lib.dmdx_lag_moments_ring())

    def lag_moments(self, Xt: torch.Tensor, lags, mu: torch.Tensor | None = None, seg: int = 1024,
                    out: torch.Tensor | None = None, ring: bool = True) -> torch.Tensor:
        """The lagged second moments of every row of a block.  Xt: (T, m) fp32 (any row stride); ``lags``: 1 .. 8
        strictly ascending integers, 0 <= tau < T; ``mu``: (m,) fp32 centres or None; ``seg``: the segment length of
        the fp64 sums (part of the result: :data:`baseline.SEGMENT`) -> (1 + 3L, m) fp64: plane 0 the sum of squares
        S of ``d = fp64(x) - fp64(mu)``, planes 1 + l the lagged products P_l, planes 1 + L + l and 1 + 2L + l the
        squares of the first and of the last tau_l snapshots (H_l, E_l).  ``out``: a (1 + 3L, m) fp64 view to write
        into (inner stride 1); ``ring`` False loads the earlier member of every pair again instead of keeping it
        in LDS (the same bits).  One read of Xt, time split over workgroups whenever there is more than one
        segment."""
        lags = [int(v) for v in lags]
        L = len(lags)
        if not 1 <= L <= self.lag_max_lags or int(seg) < 1:
            raise _lib.DmdxError(f"lag_moments: {L} lags outside 1..{self.lag_max_lags} or seg = {seg} < 1")
        if Xt.dim() != 2:
            raise _lib.DmdxError(f"lag_moments: X must be (T, m), got {tuple(Xt.shape)}")
        T, m = int(Xt.shape[0]), int(Xt.shape[1])
        # here and not only in C: the int32 array below would wrap a lag of 2^32 + 1 to 1, which passes there
        if T > 0 and (lags[0] < 0 or lags[-1] >= T or any(b <= a for a, b in zip(lags, lags[1:]))):
            raise _lib.DmdxError(f"lag_moments: lags must be strictly ascending with 0 <= tau < T = {T}, got {lags}")
        ldx = _check_snapshots(Xt, m, T, Xt.device, "lag_moments")
        _check_vec(mu, m, Xt.device, "lag_moments", "mu")
        planes, ldo = _out_view(out, m, 1 + 3 * L, torch.float64, Xt.device, "lag_moments")
        split = T > int(seg)
        nbytes = int(self._lib.dmdx_lag_moments_workspace_bytes(m, T, L, int(seg))) if split else 0
        ws = self._workspace(Xt.device, nbytes) if split else None
        host = (ctypes.c_int32 * L)(*lags)
        rc = self._timed("lag_moments", (m, T, L), lambda: self._lib.dmdx_lag_moments_f32(
            _ptr(Xt), m, T, ldx, _ptr(mu), host, L, int(seg), _ptr(planes), ldo, 0 if ring else 1, _ptr(ws), nbytes,
            self._stream()
        ))
        _lib.check(rc, "dmdx_lag_moments_f32")
        return planes

    # -- K27 ----------------------------------------------------------------
    @property
    def spell_max_thresholds(self) -> int:
        return int(self._lib.dmdx_spell_max_thresholds())

    @property
    def spell_max_periods(self) -> int:
        """The periods of one launch (their bounds travel by value); :meth:`spells` loops beyond."""
        return int(self._lib.dmdx_spell_max_periods())

    def spells(self, Xt: torch.Tensor, thr: torch.Tensor, bounds, min_len=1, above=True,
               slot: torch.Tensor | None = None, seg: int = 512, out: torch.Tensor | None = None) -> torch.Tensor:
        """Spell and exceedance-count indices of every row of a block, per threshold and period.  Xt: (T, m) fp32 (any
        row stride); thr: (J, S, m) or (J, m) fp32, threshold j of every row for slot s (as :meth:`exceed_prob`), J <=
        ``spell_max_thresholds``; ``bounds``: P + 1 strictly ascending integers in 0 .. T, period p is the snapshots
        [b_p, b_{p+1}); ``min_len``: the shortest run that qualifies, one integer >= 1 or one per threshold;
        ``above``: the event is x > thr, otherwise x < thr (strict), one bool or one per threshold; slot: (T,) device
        int32 labels or None (S = 1); a label outside 0 .. S - 1 makes its snapshot invalid -> (J, 7, P, m) int32:
        n_valid, n_event, n_spell, n_in_spell, longest, first, last (include/dmdx.h, K27).  A run never spans two
        periods.

        ``seg``: the snapshots of a piece of the time split; no value depends on it.  Time is split over workgroups
        whenever there is more than one piece; any number of periods runs in launches of ``spell_max_periods``.
        ``out``: a contiguous (J, 7, P, m) int32 tensor to write into."""
        who = "spells"
        if Xt.dim() != 2:
            raise _lib.DmdxError(f"{who}: X must be (T, m), got {tuple(Xt.shape)}")
        T, m = int(Xt.shape[0]), int(Xt.shape[1])
        ldx = _check_snapshots(Xt, m, T, Xt.device, who)
        # (a label outside 0 .. S - 1 is no error here: its snapshot is invalid)
        thr3, J, S = _check_threshold_table(thr, slot, m, T, Xt.device, self.spell_max_thresholds, who, False)
        b = _check_bounds(bounds, T, who)
        ml = [int(v) for v in np.atleast_1d(np.asarray(min_len)).reshape(-1)]
        ab = [bool(v) for v in np.atleast_1d(np.asarray(above)).reshape(-1)]
        ml, ab = (ml * J if len(ml) == 1 else ml), (ab * J if len(ab) == 1 else ab)
        if len(ml) != J or len(ab) != J or min(ml) < 1 or max(ml) >= 2**31 or not 1 <= int(seg) < 2**31:
            raise _lib.DmdxError(f"{who}: min_len and above hold one value or {J}, min_len >= 1 and seg >= 1 asked for "
                                 f"(min_len = {min_len!r}, above = {above!r}, seg = {seg})")
        P = len(b) - 1
        planes = _accumulator(out, (J, DMDX_SPELL_NQ, P, m), torch.int32, Xt.device, who)
        if m == 0:
            return planes
        mask = sum(1 << j for j in range(J) if ab[j])
        host_ml = (ctypes.c_int32 * J)(*ml)
        seg = int(seg)
        return self._per_period(
            "spells", "dmdx_spell_f32", planes, 2, b, self.spell_max_periods, (J,), lambda n: -(-n // seg),
            lambda hb, n: self._lib.dmdx_spell_workspace_bytes(m, hb, n, J, seg),
            lambda hb, n, part, ws, nbytes: self._lib.dmdx_spell_f32(
                _ptr(Xt), m, T, ldx, _ptr(thr3), m, J, S, _ptr(slot), mask, host_ml, hb, n, seg, _ptr(part), m, 0, _ptr(ws),
                nbytes, self._stream()))

    # -- K29 ----------------------------------------------------------------
    @property
    def period_stats_max_window(self) -> int:
        return int(self._lib.dmdx_period_stats_max_window())

    @property
    def period_stats_max_periods(self) -> int:
        """The periods of one launch (their bounds travel by value); :meth:`period_stats` loops beyond."""
        return int(self._lib.dmdx_period_stats_max_periods())

    def period_stats(self, Xt: torch.Tensor, bounds, group: int = 1, inner: str = "sum", window: int = 1,
                     min_count: int | None = None, thr: torch.Tensor | None = None, below: bool = False,
                     inclusive: bool = False, seg: int = 64, out: torch.Tensor | None = None) -> torch.Tensor:
        """Extremes and totals of a daily statistic of every row of a block, per period.  Xt: (T, m) fp32 (any row
        stride); ``bounds``: P + 1 strictly ascending integers in 0 .. T, period p is the snapshots [b_p, b_{p+1});
        ``group``: the snapshots of a day, cut from the period's start; ``inner``: ``"sum"``, ``"mean"``, ``"max"``,
        ``"min"`` or ``"range"`` of the finite snapshots of a day; ``min_count``: the finite snapshots a valid day
        needs (None: all ``group``); ``window``: the days of the running sum, 1 .. ``period_stats_max_window``, never
        across a period; ``thr``: (m,) fp32 thresholds or None; the event is r > thr, r < thr with ``below``, >= / <=
        with ``inclusive`` -> (8, P, m) fp64: n, max, argmax, min, argmin, total, event total, event count
        (include/dmdx.h, K29).

        ``seg``: the days of a piece of the time split; part of the totals (planes 5 and 6) and of nothing else
        (:data:`extremes.SEGMENT`).  Time is split over workgroups whenever there is more than one piece; any number
        of periods runs in launches of ``period_stats_max_periods``.  ``out``: a contiguous (8, P, m) fp64 tensor to
        write into."""
        who = "period_stats"
        if Xt.dim() != 2:
            raise _lib.DmdxError(f"{who}: X must be (T, m), got {tuple(Xt.shape)}")
        T, m = int(Xt.shape[0]), int(Xt.shape[1])
        ldx = _check_snapshots(Xt, m, T, Xt.device, who)
        _check_vec(thr, m, Xt.device, who, "thr")
        b = _check_bounds(bounds, T, who)
        if inner not in PSTAT_INNER:
            raise _lib.DmdxError(f"{who}: inner = {inner!r}, expected one of {PSTAT_INNER}")
        g, w, seg = int(group), int(window), int(seg)
        mc = g if min_count is None else int(min_count)
        if not (1 <= g < 2**31 and 1 <= w <= self.period_stats_max_window and 1 <= mc <= g and 1 <= seg < 2**31):
            raise _lib.DmdxError(f"{who}: group >= 1, window in 1 .. {self.period_stats_max_window}, min_count in 1 .. group "
                                 f"and seg >= 1 asked for (group = {group}, window = {window}, min_count = {min_count}, "
                                 f"seg = {seg})")
        P = len(b) - 1
        planes = _accumulator(out, (DMDX_PSTAT_NQ, P, m), torch.float64, Xt.device, who)
        if m == 0:
            return planes
        flags = (1 if below else 0) | (2 if inclusive else 0)
        return self._per_period(
            "period_stats", "dmdx_period_stats_f32", planes, 1, b, self.period_stats_max_periods, (g, w),
            lambda n: -(-(-(-n // g)) // seg), lambda hb, n: self._lib.dmdx_period_stats_workspace_bytes(m, hb, n, g, seg),
            lambda hb, n, part, ws, nbytes: self._lib.dmdx_period_stats_f32(
                _ptr(Xt), m, T, ldx, hb, n, g, PSTAT_INNER.index(inner), w, mc, _ptr(thr), seg, _ptr(part), m, flags,
                _ptr(ws), nbytes, self._stream()))

    # -- K22 ----------------------------------------------------------------
    @property
    def tfilt_max_taps(self) -> int:
        return int(self._lib.dmdx_tfilt_max_taps())

    def tfilt(self, Xt: torch.Tensor, h: torch.Tensor, stride: int = 1, out: torch.Tensor | None = None) -> torch.Tensor:
        """A FIR filter along time with an output stride.  Xt: (T, m) fp32 (any row stride); h: (L,) fp64 contiguous
        on the device, L <= :attr:`tfilt_max_taps` -> Yt (T_out, m) fp32, ``T_out = (T - L) // stride + 1`` (valid
        windows only): ``Yt[u] = fp32(sum over j of fp64(Xt[u stride + j]) * h[j])``, an fp64 chain in ascending j
        with every product rounded.  ``out``: a (T_out, m) fp32 view that does not overlap Xt (inner stride 1).  One
        read of the windows of Xt, one write."""
        if not isinstance(h, torch.Tensor) or h.dim() != 1:
            raise _lib.DmdxError("tfilt: h must be an (L,) fp64 tensor")
        L, stride = int(h.shape[0]), int(stride)
        if not 1 <= L <= self.tfilt_max_taps or stride < 1:
            raise _lib.DmdxError(f"tfilt: L = {L} outside 1..{self.tfilt_max_taps} or stride = {stride} < 1")
        m, T = (int(Xt.shape[1]), int(Xt.shape[0])) if Xt.dim() == 2 else (-1, -1)
        ldx = _check_snapshots(Xt, m, T, Xt.device, "tfilt")
        _accumulator(h, (L,), torch.float64, Xt.device, "tfilt", "h")
        if T < L:
            raise _lib.DmdxError(f"tfilt: {T} snapshots are fewer than the {L} taps of one window")
        T_out = (T - L) // stride + 1
        Yt, ldy = _out_view(out, m, T_out, torch.float32, Xt.device, "tfilt")
        rc = self._timed("tfilt", (m, T, L, stride), lambda: self._lib.dmdx_tfilt_f32(
            _ptr(Xt), m, T, ldx, _ptr(h), L, stride, _ptr(Yt), T_out, ldy, self._stream()
        ))
        _lib.check(rc, "dmdx_tfilt_f32")
        return Yt

    # -- K23 ----------------------------------------------------------------
    @property
    def coarsen_max_factor(self) -> int:
        return int(self._lib.dmdx_coarsen_max_factor())

    def coarsen(self, Xt: torch.Tensor, planes: int, nlat: int, nlon: int, w: torch.Tensor, fy: int, fx: int, *,
                ldp: int | None = None, lat0: int = 0, lon0: int = 0, n_lat_out: int | None = None,
                n_lon_out: int | None = None, skipna: bool = False, min_frac: float = 0.0,
                out: torch.Tensor | None = None, ldq: int | None = None) -> torch.Tensor:
        """The area-weighted block mean over ``fy x fx`` cells of the latitude / longitude grid.  Xt: (T, m) fp32 (any
        row stride), every snapshot ``planes`` planes of ``nlat x nlon`` points, plane p at ``p * ldp`` (default
        ``nlat * nlon``; rows beyond the last plane are pad and are not read); w: (nlat,) fp64 contiguous on the
        device, the weight of every fine latitude row -> Yt (T, rows_out) fp32, ``rows_out = (planes - 1) ldq + NLAT
        NLON``, plane p at ``p * ldq`` (default ``NLAT * NLON``), cell (I, J) at ``I * NLON + J``: the weighted mean
        of the fine rows ``lat0 + I fy ..`` and longitudes ``lon0 + J fx ..``, an fp64 chain in ascending order with one
        rounding to fp32 (include/dmdx.h, K23).  ``n_lat_out`` / ``n_lon_out``: fewer cells than fit (default: all
        whole cells).  ``skipna``: values that are not finite are left out of a cell, and a cell whose kept weight is
        below ``min_frac`` of its full weight is NaN.  ``out``: a (T, rows_out) fp32 view that does not overlap Xt
        (inner stride 1).  One read of the cells of Xt, one write."""
        planes, nlat, nlon, fy, fx, lat0, lon0 = (int(v) for v in (planes, nlat, nlon, fy, fx, lat0, lon0))
        fmax = self.coarsen_max_factor
        if not (1 <= fy <= fmax and 1 <= fx <= fmax) or min(planes, nlat, nlon, lat0, lon0) < 0:
            raise _lib.DmdxError(f"coarsen: fy = {fy} or fx = {fx} outside 1..{fmax}, or a negative size or offset")
        NLAT = max(0, (nlat - lat0) // fy) if n_lat_out is None else int(n_lat_out)
        NLON = max(0, (nlon - lon0) // fx) if n_lon_out is None else int(n_lon_out)
        ldp = nlat * nlon if ldp is None else int(ldp)
        ldq = NLAT * NLON if ldq is None else int(ldq)
        if NLAT < 0 or NLON < 0 or ldp < nlat * nlon or ldq < NLAT * NLON:
            raise _lib.DmdxError(f"coarsen: NLAT = {NLAT} or NLON = {NLON} negative, ldp = {ldp} < nlat nlon or "
                                 f"ldq = {ldq} < NLAT NLON")
        m, T = (int(Xt.shape[1]), int(Xt.shape[0])) if Xt.dim() == 2 else (-1, -1)
        ldx = _check_snapshots(Xt, m, T, Xt.device, "coarsen")
        need = (planes - 1) * ldp + nlat * nlon if planes else 0
        if m < need:
            raise _lib.DmdxError(f"coarsen: X holds {m} rows, {planes} planes of {nlat} x {nlon} (ldp = {ldp}) need {need}")
        if not isinstance(w, torch.Tensor):
            raise _lib.DmdxError("coarsen: w must be an (nlat,) fp64 tensor")
        _accumulator(w, (nlat,), torch.float64, Xt.device, "coarsen", "w")
        rows_out = (planes - 1) * ldq + NLAT * NLON if planes else 0
        Yt, ldy = _out_view(out, rows_out, T, torch.float32, Xt.device, "coarsen")
        rc = self._timed("coarsen", (planes, nlat, nlon, T, fy, fx), lambda: self._lib.dmdx_coarsen_f32(
            _ptr(Xt), T, ldx, planes, ldp, nlat, nlon, _ptr(w), fy, fx, lat0, lon0, NLAT, NLON,
            int(bool(skipna)), float(min_frac), _ptr(Yt), ldy, ldq, self._stream()
        ))
        _lib.check(rc, "dmdx_coarsen_f32")
        return Yt

    # -- K28 ----------------------------------------------------------------
    @property
    def remap_max_span(self) -> int:
        return int(self._lib.dmdx_remap_max_span())

    def remap(self, Xt: torch.Tensor, planes: int, nlat: int, nlon: int, iy0: torch.Tensor, ny: torch.Tensor,
              wy: torch.Tensor, jx0: torch.Tensor, nx: torch.Tensor, wx: torch.Tensor, *, ldp: int | None = None,
              skipna: bool = False, min_frac: float = 0.0, out: torch.Tensor | None = None,
              ldq: int | None = None) -> torch.Tensor:
        """First-order conservative remapping onto another regular latitude / longitude grid, separable in the two
        axes.  Xt: (T, m) fp32 (any row stride), every snapshot ``planes`` planes of ``nlat x nlon`` points, plane p
        at ``p * ldp`` (default ``nlat * nlon``; rows beyond the last plane are pad and are not read).  The six
        tables are contiguous on the device: ``iy0``, ``ny`` (NLAT,) int32 and ``wy`` (NLAT, SY) fp64 -- target row
        I overlaps the ``ny[I]`` source rows from ``iy0[I]`` on with the weights ``wy[I, :ny[I]]`` -- and ``jx0``,
        ``nx`` (NLON,) int32 and ``wx`` (NLON, SX) fp64, the source columns ``(jx0[J] + b) mod nlon`` -> Yt (T,
        rows_out) fp32, ``rows_out = (planes - 1) ldq + NLAT NLON``, plane p at ``p * ldq`` (default ``NLAT * NLON``),
        cell (I, J) at ``I * NLON + J``: the weighted mean of what the cell overlaps, an fp64 chain in ascending order
        with one rounding to fp32 (include/dmdx.h, K28).  ``skipna``: values that are not finite are left out of a
        cell, and a cell whose kept weight is below ``min_frac`` of its full weight is NaN.  ``out``: a (T, rows_out)
        fp32 view that does not overlap Xt (inner stride 1).  ``regrid.Remap`` forms the tables."""
        planes, nlat, nlon = int(planes), int(nlat), int(nlon)
        if min(planes, nlat, nlon) < 0:
            raise _lib.DmdxError("remap: a negative size")
        for name, t in (("iy0", iy0), ("ny", ny), ("wy", wy), ("jx0", jx0), ("nx", nx), ("wx", wx)):
            if not isinstance(t, torch.Tensor):
                raise _lib.DmdxError(f"remap: {name} must be a device tensor")
        if wy.dim() != 2 or wx.dim() != 2:
            raise _lib.DmdxError(f"remap: wy must be (NLAT, SY) and wx (NLON, SX), got {tuple(wy.shape)} and {tuple(wx.shape)}")
        (NLAT, SY), (NLON, SX) = (int(v) for v in wy.shape), (int(v) for v in wx.shape)
        smax = self.remap_max_span
        if not (1 <= SY <= smax and 1 <= SX <= smax):
            raise _lib.DmdxError(f"remap: SY = {SY} or SX = {SX} outside 1..{smax}")
        ldp = nlat * nlon if ldp is None else int(ldp)
        ldq = NLAT * NLON if ldq is None else int(ldq)
        if ldp < nlat * nlon or ldq < NLAT * NLON:
            raise _lib.DmdxError(f"remap: ldp = {ldp} < nlat nlon or ldq = {ldq} < NLAT NLON")
        m, T = (int(Xt.shape[1]), int(Xt.shape[0])) if Xt.dim() == 2 else (-1, -1)
        ldx = _check_snapshots(Xt, m, T, Xt.device, "remap")
        need = (planes - 1) * ldp + nlat * nlon if planes else 0
        if m < need:
            raise _lib.DmdxError(f"remap: X holds {m} rows, {planes} planes of {nlat} x {nlon} (ldp = {ldp}) need {need}")
        _check_ivec(iy0, Xt.device, "remap", "iy0", NLAT)
        _check_ivec(ny, Xt.device, "remap", "ny", NLAT)
        _check_ivec(jx0, Xt.device, "remap", "jx0", NLON)
        _check_ivec(nx, Xt.device, "remap", "nx", NLON)
        _accumulator(wy, (NLAT, SY), torch.float64, Xt.device, "remap", "wy")
        _accumulator(wx, (NLON, SX), torch.float64, Xt.device, "remap", "wx")
        rows_out = (planes - 1) * ldq + NLAT * NLON if planes else 0
        Yt, ldy = _out_view(out, rows_out, T, torch.float32, Xt.device, "remap")
        rc = self._timed("remap", (planes, nlat, nlon, T, NLAT, NLON), lambda: self._lib.dmdx_remap_f32(
            _ptr(Xt), T, ldx, planes, ldp, nlat, nlon, _ptr(iy0), _ptr(ny), _ptr(wy), SY, _ptr(jx0), _ptr(nx), _ptr(wx), SX,
            NLAT, NLON, int(bool(skipna)), float(min_frac), _ptr(Yt), ldy, ldq, self._stream()
        ))
        _lib.check(rc, "dmdx_remap_f32")
        return Yt

    # -- K20 ----------------------------------------------------------------
    def row_missing_count(self, Xt: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """How many snapshots of every row of a block are not finite (NaN of any payload, +-Inf; tested on the
        bits).  Xt: (n, m) fp32 (any row stride) -> count (m,) int32.  ``out``: a device int32 vector the counts
        are ADDED to (time slabs accumulate); a fresh one starts at zero.  One read of Xt, no temporary."""
        m, n, ldx = _check_mat(Xt, torch.float32, "row_missing_count X")
        count = out if out is not None else torch.zeros(m, dtype=torch.int32, device=Xt.device)
        _check_ivec(count, Xt.device, "row_missing_count", "count", m)
        rc = self._timed("row_missing_count", (m, n), lambda: self._lib.dmdx_row_missing_count_f32(
            _ptr(Xt), n, m, ldx, _ptr(count), self._stream()
        ))
        _lib.check(rc, "dmdx_row_missing_count_f32")
        return count

    def row_mask_apply_(self, Xt: torch.Tensor, count: torch.Tensor, value: float = 0.0) -> torch.Tensor:
        """In place: every element of the rows of Xt ((n, m) fp32, any row stride) with ``count[i] != 0`` becomes
        ``value`` (its bits: -0.0, NaN); the other rows are neither read nor written.  Xt may be a block of
        snapshots, a (k, rows) block of U^T or a stored field.  -> Xt."""
        m, n, ldx = _check_mat(Xt, torch.float32, "row_mask_apply X")
        _check_ivec(count, Xt.device, "row_mask_apply", "count", m)
        rc = self._timed("row_mask_apply", (m, n), lambda: self._lib.dmdx_row_mask_apply_f32(
            _ptr(Xt), n, m, ldx, _ptr(count), float(value), self._stream()
        ))
        _lib.check(rc, "dmdx_row_mask_apply_f32")
        return Xt

    # -- K31 ----------------------------------------------------------------
    @property
    def gap_fill_max_k(self) -> int:
        return int(self._lib.dmdx_gap_fill_max_k())

    @property
    def gap_mask_segment(self) -> int:
        """Snapshots of one fp64 chain of ``gap_mask``'s sums (part of their bits)."""
        return int(self._lib.dmdx_gap_mask_segment())

    @staticmethod
    def _gap_words(W, m: int, T: int, device, who: str) -> int:
        """The packed mask of a (T, m) block: (ceil(T / 32), m) int32 on `device` (inner stride 1) -> ldw."""
        return _check_field(W, m, -(-T // 32), torch.int32, device, who, "W", " int32")

    def gap_mask(self, Xt: torch.Tensor, want_sums: bool = True, split: bool = True):
        """The gaps of a block.  Xt: (T, m) fp32 (any row stride >= m) -> (W, nmiss, sums): ``W`` the
        (ceil(T / 32), m) int32 words, bit b of W[tw, i] set where Xt[32 tw + b, i] is not finite (NaN of any payload,
        +-Inf; tested on the bits); ``nmiss`` (m,) int32 the gaps per row; ``sums`` (2, m) fp64 the sum and the sum of
        squares of the finite values of every row (None without ``want_sums``), summed in segments of
        :attr:`gap_mask_segment` snapshots.  ``split`` False lets one lane walk all segments of its row instead of
        spreading them over the launch: the same bits.  One read of Xt."""
        m, T, ldx = _check_mat(Xt, torch.float32, "gap_mask X")
        dev = Xt.device
        W = torch.empty((-(-T // 32), m), dtype=torch.int32, device=dev)
        nmiss = torch.empty(m, dtype=torch.int32, device=dev)
        sums = torch.empty((2, m), dtype=torch.float64, device=dev) if want_sums else None
        use_ws = bool(split) and T > self.gap_mask_segment
        nbytes = int(self._lib.dmdx_gap_mask_workspace_bytes(m, T)) if use_ws else 0
        ws = self._workspace(dev, nbytes) if use_ws else None
        rc = self._timed("gap_mask", (m, T), lambda: self._lib.dmdx_gap_mask_f32(
            _ptr(Xt), m, T, ldx, _ptr(W), m, _ptr(nmiss), _ptr(sums), m, _ptr(ws), nbytes, self._stream()
        ))
        _lib.check(rc, "dmdx_gap_mask_f32")
        return W, nmiss, sums

    def gap_standardize_(self, Xt: torch.Tensor, W: torch.Tensor | None, mean: torch.Tensor | None,
                         std: torch.Tensor | None, back: bool = False) -> torch.Tensor:
        """In place.  Forward: an element whose bit of ``W`` is set becomes +0.0, every other
        ``fl(fl(x - mean) / std)`` (what ``row_center_scale_`` leaves for the same moments).  ``back``: every element
        becomes ``fl(fl(x std) + mean)`` and ``W`` is not looked at.  mean / std: (m,) fp32 or None (0 and 1). -> Xt."""
        m, T, ldx = _check_mat(Xt, torch.float32, "gap_standardize X")
        ldw = m if W is None else self._gap_words(W, m, T, Xt.device, "gap_standardize")
        for v, name in ((mean, "mean"), (std, "std")):
            _check_vec(v, m, Xt.device, "gap_standardize", name)
        rc = self._timed("gap_standardize", (m, T), lambda: self._lib.dmdx_gap_standardize_f32(
            _ptr(Xt), m, T, ldx, _ptr(W), ldw, _ptr(mean), _ptr(std), int(bool(back)), self._stream()
        ))
        _lib.check(rc, "dmdx_gap_standardize_f32")
        return Xt

    def gap_fill_(self, Ut: torch.Tensor, Ct: torch.Tensor, W: torch.Tensor, Xt: torch.Tensor,
                  mean: torch.Tensor | None = None, std: torch.Tensor | None = None, want_change: bool = True):
        """In place: Xt = mean + std * (U C) where the bit of ``W`` is set -- bit for bit what :meth:`expand` stores
        there -- and Xt neither read nor written where it is clear.  Ut: (k, m), Ct: (T, k), Xt: (T, m) fp32, W the
        words of :meth:`gap_mask` -> ``change_row`` (m,) fp64, sum_t bit (new - old)^2, or None without
        ``want_change``."""
        m, k, ldu, T, Ct, ldc = self._expand_args(Ut, Ct, mean, std, "gap_fill")
        ldx = _check_snapshots(Xt, m, T, Ut.device, "gap_fill")
        if ldx < m:
            raise _lib.DmdxError("gap_fill: X must not be a delay view")
        ldw = self._gap_words(W, m, T, Ut.device, "gap_fill")
        change = torch.empty(m, dtype=torch.float64, device=Ut.device) if want_change else None
        nbytes = int(self._lib.dmdx_gap_fill_workspace_bytes(m, k, T)) if want_change else 0
        ws = self._workspace(Ut.device, nbytes) if want_change else None
        rc = self._timed("gap_fill", (m, k, T), lambda: self._lib.dmdx_gap_fill_f32(
            _ptr(Ut), m, k, ldu, _ptr(Ct), ldc, T, _ptr(mean), _ptr(std), _ptr(W), ldw, _ptr(Xt), ldx, _ptr(change),
            _ptr(ws), nbytes, self._stream()
        ))
        _lib.check(rc, "dmdx_gap_fill_f32")
        return change

    # -- K32 ----------------------------------------------------------------
    @property
    def mk_max_n(self) -> int:
        """The longest series (time points per row) of :meth:`mk_stats` and :meth:`sen_slopes`."""
        return int(self._lib.dmdx_mk_max_n())

    @property
    def sen_max_ranks(self) -> int:
        return int(self._lib.dmdx_sen_max_ranks())

    def _mk_series(self, Yt: torch.Tensor, who: str) -> tuple[int, int, int]:
        m, n, ldy = _check_mat(Yt, torch.float32, f"{who} Y")
        if not 1 <= n <= self.mk_max_n:
            raise _lib.DmdxError(f"{who}: {n} time points, 1 .. {self.mk_max_n} asked for")
        return m, n, ldy

    def mk_stats(self, Yt: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """The Mann-Kendall statistics of every row of a series block.  Yt: (n, m) fp32 (any row stride), n <=
        ``mk_max_n`` time points; a point counts if it is finite -> (4, m) int32: the valid points v, S = sum over the
        pairs a < b of sgn(y_b - y_a), the tied pairs E, and the tie term G of Var(S), the sum over the tie groups of
        g (g - 1) (2 g + 5).  ``out``: a (4, m) int32 view to write into (inner stride 1).  One read of Yt."""
        m, n, ldy = self._mk_series(Yt, "mk_stats")
        res, ldo = _out_view(out, m, 4, torch.int32, Yt.device, "mk_stats", " int32")
        rc = self._timed("mk_stats", (m, n), lambda: self._lib.dmdx_mk_stats_f32(
            _ptr(Yt), m, n, ldy, _ptr(res), ldo, self._stream()
        ))
        _lib.check(rc, "dmdx_mk_stats_f32")
        return res

    def sen_slopes(self, Yt: torch.Tensor, coord, ranks: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Order statistics of the pairwise slopes of every row of a series block.  Yt as :meth:`mk_stats`; ``coord``:
        the n time coordinates (host numbers, finite, strictly ascending); ``ranks``: (J, m) int32 on the device
        (inner stride 1), J <= ``sen_max_ranks``, 0-based ranks per row among the N = v (v - 1) / 2 slopes
        fp32(fp64(y_b - y_a) / (t_b - t_a)) of the valid points, ordered by the key of their bits (-0.0 before +0.0)
        -> (J, m) fp32: the slope of that rank with its bits, NaN where the rank lies outside 0 .. N - 1.  ``out``: a
        (J, m) fp32 view to write into.  One read of Yt, no workspace."""
        who = "sen_slopes"
        m, n, ldy = self._mk_series(Yt, who)
        tc = np.asarray(coord, dtype=np.float64).reshape(-1)
        if tc.shape[0] != n or not np.isfinite(tc).all() or not (np.diff(tc) > 0).all():
            raise _lib.DmdxError(f"{who}: coord must hold {n} finite, strictly ascending numbers")
        if not isinstance(ranks, torch.Tensor) or ranks.dim() != 2 or not 1 <= int(ranks.shape[0]) <= self.sen_max_ranks:
            raise _lib.DmdxError(f"{who}: ranks must be a (J, {m}) int32 tensor, J in 1 .. {self.sen_max_ranks}")
        J = int(ranks.shape[0])
        ldr = _check_field(ranks, m, J, torch.int32, Yt.device, who, "ranks", " int32")
        res, ldo = _out_view(out, m, J, torch.float32, Yt.device, who)
        host = (ctypes.c_double * n)(*tc.tolist())
        rc = self._timed("sen_slopes", (m, n, J), lambda: self._lib.dmdx_sen_slopes_f32(
            _ptr(Yt), m, n, ldy, host, _ptr(ranks), ldr, J, _ptr(res), ldo, self._stream()
        ))
        _lib.check(rc, "dmdx_sen_slopes_f32")
        return res

    # -- K6 -----------------------------------------------------------------
    def delay_shift_sum(self, G64: torch.Tensor, d: int, want32: bool = False):
        """Gd[i, j] = sum_{k<d} G[i+k, j+k]."""
        if G64.dtype != torch.float64 or G64.dim() != 2 or G64.shape[0] != G64.shape[1]:
            raise _lib.DmdxError("delay_shift_sum: expected a square fp64 matrix")
        if not G64.is_cuda or not G64.is_contiguous():
            raise _lib.DmdxError("delay_shift_sum: expected a contiguous device tensor")
        n = G64.shape[0]
        nd = n - d + 1
        Gd = torch.empty((nd, nd), dtype=torch.float64, device=G64.device)
        Gd32 = torch.empty((nd, nd), dtype=torch.float32, device=G64.device) if want32 else None
        rc = self._lib.dmdx_delay_shift_sum_f64(
            _ptr(G64), n, n, int(d), _ptr(Gd), nd, _ptr(Gd32), nd, self._stream()
        )
        _lib.check(rc, "dmdx_delay_shift_sum_f64")
        return (Gd, Gd32) if want32 else Gd

    # -- helper -------------------------------------------------------------
    def scale_columns_(self, Yt: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
        """Y[:, j] *= alpha[j]  (Yt: (l, m), alpha: (l,) fp32)."""
        m, l, ldy = _check_mat(Yt, torch.float32, "scale_columns Y")
        if alpha.dtype != torch.float32 or alpha.numel() != l or not alpha.is_cuda:
            raise _lib.DmdxError("scale_columns: alpha must be a device fp32 vector of length l")
        rc = self._lib.dmdx_scale_columns_f32(
            _ptr(Yt), m, l, ldy, _ptr(alpha.contiguous()), self._stream()
        )
        _lib.check(rc, "dmdx_scale_columns_f32")
        return Yt


    # -- K7 -----------------------------------------------------------------
    @property
    def eigh_small_max_n(self) -> int:
        return int(self._lib.dmdx_eigh_small_max_n())

    def eigh_small(self, T: torch.Tensor):
        """Eigenpairs of a small symmetric fp64 device matrix (n <= eigh_small_max_n), one
        launch: -> (w (n,) descending, V (n, n) with the eigenvectors in its columns)."""
        if T.dim() != 2 or T.shape[0] != T.shape[1] or T.dtype != torch.float64 or not T.is_cuda:
            raise _lib.DmdxError("eigh_small: T must be a square fp64 device matrix")
        if T.stride(1) != 1:
            T = T.contiguous()
        n = T.shape[0]
        w = torch.empty(n, dtype=torch.float64, device=T.device)
        V = torch.empty((n, n), dtype=torch.float64, device=T.device)
        info = torch.zeros(1, dtype=torch.int32, device=T.device)
        rc = self._timed("eigh_small", (n,), lambda: self._lib.dmdx_eigh_small_f64(
            _ptr(T), n, T.stride(0), _ptr(w), _ptr(V), n, _ptr(info), self._stream()
        ))
        _lib.check(rc, "dmdx_eigh_small_f64")
        # the kernel stops silently at its sweep limit (30): eigenpairs of a run that did not
        # converge must not be used as exact by the Rayleigh-Ritz steps
        self.last_eigh_sweeps = int(info.item())
        if self.last_eigh_sweeps > 30:      # (31 = no rotation-free sweep within the limit of 30)
            raise _lib.DmdxError(f"eigh_small: no convergence in {self.last_eigh_sweeps} Jacobi sweeps (n = {n})")
        return w, V


    # -- K7L ----------------------------------------------------------------
    @property
    def svd_jacobi_max_n(self) -> int:
        return int(self._lib.dmdx_svd_jacobi_max_n())

    def svd_jacobi(self, Ct: torch.Tensor):
        """One-sided Jacobi SVD of a square fp64 device matrix C, given as ``Ct`` with row c =
        column c of C (2 <= n <= svd_jacobi_max_n), one launch: -> (sigma (n,) descending,
        Zt (n, n) with row j = left singular vector j).  ``Ct`` is overwritten.  Raises if the
        workgroups of the launch could not synchronise or the sweeps did not converge."""
        if Ct.dim() != 2 or Ct.shape[0] != Ct.shape[1] or Ct.dtype != torch.float64 or not Ct.is_cuda \
                or Ct.stride(1) != 1:
            raise _lib.DmdxError("svd_jacobi: Ct must be a square fp64 device matrix with inner stride 1")
        n = Ct.shape[0]
        sigma = torch.empty(n, dtype=torch.float64, device=Ct.device)
        Zt = torch.empty((n, n), dtype=torch.float64, device=Ct.device)
        info = torch.zeros(1, dtype=torch.int32, device=Ct.device)
        ws = torch.empty(self._lib.dmdx_svd_jacobi_workspace_bytes(n), dtype=torch.uint8, device=Ct.device)
        rc = self._timed("svd_jacobi", (n,), lambda: self._lib.dmdx_svd_jacobi_f64(
            _ptr(Ct), n, Ct.stride(0), _ptr(sigma), _ptr(Zt), n, _ptr(info), _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_svd_jacobi_f64")
        sweeps = int(info.item())
        if sweeps < 0:
            raise _lib.DmdxError("svd_jacobi: the workgroups of the launch could not synchronise "
                                 "(the device is occupied by another kernel that does not end)")
        if sweeps > 40:                     # (41 = no rotation-free sweep within the limit of 40)
            raise _lib.DmdxError(f"svd_jacobi: no convergence in {sweeps} sweeps (n = {n})")
        self.last_jacobi_sweeps = sweeps
        return sigma, Zt

    # -- K8 -----------------------------------------------------------------
    def symm_skinny(self, G: torch.Tensor, Q: torch.Tensor, shift: float = 0.0,
                    out: torch.Tensor | None = None) -> torch.Tensor:
        """Y = G Q - shift Q for a SYMMETRIC fp64 device matrix G (n, n) and a block Q (n, b):
        the products of the top-eigenpair solver (fp64 MFMA, one pass over G).  Shapes the
        kernel's 16-byte fragment loads cannot take (odd n or b, unaligned views) go through
        the library GEMM -- same result, ~1 ms at n = 8760."""
        if G.dtype != torch.float64 or Q.dtype != torch.float64 or G.dim() != 2 or Q.dim() != 2 \
                or G.shape[0] != G.shape[1] or Q.shape[0] != G.shape[0] or not (G.is_cuda and Q.is_cuda):
            raise _lib.DmdxError("symm_skinny: G (n, n) and Q (n, b) must be fp64 device matrices")
        n, b = Q.shape
        ok = (n >= 2 and b >= 2 and n % 2 == 0 and b % 2 == 0 and G.stride(1) == 1 and Q.stride(1) == 1
              and G.stride(0) % 2 == 0 and Q.stride(0) % 2 == 0 and G.data_ptr() % 16 == 0
              and Q.data_ptr() % 16 == 0 and b <= 4096)
        if not ok:
            Y = torch.addmm(Q, G, Q, beta=-float(shift)) if shift != 0.0 else G @ Q
            if out is not None:
                out.copy_(Y)
                return out
            return Y
        Y = out if out is not None else torch.empty((n, b), dtype=torch.float64, device=G.device)
        if Y.shape != (n, b) or Y.dtype != torch.float64 or Y.stride(1) != 1 or Y.data_ptr() == Q.data_ptr():
            raise _lib.DmdxError("symm_skinny: out must be an (n, b) fp64 tensor that does not alias Q")
        ws = self._workspace(G.device, self._lib.dmdx_symm_skinny_workspace_bytes(n, b))
        rc = self._timed("symm_skinny", (n, b), lambda: self._lib.dmdx_symm_skinny_f64(
            _ptr(G), n, G.stride(0), _ptr(Q), Q.stride(0), b, float(shift), _ptr(Y), Y.stride(0),
            _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_symm_skinny_f64")
        return Y

    # -- K9 -----------------------------------------------------------------
    def gemm_tn64(self, A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        """C = A^T B for tall fp64 device blocks A (n, b1), B (n, b2): the small Gram-type products
        of the eigen stage (fp64 MFMA, one launch + a reduce).  Odd widths / unaligned views go
        through the library GEMM."""
        if A.dtype != torch.float64 or B.dtype != torch.float64 or A.dim() != 2 or B.dim() != 2 \
                or A.shape[0] != B.shape[0] or not (A.is_cuda and B.is_cuda):
            raise _lib.DmdxError("gemm_tn64: A (n, b1) and B (n, b2) must be fp64 device matrices")
        n, b1 = A.shape
        b2 = B.shape[1]
        ok = (b1 >= 2 and b2 >= 2 and b1 % 2 == 0 and b2 % 2 == 0 and A.stride(1) == 1 and B.stride(1) == 1
              and A.stride(0) % 2 == 0 and B.stride(0) % 2 == 0 and A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0
              and n >= 256)
        if not ok:
            return A.T @ B
        Cm = torch.empty((b1, b2), dtype=torch.float64, device=A.device)
        ws = self._workspace(A.device, self._lib.dmdx_gemm_tn_f64_workspace_bytes(n, b1, b2))
        rc = self._timed("gemm_tn64", (n, b1, b2), lambda: self._lib.dmdx_gemm_tn_f64(
            _ptr(A), A.stride(0), _ptr(B), B.stride(0), n, b1, b2, _ptr(Cm), b2, _ptr(ws), ws.numel(), self._stream()
        ))
        _lib.check(rc, "dmdx_gemm_tn_f64")
        return Cm

    # -- K10 / K11 --------------------------------------------------------------
    @property
    def chol_max_n(self) -> int:
        return int(self._lib.dmdx_potrf_trtri_max_n())

    def chol_inv(self, A: torch.Tensor, shift: float = 0.0, want_inv: bool = True):
        """A + shift I = L L^T for a symmetric fp64 device matrix (n <= chol_max_n), one launch:
        -> (L (n, n) lower, Linv (n, n) lower or None, info) with ``info`` a 3-vector of device
        doubles: status (0 ok; j + 1 = first bad pivot, outputs finite but meaningless; -1 = the
        launch could not synchronise), min and max of diag(L).  Nothing is read back here: the
        caller queues what follows and looks at ``info`` once."""
        if A.dim() != 2 or A.shape[0] != A.shape[1] or A.dtype != torch.float64 or not A.is_cuda:
            raise _lib.DmdxError("chol_inv: A must be a square fp64 device matrix")
        if A.stride(1) != 1:
            A = A.contiguous()
        n = A.shape[0]
        L = torch.empty((n, n), dtype=torch.float64, device=A.device)
        Linv = torch.empty((n, n), dtype=torch.float64, device=A.device) if want_inv else None
        info = torch.empty(3, dtype=torch.float64, device=A.device)
        ws = torch.empty(self._lib.dmdx_potrf_trtri_workspace_bytes(n), dtype=torch.uint8, device=A.device)
        rc = self._timed("chol_inv", (n,), lambda: self._lib.dmdx_potrf_trtri_f64(
            _ptr(A), n, A.stride(0), float(shift), _ptr(L), n, _ptr(Linv), n, _ptr(info), _ptr(ws), ws.numel(),
            self._stream()
        ))
        _lib.check(rc, "dmdx_potrf_trtri_f64")
        return L, Linv, info

    def gemm_nt64(self, Q: torch.Tensor, Mt: torch.Tensor) -> torch.Tensor:
        """Y = Q Mt^T for a tall fp64 device block Q (n, b1) and a small Mt (b2, b1): fp64 MFMA, one
        launch.  Odd b1 / unaligned views go through the library GEMM."""
        if Q.dtype != torch.float64 or Mt.dtype != torch.float64 or Q.dim() != 2 or Mt.dim() != 2 \
                or Q.shape[1] != Mt.shape[1] or not (Q.is_cuda and Mt.is_cuda):
            raise _lib.DmdxError("gemm_nt64: Q (n, b1) and Mt (b2, b1) must be fp64 device matrices")
        n, b1 = Q.shape
        b2 = Mt.shape[0]
        ok = (b1 >= 2 and b1 % 2 == 0 and Q.stride(1) == 1 and Mt.stride(1) == 1 and Q.stride(0) % 2 == 0
              and Mt.stride(0) % 2 == 0 and Q.data_ptr() % 16 == 0 and Mt.data_ptr() % 16 == 0 and n >= 1 and b2 >= 1)
        if not ok:
            return Q @ Mt.T
        Y = torch.empty((n, b2), dtype=torch.float64, device=Q.device)
        rc = self._timed("gemm_nt64", (n, b1, b2), lambda: self._lib.dmdx_gemm_nt_f64(
            _ptr(Q), Q.stride(0), n, b1, _ptr(Mt), Mt.stride(0), b2, _ptr(Y), b2, self._stream()
        ))
        _lib.check(rc, "dmdx_gemm_nt_f64")
        return Y

    # -- packed upper triangle (the Gram all-reduce of the row-sharded path) -----
    def pack_triu(self, A: torch.Tensor) -> torch.Tensor:
        """Upper triangle of a square fp64 device matrix, row by row: n (n + 1) / 2 doubles."""
        if A.dtype != torch.float64 or A.dim() != 2 or A.shape[0] != A.shape[1] or not A.is_cuda or A.stride(1) != 1:
            raise _lib.DmdxError("pack_triu: expected a square fp64 device matrix with inner stride 1")
        n = A.shape[0]
        packed = torch.empty(n * (n + 1) // 2, dtype=torch.float64, device=A.device)
        _lib.check(self._lib.dmdx_pack_triu_f64(_ptr(A), n, A.stride(0), _ptr(packed), self._stream()),
                   "dmdx_pack_triu_f64")
        return packed

    def unpack_triu(self, packed: torch.Tensor, n: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """The symmetric (n, n) matrix whose upper triangle ``packed`` holds (both triangles written)."""
        if packed.dtype != torch.float64 or packed.numel() != n * (n + 1) // 2 or not packed.is_cuda:
            raise _lib.DmdxError("unpack_triu: packed must hold n (n + 1) / 2 fp64 device values")
        A = out if out is not None else torch.empty((n, n), dtype=torch.float64, device=packed.device)
        _lib.check(self._lib.dmdx_unpack_triu_f64(_ptr(packed.contiguous()), n, _ptr(A), A.stride(0), self._stream()),
                   "dmdx_unpack_triu_f64")
        return A

    # -- optimized DMD ---------------------------------------------------------
    def exp_basis(self, alpha: torch.Tensor, t: torch.Tensor, dtype: torch.dtype, want_w: bool = True):
        """Phi = exp(t alpha^T) (n, r) and W = diag(t) Phi in ``dtype`` (complex64 / complex128) from
        complex128 alpha (r,) and fp64 t (n,) on the device: one launch, exponent in fp64."""
        if alpha.dtype != torch.complex128 or t.dtype != torch.float64 or not (alpha.is_cuda and t.is_cuda):
            raise _lib.DmdxError("exp_basis: alpha complex128 and t float64 device tensors expected")
        if dtype not in (torch.complex64, torch.complex128):
            raise _lib.DmdxError("exp_basis: dtype must be complex64 or complex128")
        n, r = t.numel(), alpha.numel()
        a = torch.view_as_real(alpha.contiguous()).contiguous()
        Phi = torch.empty((n, r), dtype=dtype, device=t.device)
        W = torch.empty((n, r), dtype=dtype, device=t.device) if want_w else None
        rc = self._lib.dmdx_exp_basis(_ptr(a), _ptr(t.contiguous()), n, r, _ptr(Phi), _ptr(W),
                                      int(dtype == torch.complex64), self._stream())
        _lib.check(rc, "dmdx_exp_basis")
        return Phi, W

    # -- measurement aid ------------------------------------------------------
    def clock_probe(self, counters: torch.Tensor | None) -> None:
        """Switch the per-workgroup clock stamps of the batched Gram launch on (3 zeroed device
        uint64 / int64) or off (None): bench.py's calibration block only."""
        _lib.check(self._lib.dmdx_set_clock_probe(_ptr(counters)), "dmdx_set_clock_probe")


_default: HipKernels | None = None


def default_kernels() -> HipKernels:
    """The process-wide HIP kernel provider (raises if library / GPU is missing)."""
    global _default
    if _default is None:
        _default = HipKernels()
    return _default


def release_cached_workspaces() -> int:
    """Free the partial-tile workspaces of the process-wide provider, if one exists (main() does
    after every run: 5-10 GB at cfg2 / cfg3 that the next, possibly larger, slice may need)."""
    return _default.release_workspace() if _default is not None else 0
