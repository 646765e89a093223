"""Guard zones, poisoned pads and exact workspaces for the kernel memory tests.

The C ABI (include/dmdx.h) takes plain pointers, sizes and leading dimensions.  Its memory
contract -- elements outside the logical (rows, cols) of an operand are never used for a result
and never written; a workspace of ``*_workspace_bytes`` needs no initialisation and is enough --
cannot be seen through tight ``torch.empty`` tensors.  This module builds operands whose
surroundings are recognisable, so that a stray load shows up as a NaN in the result and a stray
store as a changed bit pattern.  It is a plain helper (no fixtures, no pytest hooks) and works on
CPU tensors as well, which is how tests/test_memguard.py checks it.

Layout of one guarded matrix (one flat allocation, element offsets)::

    | front guard | matrix region: cols * ld elements                  | back guard |
                  ^ start: `base_offset_elems` past a 16-byte boundary
                  column j = [start + j*ld, start + j*ld + rows) logical, then ld - rows of pad

``rows > ld`` (the zero-copy delay-embedding view of the input X, columns overlap) is allowed:
the region is then ``(cols - 1) * ld + rows`` elements, all of them logical.

Every element of the allocation starts as the CANARY, a quiet NaN with a fixed payload
(fp32 0x7FC0DEAD, fp64 0x7FF8DEADDEADDEAD), and all comparisons are made on the integer view of
the buffer: NaN != NaN would hide everything in a float comparison, and a kernel that reads a
canary and writes "the same" NaN back through an arithmetic instruction (x * 0, x - x) is caught
because the payload or the sign does not survive.

Guard sizes, and why.  The kernels work in tiles of at most 128 columns and chunks of at most
64 rows; their partial tiles are at most 128 KiB.  A kernel that is off by one tile column writes
up to 128 * ld elements past the matrix, one that is off by a tile row or a chunk a few hundred
elements.  So
  * the back guard is ``128 * ld + 4096`` elements while that stays <= 256 MiB, and 1 MiB
    otherwise (the leading-dimension threshold cases, where 128 columns are gigabytes);
  * the front guard is 64 KiB (negative offsets: the LDS-DMA path of K1 / K3 biases its base
    pointer by -3 KiB), rounded so that the requested alignment holds;
  * an exact workspace is followed by 4 MiB of canary bytes (32 of the largest partial tiles) and
    preceded by 64 KiB.
An off-by-one-tile store then lands in allocated memory and the test fails on an assertion
instead of a GPU fault.  An error larger than that can still fault; the tests are written so
that every argument describes memory that exists.
"""

from __future__ import annotations

import numpy as np
import torch

CANARY32 = 0x7FC0DEAD
CANARY64 = 0x7FF8DEADDEADDEAD
FRONT_GUARD_BYTES = 64 * 1024
BACK_GUARD_COLS = 128
BACK_GUARD_EXTRA = 4096
BACK_GUARD_LIMIT_BYTES = 256 * 2**20
BACK_GUARD_MIN_BYTES = 2**20
WS_GUARD_BYTES = 4 * 2**20
POISON_BYTE = 0xFF
_CHUNK = 1 << 27          # elements compared per step (bounds the temporaries on 17 GB operands)

_INT = {torch.float32: torch.int32, torch.float64: torch.int64}
_CANARY = {torch.float32: CANARY32, torch.float64: CANARY64}


class GuardError(AssertionError):
    pass


def _first_bad(bad: torch.Tensor):
    """Index (tuple) of the first True of a boolean tensor, or None."""
    if not bool(bad.any()):
        return None
    return tuple(int(v) for v in torch.nonzero(bad)[0])


class Guarded:
    """Handle of one guarded matrix: where it lives and how to check its surroundings."""

    def __init__(self, rows, cols, ld, dtype, base_offset_elems, device):
        if dtype not in _INT:
            raise ValueError(f"guarded: fp32 or fp64 only, got {dtype}")
        if rows < 1 or cols < 1 or ld < 1 or base_offset_elems < 0:
            raise ValueError("guarded: rows, cols, ld >= 1 and base_offset_elems >= 0")
        self.rows, self.cols, self.ld, self.dtype = int(rows), int(cols), int(ld), dtype
        self.itemsize = 4 if dtype == torch.float32 else 8
        self.canary = _CANARY[dtype]
        self.overlapping = rows > ld
        self.region = (cols - 1) * ld + rows if self.overlapping else cols * ld
        back = BACK_GUARD_COLS * ld + BACK_GUARD_EXTRA
        if back * self.itemsize > BACK_GUARD_LIMIT_BYTES:
            back = BACK_GUARD_MIN_BYTES // self.itemsize
        front = FRONT_GUARD_BYTES // self.itemsize
        per16 = 16 // self.itemsize
        # worst-case slack for the alignment adjustment: one 16-byte unit + the requested offset
        total = front + per16 + base_offset_elems + self.region + back
        self.ibuf = torch.empty(total, dtype=_INT[dtype], device=device)
        self.ibuf.fill_(self.canary)
        self.fbuf = self.ibuf.view(dtype)
        misalign = (self.ibuf.data_ptr() // self.itemsize + front) % per16
        self.start = front + (per16 - misalign) % per16 + int(base_offset_elems)
        self.back = total - self.start - self.region
        self.view = self.fbuf.as_strided((self.cols, self.rows), (self.ld, 1), self.start)
        self.iview = self.ibuf.as_strided((self.cols, self.rows), (self.ld, 1), self.start)
        self._snapshot = None

    # ---- addresses -------------------------------------------------------
    @property
    def ptr(self) -> int:
        """Device address of element (0, 0)."""
        return self.ibuf.data_ptr() + self.start * self.itemsize

    def col_ptr(self, j: int) -> int:
        return self.ptr + j * self.ld * self.itemsize

    # ---- content ---------------------------------------------------------
    def fill(self, host_array) -> "Guarded":
        fill(self.view, host_array)
        return self

    def snapshot(self) -> "Guarded":
        """Remember the logical elements bit for bit (an input that must not be modified)."""
        self._snapshot = self.iview.clone() if not self.overlapping else \
            self.ibuf[self.start:self.start + self.region].clone()
        return self

    def logical(self) -> np.ndarray:
        """The logical elements as a host array of shape (rows, cols)."""
        return self.view.cpu().numpy().T.copy()

    # ---- checks ------------------------------------------------------------
    def check_untouched(self, name="operand"):
        c = self.canary
        off = _first_bad(self.ibuf[:self.start] != c)
        if off is not None:
            raise GuardError(f"{name}: front guard modified at buffer offset {off[0]} "
                             f"({self.start - off[0]} elements before the matrix)")
        tail = self.ibuf[self.start + self.region:]
        off = _first_bad(tail != c)
        if off is not None:
            raise GuardError(f"{name}: back guard modified at buffer offset {self.start + self.region + off[0]} "
                             f"({off[0]} elements past the matrix region)")
        npad = self.ld - self.rows
        if self.overlapping or npad <= 0:
            return
        pad = self.ibuf.as_strided((self.cols, npad), (self.ld, 1), self.start + self.rows)
        step = max(1, _CHUNK // npad)
        for j0 in range(0, self.cols, step):
            off = _first_bad(pad[j0:j0 + step] != c)
            if off is not None:
                j, i = j0 + off[0], self.rows + off[1]
                raise GuardError(f"{name}: pad modified at column {j}, row {i} (rows = {self.rows}, ld = {self.ld}; "
                                 f"buffer offset {self.start + j * self.ld + i})")

    def check_fully_written(self, name="output"):
        if self.overlapping:
            raise ValueError("assert_fully_written: not defined for an overlapping view")
        step = max(1, _CHUNK // self.rows)
        for j0 in range(0, self.cols, step):
            off = _first_bad(self.iview[j0:j0 + step] == self.canary)
            if off is not None:
                raise GuardError(f"{name}: logical element (row {off[1]}, column {j0 + off[0]}) was never written "
                                 f"(still the canary)")

    def check_unchanged(self, name="input"):
        if self._snapshot is None:
            raise ValueError("assert_unchanged: no snapshot taken")
        now = self.iview if not self.overlapping else self.ibuf[self.start:self.start + self.region]
        off = _first_bad(now != self._snapshot)
        if off is not None:
            raise GuardError(f"{name}: logical element {off} of an input was modified")


class Workspace:
    """Exactly `nbytes` usable bytes of 0xFF (NaN as float or double) between canary guards."""

    def __init__(self, nbytes, device):
        self.nbytes = int(nbytes)
        if self.nbytes < 0:
            raise ValueError("exact_workspace: nbytes >= 0")
        total = FRONT_GUARD_BYTES + 16 + self.nbytes + WS_GUARD_BYTES
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        self.start = FRONT_GUARD_BYTES + (-(self.buf.data_ptr() + FRONT_GUARD_BYTES)) % 16
        pat = torch.tensor([(CANARY32 >> (8 * k)) & 0xFF for k in range(4)], dtype=torch.uint8, device=device)
        self._expect = pat.repeat((total + 3) // 4)[:total]
        self.buf.copy_(self._expect)
        self.buf[self.start:self.start + self.nbytes] = POISON_BYTE

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + self.start

    def check_untouched(self, name="workspace"):
        off = _first_bad(self.buf[:self.start] != self._expect[:self.start])
        if off is not None:
            raise GuardError(f"{name}: front guard modified {self.start - off[0]} bytes before the workspace")
        end = self.start + self.nbytes
        off = _first_bad(self.buf[end:] != self._expect[end:])
        if off is not None:
            raise GuardError(f"{name}: back guard modified {off[0]} bytes past the declared {self.nbytes} bytes")

    def check_unused(self, name="workspace"):
        """The usable part still holds the poison (a refused call must not touch it)."""
        off = _first_bad(self.buf[self.start:self.start + self.nbytes] != POISON_BYTE)
        if off is not None:
            raise GuardError(f"{name}: byte {off[0]} of the usable part was written")


# ---- the functional face -----------------------------------------------------
def guarded(rows, cols, ld, dtype, base_offset_elems=0, device="cuda"):
    """-> (view, handle): `view` is the (cols, rows) tensor with strides (ld, 1) that
    dmd_era5_amd/kernels.py's layout convention expects for a column-major rows x cols matrix
    with leading dimension ld, starting `base_offset_elems` past a 16-byte boundary; every
    element of the allocation is the canary."""
    h = Guarded(rows, cols, ld, dtype, base_offset_elems, device)
    return h.view, h


def fill(view, host_array) -> None:
    """Write the logical elements only: `host_array` is the rows x cols matrix (or anything that
    broadcasts against it, e.g. a scalar)."""
    a = np.asarray(host_array)
    if a.ndim == 0:
        view.fill_(float(a))
        return
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.shape != (view.shape[1], view.shape[0]):
        raise ValueError(f"fill: expected a {(view.shape[1], view.shape[0])} array, got {a.shape}")
    src = torch.from_numpy(np.ascontiguousarray(a.T)).to(dtype=view.dtype)
    view.copy_(src.to(view.device))


def assert_untouched(handle, name=None) -> None:
    """Front guard, back guard and the ld - rows pad of every column still hold the canary,
    compared as integers; names the first offending offset and its region."""
    handle.check_untouched(*([name] if name else []))


def assert_fully_written(handle, name=None) -> None:
    """No logical element still carries the canary bit pattern."""
    handle.check_fully_written(*([name] if name else []))


def assert_unchanged(handle, name=None) -> None:
    """The logical elements equal the snapshot taken with handle.snapshot(), bit for bit."""
    handle.check_unchanged(*([name] if name else []))


def exact_workspace(nbytes, device="cuda") -> Workspace:
    return Workspace(nbytes, device)
