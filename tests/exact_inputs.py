"""Inputs whose kernel results are known exactly, and the NaN / Inf class reference
(tests/test_gpu_value_domain.py uses them on the GPU, tests/test_exact_inputs.py checks them on the CPU).

Exact integer operands.  A tall operand of m rows is never built on the host: row i is entry d(i)
of a small dictionary R (D distinct integer rows of length n, entries in [-a, a]), d(i) a fixed
integer hash of i (`row_map`, no period).  Then, whatever m is,
    X^T X = R^T diag(c) R            c = dictionary counts              (`gram_ref`)
    A^T B = R_A^T C R_B              C = D_A x D_B co-occurrence counts (`tn_ref`)
    X W   = (R W)[d(i), :]                                              (`skinny_ref`)
are integer matrices that cost milliseconds.  With a_A a_B K < 2^24 (`product_exact`) every partial
sum of every summation order and grouping is an integer below 2^24 in magnitude, i.e. exactly
representable in fp32: ANY correct kernel returns the reference bit for bit, and a kernel that
drops, repeats or swaps ONE row differs by a non-zero integer matrix.  Nothing here leans on how the
kernels chain or split their sums.

The references are evaluated by the fp64 BLAS on integer-valued operands: exact while every partial
sum stays below 2^53, which the functions assert (the brute-force int64 products of
test_exact_inputs.py confirm it).
"""
import math

import numpy as np

D_DEFAULT = 61
TWO24 = 1 << 24
_MASK = 0xFFFFFFFF
_MUL = 0x45D9F3B            # (< 2^27: the products below stay inside int64 for numpy and torch alike)


# ------------------------------------------------------------------ the row map
def _mix(h):
    """Integer hash on int64 arrays / tensors (the same expression serves numpy and torch)."""
    h = ((h >> 16) ^ h) * _MUL & _MASK
    h = ((h >> 16) ^ h) * _MUL & _MASK
    return (h >> 16) ^ h


def row_map(m, D=D_DEFAULT, salt=0, start=0):
    """d(i) for i = start .. start + m - 1 (int64 numpy)."""
    i = np.arange(start, start + m, dtype=np.int64)
    return _mix(i + (int(salt) * 7919 + 1)) % D


def row_map_torch(m, D=D_DEFAULT, salt=0, start=0, device="cuda"):
    import torch

    i = torch.arange(start, start + m, dtype=torch.int64, device=device)
    return _mix(i + (int(salt) * 7919 + 1)) % D


# ------------------------------------------------------------------ the dictionary
def dictionary(D, n, a, seed=0):
    """(D, n) int64, entries in [-a, a]: the rows are distinct, none is zero, both extremes occur and
    every column is non-zero in most rows."""
    assert a >= 1 and D >= 2 and n >= 1 and 2 * D < (2 * a + 1) ** min(n, 20)
    rs = np.random.RandomState(1000 + seed)
    for _ in range(100):
        rows, seen = [], set()
        while len(rows) < D:
            r = rs.randint(-a, a + 1, size=n).astype(np.int64)
            if a == 1:                               # (a third of the entries would be zero: thin them out)
                z = (r == 0) & (rs.rand(n) < 0.5)
                r[z] = rs.choice([-1, 1], size=int(z.sum()))
            if len(rows) == 0:
                r[0] = a
            if len(rows) == D - 1:
                r[-1] = -a
            if r.any() and r.tobytes() not in seen:
                seen.add(r.tobytes())
                rows.append(r)
        R = np.stack(rows)
        if D < 20 or bool(np.all((R != 0).mean(axis=0) > 0.5)):
            return R
    raise AssertionError("no admissible dictionary drawn")


def max_a_product(K_total, a_other=None):
    """Largest a with a * a_other * K_total < 2^24 (a_other = a when None); 0 if there is none."""
    K_total = int(K_total)
    if a_other is None:
        a = math.isqrt((TWO24 - 1) // K_total)
        return a
    return (TWO24 - 1) // (K_total * int(a_other))


def product_exact(a_A, a_B, K_total):
    """The exactness condition of A^T B (and of X^T X with a_A = a_B): every partial sum of every
    order and grouping is an integer of magnitude < 2^24."""
    return int(a_A) * int(a_B) * int(K_total) < TWO24


def max_a_skinny(n, a_W=None):
    """Largest a_X with n * a_X * a_W < 2^24 (a_W = a_X when None)."""
    return max_a_product(n, a_W)


def skinny_exact(n, a_X, a_W):
    return product_exact(a_X, a_W, n)


# ------------------------------------------------------------------ closed forms
def counts(d, D=D_DEFAULT):
    return np.bincount(d, minlength=D).astype(np.int64)


def cooccurrence(dA, dB, DA=D_DEFAULT, DB=D_DEFAULT):
    return np.bincount(dA * DB + dB, minlength=DA * DB).astype(np.int64).reshape(DA, DB)


def _exact_matmul(P, Q):
    """Integer P @ Q through the fp64 BLAS; exact because |P| @ |Q| < 2^53 bounds every partial sum."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    assert float(np.abs(P).sum(axis=1).max()) * float(np.abs(Q).max()) < 2.0 ** 53
    out = P @ Q
    assert np.array_equal(out, np.rint(out))
    return out.astype(np.int64)


def gram_ref(R, c):
    """X^T X (n x n int64) of the operand whose dictionary entry k occurs c[k] times."""
    return _exact_matmul((R * np.asarray(c)[:, None]).T, R)


def tn_ref(RA, RB, Cc):
    """A^T B (na x nb int64) from the co-occurrence counts Cc[ka, kb]."""
    return _exact_matmul(RA.T, _exact_matmul(Cc, RB))


def skinny_ref(R, W):
    """R W (D x l int64): row i of X W is row d(i) of it."""
    return _exact_matmul(R, W)


def embed_dictionary(R, d):
    """Dictionary of the delay-embedded view E[k m + s, t] = X[s, t + k] of an operand with
    dictionary R (D x n): entry k D + e = R[e, k : k + n - d + 1]; row k m + s maps to k D + d(s)."""
    nd = R.shape[1] - d + 1
    return np.concatenate([R[:, k:k + nd] for k in range(d)])


def device_operand(R, d_dev):
    """The (n, m) fp32 device tensor X^T of the operand with rows R[d(i)] (column-major m x n, ld = m)."""
    import torch

    Rt = torch.from_numpy(np.ascontiguousarray(R.T).astype(np.float32)).to(d_dev.device)
    return torch.index_select(Rt, 1, d_dev)


def host_operand(R, d):
    """The m x n int64 operand itself (small m only: the CPU checks)."""
    return R[d]


# ------------------------------------------------------------------ NaN / Inf classes
FINITE, NAN, PINF, NINF = 0, 1, 2, 3


def value_class(x):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf, element-wise (numpy arrays; torch tensors via .numpy())."""
    x = np.asarray(x)
    return (np.isnan(x) * NAN + np.isposinf(x) * PINF + np.isneginf(x) * NINF).astype(np.int8)


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def tn_class_ref(A, B):
    """Classes of A^T B evaluated by numpy in fp64 on the fp32 inputs (K x na, K x nb)."""
    with np.errstate(all="ignore"):
        return value_class(_f64(A).T @ _f64(B))


def nn_class_ref(X, W):
    with np.errstate(all="ignore"):
        return value_class(_f64(X) @ _f64(W))


def touched_tn(A, B):
    """na x nb bool: the entries of A^T B a non-finite element of A or B takes part in."""
    ra = ~np.isfinite(np.asarray(A)).all(axis=0)
    rb = ~np.isfinite(np.asarray(B)).all(axis=0)
    return ra[:, None] | rb[None, :]


# ------------------------------------------------------------------ the chain bound of part C
def chain_bound_factor(K):
    """Relative worst case (Higham) of what the header of dmdx.h promises for K1 / K3: one fp32 chain
    of at most 4096 rows, a blocked fp32 sum of at most 16 chain results, fp64 beyond (+ 2 for the
    roundings of the products and of the fp32 copy); times sum |a||b|.  Does not grow with K."""
    return (min(int(K), 4096) / 2 + 16 + 2) * 2.0 ** -24 * 1.01
