"""CPU checks of tests/exact_inputs.py, the machinery behind tests/test_gpu_value_domain.py:
the closed forms equal brute-force int64 products, the exactness condition is right at its boundary
(fp32 sums in any order are bit-identical to the integers), one flipped row changes the expected
result, and the NaN / Inf class reference agrees with the CPU kernel double."""
import numpy as np
import pytest
import torch

import exact_inputs as ei
from kernel_double import CpuKernelDouble

K = CpuKernelDouble()


def _f32_sum_orders(A, B):
    """fp32 evaluations of A^T B in several summation orders (every partial sum rounded to fp32)."""
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    m = A.shape[0]
    rs = np.random.RandomState(m)

    def chain(order):
        acc = np.zeros((A.shape[1], B.shape[1]), dtype=np.float32)
        for i in order:
            acc += np.outer(A32[i], B32[i])          # fp32 product (exact: |a b| < 2^24), fp32 add
        return acc

    yield "natural", chain(range(m))
    yield "reversed", chain(range(m - 1, -1, -1))
    yield "permuted", chain(rs.permutation(m))
    parts = [chain(range(s, min(s + 37, m))) for s in range(0, m, 37)]      # chunked, then summed
    tot = np.zeros_like(parts[0])
    for p in parts[::-1]:
        tot += p
    yield "chunked", tot
    yield "blas", A32.T @ B32                         # whatever order sgemm takes


@pytest.mark.parametrize("m,n,D", [(1, 5, 7), (257, 9, 61), (5000, 13, 61)])
def test_gram_closed_form_equals_brute_force(m, n, D):
    a = ei.max_a_product(m)
    R = ei.dictionary(D, n, min(a, 9), seed=m)
    d = ei.row_map(m, D)
    X = ei.host_operand(R, d)
    ref = ei.gram_ref(R, ei.counts(d, D))
    assert ref.dtype == np.int64 and np.array_equal(ref, X.T @ X)
    # the blocks variants: the counts of the row ranges add up
    cuts = [0, m // 3, m // 3 + 1 if m > 3 else m // 3, m]
    tot = sum(ei.gram_ref(R, ei.counts(ei.row_map(b - s, D, start=s), D)) for s, b in zip(cuts[:-1], cuts[1:]) if b > s)
    assert np.array_equal(tot, ref)


@pytest.mark.parametrize("m,na,nb", [(1, 3, 2), (300, 7, 5), (4099, 11, 3)])
def test_tn_closed_form_equals_brute_force(m, na, nb):
    RA, RB = ei.dictionary(61, na, 3, seed=1), ei.dictionary(11, nb, 2, seed=2)
    dA, dB = ei.row_map(m, 61, salt=1), ei.row_map(m, 11, salt=2)
    A, B = ei.host_operand(RA, dA), ei.host_operand(RB, dB)
    ref = ei.tn_ref(RA, RB, ei.cooccurrence(dA, dB, 61, 11))
    assert np.array_equal(ref, A.T @ B)
    half = m // 2
    parts = [(0, half), (half, m)]
    tot = sum(ei.tn_ref(RA, RB, ei.cooccurrence(ei.row_map(b - s, 61, 1, s), ei.row_map(b - s, 11, 2, s), 61, 11))
              for s, b in parts)
    assert np.array_equal(tot, ref)


@pytest.mark.parametrize("m,n,l,delay", [(100, 12, 5, 1), (1003, 40, 17, 1), (255, 40, 7, 3)])
def test_skinny_closed_form_equals_brute_force(m, n, l, delay):
    a = ei.max_a_skinny(n)
    assert ei.skinny_exact(n, a, a) and not ei.skinny_exact(n, a + 1, a + 1)
    R = ei.dictionary(61, n, a, seed=3)
    d = ei.row_map(m)
    X = ei.host_operand(R, d)
    nd = n - delay + 1
    W = np.random.RandomState(l).randint(-a, a + 1, size=(nd, l)).astype(np.int64)
    E = np.concatenate([X[:, k:k + nd] for k in range(delay)])           # (delay m, nd): row k m + s
    Re = ei.embed_dictionary(R, delay)
    de = np.concatenate([k * 61 + d for k in range(delay)])
    assert np.array_equal(Re[de], E)
    assert np.array_equal(ei.skinny_ref(Re, W)[de], E @ W)


def test_row_map_has_no_short_period_and_matches_torch():
    d = ei.row_map(1 << 16)
    for p in (1, 2, 4, 32, 61, 64, 256, 4096):
        assert np.mean(d[p:] == d[:-p]) < 0.05                       # (1 / 61 expected)
    c = ei.counts(d)
    assert c.min() > 0.8 * (1 << 16) / 61 and c.sum() == 1 << 16
    assert np.array_equal(ei.row_map(1000, 61, salt=3, start=12345),
                          ei.row_map_torch(1000, 61, salt=3, start=12345, device="cpu").numpy())
    assert np.array_equal(ei.row_map(100, start=50), ei.row_map(150)[50:])
    assert not np.array_equal(ei.row_map(1000, salt=1), ei.row_map(1000, salt=2))


def test_dictionary_properties():
    for a in (1, 3, 7):
        R = ei.dictionary(61, 300, a)
        assert R.min() == -a and R.max() == a and len({r.tobytes() for r in R}) == 61
        assert np.all(np.any(R != 0, axis=1)) and np.all((R != 0).mean(axis=0) > 0.5)


@pytest.mark.parametrize("K_total", [1, 1000, 4099, 131072, 1038240, 1864135, 16777215])
def test_admissible_a_at_its_boundary(K_total):
    a = ei.max_a_product(K_total)
    assert a >= 1 and ei.product_exact(a, a, K_total) and not ei.product_exact(a + 1, a + 1, K_total)
    b = ei.max_a_product(K_total, a_other=1)
    assert ei.product_exact(b, 1, K_total) and not ei.product_exact(b + 1, 1, K_total)
    assert ei.max_a_product(1 << 24) == 0


@pytest.mark.parametrize("m", [1864, 4099])
def test_fp32_sums_are_exact_in_any_order_at_the_boundary(m):
    """With a at its largest admissible value and every row at +-a in some column (the worst case is
    reached: a column of all a gives a^2 m), fp32 sums of any order equal the int64 result."""
    a = ei.max_a_product(m)
    assert ei.product_exact(a, a, m)
    R = ei.dictionary(61, 6, a, seed=m)
    R[:, 0] = a                                            # G[0, 0] = a^2 m, the largest admissible sum
    R[:, 1] = -a
    d = ei.row_map(m)
    X = ei.host_operand(R, d)
    ref = ei.gram_ref(R, ei.counts(d))
    assert ref[0, 0] == a * a * m and ref[0, 1] == -a * a * m and ref[0, 0] < ei.TWO24
    for name, got in _f32_sum_orders(X, X):
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), ref), name
    # one step beyond the condition the worst case is no longer representable
    big = (a + 1) * (a + 1) * m
    assert big >= ei.TWO24


def test_one_flipped_row_changes_every_reference():
    m, n, l = 100003, 20, 6
    R = ei.dictionary(61, n, 3)
    d = ei.row_map(m)
    d2 = d.copy()
    d2[77777] = (d2[77777] + 1) % 61
    assert np.any(ei.gram_ref(R, ei.counts(d)) != ei.gram_ref(R, ei.counts(d2)))
    RB, dB = ei.dictionary(53, 4, 2, seed=5), ei.row_map(m, 53, salt=9)
    assert np.any(ei.tn_ref(R, RB, ei.cooccurrence(d, dB, 61, 53)) != ei.tn_ref(R, RB, ei.cooccurrence(d2, dB, 61, 53)))
    W = np.random.RandomState(0).randint(-3, 4, size=(n, l)).astype(np.int64)
    Y = ei.skinny_ref(R, W)
    assert np.any(Y[d] != Y[d2]) and np.array_equal(np.nonzero(np.any(Y[d] != Y[d2], axis=1))[0], [77777])
    # a dropped row as well: the dictionary has no zero row, and its Gram contribution r r^T is non-zero
    c = ei.counts(d)
    c[d[-1]] -= 1
    assert np.any(ei.gram_ref(R, c) != ei.gram_ref(R, ei.counts(d)))


def _plant(X, i, j, v):
    Y = X.copy()
    Y[i, j] = v
    return Y


@pytest.mark.parametrize("v", [np.nan, np.inf, -np.inf])
def test_class_reference_agrees_with_the_cpu_kernel_double(v):
    rs = np.random.RandomState(7)
    X = rs.standard_normal((203, 9)).astype(np.float32)
    X[5, 2] = 0.0                                     # Inf * 0 = NaN in column 2
    B = rs.standard_normal((203, 4)).astype(np.float32)
    Xp = _plant(X, 5, 3, v)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.T))        # noqa: E731
    G = K.syrk(t(Xp)).numpy()
    cls = ei.tn_class_ref(Xp, Xp)
    assert np.array_equal(ei.value_class(G), cls)
    assert cls[3, 3] != ei.FINITE and np.all(cls[3, :] != ei.FINITE) and np.all(cls[:, 3] != ei.FINITE)
    touched = ei.touched_tn(Xp, Xp)
    assert np.array_equal(touched, cls != ei.FINITE)
    if not np.isnan(v):
        assert cls[3, 2] == ei.NAN and cls[3, 3] == ei.PINF
    Ct = K.gemm_tn(t(Xp), t(B)).numpy()              # (nb, na)
    assert np.array_equal(ei.value_class(Ct.T), ei.tn_class_ref(Xp, B))
    assert np.array_equal(ei.touched_tn(Xp, B), np.repeat((np.arange(9) == 3)[:, None], 4, axis=1))
    W = rs.standard_normal((9, 5)).astype(np.float32)
    Yt = K.skinny(t(Xp), t(W)).numpy()               # (l, m)
    cy = ei.nn_class_ref(Xp, W)
    assert np.array_equal(ei.value_class(Yt.T), cy)
    assert np.all(cy[5] != ei.FINITE) and np.all(np.delete(cy, 5, axis=0) == ei.FINITE)


def test_plus_and_minus_inf_in_one_column():
    """+Inf and -Inf in the same column: the diagonal entry is (+Inf)^2 + (-Inf)^2 = +Inf, the
    off-diagonal ones Inf - Inf = NaN where the partners have equal signs.  numpy fp64 says so, and
    the host's finiteness check of diag(G) catches either."""
    X = np.ones((50, 3), dtype=np.float32)
    X[3, 1], X[40, 1] = np.inf, -np.inf
    cls = ei.tn_class_ref(X, X)
    assert cls[1, 1] == ei.PINF and cls[1, 0] == ei.NAN and cls[0, 0] == ei.FINITE


def test_chain_bound_does_not_grow_with_K():
    assert ei.chain_bound_factor(4096) == ei.chain_bound_factor(1000003) == (2048 + 18) * 2.0 ** -24 * 1.01
    assert ei.chain_bound_factor(100) == (50 + 18) * 2.0 ** -24 * 1.01
