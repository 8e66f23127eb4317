"""CPU: spgpu_amd.formats.csr_trsv_plan and csr_trsv, numpy's restatement of include/spgpu/ext/trsv_device.h that the GPU tests
compare bytes with, checked on its own: against the dense substitution where every operation is exact, against scipy where it
imports, against closed-form levels, and on each detail of the contract that a different order or a fused operation would change."""
from fractions import Fraction

import numpy as np
import pytest

import exact_ref as X
import trsv_cases as T
from spgpu_amd import capi, formats
from test_spgemm_restated import inexact_pair
from trsv_cases import LOWER, STORED, UNIT, UPPER


def test_the_constants_are_the_librarys():
    assert (LOWER, UPPER, STORED, UNIT) == (capi.TRSV_LOWER, capi.TRSV_UPPER, capi.TRSV_DIAG_STORED, capi.TRSV_DIAG_UNIT)


def _dense(mat, n, base):
    ptr, cols, vals = mat
    out = np.zeros((n, n), np.complex128)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    out[rows, cols.astype(np.int64) - base] = vals
    return out


def _as(dtype, a):
    """complex128 -> dtype; for a real dtype the (zero) imaginary parts are dropped on purpose."""
    a = np.asarray(a, np.complex128)
    return a.astype(dtype) if np.dtype(dtype).kind == "c" else a.real.astype(dtype)


def _dense_solve(dense, b, side, diag):
    """Substitution on the dense triangle in complex128."""
    n = b.size
    x = np.zeros(n, np.complex128)
    for i in (range(n) if side == LOWER else range(n - 1, -1, -1)):
        js = np.arange(0, i) if side == LOWER else np.arange(i + 1, n)
        acc = b[i] - dense[i, js] @ x[js]
        x[i] = acc if diag == UNIT else acc / dense[i, i]
    return x


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("side", [LOWER, UPPER])
@pytest.mark.parametrize("diag", [STORED, UNIT])
def test_small_integer_systems_equal_the_dense_solve(letter, base, side, diag):
    """Off-diagonals in {-2, .., 2} (complex: Gaussian integers), at most two per row on the side, diagonals 1 or 2, six rows: every
    product, difference and quotient is a dyadic number of fewer than 24 bits, so each rounding is exact and the comparison is ==."""
    dtype = X.DTYPE_OF[letter]
    rng = np.random.default_rng(10 * ord(letter) + 4 * base + 2 * side + diag)
    n = 6
    for _ in range(5):
        rows = []
        for i in range(n):
            pool = np.arange(0, i) if side == LOWER else np.arange(i + 1, n)
            other = np.arange(i + 1, n) if side == LOWER else np.arange(0, i)
            cols = list(rng.choice(pool, min(2, pool.size), replace=False)) + list(rng.choice(other, min(1, other.size), replace=False))
            vals = [complex(rng.integers(-2, 3), rng.integers(-2, 3) if letter in "CZ" else 0) for _ in cols]
            if diag == STORED or i % 2:
                cols.append(i)
                vals.append(complex(rng.choice([1.0, 2.0])))
            order = rng.permutation(len(cols))
            rows.append((np.asarray(cols, np.int64)[order], _as(dtype, vals)[order]))
        mat = T.from_rows(rows, letter, base)
        b = _as(dtype, [complex(rng.integers(-3, 4), rng.integers(-3, 4) if letter in "CZ" else 0) for _ in range(n)])
        want = _dense_solve(_dense(mat, n, base), b.astype(np.complex128), side, diag)
        assert np.array_equal(_as(dtype, want).astype(np.complex128), want)          # representable: nothing was rounded
        got = formats.csr_trsv(*mat, b, base, side, diag)
        assert got.dtype == dtype and np.array_equal(got.astype(np.complex128), want)
        assert np.abs(want).max() > 0


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("side", [LOWER, UPPER])
def test_random_systems_agree_with_scipy_within_the_bound_of_substitution(letter, side):
    """Higham, Accuracy and Stability of Numerical Algorithms, Theorem 8.5: the computed solution solves (T + dT) x = b with
    |dT| <= gamma_k |T|, k - 1 the entries of the longest row and gamma_k = k u / (1 - k u), hence the forward error is at most
    cond gamma_k / (1 - cond gamma_k) relative to |x|_inf, where cond <= | |T^-1| |T| |_inf.  For a row-dominant T with
    rho = max_i sum_j |t_ij| / |t_ii| < 1 the comparison matrix gives |T^-1| <= M(T)^-1, so cond <= (max |t_ii| / min |t_ii|) *
    (1 + rho) / (1 - rho).  A complex operation costs at most 2 sqrt(2) u (ibid. Lemma 3.5) and the textbook quotient a few more: 8 u
    covers each.  scipy solves the same system in double precision, which for the single types is exact by comparison."""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.linalg import spsolve_triangular
    dtype = X.DTYPE_OF[letter]
    rng = np.random.default_rng(77 + ord(letter) + side)
    n = 200
    mat, b = T.random_system(rng, n, letter, 0, side, STORED, longest=9, poison=False)
    ptr, cols, vals = mat
    wide = np.complex128 if letter in "CZ" else np.float64
    whole = sp.csr_matrix((vals.astype(wide), cols, ptr), shape=(n, n))
    triangle = sp.csr_matrix(sp.tril(whole) if side == LOWER else sp.triu(whole))
    triangle.sort_indices()
    want = spsolve_triangular(triangle, b.astype(wide), lower=side == LOWER)
    got = formats.csr_trsv(ptr, cols, vals, b, 0, side, STORED)
    d = np.abs(triangle.diagonal())
    off = np.asarray(abs(triangle).sum(axis=1)).ravel() - d
    rho = float((off / d).max())
    assert rho < 1                                                                       # row-dominant: the derivation holds
    cond = float(d.max() / d.min()) * (1 + rho) / (1 - rho)
    k = int(np.diff(triangle.indptr).max()) + 1
    u = float(np.finfo(X.REAL_OF[letter]).eps) / 2 * (8 if letter in "CZ" else 1)
    gamma = k * u / (1 - k * u)
    margin = 2 * cond * gamma / (1 - cond * gamma)                                       # both solutions carry the error
    error = float(np.abs(got.astype(wide) - want).max() / np.abs(want).max())
    print(f"{letter} side {side}: error {error:.3e}, margin {margin:.3e}, cond <= {cond:.2f}, k = {k}")
    assert 0 < margin < 1e-2 and error <= margin


def test_the_levels_of_a_bidiagonal_a_diagonal_and_a_stencil_matrix_in_closed_form():
    rng = np.random.default_rng(5)
    for base in (0, 1):
        for side in (LOWER, UPPER):
            n = 37
            ptr, cols, _ = T.bidiagonal(n, "D", base, side, rng)
            levels, order, level_ptr = formats.csr_trsv_plan(ptr, cols, base, side, STORED)
            assert levels == n and level_ptr.tolist() == list(range(n + 1))
            assert order.tolist() == (list(range(n)) if side == LOWER else list(range(n - 1, -1, -1)))
            assert order.dtype == np.int32 and level_ptr.dtype == np.int32
            ptr, cols, _ = T.from_rows([([i], [1.0]) for i in range(n)], "D", base)
            for diag in (STORED, UNIT):
                assert formats.csr_trsv_plan(ptr, cols, base, side, diag)[0] == 1
            levels, order, level_ptr = formats.csr_trsv_plan(ptr, cols, base, side, STORED)
            assert order.tolist() == list(range(n)) and level_ptr.tolist() == [0, n]
            for g, dims in ((7, 2), (4, 3)):
                ptr, cols, _ = T.stencil(g, dims, "D", base)
                want = T.stencil_levels(g, dims, side)
                levels, order, level_ptr = formats.csr_trsv_plan(ptr, cols, base, side, STORED)
                assert levels == dims * (g - 1) + 1 and level_ptr[-1] == g ** dims
                assert order.tolist() == np.lexsort((np.arange(g ** dims), want)).tolist()
                assert np.diff(level_ptr).tolist() == np.bincount(want).tolist()
    assert formats.csr_trsv_plan(np.zeros(1, np.int32), np.zeros(0, np.int32))[0] == 0     # no rows: no levels
    # symbolic: a stored zero is a dependency
    ptr, cols, _ = T.from_rows([([0], [1.0]), ([1, 0], [1.0, 0.0])], "D")
    assert formats.csr_trsv_plan(ptr, cols, 0, LOWER, STORED)[0] == 2 and formats.csr_trsv_plan(ptr, cols, 0, UPPER, STORED)[0] == 1


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("side", [LOWER, UPPER])
@pytest.mark.parametrize("diag", [STORED, UNIT])
def test_what_the_solve_must_not_read_may_be_nan(letter, side, diag):
    rng = np.random.default_rng(31)
    clean, b = T.random_system(rng, 40, letter, 1, side, diag, poison=False)
    rng = np.random.default_rng(31)
    poisoned, b2 = T.random_system(rng, 40, letter, 1, side, diag, poison=True)
    assert np.isnan(poisoned[2]).any() and not np.isnan(clean[2]).any() and b.tobytes() == b2.tobytes()
    assert clean[0].tobytes() == poisoned[0].tobytes() and clean[1].tobytes() == poisoned[1].tobytes()
    want, got = formats.csr_trsv(*clean, b, 1, side, diag), formats.csr_trsv(*poisoned, b, 1, side, diag)
    assert want.tobytes() == got.tobytes() and not np.isnan(got).any()
    assert formats.csr_trsv_plan(clean[0], clean[1], 1, side, diag)[0] > 2


@pytest.mark.parametrize("dtype,big", [(np.float32, 1e8), (np.float64, 1e16)])
def test_the_subtractions_follow_the_storage_order(dtype, big):
    """b = big with the terms 1 and big: (big - 1) - big = 0 because big - 1 rounds to big; stored the other way round,
    (big - big) - 1 = -1."""
    letter = "S" if dtype == np.float32 else "D"
    assert dtype(big) - dtype(1) == dtype(big)
    b = np.array([1, big, big], dtype)
    one = lambda cols: formats.csr_trsv(*T.from_rows([([], []), ([], []), (cols, [1.0, 1.0])], letter), b, 0, LOWER, UNIT)
    assert one([0, 1]).tolist() == [1.0, big, 0.0] and one([1, 0]).tolist() == [1.0, big, -1.0]


@pytest.mark.parametrize("letter", "SD")
def test_the_product_is_rounded_before_it_is_subtracted(letter):
    """acc = p - (a * x) with p = round(a * x): exactly +0 when the product is rounded first, the rounding error from one fused
    multiply-add."""
    dtype = X.DTYPE_OF[letter]
    rng = np.random.default_rng(8)
    for _ in range(20):
        a, x, p, error = inexact_pair(rng, dtype)
        mat = T.from_rows([([], []), ([0], [a])], letter)
        got = formats.csr_trsv(*mat, np.array([x, p], dtype), 0, LOWER, UNIT)
        assert got[1] == 0 and not np.signbit(got[1]) and float(error) != 0
        assert Fraction(float(p)) - Fraction(float(a)) * Fraction(float(x)) == -Fraction(float(error))   # what the fused form gives


@pytest.mark.parametrize("letter", "CZ")
def test_the_complex_product_and_quotient_are_rounded_operation_by_operation(letter):
    dtype, real = X.DTYPE_OF[letter], X.REAL_OF[letter]
    rng = np.random.default_rng(9)
    for _ in range(20):
        s, t, p, error = inexact_pair(rng, real)
        # re = ar*xr - ai*xi with ai*xi = p (xi = 1): the real part of the product is round(s*t) - p = 0, so acc keeps b's real part
        mat = T.from_rows([([], []), ([0], [complex(s, p)])], letter)
        b = np.array([complex(t, 1), complex(3, 0)], dtype)
        got = formats.csr_trsv(*mat, b, 0, LOWER, UNIT)
        assert got[1].real == 3 and float(error) != 0
        # the quotient: n = (s, 0), d = (t, 0): re = round(round(s*t) / round(t*t)), not s / t
        mat = T.from_rows([([0], [complex(t, 0)])], letter)
        got = formats.csr_trsv(*mat, np.array([complex(s, 0)], dtype), 0, LOWER, STORED)
        assert got[0].real == real(real(s * t) / real(t * t)) and got[0].imag == 0


@pytest.mark.parametrize("letter", "SD")
def test_a_lone_negative_zero_keeps_its_bits_under_unit(letter):
    dtype = X.DTYPE_OF[letter]
    mat = T.from_rows([([], []), ([1], [np.nan]), ([], [])], letter)
    b = np.array([-0.0, -0.0, 0.0], dtype)
    for side in (LOWER, UPPER):
        got = formats.csr_trsv(*mat, b, 0, side, UNIT)
        assert got.tobytes() == b.tobytes() and np.signbit(got).tolist() == [True, True, False]


def test_one_correctly_rounded_division_and_a_zero_pivot_left_to_ieee():
    n, d = T.division_operands(np.random.default_rng(4), 16)
    for t in range(16):
        got = formats.csr_trsv(*T.from_rows([([0], [d[t]])], "S"), n[t:t + 1], 0, LOWER, STORED)
        assert got[0] == n[t] / d[t] != n[t] * (np.float32(1) / d[t])
    got = formats.csr_trsv(*T.from_rows([([0], [0.0]), ([1], [0.0])], "D"), np.array([1.0, 0.0]), 0, UPPER, STORED)
    assert np.isposinf(got[0]) and np.isnan(got[1])


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("side", [LOWER, UPPER])
def test_bad_input_is_an_error(base, side):
    good = T.from_rows([([0, 1], [2.0, 1.0]), ([1, 0], [2.0, 1.0]), ([2], [1.0])], "D", base)
    b = np.ones(3)
    formats.csr_trsv(*good, b, base, side, STORED)

    def refused(rows, diag):
        mat = T.from_rows(rows, "D", base)
        with pytest.raises(ValueError):
            formats.csr_trsv_plan(mat[0], mat[1], base, side, diag)
        with pytest.raises(ValueError):
            formats.csr_trsv(*mat, b, base, side, diag)

    for diag in (STORED, UNIT):
        refused([([0, 3], [2.0, 1.0]), ([1], [2.0]), ([2], [1.0])], diag)                 # a column at base + rows
        refused([([0], [2.0]), ([1, -1], [2.0, 1.0]), ([2], [1.0])], diag)                # a column below the base
    refused([([0], [2.0]), ([0, 2], [1.0, 1.0]), ([2], [1.0])], STORED)                   # row 1 stores no diagonal
    refused([([0], [2.0]), ([1, 0, 1], [1.0, 1.0, 1.0]), ([2], [1.0])], STORED)           # row 1 stores it twice
    unit = T.from_rows([([0], [2.0]), ([1, 0, 1], [1.0, 1.0, 1.0]), ([], [])], "D", base)
    assert formats.csr_trsv_plan(unit[0], unit[1], base, side, UNIT)[0] == (2 if side == LOWER else 1)   # under UNIT neither matters
    for bad_side, bad_diag in ((2, STORED), (LOWER, 2)):
        with pytest.raises(ValueError):
            formats.csr_trsv_plan(good[0], good[1], base, bad_side, bad_diag)
