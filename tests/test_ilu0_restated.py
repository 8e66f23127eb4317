"""CPU: spgpu_amd.formats.csr_ilu0_plan and csr_ilu0, numpy's restatement of include/spgpu/ext/ilu0_device.h that the GPU tests compare
bytes with, checked on its own: against a right-looking masked dense elimination written here (the same update sequence per entry, so
the bytes are equal), against A = L U within the bound of Gaussian elimination on patterns without fill, on each detail of the
contract that a different order or a fused operation would change, and the generators of tests/ilu0_cases.py on what they promise."""
import numpy as np
import pytest

import exact_ref as X
import ilu0_cases as I
import trsv_cases as T
from spgpu_amd import capi, formats


# ---- an elimination of its own: k outermost, on dense arrays with a mask, in the type's own scalar arithmetic ----------------
def _quotient(n, d, real):
    if real:
        return n / d
    (nr, ni), (dr, di) = n, d
    rr, ii = dr * dr, di * di
    den = rr + ii
    a, b, c, e = nr * dr, ni * di, ni * dr, nr * di
    top, bottom = a + b, c - e
    return np.array([top / den, bottom / den])


def _minus_product(acc, a, x, real):
    if real:
        product = a * x
        return acc - product
    (ar, ai), (xr, xi) = a, x
    rr, ii, ri, ir = ar * xr, ai * xi, ar * xi, ai * xr
    re, im = rr - ii, ri + ir
    return np.array([acc[0] - re, acc[1] - im])


def right_looking(mat, base):
    """After step k column k of L and row k of U are final: every (i, j) with i, j > k gets its k-th update, in ascending k."""
    dense, mask = I.dense_of(mat, base)
    n = dense.shape[0]
    real = dense.dtype.kind != "c"
    part = dense.dtype if real else np.dtype("f%d" % (dense.dtype.itemsize // 2))
    lu = dense.view(part).reshape(n, n, -1).copy() if not real else dense.copy()
    with np.errstate(all="ignore"):
        for k in range(n):
            for i in range(k + 1, n):
                if not mask[i, k]:
                    continue
                lu[i, k] = _quotient(lu[i, k], lu[k, k], real)
                for j in range(k + 1, n):
                    if mask[k, j] and mask[i, j]:
                        lu[i, j] = _minus_product(lu[i, j], lu[i, k], lu[k, j], real)
    out = lu if real else np.ascontiguousarray(lu).view(dense.dtype).reshape(n, n)
    return out[mask]                                                         # row-major: the CSR order of ascending rows


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
def test_the_restatement_gives_the_bytes_of_a_right_looking_elimination(letter, base):
    rng = np.random.default_rng(3 * ord(letter) + base)
    for mat in (I.random_system(rng, 40, letter, base), I.stencil(rng, 5, 2, letter, base), I.dense_block(rng, 9, letter, base),
                I.from_levels(rng, [3, 5, 2, 6], letter, base)[0], I.rows_around(rng, 2, letter, base)):
        got = formats.csr_ilu0(*mat, base)
        assert got.dtype == mat[2].dtype and got.tobytes() == right_looking(mat, base).tobytes()
        assert got.tobytes() != mat[2].tobytes()


@pytest.mark.parametrize("letter", "SD")
@pytest.mark.parametrize("name", ["tridiagonal", "block", "arrow"])
def test_without_fill_the_factor_is_the_lu(letter, name):
    """Higham, Accuracy and Stability of Numerical Algorithms, Theorem 9.3: the computed factors satisfy
    |A - L U| <= gamma_n |L| |U| elementwise, gamma_n = n u / (1 - n u).  On a pattern without fill ILU(0) drops nothing, so it is
    that elimination.  Evaluated in fp64 for both types."""
    rng = np.random.default_rng(40 + ord(letter))
    mat = {"tridiagonal": lambda: I.tridiagonal(rng, 300, letter), "block": lambda: I.dense_block(rng, 12, letter),
           "arrow": lambda: I.arrow(rng, 50, letter)}[name]()
    n = mat[0].size - 1
    assert I.update_counts(mat[0], mat[1])[1] == 0                                          # nothing is dropped: no fill
    a, _ = I.dense_of(mat)
    lu, _ = I.dense_of((mat[0], mat[1], formats.csr_ilu0(*mat)))
    lower, upper = np.tril(lu.astype(np.float64), -1) + np.eye(n), np.triu(lu.astype(np.float64))
    u = float(np.finfo(X.REAL_OF[letter]).eps) / 2
    gamma = n * u / (1 - n * u)
    residual = np.abs(a.astype(np.float64) - lower @ upper)
    bound = gamma * (np.abs(lower) @ np.abs(upper))
    print(f"{letter} {name}: largest residual {residual.max():.3e}, largest ratio to the bound {(residual / np.maximum(bound, 1e-300)).max():.3e}")
    assert residual.max() > 0 and np.all(residual <= bound)


def test_the_plan_is_the_lower_solves_plus_the_diagonal_positions():
    rng = np.random.default_rng(6)
    for base in (0, 1):
        mat, level = I.from_levels(rng, [4, 1, 7, 2], "D", base)
        levels, order, level_ptr, diag_pos = formats.csr_ilu0_plan(mat[0], mat[1], base)
        want = formats.csr_trsv_plan(mat[0], mat[1], base, capi.TRSV_LOWER, capi.TRSV_DIAG_STORED)
        assert levels == want[0] == 4 and order.tobytes() == want[1].tobytes() and level_ptr.tobytes() == want[2].tobytes()
        unit = formats.csr_trsv_plan(mat[0], mat[1], base, capi.TRSV_LOWER, capi.TRSV_DIAG_UNIT)      # the L solve reuses the arrays
        assert unit[0] == levels and unit[1].tobytes() == order.tobytes() and unit[2].tobytes() == level_ptr.tobytes()
        assert np.diff(level_ptr).tolist() == [4, 1, 7, 2] and np.array_equal(level[order], np.repeat(np.arange(4), [4, 1, 7, 2]))
        assert diag_pos.dtype == np.int32 and np.array_equal(mat[1][diag_pos] - base, np.arange(14))
    assert formats.csr_ilu0_plan(np.zeros(1, np.int32), np.zeros(0, np.int32))[0] == 0
    assert formats.csr_ilu0(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)).size == 0


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
def test_the_random_systems_hit_and_drop(letter, base):
    """What tests/test_gpu_zz_ilu0_device.py runs: the share of dropped updates is neither 0 nor 1."""
    rng = np.random.default_rng(200 + ord(letter) + base)
    ptr, cols, vals = I.random_system(rng, 70, letter, base)
    hit, dropped = I.update_counts(ptr, cols, base)
    assert hit > 0 and dropped > 0
    assert np.diff(ptr).max() <= 7 and np.all(np.diff(ptr) >= 1)
    formats.csr_ilu0_plan(ptr, cols, base)


def test_the_generators_keep_their_promises():
    rng = np.random.default_rng(12)
    for L in (2, 8, 32):
        ptr, cols, _ = I.rows_around(rng, L, "D")
        lengths = np.diff(ptr)
        assert {L - 1, L, L + 1, 2 * L + 1} <= set(lengths.tolist()) and lengths[0] == 1
        assert lengths[1] == 2 and cols[ptr[1]] == 0                                        # row 1: an empty upper part ...
        diag_pos = formats.csr_ilu0_plan(ptr, cols)[3]
        assert (cols[ptr[:-1]] == 1).sum() >= 4                                             # ... that long rows depend on
        no_lower, no_upper = diag_pos == ptr[:-1], diag_pos == ptr[1:] - 1
        assert (no_lower & (lengths > L)).any() and (no_upper & (lengths > L)).any()
        hit, dropped = I.update_counts(ptr, cols)
        assert hit > 0 and dropped > 0
    ptr, cols, _ = I.dense_block(rng, 40, "D")
    hit, dropped = I.update_counts(ptr, cols)
    assert dropped == 0 and hit == sum((40 - 1 - k) * (40 - 1 - k) for k in range(40))
    assert I.update_counts(*I.bidiagonal(rng, 30, "D")[:2]) == (0, 0)
    assert formats.csr_ilu0_plan(*I.bidiagonal(rng, 30, "D", 1)[:2], 1)[0] == 30
    for g, dims in ((16, 2), (8, 3)):
        hit, dropped = I.update_counts(*I.stencil(rng, g, dims, "D")[:2])
        assert hit > 0 and dropped > 0


# ---- the details of the contract ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SD")
def test_the_product_is_rounded_before_it_is_subtracted(letter):
    mat = I.fused_update_blocks(np.random.default_rng(8), letter, 20)
    lu = formats.csr_ilu0(*mat)
    assert np.all(lu[3::4] == 0) and not np.signbit(lu[3::4]).any()
    assert lu[0::4].tobytes() == mat[2][0::4].tobytes() and lu[2::4].tobytes() == mat[2][2::4].tobytes()   # l / 1 = l


@pytest.mark.parametrize("letter", "CZ")
def test_each_fused_multiply_add_inside_the_complex_product_would_change_the_update(letter):
    """Every block of the pin aims at one of the four multiplies of the product.  Emulated with exact fractions, fusing that multiply
    into the add or subtract behind it changes the component the block watches from 0 to the product's rounding error; the
    restatement gives the 0."""
    real = X.REAL_OF[letter]
    mat, aims = I.fused_complex_product_blocks(np.random.default_rng(9), letter)
    lu = formats.csr_ilu0(*mat)
    assert {fusion for _, _, fusion, _ in aims} == set(I.PRODUCT_FUSIONS)
    for t, (l, u, fusion, zero) in enumerate(aims):
        at = 0 if zero == "real" else 1
        plain, fused = I.complex_product(l, u, real), I.complex_product(l, u, real, fusion)
        assert plain[at] == 0 and fused[at] != 0, (t, fusion)
        assert lu[4 * t + 2] == mat[2][4 * t + 2]                                             # the multiplier is l exactly
        got = lu[4 * t + 3]
        assert (got.real, got.imag)[at] == 0 and (got.real, got.imag) == (real(0) - plain[0], real(0) - plain[1]), (t, fusion)


@pytest.mark.parametrize("letter", "CZ")
def test_each_fused_multiply_add_inside_the_complex_quotient_would_change_the_multiplier(letter):
    """The same for the six multiplies of the quotient: four blocks in six watch a numerator that is 0 only unfused, two were drawn
    until the fused sum of squares changes a byte of the quotient."""
    real = X.REAL_OF[letter]
    mat, aims = I.complex_quotient_blocks(np.random.default_rng(10), letter)
    lu = formats.csr_ilu0(*mat)
    assert {fusion for _, _, fusion, _ in aims} == set(I.QUOTIENT_FUSIONS)
    for t, (l, d, fusion, zero) in enumerate(aims):
        plain, fused = I.complex_quotient(l, d, real), I.complex_quotient(l, d, real, fusion)
        got = lu[4 * t + 2]
        assert (got.real, got.imag) == plain and fused != plain, (t, fusion)
        if zero:
            at = 0 if zero == "real" else 1
            assert plain[at] == 0 and fused[at] != 0, (t, fusion)


def test_the_emulated_fused_multiply_add_rounds_once_to_nearest_even():
    from fractions import Fraction
    for real in (np.float32, np.float64):
        eps = float(np.finfo(real).eps)
        assert I.rounded(Fraction(1) + Fraction(eps) / 2, real) == 1 and I.rounded(Fraction(1) + Fraction(eps) * 3 / 2, real) == real(1 + 2 * eps)
        assert I.rounded(Fraction(1) + Fraction(eps) * 3 / 4, real) == real(1 + eps) and I.rounded(Fraction(-3, 8), real) == real(-0.375)
        a = real(1 + eps)
        assert I.fma(a, a, -real(a * a), real) == real(eps * eps) and real(a * a) - real(a * a) == 0     # the error of a product, exactly


def test_one_correctly_rounded_division_and_a_zero_pivot_left_to_ieee():
    mat, n, d = I.division_blocks(np.random.default_rng(4), 16)
    lu = formats.csr_ilu0(*mat)
    assert np.all(lu[2::4] == n / d) and np.all(lu[2::4] != n * (np.float32(1) / d))
    lu = formats.csr_ilu0(*T.from_rows([([0, 1], [0.0, 1.0]), ([0, 1], [1.0, 1.0])], "D"))
    assert lu.tolist()[:2] == [0.0, 1.0] and np.isposinf(lu[2]) and np.isneginf(lu[3])
    lu = formats.csr_ilu0(*T.from_rows([([0, 1], [0.0, 1.0]), ([0, 1], [0.0, 1.0])], "D"))
    assert np.isnan(lu[2]) and np.isnan(lu[3])


@pytest.mark.parametrize("letter,big", [("S", 1e8), ("D", 1e16)])
def test_the_updates_of_one_entry_arrive_in_ascending_k(letter, big):
    dtype = X.DTYPE_OF[letter]
    assert dtype(big) - dtype(1) == dtype(big)
    assert formats.csr_ilu0(*I.cancellation(letter, big, big_first=False))[-1] == 0.0       # (big - 1) - big
    assert formats.csr_ilu0(*I.cancellation(letter, big, big_first=True))[-1] == -1.0       # (big - big) - 1


@pytest.mark.parametrize("letter", "SD")
def test_a_row_without_lower_entries_keeps_its_bits(letter):
    mat = I.lone_negative_zero(letter)
    lu = formats.csr_ilu0(*mat)
    assert lu.tobytes() == mat[2].tobytes() and np.signbit(lu).tolist() == [True, True, True, False]


@pytest.mark.parametrize("base", [0, 1])
def test_bad_input_is_an_error(base):
    good = T.from_rows([([0, 1], [2.0, 1.0]), ([0, 1], [1.0, 2.0]), ([2], [1.0])], "D", base)
    formats.csr_ilu0(*good, base)

    def refused(rows):
        mat = T.from_rows(rows, "D", base)
        with pytest.raises(ValueError):
            formats.csr_ilu0_plan(mat[0], mat[1], base)
        with pytest.raises(ValueError):
            formats.csr_ilu0(*mat, base)

    refused([([0, 3], [2.0, 1.0]), ([1], [2.0]), ([2], [1.0])])                            # a column at base + rows
    refused([([-1, 0], [2.0, 1.0]), ([1], [2.0]), ([2], [1.0])])                           # a column below the base
    refused([([0], [2.0]), ([1, 0], [2.0, 1.0]), ([2], [1.0])])                            # row 1 descends
    refused([([0], [2.0]), ([0, 1, 1], [1.0, 1.0, 1.0]), ([2], [1.0])])                    # row 1 repeats a column
    refused([([0], [2.0]), ([0, 2], [1.0, 1.0]), ([2], [1.0])])                            # row 1 stores no diagonal
