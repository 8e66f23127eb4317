"""CPU: formats.csr_spgemm, numpy's restatement of the contract of include/spgpu/ext/spgemm_device.h, which the GPU tests compare
bytes with.  Against a dense integer product on small random matrices (every type, both bases, A's rows shuffled and with repeated
columns, empty rows on both sides); its pattern against scipy's A @ B on strictly positive values (scipy drops sums that cancel, so
only there); and on hand-made rows the properties a dense product cannot show: the additions follow A's storage order, the product
is rounded before it is added, a complex product is six separately rounded operations, cancelled entries stay, and a lone -0.0
product is stored as +0.0."""
import math
from fractions import Fraction

import numpy as np
import pytest

from spgpu_amd import formats

DTYPES = {"S": np.float32, "D": np.float64, "C": np.complex64, "Z": np.complex128}


def random_csr(rng, n_rows, n_cols, longest, dtype, empty=(), ascending=True, repeats=False, integers=None, base=0):
    """(ptr, cols, vals) in `base`: rows of 0 .. longest distinct columns, none in the rows `empty`; ascending, or shuffled and, with
    `repeats`, with one column of every other row listed twice.  Values standard normal, or integers of magnitude <= `integers`."""
    dtype = np.dtype(dtype)
    ptr, cols = [0], []
    for r in range(n_rows):
        length = 0 if r in empty else int(rng.integers(0, min(longest, n_cols) + 1))
        row = np.sort(rng.choice(n_cols, length, replace=False))
        if not ascending:
            if repeats and r % 2 == 0 and length:
                row = np.append(row, row[rng.integers(0, length)])
            row = row[rng.permutation(row.size)]
        cols.append(row)
        ptr.append(ptr[-1] + row.size)
    cols = np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, np.int64)
    parts = 2 if dtype.kind == "c" else 1
    real = np.dtype("f%d" % (dtype.itemsize // parts))
    if integers is None:
        vals = rng.standard_normal(parts * cols.size).astype(real).view(dtype)
    else:
        vals = rng.integers(-integers, integers + 1, parts * cols.size).astype(real).view(dtype)
    return (np.asarray(ptr) + base).astype(np.int32), (cols + base).astype(np.int32), vals


def dense_of(ptr, cols, vals, n_cols, base=0):
    """The dense matrix, duplicates added, in complex128 (exact for small integers)."""
    ptr, cols = np.asarray(ptr, np.int64) - base, np.asarray(cols, np.int64) - base
    out = np.zeros((ptr.size - 1, n_cols), np.complex128)
    np.add.at(out, (np.repeat(np.arange(ptr.size - 1), np.diff(ptr)), cols), vals)
    return out


def stored_of(ptr, cols, n_cols, base=0):
    ptr, cols = np.asarray(ptr, np.int64) - base, np.asarray(cols, np.int64) - base
    out = np.zeros((ptr.size - 1, n_cols), bool)
    out[np.repeat(np.arange(ptr.size - 1), np.diff(ptr)), cols] = True
    return out


def csr(rows, dtype, base=0):
    """[(columns, values), ...] -> (ptr, cols, vals)."""
    ptr = np.cumsum([0] + [len(c) for c, _ in rows]) + base
    cols = np.concatenate([np.asarray(c, np.int64) for c, _ in rows] + [np.zeros(0, np.int64)]) + base
    vals = np.concatenate([np.asarray(v, dtype) for _, v in rows] + [np.zeros(0, dtype)])
    return ptr.astype(np.int32), cols.astype(np.int32), vals.astype(dtype)


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
def test_small_integer_products_equal_the_dense_product(letter, base):
    rng = np.random.default_rng(ord(letter) + base)
    dtype = DTYPES[letter]
    for n, k, m in ((1, 1, 1), (7, 5, 9), (30, 20, 40)):
        a = random_csr(rng, n, k, 6, dtype, empty=(0, n - 1) if n > 2 else (), ascending=False, repeats=True, integers=8, base=base)
        b = random_csr(rng, k, m, 7, dtype, empty=(1,) if k > 2 else (), integers=8, base=base)
        products, c_ptr, c_cols, c_vals = formats.csr_spgemm(*a, *b, m, base)
        assert c_ptr.dtype == np.int32 and c_cols.dtype == np.int32 and c_vals.dtype == dtype and c_ptr[0] == base
        lengths = np.diff(np.asarray(b[0], np.int64))
        assert products == int(lengths[np.asarray(a[1], np.int64) - base].sum())
        want = dense_of(*a, k, base) @ dense_of(*b, m, base)              # small integers: exact in any order
        assert np.array_equal(dense_of(c_ptr, c_cols, c_vals, m, base), want)
        symbolic = (stored_of(a[0], a[1], k, base).astype(np.int64) @ stored_of(b[0], b[1], m, base).astype(np.int64)) > 0
        assert np.array_equal(stored_of(c_ptr, c_cols, m, base), symbolic) and c_cols.size == int(symbolic.sum())
        for i in range(n):                                               # ascending and duplicate-free
            assert np.all(np.diff(c_cols[c_ptr[i] - base:c_ptr[i + 1] - base]) > 0)


def test_the_pattern_is_scipys_on_positive_values():
    import scipy.sparse as sp
    rng = np.random.default_rng(3)
    a_ptr, a_cols, a_vals = random_csr(rng, 60, 45, 9, np.float64, empty=(0, 17), ascending=False)
    b_ptr, b_cols, b_vals = random_csr(rng, 45, 80, 11, np.float64, empty=(3, 44))
    a_vals, b_vals = np.abs(a_vals) + 0.5, np.abs(b_vals) + 0.5
    _, c_ptr, c_cols, c_vals = formats.csr_spgemm(a_ptr, a_cols, a_vals, b_ptr, b_cols, b_vals, 80)
    ref = sp.csr_matrix((a_vals, a_cols, a_ptr), shape=(60, 45)) @ sp.csr_matrix((b_vals, b_cols, b_ptr), shape=(45, 80))
    ref.sum_duplicates()
    ref.sort_indices()
    assert np.array_equal(ref.indptr, c_ptr) and np.array_equal(ref.indices, c_cols)
    assert np.allclose(ref.data, c_vals, rtol=1e-13, atol=0)


def test_bad_input_is_an_error():
    ok = csr([([0, 1], [1.0, 2.0])], np.float64)
    b = csr([([0, 2], [1.0, 1.0]), ([1], [1.0])], np.float64)
    formats.csr_spgemm(*ok, *b, 3)
    with pytest.raises(ValueError):
        formats.csr_spgemm(*csr([([0, 2], [1.0, 2.0])], np.float64), *b, 3)                 # A names row 2 of a B with two rows
    with pytest.raises(ValueError):
        formats.csr_spgemm(*ok, *b, 2)                                                       # B's column 2 of 2
    with pytest.raises(ValueError):
        formats.csr_spgemm(*ok, *csr([([2, 0], [1.0, 1.0]), ([1], [1.0])], np.float64), 3)   # B's row descends
    with pytest.raises(ValueError):
        formats.csr_spgemm(*ok, *csr([([1, 1], [1.0, 1.0]), ([1], [1.0])], np.float64), 3)   # B's row repeats a column


@pytest.mark.parametrize("dtype,big", [(np.float64, 1e16), (np.float32, 1e8)])
def test_the_additions_follow_the_storage_order_of_as_row(dtype, big):
    """A's row stored as columns (5, 2, 9) with the terms big, 1, -big into one c(0, 0): ((0 + big) + 1) - big = 0 because big + 1
    rounds to big; stored as (5, 9, 2) the terms are big, -big, 1 and the sum is 1."""
    b = csr([([], [])] * 2 + [([0], [1.0])] + [([], [])] * 2 + [([0], [big])] + [([], [])] * 3 + [([0], [-big])], dtype)
    assert dtype(big) + dtype(1) == dtype(big)
    one = lambda cols: formats.csr_spgemm(*csr([(cols, [1.0, 1.0, 1.0])], dtype), *b, 1)
    assert one([5, 2, 9])[3].tolist() == [0.0] and one([5, 9, 2])[3].tolist() == [1.0] and one([2, 5, 9])[3].tolist() == [0.0]
    assert one([5, 2, 9])[0] == 3


def inexact_pair(rng, dtype):
    """(a, b) of `dtype` whose product is not representable, with the rounded product p and the error a * b - p, which is."""
    dtype = np.dtype(dtype).type
    while True:
        a, b = dtype(1 + rng.random()), dtype(1 + rng.random())
        p = dtype(a * b)
        error = Fraction(float(a)) * Fraction(float(b)) - Fraction(float(p))
        if error != 0:
            assert Fraction(float(dtype(float(error)))) == error
            return a, b, p, dtype(float(error))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_product_is_rounded_before_it_is_added(dtype):
    """c = (0 + 1 * s) + a * b with s = -round(a * b): rounded separately the sum is exactly 0; one fused multiply-add would give the
    rounding error of the product, which is not 0."""
    rng = np.random.default_rng(11)
    for _ in range(20):
        a, b, p, error = inexact_pair(rng, dtype)
        if dtype is np.float64 and hasattr(math, "fma"):
            assert math.fma(float(a), float(b), -float(p)) == float(error)
        c = formats.csr_spgemm(*csr([([0, 1], [1.0, a])], dtype), *csr([([0], [-p]), ([0], [b])], dtype), 1)[3]
        assert c.dtype == dtype and c.tolist() == [0.0] and error != 0


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_a_complex_product_is_six_separately_rounded_operations(dtype):
    """re = ar*br - ai*bi with ai*bi = round(ar*br) exactly (bi = 1), and the mirror image with ar*br = round(ai*bi): both real parts
    are exactly 0 only if neither product is fused into the subtraction.  im = ar*bi + ai*br likewise with ai*br = -round(ar*bi)."""
    part = np.float32 if dtype is np.complex64 else np.float64
    rng = np.random.default_rng(12)
    for _ in range(20):
        x, y, p, error = inexact_pair(rng, part)
        for a, b in ((complex(x, p), complex(y, 1)), (complex(p, x), complex(1, y))):
            c = formats.csr_spgemm(*csr([([0], [a])], dtype), *csr([([0], [b])], dtype), 1)[3]
            assert c.dtype == dtype and c[0].real == 0.0 and not np.signbit(c[0].real)
        c = formats.csr_spgemm(*csr([([0], [complex(x, -p)])], dtype), *csr([([0], [complex(1, y)])], dtype), 1)[3]
        assert c[0].imag == 0.0 and float(error) != 0.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_cancelled_entries_stay_and_a_lone_negative_zero_becomes_positive(dtype):
    a = csr([([0, 1], [1.0, 1.0]), ([2], [-1.0])], dtype)
    b = csr([([0, 3], [2.5, 1.0]), ([0], [-2.5]), ([1], [0.0])], dtype)
    products, c_ptr, c_cols, c_vals = formats.csr_spgemm(*a, *b, 4)
    assert products == 4 and c_ptr.tolist() == [0, 2, 3] and c_cols.tolist() == [0, 3, 1]
    assert c_vals[0] == 0 and c_vals[1] == 1                                  # +x and -x: the entry stays, value 0
    assert np.signbit(np.asarray(-1.0, dtype).real * np.asarray(0.0, dtype).real)      # the lone product is -0.0 ...
    assert c_vals[2] == 0 and not np.signbit(c_vals[2].real)                  # ... and 0 + -0.0 is +0.0
    assert c_vals.view(np.uint8).tolist()[-c_vals.itemsize:] == [0] * c_vals.itemsize
