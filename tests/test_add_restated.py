"""CPU: formats.csr_add, numpy's restatement of the contract of include/spgpu/ext/add_device.h, which the GPU tests compare bytes
with.  Against the dense alpha * A + beta * B on small integers (every type, both bases, empty rows on either side and on both); the
pattern as the union, cancelled entries included; and on hand-made rows what a dense sum cannot show: a lone entry is its product
alone (-0.0 keeps its sign for the real types), each product is rounded before the sum, a complex product is six separately rounded
operations, and everything the Plan refuses is a ValueError."""
import math

import numpy as np
import pytest

from spgpu_amd import formats
from test_spgemm_restated import csr, dense_of, inexact_pair, random_csr, stored_of

DTYPES = {"S": np.float32, "D": np.float64, "C": np.complex64, "Z": np.complex128}


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
def test_small_integer_sums_equal_the_dense_sum(letter, base):
    rng = np.random.default_rng(ord(letter) + base)
    dtype = DTYPES[letter]
    alpha, beta = (3, -2) if letter in "SD" else (complex(2, -1), complex(-1, 3))
    for n, m in ((1, 1), (7, 9), (30, 40)):
        a = random_csr(rng, n, m, 6, dtype, empty=(0, n - 1) if n > 2 else (), integers=8, base=base)
        b = random_csr(rng, n, m, 7, dtype, empty=(1, n - 1) if n > 2 else (), integers=8, base=base)
        c_ptr, c_cols, c_vals = formats.csr_add(*a, *b, m, alpha, beta, base)
        assert c_ptr.dtype == np.int32 and c_cols.dtype == np.int32 and c_vals.dtype == dtype and c_ptr[0] == base
        want = alpha * dense_of(*a, m, base) + beta * dense_of(*b, m, base)          # small integers: exact
        assert np.array_equal(dense_of(c_ptr, c_cols, c_vals, m, base), want)
        union = stored_of(a[0], a[1], m, base) | stored_of(b[0], b[1], m, base)
        assert np.array_equal(stored_of(c_ptr, c_cols, m, base), union) and c_cols.size == int(union.sum()) == c_ptr[-1] - base
        for i in range(n):                                                          # ascending and duplicate-free
            assert np.all(np.diff(c_cols[c_ptr[i] - base:c_ptr[i + 1] - base]) > 0)
        if n > 2:
            assert c_ptr[n] == c_ptr[n - 1]                                          # empty in both


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_the_pattern_is_the_union_and_keeps_cancelled_entries(dtype):
    a = csr([([0, 2, 5], [1.5, 2.0, -4.0]), ([], []), ([1], [7.0]), ([], [])], dtype)
    b = csr([([2, 3, 5], [-1.0, 3.0, 2.0]), ([4], [1.0]), ([], []), ([], [])], dtype)
    c_ptr, c_cols, c_vals = formats.csr_add(*a, *b, 6, 1, 2)
    assert c_ptr.tolist() == [0, 4, 5, 6, 6] and c_cols.tolist() == [0, 2, 3, 5, 4, 1]
    assert c_vals.tolist() == [1.5, 0.0, 6.0, 0.0, 2.0, 7.0]                         # 2 - 2 and -4 + 4: the entries stay, value 0
    assert not np.signbit(c_vals[[1, 3]].real).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_lone_entry_is_its_product_alone_and_keeps_a_negative_zero(dtype):
    a = csr([([0, 1, 2], [-0.0, 0.0, -0.0])], dtype)
    b = csr([([2, 3], [0.0, -0.0])], dtype)
    _, c_cols, c_vals = formats.csr_add(*a, *b, 4, 1, 1)
    assert c_cols.tolist() == [0, 1, 2, 3]
    assert np.signbit(c_vals).tolist() == [True, False, False, True]                 # alone, alone, -0.0 + 0.0 = +0.0, alone
    assert c_vals[[0, 1]].tobytes() == a[2][:2].tobytes() and c_vals[3:].tobytes() == b[2][1:].tobytes()
    _, _, flipped = formats.csr_add(*a, *b, 4, -1, 1)
    assert np.signbit(flipped).tolist() == [False, True, False, True]                # -1 * -0.0 = +0.0; 0.0 + 0.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_each_product_is_rounded_before_the_sum(dtype):
    """c = alpha * a + beta * b with beta * b = -round(alpha * a) (beta = 1): rounded separately the sum is exactly 0; a fused
    multiply-add would leave the rounding error of the product, which is not 0.  And mirrored, with alpha = 1 and the inexact product
    on B's side."""
    rng = np.random.default_rng(21)
    for _ in range(20):
        s, v, p, error = inexact_pair(rng, dtype)
        if dtype is np.float64 and hasattr(math, "fma"):
            assert math.fma(float(s), float(v), -float(p)) == float(error)
        c = formats.csr_add(*csr([([0], [v])], dtype), *csr([([0], [-p])], dtype), 1, s, 1)[2]
        assert c.dtype == dtype and c.tolist() == [0.0] and error != 0
        c = formats.csr_add(*csr([([0], [-p])], dtype), *csr([([0], [v])], dtype), 1, 1, s)[2]
        assert c.tolist() == [0.0]


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_a_complex_product_is_six_separately_rounded_operations(dtype):
    """re = sr*vr - si*vi with si*vi = round(sr*vr) exactly (vi = 1), and the mirror image with sr*vr = round(si*vi): both real parts
    are exactly 0 only if neither product is fused into the subtraction.  im = sr*vi + si*vr likewise with si*vr = -round(sr*vi).
    On a lone entry, on A's side and on B's."""
    part = np.float32 if dtype is np.complex64 else np.float64
    rng = np.random.default_rng(22)
    nothing = csr([([], [])], dtype)
    for _ in range(20):
        x, y, p, error = inexact_pair(rng, part)
        for s, v in ((complex(x, p), complex(y, 1)), (complex(p, x), complex(1, y))):
            for c in (formats.csr_add(*csr([([0], [v])], dtype), *nothing, 1, s, 1)[2], formats.csr_add(*nothing, *csr([([0], [v])], dtype), 1, 1, s)[2]):
                assert c.dtype == dtype and c[0].real == 0.0 and not np.signbit(c[0].real) and c[0].imag != 0
        c = formats.csr_add(*csr([([0], [complex(1, y)])], dtype), *nothing, 1, complex(x, -p), 1)[2]
        assert c[0].imag == 0.0 and float(error) != 0.0
        # both present: the sum is componentwise, of two products rounded like that
        c = formats.csr_add(*csr([([0], [complex(y, 1)])], dtype), *csr([([0], [complex(2, 3)])], dtype), 1, complex(x, p), 1)[2]
        assert type(p * y) is part and c[0].real == 2.0 and c[0].imag == (x + p * y) + part(3)


def test_bad_input_is_an_error():
    a = csr([([0, 2], [1.0, 2.0]), ([1], [1.0])], np.float64)
    b = csr([([1, 2], [1.0, 1.0]), ([], [])], np.float64)
    assert formats.csr_add(*a, *b, 3, 1, 1)[1].tolist() == [0, 1, 2, 1]
    bad = lambda rows: csr(rows, np.float64)
    for broken in (bad([([0, 3], [1.0, 2.0]), ([1], [1.0])]),          # column 3 of 3
                   bad([([-1, 2], [1.0, 2.0]), ([1], [1.0])]),         # a column below the base
                   bad([([2, 0], [1.0, 2.0]), ([1], [1.0])]),          # the row descends
                   bad([([2, 2], [1.0, 2.0]), ([1], [1.0])])):         # the row repeats a column
        with pytest.raises(ValueError):
            formats.csr_add(*broken, *b, 3, 1, 1)                      # in A
        with pytest.raises(ValueError):
            formats.csr_add(*a, *broken, 3, 1, 1)                      # in B
    with pytest.raises(ValueError):
        formats.csr_add(*a, *csr([([0], [1.0])], np.float64), 3, 1, 1)                                 # one row against two
    with pytest.raises(ValueError):
        formats.csr_add(*a, *csr([([1, 2], [1.0, 1.0]), ([], [])], np.float32), 3, 1, 1)                # two types
    with pytest.raises(ValueError):
        formats.csr_add(*csr([([1], [1.0])], np.float64, 1), *csr([([-1], [1.0])], np.float64, 1), 3, 1, 1, 1)  # column 0 in base 1
    with pytest.raises(ValueError):
        formats.csr_add(*csr([([1], [1.0])], np.float64, 1), *csr([([3], [1.0])], np.float64, 1), 3, 1, 1, 1)   # column 4 of 3, base 1
    assert formats.csr_add(*csr([([1], [1.0])], np.float64, 1), *csr([([2], [1.0])], np.float64, 1), 3, 1, 1, 1)[1].tolist() == [2, 3]
    # a row's last column may be larger than the next row's first: only a row's own order counts
    assert formats.csr_add(*csr([([2], [1.0]), ([0], [1.0])], np.float64), *b, 3, 1, 1)[1].tolist() == [1, 2, 0]
