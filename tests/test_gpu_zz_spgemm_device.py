"""GPU: the sparse product C = A * B on CSR arrays (include/spgpu/ext/spgemm_device.h).

Every output array -- cRowPtr, cColIndices, cValues -- and the scratch lie between 64 guard bytes, are poisoned as a whole with one
byte pattern, and the outputs must afterwards equal numpy's restatement of the contract (formats.csr_spgemm) BYTE FOR BYTE: the
number of products, the row pointers, the columns and the sums in the storage order of A's rows.  The fills run through the public
calls and through each of the two fills behind them (one thread per entry of C; a wavefront per row of C with the row's
accumulators in LDS), pattern + values and values only, on the whole grid and on a capped one: all must give the same bytes
(_multiply).  The values-only runs come after the scratch has been overwritten.  The matrices are the smallest at which each branch
of the analysis and of the staged fill can go wrong."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
from test_gpu_csr_device import _hell_plan, _p, _row_lengths, _zeros
from test_gpu_to_csr_device import _Guarded, _to_csr
from test_spgemm_restated import csr, dense_of, inexact_pair, random_csr

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


def _device(mat):
    """(ptr, cols, vals) -> the same as device tensors (an empty array as one element that nobody reads)."""
    from spgpu_amd import formats
    some = lambda a: a if a.size else np.zeros(1, a.dtype)
    return tuple(formats.to_device(some(np.ascontiguousarray(a))) for a in mat)


def _work(nbytes):
    """Scratch between guards, 256-byte aligned."""
    return _Guarded(nbytes, 192)


def _products(gpu, a, d_a, d_b, n_inner, base):
    """spgpuCsrSpgemmProductsDevice with the scratch of productsCount = 0: (status, productsCount)."""
    import torch
    from spgpu_amd import capi
    n_rows = a[0].size - 1
    small = _work(capi.spgpuCsrSpgemmWorkBytes(n_rows, 1, 0))
    count = C.c_int(-7)
    torch.cuda.synchronize()
    st = capi.spgpuCsrSpgemmProductsDevice(gpu, C.byref(count), n_rows, n_inner, _p(d_a[0]), _p(d_a[1]), _p(d_b[0]), base, small.ptr())
    torch.cuda.synchronize()
    assert small.guards_intact()
    return st, count.value


def _plan(gpu, a, d_a, d_b, n_inner, n_b_cols, base, products):
    """spgpuCsrSpgemmPlanDevice: (status, cNonZerosCount, cRowPtr as _Guarded, the scratch as _Guarded)."""
    import torch
    from spgpu_amd import capi
    n_rows = a[0].size - 1
    work = _work(capi.spgpuCsrSpgemmWorkBytes(n_rows, n_b_cols, products))
    row_ptr = _Guarded((n_rows + 1) * 4)
    entries = C.c_int(-7)
    torch.cuda.synchronize()
    st = capi.spgpuCsrSpgemmPlanDevice(gpu, C.byref(entries), row_ptr.ptr(), n_rows, n_inner, n_b_cols, _p(d_a[0]), _p(d_a[1]), _p(d_b[0]),
                                       _p(d_b[1]), base, products, work.ptr())
    torch.cuda.synchronize()
    assert row_ptr.guards_intact() and work.guards_intact()
    return st, entries.value, row_ptr, work


def _multiply(gpu, a, b, n_b_cols, letter, base=0, caps=(0,)):
    """Products, Plan and every fill on host CSR arrays given in `base`, everything against formats.csr_spgemm.  Returns the
    restated (products, c_ptr, c_cols, c_vals)."""
    import torch
    from spgpu_amd import capi, formats
    dtype = np.dtype(X.DTYPE_OF[letter])
    assert a[2].dtype == dtype and b[2].dtype == dtype
    n_rows, n_inner = a[0].size - 1, b[0].size - 1
    want = formats.csr_spgemm(*a, *b, n_b_cols, base)
    w_products, w_ptr, w_cols, w_vals = want
    case = (letter, n_rows, n_inner, n_b_cols, base)
    d_a, d_b = _device(a), _device(b)
    st, products = _products(gpu, a, d_a, d_b, n_inner, base)
    assert st == capi.SPGPU_SUCCESS and products == w_products, case
    st, entries, row_ptr, work = _plan(gpu, a, d_a, d_b, n_inner, n_b_cols, base, products)
    assert st == capi.SPGPU_SUCCESS and entries == w_cols.size, case
    assert row_ptr.numpy(np.int32).tobytes() == w_ptr.tobytes(), case
    code, size = capi.TYPE_CODE[letter], dtype.itemsize
    runs = [(None, 0)] + [(fill, cap) for fill in (capi.SPGEMM_FILL_PLAIN, capi.SPGEMM_FILL_STAGED) for cap in caps]
    d_cols = formats.to_device(w_cols if w_cols.size else np.zeros(1, np.int32))
    for what in ("full", "values"):
        if what == "values":
            work.buf[work.first:work.first + work.nbytes].fill_(0xFF)      # the values-only call never reads the scratch
        for fill, cap in runs:
            cols, vals = _Guarded(entries * 4), _Guarded(entries * size)
            torch.cuda.synchronize()
            if what == "full":
                args = (gpu, cols.ptr(), vals.ptr(), entries, n_rows, _p(d_a[0]), _p(d_a[1]), _p(d_a[2]), _p(d_b[0]), _p(d_b[1]), _p(d_b[2]),
                        row_ptr.ptr(), base, code, work.ptr())
                st = capi.spgpuCsrSpgemmDevice(*args) if fill is None else capi.spgpuCsrSpgemmDeviceWith(*args, fill, cap)
            else:
                args = (gpu, vals.ptr(), n_rows, _p(d_a[0]), _p(d_a[1]), _p(d_a[2]), _p(d_b[0]), _p(d_b[1]), _p(d_b[2]), row_ptr.ptr(),
                        _p(d_cols), base, code)
                st = capi.spgpuCsrSpgemmValuesDevice(*args) if fill is None else capi.spgpuCsrSpgemmValuesDeviceWith(*args, fill, cap)
            assert st == capi.SPGPU_SUCCESS, (case, what, fill, cap)
            torch.cuda.synchronize()
            assert cols.guards_intact() and vals.guards_intact() and row_ptr.guards_intact() and work.guards_intact(), (case, what, fill, cap)
            if what == "full":
                assert cols.numpy(np.int32).tobytes() == w_cols.tobytes(), (case, what, fill, cap)
            else:
                assert cols.untouched(), (case, fill, cap)
            assert vals.numpy(np.uint8).tobytes() == w_vals.tobytes(), (case, what, fill, cap)
    assert row_ptr.numpy(np.int32).tobytes() == w_ptr.tobytes() and d_cols.cpu().numpy()[:entries].tobytes() == w_cols.tobytes(), case
    return want


# ---- 1. every type x both bases: empty rows on both sides, A shuffled and with repeated columns --------------------------------
def _seventy_by_ninety(rng, letter, base):
    """A 70 x 50 with rows 0, 33 and 69 empty, shuffled, a column repeated in every other row, and row 5 naming only the empty rows of
    B; B 50 x 90 ascending with rows 3, 20 and 49 empty."""
    dtype = X.DTYPE_OF[letter]
    length = 0
    while length < 3:                                                    # row 5 needs three entries for the three empty rows
        a_ptr, a_cols, a_vals = random_csr(rng, 70, 50, 12, dtype, empty=(0, 33, 69), ascending=False, repeats=True, base=base)
        first, length = a_ptr[5] - base, a_ptr[6] - a_ptr[5]
    b = random_csr(rng, 50, 90, 14, dtype, empty=(3, 20, 49), base=base)
    a_cols[first:first + length] = np.resize(np.array([3, 20, 49, 20], np.int32) + base, length)
    return (a_ptr, a_cols, a_vals), b


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
def test_random_products_give_numpys_arrays(gpu, letter, base):
    rng = np.random.default_rng(100 + ord(letter))
    a, b = _seventy_by_ninety(rng, letter, base)
    products, c_ptr, c_cols, _ = _multiply(gpu, a, b, 90, letter, base, caps=(0, 1))
    lengths = np.diff(c_ptr)
    assert lengths[0] == lengths[5] == lengths[33] == lengths[69] == 0 and lengths.max() > 20 and products > c_cols.size
    assert a[0][6] - a[0][5] >= 3


# ---- 2. the grid-stride loops --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 255, 256, 257])
def test_row_counts_around_the_wavefront_and_the_workgroup_on_capped_grids(gpu, n_rows):
    rng = np.random.default_rng(n_rows)
    for letter in "SZ":
        a = random_csr(rng, n_rows, 40, 5, X.DTYPE_OF[letter], ascending=False, repeats=True)
        while a[1].size == 0:                                              # a single row: not an empty one
            a = random_csr(rng, n_rows, 40, 5, X.DTYPE_OF[letter], ascending=False, repeats=True)
        b = random_csr(rng, 40, 60, 6, X.DTYPE_OF[letter], empty=(7,))
        _multiply(gpu, a, b, 60, letter, 0, caps=(1, 2))


# ---- 3. rows of C around the staged fill's row cap -------------------------------------------------------------------------
def _rows_around_the_cap(rng, letter, cap):
    """B: for every length L in (cap - 1, cap, cap + 1, 3 cap) one long row of L columns and a row of 8 of those columns; blocks of 8
    consecutive columns; unit rows of one column.  A: for every L a row that names the long row (and the 8 columns inside it, so
    that some sums have two terms) and a
    row whose L columns are the union of L // 8 blocks and L % 8 unit rows, named in a shuffled order with two blocks named twice;
    short rows in between, so that every workgroup of four wavefronts has long and short rows."""
    dtype = X.DTYPE_OF[letter]
    lengths = (cap - 1, cap, cap + 1, 3 * cap)
    n_cols = 3 * cap + 40
    blocks = n_cols // 8
    rows_b = [(np.sort(rng.choice(n_cols, L, replace=False)), None) for L in lengths]
    rows_b += [(np.arange(8 * m, 8 * m + 8), None) for m in range(blocks)]
    rows_b += [(np.array([c]), None) for c in range(n_cols)]
    rows_b += [(rows_b[k][0][L // 4:L // 4 + 8], None) for k, L in enumerate(lengths)]
    long_row, block_row, unit_row = (lambda k: k), (lambda m: len(lengths) + m), (lambda c: len(lengths) + blocks + c)
    inside_row = lambda k: len(lengths) + blocks + n_cols + k
    rows_a = []
    for k, L in enumerate(lengths):
        rows_a.append([inside_row(k), long_row(k)])
        rows_a.append([block_row(int(rng.integers(0, blocks)))])
        named = [block_row(m) for m in range(L // 8)] + [unit_row(8 * (L // 8) + c) for c in range(L % 8)] + [block_row(0), block_row(L // 16)]
        rows_a.append([named[t] for t in rng.permutation(len(named))])
        rows_a.append([unit_row(int(rng.integers(0, n_cols))), block_row(int(rng.integers(0, blocks)))])
        rows_a.append([])
    parts = 2 if np.dtype(dtype).kind == "c" else 1
    values = lambda count: rng.standard_normal(parts * count).astype(X.REAL_OF[letter]).view(dtype)
    a = csr([(cols, values(len(cols))) for cols in rows_a], dtype)
    b = csr([(cols, values(len(cols))) for cols, _ in rows_b], dtype)
    return a, b, n_cols, lengths


@pytest.mark.parametrize("letter", "SDCZ")
def test_rows_of_c_one_below_at_one_above_and_three_times_the_row_cap(gpu, letter):
    from spgpu_amd import capi
    cap = capi.SPGEMM_ROW_CAP
    rng = np.random.default_rng(300 + ord(letter))
    a, b, n_cols, lengths = _rows_around_the_cap(rng, letter, cap)
    _, c_ptr, _, _ = _multiply(gpu, a, b, n_cols, letter, 0, caps=(0, 1))
    got = np.diff(c_ptr)
    for k, L in enumerate(lengths):
        assert got[5 * k] == L and got[5 * k + 2] == L, (k, L)                # the one long row; the union of short rows
        assert 0 < got[5 * k + 1] <= 8 and 0 < got[5 * k + 3] <= 9 and got[5 * k + 4] == 0
    assert got[2] == cap - 1 and got[7] == cap and got[12] == cap + 1 and got[17] == 3 * cap


# ---- 4. the order of the additions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter,big", [("D", 1e16), ("S", 1e8)])
def test_the_additions_follow_the_storage_order_of_as_row(gpu, letter, big):
    dtype = X.DTYPE_OF[letter]
    rows_b = [([], [])] * 10
    rows_b[2], rows_b[5], rows_b[9] = ([0, 1], [1.0, 3.0]), ([0], [big]), ([0, 2], [-big, 2.0])
    b = csr(rows_b, dtype)
    seen = {}
    for order in ((5, 2, 9), (5, 9, 2), (2, 5, 9)):
        _, _, c_cols, c_vals = _multiply(gpu, csr([(list(order), [1.0, 1.0, 1.0])], dtype), b, 3, letter)
        assert c_cols.tolist() == [0, 1, 2]
        seen[order] = c_vals.tolist()
    assert seen[(5, 2, 9)] == [0.0, 3.0, 2.0] and seen[(5, 9, 2)] == [1.0, 3.0, 2.0] and seen[(2, 5, 9)] == [0.0, 3.0, 2.0]


# ---- 5. the product is rounded before it is added: what a contracted kernel gets wrong ----------------------------------------
@pytest.mark.parametrize("letter", "SD")
def test_no_fused_multiply_add_joins_the_product_to_the_sum(gpu, letter):
    """64 entries c(i, 0) = (0 + 1 * s) + a * b with a * b inexact and s = -round(a * b): exactly +0 when product and sum are rounded
    separately, the product's rounding error -- not 0 -- from one fused multiply-add.  The operands are searched on the CPU and the
    restatement is shown to tell the two apart before the GPU is asked."""
    from spgpu_amd import formats
    dtype = X.DTYPE_OF[letter]
    rng = np.random.default_rng(500 + ord(letter))
    found = [inexact_pair(rng, dtype) for _ in range(64)]
    rows_a = [([2 * t, 2 * t + 1], [1.0, found[t][0]]) for t in range(64)]
    rows_b = [row for t in range(64) for row in (([0], [-found[t][2]]), ([0], [found[t][1]]))]
    a, b = csr(rows_a, dtype), csr(rows_b, dtype)
    restated = formats.csr_spgemm(*a, *b, 1)[3]
    fused = np.array([f[3] for f in found], dtype)                           # fma(a, b, s) = the exact a * b - round(a * b)
    assert np.all(restated == 0) and not np.signbit(restated).any() and np.all(fused != 0)
    _multiply(gpu, a, b, 1, letter, caps=(0, 1))


@pytest.mark.parametrize("letter", "CZ")
def test_no_fused_multiply_add_inside_a_complex_product(gpu, letter):
    """The real part ar*br - ai*bi with ai*bi = round(ar*br) (bi = 1) and, mirrored, ar*br = round(ai*bi) (br = 1); the imaginary
    part ar*bi + ai*br with ai*br = -round(ar*bi): each is exactly 0 only if no product is fused into the addition."""
    from spgpu_amd import formats
    dtype = X.DTYPE_OF[letter]
    rng = np.random.default_rng(600 + ord(letter))
    rows_a, rows_b, fused = [], [], []
    for t in range(32):
        x, y, p, error = inexact_pair(rng, X.REAL_OF[letter])
        for a_val, b_val in ((complex(x, p), complex(y, 1)), (complex(p, x), complex(1, y)), (complex(x, -p), complex(1, y))):
            rows_a.append(([len(rows_b)], [a_val]))
            rows_b.append(([0], [b_val]))
        fused.append(float(error))
    a, b = csr(rows_a, dtype), csr(rows_b, dtype)
    restated = formats.csr_spgemm(*a, *b, 1)[3]
    assert np.all(restated[0::3].real == 0) and np.all(restated[1::3].real == 0) and np.all(restated[2::3].imag == 0)
    assert np.all(np.array(fused) != 0) and np.all(restated[0::3].imag != 0)
    _multiply(gpu, a, b, 1, letter, caps=(0, 1))


# ---- 6. cancellation keeps the entry; a lone -0.0 product is stored as +0.0 -------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
def test_cancelled_entries_stay_and_a_lone_negative_zero_becomes_positive(gpu, letter):
    dtype = X.DTYPE_OF[letter]
    a = csr([([0, 1], [1.0, 1.0]), ([2], [-1.0])], dtype)
    b = csr([([0, 3], [2.5, 1.0]), ([0], [-2.5]), ([1], [0.0])], dtype)
    products, c_ptr, c_cols, c_vals = _multiply(gpu, a, b, 4, letter, caps=(0, 1))
    assert products == 4 and c_ptr.tolist() == [0, 2, 3] and c_cols.tolist() == [0, 3, 1]
    assert c_vals.view(np.uint8).reshape(3, -1)[[0, 2]].max() == 0           # +0.0 twice, in every byte


# ---- 7. the refusals ------------------------------------------------------------------------------------------------------
def _valid_pair(rng, base):
    a = random_csr(rng, 70, 50, 8, np.float64, ascending=False, base=base)
    b = random_csr(rng, 50, 90, 9, np.float64, base=base)
    return [x.copy() for x in a], [x.copy() for x in b]


def _count(a, b, base, n_inner):
    """The products of the entries of A that name a row of B."""
    k = np.asarray(a[1], np.int64) - base
    k = k[(k >= 0) & (k < n_inner)]
    return int(np.diff(np.asarray(b[0], np.int64))[k].sum())


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("kind", ["below the base", "at base + aColumnsCount"])
def test_a_column_of_a_outside_b_is_refused(gpu, kind, base):
    from spgpu_amd import capi
    rng = np.random.default_rng(70)
    a, b = _valid_pair(rng, base)
    a[1][a[1].size // 2] = base - 1 if kind == "below the base" else base + 50
    d_a, d_b = _device(a), _device(b)
    st, products = _products(gpu, a, d_a, d_b, 50, base)
    assert st == capi.SPGPU_UNSUPPORTED and products == 0
    st, entries, _, _ = _plan(gpu, a, d_a, d_b, 50, 90, base, _count(a, b, base, 50))      # the plan checks again; guards in _plan
    assert st == capi.SPGPU_UNSUPPORTED and entries == 0
    _multiply(gpu, *_valid_pair(rng, base), 90, "D", base)                                 # the handle works on


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("kind", ["column below the base", "column at base + bColumnsCount", "row descends", "row repeats a column"])
def test_a_bad_row_of_b_is_refused(gpu, kind, base):
    from spgpu_amd import capi
    rng = np.random.default_rng(71)
    a, b = _valid_pair(rng, base)
    lengths = np.diff(b[0])
    named = np.unique(a[1]) - base
    k = int(named[np.argmax(lengths[named])])                                 # a row of B that A names, with two entries at least
    first = b[0][k] - base
    assert lengths[k] >= 2
    if kind == "column below the base":
        b[1][first] = base - 1
    elif kind == "column at base + bColumnsCount":
        b[1][first + lengths[k] - 1] = base + 90
    elif kind == "row descends":
        b[1][first], b[1][first + 1] = b[1][first + 1], b[1][first]
    else:
        b[1][first + 1] = b[1][first]
    d_a, d_b = _device(a), _device(b)
    st, products = _products(gpu, a, d_a, d_b, 50, base)
    assert st == capi.SPGPU_SUCCESS and products == _count(a, b, base, 50)                 # the products do not read B's columns
    st, entries, _, _ = _plan(gpu, a, d_a, d_b, 50, 90, base, products)
    assert st == capi.SPGPU_UNSUPPORTED and entries == 0, kind
    _multiply(gpu, *_valid_pair(rng, base), 90, "D", base)


def test_a_products_count_that_is_not_the_matrices_is_refused(gpu):
    from spgpu_amd import capi
    rng = np.random.default_rng(72)
    a, b = _valid_pair(rng, 0)
    d_a, d_b = _device(a), _device(b)
    right = _count(a, b, 0, 50)
    for wrong in (right - 1, right + 1, right // 2, 2 * right, 1):
        st, entries, _, _ = _plan(gpu, a, d_a, d_b, 50, 90, 0, wrong)                      # guards checked in _plan
        assert st == capi.SPGPU_UNSUPPORTED and entries == 0, wrong


def test_more_products_than_an_int_holds(gpu):
    """A 1 x 50 000 whose 50 000 entries all name row 7 of B, 50 000 long: 2.5e9 products."""
    from spgpu_amd import capi
    n = 50000
    assert n * n > INT_MAX
    a = (np.array([0, n], np.int32), np.full(n, 7, np.int32), np.ones(n))
    b_ptr = np.zeros(n + 1, np.int32)
    b_ptr[8:] = n
    b = (b_ptr, np.arange(n, dtype=np.int32), np.ones(n))
    d_a, d_b = _device(a), _device(b)
    st, products = _products(gpu, a, d_a, d_b, n, 0)                                        # guards checked in _products
    assert st == capi.SPGPU_UNSUPPORTED and products == -1
    a_small = (np.array([0, 3], np.int32), np.full(3, 7, np.int32), np.ones(3))            # three of them: 150 000, and it works
    want = _multiply(gpu, a_small, b, n, "D")
    assert want[0] == 3 * n and want[2].size == n and want[3].tolist() == [3.0] * n


def test_degenerate_shapes(gpu):
    import torch
    from spgpu_amd import capi
    for base in (0, 1):
        # A without entries, and A whose entries all name empty rows of B: no products, the plan writes the row pointers
        for a in (csr([([], [])] * 9, np.float64, base), csr([([2], [1.0]), ([], []), ([2, 2], [1.0, 2.0])] + [([], [])] * 6, np.float64, base)):
            b = csr([([0, 1], [1.0, 2.0]), ([3], [1.0]), ([], [])], np.float64, base)
            products, c_ptr, c_cols, _ = _multiply(gpu, a, b, 4, "D", base)
            assert products == 0 and c_cols.size == 0 and c_ptr.tolist() == [base] * 10
        d_a, d_b = _device(a), _device(b)
        st, entries, row_ptr, _ = _plan(gpu, a, d_a, d_b, 3, 4, base, 0)
        assert st == capi.SPGPU_SUCCESS and entries == 0 and row_ptr.numpy(np.int32).tolist() == [base] * 10
        cols, vals = _Guarded(64), _Guarded(64)
        assert capi.spgpuCsrSpgemmDevice(gpu, cols.ptr(), vals.ptr(), 0, 9, _p(d_a[0]), _p(d_a[1]), _p(d_a[2]), _p(d_b[0]), _p(d_b[1]),
                                         _p(d_b[2]), row_ptr.ptr(), base, capi.TYPE_DOUBLE, None) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        assert cols.untouched() and vals.untouched()
    for letter in "SDCZ":                                                    # 1 x 1 times 1 x 1: a key of no bits
        dtype = X.DTYPE_OF[letter]
        _multiply(gpu, csr([([0, 0, 0], [1.5, 2.0, -0.25])], dtype), csr([([0], [3.0])], dtype), 1, letter, caps=(0, 1))
        _multiply(gpu, csr([([0], [1.5])], dtype, 1), csr([([0], [3.0])], dtype, 1), 1, letter, 1)


# ---- 8. every kernel of the analysis on more than one workgroup, the scans on more than one tile ---------------------------------
def test_8k_rows_190k_products(gpu):
    rng = np.random.default_rng(8)
    n = 8000
    lengths_a, lengths_b = rng.integers(0, 9, n), rng.integers(0, 13, n)
    lengths_a[::50] = 0

    def banded(lengths, width):
        ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
        cols = np.concatenate([np.sort(rng.choice(np.arange(max(0, r - width), min(n, r + width)), L, replace=False))
                               for r, L in enumerate(lengths)]).astype(np.int32)
        return ptr, cols, rng.standard_normal(cols.size)

    a, b = banded(lengths_a, 40), banded(lengths_b, 40)
    products, c_ptr, c_cols, _ = _multiply(gpu, a, b, n, "D", caps=(0, 3))
    assert products > 150000 and c_cols.size > 1024 * 64 and (np.diff(c_ptr) == 0).any()


# ---- 9. determinism ----------------------------------------------------------------------------------------------------
def test_a_repeated_call_gives_the_same_bytes(gpu):
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(9)
    a = random_csr(rng, 500, 400, 20, np.float64, ascending=False, repeats=True)
    b = random_csr(rng, 400, 300, 25, np.float64)
    want = formats.csr_spgemm(*a, *b, 300)
    d_a, d_b = _device(a), _device(b)
    d_ptr, d_cols = formats.to_device(want[1]), formats.to_device(want[2])
    seen = set()
    for _ in range(3):
        out = _Guarded(want[2].size * 8)
        torch.cuda.synchronize()
        assert capi.spgpuCsrSpgemmValuesDevice(gpu, out.ptr(), 500, _p(d_a[0]), _p(d_a[1]), _p(d_a[2]), _p(d_b[0]), _p(d_b[1]), _p(d_b[2]),
                                               _p(d_ptr), _p(d_cols), 0, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        seen.add(out.buf.cpu().numpy().tobytes())
    assert len(seen) == 1 and out.numpy(np.float64).tobytes() == want[3].tobytes()


# ---- 10. the step in a captured graph -------------------------------------------------------------------------------------
def test_the_values_call_replays_from_a_captured_graph(gpu):
    """spgpuCsrSpgemmValuesDevice captured on the handle's stream, replayed after the values of A and B were overwritten in place:
    each replay gives the bytes of the restatement on the values of the moment."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(10)
    a = random_csr(rng, 300, 200, 12, np.float64, ascending=False, repeats=True)
    b = random_csr(rng, 200, 250, 15, np.float64)
    want = formats.csr_spgemm(*a, *b, 250)
    d_a, d_b = _device(a), _device(b)
    d_ptr, d_cols = formats.to_device(want[1]), formats.to_device(want[2])
    d_out = torch.zeros(want[2].size, dtype=torch.float64, device="cuda:0")

    def step():
        assert capi.spgpuCsrSpgemmValuesDevice(gpu, _p(d_out), 300, _p(d_a[0]), _p(d_a[1]), _p(d_a[2]), _p(d_b[0]), _p(d_b[1]), _p(d_b[2]),
                                               _p(d_ptr), _p(d_cols), 0, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS

    side = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
        wants = [want[3].tobytes()]
        for _ in range(2):
            new_a, new_b = rng.standard_normal(a[2].size), rng.standard_normal(b[2].size)
            wants.append(formats.csr_spgemm(a[0], a[1], new_a, b[0], b[1], new_b, 250)[3].tobytes())
            d_a[2].copy_(formats.to_device(new_a))
            d_b[2].copy_(formats.to_device(new_b))
            d_out.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert d_out.cpu().numpy().tobytes() == wants[-1]
        assert len(set(wants)) == 3
    finally:
        capi.spgpuSetStream(gpu, None)


# ---- 11. end to end: the Galerkin operator of an assembled Laplacian, in exact integers ------------------------------------------
def _device_product(gpu, a, b, n_inner, n_b_cols, base):
    """C = A * B on device CSR tuples (ptr, cols, vals, rows) through the public calls: the same kind of tuple."""
    import torch
    from spgpu_amd import capi
    n_rows = a[3]
    products, entries = C.c_int(-1), C.c_int(-1)
    small = torch.empty(capi.spgpuCsrSpgemmWorkBytes(n_rows, n_b_cols, 0), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert capi.spgpuCsrSpgemmProductsDevice(gpu, C.byref(products), n_rows, n_inner, _p(a[0]), _p(a[1]), _p(b[0]), base,
                                             _p(small)) == capi.SPGPU_SUCCESS
    work = torch.empty(capi.spgpuCsrSpgemmWorkBytes(n_rows, n_b_cols, products.value), dtype=torch.uint8, device="cuda:0")
    c_ptr = torch.zeros(n_rows + 1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert capi.spgpuCsrSpgemmPlanDevice(gpu, C.byref(entries), _p(c_ptr), n_rows, n_inner, n_b_cols, _p(a[0]), _p(a[1]), _p(b[0]), _p(b[1]), base,
                                         products.value, _p(work)) == capi.SPGPU_SUCCESS
    c_cols, c_vals = _zeros(entries.value, np.int32), _zeros(entries.value, np.float64)
    torch.cuda.synchronize()
    assert capi.spgpuCsrSpgemmDevice(gpu, _p(c_cols), _p(c_vals), entries.value, n_rows, _p(a[0]), _p(a[1]), _p(a[2]), _p(b[0]), _p(b[1]), _p(b[2]),
                                     _p(c_ptr), base, capi.TYPE_DOUBLE, _p(work)) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    return c_ptr, c_cols, c_vals, n_rows, entries.value


def test_the_galerkin_operator_of_an_assembled_laplacian(gpu):
    """16 x 16 grid, 5-point Laplacian listed with the diagonal split in two and assembled on the device; P aggregates 2 x 2 cells;
    P^T by spgpuHellTransposeDevice and spgpuHellToCsrDevice; R = P^T A, A_c = R P; A_c into HELL; one spgpuDhellspmv against the
    dense P^T A P x.  Small integers throughout: exact."""
    import torch
    from spgpu_amd import capi, formats
    from test_gpu_to_csr_device import _device_hell_of_csr
    n, base = 16, 1
    m, fine, coarse = n // 2, n * n, (n // 2) ** 2
    cell = np.arange(fine)
    gx, gy = cell % n, cell // n
    rows, cols, vals = [cell, cell], [cell, cell], [np.full(fine, 3.0), np.full(fine, 1.0)]
    for ok, to in ((gx > 0, cell - 1), (gx < n - 1, cell + 1), (gy > 0, cell - n), (gy < n - 1, cell + n)):
        rows.append(cell[ok]), cols.append(to[ok]), vals.append(np.full(int(ok.sum()), -1.0))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.random.default_rng(11).permutation(rows.size)
    rows, cols, vals = rows[order], cols[order], vals[order]
    dense_a = np.zeros((fine, fine))
    np.add.at(dense_a, (rows, cols), vals)
    aggregate = (gy // 2) * m + gx // 2
    dense_p = np.zeros((fine, coarse))
    dense_p[cell, aggregate] = 1.0
    # A: assembled on the device
    nnz = rows.size
    d_r, d_c, d_v = (formats.to_device(np.ascontiguousarray(t)) for t in ((rows + base).astype(np.int32), (cols + base).astype(np.int32), vals))
    a_ptr, perm, seg = (torch.zeros(k, dtype=torch.int32, device="cuda:0") for k in (fine + 1, nnz, nnz + 1))
    work = torch.empty(capi.spgpuCooAssembleWorkBytes(fine, fine, nnz), dtype=torch.uint8, device="cuda:0")
    unique = C.c_int(-1)
    torch.cuda.synchronize()
    assert capi.spgpuCooAssemblePlanDevice(gpu, C.byref(unique), _p(a_ptr), _p(perm), _p(seg), fine, fine, nnz, _p(d_r), _p(d_c), base, base,
                                           _p(work)) == capi.SPGPU_SUCCESS
    a_cols, a_vals = _zeros(unique.value, np.int32), _zeros(unique.value, np.float64)
    assert capi.spgpuCooAssembleDevice(gpu, _p(a_cols), _p(a_vals), unique.value, nnz, _p(d_c), _p(d_v), base, base, capi.TYPE_DOUBLE, _p(perm),
                                       _p(seg)) == capi.SPGPU_SUCCESS
    A = (a_ptr, a_cols, a_vals, fine)
    # P in CSR; P^T through HELL, the transpose and back to CSR
    p_host = ((cell + base).astype(np.int32), (aggregate + base).astype(np.int32), np.ones(fine))
    p_host = (np.append(p_host[0], fine + base).astype(np.int32), p_host[1], p_host[2])
    P = _device(p_host) + (fine,)
    src, _ = _device_hell_of_csr(gpu, fine, *p_host, base, 32, None)
    t = formats.hell_transpose_device(gpu, src["cM"], src["rP"], src["hack_offsets"], src["rS"], None, fine, coarse, 32, base, src["slots"], "D",
                                      t_hack_size=32, t_base=base)
    t_src = dict(kind="hell", dtype=np.dtype(np.float64), rows=coarse, base=base, hack_size=32, slots=t["slots"], cM=t["cM"], rP=t["rP"],
                 hack_offsets=t["hack_offsets"], rS=t["rS"])
    _, _, pt_ptr, pt_cols, pt_vals = _to_csr(gpu, t_src, base, runs=((None, 0),))
    assert np.array_equal(dense_of(pt_ptr, pt_cols, pt_vals, fine, base).real, dense_p.T)
    PT = _device((pt_ptr, pt_cols, pt_vals)) + (coarse,)
    # the two products
    R = _device_product(gpu, PT, A, fine, fine, base)
    Ac = _device_product(gpu, R, P, fine, coarse, base)
    host = lambda mat: tuple(x.cpu().numpy()[:k] for x, k in zip(mat[:3], (mat[3] + 1, mat[4], mat[4])))
    assert np.array_equal(dense_of(*host(R), fine, base).real, dense_p.T @ dense_a)
    want = dense_p.T @ dense_a @ dense_p
    assert np.array_equal(dense_of(*host(Ac), coarse, base).real, want) and Ac[4] == int((want != 0).sum())
    # A_c in HELL, one product
    st, longest, rs = _row_lengths(gpu, coarse, Ac[0], base)
    assert st == capi.SPGPU_SUCCESS and longest == 5
    height, ho = _hell_plan(gpu, coarse, 32, rs)
    cm, rp = _zeros(32 * height, np.float64), _zeros(32 * height, np.int32)
    assert capi.spgpuCsrToHellDevice(gpu, _p(cm), _p(rp), _p(ho), 32, base, coarse, _p(Ac[0]), _p(Ac[1]), _p(Ac[2]), base, capi.TYPE_DOUBLE,
                                     None) == capi.SPGPU_SUCCESS
    x = np.arange(coarse) % 13 + 1.0
    d_x, d_z = formats.to_device(x), _zeros(coarse, np.float64)
    capi.hellspmv["D"](gpu, _p(d_z), _p(d_z), capi.scalar("D", 1), _p(cm), _p(rp), 32, _p(ho), _p(rs), None, 0, coarse, _p(d_x),
                       capi.scalar("D", 0), base)
    torch.cuda.synchronize()
    assert np.array_equal(d_z.cpu().numpy(), want @ x) and np.abs(want @ x).max() > 0
