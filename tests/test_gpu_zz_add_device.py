"""GPU: the sparse sum C = alpha * A + beta * B on CSR arrays (include/spgpu/ext/add_device.h).

Every output array -- cRowPtr, cColIndices, cValues -- and the scratch lie between 64 guard bytes, are poisoned as a whole with one
byte pattern, and the outputs must afterwards equal numpy's restatement of the contract (formats.csr_add) BYTE FOR BYTE.  The fills
run through the public calls and through each of the two fills behind them (one thread per stored entry of A and of B; a workgroup
per tile of C with the column slices of its rows in LDS), columns + values and values only, with alpha and beta on the host and in
device memory, on the whole grid and on a capped one: all must give the same bytes (_add).  The values-only runs come after the
scratch has been overwritten.  The matrices are the smallest at which each branch of the plan and of the staged fill can go wrong."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import exact_ref as X
from test_gpu_csr_device import _hell_plan, _p, _row_lengths, _zeros
from test_gpu_to_csr_device import _Guarded
from test_spgemm_restated import csr, dense_of, inexact_pair, random_csr

pytestmark = pytest.mark.gpu


def _device(mat):
    """(ptr, cols, vals) -> the same as device tensors (an empty array as one element that nobody reads)."""
    from spgpu_amd import formats
    some = lambda a: a if a.size else np.zeros(1, a.dtype)
    return tuple(formats.to_device(some(np.ascontiguousarray(a))) for a in mat)


def _plan(gpu, d_a, d_b, n_rows, n_cols, base):
    """spgpuCsrAddPlanDevice: (status, cNonZerosCount, cRowPtr as _Guarded, the scratch as _Guarded); the guards are checked here."""
    import torch
    from spgpu_amd import capi
    work = _Guarded(capi.spgpuCsrAddWorkBytes(n_rows), 192)                  # 256-byte aligned
    row_ptr = _Guarded((n_rows + 1) * 4)
    entries = C.c_int(-7)
    torch.cuda.synchronize()
    st = capi.spgpuCsrAddPlanDevice(gpu, C.byref(entries), row_ptr.ptr(), n_rows, n_cols, _p(d_a[0]), _p(d_a[1]), _p(d_b[0]), _p(d_b[1]), base,
                                    work.ptr())
    torch.cuda.synchronize()
    assert row_ptr.guards_intact() and work.guards_intact()
    return st, entries.value, row_ptr, work


def _add(gpu, a, b, n_cols, letter, alpha, beta, base=0, caps=(0, 1)):
    """The Plan and every fill on host CSR arrays given in `base`, everything against formats.csr_add.  Returns the restated
    (c_ptr, c_cols, c_vals)."""
    import torch
    from spgpu_amd import capi, formats
    dtype = np.dtype(X.DTYPE_OF[letter])
    assert a[2].dtype == dtype and b[2].dtype == dtype
    n_rows = a[0].size - 1
    want = formats.csr_add(*a, *b, n_cols, alpha, beta, base)
    w_ptr, w_cols, w_vals = want
    case = (letter, n_rows, n_cols, base)
    d_a, d_b = _device(a), _device(b)
    st, entries, row_ptr, work = _plan(gpu, d_a, d_b, n_rows, n_cols, base)
    assert st == capi.SPGPU_SUCCESS and entries == w_cols.size, case
    assert row_ptr.numpy(np.int32).tobytes() == w_ptr.tobytes(), case
    work.buf[work.first:work.first + work.nbytes].fill_(0xFF)               # no fill reads the scratch
    code, size = capi.TYPE_CODE[letter], dtype.itemsize
    h_alpha, h_beta = np.asarray([alpha], dtype), np.asarray([beta], dtype)   # one element each, on the host ...
    d_alpha, d_beta = formats.to_device(h_alpha), formats.to_device(h_beta)   # ... and in device memory
    at = lambda h: C.c_void_p(h.ctypes.data)
    runs = [(None, 0)] + [(fill, cap) for fill in (capi.ADD_FILL_PLAIN, capi.ADD_FILL_STAGED) for cap in caps]
    for what in ("full", "values", "device scalars"):
        for fill, cap in runs:
            cols, vals = _Guarded(entries * 4), _Guarded(entries * size)
            torch.cuda.synchronize()
            matrices = lambda al, be: (al, _p(d_a[0]), _p(d_a[1]), _p(d_a[2]), be, _p(d_b[0]), _p(d_b[1]), _p(d_b[2]), row_ptr.ptr(), base, code)
            if what == "full":
                args = (gpu, cols.ptr(), vals.ptr(), entries, n_rows) + matrices(at(h_alpha), at(h_beta))
                st = capi.spgpuCsrAddDevice(*args) if fill is None else capi.spgpuCsrAddDeviceWith(*args, fill, cap)
            elif what == "values":
                args = (gpu, vals.ptr(), n_rows) + matrices(at(h_alpha), at(h_beta))
                st = capi.spgpuCsrAddValuesDevice(*args) if fill is None else capi.spgpuCsrAddValuesDeviceWith(*args, fill, cap)
            else:
                args = (gpu, vals.ptr(), n_rows) + matrices(_p(d_alpha), _p(d_beta))
                st = capi.spgpuCsrAddValuesDeviceScalars(*args) if fill is None else capi.spgpuCsrAddValuesDeviceScalarsWith(*args, fill, cap)
            assert st == capi.SPGPU_SUCCESS, (case, what, fill, cap)
            torch.cuda.synchronize()
            assert cols.guards_intact() and vals.guards_intact() and row_ptr.guards_intact() and work.guards_intact(), (case, what, fill, cap)
            if what == "full":
                assert cols.numpy(np.int32).tobytes() == w_cols.tobytes(), (case, what, fill, cap)
            else:
                assert cols.untouched(), (case, what, fill, cap)
            assert vals.numpy(np.uint8).tobytes() == w_vals.tobytes(), (case, what, fill, cap)
    assert row_ptr.numpy(np.int32).tobytes() == w_ptr.tobytes(), case
    for d, h in zip(d_a + d_b, a + b):                                       # the inputs are as they were
        assert d.cpu().numpy()[:h.size].tobytes() == h.tobytes(), case
    return want


def _values(rng, count, letter):
    parts = 2 if letter in "CZ" else 1
    return rng.standard_normal(parts * count).astype(X.REAL_OF[letter]).view(X.DTYPE_OF[letter])


KINDS = ("interleaved", "empty in both", "empty in A", "empty in B", "identical", "disjoint")


def _mixed_pair(rng, n_rows, n_cols, letter, base, longest=12):
    """Row r is of kind KINDS[r % 6]: A's and B's columns drawn independently (some shared, some not), no entry on either side,
    none in A, none in B, the same columns on both sides, A on even and B on odd columns."""
    rows_a, rows_b = [], []
    draw = lambda pool: np.sort(rng.choice(pool, int(rng.integers(1, min(longest, pool.size) + 1)), replace=False))
    for r in range(n_rows):
        kind = KINDS[r % 6]
        ca = cb = np.zeros(0, np.int64)
        if kind == "interleaved":
            ca, cb = draw(np.arange(n_cols)), draw(np.arange(n_cols))
            if n_cols > 1:
                shared = int(rng.integers(0, n_cols))
                ca, cb = np.union1d(ca, [shared]), np.union1d(cb, [shared, (shared + 1) % n_cols])
        elif kind == "empty in A":
            cb = draw(np.arange(n_cols))
        elif kind == "empty in B":
            ca = draw(np.arange(n_cols))
        elif kind == "identical":
            ca = cb = draw(np.arange(n_cols))
        elif kind == "disjoint" and n_cols > 1:
            ca, cb = draw(np.arange(0, n_cols, 2)), draw(np.arange(1, n_cols, 2))
        rows_a.append((ca, _values(rng, ca.size, letter)))
        rows_b.append((cb, _values(rng, cb.size, letter)))
    dtype = X.DTYPE_OF[letter]
    return csr(rows_a, dtype, base), csr(rows_b, dtype, base)


def _scalars(letter):
    return (1.75, -0.3) if letter in "SD" else (complex(1.75, -0.6), complex(-0.3, 2.2))


# ---- 1. every type x both bases: rows empty on either side and on both, identical, disjoint and interleaved patterns -----------
@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
def test_random_sums_give_numpys_arrays(gpu, letter, base):
    rng = np.random.default_rng(100 + ord(letter))
    a, b = _mixed_pair(rng, 70, 90, letter, base)
    c_ptr, c_cols, _ = _add(gpu, a, b, 90, letter, *_scalars(letter), base)
    la, lb, lc = np.diff(a[0]), np.diff(b[0]), np.diff(c_ptr)
    assert lc[1] == 0 and la[2] == 0 and lc[2] == lb[2] > 0 and lb[3] == 0 and lc[3] == la[3] > 0            # the empty rows
    assert lc[4] == la[4] == lb[4] > 0 and lc[5] == la[5] + lb[5] and max(la[0], lb[0]) < lc[0] < la[0] + lb[0]  # same, disjoint, mixed
    assert c_cols.size < a[1].size + b[1].size


# ---- 2. the grid-stride loops --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 255, 256, 257])
def test_row_counts_around_the_wavefront_and_the_workgroup_on_capped_grids(gpu, n_rows):
    rng = np.random.default_rng(n_rows)
    for letter in "SZ":
        a, b = _mixed_pair(rng, n_rows, 40, letter, 0, longest=5)
        _add(gpu, a, b, 40, letter, *_scalars(letter), 0, caps=(1, 2))


# ---- 3. rows around the staged fill's tile and row cap ---------------------------------------------------------------------
def _rows_around(rng, letter, bound):
    """For every length L in (bound - 1, bound, bound + 1, 3 bound) three rows whose union has L columns: all of them in A and a few
    of them in B; the mirror image; and about 0.6 L on each side -- both under the bound, the union over it.  The first and the last
    row of the matrix are such rows, and seven short rows of every kind lie between two of them, so that tiles start and end inside
    long rows and long rows start anywhere in a tile."""
    n_cols = 3 * bound + 40
    lengths = (bound - 1, bound, bound + 1, 3 * bound)
    rows_a, rows_b, long_rows = [], [], []
    short_a, short_b = _mixed_pair(rng, 7 * 12, n_cols, letter, 0, longest=6)

    def short(mat, k):
        ptr, cols, vals = mat
        return [(cols[ptr[r]:ptr[r + 1]].astype(np.int64), vals[ptr[r]:ptr[r + 1]]) for r in range(7 * k, 7 * k + 7)]

    k = 0
    for L in lengths:
        union = np.sort(rng.choice(n_cols, L, replace=False))
        few = np.sort(rng.choice(union, 5, replace=False))
        left = np.sort(rng.choice(union, int(0.6 * L), replace=False))
        right = np.union1d(np.setdiff1d(union, left), left[::3])
        for ca, cb in ((union, few), (few, union), (left, right)):
            if rows_a:
                rows_a += short(short_a, k)
                rows_b += short(short_b, k)
                k += 1
            long_rows.append((len(rows_a), L, ca.size, cb.size))
            rows_a.append((ca, _values(rng, ca.size, letter)))
            rows_b.append((cb, _values(rng, cb.size, letter)))
    dtype = X.DTYPE_OF[letter]
    return csr(rows_a, dtype), csr(rows_b, dtype), n_cols, long_rows


@pytest.mark.parametrize("letter", "SDCZ")
def test_rows_one_below_at_one_above_and_three_times_every_bound_of_the_staged_fill(gpu, letter):
    from spgpu_amd import capi
    for bound in sorted({capi.ADD_TILE, capi.ADD_ROW_CAP}):
        rng = np.random.default_rng(300 + ord(letter) + bound)
        a, b, n_cols, long_rows = _rows_around(rng, letter, bound)
        c_ptr, _, _ = _add(gpu, a, b, n_cols, letter, *_scalars(letter), 0)
        got = np.diff(c_ptr)
        assert long_rows[0][0] == 0 and long_rows[-1][0] == got.size - 1 and len(long_rows) == 12
        for t, (row, L, in_a, in_b) in enumerate(long_rows):
            assert got[row] == L, (row, L)
            if t % 3 == 2:
                assert max(in_a, in_b) < L and in_a + in_b > L                # neither holds the other, and they share columns
                assert (in_a < bound and in_b < bound) == (L < 3 * bound)     # both under the bound, the union at or over it;
            else:                                                             # at 3 x bound both are over it
                assert max(in_a, in_b) == L and min(in_a, in_b) == 5
        starts = (c_ptr[[row for row, _, _, _ in long_rows]] % capi.ADD_TILE)
        assert len(set(starts.tolist())) > 6                                  # the long rows start at many places of a tile


# ---- 4. each product is rounded before the sum: what a contracted kernel gets wrong ------------------------------------------
def _inexact_for(rng, s, dtype, count):
    """`count` values v of `dtype` whose product with s is not representable: (v, round(s * v)) as two arrays."""
    vs, ps = [], []
    while len(vs) < count:
        v = dtype(1 + rng.random())
        p = dtype(s * v)
        if Fraction(float(s)) * Fraction(float(v)) != Fraction(float(p)):
            vs.append(v), ps.append(p)
    return np.array(vs, dtype), np.array(ps, dtype)


@pytest.mark.parametrize("letter", "SD")
def test_no_fused_multiply_add_joins_a_product_to_the_sum(gpu, letter):
    """64 entries c(i, 0) = s * v + 1 * (-round(s * v)) with s * v inexact: exactly +0 when the products and the sum are rounded
    separately, the product's rounding error -- not 0 -- from one fused multiply-add.  Then the mirror image, the inexact product on
    B's side.  The operands are searched on the CPU and the restatement is shown to give 0 before the GPU is asked."""
    from spgpu_amd import formats
    dtype = X.DTYPE_OF[letter]
    rng = np.random.default_rng(500 + ord(letter))
    s = inexact_pair(rng, dtype)[0]
    v, p = _inexact_for(rng, s, dtype, 64)
    left = csr([([0], [v[t]]) for t in range(64)], dtype)
    right = csr([([0], [-p[t]]) for t in range(64)], dtype)
    for a, b, alpha, beta in ((left, right, s, 1), (right, left, 1, s)):
        restated = formats.csr_add(*a, *b, 1, alpha, beta)[2]
        assert np.all(restated == 0) and not np.signbit(restated).any()
        _add(gpu, a, b, 1, letter, alpha, beta)


@pytest.mark.parametrize("letter", "CZ")
def test_no_fused_multiply_add_inside_a_complex_product(gpu, letter):
    """The real part sr*vr - si*vi with si*vi = round(sr*vr) (vi = 1) on a lone entry of A and, mirrored, sr*vr = round(si*vi) on a
    lone entry of B; an entry with both terms; and the imaginary part sr*vi + si*vr with si*vr = -round(sr*vi): each is exactly 0
    only if no product is fused into the addition."""
    from spgpu_amd import formats
    dtype = X.DTYPE_OF[letter]
    rng = np.random.default_rng(600 + ord(letter))
    for _ in range(6):
        x, y, p, error = inexact_pair(rng, X.REAL_OF[letter])
        a = csr([([0], [complex(y, 1)]), ([], []), ([1], [complex(y, 1)])], dtype)
        b = csr([([], []), ([0], [complex(1, y)]), ([1], [complex(1, y)])], dtype)
        alpha, beta = complex(x, p), complex(p, x)
        restated = formats.csr_add(*a, *b, 2, alpha, beta)[2]
        assert np.all(restated.real == 0) and np.all(restated.imag != 0) and float(error) != 0
        _add(gpu, a, b, 2, letter, alpha, beta)
        a = csr([([0], [complex(1, y)])], dtype)
        b = csr([([], [])], dtype)
        assert formats.csr_add(*a, *b, 1, complex(x, -p), 1)[2][0].imag == 0
        _add(gpu, a, b, 1, letter, complex(x, -p), 1)


@pytest.mark.parametrize("letter", "SDCZ")
def test_cancelled_entries_stay(gpu, letter):
    dtype = X.DTYPE_OF[letter]
    a = csr([([0, 2, 5], [1.5, 2.0, -4.0]), ([], []), ([1], [7.0]), ([], [])], dtype)
    b = csr([([2, 3, 5], [-1.0, 3.0, 2.0]), ([4], [1.0]), ([], []), ([], [])], dtype)
    c_ptr, c_cols, c_vals = _add(gpu, a, b, 6, letter, 1, 2)
    assert c_ptr.tolist() == [0, 4, 5, 6, 6] and c_cols.tolist() == [0, 2, 3, 5, 4, 1]
    assert c_vals.tolist() == [1.5, 0.0, 6.0, 0.0, 2.0, 7.0] and c_vals.view(np.uint8).reshape(6, -1)[[1, 3]].max() == 0


@pytest.mark.parametrize("letter", "SD")
def test_a_lone_negative_zero_keeps_its_bits(gpu, letter):
    dtype = X.DTYPE_OF[letter]
    a = csr([([0, 1, 2], [-0.0, 0.0, -0.0])], dtype)
    b = csr([([2, 3], [0.0, -0.0])], dtype)
    _, _, c_vals = _add(gpu, a, b, 4, letter, 1, 1)
    assert np.signbit(c_vals).tolist() == [True, False, False, True]
    _, _, c_vals = _add(gpu, a, b, 4, letter, -1, 1)
    assert np.signbit(c_vals).tolist() == [False, True, False, True]


# ---- 5. the refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("kind", ["column below the base", "column at base + columnsCount", "row descends", "row repeats a column"])
def test_a_bad_row_is_refused(gpu, kind, side, base):
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(70)
    pair = [[x.copy() for x in random_csr(rng, 70, 90, 9, np.float64, base=base)] for _ in range(2)]
    bad = pair[0 if side == "A" else 1]
    lengths = np.diff(bad[0])
    k = int(np.argmax(lengths))
    first = bad[0][k] - base
    assert lengths[k] >= 2
    if kind == "column below the base":
        bad[1][first] = base - 1
    elif kind == "column at base + columnsCount":
        bad[1][first + lengths[k] - 1] = base + 90
    elif kind == "row descends":
        bad[1][first], bad[1][first + 1] = bad[1][first + 1], bad[1][first]
    else:
        bad[1][first + 1] = bad[1][first]
    with pytest.raises(ValueError):
        formats.csr_add(*pair[0], *pair[1], 90, 1, 1, base)
    st, entries, _, _ = _plan(gpu, _device(pair[0]), _device(pair[1]), 70, 90, base)           # the guards are checked in _plan
    assert st == capi.SPGPU_UNSUPPORTED and entries == 0, (kind, side)
    good = [random_csr(rng, 70, 90, 9, np.float64, base=base) for _ in range(2)]               # the handle works on
    _add(gpu, good[0], good[1], 90, "D", 2.0, -1.0, base, caps=(0,))


def test_degenerate_shapes(gpu):
    import torch
    from spgpu_amd import capi
    one = np.ones(1)
    at = C.c_void_p(one.ctypes.data)
    for base in (0, 1):
        nothing = csr([([], [])] * 9, np.float64, base)
        c_ptr, c_cols, _ = _add(gpu, nothing, nothing, 4, "D", 1, 1, base)                     # no entry at all: the Plan writes cRowPtr
        assert c_cols.size == 0 and c_ptr.tolist() == [base] * 10
        d = _device(nothing)
        cols, vals = _Guarded(64), _Guarded(64)
        assert capi.spgpuCsrAddDevice(gpu, cols.ptr(), vals.ptr(), 0, 9, at, _p(d[0]), _p(d[1]), _p(d[2]), at, _p(d[0]), _p(d[1]), _p(d[2]),
                                      _p(d[0]), base, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        assert cols.untouched() and vals.untouched()
    for letter in "SDCZ":                                                    # 1 x 1
        dtype = X.DTYPE_OF[letter]
        _add(gpu, csr([([0], [1.5])], dtype), csr([([0], [3.0])], dtype), 1, letter, 2, -1)
        _add(gpu, csr([([0], [1.5])], dtype, 1), csr([([], [])], dtype, 1), 1, letter, 2, -1, 1)


# ---- the plan's scan on more than one tile, every kernel on more than one workgroup --------------------------------------------
def test_9k_rows_two_stencils(gpu):
    """M + dt K in miniature, 96 x 96 grid points and more than 8 scan tiles of row counts: the 5-point pattern plus its
    tridiagonal-in-x subset, and the upwind pattern plus its transpose."""
    n = 96
    cell = np.arange(n * n)
    gx, gy = cell % n, cell // n
    rng = np.random.default_rng(8)

    def pattern(offsets):
        rows, cols = [], []
        for ok, to in offsets:
            rows.append(cell[ok]), cols.append(to[ok])
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        order = np.lexsort((cols, rows))
        ptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n * n)))).astype(np.int32)
        return ptr, cols[order].astype(np.int32), rng.standard_normal(rows.size)

    everywhere = np.ones(n * n, bool)
    left, right, down, up = (gx > 0, cell - 1), (gx < n - 1, cell + 1), (gy > 0, cell - n), (gy < n - 1, cell + n)
    five, three = pattern([(everywhere, cell), left, right, down, up]), pattern([(everywhere, cell), left, right])
    c_ptr, c_cols, _ = _add(gpu, three, five, n * n, "D", 1.0, 0.01)
    assert c_ptr.tobytes() == five[0].tobytes() and c_cols.tobytes() == five[1].tobytes() and c_cols.size > 40000
    upwind, transposed = pattern([(everywhere, cell), left, down]), pattern([(everywhere, cell), right, up])
    c_ptr, c_cols, _ = _add(gpu, upwind, transposed, n * n, "D", 1.0, 1.0, caps=(0, 3))
    assert c_ptr.tobytes() == five[0].tobytes() and c_cols.tobytes() == five[1].tobytes()


# ---- 6. determinism ----------------------------------------------------------------------------------------------------
def test_a_repeated_call_gives_the_same_bytes(gpu):
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(9)
    a, b = random_csr(rng, 500, 400, 20, np.float64), random_csr(rng, 500, 400, 25, np.float64)
    alpha, beta = np.array([0.7]), np.array([-1.3])
    want = formats.csr_add(*a, *b, 400, alpha[0], beta[0])
    d_a, d_b = _device(a), _device(b)
    d_ptr = formats.to_device(want[0])
    seen = set()
    for _ in range(2):
        cols, vals = _Guarded(want[1].size * 4), _Guarded(want[1].size * 8)
        torch.cuda.synchronize()
        assert capi.spgpuCsrAddDevice(gpu, cols.ptr(), vals.ptr(), want[1].size, 500, C.c_void_p(alpha.ctypes.data), _p(d_a[0]), _p(d_a[1]),
                                      _p(d_a[2]), C.c_void_p(beta.ctypes.data), _p(d_b[0]), _p(d_b[1]), _p(d_b[2]), _p(d_ptr), 0,
                                      capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        seen.add(cols.buf.cpu().numpy().tobytes() + vals.buf.cpu().numpy().tobytes())
    assert len(seen) == 1 and vals.numpy(np.float64).tobytes() == want[2].tobytes() and cols.numpy(np.int32).tobytes() == want[1].tobytes()


# ---- 7. the step in a captured graph -------------------------------------------------------------------------------------
def test_the_values_calls_replay_from_a_captured_graph(gpu):
    """spgpuCsrAddValuesDevice captured on the handle's stream and replayed after the values of A and B were overwritten in place;
    spgpuCsrAddValuesDeviceScalars captured and replayed after alpha and beta were overwritten in device memory: each replay gives
    the bytes of the restatement on the values and scalars of the moment."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(10)
    a, b = random_csr(rng, 300, 250, 12, np.float64), random_csr(rng, 300, 250, 15, np.float64)
    alpha, beta = np.array([1.0]), np.array([0.125])
    want = formats.csr_add(*a, *b, 250, alpha[0], beta[0])
    d_a, d_b = _device(a), _device(b)
    d_ptr = formats.to_device(want[0])
    d_alpha, d_beta = formats.to_device(alpha), formats.to_device(beta)
    d_out, d_out2 = (torch.zeros(want[1].size, dtype=torch.float64, device="cuda:0") for _ in range(2))
    matrices = lambda al, be: (al, _p(d_a[0]), _p(d_a[1]), _p(d_a[2]), be, _p(d_b[0]), _p(d_b[1]), _p(d_b[2]), _p(d_ptr), 0, capi.TYPE_DOUBLE)

    def step():
        assert capi.spgpuCsrAddValuesDevice(gpu, _p(d_out), 300, *matrices(C.c_void_p(alpha.ctypes.data),
                                                                            C.c_void_p(beta.ctypes.data))) == capi.SPGPU_SUCCESS
        assert capi.spgpuCsrAddValuesDeviceScalars(gpu, _p(d_out2), 300, *matrices(_p(d_alpha), _p(d_beta))) == capi.SPGPU_SUCCESS

    side = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
        wants = [want[2].tobytes()]
        for dt in (0.25, -3.0):
            new_a, new_b = rng.standard_normal(a[2].size), rng.standard_normal(b[2].size)
            host_scalars = formats.csr_add(a[0], a[1], new_a, b[0], b[1], new_b, 250, alpha[0], beta[0])[2].tobytes()
            device_scalars = formats.csr_add(a[0], a[1], new_a, b[0], b[1], new_b, 250, dt + 1, dt)[2].tobytes()
            wants += [host_scalars, device_scalars]
            d_a[2].copy_(formats.to_device(new_a))
            d_b[2].copy_(formats.to_device(new_b))
            d_alpha.fill_(dt + 1)
            d_beta.fill_(dt)
            d_out.fill_(float("nan"))
            d_out2.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert d_out.cpu().numpy().tobytes() == host_scalars            # the scalars of the capture, the values of the moment
            assert d_out2.cpu().numpy().tobytes() == device_scalars         # both of the moment
        assert len(set(wants)) == 5
    finally:
        capi.spgpuSetStream(gpu, None)


# ---- 8. end to end: M + dt K of two assembled matrices, in exact integers ------------------------------------------------------
def _assembled(gpu, n_rows, rows, cols, vals, base):
    """A COO list with duplicates (0-based, host) -> device CSR (ptr, cols, vals) through the assembly calls."""
    import torch
    from spgpu_amd import capi, formats
    nnz = rows.size
    d_r, d_c, d_v = (formats.to_device(np.ascontiguousarray(t)) for t in ((rows + base).astype(np.int32), (cols + base).astype(np.int32), vals))
    ptr, perm, seg = (torch.zeros(k, dtype=torch.int32, device="cuda:0") for k in (n_rows + 1, nnz, nnz + 1))
    work = torch.empty(capi.spgpuCooAssembleWorkBytes(n_rows, n_rows, nnz), dtype=torch.uint8, device="cuda:0")
    unique = C.c_int(-1)
    torch.cuda.synchronize()
    assert capi.spgpuCooAssemblePlanDevice(gpu, C.byref(unique), _p(ptr), _p(perm), _p(seg), n_rows, n_rows, nnz, _p(d_r), _p(d_c), base, base,
                                           _p(work)) == capi.SPGPU_SUCCESS
    out_cols, out_vals = _zeros(unique.value, np.int32), _zeros(unique.value, np.float64)
    assert capi.spgpuCooAssembleDevice(gpu, _p(out_cols), _p(out_vals), unique.value, nnz, _p(d_c), _p(d_v), base, base, capi.TYPE_DOUBLE,
                                       _p(perm), _p(seg)) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    return ptr, out_cols, out_vals, unique.value


def test_the_system_matrix_of_two_assembled_matrices(gpu):
    """16 x 16 grid: K the 5-point Laplacian and M a mass matrix on its tridiagonal-in-x subset, each listed with the diagonal split
    in two and assembled on the device; C = M + 3 K through the Plan and the fill; C into HELL; one spgpuDhellspmv against the dense
    (M + 3 K) x.  Small integers throughout: exact."""
    import torch
    from spgpu_amd import capi, formats
    n, base, dt = 16, 1, 3.0
    size = n * n
    cell = np.arange(size)
    gx, gy = cell % n, cell // n
    rng = np.random.default_rng(11)

    def listing(diagonal, neighbours, value):
        rows, cols, vals = [cell, cell], [cell, cell], [np.full(size, diagonal - 1.0), np.full(size, 1.0)]
        for ok, to in neighbours:
            rows.append(cell[ok]), cols.append(to[ok]), vals.append(np.full(int(ok.sum()), value))
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        order = rng.permutation(rows.size)
        dense = np.zeros((size, size))
        np.add.at(dense, (rows, cols), vals)
        return rows[order], cols[order], vals[order], dense

    in_x = [(gx > 0, cell - 1), (gx < n - 1, cell + 1)]
    in_y = [(gy > 0, cell - n), (gy < n - 1, cell + n)]
    *k_list, dense_k = listing(4.0, in_x + in_y, -1.0)
    *m_list, dense_m = listing(4.0, in_x, 1.0)
    K, M = _assembled(gpu, size, *k_list, base), _assembled(gpu, size, *m_list, base)
    assert K[3] == int((dense_k != 0).sum()) and M[3] == int((dense_m != 0).sum()) < K[3]
    entries = C.c_int(-1)
    work = torch.empty(capi.spgpuCsrAddWorkBytes(size), dtype=torch.uint8, device="cuda:0")
    c_ptr = torch.zeros(size + 1, dtype=torch.int32, device="cuda:0")
    assert capi.spgpuCsrAddPlanDevice(gpu, C.byref(entries), _p(c_ptr), size, size, _p(M[0]), _p(M[1]), _p(K[0]), _p(K[1]), base,
                                      _p(work)) == capi.SPGPU_SUCCESS
    assert entries.value == K[3]                                             # M's pattern lies inside K's
    del work
    c_cols, c_vals = _zeros(entries.value, np.int32), _zeros(entries.value, np.float64)
    one, step = np.ones(1), np.array([dt])
    assert capi.spgpuCsrAddDevice(gpu, _p(c_cols), _p(c_vals), entries.value, size, C.c_void_p(one.ctypes.data), _p(M[0]), _p(M[1]), _p(M[2]),
                                  C.c_void_p(step.ctypes.data), _p(K[0]), _p(K[1]), _p(K[2]), _p(c_ptr), base, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    want = dense_m + dt * dense_k
    host = (c_ptr.cpu().numpy(), c_cols.cpu().numpy()[:entries.value], c_vals.cpu().numpy()[:entries.value])
    assert np.array_equal(dense_of(*host, size, base).real, want) and np.array_equal(host[0], K[0].cpu().numpy())
    st, longest, rs = _row_lengths(gpu, size, c_ptr, base)
    assert st == capi.SPGPU_SUCCESS and longest == 5
    height, ho = _hell_plan(gpu, size, 32, rs)
    cm, rp = _zeros(32 * height, np.float64), _zeros(32 * height, np.int32)
    assert capi.spgpuCsrToHellDevice(gpu, _p(cm), _p(rp), _p(ho), 32, base, size, _p(c_ptr), _p(c_cols), _p(c_vals), base, capi.TYPE_DOUBLE,
                                     None) == capi.SPGPU_SUCCESS
    x = np.arange(size) % 13 + 1.0
    d_x, d_z = formats.to_device(x), _zeros(size, np.float64)
    capi.hellspmv["D"](gpu, _p(d_z), _p(d_z), capi.scalar("D", 1), _p(cm), _p(rp), 32, _p(ho), _p(rs), None, 0, size, _p(d_x),
                       capi.scalar("D", 0), base)
    torch.cuda.synchronize()
    assert np.array_equal(d_z.cpu().numpy(), want @ x) and np.abs(want @ x).max() > 0
