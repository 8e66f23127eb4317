"""CPU: formats.coo_assemble, numpy's restatement of include/spgpu/ext/assemble_device.h, against a dictionary-of-lists loop in pure
Python that follows the contract word for word -- byte for byte, for every value type and both index bases on either side -- and,
where scipy is installed, against scipy's pattern (not its value bytes: scipy does not promise the order of its additions)."""
import numpy as np
import pytest

from spgpu_amd import formats

DTYPES = {"S": np.float32, "D": np.float64, "C": np.complex64, "Z": np.complex128}


def _values(rng, count, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        real = np.float32 if dtype.itemsize == 8 else np.float64
        return (rng.standard_normal(count).astype(real) + 1j * rng.standard_normal(count).astype(real)).astype(dtype)
    return rng.standard_normal(count).astype(dtype)


def _by_the_book(n_rows, n_cols, rows, cols, vals, coo_base, csr_base):
    """The contract, one entry at a time."""
    lists = {}
    for i in range(len(rows)):                                    # ascending COO position
        lists.setdefault((int(rows[i]) - coo_base, int(cols[i]) - coo_base), []).append(i)
    keys = sorted(lists)                                          # ascending row, then ascending column
    perm, seg_ptr, out_cols, out_vals = [], [0], [], []
    row_ptr = np.zeros(n_rows + 1, np.int64)
    for r, c in keys:
        ids = lists[(r, c)]
        perm.extend(ids)
        seg_ptr.append(len(perm))
        out_cols.append(c + csr_base)
        total = vals[ids[0]]                                      # a numpy scalar of the element dtype: every + rounds there
        for i in ids[1:]:
            total = total + vals[i]
        out_vals.append(total)
        row_ptr[r + 1] += 1
    row_ptr = np.cumsum(row_ptr) + csr_base
    return (row_ptr.astype(np.int32), np.array(perm, np.int32), np.array(seg_ptr, np.int32), np.array(out_cols, np.int32),
            np.array(out_vals, vals.dtype))


def _lists(rng, dtype):
    """(n_rows, n_cols, rows, cols, vals) 0-based: heavy duplication with empty rows, every entry once, one entry many times, nothing."""
    rows = rng.integers(0, 23, 600)
    rows[np.isin(rows, (0, 7, 22))] = 11
    yield 23, 17, rows, rng.integers(0, 17, 600), _values(rng, 600, dtype)
    once = rng.permutation(40 * 30)[:500]
    yield 40, 30, once // 30, once % 30, _values(rng, 500, dtype)
    rows, cols = rng.integers(0, 9, 300), rng.integers(0, 9, 300)
    rows[::3], cols[::3] = 4, 5
    yield 9, 9, rows, cols, _values(rng, 300, dtype)
    yield 5, 5, np.zeros(0, np.int64), np.zeros(0, np.int64), _values(rng, 0, dtype)
    yield 1, 1, np.zeros(7, np.int64), np.zeros(7, np.int64), _values(rng, 7, dtype)


@pytest.mark.parametrize("letter", "SDCZ")
def test_coo_assemble_is_the_contract_byte_for_byte(letter):
    rng = np.random.default_rng(ord(letter))
    for n_rows, n_cols, rows, cols, vals in _lists(rng, DTYPES[letter]):
        for coo_base, csr_base in ((0, 0), (1, 0), (0, 1), (1, 1)):
            got = formats.coo_assemble(n_rows, n_cols, rows + coo_base, cols + coo_base, vals, coo_base, csr_base)
            want = _by_the_book(n_rows, n_cols, rows + coo_base, cols + coo_base, vals, coo_base, csr_base)
            for name, g, w in zip(("row_ptr", "perm", "seg_ptr", "cols", "vals"), got, want):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, n_rows, coo_base, csr_base)
            row_ptr, perm, seg_ptr, out_cols, _ = got
            assert row_ptr[0] == csr_base and row_ptr[-1] - csr_base == out_cols.size == seg_ptr.size - 1
            assert seg_ptr[0] == 0 and seg_ptr[-1] == rows.size and sorted(perm.tolist()) == list(range(rows.size))
            for r in range(n_rows):
                assert (np.diff(out_cols[row_ptr[r] - csr_base:row_ptr[r + 1] - csr_base]) > 0).all()


def test_a_single_contribution_is_copied_as_bits():
    vals = np.array([0x7FF8DEADBEEF0001, 0x8000000000000000, 0x7FF0000000000001, 0x3FF0000000000000], np.uint64).view(np.float64)
    out = formats.coo_assemble(2, 2, [1, 0, 0, 1], [1, 1, 0, 0], vals)
    assert out[4].tobytes() == vals[[2, 1, 3, 0]].tobytes()


def test_an_entry_outside_the_matrix_is_refused():
    for rows, cols in (([0, 5], [0, 0]), ([0, -1], [0, 0]), ([0, 0], [0, 4])):
        with pytest.raises(ValueError):
            formats.coo_assemble(5, 4, rows, cols, np.ones(2))


def test_the_pattern_is_scipys():
    scipy_sparse = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(3)
    for n_rows, n_cols, rows, cols, vals in _lists(rng, np.float64):
        row_ptr, _, _, out_cols, out_vals = formats.coo_assemble(n_rows, n_cols, rows, cols, vals)
        # ones as values: scipy drops no entry whose sum happens to be zero, and every sum is a count
        csr = scipy_sparse.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(n_rows, n_cols)).tocsr()
        csr.sum_duplicates()
        csr.sort_indices()
        assert np.array_equal(csr.indptr, row_ptr) and np.array_equal(csr.indices, out_cols)
        real = scipy_sparse.coo_matrix((vals, (rows, cols)), shape=(n_rows, n_cols)).tocsr()
        real.sum_duplicates()
        real.sort_indices()
        # the values in any order of addition: at most 100 contributions of magnitude below 6 per entry, so two orders differ by
        # less than 2 * 100 * 2^-53 * 600 < 2e-11
        assert np.abs(vals).max(initial=0.0) < 6 and np.diff(row_ptr).size == n_rows
        assert np.array_equal(real.indices, out_cols) and np.abs(real.data - out_vals).max(initial=0.0) < 2e-11
