"""CPU: the restatements the GPU tests compare bytes with -- formats.coo_assemble, formats.csr_spgemm, formats.hell_transposed_coo --
on inputs whose 64-bit sort keys reach beyond bit 31, against loops in pure Python that share no code with them: the key of an entry
is a Python int built by the documented layout (assemble_device.hip and spgemm_device.hip: (row << colBits) | column; transpose_device.hip:
(column << rowBits) | row), the entries are the sorted keys of a dict, and the sums are Python integers.  Every value is a non-zero
integer of magnitude <= 8 (both parts, for the complex types), so every product and every partial sum is exact in every type and
the comparison is of bytes; the reference asserts that bound on every sum it makes.

Beside the comparison every case computes, in Python integers, the largest key the library would form and asserts that it has a bit
at or above bit 32 and that rowBits + colBits is the width the case was built for: that is what makes a case wide.  Two cases
cannot be: the 2^16 x 2^16 corner of the widths around a power of two is the 32-bit side of the 32/33-bit step (its largest key is
2^32 - 1 exactly, asserted), and the chain (A B) C is wide in the column indices the second product reads, not in its keys.

tests/test_gpu_zz_wide_keys.py imports the case builders from here: both files run the same inputs.  No array of a matrix's column
count is ever allocated: the widest matrices have 2^31 - 1 columns."""
import numpy as np
import pytest

from spgpu_amd import formats

W = 2 ** 31 - 1
DTYPES = {"S": np.float32, "D": np.float64, "C": np.complex64, "Z": np.complex128}
EXACT = {"S": 2 ** 24, "C": 2 ** 24, "D": 2 ** 53, "Z": 2 ** 53}
SCAN_CARRY = 256 * 1024          # scanned elements beyond which scanTotalsKernel (convert_scan.hip.h) loops with a carry
BASE_PAIRS = ((0, 0), (1, 1), (0, 1), (1, 0))          # (cooBaseIndex, csrBaseIndex)


def bits_for(n):
    """Smallest b with 2^b >= n: the width the three analyses give a dimension of n."""
    b = 0
    while (1 << b) < n:
        b += 1
    return b


def pool(rng, count, extra=6):
    """Columns of a matrix of `count` columns: 0, 2^16 - 1, 2^16, 2^30, count - 2, count - 1 where the matrix has them, and `extra`
    random ones; ascending Python ints."""
    fixed = [0, 2 ** 16 - 1, 2 ** 16, 2 ** 30, count - 2, count - 1]
    return sorted({c for c in fixed + [int(c) for c in rng.integers(0, count, extra)] if 0 <= c < count})


def integer_values(rng, count, letter):
    """Non-zero integers of magnitude <= 8 in the type of `letter`; both parts of a complex value are non-zero."""
    dtype = np.dtype(DTYPES[letter])
    parts = 2 if dtype.kind == "c" else 1
    v = rng.integers(1, 9, parts * count) * (2 * rng.integers(0, 2, parts * count) - 1)
    return v.astype("f%d" % (dtype.itemsize // parts)).view(dtype)


def _parts(value):
    """(re, im) of an integer-valued element as Python ints."""
    z = complex(value)
    re, im = int(z.real), int(z.imag)
    assert re == z.real and im == z.imag
    return re, im


def _elements(sums, letter):
    dtype = np.dtype(DTYPES[letter])
    assert all(abs(re) < EXACT[letter] and abs(im) < EXACT[letter] for re, im in sums)
    if dtype.kind == "c":
        return np.array([complex(re, im) for re, im in sums], dtype)
    return np.array([re for re, _ in sums], dtype)


def top_bit(key):
    return key.bit_length() - 1


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _drawn(rng, pairs, planted, count):
    """`count` contributions: every planted pair twice, the rest drawn from `pairs` and `planted` alike; shuffled.  0-based int64."""
    pairs = sorted(set(pairs) | set(planted))
    first = [p for p in planted for _ in range(2)]
    assert len(first) < count
    rest = [pairs[t] for t in rng.integers(0, len(pairs), count - len(first))]
    both = np.array(first + rest, np.int64)[rng.permutation(count)]
    return np.ascontiguousarray(both[:, 0]), np.ascontiguousarray(both[:, 1])


def assembly_narrow_rows_widest_columns():
    """70 x (2^31 - 1), 2 000 contributions.  Beside the pool: columns 5 ^ 2^k and (2^16 - 1) ^ 2^k for k = 16 .. 30, which differ
    from 5 and from 2^16 - 1 in one bit of bits 16 .. 30 only; rows r and r + 64 for r = 0 .. 5, which differ in the top row bit only."""
    rng = np.random.default_rng(2001)
    columns = pool(rng, W, 8)
    near = [b ^ (1 << k) for b in (5, 2 ** 16 - 1) for k in range(16, 31)]
    assert all(0 <= c < W for c in near)
    columns = sorted(set(columns) | set(near) | {5})
    planted = [(3, c) for c in [5] + near[:15]] + [(69, c) for c in [2 ** 16 - 1] + near[15:]]
    planted += [(r + top, c) for r in range(6) for top in (0, 64) for c in (0, 2 ** 30, W - 1)]
    pairs = [(int(r), columns[int(t)]) for r, t in zip(rng.integers(0, 70, 500), rng.integers(0, len(columns), 500))]
    rows, cols = _drawn(rng, pairs, planted, 2000)
    return dict(n_rows=70, n_cols=W, rows=rows, cols=cols, row_bits=7, col_bits=31)


def assembly_both_halves_wide():
    """(2^18 + 1) x (2^20 + 1), 5 000 contributions; rows 0 and 2^18 and columns 0 and 2^20 are present, each with the other's extremes."""
    rng = np.random.default_rng(2002)
    n_rows, n_cols = 2 ** 18 + 1, 2 ** 20 + 1
    columns = pool(rng, n_cols, 200)
    some_rows = sorted({0, 2 ** 16 - 1, 2 ** 16, 2 ** 18 - 1, 2 ** 18} | {int(r) for r in rng.integers(0, n_rows, 200)})
    planted = [(r, c) for r in (0, 2 ** 18) for c in (0, 2 ** 20)]
    pairs = [(some_rows[int(s)], columns[int(t)]) for s, t in zip(rng.integers(0, len(some_rows), 2000), rng.integers(0, len(columns), 2000))]
    rows, cols = _drawn(rng, pairs, planted, 5000)
    return dict(n_rows=n_rows, n_cols=n_cols, rows=rows, cols=cols, row_bits=19, col_bits=21)


POWER_OF_TWO_SHAPES = [(2 ** 16, 2 ** 16), (2 ** 16, 2 ** 16 + 1), (2 ** 16 + 1, 2 ** 16), (2 ** 16 + 1, 2 ** 16 + 1)]


def assembly_around_a_power_of_two(n_rows, n_cols):
    """Dimensions of 2^16 (16 bits) and 2^16 + 1 (17 bits), 1 000 contributions with the entries (rows - 1, cols - 1) and (rows - 1, 0)."""
    rng = np.random.default_rng(2003 + n_rows + 2 * n_cols)
    columns = pool(rng, n_cols, 60)
    some_rows = pool(rng, n_rows, 60)
    planted = [(n_rows - 1, n_cols - 1), (n_rows - 1, 0), (0, n_cols - 1), (0, 0)]
    pairs = [(some_rows[int(s)], columns[int(t)]) for s, t in zip(rng.integers(0, len(some_rows), 400), rng.integers(0, len(columns), 400))]
    rows, cols = _drawn(rng, pairs, planted, 1000)
    return dict(n_rows=n_rows, n_cols=n_cols, rows=rows, cols=cols, row_bits=bits_for(n_rows), col_bits=bits_for(n_cols))


def refused_assembly_list(base):
    """70 x (2^31 - 2): a valid wide list (0-based) of 2 000 contributions; the refusals move one entry of it just outside."""
    rng = np.random.default_rng(2004 + base)
    n_cols = W - 1
    columns = pool(rng, n_cols, 20)
    pairs = [(int(r), columns[int(t)]) for r, t in zip(rng.integers(0, 70, 600), rng.integers(0, len(columns), 600))]
    rows, cols = _drawn(rng, pairs, [(69, n_cols - 1), (0, 0)], 2000)
    return dict(n_rows=70, n_cols=n_cols, rows=rows, cols=cols, row_bits=7, col_bits=31)


def _csr_of_rows(rows, letter, rng, base):
    """[columns of row 0, ...] (0-based Python ints) -> (ptr, cols, vals) in `base` with integer values."""
    ptr = np.cumsum([0] + [len(r) for r in rows]) + base
    cols = np.array([c for r in rows for c in r], np.int64) + base
    assert cols.size == 0 or cols.max() <= W
    return ptr.astype(np.int32), cols.astype(np.int32), integer_values(rng, cols.size, letter)


def seventy_by_fifty(letter, base):
    """The A of test_gpu_zz_spgemm_device._seventy_by_ninety -- shuffled rows, a column repeated in every other row, rows 0, 33 and 69
    empty, row 5 naming only rows 3, 20 and 49 of B -- with integer values."""
    from test_gpu_zz_spgemm_device import _seventy_by_ninety
    rng = np.random.default_rng(2005 + ord(letter))
    (a_ptr, a_cols, _), _ = _seventy_by_ninety(rng, letter, base)
    return a_ptr, a_cols, integer_values(rng, a_cols.size, letter)


def _ascending_rows(rng, n_rows, columns, shortest, longest, empty=()):
    rows = []
    for k in range(n_rows):
        length = 0 if k in empty else int(rng.integers(shortest, longest + 1))
        rows.append(sorted(columns[int(t)] for t in rng.choice(len(columns), length, replace=False)))
    return rows


def spgemm_widest_b(letter, base, n_b_cols=W):
    """A 70 x 50 (seventy_by_fifty) times B 50 x (2^31 - 1): ascending rows of 2 to 12 pool columns, rows 3, 20 and 49 empty, the
    boundary columns in the rows that A's last non-empty row names."""
    rng = np.random.default_rng(2006 + ord(letter) + base)
    a = seventy_by_fifty(letter, base)
    columns = pool(rng, n_b_cols, 24)
    rows = _ascending_rows(rng, 50, columns, 2, 12, empty=(3, 20, 49))
    edge = [0, 2 ** 16 - 1, 2 ** 16, 2 ** 30, n_b_cols - 2, n_b_cols - 1]
    last = int(np.flatnonzero(np.diff(a[0]) > 0)[-1])                     # A's last non-empty row: beyond row 64, the top row bit
    assert 64 <= last < 69 and last != 5
    for k in np.unique(a[1][a[0][last] - base:a[0][last + 1] - base] - base):
        if k not in (3, 20, 49):
            rows[int(k)] = sorted(set(rows[int(k)]) | set(edge))
    b = _csr_of_rows(rows, letter, rng, base)
    return dict(a=a, b=b, n_b_cols=n_b_cols, base=base, last=last, row_bits=7, col_bits=bits_for(n_b_cols))


def spgemm_many_rows():
    """A (2^18 + 1) x 64 with 0 to 2 entries a row -- nine rows in ten empty, which keeps formats.csr_spgemm's Python loop to seconds;
    the first and the last row have two -- times B 64 x (2^20 + 1) with rows of 8 to 14 columns; row 63, which A's last row names,
    holds columns 0 and 2^20.  More than 262 144 row counts and more than 262 144 products: both scans of the analysis carry."""
    rng = np.random.default_rng(2007)
    n_rows, n_b_cols = 2 ** 18 + 1, 2 ** 20 + 1
    lengths = rng.choice(3, n_rows, p=(0.9, 0.05, 0.05))
    lengths[0] = lengths[-1] = 2
    a_cols = rng.integers(0, 64, int(lengths.sum()))
    a_cols[-2:] = (63, 11)
    a_ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    a = (a_ptr, a_cols.astype(np.int32), integer_values(rng, a_cols.size, "D"))
    columns = pool(rng, n_b_cols, 60)
    rows = _ascending_rows(rng, 64, columns, 8, 14)
    rows[63] = sorted(set(rows[63]) | {0, 2 ** 16 - 1, 2 ** 16, 2 ** 20 - 1, 2 ** 20})
    b = _csr_of_rows(rows, "D", rng, 0)
    return dict(a=a, b=b, n_b_cols=n_b_cols, base=0, row_bits=19, col_bits=21)


def spgemm_chain(base):
    """(A B) C: A 70 x 50, B 50 x (2^20 + 1) on pool columns, C (2^20 + 1) x 90 in which only half of those columns are non-empty
    rows (0, 2^16 and 2^20 among them).  The wide columns of A B are the aColIndices of the second product."""
    rng = np.random.default_rng(2008 + base)
    n_mid = 2 ** 20 + 1
    a = seventy_by_fifty("D", base)
    columns = pool(rng, n_mid, 30)
    b = _csr_of_rows(_ascending_rows(rng, 50, columns, 2, 10, empty=(3, 20, 49)), "D", rng, base)
    live = sorted({0, 2 ** 16, 2 ** 20} | set(columns[::2]))
    lengths = np.zeros(n_mid, np.int64)
    c_rows = _ascending_rows(rng, len(live), list(range(90)), 1, 7)
    lengths[live] = [len(r) for r in c_rows]
    c_ptr = (np.concatenate(([0], np.cumsum(lengths))) + base).astype(np.int32)
    c_cols = (np.array([j for r in c_rows for j in r], np.int64) + base).astype(np.int32)
    c = (c_ptr, c_cols, integer_values(rng, c_cols.size, "D"))
    return dict(a=a, b=b, c=c, n_mid=n_mid, n_c_cols=90, base=base)


def refused_spgemm_pair(base):
    """A 70 x 50 and a valid B 50 x (2^31 - 2) whose rows all have two columns at least."""
    case = spgemm_widest_b("D", base, n_b_cols=W - 1)
    lengths = np.diff(case["b"][0])
    k = int(case["a"][1][0]) - base                       # a row of B that A names
    assert lengths[k] >= 2
    return case, k


_TRANSPOSE = {}


def transpose_source(letter, duplicates=True, with_order=False, hack_size=32, base=0):
    """HELL of (2^17 + 1) x 2^20 built by the oracle's converters: 0 to 3 entries a row, columns ascending in a row, columns 0 and
    2^20 - 1 used (by the first and by the last matrix row among others).  With `duplicates` every 97th row of two entries or
    more names its first column twice.  With `with_order` storage row s holds matrix row r_idx[s], r_idx shuffled with
    r_idx[last] = 0.  Returns (host HELL dict -- padding as the converter left it --, r_idx or None, the matrix's COO)."""
    import oracle_api as O
    key = (letter, duplicates, with_order, hack_size, base)
    if key not in _TRANSPOSE:
        rng = np.random.default_rng(2009)
        n_rows, n_cols = 2 ** 17 + 1, 2 ** 20
        lengths = rng.integers(0, 4, n_rows)
        lengths[0] = lengths[-1] = 3
        r = np.repeat(np.arange(n_rows), lengths)
        c = rng.integers(0, n_cols, r.size)
        starts = np.cumsum(lengths) - lengths
        c[starts[0]], c[starts[-1]] = 0, 0
        c[starts[0] + 2], c[starts[-1] + 2] = n_cols - 1, n_cols - 1
        c[starts[5] if lengths[5] else starts[6]] = 2 ** 16
        order = np.lexsort((c, r))                            # ascending columns inside a row
        c = c[order]
        again = np.flatnonzero(lengths >= 2)[::97]
        if duplicates:
            c[starts[again] + 1] = c[starts[again]]
        else:                                                 # distinct columns: a repeat by chance moves up by one
            for _ in range(3):
                same = np.flatnonzero((np.diff(c) <= 0) & (np.diff(r) == 0)) + 1
                c[same] = c[same - 1] + 1
            assert c.max() < n_cols and not ((np.diff(c) <= 0) & (np.diff(r) == 0)).any()
        v = integer_values(rng, r.size, letter)
        r_idx = None
        s = r
        if with_order:
            r_idx = rng.permutation(n_rows).astype(np.int32)
            at = int(np.flatnonzero(r_idx == 0)[0])
            r_idx[at], r_idx[-1] = r_idx[-1], 0
            inverse = np.empty(n_rows, np.int64)
            inverse[r_idx] = np.arange(n_rows)
            s = inverse[r]
        by_storage = np.argsort(s, kind="stable")
        ell = O.oracle_converters.coo_to_ell(n_rows, (s[by_storage] + base).astype(np.int32), (c[by_storage] + base).astype(np.int32),
                                             v[by_storage], coo_base=base, ell_base=base)
        hell = O.oracle_converters.ell_to_hell(ell, hack_size)
        _TRANSPOSE[key] = (hell, ell, r_idx, (r, c, v), dict(n_rows=n_rows, n_cols=n_cols, row_bits=18, col_bits=21))
    return _TRANSPOSE[key]


# ---- the references: Python int keys in a dict ---------------------------------------------------------------------------------
def assemble_by_the_book(case, vals, letter, coo_base, csr_base):
    """(row_ptr, perm, seg_ptr, cols, vals, largest key) from a dict keyed by (row << colBits) | column."""
    shift = case["col_bits"]
    lists = {}
    for at, (r, c) in enumerate(zip(case["rows"].tolist(), case["cols"].tolist())):      # ascending COO position
        lists.setdefault((r << shift) | c, []).append(at)
    perm, seg_ptr, out_cols, sums = [], [0], [], []
    per_row = np.zeros(case["n_rows"] + 1, np.int64)
    for key in sorted(lists):
        perm.extend(lists[key])
        seg_ptr.append(len(perm))
        out_cols.append((key & ((1 << shift) - 1)) + csr_base)
        per_row[(key >> shift) + 1] += 1
        terms = [_parts(vals[at]) for at in lists[key]]
        sums.append((sum(t[0] for t in terms), sum(t[1] for t in terms)))
    row_ptr = np.cumsum(per_row) + csr_base
    return (row_ptr.astype(np.int32), np.array(perm, np.int32), np.array(seg_ptr, np.int32), np.array(out_cols, np.int64).astype(np.int32),
            _elements(sums, letter), max(lists))


def spgemm_by_the_book(a, b, base, col_bits, letter):
    """(products, c_ptr, c_cols, c_vals, largest key) of C = A B from a dict keyed by (i << colBits) | j, products added in the
    storage order of A's row."""
    a_ptr, a_cols, a_vals = (x.tolist() for x in a)
    b_ptr, b_cols, b_vals = b[0].tolist(), b[1].tolist(), [_parts(x) for x in b[2]]
    sums, products = {}, 0
    for i in range(len(a_ptr) - 1):
        for e in range(a_ptr[i] - base, a_ptr[i + 1] - base):
            k = a_cols[e] - base
            ar, ai = _parts(a_vals[e])
            for q in range(b_ptr[k] - base, b_ptr[k + 1] - base):
                br, bi = b_vals[q]
                key = (i << col_bits) | (b_cols[q] - base)
                re, im = sums.get(key, (0, 0))
                sums[key] = (re + ar * br - ai * bi, im + ar * bi + ai * br)
                products += 1
    keys = sorted(sums)
    per_row = np.zeros(len(a_ptr), np.int64)
    for key in keys:
        per_row[(key >> col_bits) + 1] += 1
    c_cols = np.array([(key & ((1 << col_bits) - 1)) + base for key in keys], np.int64).astype(np.int32)
    return products, (np.cumsum(per_row) + base).astype(np.int32), c_cols, _elements([sums[key] for key in keys], letter), max(keys)


def transposed_by_the_book(hell, r_idx, row_bits):
    """(rows of A^T, columns of A^T, values, largest key): the stored entries in a dict keyed by (column << rowBits) | matrix row; one
    matrix row is one storage row, so a key's entries arrive by ascending slot."""
    hs, base = hell["hack_size"], hell["base"]
    offsets, lengths, indices = hell["hack_offsets"].tolist(), hell["row_lengths"].tolist(), hell["indices"].tolist()
    order = None if r_idx is None else r_idx.tolist()
    lists = {}
    for r in range(hell["rows"]):
        i = r if order is None else order[r]
        first = offsets[r // hs] + r % hs
        for k in range(lengths[r]):
            slot = first + k * hs
            lists.setdefault(((indices[slot] - base) << row_bits) | i, []).append(slot)
    t_rows, t_cols, slots = [], [], []
    for key in sorted(lists):
        for slot in lists[key]:
            t_rows.append(key >> row_bits)
            t_cols.append(key & ((1 << row_bits) - 1))
            slots.append(slot)
    return np.array(t_rows, np.int32), np.array(t_cols, np.int32), hell["values"][slots], max(lists)


def _same(names, got, want, case):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, case)


def _wide(largest, case, width):
    assert case["row_bits"] + case["col_bits"] == width and largest >= 2 ** 32 and top_bit(largest) < width, (largest, width)


# ---- assembly -----------------------------------------------------------------------------------------------------------------
ASSEMBLY_NAMES = ("row_ptr", "perm", "seg_ptr", "cols", "vals")


def _assembly_check(case, letter, coo_base, csr_base, seed):
    vals = integer_values(np.random.default_rng(seed), case["rows"].size, letter)
    assert bits_for(case["n_rows"]) == case["row_bits"] and bits_for(case["n_cols"]) == case["col_bits"]
    got = formats.coo_assemble(case["n_rows"], case["n_cols"], case["rows"] + coo_base, case["cols"] + coo_base, vals, coo_base, csr_base)
    *want, largest = assemble_by_the_book(case, vals, letter, coo_base, csr_base)
    _same(ASSEMBLY_NAMES, got, want, (letter, coo_base, csr_base))
    assert np.diff(got[2]).max() > 1 and got[3].size < case["rows"].size          # there are duplicates to add
    return got, largest


@pytest.mark.parametrize("letter", "SZ")
def test_assembly_of_narrow_rows_and_widest_columns(letter):
    case = assembly_narrow_rows_widest_columns()
    for coo_base, csr_base in BASE_PAIRS:
        got, largest = _assembly_check(case, letter, coo_base, csr_base, 1)
        _wide(largest, case, 38)
        assert top_bit(largest) == 37 and int(case["cols"].max()) + 1 == W == int(got[3].max()) - csr_base + 1
        if coo_base:
            assert int((case["cols"] + coo_base).max()) == 2 ** 31 - 1             # the largest index an int holds
    cols, rows = set(case["cols"][case["rows"] == 3].tolist()), set(case["rows"][case["cols"] == 0].tolist())
    assert all(5 ^ (1 << k) in cols for k in range(16, 31)) and 5 in cols          # equal in bits 0 .. 15
    assert all(r in rows and r + 64 in rows for r in range(6))                     # equal below the top row bit


def test_assembly_with_both_halves_wide():
    case = assembly_both_halves_wide()
    got, largest = _assembly_check(case, "D", 1, 0, 2)
    _wide(largest, case, 40)
    assert largest == ((2 ** 18) << 21) | 2 ** 20 and top_bit(largest) == 39
    assert {0, 2 ** 18} <= set(case["rows"].tolist()) and {0, 2 ** 20} <= set(case["cols"].tolist())


@pytest.mark.parametrize("n_rows,n_cols", POWER_OF_TWO_SHAPES)
def test_assembly_around_a_power_of_two(n_rows, n_cols):
    case = assembly_around_a_power_of_two(n_rows, n_cols)
    got, largest = _assembly_check(case, "D", 0, 1, 3)
    width = 32 + (n_rows > 2 ** 16) + (n_cols > 2 ** 16)
    assert case["row_bits"] + case["col_bits"] == width and largest == ((n_rows - 1) << case["col_bits"]) | (n_cols - 1)
    if width == 32:
        assert largest == 2 ** 32 - 1                                              # the 32-bit side of the step: every bit set
    else:
        _wide(largest, case, width)
        assert top_bit(largest) == width - 1
    pairs = set(zip(case["rows"].tolist(), case["cols"].tolist()))
    assert (n_rows - 1, n_cols - 1) in pairs and (n_rows - 1, 0) in pairs


@pytest.mark.parametrize("base", [0, 1])
def test_assembly_refusals_at_width(base):
    case = refused_assembly_list(base)
    got, largest = _assembly_check(case, "D", base, base, 4)
    _wide(largest, case, 38)
    for bad_row, bad_col in ((None, base + case["n_cols"]), (base + 70, None)):
        rows, cols = case["rows"] + base, case["cols"] + base
        if bad_col is not None:
            assert bad_col <= 2 ** 31 - 1
            cols[1234] = bad_col
        else:
            rows[1234] = bad_row
        with pytest.raises(ValueError):
            formats.coo_assemble(70, case["n_cols"], rows, cols, np.ones(2000), base, base)


# ---- SpGEMM --------------------------------------------------------------------------------------------------------------------
SPGEMM_NAMES = ("c_ptr", "c_cols", "c_vals")


def _spgemm_check(a, b, n_b_cols, base, letter, col_bits):
    got = formats.csr_spgemm(*a, *b, n_b_cols, base)
    products, *want, largest = spgemm_by_the_book(a, b, base, col_bits, letter)
    assert got[0] == products
    _same(SPGEMM_NAMES, got[1:], want, (letter, base))
    return got, largest


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
def test_spgemm_with_the_widest_b(letter, base):
    case = spgemm_widest_b(letter, base)
    got, largest = _spgemm_check(case["a"], case["b"], W, base, letter, 31)
    _wide(largest, case, 38)
    assert bits_for(70) == 7 and bits_for(W) == 31 and largest == (case["last"] << 31) | (W - 1)     # row 69 of A is empty
    assert int(got[2].max()) - base == W - 1 and got[0] > got[2].size


def test_spgemm_with_many_rows_and_scans_that_carry():
    case = spgemm_many_rows()
    n_rows = case["a"][0].size - 1
    got, largest = _spgemm_check(case["a"], case["b"], case["n_b_cols"], 0, "D", 21)
    _wide(largest, case, 40)
    assert bits_for(n_rows) == 19 and bits_for(case["n_b_cols"]) == 21 and largest == ((2 ** 18) << 21) | 2 ** 20
    assert n_rows + 1 > SCAN_CARRY and got[0] > SCAN_CARRY


@pytest.mark.parametrize("base", [0, 1])
def test_spgemm_refusals_at_width(base):
    (case, k), n_b_cols = refused_spgemm_pair(base), W - 1
    got, largest = _spgemm_check(case["a"], case["b"], n_b_cols, base, "D", 31)
    _wide(largest, case, 38)
    for kind, b in bad_rows_of_b(case["b"], k, base, n_b_cols).items():
        with pytest.raises(ValueError):
            formats.csr_spgemm(*case["a"], *b, n_b_cols, base)


def bad_rows_of_b(b, k, base, n_b_cols):
    """{kind: B with row k spoiled}: a column at base + bColumnsCount; 2^30 + 1 in front of 2^30; a column above 2^16 twice."""
    first = int(b[0][k]) - base
    out = {}
    for kind, pair in (("column at base + bColumnsCount", None), ("row descends in its high bits", (2 ** 30 + 1, 2 ** 30)),
                       ("row repeats a column above 2^16", (2 ** 16 + 5, 2 ** 16 + 5))):
        cols = b[1].copy()
        if pair is None:
            assert base + n_b_cols <= 2 ** 31 - 1
            cols[int(b[0][k + 1]) - base - 1] = base + n_b_cols
        else:
            cols[first], cols[first + 1] = pair[0] + base, pair[1] + base
        out[kind] = (b[0], cols, b[2])
    return out


@pytest.mark.parametrize("base", [0, 1])
def test_spgemm_chain_through_wide_columns(base):
    """Not wide in its keys (7 + 21 and 7 + 7 bits): the second product reads column indices up to 2^20 as aColIndices."""
    case = spgemm_chain(base)
    first, _ = _spgemm_check(case["a"], case["b"], case["n_mid"], base, "D", 21)
    assert int(first[2].max()) - base == 2 ** 20 and bits_for(70) + bits_for(case["n_mid"]) == 28
    second, _ = _spgemm_check(first[1:], case["c"], 90, base, "D", 7)
    lengths = np.diff(case["c"][0])
    assert (lengths == 0).sum() > 2 ** 20 - 20 and lengths[[0, 2 ** 16, 2 ** 20]].all() and second[2].size > 70


# ---- transpose -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter,with_order", [("D", False), ("D", True), ("S", False), ("S", True)])
def test_transposed_listing_with_both_halves_wide(letter, with_order):
    hell, _, r_idx, (r, c, v), case = transpose_source(letter, with_order=with_order)
    got = formats.hell_transposed_coo(hell, r_idx)
    *want, largest = transposed_by_the_book(hell, r_idx, 18)
    _same(("t_rows", "t_cols", "t_vals"), got, want, (letter, with_order))
    assert bits_for(case["n_rows"]) == 18 and bits_for(case["n_cols"] + 1) == 21
    _wide(largest, case, 39)
    assert largest == ((2 ** 20 - 1) << 18) | 2 ** 17 and top_bit(largest) == 37              # the last column, in the last matrix row
    assert got[0][0] == 0 and got[0][-1] == 2 ** 20 - 1 and case["n_cols"] + 1 > SCAN_CARRY
    twice = np.flatnonzero((np.diff(got[0]) == 0) & (np.diff(got[1]) == 0))
    assert twice.size > 100 and (got[2][twice] != got[2][twice + 1]).any()                  # duplicates, kept apart
    if with_order:
        assert r_idx[-1] == 0 and sorted(r_idx.tolist()) == list(range(case["n_rows"]))
    else:
        order = np.lexsort((r, c))                                                         # stable: duplicates keep their slot order
        assert got[0].tobytes() == c[order].astype(np.int32).tobytes() and got[2].tobytes() == v[order].tobytes()
