"""The COO listings that tests/test_coo_convert_restated.py (CPU) and tests/test_gpu_zz_coo_convert_shapes.py (GPU) share: inputs of
the device-side COO converters of include/spgpu/convert_device.h (COO -> ELL / HELL / HDIA / DIA), each built to sit on one
threshold of those converters -- a tile edge or the carry of the three-launch scan (1 024-element tiles, scanTotalsKernel loops
beyond 256 of them), the width of the row sort key, the 32-bit edge of the HDIA diagonal key, a slot with many writers.

Every builder returns a Case: (n_rows, n_cols, rows, cols, vals, coo_base, info).  rows and cols are int32 and carry coo_base;
vals[e] is e + 1 (imaginary part -(e + 1)) in the case's type: non-zero, distinct per entry, and it names the COO position, so the
bytes of a stored value tell which entry was stored.  info holds what the threshold needs (hack size, the spoilt listings, ...)."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "n_rows n_cols rows cols vals coo_base info")

DTYPES = {"S": np.float32, "D": np.float64, "C": np.complex64, "Z": np.complex128}
W = 2 ** 31 - 1                  # the widest matrix: with base 1 its last column index is INT_MAX
TILE = 1024                      # elements per tile of the three-launch exclusive scan (convert_scan.hip.h)
CARRY_TILES = 256                # tile totals one round of scanTotalsKernel takes; beyond them it loops with a carry
BASE_PAIRS = ((0, 0), (0, 1), (1, 0), (1, 1))        # (cooBaseIndex, ellBaseIndex / hellBaseIndex)


def tiles(n):
    return (n + TILE - 1) // TILE


def values(count, letter):
    dtype = np.dtype(DTYPES[letter])
    at = np.arange(1, count + 1)
    assert count < 2 ** 24                                   # exact in fp32
    return (at - 1j * at).astype(dtype) if dtype.kind == "c" else at.astype(dtype)


def _case(n_rows, n_cols, r0, c0, letter, coo_base, rng=None, **info):
    """0-based rows / columns (any integer type) -> a Case; shuffled with `rng` when one is given."""
    r0, c0 = np.asarray(r0, np.int64), np.asarray(c0, np.int64)
    if rng is not None:
        order = rng.permutation(r0.size)
        r0, c0 = r0[order], c0[order]
    assert r0.size == 0 or (r0.min() >= 0 and r0.max() < n_rows and c0.min() >= 0 and c0.max() < n_cols)
    assert r0.size == 0 or max(int(r0.max()), int(c0.max())) + coo_base <= 2 ** 31 - 1
    return Case(n_rows, n_cols, (r0 + coo_base).astype(np.int32), (c0 + coo_base).astype(np.int32), values(r0.size, letter), coo_base, info)


def with_entries(case, rows=None, cols=None, **info):
    """The case with other index arrays (a spoilt listing)."""
    return case._replace(rows=case.rows if rows is None else rows, cols=case.cols if cols is None else cols, info=dict(case.info, **info))


def reversed_listing(case):
    """The same entries in the opposite COO order; every value stays with its entry."""
    return case._replace(rows=case.rows[::-1].copy(), cols=case.cols[::-1].copy(), vals=case.vals[::-1].copy())


def retyped(case, letter):
    return case._replace(vals=values(case.rows.size, letter))


def _rows_of_lengths(rng, lengths, n_cols, duplicates=True):
    """Entries of rows with the given lengths, columns drawn from few values so that (row, column) pairs repeat."""
    r = np.repeat(np.arange(lengths.size), lengths)
    c = rng.integers(0, min(n_cols, 12) if duplicates else n_cols, r.size)
    return r, c


# ---- ELL / HELL ------------------------------------------------------------------------------------------------------------------
def ell_base_pairs(letter, coo_base):
    """1. 70 rows x 90 columns, rows of 0 to 9 entries, rows 5, 32 and 40 empty, the first and the last row not; shuffled, and with
    twelve columns to draw from most rows name a column twice."""
    rng = np.random.default_rng(3100 + coo_base)
    lengths = rng.integers(0, 10, 70)
    lengths[[5, 32, 40]] = 0
    lengths[[0, 69]] = (4, 9)
    r, c = _rows_of_lengths(rng, lengths, 90)
    c[::7] = 89
    return _case(70, 90, r, c, letter, coo_base, rng, empty_rows=(5, 32, 40), hack_sizes=(32, 96))


ROW_COUNTS = (255, 256, 257, 65535, 65536, 65537)           # 2^k - 1, 2^k, 2^k + 1: the sort key `rows` needs 8, 9, 9, 16, 17, 17 bits


def row_key_bits(n_rows):
    """Bits of the row sort of spgpuCooRowLengthsDevice: the smallest b with 2^b > rows (keys 0 .. rows, `rows` = outside)."""
    return max(1, int(n_rows).bit_length())


def ell_row_counts(n_rows, coo_base):
    """2. 400 entries in rows drawn at random with duplicates, among them rows 0 and rows - 1 and the rows either side of every power
    of two below rows.  info: the listing with one row index at base + rows and with one at base - 1 (position 123)."""
    rng = np.random.default_rng(3200 + n_rows + coo_base)
    edges = sorted({0, n_rows - 1} | {p + d for k in range(1, 17) for p in (2 ** k,) for d in (-1, 0) if p + d < n_rows})
    r = np.concatenate((edges, rng.integers(0, n_rows, 400 - len(edges))))
    c = rng.integers(0, 50, r.size)
    case = _case(n_rows, 50, r, c, "D", coo_base, rng, key_bits=row_key_bits(n_rows))
    high, low = case.rows.copy(), case.rows.copy()
    high[123], low[123] = coo_base + n_rows, coo_base - 1
    return with_entries(case, row_too_high=high, row_too_low=low)


def ell_wide_columns(coo_base):
    """3. 70 rows x (2^31 - 1) columns: column indices up to 2^31 - 2 at base 0 and 2^31 - 1 (INT_MAX) at base 1."""
    rng = np.random.default_rng(3300 + coo_base)
    pool = np.array([0, 1, 2 ** 16 - 1, 2 ** 16, 2 ** 30, 2 ** 30 + 1, W - 3, W - 2, W - 1], np.int64)
    lengths = rng.integers(0, 8, 70)
    lengths[[0, 69]] = 5
    r = np.repeat(np.arange(70), lengths)
    c = pool[rng.integers(0, pool.size, r.size)]
    c[:5] = (W - 1, 0, W - 2, 2 ** 30, W - 1)              # row 0 names the last column twice
    c[-1] = W - 1
    return _case(70, W, r, c, "D", coo_base, rng, hack_sizes=(32,))


HELL_PLAN_HACKS = (1, 1023, 1024, 1025)
HELL_CARRY = dict(hack_size=2, n_rows=524293)               # 262 147 hacks: 257 tiles


def hell_plan_hacks(hacks, hack_size=32):
    """4. A matrix of `hacks` hacks (the last one partly filled), rows of 0 to 3 entries, a non-empty row in the first and in the
    last hack: spgpuHellPlanDevice scans one depth per hack."""
    n_rows = hacks * hack_size - (hack_size > 1) * (hack_size // 4)
    return _hell_plan_case(n_rows, hack_size, 0.4)


def hell_plan_carry():
    """4. Hack size 2 and 524 293 rows: 262 147 hacks, 257 tiles -- one more than a round of scanTotalsKernel takes.  Nine rows in
    ten are empty, which keeps the restatement in Python to about a second."""
    return _hell_plan_case(HELL_CARRY["n_rows"], HELL_CARRY["hack_size"], 0.9)


def _hell_plan_case(n_rows, hack_size, empty):
    rng = np.random.default_rng(3400 + n_rows)
    lengths = rng.choice(4, n_rows, p=(empty, (1 - empty) / 2, (1 - empty) / 4, (1 - empty) / 4))
    lengths[0], lengths[-1] = 2, 3
    r, c = _rows_of_lengths(rng, lengths, 1000, duplicates=False)
    hacks = (n_rows + hack_size - 1) // hack_size
    return _case(n_rows, 1000, r, c, "D", n_rows % 2, rng, hack_size=hack_size, hacks=hacks, scan_tiles=tiles(hacks))


def ell_degenerate(kind):
    """5. "no entries": 70 rows and an empty listing; "no rows": nothing at all; "one entry": 70 rows and the entry (37, 11)."""
    none = np.zeros(0, np.int64)
    if kind == "no entries":
        return _case(70, 90, none, none, "D", 1)
    if kind == "no rows":
        return _case(0, 0, none, none, "D", 0)
    return _case(70, 90, [37], [11], "D", 1)


# ---- HDIA ------------------------------------------------------------------------------------------------------------------------
HDIA_HACK_SIZES = (32, 64, 96, 24)                          # 24: no multiple of 32; the host converter accepts any positive size


def hdia_row_counts(hack_size):
    return (1, hack_size - 1, hack_size, hack_size + 1, 3 * hack_size + 5)


def _on_diagonals(rows, offsets, n_cols, rng, fill=0.7):
    r = np.concatenate([rows for _ in offsets] + [np.zeros(0, np.int64)])
    c = np.concatenate([rows + d for d in offsets] + [np.zeros(0, np.int64)])
    keep = (c >= 0) & (c < n_cols) & (rng.random(r.size) < fill)
    return r[keep], c[keep]


def hdia_shape(hack_size, n_rows, letter, coo_base, wide):
    """6. rows x (rows + 13) (`wide`) or rows x max(rows - 7, 1): the entries (rows - 1, 0) and (0, cols - 1) -- the offsets
    -(rows - 1) and cols - 1 --, partly filled diagonals, twelve entries named twice, shuffled.  With 3 * hackSize + 5 rows there
    are four hacks: hack 1 has no diagonal, hack 2 exactly one (offset 1), hack 3 is five rows deep."""
    rng = np.random.default_rng(3600 + 7 * hack_size + n_rows + coo_base)
    n_cols = n_rows + 13 if wide else max(n_rows - 7, 1)
    if n_rows == 3 * hack_size + 5:
        parts = [_on_diagonals(np.arange(hack_size), (0, 3, -2), n_cols, rng),
                 _on_diagonals(np.arange(2 * hack_size, 3 * hack_size), (1,), n_cols, rng),
                 _on_diagonals(np.arange(3 * hack_size, n_rows), (-9, -3 * hack_size), n_cols, rng, fill=1.0)]
    else:
        parts = [_on_diagonals(np.arange(n_rows), (0, 2, -1), n_cols, rng)]
    r = np.concatenate([p[0] for p in parts] + [[n_rows - 1, 0]])
    c = np.concatenate([p[1] for p in parts] + [[0, n_cols - 1]])
    again = rng.integers(0, r.size, 12)
    return _case(n_rows, n_cols, np.concatenate((r, r[again])), np.concatenate((c, c[again])), letter, coo_base, rng, hack_size=hack_size)


def hdia_single_entry(coo_base):
    """6. nnz == 1: the entry (40, 3) of a 70 x 50 matrix: the second hack's only diagonal, the first hack has none."""
    return _case(70, 50, [40], [3], "D", coo_base, hack_size=32)


HDIA_WIDE_HACK_SIZES = (32, 64)


def hdia_wide(hack_size, coo_base, letter="D"):
    """7. 70 rows x (2^31 - 1) columns.  Column 0 and every column of 2^31 - 2 - hackSize .. 2^31 - 2, from rows at the start, in
    the middle and at the end of their hacks.  The diagonal key's low word, column - row % hackSize + hackSize, is at least 2^31
    for the columns within hackSize - row % hackSize of the end."""
    rng = np.random.default_rng(3700 + hack_size + coo_base)
    rows = sorted({0, 1, hack_size // 2, min(hack_size, 70) - 1, min(hack_size, 69), 35, 69 // hack_size * hack_size, 68, 69})
    last = np.arange(W - 1 - hack_size, W)
    r = np.concatenate([np.full(last.size + 1, row) for row in rows])
    c = np.concatenate([np.append(last, 0) for _ in rows])
    again = rng.integers(0, r.size, 20)
    return _case(70, W, np.concatenate((r, r[again])), np.concatenate((c, c[again])), letter, coo_base, rng, hack_size=hack_size)


def _contended(writers, n, seed, hack_size=None):
    """`writers` entries that all name (n // 2 + 5, n // 2), among the entries of three partly filled diagonals; shuffled."""
    rng = np.random.default_rng(seed)
    r, c = _on_diagonals(np.arange(n), (0, 4, -5), n, rng)
    r = np.concatenate((r, np.full(writers, n // 2 + 5)))
    c = np.concatenate((c, np.full(writers, n // 2)))
    return _case(n, n, r, c, "D", 1, rng, hack_size=hack_size, slot=(n // 2 + 5, n // 2), writers=writers)


def hdia_contention():
    """8. 100 000 entries for one slot of a 200 x 200 matrix, among about 400 others."""
    return _contended(100_000, 200, 3800, hack_size=32)


OUTSIDE = ("row at base + rows", "row at base - 1", "column at base + columns", "column at base - 1")


def spoilt(case, kind, at=17):
    """The listing of `case` with entry `at` moved just outside the matrix."""
    rows, cols = case.rows.copy(), case.cols.copy()
    if kind == "row at base + rows":
        rows[at] = case.coo_base + case.n_rows
    elif kind == "row at base - 1":
        rows[at] = case.coo_base - 1
    elif kind == "column at base + columns":
        cols[at] = case.coo_base + case.n_cols
    else:
        assert kind == "column at base - 1"
        cols[at] = case.coo_base - 1
    return with_entries(case, rows, cols)


def hdia_refused(coo_base):
    """9. A good 101 x 114 matrix (hack size 32); `spoilt` moves one entry of it outside."""
    return hdia_shape(32, 101, "D", coo_base, True)


# ---- DIA -------------------------------------------------------------------------------------------------------------------------
DIA_SPANS = (1023, 1024, 1025, 1026)                        # rows + cols - 1 flags: 1, 1, 2, 2 tiles
DIA_CARRY = dict(n_rows=200001, n_cols=70000)               # 270 000 flags: 264 tiles


def dia_span(span, coo_base, letter="D"):
    """10. 500 rows x (span - 499) columns: the lowest and the highest possible offset and the diagonals at flags 1 022 to 1 025
    where the matrix has them (the last flags of tile 0 and the first of tile 1), partly filled."""
    rng = np.random.default_rng(3900 + span + coo_base)
    n_rows, n_cols = 500, span - 499
    assert n_rows + n_cols - 1 == span
    flags = [f for f in (300, 499, 1022, 1023, 1024, 1025) if f < span - 1]
    r, c = _on_diagonals(np.arange(n_rows), [f - (n_rows - 1) for f in flags], n_cols, rng)
    top = [f - (n_rows - 1) for f in flags if f >= n_rows - 1]                     # row 0 holds every one of them, whatever was kept
    r, c = np.concatenate((r, [n_rows - 1, 0], np.zeros(len(top), np.int64))), np.concatenate((c, [0, n_cols - 1], top))
    again = rng.integers(0, r.size, 12)
    return _case(n_rows, n_cols, np.concatenate((r, r[again])), np.concatenate((c, c[again])), letter, coo_base, rng, span=span,
                 scan_tiles=tiles(span))


def dia_carry():
    """10. 200 001 x 70 000: 270 000 flags.  Eight diagonals: the lowest and the highest possible offset (one entry each), the two
    at flags 262 143 and 262 144 -- the last one of the first round of scanTotalsKernel and the first one of the second -- and
    four long ones with every sixteenth row left out: about 277 000 entries."""
    rng = np.random.default_rng(3950)
    n_rows, n_cols = DIA_CARRY["n_rows"], DIA_CARRY["n_cols"]
    astride = [TILE * CARRY_TILES - 1 - (n_rows - 1), TILE * CARRY_TILES - (n_rows - 1)]
    rows = np.arange(n_rows)
    r, c = _on_diagonals(rows[rows % 16 != 3], astride + [0, -50000, -100000, -130001], n_cols, rng, fill=1.0)
    r, c = np.concatenate((r, [n_rows - 1, 0])), np.concatenate((c, [0, n_cols - 1]))
    return _case(n_rows, n_cols, r, c, "D", 1, rng, span=n_rows + n_cols - 1, scan_tiles=tiles(n_rows + n_cols - 1), astride=astride)


def dia_contention():
    """11. 50 000 entries for one slot of a 300 x 300 matrix, among about 600 others."""
    return _contended(50_000, 300, 3960)


def dia_refused(coo_base):
    """12. A good 500 x 526 matrix; `spoilt` moves one entry of it outside."""
    return dia_span(1025, coo_base)
