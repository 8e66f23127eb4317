"""Matrices and independent checks shared by the aggregation tests (include/spgpu/ext/aggregate_device.h): CSR arrays of 5-point
grids, chains, random unsymmetric patterns, a strip of 1025 rows with one long row, the matrix of the threshold edge cases, and the
greedy distance-2 maximal independent set that the rounds must reproduce on a structurally symmetric pattern.  Nothing here imports
the device code; the greedy pass shares nothing with formats.csr_aggregate but the priority."""
import numpy as np


def from_rows(rows, base=0, dtype=np.float64):
    """rows[i] = [(column (0-based), value), ...] in the order stored -> (row_ptr, col, vals) in `base`."""
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([c for r in rows for c, _ in r], np.int64).astype(np.int32) + np.int32(base)
    vals = np.array([v for r in rows for _, v in r], dtype)
    return ptr + np.int32(base), col, vals


def grid_5pt(g, base=0, dtype=np.float64, cx=1.0, cy=1.0):
    """The 5-point matrix of a g x g grid: -cx to the neighbours in x, -cy in y, 2 cx + 2 cy on the diagonal; ascending columns."""
    rows = []
    for i in range(g * g):
        x, y = i % g, i // g
        row = []
        if y > 0:
            row.append((i - g, -cy))
        if x > 0:
            row.append((i - 1, -cx))
        row.append((i, 2 * cx + 2 * cy))
        if x < g - 1:
            row.append((i + 1, -cx))
        if y < g - 1:
            row.append((i + g, -cy))
        rows.append(row)
    return from_rows(rows, base, dtype)


def chain(n, base=0, dtype=np.float64):
    """The tridiagonal matrix (-1, 2, -1) of a chain of n nodes."""
    return from_rows([[(j, 2.0 if j == i else -1.0) for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)], base, dtype)


def random_unsymmetric(rng, n=200, base=0, dtype=np.float64):
    """n rows with 0-4 off-diagonal entries anywhere, most with a diagonal somewhere in the row; the pattern is not symmetric.  Row 0
    is empty, row 1 has no diagonal, row 2 stores a column twice, row 3 descends."""
    rows = []
    for i in range(n):
        k = int(rng.integers(0, 5))
        others = [int(c) for c in rng.integers(0, n, k) if c != i]
        row = [(c, float(rng.integers(1, 8))) for c in others]
        if rng.random() < 0.8:
            row.insert(int(rng.integers(0, len(row) + 1)), (i, float(rng.integers(1, 8))))
        rows.append(row)
    rows[0] = []
    rows[1] = [(5, 2.0), (9, 3.0)]
    rows[2] = [(7, 1.0), (2, 4.0), (7, 5.0)]
    rows[3] = [(90, 1.0), (40, 2.0), (3, 3.0), (1, 6.0)]
    return from_rows(rows, base, dtype)


def strip_1025(base=0, dtype=np.float64):
    """1025 rows (past one workgroup-stride of every shape at one workgroup): row 7 has 200 off-diagonal entries of magnitude 1 --
    longer than any group of lanes --, every other row one to three -- lanes without an entry --, and a unit diagonal."""
    n = 1025
    rows = []
    for i in range(n):
        if i == 7:
            others = [100 + 4 * k for k in range(200)]
        else:
            others = sorted({(i * 37 + 11 * k + 1) % n for k in range(1 + i % 3)} - {i})
        rows.append([(i, 1.0)] + [(c, -1.0) for c in others])
    return from_rows(rows, base, dtype)


def neighbours(row_ptr, col, strong, base):
    """S(i) as a list of sets."""
    ptr = np.asarray(row_ptr, np.int64) - base
    col = np.asarray(col, np.int64) - base
    out = []
    for i in range(ptr.size - 1):
        out.append({int(col[p]) for p in range(ptr[i], ptr[i + 1]) if (strong is None or strong[p]) and col[p] != i})
    return out


def symmetric(S):
    return all(i in S[j] for i in range(len(S)) for j in S[i])


def within_two(S, i):
    """The nodes at distance 1 or 2 from i."""
    out = set(S[i])
    for j in S[i]:
        out |= S[j]
    out.discard(i)
    return out


def greedy_mis2(S, priority):
    """The greedy pass on the squared graph in descending (priority, i): a node is selected when nothing selected lies within
    distance 2.  For a structurally symmetric S."""
    n = len(S)
    order = sorted(range(n), key=lambda i: (int(priority[i]), i), reverse=True)
    selected, blocked = np.zeros(n, bool), np.zeros(n, bool)
    for i in order:
        if blocked[i]:
            continue
        selected[i] = True
        blocked[i] = True
        for j in within_two(S, i):
            blocked[j] = True
    return selected


def threshold_matrix(dtype, base=0):
    """The edge cases of the strength test around rhs = (t * 4) * 4 = 4 at theta = 0.5 (t = 0.25, all powers of two).  Returns
    (row_ptr, col, vals, strong at theta = 0.5, strong at theta = 0, diag_abs), the expectations written by hand."""
    T = np.dtype(dtype).type
    nan, below = T(np.nan), np.nextafter(T(2), T(0))
    rows = [
        # row 0, d = 4:   equality, one ulp below, NaN value, NaN diagonal at the other end, -0.0 against a zero diagonal,
        #                 a missing diagonal at the other end, a column outside the matrix, a stored zero against d = |-0.0|
        [(0, 4.0), (1, 2.0), (2, below), (3, nan), (4, 2.0), (5, -0.0), (6, 1.0), (8 + 3, 2.0), (7, 0.0)],
        [(0, -2.0), (1, 4.0)],                           # row 1: the sign of a_ij does not matter
        [(0, 1.0), (2, 4.0)],                            # row 2: 1 < 4
        [(3, 4.0)],
        [(4, nan), (0, 100.0)],                          # row 4: its own diagonal is NaN
        [(5, 0.0), (0, 0.0)],                            # row 5: zero diagonal, a stored zero is strong
        [(0, 1.0)],                                      # row 6: no diagonal
        [(7, -0.0), (1, 0.5), (7, 4.0)],                 # row 7: the FIRST stored diagonal counts, |-0.0| = +0
    ]
    at_half = [0, 1, 0, 0, 0, 1, 1, 0, 1,   1, 0,   0, 0,   0,   0, 0,   0, 1,   1,   0, 1, 0]
    at_zero = [0, 1, 1, 0, 0, 1, 1, 0, 1,   1, 0,   1, 0,   0,   0, 0,   0, 1,   1,   0, 1, 0]
    diag = np.array([4, 4, 4, 4, np.nan, 0, 0, 0], dtype)
    ptr, col, vals = from_rows(rows, base, dtype)
    return ptr, col, vals, np.array(at_half, np.uint8), np.array(at_zero, np.uint8), diag
