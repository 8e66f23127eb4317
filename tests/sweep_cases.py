"""Matrices, colourings and independent checks shared by the sweep tests (include/spgpu/ext/sweep_device.h).  A case is a list of
rows, rows[i] = [(column, value), ...] in the order stored, with a colouring written by hand (colour_of); the CSR arrays come from
aggregate_cases.from_rows.  The cases are the smallest at which a branch of the device code can go wrong.  sweep_literal and
residual_literal restate the contract row by row on those lists, in the element type's own scalar arithmetic; they share nothing
with spgpu_amd.formats.  Nothing here imports the device code."""
import numpy as np

from aggregate_cases import from_rows

FORWARD, BACKWARD, SYMMETRIC = 0, 1, 2


def _values(rows, seed, dtype):
    """The pattern with random values: off-diagonals in (-1, 1), a diagonal that dominates its row; complex types get both parts."""
    rng = np.random.default_rng(seed)
    cx = np.dtype(dtype).kind == "c"
    out = []
    for i, row in enumerate(rows):
        new = []
        for c, _ in row:
            v = rng.uniform(-1, 1) + (1j * rng.uniform(-1, 1) if cx else 0)
            if c == i:
                v = len(row) + 1 + rng.uniform(0, 1) + (1j * rng.uniform(-1, 1) if cx else 0)
            new.append((c, v))
        out.append(new)
    return out


def diagonal(n=6):
    return [[(i, 1.0)] for i in range(n)], [0] * n


def chain(n):
    """The tridiagonal pattern, red-black: two colours (one for n = 1)."""
    return [[(j, 1.0) for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)], [i % 2 for i in range(n)]


def grid5_unsorted(g=4):
    """The 5-point pattern of a g x g grid, red-black, the columns of a row rotated by the row number: the diagonal comes first,
    last and in the middle of its row."""
    rows, colour = [], []
    for i in range(g * g):
        x, y = i % g, i // g
        cols = [j for j, ok in ((i - g, y > 0), (i - 1, x > 0), (i, True), (i + 1, x < g - 1), (i + g, y < g - 1)) if ok]
        k = i % len(cols)
        rows.append([(c, 1.0) for c in cols[k:] + cols[:k]])
        colour.append((x + y) % 2)
    firsts = {[c for c, _ in r].index(i) for i, r in enumerate(rows)}
    assert 0 in firsts and any([c for c, _ in r][-1] == i for i, r in enumerate(rows)) and len(firsts) >= 3
    return rows, colour


def arrow(n=20):
    """Row 0 is full (n entries: longer than one chunk of 8, shorter than 32), the others store their diagonal and column 0."""
    return [[(j, 1.0) for j in range(n)]] + [[(0, 1.0), (i, 1.0)] for i in range(1, n)], [0] + [1] * (n - 1)


def hubs(lengths=(8, 9, 32, 33)):
    """Hub rows of exactly the given numbers of entries (a diagonal in the middle and leaves), and leaves that store their diagonal
    and hub 0: a whole chunk, a chunk and one, for groups of 8 and of 32."""
    h = len(lengths)
    n = h + max(lengths) - 1
    rows = []
    for k, length in enumerate(lengths):
        leaves = [(h + j, 1.0) for j in range(length - 1)]
        rows.append(leaves[:length // 2] + [(k, 1.0)] + leaves[length // 2:])
    rows += [[(i, 1.0), (0, 1.0)] for i in range(h, n)]
    assert [len(r) for r in rows[:h]] == list(lengths)
    return rows, [0] * h + [1] * (n - h)


def twice(n=5):
    """The chain with the off-diagonal column 1 of row 2 stored twice."""
    rows, colour = chain(n)
    rows[2] = [(1, 1.0), (2, 1.0), (1, 1.0), (3, 1.0)]
    return rows, colour


def joined(parts):
    """Block-diagonal join of (rows, colour_of) cases; the colours of a block come after those of the block before."""
    rows, colour, shift, first = [], [], 0, 0
    for part_rows, part_colour in parts:
        rows += [[(c + shift, v) for c, v in r] for r in part_rows]
        colour += [c + first for c in part_colour]
        shift += len(part_rows)
        first += max(part_colour) + 1
    return rows, colour


def mixed():
    """Narrow, wide, wide, narrow colours: chain of 5 | tridiagonal of 600 (300 rows a colour) | chain of 7: colour sizes 3, 2, 300,
    300, 4, 3 -- chained and plain segments mix, forwards and backwards."""
    return joined([chain(5), chain(600), chain(7)])


def empty_row_case():
    """For the residual only: row 1 stores nothing, row 3 lacks its diagonal."""
    return [[(0, 2.0), (1, 1.0)], [], [(2, 3.0), (0, 1.0)], [(0, 1.0), (2, -1.0)]], None


CASES = {"diagonal": diagonal, "row1": lambda: chain(1), "chain5": lambda: chain(5), "grid5_unsorted": grid5_unsorted,
         "tridiagonal600": lambda: chain(600), "arrow20": arrow, "hubs": hubs, "twice": twice, "mixed": mixed}


def build(name, dtype=np.float64, base=0, seed=0):
    """-> (rows with values, (row_ptr, col, vals), colours, colour_of, order, colour_ptr) of a named case."""
    rows, colour = CASES[name]()
    rows = _values(rows, 100 + seed, dtype)
    colour_of = np.array(colour, np.int32)
    colours = int(colour_of.max()) + 1
    order = np.array(sorted(range(len(rows)), key=lambda i: (colour[i], i)), np.int32)
    colour_ptr = np.array([int((colour_of < c).sum()) for c in range(colours + 1)], np.int32)
    return rows, from_rows(rows, base, dtype), colours, colour_of, order, colour_ptr


def vectors(n, dtype, seed=0):
    """(b, x) of n elements: a random right-hand side and a random guess."""
    rng = np.random.default_rng(500 + seed)
    make = lambda: (rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(dtype).kind == "c" else 0)).astype(dtype)
    return make(), make()


def permuted(rows, order):
    """B = A(order, order) as lists of rows: row k is row order[k], columns renamed, ascending (equal columns in storage order)."""
    inverse = {int(r): k for k, r in enumerate(order)}
    return [sorted(((inverse[c], v) for c, v in rows[int(r)]), key=lambda cv: cv[0]) for r in order]


# ---- the contract, row by row on the lists ------------------------------------------------------------------------------------
def _parts(z, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind != "c":
        return [dtype.type(z)]
    part = np.float32 if dtype == np.complex64 else np.float64
    z = dtype.type(z)
    return [part(z.real), part(z.imag)]


def _mul(a, b):
    if len(a) == 1:
        return [a[0] * b[0]]
    rr, ii, ri, ir = a[0] * b[0], a[1] * b[1], a[0] * b[1], a[1] * b[0]
    return [rr - ii, ri + ir]


def _div(n, d):
    if len(n) == 1:
        return [n[0] / d[0]]
    den = d[0] * d[0] + d[1] * d[1]
    top, bottom = n[0] * d[0] + n[1] * d[1], n[1] * d[0] - n[0] * d[1]
    return [top / den, bottom / den]


def _join(parts, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind != "c":
        return np.array([p[0] for p in parts], dtype)
    part = np.float32 if dtype == np.complex64 else np.float64
    return np.array([[p[0], p[1]] for p in parts], part).reshape(-1).view(dtype) if parts else np.zeros(0, dtype)


def sweep_literal(rows, colour_of, b, x, dtype, direction=FORWARD, omega=None):
    """x after one sweep, by the words of the contract: every colour of the direction, every row of it, every stored entry whose
    column is not the row (a sound matrix stores one diagonal, so that is the entry at diagPos)."""
    colours = max(colour_of) + 1
    xs = [_parts(v, dtype) for v in x]
    bs = [_parts(v, dtype) for v in b]
    w = None if omega is None else _parts(omega, dtype)
    up, down = list(range(colours)), list(range(colours - 1, -1, -1))
    with np.errstate(all="ignore"):
        for c in {FORWARD: up, BACKWARD: down, SYMMETRIC: up + down}[direction]:
            for i in [k for k in range(len(rows)) if colour_of[k] == c]:
                acc, pivot = bs[i], None
                for col, val in rows[i]:
                    if col == i:
                        pivot = _parts(val, dtype)
                        continue
                    p = _mul(_parts(val, dtype), xs[col])
                    acc = [s - t for s, t in zip(acc, p)]
                g = _div(acc, pivot)
                if w is not None:
                    d = [s - t for s, t in zip(g, xs[i])]
                    g = [s + t for s, t in zip(xs[i], _mul(w, d))]
                xs[i] = g
    return _join(xs, dtype)


def residual_literal(rows, b, x, dtype):
    xs = [_parts(v, dtype) for v in x]
    out = []
    with np.errstate(all="ignore"):
        for i, row in enumerate(rows):
            acc = _parts(b[i], dtype)
            for col, val in row:
                acc = [s - t for s, t in zip(acc, _mul(_parts(val, dtype), xs[col]))]
            out.append(acc)
    return _join(out, dtype)


# ---- what the Plan refuses: (name, rows, colour_of) with the chain of 6 as the sound matrix --------------------------------------
def refusals():
    out = []
    rows, colour = chain(6)
    bad = [list(r) for r in rows]
    bad[3] = [(2, 1.0), (3, 1.0), (6, 1.0)]
    out.append(("a column outside the matrix", bad, colour))
    bad = [list(r) for r in rows]
    bad[2] = [(1, 1.0), (3, 1.0)]
    out.append(("a row without its diagonal", bad, colour))
    bad = [list(r) for r in rows]
    bad[4] = [(3, 1.0), (4, 1.0), (4, 2.0), (5, 1.0)]
    out.append(("a diagonal stored twice", bad, colour))
    bad = [list(r) for r in rows]
    bad[0] = [(0, 1.0), (1, 1.0), (2, 1.0)]
    out.append(("two nodes of one colour joined", bad, colour))
    return out


def unsymmetric_pair():
    """Row 0 stores its diagonal, row 1 its diagonal and column 0: node 0 has no neighbour and node 1 has the larger tuple, so the
    colouring gives both colour 0 in its first round, and the stored entry (1, 0) joins two nodes of one colour."""
    return [[(0, 2.0)], [(1, 2.0), (0, -1.0)]]
