"""The matrices that tests/test_ilu0_restated.py (CPU) and tests/test_gpu_zz_ilu0_device.py (GPU) share: whole matrices for the ILU(0) of
include/spgpu/ext/ilu0_device.h, as host CSR arrays with strictly ascending rows that store their diagonal.  Values are diagonally
dominant as in trsv_cases -- off-diagonals scaled by the row length, diagonals of modulus in [1, 2.1) -- so that no pivot is small."""
import numpy as np

import exact_ref as X
import trsv_cases as T
from trsv_cases import from_rows, pivot, values


def row(rng, i, others, letter):
    """Row i: the diagonal and the distinct columns `others`, ascending, dominant."""
    others = np.unique(np.asarray(others, np.int64))
    others = others[others != i]
    cols = np.sort(np.append(others, i))
    vals = values(rng, cols.size, letter, 0.5 / max(others.size, 1))
    vals[cols == i] = pivot(rng, letter)
    return cols, vals


def from_columns(rng, columns, letter, base=0):
    """[off-diagonal columns of row i, ...] -> (ptr, cols, vals) in `base`."""
    return from_rows([row(rng, i, others, letter) for i, others in enumerate(columns)], letter, base)


def random_system(rng, n, letter, base, longest=6):
    """Up to `longest` off-diagonals per row, anywhere on both sides."""
    columns = []
    for i in range(n):
        others = np.setdiff1d(np.arange(n), [i])
        columns.append(rng.choice(others, int(rng.integers(0, min(longest, others.size) + 1)), replace=False))
    return from_columns(rng, columns, letter, base)


def update_counts(ptr, cols, base=0):
    """(updates that hit a stored entry, updates that are dropped) of the ILU(0) of this pattern."""
    ptr, cols = np.asarray(ptr, np.int64) - base, np.asarray(cols, np.int64) - base
    hit = dropped = 0
    for i in range(ptr.size - 1):
        mine = set(cols[ptr[i]:ptr[i + 1]].tolist())
        for k in cols[ptr[i]:ptr[i + 1]]:
            if k >= i:
                break
            upper = [j for j in cols[ptr[k]:ptr[k + 1]].tolist() if j > k]
            here = sum(j in mine for j in upper)
            hit, dropped = hit + here, dropped + len(upper) - here
    return hit, dropped


def rows_around(rng, L, letter, base=0):
    """Rows of L - 1, L, L + 1 and 2 L + 1 stored entries (L >= 2), each once with its entries on both sides, once with no lower part
    and once with no upper part.  Row 0 is only its diagonal; row 1 has an empty upper part and is a dependency of the long rows;
    rows 2 .. 2 L + 2 are the other dependencies, and each stores the long rows' own columns and one of the padding columns behind
    them, so some updates hit (the diagonal of a row without an upper part among them) and some are dropped."""
    lengths = (L - 1, L, L + 1, 2 * L + 1)
    deps = 2 * L + 3
    padding = deps + 3 * len(lengths)
    n = padding + 2 * L + 1
    columns = [[] for _ in range(n)]
    columns[1] = [0]
    for r in range(2, deps):
        columns[r] = [r - 1] + list(range(deps, padding)) + [padding + r % (2 * L + 1)]
    at = deps
    for length in lengths:
        off = length - 1
        below = off // 2
        columns[at] = list(range(1, 1 + below)) + list(range(at + 1, at + 1 + off - below))
        columns[at + 1] = list(range(at + 2, at + 2 + off))
        columns[at + 2] = list(range(1, 1 + off))
        at += 3
    mat = from_columns(rng, columns, letter, base)
    assert np.diff(mat[0])[deps:padding].tolist() == [length for length in lengths for _ in range(3)]
    return mat


def dense_block(rng, n, letter, base=0):
    return from_columns(rng, [np.arange(n)] * n, letter, base)


def from_levels(rng, widths, letter, base=0):
    """A matrix whose level l (of the lower triangle) has exactly widths[l] consecutive rows: every row of level l > 0 stores an
    entry in a row of level l - 1 and up to two more in earlier levels; every row but the last stores the last column and up to one
    more upper entry, so that the updates of the last column hit and the others are mostly dropped.  Returns ((ptr, cols, vals),
    levels as the Plan must find them)."""
    n = int(sum(widths))
    starts = np.concatenate(([0], np.cumsum(widths)))
    level_of = np.repeat(np.arange(len(widths)), widths)
    columns = []
    for r in range(n):
        l = level_of[r]
        others = []
        if l > 0:
            others.append(int(rng.integers(starts[l - 1], starts[l])))
            others += [int(d) for d in rng.integers(0, starts[l], 2)]
        if r < n - 1:
            others += [n - 1, int(rng.integers(r + 1, n))]
        columns.append(others)
    return from_columns(rng, columns, letter, base), level_of


def bidiagonal(rng, n, letter, base=0):
    """Row i stores (i, i - 1) and its diagonal: n levels of one row, and nothing to update."""
    return from_columns(rng, [[i - 1] if i else [] for i in range(n)], letter, base)


def tridiagonal(rng, n, letter, base=0):
    """No fill: ILU(0) is the LU.  Real types: diagonal in [1, 2), each off-diagonal in [-0.25, 0.25), so those of a row sum to at
    most 0.5 in modulus."""
    dtype = X.DTYPE_OF[letter]
    rows = []
    for i in range(n):
        cols = [c for c in (i - 1, i, i + 1) if 0 <= c < n]
        rows.append((cols, [dtype(1 + rng.random()) if c == i else dtype(0.5 * rng.random() - 0.25) for c in cols]))
    return from_rows(rows, letter, base)


def arrow(rng, n, letter, base=0):
    """Diagonal plus a dense last row and last column: no fill either."""
    return from_columns(rng, [[n - 1] for _ in range(n - 1)] + [np.arange(n - 1)], letter, base)


def stencil(rng, g, dims, letter, base=0):
    return T.stencil(g, dims, letter, base, rng)


def dense_of(mat, base=0):
    ptr, cols, vals = mat
    n = ptr.size - 1
    out = np.zeros((n, n), vals.dtype)
    mask = np.zeros((n, n), bool)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    out[rows, cols.astype(np.int64) - base] = vals
    mask[rows, cols.astype(np.int64) - base] = True
    return out, mask


# ---- the arithmetic pins: block-diagonal matrices of 2 x 2 blocks [[d, u], [l, a]], lu's last entry = a - ((l / d) * u) -----------
def blocks(entries, letter, base=0):
    rows = []
    for t, (d, u, l, a) in enumerate(entries):
        rows += [([2 * t, 2 * t + 1], [d, u]), ([2 * t, 2 * t + 1], [l, a])]
    return from_rows(rows, letter, base)


def fused_update_blocks(rng, letter, count=64):
    """d = 1, l = a', u = x', a = round(a' * x') with a' * x' inexact: the update is exactly +0 when the product is rounded first,
    the product's rounding error from one fused multiply-add."""
    from test_spgemm_restated import inexact_pair
    entries = []
    for _ in range(count):
        a, x, p, error = inexact_pair(rng, X.DTYPE_OF[letter])
        assert float(error) != 0
        entries.append((1.0, x, a, p))
    return blocks(entries, letter)


# ---- one fused multiply-add inside the complex product or quotient, emulated with exact fractions ---------------------------------
def rounded(exact, real):
    """The Fraction `exact` rounded to `real`, to nearest, ties to even."""
    from fractions import Fraction
    real = np.dtype(real).type
    near = real(float(exact))
    bits = np.uint32 if real == np.float32 else np.uint64
    candidates = [np.nextafter(near, real(-np.inf)), near, np.nextafter(near, real(np.inf))]
    return min(candidates, key=lambda c: (abs(Fraction(float(c)) - exact), int(real(c).view(bits)) & 1))


def fma(a, b, c, real):
    from fractions import Fraction
    return rounded(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)), real)


PRODUCT_FUSIONS = ("re = fma(ar, xr, -ii)", "re = fma(-ai, xi, rr)", "im = fma(ar, xi, ir)", "im = fma(ai, xr, ri)")
QUOTIENT_FUSIONS = ("top = fma(nr, dr, b)", "top = fma(ni, di, a)", "bottom = fma(ni, dr, -e)", "bottom = fma(-nr, di, c)",
                    "den = fma(dr, dr, ii)", "den = fma(di, di, rr)")


def complex_product(a, x, real, fusion=None):
    """(re, im) of a * x in the six-operation form of the contract, every operation in `real`; with `fusion` (one of
    PRODUCT_FUSIONS) that one multiply is joined to the add or subtract behind it."""
    real = np.dtype(real).type
    ar, ai, xr, xi = real(a.real), real(a.imag), real(x.real), real(x.imag)
    rr, ii, ri, ir = ar * xr, ai * xi, ar * xi, ai * xr
    re = {PRODUCT_FUSIONS[0]: lambda: fma(ar, xr, -ii, real), PRODUCT_FUSIONS[1]: lambda: fma(-ai, xi, rr, real)}.get(fusion, lambda: rr - ii)()
    im = {PRODUCT_FUSIONS[2]: lambda: fma(ar, xi, ir, real), PRODUCT_FUSIONS[3]: lambda: fma(ai, xr, ri, real)}.get(fusion, lambda: ri + ir)()
    return real(re), real(im)


def complex_quotient(n, d, real, fusion=None):
    """(re, im) of n / d in the textbook form of the contract; with `fusion` (one of QUOTIENT_FUSIONS) one multiply is joined."""
    real = np.dtype(real).type
    nr, ni, dr, di = real(n.real), real(n.imag), real(d.real), real(d.imag)
    rr, ii = dr * dr, di * di
    a, b, c, e = nr * dr, ni * di, ni * dr, nr * di
    top = {QUOTIENT_FUSIONS[0]: lambda: fma(nr, dr, b, real), QUOTIENT_FUSIONS[1]: lambda: fma(ni, di, a, real)}.get(fusion, lambda: a + b)()
    bottom = {QUOTIENT_FUSIONS[2]: lambda: fma(ni, dr, -e, real), QUOTIENT_FUSIONS[3]: lambda: fma(-nr, di, c, real)}.get(fusion, lambda: c - e)()
    den = {QUOTIENT_FUSIONS[4]: lambda: fma(dr, dr, ii, real), QUOTIENT_FUSIONS[5]: lambda: fma(di, di, rr, real)}.get(fusion, lambda: rr + ii)()
    with np.errstate(all="ignore"):
        return real(real(top) / real(den)), real(real(bottom) / real(den))


def fused_complex_product_blocks(rng, letter, count=32):
    """d = 1, so the multiplier is l exactly; a = 0, so lu's last entry is minus the product l * u.  With p = round(s * t) and s * t
    inexact, block t aims at PRODUCT_FUSIONS[t % 4]: l and u are chosen so that one component of the product is round(s * t) - p,
    exactly 0 when every operation is rounded, and s * t - p, the rounding error and not 0, when that multiply is fused.  Returns the
    matrix and per block (l, u, the fusion aimed at, the component that is 0: "real" or "imag")."""
    from test_spgemm_restated import inexact_pair
    entries, aims = [], []
    for k in range(count):
        s, t, p, _ = (float(v) for v in inexact_pair(rng, X.REAL_OF[letter]))
        l, u = ((complex(s, p), complex(t, 1)), (complex(p, s), complex(1, t)), (complex(s, -p), complex(1, t)), (complex(-p, s), complex(t, 1)))[k % 4]
        entries.append((complex(1, 0), u, l, complex(0, 0)))
        aims.append((l, u, PRODUCT_FUSIONS[k % 4], "real" if k % 4 < 2 else "imag"))
    return blocks(entries, letter), aims


def complex_quotient_blocks(rng, letter, count=36):
    """The multiplier l / d of block t aims at QUOTIENT_FUSIONS[t % 6].  The first four: l and d are chosen from s, t and
    p = round(s * t) so that the numerator of one component is round(s * t) - p, exactly 0, and the rounding error when that multiply
    is fused.  The last two: l and d are drawn until the fused sum of squares changes a byte of the quotient.  Returns the matrix and
    per block (l, d, the fusion aimed at, the component that is 0 or None)."""
    from test_spgemm_restated import inexact_pair
    real = X.REAL_OF[letter]
    entries, aims = [], []
    for k in range(count):
        kind = k % 6
        if kind < 4:
            s, t, p, _ = (float(v) for v in inexact_pair(rng, real))
            l, d = ((complex(s, -p), complex(t, 1)), (complex(-p, s), complex(1, t)), (complex(p, s), complex(t, 1)), (complex(s, p), complex(1, t)))[kind]
            zero = "real" if kind < 2 else "imag"
        else:
            while True:
                l, d = (complex(float(real(1 + rng.random())), float(real(1 + rng.random()))) for _ in range(2))
                if complex_quotient(l, d, real, QUOTIENT_FUSIONS[kind]) != complex_quotient(l, d, real):
                    break
            zero = None
        entries.append((d, complex(0.25, 0), l, complex(2, 0)))
        aims.append((l, d, QUOTIENT_FUSIONS[kind], zero))
    return blocks(entries, letter), aims


def division_blocks(rng, count=64):
    """fp32: d and l = n with n / d != n * (1 / d).  Returns the matrix, n and d."""
    n, d = T.division_operands(rng, count)
    return blocks([(d[t], 0.25, n[t], 2.0) for t in range(count)], "S"), n, d


def cancellation(letter, big, big_first):
    """Row 2 stores (2, 0), (2, 1) and its diagonal `big`; rows 0 and 1 have unit pivots and store (0, 2) and (1, 2): 1 and big, or
    big and 1.  In ascending k: (big - 1) - big = 0, because big - 1 rounds to big; or (big - big) - 1 = -1."""
    first, second = (big, 1.0) if big_first else (1.0, big)
    return from_rows([([0, 2], [1.0, first]), ([1, 2], [1.0, second]), ([0, 1, 2], [1.0, 1.0, big])], letter)


def lone_negative_zero(letter):
    """Rows without lower entries: a diagonal -0.0 alone, a -0.0 beside an upper entry, a +0.0."""
    return from_rows([([0], [-0.0]), ([1, 2], [-0.0, -0.0]), ([2], [0.0])], letter)
