"""The matrices and operands that tests/test_trsv_restated.py (CPU) and tests/test_gpu_zz_trsv_device.py (GPU) share: systems for the
sparse triangular solve of include/spgpu/ext/trsv_device.h, as host CSR arrays.  Values are diagonally dominant -- off-diagonals
scaled by the row length, diagonals in [1, 2] -- so that nothing overflows."""
import numpy as np

import exact_ref as X

LOWER, UPPER = 0, 1
STORED, UNIT = 0, 1


def values(rng, count, letter, scale=1.0):
    parts = 2 if letter in "CZ" else 1
    return (scale * rng.standard_normal(parts * count)).astype(X.REAL_OF[letter]).view(X.DTYPE_OF[letter])


def pivot(rng, letter):
    """A diagonal entry of modulus in [1, 2.1): real part in [1, 2), for the complex types an imaginary part in [-0.5, 0.5)."""
    re = 1 + rng.random()
    return X.DTYPE_OF[letter](complex(re, rng.random() - 0.5) if letter in "CZ" else re)


def from_rows(rows, letter, base=0):
    """[(columns, values), ...] (0-based columns) -> (ptr, cols, vals) in `base`."""
    dtype = X.DTYPE_OF[letter]
    ptr = np.cumsum([0] + [len(c) for c, _ in rows]) + base
    cols = np.concatenate([np.asarray(c, np.int64) for c, _ in rows] + [np.zeros(0, np.int64)]) + base
    vals = np.concatenate([np.asarray(v, dtype) for _, v in rows] + [np.zeros(0, dtype)])
    return ptr.astype(np.int32), cols.astype(np.int32), vals.astype(dtype)


def random_system(rng, n, letter, base, side, diag, longest=6, poison=True):
    """A whole matrix with entries on both sides of the diagonal in shuffled storage order, and a right-hand side.  Under STORED
    every row stores its diagonal once; under UNIT a third of the rows store nothing at all, a third store a diagonal and a third
    do not.  With `poison` every entry the solve must not read -- the other side, and the diagonal under UNIT -- is NaN."""
    dtype = X.DTYPE_OF[letter]
    nan = dtype(complex(np.nan, np.nan)) if letter in "CZ" else dtype(np.nan)
    rows = []
    for i in range(n):
        if diag == UNIT and i % 3 == 1:
            rows.append(([], []))
            continue
        others = np.setdiff1d(np.arange(n), [i])
        off = rng.choice(others, int(rng.integers(0, min(longest, others.size) + 1)), replace=False) if others.size else others
        vals = values(rng, off.size, letter, 0.5 / max(off.size, 1))
        with_diagonal = diag == STORED or i % 3 == 0
        if with_diagonal:
            off = np.append(off, i)
            vals = np.append(vals, pivot(rng, letter))
        order = rng.permutation(off.size)
        off, vals = off[order], vals[order].astype(dtype)
        if poison:
            unused = (off > i) if side == LOWER else (off < i)
            if diag == UNIT:
                unused |= off == i
            vals[unused] = nan
        rows.append((off, vals))
    return from_rows(rows, letter, base), values(rng, n, letter)


def from_levels(rng, widths, letter, base, side, diag=STORED):
    """A matrix whose level l has exactly widths[l] rows: the rows of a level are consecutive (ascending for LOWER, the mirror image
    for UPPER), and every row of level l > 0 stores an entry in a row of level l - 1 and up to two more in earlier levels.  Returns
    ((ptr, cols, vals), b, levels as the Plan must find them)."""
    n = int(sum(widths))
    starts = np.concatenate(([0], np.cumsum(widths)))
    level_of = np.repeat(np.arange(len(widths)), widths)
    flip = (lambda r: r) if side == LOWER else (lambda r: n - 1 - r)
    rows = [None] * n
    for r in range(n):
        l = level_of[r]
        deps = []
        if l > 0:
            deps.append(int(rng.integers(starts[l - 1], starts[l])))
            deps += [int(d) for d in rng.integers(0, starts[l], 2) if d not in deps]
        cols = [flip(d) for d in deps] + [flip(r)]
        vals = np.append(values(rng, len(deps), letter, 0.5 / max(len(deps), 1)), pivot(rng, letter))
        if diag == UNIT:
            cols, vals = cols[:-1], vals[:-1]
        order = rng.permutation(len(cols))
        rows[flip(r)] = (np.asarray(cols, np.int64)[order], vals[order])
    level = np.empty(n, np.int64)
    level[[flip(r) for r in range(n)]] = level_of
    return from_rows(rows, letter, base), values(rng, n, letter), level


def stencil(g, dims, letter, base=0, rng=None):
    """The 5-point (dims = 2) or 7-point (dims = 3) matrix on a g^dims grid, columns ascending: diagonal 2 * dims + 1, neighbours -1
    (or, with rng, random of magnitude about 1 / (2 * dims) and a diagonal in [1, 2])."""
    dtype = X.DTYPE_OF[letter]
    n = g ** dims
    rows = []
    for i in range(n):
        coords = [(i // g ** d) % g for d in range(dims)]
        cols = [i]
        for d in range(dims):
            if coords[d] > 0:
                cols.append(i - g ** d)
            if coords[d] < g - 1:
                cols.append(i + g ** d)
        cols = np.sort(np.asarray(cols, np.int64))
        if rng is None:
            vals = np.where(cols == i, 2.0 * dims + 1, -1.0).astype(dtype)
        else:
            vals = values(rng, cols.size, letter, 0.5 / (2 * dims))
            vals[cols == i] = pivot(rng, letter)
        rows.append((cols, vals))
    return from_rows(rows, letter, base)


def stencil_levels(g, dims, side):
    i = np.arange(g ** dims)
    coords = [(i // g ** d) % g for d in range(dims)]
    return sum(coords) if side == LOWER else sum(g - 1 - c for c in coords)


def bidiagonal(n, letter, base, side, rng):
    """Row i stores its diagonal and, for LOWER, (i, i - 1) -- for UPPER (i, i + 1): n levels of one row."""
    rows = []
    for i in range(n):
        j = i - 1 if side == LOWER else i + 1
        cols, vals = [i], [pivot(rng, letter)]
        if 0 <= j < n:
            cols.append(j)
            vals.append(values(rng, 1, letter, 0.5)[0])
        rows.append((cols, vals))
    return from_rows(rows, letter, base)


def division_operands(rng, count=64):
    """fp32 pairs (n, d) whose correctly rounded quotient differs from n * (1 / d) with the reciprocal rounded first."""
    ns, ds = [], []
    while len(ns) < count:
        n, d = np.float32(1 + rng.random()), np.float32(1 + rng.random())
        if n / d != n * (np.float32(1) / d):
            ns.append(n), ds.append(d)
    return np.array(ns, np.float32), np.array(ds, np.float32)
