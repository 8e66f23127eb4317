"""Matrices and independent checks shared by the multicolour-ordering tests (include/spgpu/ext/colour_device.h): CSR arrays of 5-,
7- and 27-point grids, the chain, cliques that fill one and two 64-colour windows, random unsymmetric patterns, a strip of 1025 rows
with one row of 200 entries, a matrix with a column out of range; and the sequential greedy colouring, a literal per-node
implementation of the rounds, and the level count of a lower triangle.  Nothing here imports the device code; the independent
implementations share nothing with formats.csr_colour but the priority."""
import numpy as np

from aggregate_cases import chain, from_rows, grid_5pt, neighbours, random_unsymmetric, strip_1025, symmetric  # noqa: F401

# name -> (rows, colours, rounds, levels of the lower triangle in the natural order, in the coloured order): the figures of a CPU
# prototype of the contract, the lowbias32 priorities and the smallest free colour
TABLE = {
    "grid5_4": (16, 2, 5, 7, 2),
    "grid5_16": (256, 4, 8, 31, 4),
    "chain_300": (300, 3, 5, 300, 3),
    "grid7_8": (512, 6, 11, 22, 6),
    "grid7_24": (13824, 6, 17, 70, 6),
    "grid27_6": (216, 15, 28, 36, 15),
    "clique_70": (70, 70, 70, 70, 70),
    "clique_130": (130, 130, 130, 130, 130),
}


def grid_3d(n, base=0, dtype=np.float64, corners=False):
    """The 7-point (or, with corners, 27-point) matrix of an n^3 grid: -1 to every neighbour, the stencil size on the diagonal;
    ascending columns."""
    rows = []
    reach = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
             if corners or abs(dx) + abs(dy) + abs(dz) <= 1]
    for i in range(n ** 3):
        x, y, z = i % n, (i // n) % n, i // (n * n)
        row = []
        for dx, dy, dz in reach:
            if 0 <= x + dx < n and 0 <= y + dy < n and 0 <= z + dz < n:
                j = i + dx + n * dy + n * n * dz
                row.append((j, float(len(reach)) if j == i else -1.0))
        rows.append(row)
    return from_rows(rows, base, dtype)


def clique(n, base=0, dtype=np.float64):
    """Every node next to every other: n colours, one per round."""
    return from_rows([[(j, float(n) if j == i else -1.0) for j in range(n)] for i in range(n)], base, dtype)


def named(name, base=0, dtype=np.float64):
    kind, size = name.split("_")
    size = int(size)
    if kind == "grid5":
        return grid_5pt(size, base, dtype)
    if kind == "chain":
        return chain(size, base, dtype)
    if kind == "grid7":
        return grid_3d(size, base, dtype)
    if kind == "grid27":
        return grid_3d(size, base, dtype, corners=True)
    assert kind == "clique"
    return clique(size, base, dtype)


def strip_descending(base=0, dtype=np.float64):
    """strip_1025 with the 201 entries of row 7 stored in descending columns."""
    ptr, col, vals = strip_1025(base, dtype)
    a, b = int(ptr[7]) - base, int(ptr[8]) - base
    col, vals = col.copy(), vals.copy()
    col[a:b], vals[a:b] = col[a:b][::-1].copy(), vals[a:b][::-1].copy()
    assert np.all(np.diff(col[a:b].astype(np.int64)) < 0)
    return ptr, col, vals


def out_of_range(bad, base=0):
    """The chain of 10 with one column replaced by `bad` (given in `base`)."""
    ptr, col, vals = chain(10, base)
    col = col.copy()
    col[4] = bad
    return ptr, col, vals


def distinct_values(mat, dtype):
    """The matrix with one value per stored entry that names its position (exact in every type): 1, 2, 3, ... and, for the complex
    types, the negative of it as the imaginary part."""
    ptr, col, _ = mat
    v = np.arange(1, col.size + 1).astype(np.float64)
    vals = (v - 1j * v).astype(dtype) if np.dtype(dtype).kind == "c" else v.astype(dtype)
    return ptr, col, vals


def greedy_colouring(S, priority):
    """One sequential pass in descending (priority, i): every node takes the smallest colour none of its already coloured neighbours
    holds.  For a structurally symmetric S."""
    n = len(S)
    colour = [-1] * n
    for i in sorted(range(n), key=lambda i: (int(priority[i]), i), reverse=True):
        held = {colour[j] for j in S[i] if colour[j] >= 0}
        c = 0
        while c in held:
            c += 1
        colour[i] = c
    return np.array(colour, np.int32)


def rounds_literal(S, priority):
    """The rounds of the contract, node by node and set by set -> (colours, rounds, colour_of)."""
    n = len(S)
    key = [(int(priority[i]), i) for i in range(n)]
    c0, rounds = [-1] * n, 0
    while any(c < 0 for c in c0):
        c1 = list(c0)
        for i in range(n):
            if c0[i] >= 0:
                continue
            if all(c0[j] >= 0 or key[j] < key[i] for j in S[i]):
                held = {c0[j] for j in S[i]}
                c1[i] = min(c for c in range(len(S[i]) + 1) if c not in held)
        c0, rounds = c1, rounds + 1
        assert rounds <= n
    return (max(c0) + 1 if n else 0), rounds, np.array(c0, np.int32)


def lower_levels(row_ptr, col, base):
    """The number of levels of the strictly lower triangle: level(i) = 1 + the largest level over the stored j < i, 0 without one."""
    ptr = np.asarray(row_ptr, np.int64) - base
    col = np.asarray(col, np.int64) - base
    level = np.zeros(ptr.size - 1, np.int64)
    for i in range(ptr.size - 1):
        js = col[ptr[i]:ptr[i + 1]]
        js = js[js < i]
        if js.size:
            level[i] = 1 + level[js].max()
    return int(level.max()) + 1 if level.size else 0


def dense(mat, base):
    """The dense matrix of CSR arrays without repeated columns."""
    ptr, col, vals = mat
    n = ptr.size - 1
    out = np.zeros((n, n), vals.dtype)
    for i in range(n):
        for p in range(int(ptr[i]) - base, int(ptr[i + 1]) - base):
            out[i, int(col[p]) - base] = vals[p]
    return out
