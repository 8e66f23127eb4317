"""CPU: numpy's restatement of the multicolour ordering (spgpu_amd.formats.csr_colour, csr_colour_order, csr_permute), which the GPU
tests compare bytes with, against implementations that share nothing with it but the priority (tests/colour_cases.py): the
sequential greedy colouring in descending tuple order on structurally symmetric patterns, a literal node-by-node implementation of
the rounds on unsymmetric ones, the figures of the issue's table, a dense P A P^T, and the level count of the permuted pattern."""
import numpy as np
import pytest

import colour_cases as K
from spgpu_amd import formats

SYMMETRIC = sorted(K.TABLE)
SMALL = [name for name in SYMMETRIC if K.TABLE[name][0] <= 600]


@pytest.fixture(scope="module")
def coloured():
    """name -> (matrix, (colours, rounds, colour_of)), base 0, computed once."""
    out = {}
    for name in SYMMETRIC:
        mat = K.named(name)
        out[name] = (mat, formats.csr_colour(mat[0], mat[1], 0))
    return out


@pytest.mark.parametrize("name", SYMMETRIC)
def test_the_counts_are_the_prototypes(coloured, name):
    mat, (colours, rounds, colour_of) = coloured[name]
    rows, want_colours, want_rounds, natural, _ = K.TABLE[name]
    assert mat[0].size - 1 == rows and colour_of.dtype == np.int32 and colour_of.size == rows
    assert (colours, rounds) == (want_colours, want_rounds)
    assert K.lower_levels(mat[0], mat[1], 0) == natural


@pytest.mark.parametrize("name", SYMMETRIC)
def test_a_symmetric_pattern_gets_the_sequential_greedy_colouring(coloured, name):
    """Equal arrays; a proper colouring; at most 1 + the largest degree colours."""
    mat, (colours, _, colour_of) = coloured[name]
    S = K.neighbours(mat[0], mat[1], None, 0)
    assert K.symmetric(S)
    assert colour_of.tolist() == K.greedy_colouring(S, formats.aggregate_priority(len(S))).tolist()
    assert all(colour_of[i] != colour_of[j] for i in range(len(S)) for j in S[i])
    assert colour_of.min() == 0 and colours == colour_of.max() + 1 <= 1 + max(len(s) for s in S)


@pytest.mark.parametrize("name", SMALL)
def test_the_rounds_agree_with_the_literal_implementation_on_symmetric_patterns(coloured, name):
    mat, (colours, rounds, colour_of) = coloured[name]
    S = K.neighbours(mat[0], mat[1], None, 0)
    want = K.rounds_literal(S, formats.aggregate_priority(len(S)))
    assert (colours, rounds) == want[:2] and colour_of.tolist() == want[2].tolist()


def test_the_base_changes_nothing():
    for g in (4, 16):
        zero, one = K.grid_5pt(g, 0), K.grid_5pt(g, 1)
        a, b = formats.csr_colour(zero[0], zero[1], 0), formats.csr_colour(one[0], one[1], 1)
        assert a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() and a[2].min() == 0


@pytest.mark.parametrize("seed", range(20))
def test_random_unsymmetric_patterns_terminate_and_agree_with_the_literal_rounds(seed):
    rng = np.random.default_rng(500 + seed)
    base = seed % 2
    n = 100 + 9 * seed                                                         # row 3 of the pattern stores column 90
    ptr, col, _ = K.random_unsymmetric(rng, n, base)
    S = K.neighbours(ptr, col, None, base)
    assert not K.symmetric(S)
    colours, rounds, colour_of = formats.csr_colour(ptr, col, base)
    want = K.rounds_literal(S, formats.aggregate_priority(n))
    assert (colours, rounds) == want[:2] and colour_of.tolist() == want[2].tolist()
    assert 1 <= rounds <= n and colour_of.min() == 0 and colours <= 1 + max(len(s) for s in S)
    # a given priority replaces the hash: with ascending priorities node n - 1 goes first
    by_row = formats.csr_colour(ptr, col, base, priority=np.arange(n, dtype=np.uint64))
    want = K.rounds_literal(S, np.arange(n))
    assert by_row[:2] == want[:2] and by_row[2].tolist() == want[2].tolist()


def test_a_column_outside_the_matrix_is_refused():
    for base in (0, 1):
        for bad in (10 + base, base - 1, 2 ** 31 - 1):
            ptr, col, _ = K.out_of_range(bad, base)
            with pytest.raises(ValueError):
                formats.csr_colour(ptr, col, base)


def test_no_rows_no_colours():
    assert formats.csr_colour(np.zeros(1, np.int32), np.zeros(0, np.int32), 0)[:2] == (0, 0)
    empty = formats.csr_colour(np.ones(4, np.int32), np.zeros(0, np.int32), 1)          # three empty rows: one colour, one round
    assert empty[:2] == (1, 1) and empty[2].tolist() == [0, 0, 0]


@pytest.mark.parametrize("name", SYMMETRIC)
def test_the_order_lists_the_rows_by_colour_and_row(coloured, name):
    _, (colours, _, colour_of) = coloured[name]
    order, inverse, colour_ptr = formats.csr_colour_order(colour_of, colours)
    n = colour_of.size
    assert order.dtype == inverse.dtype == colour_ptr.dtype == np.int32
    assert sorted(order.tolist()) == list(range(n)) and inverse[order].tolist() == list(range(n))
    keys = list(zip(colour_of[order].tolist(), order.tolist()))
    assert keys == sorted(keys)
    assert colour_ptr.size == colours + 1 and colour_ptr[0] == 0 and colour_ptr[-1] == n
    for c in range(colours):
        assert (colour_of[order[colour_ptr[c]:colour_ptr[c + 1]]] == c).all() and colour_ptr[c] < colour_ptr[c + 1]


@pytest.mark.parametrize("name", SYMMETRIC)
def test_the_permuted_pattern_has_as_many_levels_as_colours(coloured, name):
    """Rows of one colour do not depend on each other, and greedy colour c has a neighbour of every colour below c."""
    mat, (colours, _, colour_of) = coloured[name]
    order, inverse, _ = formats.csr_colour_order(colour_of, colours)
    b_ptr, b_cols, _ = formats.csr_permute(order, inverse, *mat, 0)
    assert K.lower_levels(b_ptr, b_cols, 0) == colours == K.TABLE[name][4]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("base", [0, 1])
def test_the_permutation_is_p_a_pt(dtype, base):
    for mat in (K.grid_5pt(4, base), K.chain(30, base), K.grid_3d(3, base, corners=True)):
        ptr, col, vals = K.distinct_values(mat, dtype)
        n = ptr.size - 1
        colours, _, colour_of = formats.csr_colour(ptr, col, base)
        order, inverse, _ = formats.csr_colour_order(colour_of, colours)
        b_ptr, b_cols, b_vals = formats.csr_permute(order, inverse, ptr, col, vals, base)
        assert b_ptr.dtype == b_cols.dtype == np.int32 and b_vals.dtype == np.dtype(dtype)
        P = np.zeros((n, n))
        P[np.arange(n), order] = 1                                             # row k of P A is row order[k] of A
        want = (P @ K.dense((ptr, col, vals), base) @ P.T).astype(dtype)       # one term per sum: exact
        assert np.array_equal(K.dense((b_ptr, b_cols, b_vals), base), want)
        assert b_ptr[0] == base and np.array_equal(np.diff(b_ptr), np.diff(ptr)[order])
        for k in range(n):                                                     # strictly ascending rows
            assert np.all(np.diff(b_cols[b_ptr[k] - base:b_ptr[k + 1] - base].astype(np.int64)) > 0)
        formats.csr_ilu0_plan(b_ptr, b_cols, base)                             # what the ILU(0) Plan demands


def test_repeated_columns_keep_their_storage_order_and_bits_survive():
    base = 1
    rng = np.random.default_rng(3)
    ptr, col, vals = K.random_unsymmetric(rng, 120, base)
    vals = vals.copy()
    vals[0] = -0.0
    raw = vals.view(np.uint64)
    raw[1] = 0x7FF8000000000000 | 0x123456789
    n = ptr.size - 1
    order = rng.permutation(n)
    inverse = np.empty(n, np.int64)
    inverse[order] = np.arange(n)
    b_ptr, b_cols, b_vals = formats.csr_permute(order, inverse, ptr, col, vals, base)
    for k in range(n):
        i = order[k]
        a = slice(ptr[i] - base, ptr[i + 1] - base)
        b = slice(b_ptr[k] - base, b_ptr[k + 1] - base)
        new = inverse[col[a].astype(np.int64) - base]
        at = sorted(range(new.size), key=lambda p: (new[p], p))                # stable by construction
        assert (b_cols[b] - base).tolist() == [int(new[p]) for p in at]
        assert b_vals[b].tobytes() == vals[a][at].tobytes()
    row2 = slice(b_ptr[inverse[2]] - base, b_ptr[inverse[2] + 1] - base)       # row 2 stores column 7 twice: 1.0 before 5.0
    twice = b_vals[row2][(b_cols[row2] - base) == inverse[7]]
    assert twice.tolist() == [1.0, 5.0]
    identity = np.arange(n)
    s_ptr, s_cols, _ = formats.csr_permute(identity, identity, ptr, col, vals, base)    # the identity: A with sorted rows
    assert s_ptr.tobytes() == ptr.tobytes()
    assert all(sorted(col[ptr[i] - base:ptr[i + 1] - base].tolist()) == s_cols[ptr[i] - base:ptr[i + 1] - base].tolist() for i in range(n))
