"""CPU: numpy's restatement of the aggregation (spgpu_amd.formats.csr_strength, csr_aggregate, csr_tentative), which the GPU tests
compare bytes with, against checks that share nothing with it.  On structurally symmetric patterns the roots of the rounds are the
greedy distance-2 maximal independent set in descending tuple order (tests/aggregate_cases.py greedy_mis2, a sequential pass on the
squared graph): no two roots within distance 2, every node assigned to a root within distance 2, the sizes a bincount, the
singletons exactly the rows with empty S.  On unsymmetric patterns the rounds end and every node is assigned.  Hashed priorities
finish a chain in far fewer rounds than identity priorities.  The threshold of the strength of connection is checked at equality, one
ulp below it, and with NaN, zero, missing and -0.0 operands, against expectations written by hand."""
import numpy as np
import pytest

import aggregate_cases as A
from spgpu_amd import formats

SYMMETRIC = {
    "grid 4x4": lambda: A.grid_5pt(4),
    "grid 12x12": lambda: A.grid_5pt(12, base=1),
    "grid 16x16": lambda: A.grid_5pt(16),
    "chain 300": lambda: A.chain(300, base=1),
}


def _base_of(ptr):
    return int(ptr[0])


@pytest.mark.parametrize("name", sorted(SYMMETRIC))
def test_on_a_symmetric_pattern_the_roots_are_the_greedy_mis2(name):
    ptr, col, vals = SYMMETRIC[name]()
    base = _base_of(ptr)
    n = ptr.size - 1
    strong, _ = formats.csr_strength(ptr, col, vals, base, 0.25)
    S = A.neighbours(ptr, col, strong, base)
    assert A.symmetric(S) and all(S)
    count, rounds, aggregate_of, sizes = formats.csr_aggregate(ptr, col, strong, base)
    # roots are numbered by ascending row, so the greedy set is the set of roots when there are as many aggregates as greedy nodes
    # and the k-th greedy node by ascending row carries the number k
    want = A.greedy_mis2(S, formats.aggregate_priority(n))
    assert count == int(want.sum()) and rounds >= 1
    assert np.array_equal(aggregate_of[want], np.arange(count)), name
    root_of = np.flatnonzero(want)
    for i in root_of:
        assert not (A.within_two(S, int(i)) & set(root_of.tolist())), (name, i)  # no two roots within distance 2
    for i in range(n):                                                        # every node joins a root within distance 2
        r = int(root_of[aggregate_of[i]])
        assert r == i or r in A.within_two(S, i), (name, i, r)
    assert aggregate_of.dtype == np.int32 and sizes.dtype == np.int32
    assert np.array_equal(sizes, np.bincount(aggregate_of, minlength=count)) and sizes.sum() == n and sizes.min() >= 1
    # with strong == None every stored off-diagonal counts: on these matrices the same graph
    assert all(np.array_equal(a, b) for a, b in zip(formats.csr_aggregate(ptr, col, None, base)[2:], (aggregate_of, sizes)))


def test_singletons_are_exactly_the_rows_with_empty_s():
    """A symmetric pattern with isolated nodes: a 6 x 6 grid whose rows 0, 17 and 35 keep only their diagonal (and lose their place in
    their neighbours' rows)."""
    ptr, col, vals = A.grid_5pt(6)
    alone = {0, 17, 35}
    rows = []
    for i in range(36):
        entries = [(int(col[p]), float(vals[p])) for p in range(ptr[i], ptr[i + 1])]
        rows.append([(c, v) for c, v in entries if c == i or (i not in alone and c not in alone)])
    ptr, col, vals = A.from_rows(rows)
    S = A.neighbours(ptr, col, None, 0)
    assert A.symmetric(S) and {i for i in range(36) if not S[i]} == alone
    count, _, aggregate_of, sizes = formats.csr_aggregate(ptr, col, None, 0)
    singles = {int(np.flatnonzero(aggregate_of == a)[0]) for a in np.flatnonzero(sizes == 1)}
    assert singles == alone and count == int(A.greedy_mis2(S, formats.aggregate_priority(36)).sum())


def test_on_random_unsymmetric_patterns_the_rounds_end_and_every_node_is_assigned():
    unsymmetric = 0
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        ptr, col, vals = A.random_unsymmetric(rng, 200, base=seed % 2)
        base = seed % 2
        S = A.neighbours(ptr, col, None, base)
        unsymmetric += not A.symmetric(S)
        count, rounds, aggregate_of, sizes = formats.csr_aggregate(ptr, col, None, base)
        assert 1 <= rounds <= 200 and 1 <= count <= 200
        assert aggregate_of.min() >= 0 and aggregate_of.max() == count - 1
        assert np.array_equal(sizes, np.bincount(aggregate_of, minlength=count)) and sizes.min() >= 1
        empty = [i for i in range(200) if not S[i]]                           # roots each: no two of them share an aggregate
        assert empty and len(set(aggregate_of[empty].tolist())) == len(empty)
    assert unsymmetric == 20


def test_hashed_priorities_finish_a_chain_in_far_fewer_rounds_than_identity_priorities():
    n = 300
    ptr, col, _ = A.chain(n)
    _, hashed, _, _ = formats.csr_aggregate(ptr, col, None, 0)
    _, identity, _, _ = formats.csr_aggregate(ptr, col, None, 0, priority=np.arange(n, dtype=np.uint64))
    assert hashed < n / 10 < identity, (hashed, identity)
    ptr, col, _ = A.grid_5pt(16)
    assert formats.csr_aggregate(ptr, col, None, 0)[1] < 256 / 10


def test_the_priority_is_lowbias32_shifted_by_one():
    def lowbias32(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    got = formats.aggregate_priority(1000)
    assert got.dtype == np.uint64 and [int(v) for v in got] == [lowbias32(i) >> 1 for i in range(1000)]
    assert lowbias32(0) == 0 and int(got.max()) < 2 ** 31 and len(set(got.tolist())) == 1000


def test_a_neighbour_outside_the_matrix_is_refused():
    ptr, col, vals = A.chain(10)
    for bad in (10, -1, 2 ** 31 - 1):
        wrong = col.copy()
        wrong[4] = bad
        with pytest.raises(ValueError):
            formats.csr_aggregate(ptr, wrong, None, 0)
        mask = np.ones(col.size, np.uint8)
        with pytest.raises(ValueError):
            formats.csr_aggregate(ptr, wrong, mask, 0)
        mask[4] = 0                                                          # masked out: no neighbour, nothing to refuse
        assert formats.csr_aggregate(ptr, wrong, mask, 0)[0] >= 1


# ---- the strength of connection ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("base", [0, 1])
def test_the_threshold_edge_cases(dtype, base):
    """Equality at the threshold with powers of two is strong, one ulp below is not; a NaN value, a NaN diagonal at either end, a zero
    diagonal, a missing diagonal, theta = 0, -0.0 and a column outside the matrix (tests/aggregate_cases.py threshold_matrix)."""
    ptr, col, vals, at_half, at_zero, diag = A.threshold_matrix(dtype, base)
    strong, diag_abs = formats.csr_strength(ptr, col, vals, base, 0.5)
    assert strong.dtype == np.uint8 and diag_abs.dtype == np.dtype(dtype)
    assert strong.tolist() == at_half.tolist()
    assert diag_abs.tobytes() == diag.tobytes()                               # |-0.0| = +0 and the FIRST diagonal, by their bits
    strong, diag_abs = formats.csr_strength(ptr, col, vals, base, 0.0)
    assert strong.tolist() == at_zero.tolist() and diag_abs.tobytes() == diag.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_threshold_is_computed_in_the_value_type(dtype):
    """theta = 0.3: t = T(0.09) differs between the types, and rhs = (t * d_i) * d_j is rounded at every step; an entry exactly at the
    type's own rhs is strong, the next value below is not."""
    T = np.dtype(dtype).type
    t = T(0.3 * 0.3)
    d0, d1 = T(3), T(7)
    rhs = (t * d0) * d1
    a = np.sqrt(rhs)
    while a * a < rhs:
        a = np.nextafter(a, T(np.inf))
    while np.nextafter(a, T(0)) * np.nextafter(a, T(0)) >= rhs:
        a = np.nextafter(a, T(0))
    ptr, col, vals = A.from_rows([[(0, d0), (1, a)], [(0, np.nextafter(a, T(0))), (1, -d1)]], 0, dtype)
    strong, diag_abs = formats.csr_strength(ptr, col, vals, 0, 0.3)
    assert strong.tolist() == [0, 1, 0, 0] and diag_abs.tolist() == [3, 7]


def test_complex_values_have_no_strength():
    ptr, col, vals = A.chain(4)
    with pytest.raises(ValueError):
        formats.csr_strength(ptr, col, vals.astype(np.complex128), 0, 0.25)


def test_anisotropy_keeps_the_aggregates_on_their_grid_lines():
    """Coupling 1 in x and 2^-10 in y at theta = 0.25: strong edges run along x only, so no aggregate spans two grid lines."""
    g = 16
    ptr, col, vals = A.grid_5pt(g, cx=1.0, cy=2.0 ** -10)
    strong, _ = formats.csr_strength(ptr, col, vals, 0, 0.25)
    S = A.neighbours(ptr, col, strong, 0)
    assert all(j // g == i // g for i in range(g * g) for j in S[i]) and all(S)
    count, _, aggregate_of, _ = formats.csr_aggregate(ptr, col, strong, 0)
    lines = np.arange(g * g) // g
    for a in range(count):
        assert np.unique(lines[aggregate_of == a]).size == 1


# ---- the tentative prolongator -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_the_tentative_prolongator_has_one_entry_per_row(dtype):
    aggregate_of = np.array([2, 0, 1, 1, 0], np.int32)
    for base in (0, 1):
        t_ptr, t_cols, t_vals = formats.csr_tentative(aggregate_of, None, base, dtype)
        assert t_ptr.tolist() == [base + i for i in range(6)] and t_cols.tolist() == (aggregate_of + base).tolist()
        assert t_vals.dtype == np.dtype(dtype) and t_vals.tolist() == [1] * 5
        assert t_ptr.dtype == t_cols.dtype == np.int32
    candidate = np.array([1.5, -0.0, np.nan, 3, -2], dtype)
    assert formats.csr_tentative(aggregate_of, candidate, 0, dtype)[2].tobytes() == candidate.tobytes()
