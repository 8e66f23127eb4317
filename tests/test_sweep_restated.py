"""CPU: the three restatements of include/spgpu/ext/sweep_device.h in spgpu_amd.formats -- csr_sweep_plan, csr_sweep, csr_residual --
against the row-by-row loops of tests/sweep_cases.py, which share nothing with them, BYTE FOR BYTE in all four value types, with and
without an order, in both bases; the properties the contract states (SYMMETRIC is FORWARD then BACKWARD; omega = 1 is another
expression tree than no omega); the A-norm of the error under Gauss-Seidel and SOR sweeps; and the Plan's refusals."""
import numpy as np
import pytest

import sweep_cases as K
from aggregate_cases import from_rows
from colour_cases import grid_3d
from spgpu_amd import formats

TYPES = [np.float32, np.float64, np.complex64, np.complex128]
NAMES = ["diagonal", "row1", "chain5", "grid5_unsorted", "arrow20", "hubs", "twice", "mixed"]


def _omega(dtype):
    return 1.2 - 0.1j if np.dtype(dtype).kind == "c" else 1.2


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("base", [0, 1])
def test_the_plan_restated(name, base):
    rows, (ptr, col, vals), colours, colour_of, order, colour_ptr = K.build(name, np.float64, base)
    diag_pos, cp, entries = formats.csr_sweep_plan(ptr, col, base, colours, colour_ptr, colour_of, order)
    at = 0
    for i, row in enumerate(rows):
        assert diag_pos[i] == at + [c for c, _ in row].index(i)
        at += len(row)
    assert entries == at and cp.tobytes() == colour_ptr.tobytes() and diag_pos.dtype == cp.dtype == np.int32
    # the permuted matrix without an order: the same positions of the diagonals, row by row
    b_rows = K.permuted(rows, order)
    b_ptr, b_col, _ = from_rows(b_rows, base)
    b_diag, _, b_entries = formats.csr_sweep_plan(b_ptr, b_col, base, colours, colour_ptr)
    starts = np.cumsum([0] + [len(r) for r in b_rows])
    assert b_entries == entries and all(b_col[b_diag[k]] - base == k and starts[k] <= b_diag[k] < starts[k + 1] for k in range(len(rows)))


# the 612-row case is restated in one type: the loops are slow and its rows are those of chain5
@pytest.mark.parametrize("name,dtype", [(name, dtype) for name in NAMES for dtype in TYPES if name != "mixed" or dtype is np.float64])
def test_the_sweep_and_the_residual_restated(name, dtype):
    base = 1 if np.dtype(dtype).itemsize == 8 else 0
    rows, (ptr, col, vals), colours, colour_of, order, colour_ptr = K.build(name, dtype, base)
    b, x = K.vectors(len(rows), dtype)
    diag_pos, cp, _ = formats.csr_sweep_plan(ptr, col, base, colours, colour_ptr, colour_of, order)
    b_rows = K.permuted(rows, order)
    b_mat = from_rows(b_rows, base, dtype)
    b_diag, _, _ = formats.csr_sweep_plan(b_mat[0], b_mat[1], base, colours, colour_ptr)
    for direction in (K.FORWARD, K.BACKWARD, K.SYMMETRIC):
        for omega in (None, _omega(dtype)):
            want = K.sweep_literal(rows, list(colour_of), b, x, dtype, direction, omega)
            got = formats.csr_sweep(ptr, col, vals, b, x, base, colours, cp, diag_pos, order, direction, omega)
            assert got.tobytes() == want.tobytes() and got.dtype == np.dtype(dtype), (name, direction, omega)
            # on B without an order: the sweep of B's own rows, whose entries ascend by column -- another storage order, so
            # another order of the differences, and close to the sweep on A, not equal to it in bytes
            want_b = K.sweep_literal(b_rows, sorted(colour_of), b[order], x[order], dtype, direction, omega)
            got_b = formats.csr_sweep(*b_mat, b[order], x[order], base, colours, cp, b_diag, None, direction, omega)
            assert got_b.tobytes() == want_b.tobytes(), (name, direction, omega)
            assert np.allclose(got_b, want[order], rtol=1e-3, atol=1e-4)
    assert formats.csr_residual(ptr, col, vals, b, x, base).tobytes() == K.residual_literal(rows, b, x, dtype).tobytes()


@pytest.mark.parametrize("dtype", TYPES)
def test_the_residual_of_an_empty_row_moves_b(dtype):
    rows, _ = K.empty_row_case()
    ptr, col, vals = from_rows(rows, 1, dtype)
    b, x = K.vectors(4, dtype)
    b[1] = -0.0
    got = formats.csr_residual(ptr, col, vals, b, x, 1)
    assert got.tobytes() == K.residual_literal(rows, b, x, dtype).tobytes() and got[1:2].tobytes() == b[1:2].tobytes()


@pytest.mark.parametrize("dtype", TYPES)
def test_symmetric_is_forward_then_backward_and_omega_one_is_another_tree(dtype):
    base = 0
    rows, (ptr, col, vals), colours, colour_of, order, colour_ptr = K.build("grid5_unsorted", dtype, base, seed=3)
    b, x = K.vectors(len(rows), dtype, seed=3)
    diag_pos, cp, _ = formats.csr_sweep_plan(ptr, col, base, colours, colour_ptr, colour_of, order)
    sweep = lambda start, direction, omega=None: formats.csr_sweep(ptr, col, vals, b, start, base, colours, cp, diag_pos, order, direction, omega)
    for omega in (None, _omega(dtype)):
        both = sweep(x, K.SYMMETRIC, omega)
        assert both.tobytes() == sweep(sweep(x, K.FORWARD, omega), K.BACKWARD, omega).tobytes()
        assert both.tobytes() != sweep(sweep(x, K.BACKWARD, omega), K.FORWARD, omega).tobytes()
    # omega = 1 computes x + 1 * (g - x), which rounds twice where omega == NULL stores g: close, and not promised equal in bytes
    plain, one = sweep(x, K.FORWARD), sweep(x, K.FORWARD, 1.0)
    eps = np.finfo(np.dtype(dtype).type(0).real.dtype).eps
    assert np.max(np.abs(plain - one)) <= 8 * eps * np.max(np.abs(plain))
    if np.dtype(dtype) == np.float64:
        assert plain.tobytes() != one.tobytes()           # on this input the two trees do differ: the documented departure


def test_the_a_norm_of_the_error_does_not_increase():
    """The fp64 7-point matrix of an 8^3 grid (symmetric positive definite) with the library's own colouring and a random guess: ten
    forward Gauss-Seidel sweeps, and ten SOR sweeps with omega = 1.2 (inside (0, 2)), never increase the A-norm of the error."""
    ptr, col, vals = grid_3d(8)
    n = ptr.size - 1
    colours, _, colour_of = formats.csr_colour(ptr, col, 0)
    order, _, colour_ptr = formats.csr_colour_order(colour_of, colours)
    diag_pos, cp, _ = formats.csr_sweep_plan(ptr, col, 0, colours, colour_ptr, colour_of, order)
    dense = np.zeros((n, n))
    for i in range(n):
        dense[i, col[ptr[i]:ptr[i + 1]]] = vals[ptr[i]:ptr[i + 1]]
    rng = np.random.default_rng(8)
    exact, guess = rng.standard_normal(n), rng.standard_normal(n)
    b = dense @ exact
    for omega in (None, 1.2):
        x = guess
        norms = [float((x - exact) @ dense @ (x - exact))]
        for _ in range(10):
            x = formats.csr_sweep(ptr, col, vals, b, x, 0, colours, cp, diag_pos, order, K.FORWARD, omega)
            norms.append(float((x - exact) @ dense @ (x - exact)))
        assert all(after <= before for before, after in zip(norms, norms[1:])), (omega, norms)
        assert norms[-1] < 0.5 * norms[0]
        assert np.linalg.norm(formats.csr_residual(ptr, col, vals, b, x, 0) - (b - dense @ x)) <= 1e-12 * np.linalg.norm(b)


def test_the_plan_refuses_each_bad_input():
    for what, rows, colour in K.refusals():
        for base in (0, 1):
            ptr, col, _ = from_rows(rows, base)
            colour_of = np.array(colour, np.int32)
            order, _, colour_ptr = formats.csr_colour_order(colour_of, 2)
            with pytest.raises(ValueError):
                formats.csr_sweep_plan(ptr, col, base, 2, colour_ptr, colour_of, order)
    rows, colour = K.chain(6)
    ptr, col, _ = from_rows(rows, 0)
    good = np.array(colour, np.int32)
    order, _, colour_ptr = formats.csr_colour_order(good, 2)
    formats.csr_sweep_plan(ptr, col, 0, 2, colour_ptr, good, order)                       # the sound matrix passes
    for bad_colour in (-1, 2):
        colour_of = good.copy()
        colour_of[3] = bad_colour
        with pytest.raises(ValueError):
            formats.csr_sweep_plan(ptr, col, 0, 2, colour_ptr, colour_of, order)
    with pytest.raises(ValueError):                                                       # without an order the chain is not in colour order
        formats.csr_sweep_plan(ptr, col, 0, 2, colour_ptr)
    for bad_ptr in ([1, 3, 6], [0, 4, 3], [0, 3, 5]):
        with pytest.raises(ValueError):
            formats.csr_sweep_plan(ptr, col, 0, 2, np.array(bad_ptr, np.int32), good, order)


def test_an_unsymmetric_pattern_that_the_colouring_accepts_and_the_plan_refuses():
    ptr, col, _ = from_rows(K.unsymmetric_pair(), 0)
    colours, _, colour_of = formats.csr_colour(ptr, col, 0)
    assert colours == 1 and colour_of.tolist() == [0, 0]
    order, _, colour_ptr = formats.csr_colour_order(colour_of, colours)
    with pytest.raises(ValueError):
        formats.csr_sweep_plan(ptr, col, 0, colours, colour_ptr, colour_of, order)
    # the remedy of the header: the colouring of the pattern of A + A^T is proper in both directions
    sym_ptr, sym_col, _ = from_rows([[(0, 1.0), (1, 1.0)], [(1, 1.0), (0, 1.0)]], 0)
    colours, _, colour_of = formats.csr_colour(sym_ptr, sym_col, 0)
    order, _, colour_ptr = formats.csr_colour_order(colour_of, colours)
    assert colours == 2 and formats.csr_sweep_plan(ptr, col, 0, colours, colour_ptr, colour_of, order)[2] == 3
