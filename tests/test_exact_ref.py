"""CPU: the extended-precision reference of the GPU bounds (tests/exact_ref.py) pinned against the committed golden products and
against dense numpy -- complex alpha / beta, a row order, both index bases, holes, SpMM with ld > count -- and its assertion
helper against values just inside and just outside the bound."""
import glob
import os

import numpy as np
import pytest

import exact_ref as X


def _golden(golden_dir):
    for path in sorted(glob.glob(os.path.join(golden_dir, "*.npz"))):
        with np.load(path) as f:
            if "z_expected" in f.files:
                yield os.path.basename(path)[:-4], {k: f[k] for k in f.files}


def test_golden_products(golden_dir):
    names = []
    for name, g in _golden(golden_dir):
        alpha, beta = g["alpha"][()], g["beta"][()]
        n, base = int(g["n_rows"]), int(g["base"])
        z, scale = X.spmv(n, g["coo_rows"], g["coo_cols"], g["coo_vals"], g["x"], g["y"] if beta != 0 else None, alpha, beta, base=base)
        want = g["z_expected"]
        assert np.max(np.abs(z - want.astype(z.dtype)).astype(np.float64) - 1e-13 * g["z_scale"], initial=0.0) <= 1e-300, name
        np.testing.assert_allclose(scale, g["z_scale"], rtol=1e-13, atol=0.0, err_msg=name)
        X.assert_within(want.astype(np.complex128 if np.iscomplexobj(want) else np.float64), z, scale, "D", name)
        names.append(name)
    assert len(names) >= 8
    assert np.iscomplexobj(dict(_golden(golden_dir))["powerlaw_c_b1_h64"]["alpha"])     # a complex alpha and beta among them


def _dense_case(rng, letter, n, m, nnz, base):
    rows = rng.integers(0, n, nnz)
    cols = rng.integers(0, m, nnz)
    real = X.REAL_OF[letter]
    vals = rng.standard_normal(nnz).astype(real)
    if letter in "CZ":
        vals = (vals + 1j * rng.standard_normal(nnz).astype(real)).astype(X.DTYPE_OF[letter])
    dense = np.zeros((n, m), np.complex128)
    np.add.at(dense, (rows, cols), vals.astype(np.complex128))      # duplicates add, as the COO sum does
    return rows + base, cols + base, vals, dense


@pytest.mark.parametrize("letter", ["S", "D", "C", "Z"])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("ordered", [False, True])
def test_against_dense_numpy(letter, base, ordered):
    rng = np.random.default_rng(17 + 4 * base + ordered)
    n, m = 37, 29
    rows, cols, vals, dense = _dense_case(rng, letter, n, m, 200, base)
    x = rng.standard_normal(m) + (1j * rng.standard_normal(m) if letter in "CZ" else 0)
    y = rng.standard_normal(n) + (1j * rng.standard_normal(n) if letter in "CZ" else 0)
    alpha, beta = (0.75 - 1.5j, -0.5 + 0.25j) if letter in "CZ" else (-1.25, 0.5)
    r_idx = rng.permutation(n).astype(np.int32) if ordered else None
    z, scale = X.spmv(n, rows, cols, vals, x, y, alpha, beta, r_idx=r_idx, base=base)
    row_sums = dense @ x
    want = np.empty(n, np.complex128)
    if ordered:
        want[r_idx] = alpha * row_sums
    else:
        want[:] = alpha * row_sums
    want = want + beta * y
    assert np.max(np.abs(z.astype(np.complex128) - want)) <= 1e-12 * np.max(np.abs(want))
    mag = np.abs(dense * x[None, :]).sum(axis=1)       # (duplicates: |a1 x + a2 x| <= |a1 x| + |a2 x|)
    mag_at = np.empty(n)
    if ordered:
        mag_at[r_idx] = mag
    else:
        mag_at[:] = mag
    assert np.all(scale >= abs(alpha) * mag_at + np.abs(beta * y) - 1e-12 * scale)
    # beta = 0 needs no y, and the scale then has no |beta y| term
    z0, s0 = X.spmv(n, rows, cols, vals, x, None, alpha, 0.0, r_idx=r_idx, base=base)
    assert np.max(np.abs(z0.astype(np.complex128) - (want - beta * y))) <= 1e-12 * np.max(np.abs(want))
    assert np.all(s0 <= scale)


def test_holes_below_the_base_are_not_used():
    rows = np.array([1, 1, 2, 2])
    cols = np.array([1, 0, 3, 0])        # 1-based: column 0 is -1, a hole
    vals = np.array([2.0, 1e30, 3.0, -1e30])
    x = np.array([5.0, 7.0, 11.0])
    z, scale = X.spmv(2, rows, cols, vals, x, None, 1.0, 0.0, base=1)
    assert z.astype(np.float64).tolist() == [10.0, 33.0]
    assert scale.tolist() == [10.0, 33.0]


@pytest.mark.parametrize("letter", ["D", "C"])
def test_spmm_interleaved_with_leading_dimensions(letter):
    rng = np.random.default_rng(5)
    n, m, count, ldx, ldy = 23, 19, 3, 5, 4
    rows, cols, vals, dense = _dense_case(rng, letter, n, m, 90, 0)
    Xf = rng.standard_normal(m * ldx) + (1j * rng.standard_normal(m * ldx) if letter == "C" else 0)
    Yf = rng.standard_normal(n * ldy) + (1j * rng.standard_normal(n * ldy) if letter == "C" else 0)
    alpha, beta = (1.5 + 0.5j, 0.25 - 1j) if letter == "C" else (1.5, -0.75)
    r_idx = rng.permutation(n)
    Z, S = X.spmm(n, rows, cols, vals, Xf, Yf, alpha, beta, count, ldx=ldx, ldy=ldy, r_idx=r_idx)
    assert Z.shape == (n, count) and S.shape == (n, count)
    for k in range(count):
        want = np.empty(n, np.complex128)
        want[r_idx] = alpha * (dense @ Xf.reshape(m, ldx)[:, k])
        want += beta * Yf.reshape(n, ldy)[:, k]
        assert np.max(np.abs(Z[:, k].astype(np.complex128) - want)) <= 1e-12 * np.max(np.abs(want))
        z1, s1 = X.spmv(n, rows, cols, vals, Xf.reshape(m, ldx)[:, k], Yf.reshape(n, ldy)[:, k], alpha, beta, r_idx=r_idx)
        assert np.array_equal(Z[:, k], z1) and np.array_equal(S[:, k], s1)


@pytest.mark.parametrize("letter", ["S", "D", "C", "Z"])
def test_assert_within_fails_just_outside_the_bound(letter):
    want = np.array([1.0, -2.0, 3.0], np.longdouble if letter in "SD" else np.clongdouble)
    scale = np.array([1.0, 4.0, 3.0])
    tol = X.TOL[letter]
    dtype = X.DTYPE_OF[letter]
    inside = (want.astype(np.complex128) + np.array([0.5, 0.5, -0.5]) * tol * scale).astype(dtype) if letter in "CZ" else \
        (want.astype(np.float64) + np.array([0.5, 0.5, -0.5]) * tol * scale).astype(dtype)
    X.assert_within(inside, want, scale, letter, "inside")
    outside = inside.copy()
    outside[1] = dtype(-2.0 - 3.0 * tol * 4.0)
    with pytest.raises(AssertionError, match=r"worst at 1"):
        X.assert_within(outside, want, scale, letter, "outside")
    if letter in "CZ":            # an error in the imaginary part alone counts
        rot = inside.copy()
        rot[2] = dtype(3.0 + 3j * tol * 3.0)
        with pytest.raises(AssertionError, match=r"worst at 2"):
            X.assert_within(rot, want, scale, letter, "imaginary")
    nan = inside.copy()
    nan[0] = np.nan
    with pytest.raises(AssertionError, match=r"worst at 0"):
        X.assert_within(nan, want, scale, letter, "nan")


def test_unordered_escape_count():
    """The frozen form's rule on a hand-made group: offsets 65 533 / 65 534 fit, 65 535 / 65 536 and negative columns escape."""
    rows = np.zeros(7, np.int64)
    cols = np.array([10, 10 + 65533, 10 + 65534, 10 + 65535, 10 + 65536, -1, 500000])
    assert X.unordered_escapes(1, rows, cols, "D") == (7, 4)
    # another group (row 128 for the 8-byte types, row 32 for fp32) counts from its own lowest column
    rows2 = np.array([0, 0, 128, 128])
    cols2 = np.array([0, 65534, 70000, 70000 + 65535])
    assert X.unordered_escapes(129, rows2, cols2, "D") == (4, 1)
    assert X.unordered_escapes(129, rows2, cols2, "S") == (4, 1)
    assert X.unordered_escapes(129, np.array([0, 0, 31, 32]), np.array([0, 65534, 65535, 65535]), "S") == (4, 1)
    assert X.freeze_keeps(100, 1) and not X.freeze_keeps(100, 2) and not X.freeze_keeps(99, 1) and X.freeze_keeps(5, 5, 100)


@pytest.mark.parametrize("base", [0, 1])
def test_hell_coo_gives_back_the_triplets(golden_dir, base):
    """The entries read out of a HELL matrix (the tests' way to the exact product of a matrix built on the device) are the COO
    triplets it was built from, in the matrix' base."""
    from spgpu_amd import formats
    with np.load(os.path.join(golden_dir, "powerlaw_d_b1_h64.npz")) as f:
        n, b0 = int(f["n_rows"]), int(f["base"])
        rows, cols, vals = f["coo_rows"] - b0, f["coo_cols"] - b0, f["coo_vals"]
    hell = formats.ell_to_hell(formats.coo_to_ell(n, rows + base, cols + base, vals, coo_base=base, ell_base=base), 64)
    r, c, v = X.hell_coo(hell)
    assert sorted(zip(r.tolist(), c.tolist(), v.tolist())) == sorted(zip((rows + base).tolist(), (cols + base).tolist(), vals.tolist()))
    x = np.random.default_rng(1).standard_normal(int(cols.max()) + 1)
    z1, s1 = X.spmv(n, r, c, v, x, None, 1.5, 0.0, base=base)
    z2, s2 = X.spmv(n, rows, cols, vals, x, None, 1.5, 0.0)
    assert np.max(np.abs(z1 - z2)) <= 1e-15 * np.max(s2) and np.allclose(s1, s2, rtol=1e-15, atol=0)


# ---- the Level-1 references ---------------------------------------------------------------------------------------------------

def test_level1_hand_computed_real():
    x, y, z = np.array([1.0, -2.0, 0.5]), np.array([4.0, 0.25, -8.0]), np.array([10.0, -1.0, 3.0])
    alpha, beta = 1.5, -0.75
    cases = {"axpby": ([-1.5, -3.1875, 6.75], [4.5, 3.1875, 6.75]),            # 1.5 x - 0.75 y ; |1.5 x| + |0.75 y|
             "scal": ([1.5, -3.0, 0.75], [1.5, 3.0, 0.75]),
             "abs": ([1.5, 3.0, 0.75], [1.5, 3.0, 0.75]),
             "axy": ([6.0, -0.75, -6.0], [6.0, 0.75, 6.0]),
             "axypbz": ([-1.5, 0.0, -8.25], [13.5, 1.5, 8.25]),                 # 1.5 x y - 0.75 z
             "scat": ([-2.0, -2.1875, 6.5], [4.0, 2.1875, 6.5])}               # -0.75 y + x
    for op, (want, scale) in cases.items():
        out, s = X.level1(op, "D", alpha, x, y, beta, z)
        assert out.dtype == np.longdouble and out.astype(np.float64).tolist() == want, op
        assert s.astype(np.float64).tolist() == scale, op


def test_level1_hand_computed_complex():
    x, y, z = np.array([1 + 2j, -3j]), np.array([2 - 1j, 1 + 1j]), np.array([1j, 4.0])
    alpha, beta = 2j, 1 - 1j
    out, s = X.level1("axpby", "Z", alpha, x, y, beta)
    assert out.dtype == np.clongdouble and out.astype(np.complex128).tolist() == [-4 + 2j - 3j + 1, 6 + 2]
    np.testing.assert_allclose(s.astype(np.float64), [2 * 5 ** 0.5 + 2 ** 0.5 * 5 ** 0.5, 6 + 2], rtol=1e-15)
    out, s = X.level1("abs", "C", alpha, np.array([3 + 4j, -5j], np.complex64))
    assert out.astype(np.complex128).tolist() == [10j, 10j] and s.astype(np.float64).tolist() == [10.0, 10.0]
    out, s = X.level1("axypbz", "Z", alpha, x, y, beta, z)
    assert out.astype(np.complex128).tolist() == [2j * (4 + 3j) + (1 - 1j) * 1j, 2j * (3 - 3j) + (1 - 1j) * 4]
    out, _ = X.level1("axy", "Z", alpha, x, y)
    assert out.astype(np.complex128).tolist() == [2j * (4 + 3j), 2j * (3 - 3j)]
    out, _ = X.level1("scat", "Z", 1.0, x, y, beta)
    assert out.astype(np.complex128).tolist() == [(1 - 1j) * (2 - 1j) + 1 + 2j, (1 - 1j) * (1 + 1j) - 3j]


def test_level1_zero_coefficients_leave_operands_unread():
    """The routes of the reference's dispatch: the operand a route does not read may be NaN or absent."""
    x, y, z = np.array([1.0, 2.0]), np.array([3.0, 4.0]), np.array([5.0, 6.0])
    nan = np.full(2, np.nan)
    assert X.level1_route("axpby", 2.0, 0.0) == "scal" and X.level1_route("axypbz", 0.0, 2.0) == "scal_z"
    assert X.level1_route("axypbz", 2.0, 0j) == "axy" and X.level1_route("scat", 1.0, 0.0) == "copy"
    assert X.level1_route("axypbz", 2.0, 1e-300) == "axypbz"
    assert X.level1("axpby", "D", 2.0, x, nan, 0.0)[0].astype(float).tolist() == [2.0, 4.0]
    assert X.level1("axpby", "D", 2.0, x, None, 0.0)[0].astype(float).tolist() == [2.0, 4.0]
    assert X.level1("axypbz", "D", 0.0, nan, nan, 3.0, z)[0].astype(float).tolist() == [15.0, 18.0]
    assert X.level1("axypbz", "D", 2.0, x, y, 0.0, nan)[0].astype(float).tolist() == [6.0, 16.0]
    assert X.level1("scat", "D", 1.0, x, nan, 0.0)[0].astype(float).tolist() == [1.0, 2.0]
    assert np.isnan(X.level1("axypbz", "D", 2.0, x, y, 1.0, nan)[0].astype(float)).all()


def test_level1_k_of_each_operation():
    """The table of level1_k's docstring, spelled out: real / complex, and the shorter trees behind a zero coefficient."""
    full = {"scal": (1, 2), "abs": (1, 6), "axy": (2, 4), "axpby": (2, 4), "axypbz": (2, 4), "scat": (1, 2)}
    assert set(full) == set(X.LEVEL1_OPS)
    for op, (real, cplx) in full.items():
        for letter in "SD":
            assert X.level1_k(op, letter, 1.5, -0.75) == real, (op, letter)
        for letter in "CZ":
            assert X.level1_k(op, letter, 1.5 - 0.5j, 2j) == cplx, (op, letter)
    assert X.level1_k("axpby", "D", 1.5, 0.0) == 1 and X.level1_k("axpby", "Z", 1.5, 0.0) == 2
    assert X.level1_k("axypbz", "S", 0.0, 2.0) == 1 and X.level1_k("axypbz", "C", 0.0, 2.0) == 2
    assert X.level1_k("axypbz", "S", 2.0, 0.0) == 2 and X.level1_k("axypbz", "C", 2.0, 0.0) == 4
    assert X.level1_k("scat", "D", 1.0, 0.0) == 0 and X.level1_k("scat", "Z", 1.0, 0.0) == 0
    assert X.level1_k("abs", "D", 1.0) == 0 and X.level1_k("abs", "Z", 1.0) == 4
    assert X.EPS["S"] == X.EPS["C"] == 2.0 ** -24 and X.EPS["D"] == X.EPS["Z"] == 2.0 ** -53


@pytest.mark.parametrize("letter", ["S", "D", "C", "Z"])
@pytest.mark.parametrize("op", X.LEVEL1_OPS)
def test_level1_bound_holds_for_the_rounded_value_and_fails_outside(letter, op):
    """The long double value rounded once to the type (half an ulp per component, less than any k >= 1 allows; k = 0 is a copy and
    exact) lies inside the bound; a value k + 1 bounds away does not, and the report names its index.  Chunked with several
    workers = unchunked."""
    rng = np.random.default_rng(3)
    n = 1000
    dt = X.DTYPE_OF[letter]
    mk = lambda: (rng.standard_normal(n) + (1j * rng.standard_normal(n) if letter in "CZ" else 0)).astype(dt)
    x, y, z = mk(), mk(), mk()
    alpha, beta = (dt(1.5 - 0.5j), dt(-0.75 + 2j)) if letter in "CZ" else (dt(1.5), dt(-0.75))
    want, scale = X.level1(op, letter, alpha, x, y, beta, z)
    got = want.astype(dt)                                  # the correctly rounded result: half an ulp per component
    X.assert_level1(op, letter, got, alpha, x, y, beta, z)
    whole = X.level1_worst(op, letter, got, alpha, x, y, beta, z)
    parts = X.level1_worst(op, letter, got, alpha, x, y, beta, z, chunk=7, workers=3)
    assert whole == parts and whole[0] == 0 and whole[1] <= 0
    bad = got.copy()
    k = X.level1_k(op, letter, alpha, beta)
    bad[617] = dt(want[617] + 2 * (2 * k + 2) * X.EPS[letter] * scale[617])
    with pytest.raises(AssertionError, match=r"1 of 1000 outside .* worst at 617"):
        X.assert_level1(op, letter, bad, alpha, x, y, beta, z, chunk=64, workers=2)
    bad = got.copy()
    bad[3] = np.nan
    assert X.level1_worst(op, letter, bad, alpha, x, y, beta, z, chunk=5)[::2] == (1, 3)


def test_integer_sums_hand_computed():
    a, b = np.array([1.0, -2.0, 0.0, 3.0], np.float32), np.array([2.0, 3.0, 5.0, -1.0], np.float32)
    s = X.integer_sums("S", a, b)
    assert s == {"nrm2sq": 14, "asum": 6, "amax": 3, "dot": (-7, 0), "dot_terms": 11}
    c, d = np.array([1 + 2j, -3j], np.complex64), np.array([2 - 1j, 1 + 1j], np.complex64)
    s = X.integer_sums("C", c, d)                          # un-conjugated: (1+2j)(2-1j) + (-3j)(1+1j) = 4+3j + 3-3j
    assert s["dot"] == (7, 0) and s["nrm2sq"] == 14 and s["asum"] is None and s["amax"] is None
    assert s["dot_terms"] == max(2 + 2 + 0 + 3, 1 + 4 + 0 + 3)
    s = X.integer_sums("Z", np.array([3j, -2.0, 0.0]))
    assert s["asum"] == 5 and s["amax"] == 3 and s["nrm2sq"] == 13
    with pytest.raises(AssertionError, match="not integer-valued"):
        X.integer_sums("D", np.array([0.5]))
    X.assert_sums_exact("S", {"nrm2sq": (1 << 24) - 1, "asum": None})
    with pytest.raises(AssertionError, match="nrm2sq"):
        X.assert_sums_exact("S", {"nrm2sq": 1 << 24})
    X.assert_sums_exact("D", {"dot_terms": 1 << 24})
    assert X.rounded_sqrt("S", 14) == np.sqrt(np.float32(14)) and X.rounded_sqrt("D", 14) == 14 ** 0.5
    assert X.rounded_sqrt("S", 14).dtype == np.float32


def test_integer_vectors_are_what_they_say():
    for letter in "SDCZ":
        v = X.integer_vector(letter, 5, 100_000, support_seed=9)
        w = X.integer_vector(letter, 6, 100_000, support_seed=9)
        assert v.dtype == X.DTYPE_OF[letter] and np.array_equal(v != 0, w != 0) and not np.array_equal(v, w)
        share = np.count_nonzero(v) / v.size
        assert 0.02 < share < 0.04 and np.all(v[:8] != 0) and np.all(v[-8:] != 0)
        comps = np.concatenate([v.real, v.imag]) if letter in "CZ" else v
        assert set(np.unique(comps)) == {-3, -2, -1, 0, 1, 2, 3}
    axis = X.integer_vector("C", 7, 100_000, axis_only=True)
    assert not np.any((axis.real != 0) & (axis.imag != 0)) and np.any(axis.real != 0) and np.any(axis.imag != 0)
    assert X.integer_density("S", 1000) == 0.03 and X.integer_density("S", 1 << 26) < 0.02 and X.integer_density("D", 1 << 30) == 0.03


@pytest.mark.parametrize("letter", ["S", "D", "C", "Z"])
def test_chosen_integer_inputs_keep_every_partial_sum_exact(letter):
    """The vectors tests/test_gpu_level1_shapes.py reduces at its two largest sizes (same seeds, same makers): the sum of the
    magnitudes of the terms of dot, nrm2^2 and asum is below 2^24 / 2^53, and well above zero (a lost tile would show)."""
    import level1_launch_shapes as shapes
    sizes = [(*shapes.REDUCE_CAP_SEEDS, shapes.n_past_reduce_cap(letter))] + \
        ([(*shapes.REDUCE_NT_SEEDS, shapes.n_reduce_nt(letter))] if letter != "Z" else [])
    for seed, axis_seed, n in sizes:
        a, b, sums = X.integer_pair(letter, seed, n)          # asserts the condition itself
        v, vs = X.axis_vector(letter, axis_seed, n)
        limit = X.EXACT_LIMIT[letter]
        assert max(sums["nrm2sq"], sums["dot_terms"], vs["asum"]) < limit
        tiles = n // (shapes.TILE * shapes.WIDE[letter])
        assert min(sums["nrm2sq"], sums["dot_terms"], vs["asum"]) > 20 * tiles       # tens of terms per tile of 1 024 packs
        assert sums["dot"] != (0, 0) and a[-1] * b[-1] != 0 and v[-1] != 0            # the tail element counts
