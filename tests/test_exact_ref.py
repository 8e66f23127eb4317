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
