"""Extended-precision references for the SpMV / SpMM tests, independent of every launch decision of the library.

The product is z* = alpha * sum_j a_ij x_j + beta * y, summed from COO triplets in long double (numpy's longdouble /
clongdouble), with the north_star magnitude of each row beside it:

    scale_i = |alpha| * sum_j |a_ij x_j| + |beta y_i|

and the bound a result must keep: |z_i - z*_i| <= tol * scale_i + tiny, tol 1e-6 (fp64, complex fp64) / 1e-4 (fp32, complex fp32).
Nothing here knows about hacks, slabs, groups of rows or the order in which a kernel adds: that is the point of it.

Row order (rIdx): row i of the matrix as stored is written to z[rIdx[i]] and y is read there too, the ABI's contract
(hell.h / ell.h).  Entries whose column lies below the index base (holes: a stored column of -1 in a 1-based matrix) are
never used, as in every kernel of the family."""
import numpy as np

TOL = {"S": 1e-4, "C": 1e-4, "D": 1e-6, "Z": 1e-6}
TINY = 1e-300
REAL_OF = {"S": np.float32, "D": np.float64, "C": np.float32, "Z": np.float64}
DTYPE_OF = {"S": np.float32, "D": np.float64, "C": np.complex64, "Z": np.complex128}


def _wide(*arrays, alpha=0.0, beta=0.0):
    cplx = any(np.iscomplexobj(a) for a in arrays if a is not None) or np.iscomplexobj(alpha) or np.iscomplexobj(beta)
    return np.clongdouble if cplx else np.longdouble


def spmv(n, rows, cols, vals, x, y, alpha, beta, r_idx=None, base=0):
    """(z*, scale) of an SpMV given by COO triplets (rows, cols in `base`); y may be None when beta == 0."""
    rows = np.asarray(rows, np.int64) - base
    cols = np.asarray(cols, np.int64) - base
    vals = np.asarray(vals)
    wide = _wide(vals, x, y, alpha=alpha, beta=beta)
    used = cols >= 0
    rows, cols, vals = rows[used], cols[used], vals[used]
    if r_idx is not None:
        rows = np.asarray(r_idx, np.int64)[rows]
    prod = vals.astype(wide) * np.asarray(x).astype(wide)[cols]
    acc = np.zeros(n, wide)
    np.add.at(acc, rows, prod)
    mag = np.zeros(n, np.longdouble)
    np.add.at(mag, rows, np.abs(prod))
    z = wide(alpha) * acc
    scale = np.longdouble(abs(alpha)) * mag
    if beta != 0:
        by = wide(beta) * np.asarray(y).astype(wide)
        z = z + by
        scale = scale + np.abs(by)
    return z, scale.astype(np.float64)


def spmm(n, rows, cols, vals, X, Y, alpha, beta, count, ldx=None, ldy=None, r_idx=None, base=0):
    """(Z*, scale) of an SpMM with interleaved multivectors: X[c * ldx + k] is x_k[c], Y[r * ldy + k] is y_k[r] (flat arrays or 2-D
    with rows of ld elements).  Returns [n, count] arrays: column k of the product."""
    X = np.asarray(X).reshape(-1)
    ldx = count if ldx is None else ldx
    assert ldx >= count
    cols_n = X.size // ldx
    Xk = X[:cols_n * ldx].reshape(cols_n, ldx)[:, :count]
    if Y is not None:
        Y = np.asarray(Y).reshape(-1)
        ldy = count if ldy is None else ldy
        assert ldy >= count
        Yk = Y[:n * ldy].reshape(n, ldy)[:, :count]
    Z = None
    S = np.zeros((n, count))
    for k in range(count):
        z, s = spmv(n, rows, cols, vals, Xk[:, k], Yk[:, k] if Y is not None else None, alpha, beta, r_idx=r_idx, base=base)
        if Z is None:
            Z = np.zeros((n, count), z.dtype)
        Z[:, k] = z
        S[:, k] = s
    if Z is None:
        Z = np.zeros((n, count), _wide(vals, X, alpha=alpha, beta=beta))
    return Z, S


def violations(got, want, scale, letter):
    """Per-element |got - want| - bound (positive: outside the bound; NaN counts as outside)."""
    got = np.asarray(got)
    err = np.abs(got.astype(want.dtype) - want).astype(np.float64)
    bound = TOL[letter] * np.asarray(scale, np.float64) + TINY
    return np.where(np.isnan(err), np.inf, err - bound)


def assert_within(got, want, scale, letter, case=""):
    """|got - want| <= tol * scale + tiny, element by element; on failure the worst element, what it holds and what it should."""
    over = violations(got, want, scale, letter)
    if over.size == 0 or np.all(over <= 0):
        return
    flat = int(np.argmax(over))
    at = np.unravel_index(flat, over.shape)
    at = at[0] if len(at) == 1 else at
    got_a = np.asarray(got)
    bad = int(np.count_nonzero(over > 0))
    raise AssertionError(f"{case}: {bad} of {over.size} outside tol {TOL[letter]:g} x scale; worst at {at}: got {got_a[at]!r}, "
                         f"want {complex(want[at]) if np.iscomplexobj(want) else float(want[at])!r}, "
                         f"scale {float(np.asarray(scale)[at]):.6g}")


# ---- the 16-bit copy's rule (include/spgpu/tuning.h, Freeze) ------------------------------------------------------------

def group_rows_of(letter):
    """Rows of one group of the unordered frozen form: those one wavefront of the default kernel owns."""
    return {"S": 32, "D": 128, "C": 128}[letter]


def unordered_escapes(n, rows, cols, letter, base=0):
    """(entries, escapes) of the unordered frozen form as tuning.h states it: per group of rows, offsets from the group's lowest
    column (>= 0); an entry whose column is negative or 65 535 or more above that lowest is an escape."""
    rows = np.asarray(rows, np.int64) - base
    cols = np.asarray(cols, np.int64) - base
    g = rows // group_rows_of(letter)
    lowest = np.full((n + group_rows_of(letter) - 1) // group_rows_of(letter) + 1, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(lowest, g[cols >= 0], cols[cols >= 0])
    off = cols - lowest[g]
    escapes = int(np.count_nonzero((cols < 0) | (off >= 0xFFFF)))
    return int(rows.size), escapes


def freeze_keeps(entries, escapes, pct=1):
    """The share rule: a copy is kept if escapes * 100 <= entries * pct."""
    return escapes * 100 <= entries * pct


def hell_coo(mat):
    """COO triplets (rows and columns in the matrix' base, values) of the entries of a host HELL dict (spgpu_amd.formats.ell_to_hell's
    keys): row i's k-th entry is slot hack_offsets[i / hack] + i % hack + k * hack.  Pass base=mat["base"] on to spmv / spmm."""
    n, hack = mat["rows"], mat["hack_size"]
    lengths = np.asarray(mat["row_lengths"][:n], np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), lengths)
    k = np.arange(rows.size, dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    slots = np.asarray(mat["hack_offsets"], np.int64)[rows // hack] + rows % hack + k * hack
    return rows + mat["base"], np.asarray(mat["indices"])[slots].astype(np.int64), np.asarray(mat["values"])[slots]
