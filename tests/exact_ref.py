"""Extended-precision references for the SpMV / SpMM tests and (second half of the file) the Level-1 tests, independent of every
launch decision of the library.

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


# ---- Level-1: element-wise operations in extended precision ------------------------------------------------------------------
#
# out_i of each operation of spgpu_amd/csrc/level1.hip evaluated in longdouble / clongdouble, with scale_i = the sum of the magnitudes
# of its terms, and the bound  |got_i - out_i| <= 2 * k * eps * scale_i + tiny.  eps is the unit roundoff of the real type and k the
# number of rounded operations on the longest path of the expression tree the kernel evaluates (level1_k).  The factor 2 pays for
# the second-order terms and, for the complex types, for the step from an error per component to the modulus of the error (sqrt 2).

EPS = {"S": 2.0 ** -24, "C": 2.0 ** -24, "D": 2.0 ** -53, "Z": 2.0 ** -53}
LEVEL1_OPS = ("axpby", "scal", "abs", "axy", "axypbz", "scat")


def _is_zero(v):
    return complex(v) == 0


def level1_route(op, alpha, beta):
    """The expression a call evaluates after the dispatch on zero coefficients: axpby with beta == 0 is alpha*x (y is not read),
    axypbz with alpha == 0 is scal(beta, z) and with beta == 0 is axy (axy_base.cuh:139-176), scat with beta == 0 is a copy."""
    if op == "axpby" and _is_zero(beta):
        return "scal"
    if op == "axypbz":
        return "scal_z" if _is_zero(alpha) else ("axy" if _is_zero(beta) else "axypbz")
    if op == "scat" and _is_zero(beta):
        return "copy"
    return op


def level1_k(op, letter, alpha=1.0, beta=1.0):
    """Rounded operations on the longest path of the expression tree, as level1.hip and numeric.hip.h write it.

    Real types (S, D); a product, a sum and a fused multiply-add round once each:
      scal    alpha*x                                  1
      abs     alpha*|x|  (|x| is exact)                1     (alpha == 1: the multiply is skipped, 0)
      axy     alpha*(x*y)                              2
      axpby   fma(alpha, x, beta*y)                    2     (beta == 0: alpha*x, 1)
      axypbz  fma(alpha, x*y, beta*z)                  2     (x*y -> fma, or beta*z -> fma; routed to scal 1 / axy 2 on a zero)
      scat    fma(beta, y, v)                          1     (beta == 0: a copy, 0)
    Complex types (C, Z); a complex multiply counted as its real operations.  mul(a, b) is re = fma(a.x, b.x, -(a.y*b.y)),
    im = fma(a.x, b.y, a.y*b.x): a product and an fma, 2.  mulAdd(p, q, r) is re = fma(-p.y, q.y, fma(p.x, q.x, r.x)) and the like
    for im: two fma on top of r, 2 more than r's own depth:
      scal    mul(alpha, x)                            2
      axy     mul(alpha, mul(x, y))                    4
      axpby   C: mulAdd(beta, y, mul(alpha, x))        4     Z: mulAdd(alpha, x, mul(beta, y))  4     (beta == 0: mul, 2)
      axypbz  mulAdd(alpha, mul(x, y), mul(beta, z))   4     (routed to scal 2 / axy 4 on a zero)
      scat    mulAdd(beta, y, v)                       2     (beta == 0: 0)
      abs     magnitude(): w/v, fma(t, t, 1), sqrt, v*  4, then mul(alpha, (m, 0))  +2 = 6   (alpha == 1: 4)
    """
    route = level1_route(op, alpha, beta)
    cplx = letter in "CZ"
    if route == "copy":
        return 0
    if route in ("scal", "scal_z"):
        return 2 if cplx else 1
    if route == "abs":
        one = complex(alpha) == 1
        return (4 if one else 6) if cplx else (0 if one else 1)
    if route == "axy":
        return 4 if cplx else 2
    if route in ("axpby", "axypbz"):
        return 4 if cplx else 2
    if route == "scat":
        return 2 if cplx else 1
    raise ValueError(op)


def level1(op, letter, alpha, x, y=None, beta=0.0, z=None):
    """(out*, scale) of one Level-1 operation on whole vectors, in long double.  Operands (level1.hip's names):
      axpby  alpha*x + beta*y            scal   alpha*x             abs     alpha*|x|
      axy    alpha*x*y                   axypbz alpha*x*y + beta*z  scat    beta*y + x   (x: the values, y: vector[indices - base])
    An operand that the route does not read (level1_route) is not touched here either: it may be None or full of NaN."""
    wide = np.clongdouble if letter in "CZ" else np.longdouble
    route = level1_route(op, alpha, beta)
    w = lambda a: np.asarray(a).astype(wide)
    al, be = wide(alpha), wide(beta)
    if route == "copy":
        out = w(x)
        return out, np.abs(out).astype(np.longdouble)
    if route == "scal":
        out = al * w(x)
        return out, np.abs(out).astype(np.longdouble)
    if route == "scal_z":
        out = be * w(z)
        return out, np.abs(out).astype(np.longdouble)
    if route == "abs":
        out = al * np.abs(w(x)).astype(wide)
        return out, np.abs(out).astype(np.longdouble)
    if route == "axy":
        out = al * (w(x) * w(y))
        return out, np.abs(out).astype(np.longdouble)
    if route == "axpby":
        t1, t2 = al * w(x), be * w(y)
    elif route == "axypbz":
        t1, t2 = al * (w(x) * w(y)), be * w(z)
    elif route == "scat":
        t1, t2 = w(x), be * w(y)
    else:
        raise ValueError(op)
    return t1 + t2, (np.abs(t1) + np.abs(t2)).astype(np.longdouble)


def level1_bound(op, letter, scale, alpha=1.0, beta=1.0):
    return 2 * level1_k(op, letter, alpha, beta) * np.longdouble(EPS[letter]) * scale + TINY


def level1_worst(op, letter, got, alpha, x, y=None, beta=0.0, z=None, chunk=1 << 18, workers=1):
    """(count outside the bound, worst |got - out*| - bound, its index) over the whole vector, evaluated `chunk` elements at a time
    (about ten long double temporaries of `chunk` elements are alive at once per worker: 2^18 elements are 4 MB each, 8 MB
    complex, so 8 workers hold well under a GB), chunks spread over `workers` threads.
    NaN in got counts as outside."""
    got = np.asarray(got)
    n = got.size
    sl = lambda a, s: None if a is None else np.asarray(a)[s]

    def one(lo):
        s = slice(lo, min(lo + chunk, n))
        want, scale = level1(op, letter, alpha, sl(x, s), sl(y, s), beta, sl(z, s))
        err = np.abs(got[s].astype(want.dtype) - want)
        over = err - level1_bound(op, letter, scale, alpha, beta)
        over = np.where(np.isnan(over), np.inf, over)
        at = int(np.argmax(over)) if over.size else 0
        return int(np.count_nonzero(over > 0)), float(over[at]) if over.size else -np.inf, lo + at

    starts = range(0, n, chunk)
    if workers > 1 and n > chunk:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=workers) as pool:
            parts = list(pool.map(one, starts))
    else:
        parts = [one(lo) for lo in starts]
    bad = sum(p[0] for p in parts)
    worst = max(parts, key=lambda p: p[1], default=(0, -np.inf, 0))
    return bad, worst[1], worst[2]


def assert_level1(op, letter, got, alpha, x, y=None, beta=0.0, z=None, case="", chunk=1 << 18, workers=1):
    bad, over, at = level1_worst(op, letter, got, alpha, x, y, beta, z, chunk=chunk, workers=workers)
    if bad:
        raise AssertionError(f"{case or op}: {bad} of {np.asarray(got).size} outside 2*{level1_k(op, letter, alpha, beta)}*eps*scale; "
                             f"worst at {at}: got {np.asarray(got)[at]!r}, excess {over:.3g}")


# ---- Level-1: reductions whose result does not depend on the order of addition ------------------------------------------------
#
# Integer-valued, sparse vectors: values in {-3 ... 3}, a few percent nonzero.  If the sum of the magnitudes of all the terms a
# reduction adds stays below 2^24 (fp32) / 2^53 (fp64), every partial sum in every order is an integer the format holds exactly,
# every fused multiply-add on the way is exact, and the result IS the integer a host computes in int64.

EXACT_LIMIT = {"S": 1 << 24, "C": 1 << 24, "D": 1 << 53, "Z": 1 << 53}


def integer_density(letter, n):
    """Share of nonzero elements: 3 %, less where n is so large that the expected sum of squares (14/3 per nonzero component, two
    components for the complex types) would pass a quarter of the limit."""
    comps = 2 if letter in "CZ" else 1
    return min(0.03, EXACT_LIMIT[letter] / 4 / (n * comps * 14.0 / 3.0))


def integer_vector(letter, seed, n, support_seed=None, axis_only=False, density=None):
    """Sparse vector of small integers (Gaussian integers for C and Z).  Vectors made with one support_seed are nonzero at the
    same places (so that their dot product has as many terms as each has elements); axis_only: complex elements with one zero
    component, whose modulus is exact.  The first and the last 8 elements are always nonzero (first pack, last pack and tail)."""
    density = integer_density(letter, n) if density is None else density
    mask = np.random.default_rng(seed if support_seed is None else support_seed).random(n, dtype=np.float32) < density
    mask[:8] = True
    mask[-8:] = True
    rng = np.random.default_rng(seed + 1000003)
    real = REAL_OF[letter]

    def component():
        v = rng.integers(1, 4, n, dtype=np.int8) * (rng.integers(0, 2, n, dtype=np.int8) * 2 - 1)
        return (v * mask).astype(real)

    if letter in "SD":
        return component()
    out = np.zeros(n, DTYPE_OF[letter])
    if axis_only:
        v, which = component(), rng.integers(0, 2, n, dtype=np.int8).astype(bool)
        out.real, out.imag = np.where(which, v, 0), np.where(which, 0, v)
    else:
        out.real, out.imag = component(), component()
    return out


def _ints(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        re, im = a.real.astype(np.int64), a.imag.astype(np.int64)
        assert np.array_equal(re, a.real) and np.array_equal(im, a.imag), "not integer-valued"
        return re, im
    re = a.astype(np.int64)
    assert np.array_equal(re, a), "not integer-valued"
    return re, None


def integer_sums(letter, a, b=None):
    """Exact results in int64 and, beside each, the sum of the magnitudes of the terms its accumulator adds:
      dot (with b): (re, im) of sum a_i*b_i, un-conjugated; terms per component: re a.x*b.x and a.y*b.y, im a.x*b.y and a.y*b.x
      nrm2sq: sum |a_i|^2 (its terms are non-negative: the magnitude sum is the result)
      asum:   sum |a_i|, for complex vectors only where every element has a zero component (None otherwise)
      amax:   max |a_i| under the same condition."""
    ar, ai = _ints(a)
    out = {}
    cplx = ai is not None
    out["nrm2sq"] = int(np.sum(ar * ar) + (np.sum(ai * ai) if cplx else 0))
    if not cplx or not np.any((ar != 0) & (ai != 0)):
        mag = np.abs(ar) + (np.abs(ai) if cplx else 0)
        out["asum"], out["amax"] = int(mag.sum()), int(mag.max(initial=0))
    else:
        out["asum"] = out["amax"] = None
    if b is not None:
        br, bi = _ints(b)
        if cplx:
            out["dot"] = (int(np.sum(ar * br) - np.sum(ai * bi)), int(np.sum(ar * bi) + np.sum(ai * br)))
            out["dot_terms"] = max(int(np.sum(np.abs(ar * br)) + np.sum(np.abs(ai * bi))),
                                   int(np.sum(np.abs(ar * bi)) + np.sum(np.abs(ai * br))))
        else:
            out["dot"] = (int(np.sum(ar * br)), 0)
            out["dot_terms"] = int(np.sum(np.abs(ar * br)))
    return out


def assert_sums_exact(letter, sums):
    """The condition on the inputs under which a reduction in the type's precision is exact in any order of addition."""
    limit = EXACT_LIMIT[letter]
    for key in ("nrm2sq", "asum", "dot_terms"):
        if sums.get(key) is not None:
            assert sums[key] < limit, f"{key}: sum of term magnitudes {sums[key]} not below {limit}"


def integer_pair(letter, seed, n):
    """(a, b, their exact sums) with the exactness condition asserted; (axis vector, its sums) for asum / amax."""
    a = integer_vector(letter, seed, n, support_seed=seed)
    b = integer_vector(letter, seed + 1, n, support_seed=seed)
    sums = integer_sums(letter, a, b)
    assert_sums_exact(letter, sums)
    return a, b, sums


def axis_vector(letter, seed, n):
    v = integer_vector(letter, seed, n, axis_only=True)
    sums = integer_sums(letter, v)
    assert sums["asum"] is not None
    assert_sums_exact(letter, sums)
    return v, sums


def rounded_sqrt(letter, value):
    """sqrt of an exactly representable integer, correctly rounded in the real type of `letter` (IEEE sqrt of numpy)."""
    real = REAL_OF[letter]
    assert int(real(value)) == value
    return np.sqrt(real(value))
