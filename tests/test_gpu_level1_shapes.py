"""GPU: the Level-1 set (spgpu_amd/csrc/level1.hip, reduce.hip.h) on every launch shape its dispatch can choose.

The launchers pick among kernel instantiations by size, alignment, pitch and vector count; this module computes the sizes at
which each choice flips from the constants below and runs every operation there:

  * past the grid caps (a second trip of the tile-stride loop, a ragged last tile, a non-empty tail),
  * past 256 MiB streamed (the non-temporal instantiations),
  * one element past a 16-byte boundary and with odd pitches (VEC = 1),
  * with so many vectors that the per-vector block cap engages, and past 1 024 vectors (the second pass of reduceVectors),
  * gath / scat / setscal past one sweep of their grid,
  * special values of the complex modulus, operands that must not be read, empty calls, in-place calls.

Element-wise results are checked twice: bit for bit against the oracle (a changed expression tree fails that) and against a
long double evaluation within 2*k*eps*scale (tests/exact_ref.py: an error shared by kernel and oracle fails that).  Reductions run on
sparse integer-valued vectors whose sums are exact in any order of addition, so that they must EQUAL the integer computed on
the host; the condition that makes them exact is asserted on the inputs before the GPU is called.

cdouble (Z) has WIDE = 1: mapKernel and reduceKernel have no wide and no non-temporal instantiation for it (both need WIDE > 1),
only axpbyKernel<cdouble, 1, ., NT> exists.  The Z cases below run the VEC = 1 kernels at the same sizes and say so."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_ref as X
import oracle_api as O

pytestmark = pytest.mark.gpu

# the constants of the dispatch, each with the source line that sets it, and the sizes computed from them: level1_launch_shapes.py
from level1_launch_shapes import (MAP_MAX_BLOCKS, NT_BYTES, RAGGED, REDUCE_CAP_SEEDS, REDUCE_MAX_BLOCKS, REDUCE_NT_SEEDS, SIZEOF, THREADS, TILE,
                                  WIDE, n_past_map_cap, n_past_reduce_cap, n_reduce_nt)

WORKERS = 8                                        # threads of the long double evaluation (a fixed number, not the machine's)

ALPHA = {"S": 1.5, "D": 1.5, "C": 1.5 - 0.5j, "Z": 1.5 - 0.5j}
BETA = {"S": -0.75, "D": -0.75, "C": -0.75 + 2j, "Z": -0.75 + 2j}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _hp(a):
    return C.c_void_p(a.ctypes.data)


def _dev(a):
    from spgpu_amd import formats
    return formats.to_device(a)


def _assert_aligned(*tensors):
    """Every device operand of a test that is there for a wide or non-temporal instantiation starts on a 16-byte boundary: off one,
    the launcher would take VEC = 1 (and, for maps and reductions, the plain kernel), with the same bits, and the test would not notice."""
    for t in tensors:
        assert t.data_ptr() % 16 == 0, "device operand off a 16-byte boundary: the wide kernel would not run"


def _rand(letter, seed, n):
    rng = np.random.default_rng(seed)
    real = X.REAL_OF[letter]
    if letter in "SD":
        return rng.standard_normal(n, dtype=real)
    return rng.standard_normal(2 * n, dtype=real).view(X.DTYPE_OF[letter])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 and a.dtype.kind != "c" else np.uint64)


def _assert_same_bits(got, want, case):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, case
    if not np.array_equal(g, w):
        at = int(np.flatnonzero(g != w)[0]) // (g.size // np.asarray(got).size)
        raise AssertionError(f"{case}: {np.count_nonzero(g != w)} words differ from the oracle, first at element {at}: "
                             f"got {np.asarray(got).reshape(-1)[at]!r}, want {np.asarray(want).reshape(-1)[at]!r}")


def _sc(letter, v):
    from spgpu_amd import capi
    return C.c_int(int(v)) if letter == "I" else capi.scalar(letter, v)


# ---- one calling convention for the element-wise operations: out = op(alpha, x, y, beta, z) --------------------------------------

def _launch(gpu, op, letter, out, n, alpha, x, y=None, beta=0.0, z=None, count=None, pitch=0):
    from spgpu_amd import capi
    a, b = _sc(letter, alpha), _sc(letter, beta)
    m = () if count is None else (count, pitch)
    if op == "axpby":
        (capi.axpby if count is None else capi.maxpby)[letter](gpu, _p(out), n, b, _p(y), a, _p(x), *m)
    elif op == "scal":
        capi.scal[letter](gpu, _p(out), n, a, _p(x))
    elif op == "abs":
        capi.vabs[letter](gpu, _p(out), n, a, _p(x))
    elif op == "axy":
        (capi.axy if count is None else capi.maxy)[letter](gpu, _p(out), n, a, _p(x), _p(y), *m)
    elif op == "axypbz":
        (capi.axypbz if count is None else capi.maxypbz)[letter](gpu, _p(out), n, b, _p(z), a, _p(x), _p(y), *m)
    else:
        raise ValueError(op)


def _oracle(op, letter, n, alpha, x, y=None, beta=0.0, z=None):
    if op == "axpby":
        return O.axpby(letter, n, beta, y if complex(beta) != 0 else None, alpha, x)
    return O.level1_map(letter, op, n, alpha, x, y, beta, z)


def _check_both(case, op, letter, got, alpha, x, y=None, beta=0.0, z=None):
    """Bit for bit against the oracle, and within 2*k*eps*scale of the long double value."""
    n = got.size
    _assert_same_bits(got, _oracle(op, letter, n, alpha, x, y, beta, z), case)
    X.assert_level1(op, letter, got, alpha, x, y, beta, z, case=case, workers=WORKERS)


#: (name, op, uses y, beta, uses z): the element-wise calls of vector.h that have a dense launcher
MAP_CASES = [("axpby", "axpby", True, True, False), ("axpby_beta0", "axpby", False, False, False), ("scal", "scal", False, False, False),
             ("abs", "abs", False, False, False), ("axy", "axy", True, False, False), ("axypbz", "axypbz", True, True, True)]


# ==== 1. past the map cap: second trip, ragged last tile, tail, non-temporal ====================================================

@pytest.fixture(scope="module", params="SDCZ")
def capped(request, gpu):
    """x, y, z of n_past_map_cap elements on the host and on the device, one type at a time (about 270 MB each)."""
    import torch
    letter = request.param
    n = n_past_map_cap(letter)
    host = {k: _rand(letter, s, n) for k, s in (("x", 21), ("y", 22), ("z", 23))}
    dev = {k: _dev(v) for k, v in host.items()}
    out = torch.empty_like(dev["x"])
    _assert_aligned(out, *dev.values())
    case = dict(letter=letter, n=n, out=out, **host, **{"d" + k: v for k, v in dev.items()})
    yield case
    # every reference to the device tensors goes before the cache is emptied, so that the next type starts from a free pool
    case.clear()
    dev.clear()
    host.clear()
    del out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,op,use_y,use_beta,use_z", MAP_CASES, ids=[c[0] for c in MAP_CASES])
def test_maps_past_the_block_cap(gpu, capped, name, op, use_y, use_beta, use_z):
    """blocks = 16 384 (capped), so block 0 takes tile 0 and tile 16 384 and the last tile is ragged; n % WIDE != 0 for S, D, C.
    Every call streams at least 2 * n * sizeof >= 512 MiB: axpbyKernel<., WIDE, ., NT> and mapKernel<., WIDE, op, NT> for S, D, C;
    for Z axpbyKernel<cdouble, 1, ., NT> and the plain mapKernel<cdouble, 1, op> (no wide / NT map kernel exists for Z)."""
    import torch
    L, n = capped["letter"], capped["n"]
    blocks = -(-(-(-n // WIDE[L])) // TILE)
    assert blocks > MAP_MAX_BLOCKS and n * SIZEOF[L] * 2 >= NT_BYTES and (WIDE[L] == 1 or n % WIDE[L] != 0)
    beta = BETA[L] if use_beta else 0.0
    out = capped["out"]
    out.fill_(float("nan"))
    _launch(gpu, op, L, out, n, ALPHA[L], capped["dx"], capped["dy"] if use_y else None, beta, capped["dz"] if use_z else None)
    torch.cuda.synchronize()
    _check_both(f"{L}{name} n={n}", op, L, out.cpu().numpy(), ALPHA[L], capped["x"], capped["y"] if use_y else None, beta,
                capped["z"] if use_z else None)


def test_in_place_past_the_block_cap(gpu, capped):
    """scal and abs with y == x, axypbz with w == z, axpby with z == x at the capped, non-temporal size: a lane reads its elements
    before it writes them (the comment in axpbyLaunch), so the results are the out-of-place bits."""
    import torch
    L, n = capped["letter"], capped["n"]
    x, y, z = capped["x"], capped["y"], capped["z"]
    for name, op, target in (("scal", "scal", "x"), ("abs", "abs", "x"), ("axypbz", "axypbz", "z"), ("axpby", "axpby", "x")):
        d = {k: capped["d" + k] for k in "xyz"}
        d[target] = d[target].clone()
        _assert_aligned(d[target])
        _launch(gpu, op, L, d[target], n, ALPHA[L], d["x"], d["y"], BETA[L], d["z"])
        torch.cuda.synchronize()
        _assert_same_bits(d[target].cpu().numpy(), _oracle(op, L, n, ALPHA[L], x, y, BETA[L], z), f"{L}{name} in place on {target}")
        del d


@pytest.mark.parametrize("letter", "SD")
def test_axpby_device_past_the_block_cap(gpu, letter):
    """spgpu{S,D}axpbyDevice at the capped size (its grid is capped like axpbyLaunch's; it has no non-temporal form): the bits of the
    host-scalar call, with beta != 0, *beta == 0 and beta == NULL."""
    import torch
    from spgpu_amd import capi
    L, n = letter, n_past_map_cap(letter)
    x, y = _rand(L, 25, n), _rand(L, 26, n)
    dx, dy = _dev(x), _dev(y)
    coef = _dev(np.array([ALPHA[L], BETA[L], 0.0], X.DTYPE_OF[L]))
    z_dev, z_host = torch.empty_like(dx), torch.empty_like(dx)
    _assert_aligned(dx, dy, z_dev, z_host)
    for beta_ptr, beta in ((coef[1:], BETA[L]), (coef[2:], 0.0), (None, 0.0)):
        z_dev.fill_(float("nan"))
        capi.axpby_device[L](gpu, _p(z_dev), n, _p(beta_ptr), _p(dy), _p(coef[0:]), _p(dx))
        _launch(gpu, "axpby", L, z_host, n, ALPHA[L], dx, dy, beta)
        torch.cuda.synchronize()
        assert torch.equal(z_dev, z_host), f"{L}axpbyDevice beta={beta}"
        if beta != 0:
            _assert_same_bits(z_dev.cpu().numpy(), _oracle("axpby", L, n, ALPHA[L], x, y, beta), f"{L}axpbyDevice")
    _assert_same_bits(z_dev.cpu().numpy(), _oracle("axpby", L, n, ALPHA[L], x), f"{L}axpbyDevice beta=NULL")


def test_axpby_on_both_sides_of_the_non_temporal_threshold(gpu):
    """fp64 axpby with beta != 0 streams 24 n bytes: n = 11 184 810 is the last plain launch, 11 184 811 the first non-temporal
    one.  Both against the oracle and the long double value, and the common prefix of the two against each other."""
    import torch
    L = "D"
    over = -(-NT_BYTES // (3 * SIZEOF[L]))
    under = over - 1
    assert under * 3 * SIZEOF[L] < NT_BYTES <= over * 3 * SIZEOF[L]
    x, y = _rand(L, 31, over), _rand(L, 32, over)
    dx, dy = _dev(x), _dev(y)
    got = {}
    for n in (under, over):
        out = torch.full_like(dx, float("nan"))
        _assert_aligned(dx, dy, out)
        _launch(gpu, "axpby", L, out, n, ALPHA[L], dx, dy, BETA[L])
        torch.cuda.synchronize()
        got[n] = out.cpu().numpy()
        assert np.isnan(got[n][n:]).all()
        _check_both(f"Daxpby n={n}", "axpby", L, got[n][:n], ALPHA[L], x[:n], y[:n], BETA[L])
    _assert_same_bits(got[over][:under], got[under][:under], "non-temporal against plain")


# ==== 2. reductions: exact integers ==============================================================================================

def _dot(gpu, letter, n, da, db):
    from spgpu_amd import capi
    r = capi.dot[letter](gpu, n, _p(da), _p(db))
    return (r, 0) if letter in "SD" else (r.x, r.y)


def _check_reductions(gpu, letter, n, da, db, sums, case):
    from spgpu_amd import capi
    assert _dot(gpu, letter, n, da, db) == sums["dot"], f"{case}: dot"
    got = capi.nrm2[letter](gpu, n, _p(da))
    assert got == float(X.rounded_sqrt(letter, sums["nrm2sq"])), f"{case}: nrm2 {got!r}, nrm2^2 should be {sums['nrm2sq']}"


def planted_positions(letter, n, blocks):
    """Where a maximum can get lost: element index per place of a launch of `blocks` blocks with VEC = WIDE."""
    w = WIDE[letter]
    trip = blocks * TILE * w
    assert n > trip
    places = {"first pack": 0, "last pack of the first trip": trip - 1, "first pack of the second trip": trip,
              "last full pack": (n // w) * w - 1}
    if n % w:
        places["tail"] = n - 1      # Z (WIDE = 1) has no tail: every element is a full pack
    return places


@pytest.mark.parametrize("letter", "SDCZ")
def test_reductions_past_the_block_cap(gpu, letter):
    """1 024 blocks (capped) take a second trip over a ragged last tile and a tail: dot, nrm2^2 and asum must equal the host's
    integers, nrm2 the correctly rounded root, amax the planted maximum wherever it lies.  S and D: the device-scalar calls return
    the same bits.  (Z: reduceKernel<cdouble, 1, mode>, the only form it has.)"""
    import torch
    from spgpu_amd import capi
    n = n_past_reduce_cap(letter)
    assert -(-(-(-n // WIDE[letter])) // TILE) > REDUCE_MAX_BLOCKS
    a, b, sums = X.integer_pair(letter, REDUCE_CAP_SEEDS[0], n)
    da, db = _dev(a), _dev(b)
    _assert_aligned(da, db)
    _check_reductions(gpu, letter, n, da, db, sums, f"{letter} n={n}")
    if letter in "SD":
        out = torch.full((2,), float("nan"), dtype=da.dtype, device="cuda:0")
        capi.dot_device[letter](gpu, _p(out[0:]), n, _p(da), _p(db))
        capi.nrm2_device[letter](gpu, _p(out[1:]), n, _p(da))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[0] == sums["dot"][0] and got[1] == X.rounded_sqrt(letter, sums["nrm2sq"]), f"{letter} device scalars: {got}"
    v, vs = X.axis_vector(letter, REDUCE_CAP_SEEDS[1], n)
    dv = _dev(v)
    _assert_aligned(dv)
    assert capi.asum[letter](gpu, n, _p(dv)) == vs["asum"], f"{letter}asum"
    assert capi.amax[letter](gpu, n, _p(dv)) == vs["amax"] == 3
    for place, at in planted_positions(letter, n, REDUCE_MAX_BLOCKS).items():
        keep = dv[at].clone()
        dv[at] = 7j if letter in "CZ" else -7.0
        assert capi.amax[letter](gpu, n, _p(dv)) == 7, f"{letter}amax lost the maximum in the {place} (element {at})"
        dv[at] = keep
    assert capi.amax[letter](gpu, n, _p(dv)) == 3


@pytest.mark.parametrize("letter", "SDC")
def test_reductions_non_temporal(gpu, letter):
    """reduceKernel<., WIDE, mode, NT>: nrm2 and asum on 256 MiB + a ragged end, dot on two such vectors and on the two shortest
    that reach the threshold together (2 * n * sizeof == 256 MiB exactly).  Z has no such kernel (WIDE = 1)."""
    from spgpu_amd import capi
    n = n_reduce_nt(letter)
    assert n * SIZEOF[letter] >= NT_BYTES
    a, b, sums = X.integer_pair(letter, REDUCE_NT_SEEDS[0], n)
    da, db = _dev(a), _dev(b)
    _assert_aligned(da, db)
    _check_reductions(gpu, letter, n, da, db, sums, f"{letter} n={n}")
    half = NT_BYTES // (2 * SIZEOF[letter])
    for m in (half, half - 1):              # the first non-temporal dot and the last plain one
        s = X.integer_sums(letter, a[:m], b[:m])
        assert _dot(gpu, letter, m, da, db) == s["dot"], f"{letter}dot n={m}"
    del db
    v, vs = X.axis_vector(letter, REDUCE_NT_SEEDS[1], n)
    dv = _dev(v)
    _assert_aligned(dv)
    assert capi.asum[letter](gpu, n, _p(dv)) == vs["asum"]
    at = (n // WIDE[letter]) * WIDE[letter] - 1
    dv[at] = 7j if letter == "C" else 7.0
    assert capi.amax[letter](gpu, n, _p(dv)) == 7


# ==== 3. the narrow path (VEC = 1) of the host-scalar calls ======================================================================

@pytest.mark.parametrize("letter", "SDCZ")
def test_narrow_path_one_operand_off_a_16_byte_boundary(gpu, letter):
    """Each operand in turn one element past a 16-byte boundary (the others aligned): the launcher must take VEC = 1 for the whole
    call.  For Z every element is 16 bytes, so VEC = 1 is the only path and the offset changes nothing; it runs all the same."""
    import torch
    from spgpu_amd import capi
    n = 70_001
    host = {k: _rand(letter, s, n + 1) for k, s in (("x", 61), ("y", 62), ("z", 63))}
    dev = {k: _dev(v) for k, v in host.items()}
    assert letter == "Z" or (dev["x"].data_ptr() % 16 == 0 and dev["x"][1:].data_ptr() % 16 != 0)
    for name, op, use_y, use_beta, use_z in MAP_CASES:
        operands = ["out", "x"] + (["y"] if use_y else []) + (["z"] if use_z else [])
        beta = BETA[letter] if use_beta else 0.0
        for off in operands:
            o = {k: int(k == off) for k in ("out", "x", "y", "z")}
            out = torch.full((n + 1,), float("nan"), dtype=dev["x"].dtype, device="cuda:0")
            _launch(gpu, op, letter, out[o["out"]:], n, ALPHA[letter], dev["x"][o["x"]:], dev["y"][o["y"]:] if use_y else None, beta,
                    dev["z"][o["z"]:] if use_z else None)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.isnan(got[:o["out"]]).all() and np.isnan(got[o["out"] + n:]).all(), f"{letter}{name}: wrote outside, {off} off"
            _check_both(f"{letter}{name} with {off} one element off", op, letter, got[o["out"]:o["out"] + n], ALPHA[letter],
                        host["x"][o["x"]:o["x"] + n], host["y"][o["y"]:o["y"] + n] if use_y else None, beta,
                        host["z"][o["z"]:o["z"] + n] if use_z else None)
    # reductions: a, b each in turn
    a = X.integer_vector(letter, 64, n + 1, support_seed=64)
    b = X.integer_vector(letter, 65, n + 1, support_seed=64)
    v = X.integer_vector(letter, 66, n + 1, axis_only=True)
    v[n // 2] = 7
    da, db, dv = _dev(a), _dev(b), _dev(v)
    for oa, ob in ((1, 0), (0, 1), (1, 1)):
        sums = X.integer_sums(letter, a[oa:oa + n], b[ob:ob + n])
        X.assert_sums_exact(letter, sums)
        assert _dot(gpu, letter, n, da[oa:], db[ob:]) == sums["dot"], f"{letter}dot offsets {oa}, {ob}"
    sums = X.integer_sums(letter, a[1:])
    assert capi.nrm2[letter](gpu, n, _p(da[1:])) == float(X.rounded_sqrt(letter, sums["nrm2sq"]))
    vs = X.integer_sums(letter, v[1:])
    X.assert_sums_exact(letter, vs)
    assert capi.asum[letter](gpu, n, _p(dv[1:])) == vs["asum"]
    assert capi.amax[letter](gpu, n, _p(dv[1:])) == 7


def _sentinel(letter):
    return -12345.0 if letter in "SD" else complex(-12345.0, 54321.0)


def _multivector(letter, seed, n, count, pitch, maker=_rand):
    """[count, pitch] array whose first n columns hold vectors and whose gaps hold the sentinel."""
    a = maker(letter, seed, count * pitch).reshape(count, pitch)
    a[:, n:] = _sentinel(letter)
    return a


def _assert_wide_multivector(letter, pitch, *tensors):
    assert pitch % WIDE[letter] == 0
    _assert_aligned(*tensors)


def _check_multivector_maps(gpu, letter, n, count, pitch, case, ops=("axpby", "axpby_beta0", "axy", "axypbz"), wide=False):
    """maxpby / maxy / maxypbz on [count, pitch]: every vector against both references (evaluated on the flat buffer: the operations
    are element-wise), every gap still the sentinel."""
    import torch
    host = {k: _multivector(letter, s, n, count, pitch) for k, s in (("x", 71), ("y", 72), ("z", 73))}
    dev = {k: _dev(v) for k, v in host.items()}
    if wide:
        _assert_wide_multivector(letter, pitch, *dev.values())
    flat = {k: v.reshape(-1) for k, v in host.items()}
    inside = np.zeros((count, pitch), bool)
    inside[:, :n] = True
    inside = inside.reshape(-1)
    for name, op, use_y, use_beta, use_z in MAP_CASES:
        if name not in ops:
            continue
        beta = BETA[letter] if use_beta else 0.0
        out = torch.full((count * pitch,), _sentinel(letter), dtype=dev["x"].dtype, device="cuda:0")
        if wide:
            _assert_aligned(out)
        _launch(gpu, op, letter, out, n, ALPHA[letter], dev["x"], dev["y"] if use_y else None, beta, dev["z"] if use_z else None,
                count=count, pitch=pitch)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[~inside] == _sentinel(letter)), f"{case} {letter}m{name}: a gap between vectors was written"
        _check_both(f"{case} {letter}m{name}", op, letter, got[inside], ALPHA[letter], flat["x"][inside],
                    flat["y"][inside] if use_y else None, beta, flat["z"][inside] if use_z else None)


def _check_multivector_reductions(gpu, letter, n, count, pitch, case, wide=False):
    """mdot / mnrm2 / masum / mamax on [count, pitch] integer vectors (gaps: the sentinel, which would spoil any sum that read
    it): every vector's result equals the host's integer."""
    from spgpu_amd import capi
    gauss = functools.partial(X.integer_vector, density=0.03)
    a = _multivector(letter, 81, n, count, pitch, lambda L, s, m: gauss(L, s, m, support_seed=81))
    b = _multivector(letter, 82, n, count, pitch, lambda L, s, m: gauss(L, s, m, support_seed=81))
    v = _multivector(letter, 83, n, count, pitch, lambda L, s, m: gauss(L, s, m, axis_only=True))
    peak = np.arange(count) * 7 % n
    v[np.arange(count), peak] = 5 + np.arange(count) % 3            # a maximum per vector, not the same everywhere
    want = [X.integer_sums(letter, a[j, :n], b[j, :n]) for j in range(count)]
    want_v = [X.integer_sums(letter, v[j, :n]) for j in range(count)]
    for s in want + want_v:
        X.assert_sums_exact(letter, s)
    if count > REDUCE_MAX_BLOCKS:      # a second pass that read the first pass's vectors again would show
        assert any(want[j]["nrm2sq"] != want[j - REDUCE_MAX_BLOCKS]["nrm2sq"] for j in range(REDUCE_MAX_BLOCKS, count))
        assert any(want_v[j]["asum"] != want_v[j - REDUCE_MAX_BLOCKS]["asum"] for j in range(REDUCE_MAX_BLOCKS, count))
    da, db, dv = _dev(a), _dev(b), _dev(v)
    if wide:
        _assert_wide_multivector(letter, pitch, da, db, dv)
    real = X.REAL_OF[letter]
    dot = np.full(count, np.nan, X.DTYPE_OF[letter])
    capi.mdot[letter](gpu, _hp(dot), n, _p(da), _p(db), count, pitch)
    nrm, asum, amax = (np.full(count, np.nan, real) for _ in range(3))
    capi.mnrm2[letter](gpu, _hp(nrm), n, _p(da), count, pitch)
    capi.masum[letter](gpu, _hp(asum), n, _p(dv), count, pitch)
    capi.mamax[letter](gpu, _hp(amax), n, _p(dv), count, pitch)
    for j in range(count):
        assert (dot[j].real, dot[j].imag) == want[j]["dot"], f"{case} {letter}mdot vector {j}"
        assert nrm[j] == X.rounded_sqrt(letter, want[j]["nrm2sq"]), f"{case} {letter}mnrm2 vector {j}"
        assert asum[j] == want_v[j]["asum"], f"{case} {letter}masum vector {j}"
        assert amax[j] == want_v[j]["amax"] == 5 + j % 3, f"{case} {letter}mamax vector {j}"


@pytest.mark.parametrize("letter,n,pitch", [("S", 997, 1001), ("D", 997, 1001), ("C", 1499, 1501), ("Z", 997, 1001)])
def test_multivector_narrow_path(gpu, letter, n, pitch):
    """pitch % WIDE != 0: vectors 1, 2, ... start off a 16-byte boundary, so the whole call runs VEC = 1 (Z: always)."""
    assert letter == "Z" or pitch % WIDE[letter] != 0
    _check_multivector_maps(gpu, letter, n, 5, pitch, "odd pitch")
    _check_multivector_reductions(gpu, letter, n, 5, pitch, "odd pitch")


@pytest.mark.parametrize("letter", "SDCZ")
def test_multivector_wide_path(gpu, letter):
    """count > 1 with pitch % WIDE == 0 and aligned bases: the wide kernels with grid.y = vector, every type, both coefficients of
    maxpby / maxypbz non-zero (and maxpby with beta == 0, maxy), and the four multivector reductions.  Several blocks per vector, a
    ragged last tile and a tail.  (Z: WIDE = 1, the VEC = 1 kernels again.)"""
    n = 2 * TILE * WIDE[letter] + 13
    pitch = (n // 4 + 2) * 4
    _check_multivector_maps(gpu, letter, n, 3, pitch, "wide pitch", wide=True)
    _check_multivector_reductions(gpu, letter, n, 3, pitch, "wide pitch", wide=True)


# ==== 4. the caps that depend on the number of vectors ============================================================================

def test_map_cap_per_vector_count_8192(gpu):
    """count = 8 192: cap = 16 384 / 8 192 = 2 blocks per vector; n = 2 051 packs needs 3, so block 0 of every vector loops.
    Wide (pitch % 4 == 0), 269 MB per operand: the non-temporal multivector kernels."""
    letter, count = "S", 8192
    n = 2 * TILE * WIDE[letter] + 9
    pitch = n + 3
    assert pitch % WIDE[letter] == 0 and -(-(-(-n // WIDE[letter])) // TILE) > MAP_MAX_BLOCKS // count == 2
    assert count * pitch * SIZEOF[letter] < 512 << 20
    _check_multivector_maps(gpu, letter, n, count, pitch, "count 8192", ops=("axpby", "axy", "axypbz"), wide=True)


def test_map_cap_per_vector_count_above_16384(gpu):
    """count = 16 400 > kL1MaxBlocks: cap = 1 block per vector.  Odd pitch: VEC = 1, n = 2 100 needs 3 blocks, so the one block
    loops; axpby streams 275 MB even without y: axpbyKernel<float, 1, ., NT>, the one non-temporal VEC = 1 form the launchers can
    pick (mapKernel goes non-temporal only when wide)."""
    letter, count, n, pitch = "S", 16400, 2100, 2101
    assert count > MAP_MAX_BLOCKS and -(-n // TILE) > 1 and 2 * n * count * SIZEOF[letter] >= NT_BYTES
    _check_multivector_maps(gpu, letter, n, count, pitch, "count 16400")


@pytest.mark.parametrize("letter", "SDCZ")
def test_reduction_cap_per_vector_count_600(gpu, letter):
    """count = 600: 1 024 / 600 = 1 block per vector, n > 2 048 * WIDE elements, so that block makes three trips."""
    n = 2 * TILE * WIDE[letter] + 13
    pitch = n + WIDE[letter] - n % WIDE[letter] if n % WIDE[letter] else n + WIDE[letter]
    assert pitch % WIDE[letter] == 0 and REDUCE_MAX_BLOCKS // 600 == 1
    _check_multivector_reductions(gpu, letter, n, 600, pitch, "count 600", wide=True)


@pytest.mark.parametrize("count", [1030, 1025])
@pytest.mark.parametrize("letter", "SDCZ")
def test_reduction_second_pass(gpu, letter, count):
    """More than 1 024 vectors: a second pass over vectors 1 024 ... with a0 = a + 1 024 * pitch and its own grid (1030: 6 vectors,
    whose cap is 1 024 / 6 = 170 blocks each; n = 3 000 at VEC = 1 needs 3, so 3 blocks per vector run, against 1 in the first
    pass).  The pitch is odd, so both passes of 1030 run VEC = 1.  first * pitch * sizeof is a multiple of 16 whatever the pitch,
    so a0 cannot be aligned differently from a; what the second pass does decide anew is `vectors == 1`: with 1025 vectors it
    holds one vector, which goes wide although the pitch is odd."""
    n, pitch = 3000, 3001
    _check_multivector_reductions(gpu, letter, n, count, pitch, f"count {count}")


# ==== 5. gath / scat / setscal past one sweep of the grid =========================================================================

SPARSE_SWEEP = 4 * MAP_MAX_BLOCKS * THREADS      # level1.hip: sparseGrid() caps the grid at 4 * kL1MaxBlocks blocks of kL1Threads
SPARSE_NNZ = SPARSE_SWEEP + RAGGED
SPARSE_LEN = SPARSE_NNZ + 4099


@functools.lru_cache(maxsize=1)
def _permutation_prefix():
    return np.random.default_rng(91).permutation(SPARSE_LEN)[:SPARSE_NNZ].astype(np.int32)


def _sparse_values(letter, seed, n):
    if letter == "I":
        return np.random.default_rng(seed).integers(-50, 50, n).astype(np.int32)
    return _rand(letter, seed, n)


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("letter", "ISDCZ")
def test_sparse_kernels_past_one_sweep(gpu, letter, base):
    """xNnz = 4 * 16 384 * 256 + 1 029: lanes 0 ... 1 028 of the grid take a second entry.  Distinct indices (scatter is race-free),
    every 1 000th below the base (skipped).  setscal over a range of the same length with first > baseIndex."""
    import torch
    from spgpu_amd import capi
    m, n = SPARSE_NNZ, SPARSE_LEN
    idx = _permutation_prefix() + base
    idx[::1000] = base - 1
    idx[-1] = base - 1                                   # the last lane of the second sweep skips too
    used = idx >= base
    pos = (idx[used] - base).astype(np.int64)
    y, vals = _sparse_values(letter, 92, n), _sparse_values(letter, 93, m)
    beta = 3 if letter == "I" else BETA[letter]
    dy, dvals, didx = _dev(y), _dev(vals), _dev(idx)
    for b in (beta, 0):
        dyy = dy.clone()
        capi.scat[letter](gpu, _p(dyy), m, _p(dvals), _p(didx), base, _sc(letter, b))
        torch.cuda.synchronize()
        got = dyy.cpu().numpy()
        _assert_same_bits(got, O.scat(letter, y, vals, idx, base, b), f"{letter}scat base {base} beta {b}")
        if letter != "I":
            X.assert_level1("scat", letter, got[pos], 1.0, vals[used], y[pos], b, case=f"{letter}scat beta {b}", workers=WORKERS)
        untouched = np.ones(n, bool)
        untouched[pos] = False
        _assert_same_bits(got[untouched], y[untouched], f"{letter}scat: elements no index names")
        del dyy
    g_in = _sparse_values(letter, 94, m)
    dg = _dev(g_in)
    capi.gath[letter](gpu, _p(dg), m, _p(didx), base, _p(dy))
    torch.cuda.synchronize()
    got = dg.cpu().numpy()
    _assert_same_bits(got, O.gath(letter, g_in, idx, base, y), f"{letter}gath base {base}")
    _assert_same_bits(got[used], y[pos], f"{letter}gath: the gathered values")
    _assert_same_bits(got[~used], g_in[~used], f"{letter}gath: skipped entries")
    # setscal: elements first - base ... last - base, m of them
    first = base + 5
    last = first + m - 1
    val = 42 if letter == "I" else (2.5 if letter in "SD" else 2.5 + 4j)
    capi.setscal[letter](gpu, first, last, base, _sc(letter, val), _p(dy))
    torch.cuda.synchronize()
    got = dy.cpu().numpy()
    _assert_same_bits(got, O.setscal(letter, y, first, last, base, val), f"{letter}setscal base {base}")
    assert got[4] == y[4] and got[5] == val and got[5 + m - 1] == val and got[5 + m] == y[5 + m]


# ==== 6. edge values and degenerate calls ==========================================================================================

@pytest.mark.parametrize("letter", "CZ")
def test_complex_modulus_special_values(gpu, letter):
    """The three branches of magnitude() (level1.hip): v == 0, beyond `huge`, ordinary -- zeros of both signs, denormals, components whose
    modulus still fits and whose modulus overflows, infinities.  abs bit for bit against the oracle; where the result is finite it is
    within 2 ulp of the long double hypot; where it is infinite the true modulus is beyond the format (or an operand was infinite).

    The 2: after the quotient t = w/v <= 1, magnitude() rounds three times -- fma(t, t, 1), the square root, the product with v --
    half an ulp each, and the quotient's own half ulp reaches the result scaled by t^2/(1 + t^2) <= 1/2 and halved by the root.
    No NaN here for amax: its `m > acc` rule drops a NaN element, as the reference's does, so the result with one is no statement
    about the other elements' order; NaN operands are covered by the not-read tests below."""
    import torch
    from spgpu_amd import capi
    real = X.REAL_OF[letter]
    info = np.finfo(real)
    tiny, sub = info.tiny, info.smallest_subnormal
    fits, over = (2e38, 3e38) if letter == "C" else (1e308, 1.5e308)
    assert fits * 2 ** 0.5 < float(info.max) < over * 2 ** 0.5
    inf = np.inf
    pairs = [(0.0, 0.0), (-0.0, -0.0), (0.0, 3.0), (-0.0, 3.0), (3.0, -0.0), (-3.0, 0.0), (sub, 0.0), (sub, sub), (-sub, 3 * sub),
             (tiny / 4, tiny / 8), (tiny, -tiny), (3.0, 4.0), (-5.0, 12.0), (1.0, 1e-30), (fits, fits), (-fits, fits / 3),
             (over, over), (over, -over), (info.max, info.max), (inf, 1.0), (1.0, -inf), (-inf, inf)]
    x = np.array([complex(a, b) for a, b in pairs]).astype(X.DTYPE_OF[letter])
    x.real, x.imag = [real(a) for a, _ in pairs], [real(b) for _, b in pairs]     # keeps the signs of the zeros
    n = x.size
    dx = _dev(x)
    out = torch.empty_like(dx)
    capi.vabs[letter](gpu, _p(out), n, _sc(letter, 1.0), _p(dx))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _assert_same_bits(got, O.level1_map(letter, "abs", n, 1.0, x), f"{letter}abs")
    assert not got.imag.any()
    exact = np.hypot(x.real.astype(np.longdouble), x.imag.astype(np.longdouble))
    finite = np.isfinite(got.real)
    err = np.abs(got.real[finite].astype(np.longdouble) - exact[finite])
    ulp = np.spacing(np.abs(got.real[finite])).astype(np.longdouble)
    assert np.all(err <= 2 * ulp), f"{letter}abs beyond 2 ulp: {x[finite][err > 2 * ulp]} -> {got.real[finite][err > 2 * ulp]}"
    assert np.all(got.real[~finite] == inf) and np.all(exact[~finite] > info.max)
    assert finite.sum() == n - 6                       # the three overflows and the three with an infinite component
    # amax: the order of comparisons does not matter, so the oracle's value exactly; with and without the infinite elements
    for m in (n, n - 3, n - 6):
        assert capi.amax[letter](gpu, m, _p(dx)) == O.amax(letter, x[:m]) == got.real[:m].max()
    assert capi.asum[letter](gpu, n, _p(dx)) == inf
    # asum of the finite part: a sum of n non-negative terms in any order is within (n - 1) * eps of the exact sum of those terms
    m = n - 8                                            # without the elements of the order of the format's maximum
    want = got.real[:m].astype(np.longdouble).sum()
    assert abs(np.longdouble(capi.asum[letter](gpu, m, _p(dx))) - want) <= (m - 1) * X.EPS[letter] * want
    # a general alpha, (alpha.re * m, alpha.im * m), on the zeros and the ordinary elements (a product that lands among the denormals
    # is not within a RELATIVE bound): bit for bit and within the long double bound
    plain = np.array([i for i, (a, b) in enumerate(pairs[:n - 8]) if all(c == 0 or abs(c) >= 1e-30 for c in (a, b))])
    xs = np.ascontiguousarray(x[plain])
    dxs = _dev(xs)
    capi.vabs[letter](gpu, _p(out), xs.size, _sc(letter, ALPHA[letter]), _p(dxs))
    torch.cuda.synchronize()
    _check_both(f"{letter}abs alpha", "abs", letter, out.cpu().numpy()[:xs.size], ALPHA[letter], xs)


@pytest.mark.parametrize("n", [4099, 70_001])
@pytest.mark.parametrize("letter", "SDCZ")
def test_operands_not_read_when_their_coefficient_is_zero(gpu, letter, n):
    """The operand that the reference's dispatch never touches is full of NaN: the result has none and is the oracle's.
    axpby beta == 0 (y), axypbz alpha == 0 (x and y; routed to scal(beta, z)), axypbz beta == 0 (z; routed to axy), scat beta == 0
    (the target vector), and the multivector forms."""
    import torch
    from spgpu_amd import capi
    x, y, z = (_rand(letter, s, n) for s in (101, 102, 103))
    dx, dy, dz = _dev(x), _dev(y), _dev(z)
    nan = torch.full_like(dx, float("nan"))
    nan_h = np.full(n, np.nan, X.DTYPE_OF[letter])
    cases = [("axpby beta=0", "axpby", ALPHA[letter], 0.0, (dx, nan, None), (x, nan_h, None)),
             ("axypbz alpha=0", "axypbz", 0.0, BETA[letter], (nan, nan, dz), (nan_h, nan_h, z)),
             ("axypbz beta=0", "axypbz", ALPHA[letter], 0.0, (dx, dy, nan), (x, y, nan_h))]
    count = 3
    pitch = -(-n // 4) * 4 + 4
    for name, op, alpha, beta, dev, host in cases:
        out = torch.full_like(dx, float("nan"))
        _launch(gpu, op, letter, out, n, alpha, dev[0], dev[1], beta, dev[2])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), f"{letter}{name}: NaN reached the result"
        _check_both(f"{letter}{name}", op, letter, got, alpha, host[0], host[1], beta, host[2])
        # the multivector form: count vectors at a pitch, the NaN operand NaN everywhere
        wide = {k: (None if h is None else np.full((count, pitch), np.nan, X.DTYPE_OF[letter])) for k, h in zip("xyz", host)}
        for k, h in zip("xyz", host):
            if h is not None and not np.isnan(h).all():
                wide[k][:, :n] = _rand(letter, 110 + "xyz".index(k), count * n).reshape(count, n)
        dw = {k: _dev(v) for k, v in wide.items()}
        outm = torch.full((count * pitch,), _sentinel(letter), dtype=dx.dtype, device="cuda:0")
        _launch(gpu, op, letter, outm, n, alpha, dw["x"], dw["y"], beta, dw["z"], count=count, pitch=pitch)
        torch.cuda.synchronize()
        gm = outm.cpu().numpy().reshape(count, pitch)
        assert not np.isnan(gm).any() and np.all(gm[:, n:] == _sentinel(letter)), f"{letter}m{name}"
        for j in range(count):
            row = [None if wide[k] is None else wide[k][j, :n] for k in "xyz"]
            _check_both(f"{letter}m{name} vector {j}", op, letter, gm[j, :n], alpha, row[0], row[1], beta, row[2])
    # scat with beta == 0 into a vector of NaN: the named elements become the values, the others stay NaN
    m = n // 2
    idx = (np.random.default_rng(104).permutation(n)[:m] + 1).astype(np.int32)
    vals = _rand(letter, 105, m)
    dv, dvals, didx = torch.full_like(dx, float("nan")), _dev(vals), _dev(idx)
    capi.scat[letter](gpu, _p(dv), m, _p(dvals), _p(didx), 1, _sc(letter, 0.0))
    torch.cuda.synchronize()
    got = dv.cpu().numpy()
    _assert_same_bits(got[idx - 1], vals, f"{letter}scat beta=0")
    _assert_same_bits(got, O.scat(letter, nan_h, vals, idx, 1, 0.0), f"{letter}scat beta=0 against the oracle")
    assert np.isnan(got).sum() == n - m


@pytest.mark.parametrize("letter", "SDCZ")
def test_degenerate_sizes(gpu, letter):
    """n == 0, n < 0 and count == 0: outputs keep their sentinel, reductions return 0, the multivector reductions write `count` zeros
    (none when count == 0)."""
    import torch
    from spgpu_amd import capi
    size, pitch = 64, 16
    x, y, z = (_dev(_rand(letter, s, size)) for s in (121, 122, 123))
    idx = _dev(np.arange(size, dtype=np.int32))
    real = X.REAL_OF[letter]
    for n, count in ((0, None), (-1, None), (-7, None), (0, 3), (-1, 3), (8, 0), (0, 0)):
        out = torch.full((size,), _sentinel(letter), dtype=x.dtype, device="cuda:0")
        for name, op, use_y, use_beta, use_z in MAP_CASES:
            if count is not None and op in ("scal", "abs"):
                continue
            _launch(gpu, op, letter, out, n, ALPHA[letter], x, y, BETA[letter] if use_beta else 0.0, z, count=count, pitch=pitch)
        for alpha, beta in ((0.0, BETA[letter]), (ALPHA[letter], 0.0)):
            _launch(gpu, "axypbz", letter, out, n, alpha, x, y, beta, z, count=count, pitch=pitch)
        if count is None:
            capi.scat[letter](gpu, _p(out), n, _p(x), _p(idx), 0, _sc(letter, BETA[letter]))
            capi.gath[letter](gpu, _p(out), n, _p(idx), 0, _p(x))
            capi.setscal[letter](gpu, 5, 5 + n - 1, 0, _sc(letter, 1.0), _p(out))      # last < first
        torch.cuda.synchronize()
        assert torch.all(out == _sentinel(letter)), f"{letter}: an output was written with n={n}, count={count}"
        if count is None:
            assert _dot(gpu, letter, n, x, y) == (0, 0)
            assert capi.nrm2[letter](gpu, n, _p(x)) == 0 and capi.asum[letter](gpu, n, _p(x)) == 0 and capi.amax[letter](gpu, n, _p(x)) == 0
        else:
            dot = np.full(4, 9, X.DTYPE_OF[letter])
            capi.mdot[letter](gpu, _hp(dot), n, _p(x), _p(y), count, pitch)
            assert np.all(dot[:count] == 0) and np.all(dot[count:] == 9), f"{letter}mdot n={n} count={count}: {dot}"
            for fn in (capi.mnrm2, capi.masum, capi.mamax):
                r = np.full(4, 9, real)
                fn[letter](gpu, _hp(r), n, _p(x), count, pitch)
                assert np.all(r[:count] == 0) and np.all(r[count:] == 9), f"{letter} m-reduction n={n} count={count}: {r}"
    if letter in "SD":
        res = torch.full((2,), 9.0, dtype=x.dtype, device="cuda:0")
        for n in (0, -3):
            capi.dot_device[letter](gpu, _p(res[0:]), n, _p(x), _p(y))
            capi.nrm2_device[letter](gpu, _p(res[1:]), n, _p(x))
            torch.cuda.synchronize()
            assert res.cpu().numpy().tolist() == [0.0, 0.0]
            res.fill_(9.0)
