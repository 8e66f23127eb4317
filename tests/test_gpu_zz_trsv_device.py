"""GPU: the sparse triangular solve x = T^-1 * b on CSR arrays (include/spgpu/ext/trsv_device.h).

Every device output -- rowOrder, levelPtr, x -- and the scratch lie between 64 guard bytes and are poisoned as a whole with one byte
pattern; levelPtrHost lies between sentinels.  The Plan's arrays must equal formats.csr_trsv_plan BYTE FOR BYTE, the level arrays
must be untouched behind their first levelsCount + 1 ints, and x must equal numpy's restatement of the contract
(formats.csr_trsv) BYTE FOR BYTE through the public call and through each of the two solves behind it (one launch per level; runs
of narrow levels chained in one workgroup), on the whole grid and on a capped one, out of place and in place (_solve).  The solves
run after the scratch has been overwritten.  The matrices are the smallest at which each branch of the Plan and of the two solves
can go wrong."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import trsv_cases as T
from test_gpu_csr_device import _p
from test_gpu_to_csr_device import PATTERN, _Guarded
from test_spgemm_restated import inexact_pair
from trsv_cases import LOWER, STORED, UNIT, UPPER

pytestmark = pytest.mark.gpu
SENTINEL = -7


def _device(arrays):
    from spgpu_amd import formats
    some = lambda a: a if a.size else np.zeros(1, a.dtype)
    return tuple(formats.to_device(some(np.ascontiguousarray(a))) for a in arrays)


class _Plan:
    pass


def _plan(gpu, d_ptr, d_cols, n, base, side, diag):
    """spgpuCsrTrsvPlanDevice between guards; the guards and the sentinels are checked here."""
    import torch
    from spgpu_amd import capi
    p = _Plan()
    p.work = _Guarded(capi.spgpuCsrTrsvWorkBytes(n), 192)                   # 256-byte aligned
    p.order, p.level_ptr = _Guarded(n * 4), _Guarded((n + 1) * 4)
    p.host = np.full(n + 1 + 8, SENTINEL, np.int32)                         # [4 sentinels | n + 1 ints | 4 sentinels]
    p.host_at = p.host[4:].ctypes.data_as(C.POINTER(C.c_int))
    levels = C.c_int(-7)
    torch.cuda.synchronize()
    p.status = capi.spgpuCsrTrsvPlanDevice(gpu, C.byref(levels), p.order.ptr(), p.level_ptr.ptr(), p.host_at, n, _p(d_ptr), _p(d_cols), base,
                                           side, diag, p.work.ptr())
    torch.cuda.synchronize()
    p.levels = levels.value
    assert p.order.guards_intact() and p.level_ptr.guards_intact() and p.work.guards_intact()
    assert (p.host[:4] == SENTINEL).all() and (p.host[4 + n + 1:] == SENTINEL).all()
    return p


def _solve(gpu, mat, b, letter, base, side, diag, caps=(0, 1)):
    """The Plan and every solve on host CSR arrays given in `base`, everything against formats.  Returns (levels, x) restated."""
    import torch
    from spgpu_amd import capi, formats
    dtype = np.dtype(X.DTYPE_OF[letter])
    ptr, cols, vals = mat
    assert vals.dtype == dtype and b.dtype == dtype
    n = ptr.size - 1
    case = (letter, n, base, side, diag)
    w_levels, w_order, w_level_ptr = formats.csr_trsv_plan(ptr, cols, base, side, diag)
    want = formats.csr_trsv(ptr, cols, vals, b, base, side, diag)
    d_ptr, d_cols, d_vals, d_b = _device((ptr, cols, vals, b))
    p = _plan(gpu, d_ptr, d_cols, n, base, side, diag)
    assert p.status == capi.SPGPU_SUCCESS and p.levels == w_levels, (case, p.status, p.levels, w_levels)
    assert p.order.numpy(np.int32).tobytes() == w_order.tobytes(), case
    got_ptr = p.level_ptr.numpy(np.int32)
    assert got_ptr[:w_levels + 1].tobytes() == w_level_ptr.tobytes(), case
    assert (got_ptr[w_levels + 1:].view(np.uint8) == PATTERN).all(), case                       # untouched beyond
    assert p.host[4:4 + w_levels + 1].tobytes() == w_level_ptr.tobytes() and (p.host[4 + w_levels + 1:] == SENTINEL).all(), case
    p.work.buf[p.work.first:p.work.first + p.work.nbytes].fill_(0xFF)                           # the solve never reads the scratch
    code, size = capi.TYPE_CODE[letter], dtype.itemsize
    runs = [(None, 0)] + [(solve, cap) for solve in (capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED) for cap in caps]
    for in_place in (False, True):
        for solve, cap in runs:
            x = _Guarded(n * size)
            if in_place:
                x.buf[x.first:x.first + n * size].copy_(formats.to_device(np.ascontiguousarray(b[:n]).view(np.uint8)))
            torch.cuda.synchronize()
            args = (gpu, x.ptr(), x.ptr() if in_place else _p(d_b), n, p.levels, p.order.ptr(), p.level_ptr.ptr(), p.host_at, _p(d_ptr),
                    _p(d_cols), _p(d_vals), base, side, diag, code)
            st = capi.spgpuCsrTrsvDevice(*args) if solve is None else capi.spgpuCsrTrsvDeviceWith(*args, solve, cap)
            assert st == capi.SPGPU_SUCCESS, (case, solve, cap, in_place)
            torch.cuda.synchronize()
            assert x.guards_intact() and p.order.guards_intact() and p.level_ptr.guards_intact() and p.work.guards_intact(), (case, solve, cap)
            assert x.numpy(np.uint8).tobytes() == want.tobytes(), (case, solve, cap, in_place)
    for d, h in zip((d_ptr, d_cols, d_vals, d_b), (ptr, cols, vals, b)):                         # the inputs are as they were
        assert d.cpu().numpy().reshape(-1)[:h.size].tobytes() == h.tobytes(), case
    assert p.order.numpy(np.int32).tobytes() == w_order.tobytes(), case
    return w_levels, want


# ---- 1. every type x both bases x both sides x both kinds of diagonal -------------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("side", [LOWER, UPPER])
@pytest.mark.parametrize("diag", [STORED, UNIT])
def test_random_systems_give_numpys_bytes(gpu, letter, base, side, diag):
    """70 rows in shuffled storage order with entries on both sides; NaN on the unused side and, under UNIT, on the diagonal; under
    UNIT every third row stores nothing."""
    rng = np.random.default_rng(100 + ord(letter) + 7 * side + 3 * diag)
    mat, b = T.random_system(rng, 70, letter, base, side, diag)
    assert np.isnan(mat[2]).any() and (diag == STORED or (np.diff(mat[0]) == 0).sum() >= 23)
    levels, x = _solve(gpu, mat, b, letter, base, side, diag)
    assert levels > 3 and not np.isnan(x).any()


# ---- 2. one level: the grid-stride loop of the plain solve and the single chained level --------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_one_level_around_the_wavefront_and_the_workgroup(gpu, n):
    rng = np.random.default_rng(n)
    for letter, side, diag in (("S", LOWER, STORED), ("Z", UPPER, STORED), ("D", LOWER, UNIT)):
        mat, b, _ = T.from_levels(rng, [n], letter, 0, side, diag)
        levels, _ = _solve(gpu, mat, b, letter, 0, side, diag, caps=(1, 2))
        assert levels == 1


# ---- 3. chains: as many levels as rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 300])
@pytest.mark.parametrize("side", [LOWER, UPPER])
def test_a_bidiagonal_chain(gpu, n, side):
    rng = np.random.default_rng(20 + n)
    for letter in "DC":
        mat = T.bidiagonal(n, letter, 1, side, rng)
        levels, _ = _solve(gpu, mat, T.values(rng, n, letter), letter, 1, side, STORED)
        assert levels == n


# ---- 4. levels around the chain width, alone and in sequences that start and end wide and narrow -----------------------------
def _sequences():
    from spgpu_amd import capi
    w = capi.TRSV_CHAIN_WIDTH
    return {"w-1 alone": [w - 1], "w alone": [w], "w+1 alone": [w + 1], "3w alone": [3 * w],
            "wide narrow wide narrow": [3 * w, 5, w + 1, w], "narrow wide narrow wide": [w - 1, 3 * w, w, w + 1],
            "narrow runs around wide levels": [2, 3, w + 1, 1, w - 1, 3 * w, 7, 1], "wide wide narrow narrow wide": [w + 1, w + 1, w, w - 1, w + 1]}


@pytest.mark.parametrize("name", ["w-1 alone", "w alone", "w+1 alone", "3w alone", "wide narrow wide narrow", "narrow wide narrow wide",
                                  "narrow runs around wide levels", "wide wide narrow narrow wide"])
@pytest.mark.parametrize("side", [LOWER, UPPER])
def test_levels_around_the_chain_width(gpu, name, side):
    widths = _sequences()[name]
    rng = np.random.default_rng(40 + len(name) + side)
    letter = "D" if side == LOWER else "C"
    mat, b, level = T.from_levels(rng, widths, letter, 0, side)
    levels, _ = _solve(gpu, mat, b, letter, 0, side, STORED)
    assert levels == len(widths)
    from spgpu_amd import formats
    _, order, level_ptr = formats.csr_trsv_plan(mat[0], mat[1], 0, side, STORED)
    assert np.diff(level_ptr).tolist() == widths and np.array_equal(level[order], np.repeat(np.arange(len(widths)), widths))


# ---- 5. the Plan's own thresholds: the sweeps over more than one scan tile and the rows one workgroup finishes -----------------
@pytest.mark.parametrize("widths", [[1, 1023], [1, 1024], [1025, 1], [1024, 1025, 3], [2049, 1024, 1030, 2]])
def test_the_plan_around_its_finishing_workgroup_and_its_scan_tile(gpu, widths):
    rng = np.random.default_rng(sum(widths))
    mat, b, _ = T.from_levels(rng, widths, "S", 1, UPPER if len(widths) == 3 else LOWER)
    levels, _ = _solve(gpu, mat, b, "S", 1, UPPER if len(widths) == 3 else LOWER, STORED, caps=(0, 3))
    assert levels == len(widths)


# ---- 6. stencils ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,dims", [(16, 2), (8, 3)])
@pytest.mark.parametrize("side", [LOWER, UPPER])
def test_a_stencil_matrix(gpu, g, dims, side):
    rng = np.random.default_rng(60 + g)
    mat = T.stencil(g, dims, "D", 0, rng)
    levels, _ = _solve(gpu, mat, T.values(rng, g ** dims, "D"), "D", 0, side, STORED)
    assert levels == dims * (g - 1) + 1


# ---- 7. details of the contract --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter,big", [("S", 1e8), ("D", 1e16)])
def test_the_subtractions_follow_the_storage_order(gpu, letter, big):
    dtype = X.DTYPE_OF[letter]
    b = np.array([1, big, big], dtype)
    for cols, last in (([0, 1], 0.0), ([1, 0], -1.0)):
        mat = T.from_rows([([], []), ([], []), (cols, [1.0, 1.0])], letter)
        _, x = _solve(gpu, mat, b, letter, 0, LOWER, UNIT)
        assert x.tolist() == [1.0, big, last]


@pytest.mark.parametrize("letter", "SD")
def test_no_fused_multiply_add_joins_the_product_to_the_difference(gpu, letter):
    """64 rows acc = p - (a * x) with p = round(a * x) and a * x inexact: exactly +0 when the product is rounded first, the
    product's rounding error -- not 0 -- from one fused multiply-add."""
    dtype = X.DTYPE_OF[letter]
    rng = np.random.default_rng(500 + ord(letter))
    rows, b = [], []
    for t in range(64):
        a, x, p, error = inexact_pair(rng, dtype)
        assert float(error) != 0
        rows += [([], []), ([2 * t], [a])]
        b += [x, p]
    _, x = _solve(gpu, T.from_rows(rows, letter), np.array(b, dtype), letter, 0, LOWER, UNIT)
    assert np.all(x[1::2] == 0) and not np.signbit(x[1::2]).any()


@pytest.mark.parametrize("letter", "CZ")
def test_no_fused_multiply_add_inside_a_complex_product_or_quotient(gpu, letter):
    """The real part ar*xr - ai*xi with ai*xi = round(ar*xr) is exactly 0 only if neither product is fused into the difference; the
    quotient of two real numbers held as complex ones is round(round(n*d) / round(d*d)), which no fused form gives."""
    dtype, real = X.DTYPE_OF[letter], X.REAL_OF[letter]
    rng = np.random.default_rng(600 + ord(letter))
    rows, b = [], []
    for t in range(32):
        s, u, p, _ = inexact_pair(rng, real)
        rows += [([], []), ([2 * t], [complex(s, p)])]
        b += [complex(u, 1), complex(3, 0)]
    _, x = _solve(gpu, T.from_rows(rows, letter), np.array(b, dtype), letter, 0, LOWER, UNIT)
    assert np.all(x[1::2].real == 3)
    pairs = [inexact_pair(rng, real)[:2] for _ in range(32)]
    mat = T.from_rows([([t], [complex(d, 0)]) for t, (_, d) in enumerate(pairs)], letter)
    _, x = _solve(gpu, mat, np.array([complex(n, 0) for n, _ in pairs], dtype), letter, 0, UPPER, STORED)
    assert x.real.tolist() == [real(real(n * d) / real(d * d)) for n, d in pairs] and np.all(x.imag == 0)


def test_the_fp32_division_is_correctly_rounded(gpu):
    n, d = T.division_operands(np.random.default_rng(4))
    mat = T.from_rows([([t], [d[t]]) for t in range(n.size)], "S")
    _, x = _solve(gpu, mat, n, "S", 0, LOWER, STORED)
    assert np.all(x == n / d) and np.all(x != n * (np.float32(1) / d))


@pytest.mark.parametrize("letter", "SD")
def test_a_lone_negative_zero_keeps_its_bits_under_unit(gpu, letter):
    dtype = X.DTYPE_OF[letter]
    mat = T.from_rows([([], []), ([1], [np.nan]), ([], [])], letter)
    b = np.array([-0.0, -0.0, 0.0], dtype)
    for side in (LOWER, UPPER):
        _, x = _solve(gpu, mat, b, letter, 0, side, UNIT)
        assert x.tobytes() == b.tobytes()


# ---- 8. the refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("side", [LOWER, UPPER])
@pytest.mark.parametrize("kind", ["column below the base", "column at base + rows", "missing diagonal", "diagonal stored twice"])
def test_a_bad_matrix_is_refused(gpu, kind, side, base):
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(70)
    (ptr, cols, vals), b = T.random_system(rng, 70, "D", base, side, STORED, poison=False)
    cols = cols.copy()
    lengths = np.diff(ptr)
    k = int(np.argmax(lengths))
    first = ptr[k] - base
    assert lengths[k] >= 3
    at_diagonal = first + int(np.flatnonzero(cols[first:first + lengths[k]] - base == k)[0])
    other = first if at_diagonal != first else first + 1
    if kind == "column below the base":
        cols[other] = base - 1
    elif kind == "column at base + rows":
        cols[other] = base + 70
    elif kind == "missing diagonal":
        cols[at_diagonal] = cols[other]
    else:
        cols[other] = k + base
    diags = (STORED, UNIT) if kind.startswith("column") else (STORED,)
    d_ptr, d_cols = _device((ptr, cols))
    for diag in diags:
        with pytest.raises(ValueError):
            formats.csr_trsv_plan(ptr, cols, base, side, diag)
        p = _plan(gpu, d_ptr, d_cols, 70, base, side, diag)                                       # the guards are checked in _plan
        assert p.status == capi.SPGPU_UNSUPPORTED and p.levels == 0, (kind, side, diag)
    good, b = T.random_system(rng, 70, "D", base, side, STORED)                                  # the handle works on
    _solve(gpu, good, b, "D", base, side, STORED, caps=(0,))


def test_degenerate_shapes(gpu):
    import torch
    from spgpu_amd import capi
    order, level_ptr, x = _Guarded(64), _Guarded(64), _Guarded(64)
    host = np.full(8, SENTINEL, np.int32)
    levels = C.c_int(-7)
    at = host.ctypes.data_as(C.POINTER(C.c_int))
    for rows in (0, -2):
        assert capi.spgpuCsrTrsvPlanDevice(gpu, C.byref(levels), order.ptr(), level_ptr.ptr(), at, rows, None, None, 0, LOWER, STORED,
                                           None) == capi.SPGPU_SUCCESS and levels.value == 0
        levels.value = -7
    for rows, count in ((0, 3), (5, 0), (5, -1)):
        assert capi.spgpuCsrTrsvDevice(gpu, x.ptr(), x.ptr(), rows, count, order.ptr(), level_ptr.ptr(), at, None, None, None, 0, LOWER, STORED,
                                       capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    assert order.untouched() and level_ptr.untouched() and x.untouched() and (host == SENTINEL).all()
    for letter in "SDCZ":                                                    # 1 x 1, and a matrix without a single entry
        dtype = X.DTYPE_OF[letter]
        for base in (0, 1):
            _solve(gpu, T.from_rows([([0], [1.5])], letter, base), np.array([3.0], dtype), letter, base, UPPER, STORED)
            _solve(gpu, T.from_rows([([], [])] * 9, letter, base), T.values(np.random.default_rng(1), 9, letter), letter, base, LOWER, UNIT)


# ---- 9. determinism ----------------------------------------------------------------------------------------------------
def test_a_repeated_call_gives_the_same_bytes_and_plain_equals_chained(gpu):
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(9)
    (ptr, cols, vals), b = T.random_system(rng, 3000, "D", 0, LOWER, STORED, longest=12, poison=False)
    levels, order, level_ptr = formats.csr_trsv_plan(ptr, cols, 0, LOWER, STORED)
    d_ptr, d_cols, d_vals, d_b, d_order, d_level_ptr = _device((ptr, cols, vals, b, order, level_ptr))
    host = np.ascontiguousarray(level_ptr)
    seen = set()
    for solve in (capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED, capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED, -1):
        x = _Guarded(3000 * 8)
        torch.cuda.synchronize()
        assert capi.spgpuCsrTrsvDeviceWith(gpu, x.ptr(), _p(d_b), 3000, levels, _p(d_order), _p(d_level_ptr), host.ctypes.data_as(C.POINTER(C.c_int)),
                                           _p(d_ptr), _p(d_cols), _p(d_vals), 0, LOWER, STORED, capi.TYPE_DOUBLE, solve, 0) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        seen.add(x.buf.cpu().numpy().tobytes())
    assert len(seen) == 1 and x.numpy(np.float64).tobytes() == formats.csr_trsv(ptr, cols, vals, b).tobytes()
    widths = np.diff(level_ptr)
    assert widths.max() > capi.TRSV_CHAIN_WIDTH and widths.min() <= capi.TRSV_CHAIN_WIDTH       # both kinds of segment ran


# ---- 10. the solve in a captured graph ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", [0, 1])
def test_the_solve_replays_from_a_captured_graph(gpu, solve):
    """spgpuCsrTrsvDevice captured on the handle's stream (it reads levelPtrHost at capture time) and replayed after b and the
    values were overwritten in place: each replay gives the bytes of the restatement on the values of the moment."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(10)
    mat = T.stencil(12, 2, "D", 1, rng)
    ptr, cols, vals = mat
    n = 144
    b = T.values(rng, n, "D")
    levels, order, level_ptr = formats.csr_trsv_plan(ptr, cols, 1, UPPER, STORED)
    d_ptr, d_cols, d_vals, d_b, d_order, d_level_ptr = _device((ptr, cols, vals, b, order, level_ptr))
    host = np.ascontiguousarray(level_ptr)
    d_x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    side_stream = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side_stream.cuda_stream))
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side_stream):
            assert capi.spgpuCsrTrsvDeviceWith(gpu, _p(d_x), _p(d_b), n, levels, _p(d_order), _p(d_level_ptr),
                                               host.ctypes.data_as(C.POINTER(C.c_int)), _p(d_ptr), _p(d_cols), _p(d_vals), 1, UPPER, STORED,
                                               capi.TYPE_DOUBLE, solve, 0) == capi.SPGPU_SUCCESS
        host[:] = 0                                                          # read at capture time, not at replay
        wants = set()
        for _ in range(2):
            new_vals, new_b = T.stencil(12, 2, "D", 1, rng)[2], T.values(rng, n, "D")
            want = formats.csr_trsv(ptr, cols, new_vals, new_b, 1, UPPER, STORED).tobytes()
            wants.add(want)
            d_vals.copy_(formats.to_device(new_vals))
            d_b.copy_(formats.to_device(new_b))
            d_x.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert d_x.cpu().numpy().tobytes() == want
        assert len(wants) == 2
    finally:
        capi.spgpuSetStream(gpu, None)


# ---- 11. end to end: a forward Gauss-Seidel sweep on an assembled Laplacian -----------------------------------------------------
def test_a_forward_gauss_seidel_sweep_on_an_assembled_laplacian(gpu):
    """16 x 16 grid: the 5-point Laplacian listed with the diagonal split in two and assembled on the device; the lower Plan on the
    assembled arrays; x1 = (D + L)^-1 (b - U x0) with b - U x0 formed on the host in small integers (exact), against the dense
    triangular solve.  T = D + L is row-dominant with rho = 2 / 4, so cond <= (1 + rho) / (1 - rho) = 3 (tests/test_trsv_restated.py
    has the derivation); the substitution's backward error is gamma_3 and the dense solver's at most gamma_256."""
    import torch
    from spgpu_amd import capi
    from test_gpu_zz_add_device import _assembled
    n, base = 16, 1
    size = n * n
    cell = np.arange(size)
    gx, gy = cell % n, cell // n
    rng = np.random.default_rng(11)
    rows, cols, vals = [cell, cell], [cell, cell], [np.full(size, 3.0), np.full(size, 1.0)]
    for ok, to in ((gx > 0, cell - 1), (gx < n - 1, cell + 1), (gy > 0, cell - n), (gy < n - 1, cell + n)):
        rows.append(cell[ok]), cols.append(to[ok]), vals.append(np.full(int(ok.sum()), -1.0))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    dense = np.zeros((size, size))
    np.add.at(dense, (rows, cols), vals)
    shuffle = rng.permutation(rows.size)
    a_ptr, a_cols, a_vals, entries = _assembled(gpu, size, rows[shuffle], cols[shuffle], vals[shuffle], base)
    assert entries == int((dense != 0).sum())
    work = torch.empty(capi.spgpuCsrTrsvWorkBytes(size), dtype=torch.uint8, device="cuda:0")
    order, level_ptr = (torch.zeros(k, dtype=torch.int32, device="cuda:0") for k in (size, size + 1))
    host = np.zeros(size + 1, np.int32)
    levels = C.c_int(-1)
    at = host.ctypes.data_as(C.POINTER(C.c_int))
    assert capi.spgpuCsrTrsvPlanDevice(gpu, C.byref(levels), _p(order), _p(level_ptr), at, size, _p(a_ptr), _p(a_cols), base, LOWER, STORED,
                                       _p(work)) == capi.SPGPU_SUCCESS
    assert levels.value == 2 * n - 1 and host[levels.value] == size
    del work
    x0 = (cell % 5 - 2).astype(np.float64)
    b = (cell % 7 + 1).astype(np.float64)
    rhs = b - np.triu(dense, 1) @ x0                                         # small integers: exact
    from spgpu_amd import formats
    d_rhs = formats.to_device(rhs)
    x1 = torch.zeros(size, dtype=torch.float64, device="cuda:0")
    assert capi.spgpuCsrTrsvDevice(gpu, _p(x1), _p(d_rhs), size, levels.value, _p(order), _p(level_ptr), at, _p(a_ptr), _p(a_cols), _p(a_vals),
                                   base, LOWER, STORED, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    got = x1.cpu().numpy()
    want = np.linalg.solve(np.tril(dense), rhs)
    u = np.finfo(np.float64).eps / 2
    gamma = lambda k: k * u / (1 - k * u)
    margin = 3 * (gamma(3) + gamma(size))
    error = np.abs(got - want).max() / np.abs(want).max()
    print(f"Gauss-Seidel sweep: error {error:.3e}, margin {margin:.3e}")
    assert error <= margin
    # and the residual of the sweep's own equation, row by row: (D + L) x1 = rhs
    assert np.abs(np.tril(dense) @ got - rhs).max() <= 3 * gamma(3) * (np.abs(np.tril(dense)) @ np.abs(got)).max()
