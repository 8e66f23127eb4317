"""GPU: the ILU(0) factorisation on CSR arrays (include/spgpu/ext/ilu0_device.h).

Every device output -- rowOrder, levelPtr, diagPos, lu -- and the scratch lie between 64 guard bytes and are poisoned as a whole with
one byte pattern; levelPtrHost lies between sentinels.  The Plan's arrays must equal formats.csr_ilu0_plan BYTE FOR BYTE, the level
arrays must be untouched behind what the header says is written, and lu must equal numpy's restatement of the contract
(formats.csr_ilu0) BYTE FOR BYTE through the public call and through every row shape the rules can choose (one thread per row, the
two groups of lanes), each with one launch per level and with runs of narrow levels chained in one workgroup, on the whole grid and
on a grid of one workgroup, out of place and in place (_factor).  Out of place the matrix keeps its bytes.  The factor calls run
after the scratch has been overwritten.  The matrices are the smallest at which each branch can go wrong."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import ilu0_cases as I
import trsv_cases as T
from test_gpu_csr_device import _p
from test_gpu_to_csr_device import PATTERN, _Guarded
from trsv_cases import LOWER, STORED, UNIT, UPPER

pytestmark = pytest.mark.gpu
SENTINEL = -7


def _device(arrays):
    from spgpu_amd import formats
    some = lambda a: a if a.size else np.zeros(1, a.dtype)
    return tuple(formats.to_device(some(np.ascontiguousarray(a))) for a in arrays)


class _Plan:
    pass


def _plan(gpu, d_ptr, d_cols, n, base):
    """spgpuCsrIlu0PlanDevice between guards; the guards and the sentinels are checked here."""
    import torch
    from spgpu_amd import capi
    p = _Plan()
    p.work = _Guarded(capi.spgpuCsrIlu0WorkBytes(n), 192)                   # 256-byte aligned
    p.order, p.level_ptr, p.diag_pos = _Guarded(n * 4), _Guarded((n + 1) * 4), _Guarded(n * 4)
    p.host = np.full(n + 2 + 8, SENTINEL, np.int32)                         # [4 sentinels | n + 2 ints | 4 sentinels]
    p.host_at = p.host[4:].ctypes.data_as(C.POINTER(C.c_int))
    levels = C.c_int(-7)
    torch.cuda.synchronize()
    p.status = capi.spgpuCsrIlu0PlanDevice(gpu, C.byref(levels), p.order.ptr(), p.level_ptr.ptr(), p.host_at, p.diag_pos.ptr(), n, _p(d_ptr),
                                           _p(d_cols), base, p.work.ptr())
    torch.cuda.synchronize()
    p.levels = levels.value
    assert p.order.guards_intact() and p.level_ptr.guards_intact() and p.diag_pos.guards_intact() and p.work.guards_intact()
    assert (p.host[:4] == SENTINEL).all() and (p.host[4 + n + 2:] == SENTINEL).all()
    return p


def _runs(caps=(0, 1)):
    from spgpu_amd import capi
    return [(None, None, 0)] + [(shape, solve, cap) for shape in capi.ILU0_SHAPES
                                for solve in (capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED) for cap in caps]


def _factor(gpu, mat, letter, base, caps=(0, 1)):
    """The Plan and every factor call on host CSR arrays given in `base`, everything against formats.  Returns (levels, lu) restated."""
    import torch
    from spgpu_amd import capi, formats
    dtype = np.dtype(X.DTYPE_OF[letter])
    ptr, cols, vals = mat
    assert vals.dtype == dtype
    n, nnz = ptr.size - 1, vals.size
    case = (letter, n, base)
    w_levels, w_order, w_level_ptr, w_diag = formats.csr_ilu0_plan(ptr, cols, base)
    with np.errstate(all="ignore"):
        want = formats.csr_ilu0(ptr, cols, vals, base)
    d_ptr, d_cols, d_vals = _device((ptr, cols, vals))
    p = _plan(gpu, d_ptr, d_cols, n, base)
    assert p.status == capi.SPGPU_SUCCESS and p.levels == w_levels, (case, p.status, p.levels, w_levels)
    assert p.order.numpy(np.int32).tobytes() == w_order.tobytes(), case
    assert p.diag_pos.numpy(np.int32).tobytes() == w_diag.tobytes(), case
    got_ptr = p.level_ptr.numpy(np.int32)
    assert got_ptr[:w_levels + 1].tobytes() == w_level_ptr.tobytes(), case
    assert (got_ptr[w_levels + 1:].view(np.uint8) == PATTERN).all(), case                       # untouched beyond
    assert p.host[4:4 + w_levels + 1].tobytes() == w_level_ptr.tobytes(), case
    assert p.host[4 + w_levels + 1] == nnz and (p.host[4 + w_levels + 2:] == SENTINEL).all(), case   # the extra slot, nothing beyond
    p.work.buf[p.work.first:p.work.first + p.work.nbytes].fill_(0xFF)                           # the factor call never reads the scratch
    code, size = capi.TYPE_CODE[letter], dtype.itemsize
    for in_place in (False, True):
        for shape, solve, cap in _runs(caps):
            lu = _Guarded(nnz * size)
            if in_place:
                lu.buf[lu.first:lu.first + nnz * size].copy_(formats.to_device(np.ascontiguousarray(vals).view(np.uint8)))
            torch.cuda.synchronize()
            args = (gpu, lu.ptr(), lu.ptr() if in_place else _p(d_vals), n, p.levels, p.order.ptr(), p.level_ptr.ptr(), p.host_at,
                    p.diag_pos.ptr(), _p(d_ptr), _p(d_cols), base, code)
            st = capi.spgpuCsrIlu0Device(*args) if shape is None else capi.spgpuCsrIlu0DeviceWith(*args, shape, solve, cap)
            assert st == capi.SPGPU_SUCCESS, (case, shape, solve, cap, in_place)
            torch.cuda.synchronize()
            assert lu.guards_intact() and p.order.guards_intact() and p.level_ptr.guards_intact() and p.diag_pos.guards_intact() \
                and p.work.guards_intact(), (case, shape, solve, cap)
            got = lu.numpy(np.uint8).tobytes()
            if np.isnan(want).any():                                                          # NaN payloads are not compared
                got = np.frombuffer(got, dtype)
                assert np.array_equal(np.isnan(got), np.isnan(want)) and got[~np.isnan(want)].tobytes() == want[~np.isnan(want)].tobytes()
            else:
                assert got == want.tobytes(), (case, shape, solve, cap, in_place)
    for d, h in zip((d_ptr, d_cols, d_vals), (ptr, cols, vals)):                                 # the inputs are as they were
        assert d.cpu().numpy().reshape(-1)[:h.size].tobytes() == h.tobytes(), case
    assert p.order.numpy(np.int32).tobytes() == w_order.tobytes() and p.diag_pos.numpy(np.int32).tobytes() == w_diag.tobytes(), case
    return w_levels, want


# ---- 1. every type x both bases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
def test_random_systems_give_numpys_bytes(gpu, letter, base):
    """70 rows, up to 6 off-diagonals anywhere on both sides, ascending; some updates hit a stored entry and some are dropped."""
    rng = np.random.default_rng(200 + ord(letter) + base)
    mat = I.random_system(rng, 70, letter, base)
    hit, dropped = I.update_counts(mat[0], mat[1], base)
    assert hit > 0 and dropped > 0
    levels, lu = _factor(gpu, mat, letter, base)
    assert levels > 3 and not np.isnan(lu).any() and lu.tobytes() != mat[2].tobytes()


# ---- 2. row lengths around the group widths, and a block where every update hits ------------------------------------------------
def _group_widths():
    from spgpu_amd import capi
    return [capi.ILU0_GROUP_NARROW, capi.ILU0_GROUP_WIDE]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("letter", "DC")
def test_row_lengths_around_the_group_width(gpu, which, letter):
    """Rows of L - 1, L, L + 1 and 2 L + 1 stored entries -- with both parts, without a lower part, without an upper part --, a row
    that is only its diagonal and a dependency whose upper part is empty (tests/ilu0_cases.py rows_around)."""
    L = _group_widths()[which]
    rng = np.random.default_rng(300 + L)
    mat = I.rows_around(rng, L, letter, which)
    lengths = np.diff(mat[0])
    assert {L - 1, L, L + 1, 2 * L + 1} <= set(lengths.tolist()) and lengths[0] == 1 and lengths[1] == 2
    hit, dropped = I.update_counts(mat[0], mat[1], which)
    assert hit > 0 and dropped > 0
    _factor(gpu, mat, letter, which)


@pytest.mark.parametrize("letter", "SZ")
def test_a_dense_block_where_every_update_hits(gpu, letter):
    rng = np.random.default_rng(340)
    mat = I.dense_block(rng, 40, letter, 1)
    assert I.update_counts(mat[0], mat[1], 1)[1] == 0
    levels, _ = _factor(gpu, mat, letter, 1)
    assert levels == 40


# ---- 3. levels around the factorisation's chain width ------------------------------------------------------------------------
def _sequences():
    from spgpu_amd import capi
    w = capi.ILU0_CHAIN_WIDTH
    return {"w-1 alone": [w - 1], "w alone": [w], "w+1 alone": [w + 1], "3w alone": [3 * w],
            "wide narrow wide narrow": [3 * w, 5, w + 1, w], "narrow wide narrow wide": [w - 1, 3 * w, w, w + 1],
            "narrow runs around wide levels": [2, 3, w + 1, 1, w - 1, 3 * w, 7, 1]}


@pytest.mark.parametrize("name", ["w-1 alone", "w alone", "w+1 alone", "3w alone", "wide narrow wide narrow", "narrow wide narrow wide",
                                  "narrow runs around wide levels"])
def test_levels_around_the_chain_width(gpu, name):
    widths = _sequences()[name]
    rng = np.random.default_rng(40 + len(name))
    letter = "D" if len(widths) % 2 else "C"
    mat, level = I.from_levels(rng, widths, letter, 0)
    levels, _ = _factor(gpu, mat, letter, 0)
    assert levels == len(widths)
    from spgpu_amd import formats
    _, order, level_ptr, _ = formats.csr_ilu0_plan(mat[0], mat[1], 0)
    assert np.diff(level_ptr).tolist() == widths and np.array_equal(level[order], np.repeat(np.arange(len(widths)), widths))


@pytest.mark.parametrize("n", [1, 2, 300])
def test_a_bidiagonal_chain(gpu, n):
    rng = np.random.default_rng(20 + n)
    for letter in "DC":
        levels, _ = _factor(gpu, I.bidiagonal(rng, n, letter, 1), letter, 1)
        assert levels == n


# ---- 4. stencils ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,dims", [(16, 2), (8, 3)])
def test_a_stencil_matrix(gpu, g, dims):
    rng = np.random.default_rng(60 + g)
    mat = I.stencil(rng, g, dims, "D", 0)
    hit, dropped = I.update_counts(mat[0], mat[1])
    assert hit > 0 and dropped > 0
    levels, _ = _factor(gpu, mat, "D", 0)
    assert levels == dims * (g - 1) + 1


# ---- 5. details of the contract --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SD")
def test_no_fused_multiply_add_joins_the_product_to_the_difference(gpu, letter):
    """64 blocks a - ((l / 1) * u) with a = round(l * u) and l * u inexact: exactly +0 when the product is rounded first, the
    product's rounding error -- not 0 -- from one fused multiply-add."""
    mat = I.fused_update_blocks(np.random.default_rng(500 + ord(letter)), letter)
    _, lu = _factor(gpu, mat, letter, 0)
    assert np.all(lu[3::4] == 0) and not np.signbit(lu[3::4]).any()


@pytest.mark.parametrize("letter", "CZ")
def test_no_fused_multiply_add_inside_a_complex_product_or_quotient(gpu, letter):
    """Blocks that each aim at one multiply of the complex product (four) or quotient (six): fusing it into the add or subtract
    behind it changes bytes -- tests/test_ilu0_restated.py shows that with exact fractions for these very generators.  The watched
    component is 0 only unfused; the bytes as a whole are compared in _factor."""
    rng = np.random.default_rng(600 + ord(letter))
    mat, aims = I.fused_complex_product_blocks(rng, letter)
    _, lu = _factor(gpu, mat, letter, 0)
    for t, (_, _, fusion, zero) in enumerate(aims):
        assert getattr(lu[4 * t + 3], zero) == 0, (t, fusion)
    mat, aims = I.complex_quotient_blocks(rng, letter)
    _, lu = _factor(gpu, mat, letter, 0)
    for t, (l, d, fusion, zero) in enumerate(aims):
        plain = I.complex_quotient(l, d, X.REAL_OF[letter])
        assert (lu[4 * t + 2].real, lu[4 * t + 2].imag) == plain and I.complex_quotient(l, d, X.REAL_OF[letter], fusion) != plain, (t, fusion)
        assert zero is None or getattr(lu[4 * t + 2], zero) == 0, (t, fusion)


def test_the_fp32_division_is_correctly_rounded(gpu):
    mat, n, d = I.division_blocks(np.random.default_rng(4))
    _, lu = _factor(gpu, mat, "S", 0)
    assert np.all(lu[2::4] == n / d) and np.all(lu[2::4] != n * (np.float32(1) / d))


@pytest.mark.parametrize("letter,big", [("S", 1e8), ("D", 1e16)])
def test_the_updates_of_one_entry_arrive_in_ascending_k(gpu, letter, big):
    for big_first, last in ((False, 0.0), (True, -1.0)):
        _, lu = _factor(gpu, I.cancellation(letter, big, big_first), letter, 0)
        assert lu[-1] == last


@pytest.mark.parametrize("letter", "SD")
def test_a_lone_negative_zero_keeps_its_bits(gpu, letter):
    mat = I.lone_negative_zero(letter)
    _, lu = _factor(gpu, mat, letter, 0)
    assert lu.tobytes() == mat[2].tobytes()


@pytest.mark.parametrize("letter", "SD")
def test_a_zero_pivot_is_left_to_ieee(gpu, letter):
    """a00 = 0: the multiplier is 1 / 0 = inf and the last entry 1 - inf; with a10 = 0 too, 0 / 0 = NaN.  _factor compares the NaN
    mask and the bytes of everything else."""
    _, lu = _factor(gpu, T.from_rows([([0, 1], [0.0, 1.0]), ([0, 1], [1.0, 1.0])], letter), letter, 0)
    assert np.isposinf(lu[2]) and np.isneginf(lu[3]) and lu[:2].tolist() == [0.0, 1.0]
    _, lu = _factor(gpu, T.from_rows([([0, 1], [0.0, 1.0]), ([0, 1], [0.0, 1.0])], letter), letter, 0)
    assert np.isnan(lu[2:]).all() and lu[:2].tolist() == [0.0, 1.0]


# ---- 6. the refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("kind", ["column below the base", "column at base + rows", "descending row", "repeated column", "missing diagonal"])
def test_a_bad_matrix_is_refused(gpu, kind, base):
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(70)
    ptr, cols, vals = I.random_system(rng, 70, "D", base)
    cols = cols.copy()
    lengths = np.diff(ptr)
    k = int(np.argmax((lengths >= 4) & (np.arange(70) > 2) & (np.arange(70) < 67)))
    first = ptr[k] - base
    assert lengths[k] >= 4
    mine = slice(first, first + lengths[k])
    at_diagonal = first + int(np.flatnonzero(cols[mine] - base == k)[0])
    others = [e for e in range(first, first + lengths[k]) if e != at_diagonal]
    if kind == "column below the base":
        cols[first] = base - 1
    elif kind == "column at base + rows":
        cols[first + lengths[k] - 1] = base + 70
    elif kind == "descending row":
        cols[first], cols[first + 1] = cols[first + 1], cols[first]
    elif kind == "repeated column":
        cols[others[1]] = cols[others[0]]
        cols[mine] = np.sort(cols[mine])
        assert (np.diff(cols[mine]) == 0).sum() == 1 and (cols[mine] - base == k).any()        # only the repeat is wrong
    else:
        cols[at_diagonal] = np.setdiff1d(np.arange(70) + base, cols[mine])[0]
        cols[mine] = np.sort(cols[mine])
        assert (np.diff(cols[mine]) > 0).all() and not (cols[mine] - base == k).any()          # only the diagonal is wrong
    with pytest.raises(ValueError):
        formats.csr_ilu0_plan(ptr, cols, base)
    d_ptr, d_cols = _device((ptr, cols))
    p = _plan(gpu, d_ptr, d_cols, 70, base)                                                       # the guards are checked in _plan
    assert p.status == capi.SPGPU_UNSUPPORTED and p.levels == 0, kind
    _factor(gpu, I.random_system(rng, 70, "D", base), "D", base, caps=(0,))                      # the handle works on


def test_degenerate_shapes(gpu):
    import torch
    from spgpu_amd import capi
    order, level_ptr, diag_pos, lu = _Guarded(64), _Guarded(64), _Guarded(64), _Guarded(64)
    host = np.full(8, SENTINEL, np.int32)
    levels = C.c_int(-7)
    at = host.ctypes.data_as(C.POINTER(C.c_int))
    for rows in (0, -2):
        assert capi.spgpuCsrIlu0PlanDevice(gpu, C.byref(levels), order.ptr(), level_ptr.ptr(), at, diag_pos.ptr(), rows, None, None, 0,
                                           None) == capi.SPGPU_SUCCESS and levels.value == 0
        levels.value = -7
    for rows, count in ((0, 3), (-2, 3), (5, 0), (5, -1)):
        assert capi.spgpuCsrIlu0Device(gpu, lu.ptr(), lu.ptr(), rows, count, order.ptr(), level_ptr.ptr(), at, diag_pos.ptr(), None, None, 0,
                                       capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    assert order.untouched() and level_ptr.untouched() and diag_pos.untouched() and lu.untouched() and (host == SENTINEL).all()
    for letter in "SDCZ":                                                    # 1 x 1
        for base in (0, 1):
            _, got = _factor(gpu, T.from_rows([([0], [1.5])], letter, base), letter, base)
            assert got.tolist() == [1.5]


# ---- 7. determinism ----------------------------------------------------------------------------------------------------
def test_a_repeated_call_gives_the_same_bytes_and_every_shape_equals_every_other(gpu):
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(9)
    ptr, cols, vals = I.random_system(rng, 3000, "D", 0, longest=12)
    n, nnz = 3000, vals.size
    levels, order, level_ptr, diag_pos = formats.csr_ilu0_plan(ptr, cols, 0)
    d_ptr, d_cols, d_vals, d_order, d_level_ptr, d_diag = _device((ptr, cols, vals, order, level_ptr, diag_pos))
    host = np.ascontiguousarray(np.append(level_ptr, nnz).astype(np.int32))
    seen = set()
    for shape, solve, _ in _runs((0,)) * 2 + [(2, 1, 0), (64, 0, 0)]:
        lu = _Guarded(nnz * 8)
        torch.cuda.synchronize()
        assert capi.spgpuCsrIlu0DeviceWith(gpu, lu.ptr(), _p(d_vals), n, levels, _p(d_order), _p(d_level_ptr), host.ctypes.data_as(C.POINTER(C.c_int)),
                                           _p(d_diag), _p(d_ptr), _p(d_cols), 0, capi.TYPE_DOUBLE, shape or 0, -1 if solve is None else solve,
                                           0) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        seen.add(lu.buf.cpu().numpy().tobytes())
    assert len(seen) == 1 and lu.numpy(np.float64).tobytes() == formats.csr_ilu0(ptr, cols, vals).tobytes()
    widths = np.diff(level_ptr)
    assert widths.max() > capi.ILU0_CHAIN_WIDTH and widths.min() <= capi.ILU0_CHAIN_WIDTH       # both kinds of segment ran


# ---- 8. factor and both solves in one captured graph ------------------------------------------------------------------------
def _solved(formats, ptr, cols, lu, b, base):
    y = formats.csr_trsv(ptr, cols, lu, b, base, LOWER, UNIT)
    return formats.csr_trsv(ptr, cols, lu, y, base, UPPER, STORED)


@pytest.mark.parametrize("shape,solve", [(1, 0), (8, 1), (None, None)])
def test_factor_and_both_solves_replay_from_one_captured_graph(gpu, shape, solve):
    """spgpuCsrIlu0Device, the L solve on the ILU plan's own arrays (LOWER, UNIT) and the U solve on a trsv plan of its own (UPPER,
    STORED), captured on the handle's stream and replayed after the matrix and b were overwritten in place: each replay gives the
    bytes of numpy's chain of restatements on the values of the moment.  Through two forced shapes and through the public call, which
    picks its shape from the extra slot of levelPtrHost when it is captured; the host array is zeroed before the replays."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(10)
    base, n = 1, 144
    ptr, cols, vals = I.stencil(rng, 12, 2, "D", base)
    nnz = vals.size
    b = T.values(rng, n, "D")
    levels, order, level_ptr, diag_pos = formats.csr_ilu0_plan(ptr, cols, base)
    u_levels, u_order, u_level_ptr = formats.csr_trsv_plan(ptr, cols, base, UPPER, STORED)
    d_ptr, d_cols, d_vals, d_b, d_order, d_level_ptr, d_diag, d_u_order, d_u_level_ptr = _device(
        (ptr, cols, vals, b, order, level_ptr, diag_pos, u_order, u_level_ptr))
    host, u_host = np.ascontiguousarray(np.append(level_ptr, nnz).astype(np.int32)), np.ascontiguousarray(u_level_ptr)
    at, u_at = (h.ctypes.data_as(C.POINTER(C.c_int)) for h in (host, u_host))
    d_lu, d_y, d_x = (torch.zeros(k, dtype=torch.float64, device="cuda:0") for k in (nnz, n, n))
    side_stream = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side_stream.cuda_stream))
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side_stream):
            args = (gpu, _p(d_lu), _p(d_vals), n, levels, _p(d_order), _p(d_level_ptr), at, _p(d_diag), _p(d_ptr), _p(d_cols), base, capi.TYPE_DOUBLE)
            if shape is None:                                                # the public call: it reads the extra slot here, at capture
                assert capi.spgpuCsrIlu0Device(*args) == capi.SPGPU_SUCCESS
            else:
                assert capi.spgpuCsrIlu0DeviceWith(*args, shape, solve, 0) == capi.SPGPU_SUCCESS
            assert capi.spgpuCsrTrsvDevice(gpu, _p(d_y), _p(d_b), n, levels, _p(d_order), _p(d_level_ptr), at, _p(d_ptr), _p(d_cols), _p(d_lu),
                                           base, LOWER, UNIT, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
            assert capi.spgpuCsrTrsvDevice(gpu, _p(d_x), _p(d_y), n, u_levels, _p(d_u_order), _p(d_u_level_ptr), u_at, _p(d_ptr), _p(d_cols),
                                           _p(d_lu), base, UPPER, STORED, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
        host[:] = 0                                                          # read at capture time, not at replay
        u_host[:] = 0
        wants = set()
        for _ in range(2):
            new_vals, new_b = I.stencil(rng, 12, 2, "D", base)[2], T.values(rng, n, "D")
            want_lu = formats.csr_ilu0(ptr, cols, new_vals, base)
            want_x = _solved(formats, ptr, cols, want_lu, new_b, base)
            wants.add(want_lu.tobytes() + want_x.tobytes())
            d_vals.copy_(formats.to_device(new_vals))
            d_b.copy_(formats.to_device(new_b))
            for t in (d_lu, d_y, d_x):
                t.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert d_lu.cpu().numpy().tobytes() == want_lu.tobytes() and d_x.cpu().numpy().tobytes() == want_x.tobytes()
            assert d_vals.cpu().numpy().tobytes() == new_vals.tobytes()
        assert len(wants) == 2
    finally:
        capi.spgpuSetStream(gpu, None)


# ---- 9. end to end: the three calls compose into a solver on a matrix without fill -----------------------------------------------
def test_factor_and_two_solves_solve_a_tridiagonal_system(gpu):
    """300 rows, fp64, diagonal in [1, 2), the off-diagonals of a row sum to at most 0.5 in modulus: no fill, so L U = A up to
    rounding.  By rows the matrix is dominant with rho <= 0.5, so cond_inf <= (max |a_ii| / min |a_ii|) (1 + rho) / (1 - rho) <= 6 (the
    derivation is in tests/test_trsv_restated.py), and n u is about 3e-14: the bound of 1e-10 relative in the max norm leaves three
    orders of margin.  The byte comparisons above are the sharp test; this one shows that the calls compose."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(11)
    n, base = 300, 0
    ptr, cols, vals = I.tridiagonal(rng, n, "D", base)
    dense, _ = I.dense_of((ptr, cols, vals), base)
    assert np.all((np.abs(dense).sum(axis=1) - np.abs(np.diag(dense))) <= 0.5) and np.all((np.diag(dense) >= 1) & (np.diag(dense) < 2))
    b = T.values(rng, n, "D")
    d_ptr, d_cols, d_vals, d_b = _device((ptr, cols, vals, b))
    p = _plan(gpu, d_ptr, d_cols, n, base)
    assert p.status == capi.SPGPU_SUCCESS and p.levels == n
    work = torch.empty(capi.spgpuCsrTrsvWorkBytes(n), dtype=torch.uint8, device="cuda:0")
    u_order, u_level_ptr = (torch.zeros(k, dtype=torch.int32, device="cuda:0") for k in (n, n + 1))
    u_host = np.zeros(n + 1, np.int32)
    u_levels = C.c_int(-1)
    u_at = u_host.ctypes.data_as(C.POINTER(C.c_int))
    assert capi.spgpuCsrTrsvPlanDevice(gpu, C.byref(u_levels), _p(u_order), _p(u_level_ptr), u_at, n, _p(d_ptr), _p(d_cols), base, UPPER, STORED,
                                       _p(work)) == capi.SPGPU_SUCCESS
    d_lu, d_x = torch.zeros(vals.size, dtype=torch.float64, device="cuda:0"), torch.zeros(n, dtype=torch.float64, device="cuda:0")
    assert capi.spgpuCsrIlu0Device(gpu, _p(d_lu), _p(d_vals), n, p.levels, p.order.ptr(), p.level_ptr.ptr(), p.host_at, p.diag_pos.ptr(), _p(d_ptr),
                                   _p(d_cols), base, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
    assert capi.spgpuCsrTrsvDevice(gpu, _p(d_x), _p(d_b), n, p.levels, p.order.ptr(), p.level_ptr.ptr(), p.host_at, _p(d_ptr), _p(d_cols), _p(d_lu),
                                   base, LOWER, UNIT, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
    assert capi.spgpuCsrTrsvDevice(gpu, _p(d_x), _p(d_x), n, u_levels.value, _p(u_order), _p(u_level_ptr), u_at, _p(d_ptr), _p(d_cols), _p(d_lu),
                                   base, UPPER, STORED, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    got = d_x.cpu().numpy()
    want = np.linalg.solve(dense, b)
    error = np.abs(got - want).max() / np.abs(want).max()
    print(f"ILU(0) + two solves on a tridiagonal matrix: error {error:.3e}, bound 1e-10")
    assert error <= 1e-10
    assert got.tobytes() == _solved(formats, ptr, cols, formats.csr_ilu0(ptr, cols, vals, base), b, base).tobytes()
