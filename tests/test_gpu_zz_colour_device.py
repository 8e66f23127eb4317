"""GPU: the multicolour-ordering calls on CSR arrays (include/spgpu/ext/colour_device.h).

Every device output -- colourOf, order, inverse, colourPtr, B's three arrays -- and both scratch areas lie between 64 guard bytes and
are poisoned as a whole with one byte pattern; the two host counts lie between sentinels.  Every array must equal numpy's
restatement of the contract (spgpu_amd.formats) BYTE FOR BYTE, colourPtr must keep its poison behind coloursCount + 1 ints, through
the public calls and through every row shape (one thread per row, groups of 8, 32 and 64 lanes), each on the whole grid and on a
grid of one workgroup (_run).  The matrices are the smallest at which each branch can go wrong (tests/colour_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import colour_cases as K
from test_gpu_csr_device import _p
from test_gpu_to_csr_device import PATTERN, _Guarded

pytestmark = pytest.mark.gpu
SENTINEL = -7
SHAPES = (1, 8, 32, 64)
CODE = {np.dtype(np.float32): "S", np.dtype(np.float64): "D", np.dtype(np.complex64): "C", np.dtype(np.complex128): "Z"}
TYPES = [np.float32, np.float64, np.complex64, np.complex128]


def _device(arrays):
    from spgpu_amd import formats
    some = lambda a: a if a.size else np.zeros(1, a.dtype)
    return tuple(formats.to_device(some(np.ascontiguousarray(a))) for a in arrays)


def _runs(caps=(0, 1)):
    return [(None, 0)] + [(shape, cap) for shape in SHAPES for cap in caps]


def _colour(gpu, d_ptr, d_cols, n, base, shape, cap):
    """One colouring between guards and sentinels -> (status, colours, rounds, colourOf and the scratch as _Guarded)."""
    import torch
    from spgpu_amd import capi
    work = _Guarded(capi.spgpuCsrColourWorkBytes(n), 192)                     # 256-byte aligned
    of = _Guarded(n * 4)
    host = np.full(10, SENTINEL, np.int32)                                    # [4 sentinels | colours | rounds | 4 sentinels]
    colours_at = host[4:].ctypes.data_as(C.POINTER(C.c_int))
    rounds_at = host[5:].ctypes.data_as(C.POINTER(C.c_int))
    torch.cuda.synchronize()
    args = (gpu, colours_at, rounds_at, of.ptr(), n, _p(d_ptr), _p(d_cols), base, work.ptr())
    st = capi.spgpuCsrColourDevice(*args) if shape is None else capi.spgpuCsrColourDeviceWith(*args, shape, cap)
    torch.cuda.synchronize()
    assert work.guards_intact() and of.guards_intact(), (shape, cap)
    assert (host[:4] == SENTINEL).all() and (host[6:] == SENTINEL).all()
    return st, int(host[4]), int(host[5]), of, work


def _order(gpu, d_of, n, colours, work=None):
    """One order call between guards -> (order, inverse, colourPtr) as _Guarded; colourPtr has n + 3 ints."""
    import torch
    from spgpu_amd import capi
    work = work or _Guarded(capi.spgpuCsrColourWorkBytes(n), 192)
    order, inverse, colour_ptr = _Guarded(n * 4), _Guarded(n * 4), _Guarded((n + 3) * 4)
    assert capi.spgpuCsrColourOrderDevice(gpu, order.ptr(), inverse.ptr(), colour_ptr.ptr(), n, colours, d_of, work.ptr()) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    assert work.guards_intact() and order.guards_intact() and inverse.guards_intact() and colour_ptr.guards_intact()
    return order, inverse, colour_ptr


def _permute(gpu, d_order, d_inverse, d_mat, n, nnz, base, dtype, shape, cap):
    """One permutation between guards -> B's three arrays as _Guarded."""
    import torch
    from spgpu_amd import capi
    dtype = np.dtype(dtype)
    work = _Guarded(capi.spgpuCsrPermuteWorkBytes(n), 192)
    b_ptr, b_cols, b_vals = _Guarded((n + 1) * 4), _Guarded(nnz * 4), _Guarded(nnz * dtype.itemsize)
    args = (gpu, b_ptr.ptr(), b_cols.ptr(), b_vals.ptr(), n, _p(d_order), _p(d_inverse), _p(d_mat[0]), _p(d_mat[1]), _p(d_mat[2]), base,
            capi.TYPE_CODE[CODE[dtype]], work.ptr())
    st = capi.spgpuCsrPermuteDevice(*args) if shape is None else capi.spgpuCsrPermuteDeviceWith(*args, shape, cap)
    assert st == capi.SPGPU_SUCCESS, (shape, cap)
    torch.cuda.synchronize()
    assert work.guards_intact() and b_ptr.guards_intact() and b_cols.guards_intact() and b_vals.guards_intact(), (shape, cap)
    return b_ptr, b_cols, b_vals


def _permuted_equals(gpu, mat, base, order, inverse, caps=(0, 1)):
    """The permutation of `mat` by a given order through every run against formats.csr_permute; returns the restated B."""
    from spgpu_amd import formats
    ptr, cols, vals = mat
    n, nnz = ptr.size - 1, vals.size
    want = formats.csr_permute(order, inverse, ptr, cols, vals, base)
    d_mat = _device(mat)
    d_order, d_inverse = _device((np.asarray(order, np.int32), np.asarray(inverse, np.int32)))
    for shape, cap in _runs(caps):
        got = _permute(gpu, d_order, d_inverse, d_mat, n, nnz, base, vals.dtype, shape, cap)
        for g, w, name in zip(got, want, ("bRowPtr", "bColIndices", "bValues")):
            assert g.numpy(np.uint8).tobytes() == w.tobytes(), (name, str(vals.dtype), n, base, shape, cap)
    for d, h in zip(d_mat, mat):                                              # the inputs are as they were
        assert d.cpu().numpy().reshape(-1).view(np.uint8)[:h.nbytes].tobytes() == h.tobytes()
    return want


def _run(gpu, mat, base, caps=(0, 1)):
    """Colouring, order and permutation of host CSR arrays given in `base`, every call and shape against formats.  Returns
    (colours, rounds, colour_of, order, inverse, the restated B)."""
    from spgpu_amd import capi, formats
    ptr, cols, vals = mat
    n = ptr.size - 1
    case = (str(vals.dtype), n, base)
    d_ptr, d_cols = _device((ptr, cols))
    want = formats.csr_colour(ptr, cols, base)
    kept = None
    for shape, cap in _runs(caps):
        st, colours, rounds, of, work = _colour(gpu, d_ptr, d_cols, n, base, shape, cap)
        assert st == capi.SPGPU_SUCCESS and (colours, rounds) == want[:2], (case, shape, cap, st, colours, rounds, want[:2])
        assert of.numpy(np.int32).tobytes() == want[2].tobytes(), (case, shape, cap)
        kept = of, work
    want_order = formats.csr_colour_order(want[2], want[0])
    for work in (kept[1], None):                                              # on the colouring's scratch as it was left, and on a poisoned one
        order, inverse, colour_ptr = _order(gpu, kept[0].ptr(), n, want[0], work)
        assert order.numpy(np.int32).tobytes() == want_order[0].tobytes() and inverse.numpy(np.int32).tobytes() == want_order[1].tobytes(), case
        got_ptr = colour_ptr.numpy(np.int32)
        assert got_ptr[:want[0] + 1].tobytes() == want_order[2].tobytes(), case
        assert (got_ptr[want[0] + 1:].view(np.uint8) == PATTERN).all(), case     # untouched behind coloursCount + 1
    assert kept[0].numpy(np.int32).tobytes() == want[2].tobytes()
    b = _permuted_equals(gpu, mat, base, want_order[0], want_order[1], caps)
    return want + want_order[:2] + (b,)


# ---- 1. the symmetric cases: both bases, the counts of the table ------------------------------------------------------------------
@pytest.mark.parametrize("g", [4, 16])
@pytest.mark.parametrize("base", [0, 1])
def test_a_5_point_grid_gives_numpys_bytes(gpu, g, base):
    colours, rounds = _run(gpu, K.grid_5pt(g, base), base)[:2]
    assert (colours, rounds) == K.TABLE[f"grid5_{g}"][1:3]


@pytest.mark.parametrize("name", ["chain_300", "grid7_8", "clique_70", "clique_130"])
def test_the_chain_the_cube_and_the_cliques_past_one_and_two_windows(gpu, name):
    """A clique of 70 fills the first 64-colour window, one of 130 the first two: the row is walked again with w += 64."""
    base = 1 if name == "chain_300" else 0
    colours, rounds = _run(gpu, K.named(name, base), base)[:2]
    assert (colours, rounds) == K.TABLE[name][1:3]


# ---- 2. unsymmetric patterns, the strip -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_random_unsymmetric_patterns(gpu, seed):
    """200 rows with empty rows, rows without a diagonal, a column stored twice and descending columns."""
    rng = np.random.default_rng(1000 + seed)
    mat = K.random_unsymmetric(rng, 200, seed, np.float32 if seed else np.float64)
    assert not K.symmetric(K.neighbours(mat[0], mat[1], None, seed))
    _run(gpu, mat, seed)


def test_1025_rows_on_one_workgroup_with_a_row_longer_than_every_group(gpu):
    """The grid stride of every shape (1025 rows on one workgroup), a row of 201 entries -- longer than 64 lanes, stored in descending
    columns, ranked entry against entry by the fill -- and rows of two to four -- lanes without an entry."""
    mat = K.strip_descending(0)
    assert np.diff(mat[0])[7] == 201
    b_ptr, b_cols, _ = _run(gpu, mat, 0)[5]
    assert all(np.all(np.diff(b_cols[b_ptr[k]:b_ptr[k + 1]].astype(np.int64)) > 0) for k in range(1025))


# ---- 3. the refusal --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [10, -1, 2 ** 31 - 1])
@pytest.mark.parametrize("base", [0, 1])
def test_a_column_outside_the_matrix_is_refused(gpu, bad, base):
    """SPGPU_UNSUPPORTED, both counts 0, the guards intact (_colour): the entry is never used as an index."""
    from spgpu_amd import capi
    if base == 1 and bad == 10:
        bad = 0                                                               # one below base 1; 10 is the last column there
    ptr, cols, _ = K.out_of_range(bad, base)
    d_ptr, d_cols = _device((ptr, cols))
    for shape, cap in _runs():
        st, colours, rounds, _, _ = _colour(gpu, d_ptr, d_cols, 10, base, shape, cap)
        assert (st, colours, rounds) == (capi.SPGPU_UNSUPPORTED, 0, 0), (shape, cap)


# ---- 4. the permutation on its own -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("base", [0, 1])
def test_the_permutation_moves_the_values_bits(gpu, dtype, base):
    """All four value types by a random permutation: -0.0 and a NaN that carries a payload, compared as bits; empty rows, a column
    stored twice (storage order kept), descending columns."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(5)
    ptr, cols, _ = K.random_unsymmetric(rng, 300, base)
    words = np.dtype("u4") if dtype in (np.dtype(np.float32), np.dtype(np.complex64)) else np.dtype("u8")
    part = np.dtype("f4") if words == np.dtype("u4") else np.dtype("f8")
    vals = rng.standard_normal(cols.size * dtype.itemsize // part.itemsize).astype(part)
    vals[1] = -0.0
    vals.view(words)[2] = (0x7FC00000 | 0x1234) if words.itemsize == 4 else (0x7FF8000000000000 | 0x123456789)
    vals = vals.view(dtype)
    order = rng.permutation(300)
    inverse = np.empty(300, np.int64)
    inverse[order] = np.arange(300)
    _, _, b_vals = _permuted_equals(gpu, (ptr, cols, vals), base, order, inverse)
    assert sorted(b_vals.view(words).tolist()) == sorted(vals.view(words).tolist())


def test_the_identity_order_gives_a_with_sorted_rows(gpu):
    rng = np.random.default_rng(6)
    mat = K.random_unsymmetric(rng, 200, 1)
    identity = np.arange(200)
    b_ptr, b_cols, _ = _permuted_equals(gpu, mat, 1, identity, identity)
    assert b_ptr.tobytes() == mat[0].tobytes()
    assert all(b_cols[b_ptr[i] - 1:b_ptr[i + 1] - 1].tolist() == sorted(mat[1][mat[0][i] - 1:mat[0][i + 1] - 1].tolist()) for i in range(200))


def test_a_matrix_of_empty_rows(gpu):
    """Five rows, nothing stored: one colour, one round, the identity order, and a row pointer of bases."""
    mat = (np.ones(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))
    colours, rounds, _, order, _, (b_ptr, _, _) = _run(gpu, mat, 1)
    assert (colours, rounds) == (1, 1) and order.tolist() == list(range(5)) and b_ptr.tolist() == [1] * 6


# ---- 5. composition with the Plans -----------------------------------------------------------------------------------------
def test_the_plans_find_as_many_levels_as_colours_and_ilu0_factorises_b(gpu):
    """The 7-point matrix of an 8^3 grid: spgpuCsrTrsvPlanDevice finds 22 levels on A and coloursCount on the device's B,
    spgpuCsrIlu0PlanDevice accepts B, and spgpuCsrIlu0Device on B gives the bytes of formats.csr_ilu0 on the restated B."""
    import torch
    from spgpu_amd import capi, formats
    base, n = 0, 512
    mat = K.named("grid7_8", base)
    nnz = mat[2].size
    d_mat = _device(mat)
    st, colours, _, of, work = _colour(gpu, d_mat[0], d_mat[1], n, base, None, 0)
    assert st == capi.SPGPU_SUCCESS and colours == K.TABLE["grid7_8"][1]
    order, inverse, _ = _order(gpu, of.ptr(), n, colours, work)
    d_order, d_inverse = (formats.to_device(g.numpy(np.int32).copy()) for g in (order, inverse))
    b_ptr, b_cols, b_vals = _permute(gpu, d_order, d_inverse, d_mat, n, nnz, base, np.float64, None, 0)
    want_b = formats.csr_permute(order.numpy(np.int32), inverse.numpy(np.int32), *mat, base)

    def levels_of(row_ptr, col_indices):
        trsv_work = torch.empty(capi.spgpuCsrTrsvWorkBytes(n), dtype=torch.uint8, device="cuda:0")
        rows, level_ptr = (torch.zeros(k, dtype=torch.int32, device="cuda:0") for k in (n, n + 1))
        host, levels = np.zeros(n + 1, np.int32), C.c_int(-1)
        assert capi.spgpuCsrTrsvPlanDevice(gpu, C.byref(levels), _p(rows), _p(level_ptr), host.ctypes.data_as(C.POINTER(C.c_int)), n, row_ptr,
                                           col_indices, base, capi.TRSV_LOWER, capi.TRSV_DIAG_STORED, _p(trsv_work)) == capi.SPGPU_SUCCESS
        return levels.value

    assert levels_of(_p(d_mat[0]), _p(d_mat[1])) == K.TABLE["grid7_8"][3] == 22
    assert levels_of(b_ptr.ptr(), b_cols.ptr()) == colours
    ilu_work = torch.empty(capi.spgpuCsrIlu0WorkBytes(n), dtype=torch.uint8, device="cuda:0")
    rows, level_ptr, diag_pos = (torch.zeros(k, dtype=torch.int32, device="cuda:0") for k in (n, n + 1, n))
    host, levels = np.zeros(n + 2, np.int32), C.c_int(-1)
    at = host.ctypes.data_as(C.POINTER(C.c_int))
    assert capi.spgpuCsrIlu0PlanDevice(gpu, C.byref(levels), _p(rows), _p(level_ptr), at, _p(diag_pos), n, b_ptr.ptr(), b_cols.ptr(), base,
                                       _p(ilu_work)) == capi.SPGPU_SUCCESS
    assert levels.value == colours
    d_lu = torch.zeros(nnz, dtype=torch.float64, device="cuda:0")
    assert capi.spgpuCsrIlu0Device(gpu, _p(d_lu), b_vals.ptr(), n, levels.value, _p(rows), _p(level_ptr), at, _p(diag_pos), b_ptr.ptr(),
                                   b_cols.ptr(), base, capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    assert d_lu.cpu().numpy().tobytes() == formats.csr_ilu0(*want_b, base).tobytes()


# ---- 6. order and permutation in one captured graph -------------------------------------------------------------------------
def test_order_and_permutation_replay_from_one_captured_graph(gpu):
    """spgpuCsrColourOrderDevice and spgpuCsrPermuteDevice captured on the handle's stream and replayed after aValues changed in
    place: each replay gives the bytes of numpy's restatement on the values of the moment.  The colouring synchronises and is not
    captured: colourOf is computed before."""
    import torch
    from spgpu_amd import capi, formats
    base, g = 1, 12
    n = g * g
    ptr, cols, vals = K.grid_5pt(g, base)
    nnz = vals.size
    colours, _, colour_of = formats.csr_colour(ptr, cols, base)
    want_order = formats.csr_colour_order(colour_of, colours)
    rng = np.random.default_rng(12)
    d_ptr, d_cols, d_vals, d_of = _device((ptr, cols, vals, colour_of))
    work = torch.zeros(capi.spgpuCsrColourWorkBytes(n), dtype=torch.uint8, device="cuda:0")
    permute_work = torch.zeros(capi.spgpuCsrPermuteWorkBytes(n), dtype=torch.uint8, device="cuda:0")
    d_order, d_inverse, d_colour_ptr = (torch.zeros(k, dtype=torch.int32, device="cuda:0") for k in (n, n, colours + 1))
    d_bptr, d_bcols = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0"), torch.zeros(nnz, dtype=torch.int32, device="cuda:0")
    d_bvals = torch.zeros(nnz, dtype=torch.float64, device="cuda:0")
    side_stream = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side_stream.cuda_stream))
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side_stream):
            assert capi.spgpuCsrColourOrderDevice(gpu, _p(d_order), _p(d_inverse), _p(d_colour_ptr), n, colours, _p(d_of),
                                                  _p(work)) == capi.SPGPU_SUCCESS
            assert capi.spgpuCsrPermuteDevice(gpu, _p(d_bptr), _p(d_bcols), _p(d_bvals), n, _p(d_order), _p(d_inverse), _p(d_ptr), _p(d_cols),
                                              _p(d_vals), base, capi.TYPE_DOUBLE, _p(permute_work)) == capi.SPGPU_SUCCESS
        seen = set()
        for _ in range(2):
            new_vals = rng.standard_normal(nnz)
            want = formats.csr_permute(want_order[0], want_order[1], ptr, cols, new_vals, base)
            seen.add(want[2].tobytes())
            d_vals.copy_(formats.to_device(new_vals))
            for t in (d_order, d_inverse, d_colour_ptr, d_bptr, d_bcols):
                t.fill_(-7)
            d_bvals.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            for got, w in zip((d_order, d_inverse, d_colour_ptr, d_bptr, d_bcols, d_bvals), want_order + want):
                assert got.cpu().numpy().tobytes() == w.tobytes()
        assert len(seen) == 2
    finally:
        capi.spgpuSetStream(gpu, None)
