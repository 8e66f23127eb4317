"""GPU: the aggregation calls on CSR arrays (include/spgpu/ext/aggregate_device.h).

Every device output -- strong, diagAbs, aggregateOf, aggregateSize, T's three arrays -- and the scratch lie between 64 guard bytes and
are poisoned as a whole with one byte pattern; the two host counts lie between sentinels.  strong, diagAbs, aggregateOf,
aggregateSize[:count], both counts and T's arrays must equal numpy's restatement of the contract (spgpu_amd.formats) BYTE FOR BYTE,
aggregateSize must keep its poison behind the count, through the public calls and through every row shape (one thread per row,
groups of 8, 32 and 64 lanes), each on the whole grid and on a grid of one workgroup (_run).  The matrices are the smallest at which
each branch can go wrong (tests/aggregate_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import aggregate_cases as A
from test_gpu_csr_device import _p
from test_gpu_to_csr_device import PATTERN, _Guarded

pytestmark = pytest.mark.gpu
SENTINEL = -7
SHAPES = (1, 8, 32, 64)
CODE = {np.dtype(np.float32): "S", np.dtype(np.float64): "D", np.dtype(np.complex64): "C", np.dtype(np.complex128): "Z"}


def _device(arrays):
    from spgpu_amd import formats
    some = lambda a: a if a.size else np.zeros(1, a.dtype)
    return tuple(formats.to_device(some(np.ascontiguousarray(a))) for a in arrays)


def _runs(caps=(0, 1)):
    return [(None, 0)] + [(shape, cap) for shape in SHAPES for cap in caps]


def _strength(gpu, d_ptr, d_cols, d_vals, n, nnz, base, theta, dtype, shape, cap):
    """One strength call between guards -> (strong, diagAbs) as numpy arrays; the guards are checked here."""
    import torch
    from spgpu_amd import capi
    strong, diag = _Guarded(nnz, 3), _Guarded(n * dtype.itemsize)              # the mask at an odd address: bytes have no alignment
    args = (gpu, strong.ptr(), diag.ptr(), n, _p(d_ptr), _p(d_cols), _p(d_vals), base, theta, capi.TYPE_CODE[CODE[dtype]])
    st = capi.spgpuCsrStrengthDevice(*args) if shape is None else capi.spgpuCsrStrengthDeviceWith(*args, shape, cap)
    assert st == capi.SPGPU_SUCCESS, (shape, cap)
    torch.cuda.synchronize()
    assert strong.guards_intact() and diag.guards_intact(), (shape, cap)
    return strong, diag


def _aggregate(gpu, d_ptr, d_cols, d_strong, n, base, shape, cap):
    """One aggregation between guards and sentinels -> (status, count, rounds, aggregateOf, aggregateSize as _Guarded)."""
    import torch
    from spgpu_amd import capi
    work = _Guarded(capi.spgpuCsrAggregateWorkBytes(n), 192)                   # 256-byte aligned
    of, size = _Guarded(n * 4), _Guarded(n * 4)
    host = np.full(10, SENTINEL, np.int32)                                    # [4 sentinels | count | rounds | 4 sentinels]
    count_at = host[4:].ctypes.data_as(C.POINTER(C.c_int))
    rounds_at = host[5:].ctypes.data_as(C.POINTER(C.c_int))
    torch.cuda.synchronize()
    args = (gpu, count_at, rounds_at, of.ptr(), size.ptr(), n, _p(d_ptr), _p(d_cols), d_strong, base, work.ptr())
    st = capi.spgpuCsrAggregateDevice(*args) if shape is None else capi.spgpuCsrAggregateDeviceWith(*args, shape, cap)
    torch.cuda.synchronize()
    assert work.guards_intact() and of.guards_intact() and size.guards_intact(), (shape, cap)
    assert (host[:4] == SENTINEL).all() and (host[6:] == SENTINEL).all()
    return st, int(host[4]), int(host[5]), of, size


def _tentative(gpu, d_of, n, base, dtype, candidate):
    """T between guards against formats.csr_tentative; `candidate` a numpy array or None."""
    import torch
    from spgpu_amd import capi, formats
    want_ptr, want_cols, want_vals = formats.csr_tentative(d_of.cpu().numpy()[:n], candidate, base, dtype)
    t_ptr, t_cols, t_vals = _Guarded((n + 1) * 4), _Guarded(n * 4), _Guarded(n * dtype.itemsize)
    d_candidate = None if candidate is None else _device((candidate,))[0]
    assert capi.spgpuCsrTentativeDevice(gpu, t_ptr.ptr(), t_cols.ptr(), t_vals.ptr(), n, _p(d_of), _p(d_candidate), base,
                                        capi.TYPE_CODE[CODE[dtype]]) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    assert t_ptr.guards_intact() and t_cols.guards_intact() and t_vals.guards_intact()
    assert t_ptr.numpy(np.int32).tobytes() == want_ptr.tobytes() and t_cols.numpy(np.int32).tobytes() == want_cols.tobytes()
    assert t_vals.numpy(np.uint8).tobytes() == want_vals.tobytes()
    return want_ptr, want_cols, want_vals


def _run(gpu, mat, base, theta=0.25, caps=(0, 1), mask="strength"):
    """Strength, aggregation and T on host CSR arrays given in `base`, every call and shape against formats.  mask: "strength" (the
    device's own strong), None (strong == NULL).  Returns (count, rounds, aggregate_of, sizes, strong) restated."""
    import torch
    from spgpu_amd import capi, formats
    ptr, cols, vals = mat
    dtype = vals.dtype
    n, nnz = ptr.size - 1, vals.size
    case = (str(dtype), n, base)
    d_ptr, d_cols, d_vals = _device((ptr, cols, vals))
    want_strong, want_diag = formats.csr_strength(ptr, cols, vals, base, theta)
    want = formats.csr_aggregate(ptr, cols, want_strong if mask == "strength" else None, base)
    kept = None
    for shape, cap in _runs(caps):
        strong, diag = _strength(gpu, d_ptr, d_cols, d_vals, n, nnz, base, theta, dtype, shape, cap)
        assert strong.numpy(np.uint8).tobytes() == want_strong.tobytes(), (case, shape, cap)
        assert diag.numpy(np.uint8).tobytes() == want_diag.tobytes(), (case, shape, cap)
        kept = strong
    for shape, cap in _runs(caps):
        st, count, rounds, of, size = _aggregate(gpu, d_ptr, d_cols, kept.ptr() if mask == "strength" else None, n, base, shape, cap)
        assert st == capi.SPGPU_SUCCESS and (count, rounds) == want[:2], (case, shape, cap, st, count, rounds, want[:2])
        assert of.numpy(np.int32).tobytes() == want[2].tobytes(), (case, shape, cap)
        got_size = size.numpy(np.int32)
        assert got_size[:count].tobytes() == want[3].tobytes(), (case, shape, cap)
        assert (got_size[count:].view(np.uint8) == PATTERN).all(), (case, shape, cap)          # untouched beyond the count
    d_of = formats.to_device(want[2])
    _tentative(gpu, d_of, n, base, dtype, None)
    for d, h in zip((d_ptr, d_cols, d_vals), (ptr, cols, vals)):                               # the inputs are as they were
        assert d.cpu().numpy().reshape(-1).view(np.uint8)[:h.nbytes].tobytes() == h.tobytes(), case
    assert kept.numpy(np.uint8).tobytes() == want_strong.tobytes()
    torch.cuda.synchronize()
    return want + (want_strong,)


# ---- 1. grids: both bases, both real types -----------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [4, 16])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_5_point_grid_gives_numpys_bytes(gpu, g, base, dtype):
    count, rounds, aggregate_of, sizes, strong = _run(gpu, A.grid_5pt(g, base, dtype), base)
    assert strong.sum() == 4 * g * (g - 1) and rounds >= 1 and sizes.sum() == g * g and 1 <= count < g * g


def test_anisotropy_keeps_the_aggregates_on_their_grid_lines(gpu):
    """Coupling 1 in x and 2^-10 in y: strong edges run only along x, so no aggregate spans two grid lines."""
    g = 16
    mat = A.grid_5pt(g, 1, np.float64, cx=1.0, cy=2.0 ** -10)
    count, _, aggregate_of, _, strong = _run(gpu, mat, 1)
    assert strong.sum() == 2 * g * (g - 1)
    lines = np.arange(g * g) // g
    assert all(np.unique(lines[aggregate_of == a]).size == 1 for a in range(count))


# ---- 2. unsymmetric patterns, the chain, the strip ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_random_unsymmetric_patterns(gpu, seed):
    """200 rows with empty rows, rows without a diagonal, a column stored twice and descending columns."""
    rng = np.random.default_rng(1000 + seed)
    mat = A.random_unsymmetric(rng, 200, seed, np.float32 if seed else np.float64)
    assert not A.symmetric(A.neighbours(mat[0], mat[1], None, seed))
    _run(gpu, mat, seed, theta=0.0)
    _run(gpu, mat, seed, theta=0.5, caps=(1,))


def test_a_chain_takes_several_rounds(gpu):
    _, rounds, _, _, _ = _run(gpu, A.chain(300, 1), 1)
    assert 2 <= rounds < 30


def test_1025_rows_on_one_workgroup_with_a_row_longer_than_every_group(gpu):
    """The grid stride of every shape (1025 rows on one workgroup), a row of 200 strong entries -- longer than 64 lanes -- and rows of
    one to three -- lanes without an entry."""
    mat = A.strip_1025(0)
    lengths = np.diff(mat[0])
    assert lengths[7] == 201 and {2, 3, 4} <= set(lengths[np.arange(1025) != 7].tolist()) <= {1, 2, 3, 4}
    _, _, _, _, strong = _run(gpu, mat, 0)
    assert strong.sum() == mat[2].size - 1025                                  # every off-diagonal is strong


# ---- 3. the threshold ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("base", [0, 1])
def test_the_threshold_edge_cases_through_the_device(gpu, dtype, base):
    """Equality, one ulp below, NaN value, NaN diagonal, zero and missing diagonal, -0.0, theta = 0 and a column outside the matrix:
    the hand-written expectations of tests/aggregate_cases.py threshold_matrix, through every shape."""
    ptr, cols, vals, at_half, at_zero, want_diag = A.threshold_matrix(dtype, base)
    dtype = np.dtype(dtype)
    n, nnz = ptr.size - 1, vals.size
    d_ptr, d_cols, d_vals = _device((ptr, cols, vals))
    for theta, want in ((0.5, at_half), (0.0, at_zero)):
        for shape, cap in _runs():
            strong, diag = _strength(gpu, d_ptr, d_cols, d_vals, n, nnz, base, theta, dtype, shape, cap)
            assert strong.numpy(np.uint8).tolist() == want.tolist(), (theta, shape, cap)
            assert diag.numpy(np.uint8).tobytes() == want_diag.tobytes(), (theta, shape, cap)


# ---- 4. strong == NULL, and the refusal -----------------------------------------------------------------------------------
def test_no_mask_is_an_all_ones_mask(gpu):
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(7)
    ptr, cols, vals = A.random_unsymmetric(rng, 200, 1)
    d_ptr, d_cols = _device((ptr, cols))
    ones = torch.ones(vals.size, dtype=torch.uint8, device="cuda:0")
    want = formats.csr_aggregate(ptr, cols, None, 1)
    for d_strong in (None, _p(ones)):
        for shape, cap in _runs():
            st, count, rounds, of, size = _aggregate(gpu, d_ptr, d_cols, d_strong, 200, 1, shape, cap)
            assert st == capi.SPGPU_SUCCESS and (count, rounds) == want[:2]
            assert of.numpy(np.int32).tobytes() == want[2].tobytes() and size.numpy(np.int32)[:count].tobytes() == want[3].tobytes()


@pytest.mark.parametrize("bad", [10, -1, 2 ** 31 - 1])
def test_a_neighbour_outside_the_matrix_is_refused(gpu, bad):
    """An out-of-range column under strong == NULL and with its mask byte forced to 1: SPGPU_UNSUPPORTED, both counts 0, the guards
    intact (_aggregate); with its mask byte 0 the entry is no neighbour and the call goes through."""
    import torch
    from spgpu_amd import capi, formats
    ptr, cols, _ = A.chain(10)
    wrong = cols.copy()
    wrong[4] = bad
    d_ptr, d_cols = _device((ptr, wrong))
    ones = torch.ones(cols.size, dtype=torch.uint8, device="cuda:0")
    for d_strong in (None, _p(ones)):
        for shape, cap in _runs():
            st, count, rounds, _, _ = _aggregate(gpu, d_ptr, d_cols, d_strong, 10, 0, shape, cap)
            assert (st, count, rounds) == (capi.SPGPU_UNSUPPORTED, 0, 0), (shape, cap)
    mask = np.ones(cols.size, np.uint8)
    mask[4] = 0
    want = formats.csr_aggregate(ptr, wrong, mask, 0)
    d_mask = formats.to_device(mask)                                          # held: the call reads it
    st, count, rounds, of, _ = _aggregate(gpu, d_ptr, d_cols, _p(d_mask), 10, 0, None, 0)
    assert (st, count, rounds) == (capi.SPGPU_SUCCESS,) + want[:2] and of.numpy(np.int32).tobytes() == want[2].tobytes()


# ---- 5. the tentative prolongator ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_the_tentative_prolongator_moves_the_candidates_bits(gpu, dtype):
    """All four value types; a candidate with -0.0 and a NaN that carries a payload, compared as bits; and candidate == NULL."""
    from spgpu_amd import formats
    dtype = np.dtype(dtype)
    n = 700                                                                   # three workgroups, the last one ragged
    rng = np.random.default_rng(3)
    aggregate_of = rng.integers(0, 90, n).astype(np.int32)
    words = np.dtype("u4") if dtype in (np.dtype(np.float32), np.dtype(np.complex64)) else np.dtype("u8")
    part = np.dtype("f4") if words == np.dtype("u4") else np.dtype("f8")
    candidate = rng.standard_normal(n * dtype.itemsize // part.itemsize).astype(part)
    candidate[1] = -0.0
    raw = candidate.view(words)
    raw[2] = (0x7FC00000 | 0x1234) if words.itemsize == 4 else (0x7FF8000000000000 | 0x123456789)   # a quiet NaN with a payload
    candidate = candidate.view(dtype)
    d_of = formats.to_device(aggregate_of)
    for base in (0, 1):
        _, _, vals = _tentative(gpu, d_of, n, base, dtype, candidate)
        assert vals.tobytes() == candidate.tobytes()
        _, _, ones = _tentative(gpu, d_of, n, base, dtype, None)
        assert ones.tolist() == [1] * n


# ---- 6. strength and T in one captured graph --------------------------------------------------------------------------------
def test_strength_and_tentative_replay_from_one_captured_graph(gpu):
    """spgpuCsrStrengthDevice and spgpuCsrTentativeDevice captured on the handle's stream and replayed after the values and the
    candidate changed in place: each replay gives the bytes of numpy's restatement on the values of the moment.  The aggregation
    synchronises and is not captured: aggregateOf is computed before."""
    import torch
    from spgpu_amd import capi, formats
    base, g = 1, 12
    n = g * g
    ptr, cols, vals = A.grid_5pt(g, base)
    nnz = vals.size
    aggregate_of = formats.csr_aggregate(ptr, cols, None, base)[2]
    rng = np.random.default_rng(11)
    d_ptr, d_cols, d_vals, d_of, d_candidate = _device((ptr, cols, vals, aggregate_of, np.ones(n)))
    d_strong = torch.zeros(nnz, dtype=torch.uint8, device="cuda:0")
    d_diag, d_tvals = (torch.zeros(n, dtype=torch.float64, device="cuda:0") for _ in range(2))
    d_tptr, d_tcols = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0")
    side_stream = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side_stream.cuda_stream))
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side_stream):
            assert capi.spgpuCsrStrengthDevice(gpu, _p(d_strong), _p(d_diag), n, _p(d_ptr), _p(d_cols), _p(d_vals), base, 0.25,
                                               capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
            assert capi.spgpuCsrTentativeDevice(gpu, _p(d_tptr), _p(d_tcols), _p(d_tvals), n, _p(d_of), _p(d_candidate), base,
                                                capi.TYPE_DOUBLE) == capi.SPGPU_SUCCESS
        masks = set()
        for k in range(2):
            new_vals = vals * np.where(rng.random(nnz) < 0.5, 1.0, 2.0 ** -6)          # some couplings become weak
            new_candidate = rng.standard_normal(n)
            want_strong, want_diag = formats.csr_strength(ptr, cols, new_vals, base, 0.25)
            want_t = formats.csr_tentative(aggregate_of, new_candidate, base, np.float64)
            masks.add(want_strong.tobytes())
            d_vals.copy_(formats.to_device(new_vals))
            d_candidate.copy_(formats.to_device(new_candidate))
            d_strong.fill_(0xA5)
            for t in (d_diag, d_tvals):
                t.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert d_strong.cpu().numpy().tobytes() == want_strong.tobytes() and d_diag.cpu().numpy().tobytes() == want_diag.tobytes()
            assert d_tptr.cpu().numpy().tobytes() == want_t[0].tobytes() and d_tcols.cpu().numpy().tobytes() == want_t[1].tobytes()
            assert d_tvals.cpu().numpy().tobytes() == want_t[2].tobytes()
            assert 0 < want_strong.sum() < 4 * g * (g - 1)
        assert len(masks) == 2
    finally:
        capi.spgpuSetStream(gpu, None)
