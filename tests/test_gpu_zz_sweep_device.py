"""GPU: the multicolour sweep, its Plan and the residual on CSR arrays (include/spgpu/ext/sweep_device.h).

Every device output -- diagPos, x, r -- and the Plan's scratch lie between 64 guard bytes and are poisoned as a whole with one byte
pattern; the Plan's host outputs lie between sentinels; the inputs are verified unchanged.  Every result must equal numpy's
restatement of the contract (spgpu_amd.formats) BYTE FOR BYTE, through the public calls and through every row shape (one thread per
row, groups of 8, 32 and 64 lanes), plain and chained segments, the whole grid and a grid of one workgroup (_RUNS), in three
directions, with omega null and given, in four value types, in both bases, with an order on A and without one on the permuted
matrix.  The matrices are the smallest at which each branch can go wrong (tests/sweep_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import sweep_cases as K
from aggregate_cases import from_rows
from test_gpu_csr_device import _p
from test_gpu_to_csr_device import PATTERN, _Guarded

pytestmark = pytest.mark.gpu
SENTINEL = -7
SHAPES = (1, 8, 32, 64)
PLAIN, CHAINED = 0, 1
CODE = {np.dtype(np.float32): "S", np.dtype(np.float64): "D", np.dtype(np.complex64): "C", np.dtype(np.complex128): "Z"}
TYPES = [np.float32, np.float64, np.complex64, np.complex128]
NAMES = ["diagonal", "row1", "chain5", "grid5_unsorted", "tridiagonal600", "arrow20", "hubs", "twice", "mixed"]
# (shape, solve, cap); None: the public call
_RUNS = [None] + [(shape, solve, cap) for shape in SHAPES for solve in (PLAIN, CHAINED) for cap in (0, 1)]
DIRECTIONS = (K.FORWARD, K.BACKWARD, K.SYMMETRIC)


def _device(arrays):
    from spgpu_amd import formats
    some = lambda a: a if a.size else np.zeros(1, a.dtype)
    return tuple(formats.to_device(some(np.ascontiguousarray(a))) for a in arrays)


def _unchanged(device, host):
    return all(d.cpu().numpy().reshape(-1).view(np.uint8)[:h.nbytes].tobytes() == h.tobytes() for d, h in zip(device, host))


def _filled(a):
    """A guarded device array that holds `a`."""
    import torch
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    g = _Guarded(raw.size)
    if raw.size:
        g.buf[g.first:g.first + raw.size].copy_(torch.from_numpy(raw.copy()))
    return g


def _omega(dtype):
    return 1.2 - 0.1j if np.dtype(dtype).kind == "c" else 1.2


def _plan(gpu, n, colours, d_order, d_colour_ptr, d_colour_of, d_ptr, d_col, base):
    """One Plan between guards and sentinels -> (status, entries, diagPos as _Guarded, colourPtrHost with its sentinels)."""
    import torch
    from spgpu_amd import capi
    work = _Guarded(capi.spgpuCsrSweepWorkBytes(n), 192)                       # 256-byte aligned
    diag_pos = _Guarded(n * 4)
    host = np.full(colours + 1 + 9, SENTINEL, np.int32)                        # [4 | entries | colourPtrHost | 4]
    entries_at = host[4:].ctypes.data_as(C.POINTER(C.c_int))
    ptr_at = host[5:].ctypes.data_as(C.POINTER(C.c_int))
    torch.cuda.synchronize()
    st = capi.spgpuCsrSweepPlanDevice(gpu, entries_at, diag_pos.ptr(), ptr_at, n, colours, _p(d_order), _p(d_colour_ptr), _p(d_colour_of),
                                      _p(d_ptr), _p(d_col), base, work.ptr())
    torch.cuda.synchronize()
    assert work.guards_intact() and diag_pos.guards_intact()
    assert (host[:4] == SENTINEL).all() and (host[5 + colours + 1:] == SENTINEL).all()
    return st, int(host[4]), diag_pos, host


def _sweep(gpu, run, x0, d_b, n, colours, d_order, host_ptr, diag_pos, d_mat, base, direction, omega, dtype, entries):
    """One sweep on a guarded copy of x0 -> the bytes of x."""
    import torch
    from spgpu_amd import capi
    dtype = np.dtype(dtype)
    x = _filled(x0)
    w = None if omega is None else np.array([omega], dtype)
    args = (gpu, x.ptr(), _p(d_b), n, colours, _p(d_order), host_ptr.ctypes.data_as(C.POINTER(C.c_int)), diag_pos.ptr(), _p(d_mat[0]),
            _p(d_mat[1]), _p(d_mat[2]), base, direction, None if w is None else C.c_void_p(w.ctypes.data), capi.TYPE_CODE[CODE[dtype]],
            entries)
    st = capi.spgpuCsrSweepDevice(*args) if run is None else capi.spgpuCsrSweepDeviceWith(*args, *run)
    assert st == capi.SPGPU_SUCCESS, (run, direction, omega)
    torch.cuda.synchronize()
    assert x.guards_intact(), (run, direction, omega)
    return x.numpy(np.uint8).tobytes()


def _residual(gpu, run, d_b, d_x, n, d_mat, base, dtype, entries, in_place=None):
    """One residual into a poisoned guarded r, or in place on a guarded copy of b -> the bytes of r."""
    import torch
    from spgpu_amd import capi
    dtype = np.dtype(dtype)
    r = _filled(in_place) if in_place is not None else _Guarded(n * dtype.itemsize)
    args = (gpu, r.ptr(), r.ptr() if in_place is not None else _p(d_b), _p(d_x), n, _p(d_mat[0]), _p(d_mat[1]), _p(d_mat[2]), base,
            capi.TYPE_CODE[CODE[dtype]], entries)
    st = capi.spgpuCsrResidualDevice(*args) if run is None else capi.spgpuCsrResidualDeviceWith(*args, run[0], run[2])
    assert st == capi.SPGPU_SUCCESS, run
    torch.cuda.synchronize()
    assert r.guards_intact(), run
    return r.numpy(np.uint8).tobytes()


def _check_matrix(gpu, mat, base, dtype, colours, colour_of, order, colour_ptr, runs=_RUNS):
    """Plan, sweeps and residual of one matrix against formats; order None: the matrix is in colour order."""
    from spgpu_amd import capi, formats
    ptr, col, vals = mat
    n = ptr.size - 1
    b, x0 = K.vectors(n, dtype, seed=n)
    want_plan = formats.csr_sweep_plan(ptr, col, base, colours, colour_ptr, colour_of, order)
    d_mat = _device(mat)
    d_b, d_x0, d_colour_ptr = _device((b, x0, colour_ptr))
    d_order, d_colour_of = (None, None) if order is None else _device((order, colour_of))
    st, entries, diag_pos, host = _plan(gpu, n, colours, d_order, d_colour_ptr, d_colour_of, d_mat[0], d_mat[1], base)
    assert st == capi.SPGPU_SUCCESS and entries == want_plan[2] == vals.size
    assert diag_pos.numpy(np.int32).tobytes() == want_plan[0].tobytes()
    host_ptr = host[5:5 + colours + 1].copy()
    assert host_ptr.tobytes() == want_plan[1].tobytes()
    for direction in DIRECTIONS:
        for omega in (None, _omega(dtype)):
            want = formats.csr_sweep(ptr, col, vals, b, x0, base, colours, want_plan[1], want_plan[0], order, direction, omega).tobytes()
            for run in runs:
                got = _sweep(gpu, run, x0, d_b, n, colours, d_order, host_ptr, diag_pos, d_mat, base, direction, omega, dtype, entries)
                assert got == want, (str(np.dtype(dtype)), n, base, order is None, direction, omega, run)
    want = formats.csr_residual(ptr, col, vals, b, x0, base).tobytes()
    for run in runs:
        if run is not None and run[1] == CHAINED:
            continue                                                          # the residual has no segments
        assert _residual(gpu, run, d_b, d_x0, n, d_mat, base, dtype, entries) == want, run
        assert _residual(gpu, run, None, d_x0, n, d_mat, base, dtype, entries, in_place=b) == want, run
    assert _unchanged(d_mat + (d_b, d_x0, d_colour_ptr), mat + (b, x0, colour_ptr))
    if order is not None:
        assert _unchanged((d_order, d_colour_of), (order, colour_of))
    assert diag_pos.numpy(np.int32).tobytes() == want_plan[0].tobytes()


# ---- 1. every case, every type: A with its order, and the permuted matrix without one --------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("name", NAMES)
def test_every_run_gives_numpys_bytes(gpu, name, dtype):
    base = 1 if np.dtype(dtype).itemsize in (4, 16) else 0
    rows, mat, colours, colour_of, order, colour_ptr = K.build(name, dtype, base)
    _check_matrix(gpu, mat, base, dtype, colours, colour_of, order, colour_ptr)
    b_mat = from_rows(K.permuted(rows, order), base, dtype)
    _check_matrix(gpu, b_mat, base, dtype, colours, None, None, colour_ptr, runs=[None, (1, CHAINED, 0), (8, PLAIN, 1), (32, CHAINED, 1)])


def test_the_cases_are_what_their_names_say():
    from spgpu_amd import capi
    sizes = lambda name: np.diff(K.build(name)[5]).tolist()
    assert sizes("diagonal") == [6] and sizes("chain5") == [3, 2] and sizes("tridiagonal600") == [300, 300]
    assert sizes("mixed") == [3, 2, 300, 300, 4, 3] and 300 > capi.SWEEP_CHAIN_WIDTH >= 4
    assert np.diff(K.build("hubs")[1][0])[:4].tolist() == [8, 9, 32, 33] and np.diff(K.build("arrow20")[1][0])[0] == 20
    ptr, col, _ = K.build("twice")[1]
    assert sorted(col[ptr[2]:ptr[3]].tolist()) == [1, 1, 2, 3]
    host = (C.c_int * 7)(*K.build("mixed")[5].tolist())
    assert capi.csr_sweep_launches(host, 6, capi.SWEEP_FORWARD, CHAINED) == 4 and capi.csr_sweep_launches(host, 6, capi.SWEEP_SYMMETRIC, PLAIN) == 12


def test_more_colours_than_one_chained_launch_walks(gpu):
    """A chain of 140 rows with colour = row mod 70: 70 narrow colours, so a chained sweep is two launches in each direction."""
    from spgpu_amd import capi
    rows, _ = K.chain(140)
    colour = [i % 70 for i in range(140)]
    assert 70 > capi.SWEEP_CHAIN_PASSES
    rows = K._values(rows, 7, np.float64)
    colour_of = np.array(colour, np.int32)
    order = np.array(sorted(range(140), key=lambda i: (colour[i], i)), np.int32)
    colour_ptr = np.arange(0, 142, 2, dtype=np.int32)
    _check_matrix(gpu, from_rows(rows, 0), 0, np.float64, 70, colour_of, order, colour_ptr, runs=[None, (1, CHAINED, 0), (8, CHAINED, 0), (1, PLAIN, 0)])


# ---- 2. degenerate sizes ---------------------------------------------------------------------------------------------------
def test_no_rows_and_no_colours_touch_nothing(gpu):
    from spgpu_amd import capi
    x = _Guarded(64)
    entries = C.c_int(77)
    assert capi.spgpuCsrSweepPlanDevice(gpu, C.byref(entries), None, None, 0, 3, None, None, None, None, None, 0, None) == capi.SPGPU_SUCCESS
    assert entries.value == 0
    for rows, colours in ((0, 3), (5, 0), (-1, -1)):
        assert capi.spgpuCsrSweepDevice(gpu, x.ptr(), x.ptr(), rows, colours, None, None, None, None, None, None, 0, capi.SWEEP_FORWARD, None,
                                        capi.TYPE_DOUBLE, 0) == capi.SPGPU_SUCCESS
    assert capi.spgpuCsrResidualDevice(gpu, x.ptr(), x.ptr(), x.ptr(), 0, None, None, None, 0, capi.TYPE_DOUBLE, 0) == capi.SPGPU_SUCCESS
    assert x.untouched()


@pytest.mark.parametrize("dtype", TYPES)
def test_the_residual_of_an_empty_row_and_of_a_matrix_without_entries(gpu, dtype):
    """Row 1 stores nothing, so r_1 = b_1 with its bits (-0.0); and four rows with nothing stored at all, entriesCount 0: r = b."""
    rows, _ = K.empty_row_case()
    from spgpu_amd import formats
    mat = from_rows(rows, 1, dtype)
    b, x = K.vectors(4, dtype)
    b[1] = -0.0
    want = formats.csr_residual(*mat, b, x, 1).tobytes()
    d_mat, (d_b, d_x) = _device(mat), _device((b, x))
    for run in [None] + [(shape, PLAIN, cap) for shape in SHAPES for cap in (0, 1)]:
        assert _residual(gpu, run, d_b, d_x, 4, d_mat, 1, dtype, mat[2].size) == want
        assert _residual(gpu, run, None, d_x, 4, d_mat, 1, dtype, mat[2].size, in_place=b) == want
    nothing = (np.ones(5, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype))
    d_nothing = _device(nothing)
    for entries in (0, -3):
        assert _residual(gpu, None, d_b, d_x, 4, d_nothing, 1, dtype, entries) == b.tobytes()


# ---- 3. the refusals -------------------------------------------------------------------------------------------------------
def _refused(gpu, rows, colour, base, order_given=True, colours=2, colour_ptr=None):
    from spgpu_amd import capi, formats
    ptr, col, _ = from_rows(rows, base)
    n = len(rows)
    colour_of = np.array(colour, np.int32)
    order = np.array(sorted(range(n), key=lambda i: (colour[i], i)), np.int32)
    if colour_ptr is None:
        colour_ptr = np.array([int((colour_of < c).sum()) for c in range(colours + 1)], np.int32)
    with pytest.raises(ValueError):
        formats.csr_sweep_plan(ptr, col, base, colours, colour_ptr, colour_of, order if order_given else None)
    d_ptr, d_col, d_of, d_order, d_cp = _device((ptr, col, colour_of, order, colour_ptr))
    st, entries, _, _ = _plan(gpu, n, colours, d_order if order_given else None, d_cp, d_of if order_given else None, d_ptr, d_col, base)
    assert (st, entries) == (capi.SPGPU_UNSUPPORTED, 0)


@pytest.mark.parametrize("base", [0, 1])
def test_the_plan_refuses_each_bad_input(gpu, base):
    """SPGPU_UNSUPPORTED with *entriesCount = 0, guards and sentinels intact (_plan): nothing is read or written out of bounds."""
    for what, rows, colour in K.refusals():
        _refused(gpu, rows, colour, base)
    rows, colour = K.chain(6)
    for bad_column in (-1, 2 ** 31 - 1 - base, 6):
        bad = [list(r) for r in rows]
        bad[5] = [(4, 1.0), (5, 1.0), (bad_column, 1.0)]
        _refused(gpu, bad, colour, base)
    for bad_colour in (-1, 2, 2 ** 30):
        _refused(gpu, rows, colour[:3] + [bad_colour] + colour[4:], base, colour_ptr=np.array([0, 3, 6], np.int32))
    _refused(gpu, rows, colour, base, order_given=False)                      # the chain in its natural order is not in colour order
    for bad_ptr in ([1, 3, 6], [0, 4, 3], [0, 3, 5], [0, 3, 7]):
        _refused(gpu, rows, colour, base, colour_ptr=np.array(bad_ptr, np.int32))


def test_an_unsymmetric_pattern_that_the_colouring_accepts_and_the_plan_refuses(gpu):
    """Row 1 stores (1, 0) and row 0 does not store (0, 1): spgpuCsrColourDevice gives both nodes colour 0, and the Plan refuses
    the stored entry between them.  With the colouring of the pattern of A + A^T the Plan accepts A."""
    import torch
    from spgpu_amd import capi, formats
    rows = K.unsymmetric_pair()
    ptr, col, vals = from_rows(rows, 0)
    d_ptr, d_col = _device((ptr, col))
    work = torch.zeros(capi.spgpuCsrColourWorkBytes(2), dtype=torch.uint8, device="cuda:0")
    d_of, d_order, d_inverse, d_cp = (torch.zeros(k, dtype=torch.int32, device="cuda:0") for k in (2, 2, 2, 3))
    colours, rounds = C.c_int(0), C.c_int(0)
    assert capi.spgpuCsrColourDevice(gpu, C.byref(colours), C.byref(rounds), _p(d_of), 2, _p(d_ptr), _p(d_col), 0, _p(work)) == capi.SPGPU_SUCCESS
    assert colours.value == 1 and d_of.cpu().tolist() == [0, 0]
    assert capi.spgpuCsrColourOrderDevice(gpu, _p(d_order), _p(d_inverse), _p(d_cp), 2, 1, _p(d_of), _p(work)) == capi.SPGPU_SUCCESS
    st, entries, _, _ = _plan(gpu, 2, 1, d_order, d_cp, d_of, d_ptr, d_col, 0)
    assert (st, entries) == (capi.SPGPU_UNSUPPORTED, 0)
    sym_ptr, sym_col, _ = from_rows([[(0, 1.0), (1, 1.0)], [(1, 1.0), (0, 1.0)]], 0)
    colours, _, colour_of = formats.csr_colour(sym_ptr, sym_col, 0)
    order, _, colour_ptr = formats.csr_colour_order(colour_of, colours)
    _check_matrix(gpu, (ptr, col, vals), 0, np.float64, colours, colour_of, order, colour_ptr, runs=[None, (8, PLAIN, 0)])


def test_what_the_sweep_cannot_do_is_refused_before_a_launch(gpu):
    from spgpu_amd import capi
    x = _Guarded(64)
    at = x.ptr()
    host = (C.c_int * 3)(0, 3, 5)
    def sweep(direction=capi.SWEEP_FORWARD, code=capi.TYPE_DOUBLE, host_ptr=host, run=(1, PLAIN, 0), **missing):
        a = {k: missing.get(k, at) for k in ("x", "b", "diag", "ptr", "col", "val")}
        return capi.spgpuCsrSweepDeviceWith(gpu, a["x"], a["b"], 5, 2, None, host_ptr, a["diag"], a["ptr"], a["col"], a["val"], 0, direction, None,
                                            code, 13, *run)
    for bad in (sweep(direction=3), sweep(direction=-1), sweep(code=capi.TYPE_INT), sweep(code=7), sweep(host_ptr=None), sweep(x=None),
                sweep(b=None), sweep(diag=None), sweep(ptr=None), sweep(col=None), sweep(val=None), sweep(run=(3, PLAIN, 0)),
                sweep(run=(128, PLAIN, 0)), sweep(run=(1, 2, 0)), sweep(host_ptr=(C.c_int * 3)(0, 3, 6)), sweep(host_ptr=(C.c_int * 3)(0, 6, 5)),
                sweep(host_ptr=(C.c_int * 3)(1, 3, 5))):
        assert bad == capi.SPGPU_UNSUPPORTED
    def residual(code=capi.TYPE_DOUBLE, shape=1, **missing):
        a = {k: missing.get(k, at) for k in ("r", "b", "x", "ptr", "col", "val")}
        return capi.spgpuCsrResidualDeviceWith(gpu, a["r"], a["b"], a["x"], 5, a["ptr"], a["col"], a["val"], 0, code, 13, shape, 0)
    for bad in (residual(code=capi.TYPE_INT), residual(code=9), residual(shape=3), residual(r=None), residual(b=None), residual(x=None),
                residual(ptr=None), residual(col=None), residual(val=None)):
        assert bad == capi.SPGPU_UNSUPPORTED
    assert x.untouched()


# ---- 4. a symmetric sweep and a residual in one captured graph ------------------------------------------------------------------
def test_a_sweep_and_a_residual_replay_from_one_captured_graph(gpu):
    """spgpuCsrSweepDevice (SYMMETRIC, with omega) and spgpuCsrResidualDevice captured on the handle's stream and replayed after b,
    x and values changed in place: each replay gives the bytes of numpy's restatement on the data of the moment.  The sweep reads
    colourPtrHost and *omega at capture time: both are overwritten before the replays."""
    import torch
    from spgpu_amd import capi, formats
    base, dtype = 1, np.float64
    rows, (ptr, col, vals), colours, colour_of, order, colour_ptr = K.build("mixed", dtype, base)
    n, nnz = len(rows), vals.size
    diag_want, cp, entries = formats.csr_sweep_plan(ptr, col, base, colours, colour_ptr, colour_of, order)
    d_ptr, d_col, d_order, d_of, d_cp = _device((ptr, col, order, colour_of, colour_ptr))
    st, got_entries, diag_pos, host = _plan(gpu, n, colours, d_order, d_cp, d_of, d_ptr, d_col, base)
    assert st == capi.SPGPU_SUCCESS and got_entries == entries
    host_ptr = host[5:5 + colours + 1].copy()
    d_vals, d_b, d_x, d_r = (torch.zeros(k, dtype=torch.float64, device="cuda:0") for k in (nnz, n, n, n))
    omega = np.array([1.2])
    side_stream = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side_stream.cuda_stream))
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side_stream):
            assert capi.spgpuCsrSweepDevice(gpu, _p(d_x), _p(d_b), n, colours, _p(d_order), host_ptr.ctypes.data_as(C.POINTER(C.c_int)),
                                            diag_pos.ptr(), _p(d_ptr), _p(d_col), _p(d_vals), base, capi.SWEEP_SYMMETRIC,
                                            C.c_void_p(omega.ctypes.data), capi.TYPE_DOUBLE, entries) == capi.SPGPU_SUCCESS
            assert capi.spgpuCsrResidualDevice(gpu, _p(d_r), _p(d_b), _p(d_x), n, _p(d_ptr), _p(d_col), _p(d_vals), base, capi.TYPE_DOUBLE,
                                               entries) == capi.SPGPU_SUCCESS
        host_ptr[:] = 0
        omega[0] = 7.0
        seen = set()
        for seed in (1, 2):
            new_vals = from_rows(K._values(rows, 900 + seed, dtype), base, dtype)[2]
            b, x0 = K.vectors(n, dtype, seed=seed)
            want_x = formats.csr_sweep(ptr, col, new_vals, b, x0, base, colours, cp, diag_want, order, capi.SWEEP_SYMMETRIC, 1.2)
            want_r = formats.csr_residual(ptr, col, new_vals, b, want_x, base)
            seen.add(want_x.tobytes())
            for d, h in ((d_vals, new_vals), (d_b, b), (d_x, x0)):
                d.copy_(formats.to_device(h))
            d_r.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert d_x.cpu().numpy().tobytes() == want_x.tobytes() and d_r.cpu().numpy().tobytes() == want_r.tobytes()
        assert len(seen) == 2
    finally:
        capi.spgpuSetStream(gpu, None)
