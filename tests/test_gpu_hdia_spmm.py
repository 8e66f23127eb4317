"""GPU: spgpu?hdiaspmmMv and spgpu?diaspmmMv (include/spgpu/ext/hdia_spmm.h) on all sixteen instantiations of hdiaSpmmMvKernel their
dispatch can choose (hdia_spmm.hip:229-274), with wideIO on and off, on every composition of passes, and through count == 1, which is
the SpMV.  The constants, the dispatch restated and the case table are in tests/hdia_spmm_launch_shapes.py; the matrices are the
hand-built, NaN-poisoned ones of tests/hdia_launch_shapes.py; tests/test_hdia_spmm_launch_shapes.py checks on the CPU that the table
reaches what it is there for.

Every multivector lies in a buffer with 16 bytes in front and an element and 16 bytes behind; between the vectors, in front and
behind, X and Y hold NaN and Z a sentinel.  Before it launches, a case asserts that the restated dispatch returns the passes it is
there for.  Every call is checked four ways: (a) the bytes of spgpu?hdiaspmv / spgpu?diaspmv run on the GPU vector by vector on the
same device arrays; (b) the oracle's bytes per vector; (c) exact_ref.spmv on the matrix' COO triplets per vector within
exact_ref.TOL -- the evidence that does not share the kernel's order; (d) the gaps of Z, and all of X, Y and dM, unchanged bit for
bit."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import hdia_launch_shapes as H
import hdia_spmm_launch_shapes as M
import oracle_api as O
from test_gpu_hdia_shapes import SENTINEL, _Buf, _ints

pytestmark = pytest.mark.gpu
RAN = set()   # node ids of the tests of this file that were run (test_zz_no_case_was_skipped)

_IDS = [(L, cid) for L in M.LETTERS for cid in M.cases(L)]
_TABLE = {L: M.cases(L) for L in M.LETTERS}


@pytest.fixture(autouse=True)
def _ran(request):
    """A test skipped by a mark or a condition is never set up, so it never gets here; no test of this file skips itself."""
    RAN.add(request.node.nodeid)
    yield


class _MvBuf:
    """`vectors` (count arrays of n elements) at stride `pitch` inside one device buffer: WIDE elements (16 bytes) in front, the
    first vector `shift` elements (0 or 1) behind them, an element and WIDE more behind the LAST VECTOR'S END (not behind its
    pitch); everything that is not a vector's body holds `gap`."""

    def __init__(self, vectors, pitch, shift=0, gap=np.nan):
        import torch
        n, dtype = vectors[0].size, vectors[0].dtype
        assert pitch >= n
        letter = O.LETTER_OF[dtype]
        front = H.WIDE[letter] + int(shift)
        host = np.full(front + (len(vectors) - 1) * pitch + n + 1 + H.WIDE[letter], gap, dtype=dtype)
        self.inside = np.zeros(host.size, bool)
        for j, v in enumerate(vectors):
            host[front + j * pitch:front + j * pitch + n] = v
            self.inside[front + j * pitch:front + j * pitch + n] = True
        self.front, self.n, self.pitch, self.count, self.before = front, n, pitch, len(vectors), host.copy()
        self.dev = torch.from_numpy(host).to("cuda:0")
        assert self.dev.data_ptr() % 16 == 0

    @property
    def address(self):
        return self.dev.data_ptr() + self.front * self.dev.element_size()

    @property
    def ptr(self):
        return C.c_void_p(self.address)

    def vector_ptr(self, j):
        return C.c_void_p(self.address + j * self.pitch * self.dev.element_size())

    def bodies(self):
        """[count, n] on the host; asserts that nothing between, in front of or behind the vectors changed, bit for bit."""
        host = self.dev.cpu().numpy()
        assert host[~self.inside].tobytes() == self.before[~self.inside].tobytes(), "elements outside the vectors were written"
        return np.stack([host[self.front + j * self.pitch:self.front + j * self.pitch + self.n] for j in range(self.count)])

    def assert_unchanged(self, what):
        assert self.dev.cpu().numpy().tobytes() == self.before.tobytes(), f"{what} was written"


_DEV, _REF = {}, {}


def _dev_matrix(case):
    """(dM buffer, offsets, hackOffsets or None) of a case's matrix in HBM; dM one element late where the case says so."""
    key = (M.matrix_key(case), "dM" in case["shift"])
    if key not in _DEV:
        m = M.matrix_of(case)
        _DEV[key] = (_Buf(m["values"], "dM" in case["shift"]), _ints(m["offsets"]),
                     _ints(m["hack_offsets"]) if case["fmt"] == "hdia" else None)
    return _DEV[key]


def _reference(case, j, alpha, beta):
    """(oracle's z, exact z*, scale) of vector j of one (matrix, alpha, beta): computed once, shared, left unchanged."""
    key = (M.matrix_key(case), j, alpha, beta)
    if key not in _REF:
        rows, cols = case["shape"]
        m = M.matrix_of(case)
        x, y = M.operands(case["letter"], rows, cols, j)
        y = y if beta != 0 else None
        oracle = (O.hdia_spmv if case["fmt"] == "hdia" else O.dia_spmv)(m, x, y, alpha, beta)
        r, c, v = m["coo"]
        _REF[key] = (oracle,) + tuple(X.spmv(rows, r, c, v, x, y, alpha, beta))
    return _REF[key]


def _spmm(gpu, case, m, dM, offs, hack_offsets, z, y_ptr, alpha, x, beta, count, pitch_x, pitch_yz):
    from spgpu_amd import capi
    L = case["letter"]
    if case["fmt"] == "hdia":
        capi.hdiaspmm_mv[L](gpu, z.ptr, y_ptr, capi.scalar(L, alpha), dM.ptr, C.c_void_p(offs.data_ptr()), m["hack_size"],
                            C.c_void_p(hack_offsets.data_ptr()), m["rows"], m["cols"], x.ptr, capi.scalar(L, beta), count, pitch_x,
                            pitch_yz)
    else:
        capi.diaspmm_mv[L](gpu, z.ptr, y_ptr, capi.scalar(L, alpha), dM.ptr, C.c_void_p(offs.data_ptr()), m["pitch"], m["rows"],
                           m["cols"], m["diags"], x.ptr, capi.scalar(L, beta), count, pitch_x, pitch_yz)


def _spmv(gpu, case, m, dM, offs, hack_offsets, z_ptr, y_ptr, alpha, x_ptr, beta):
    from spgpu_amd import capi
    L = case["letter"]
    if case["fmt"] == "hdia":
        capi.hdiaspmv[L](gpu, z_ptr, y_ptr, capi.scalar(L, alpha), dM.ptr, C.c_void_p(offs.data_ptr()), m["hack_size"],
                         C.c_void_p(hack_offsets.data_ptr()), m["rows"], m["cols"], x_ptr, capi.scalar(L, beta))
    else:
        capi.diaspmv[L](gpu, z_ptr, y_ptr, capi.scalar(L, alpha), dM.ptr, C.c_void_p(offs.data_ptr()), m["pitch"], m["rows"],
                        m["cols"], m["diags"], x_ptr, capi.scalar(L, beta))


def _operands(case):
    """(X buffer, make_zy): make_zy() gives a fresh (Z buffer, Y buffer or None); Z is Y where the case says so."""
    letter, (rows, cols), count = case["letter"], case["shape"], case["count"]
    pitch_x, pitch_yz = M.pitch_of(letter, case["pitch"], cols), M.pitch_of(letter, case["pitch"], rows)
    hosts = [M.operands(letter, rows, cols, j) for j in range(count)]
    x = _MvBuf([h[0] for h in hosts], pitch_x, "x" in case["shift"])
    mode = case["y_mode"]

    def make_zy():
        if mode == "z":
            z = _MvBuf([h[1] for h in hosts], pitch_yz, "z" in case["shift"], gap=SENTINEL)
            return z, z
        z = _MvBuf([np.full(rows, np.nan, hosts[0][1].dtype)] * count, pitch_yz, "z" in case["shift"], gap=SENTINEL)
        if mode == "null":
            return z, None
        return z, _MvBuf([np.full_like(h[1], np.nan) if mode == "nan" else h[1] for h in hosts], pitch_yz, "y" in case["shift"])

    return x, make_zy, pitch_x, pitch_yz


def _assert_dispatch(case, dM, x, z, y, pitch_yz):
    """The addresses about to be passed select the passes the case is in the table for."""
    off = dict(dM=dM.address % 16, z=z.address % 16, y=y.address % 16 if y is not None else 0, x=x.address % 16)
    assert off == M.offsets_of(case)
    got = tuple(M.dispatch(case["letter"], case["hp"], off, pitch_yz, case["count"], y is not None))
    assert got == case["want"], "the arguments of this case select other passes"


def _run(gpu, case):
    """One call of `case`, checked four ways: returns Z's vectors' bytes."""
    import torch
    letter, count = case["letter"], case["count"]
    m = M.matrix_of(case)
    dM, offs, hack_offsets = _dev_matrix(case)
    alpha, beta = case["scalars"]
    x, make_zy, pitch_x, pitch_yz = _operands(case)
    z, y = make_zy()
    _assert_dispatch(case, dM, x, z, y, pitch_yz)
    assert (beta != 0) == (case["y_mode"] in ("y", "z"))
    # (a)'s reference first: the SpMV, vector by vector, on the same X (and dM), into a twin of Z (and of Y where Z is Y)
    z1, y1 = make_zy()
    for j in range(count):
        _spmv(gpu, case, m, dM, offs, hack_offsets, z1.vector_ptr(j), y1.vector_ptr(j) if y1 is not None else None, alpha,
              x.vector_ptr(j), beta)
    _spmm(gpu, case, m, dM, offs, hack_offsets, z, y.ptr if y is not None else None, alpha, x, beta, count, pitch_x, pitch_yz)
    torch.cuda.synchronize()
    got, one_by_one = z.bodies(), z1.bodies()          # (d) the gaps of Z
    x.assert_unchanged("X")                            # (d)
    if y is not None and y is not z:
        y.assert_unchanged("Y")
    assert dM.body().tobytes() == m["values"].tobytes()
    for j in range(count):
        assert got[j].tobytes() == one_by_one[j].tobytes(), (case["id"], "vector", j, "differs from the SpMV on the GPU",
                                                             int(np.flatnonzero(got[j] != one_by_one[j])[0]))     # (a)
        oracle, want, scale = _reference(case, j, alpha, beta)
        assert got[j].tobytes() == oracle.tobytes(), (case["id"], "vector", j, "oracle", int(np.flatnonzero(got[j] != oracle)[0]))  # (b)
        X.assert_within(got[j], want, scale, letter, (case["id"], j, alpha, beta))                                # (c)
    return got.tobytes()


@pytest.mark.parametrize("letter,cid", _IDS, ids=[f"{L}-{cid}" for L, cid in _IDS])
def test_case(gpu, letter, cid):
    """Every row of the case table (hdia_spmm_launch_shapes.cases)."""
    _run(gpu, _TABLE[letter][cid])


@pytest.mark.parametrize("letter", M.LETTERS)
def test_same_bytes_at_every_pitch_and_placement(gpu, letter):
    """One matrix, one (alpha, beta), 2 V + 3 vectors: the wide kernels with pack stores and with element stores, the narrow ones,
    every pitch and every array off its boundary in turn."""
    first, routes = None, set()
    for shift, pitch in (("aligned", "tight"), ("aligned", "rounded"), ("aligned", "rounded+5"), ("dM-shifted", "tight"),
                         ("z-shifted", "rounded"), ("y-shifted", "rounded"), ("x-shifted", "rounded")):
        cid = f"hdia-cycle-h32-{shift}-{pitch}-with-y-n{2 * M.MAX_V + 3}"
        case = _TABLE[letter].get(cid) or M._case(cid, "hdia", letter, (H.N, H.N), "cycle", 32, True, shift, pitch, "with-y", 2 * M.MAX_V + 3)
        got = _run(gpu, case)
        routes.add(case["want"][0][0::2])
        first = got if first is None else first
        assert got == first, (letter, shift, pitch)
    assert routes == {(M.WIDE[letter], 1), (M.WIDE[letter], 0), (1, 1)}


def test_a_captured_call_replays_the_eager_bytes(gpu):
    """D, hack 32, V + 1 vectors, beta != 0: captured on a side stream (one stream, no parallel branches), replayed twice."""
    import torch
    from spgpu_amd import capi
    case = _TABLE["D"][f"hdia-cycle-h32-aligned-rounded-with-y-n{M.MAX_V + 1}"]
    assert case["scalars"][1] != 0
    eager = _run(gpu, case)
    m = M.matrix_of(case)
    dM, offs, hack_offsets = _dev_matrix(case)
    alpha, beta = case["scalars"]
    x, make_zy, pitch_x, pitch_yz = _operands(case)
    z, y = make_zy()
    side = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()   # the buffers above were written on torch's stream; `side` does not wait for it by itself

    def call():
        _spmm(gpu, case, m, dM, offs, hack_offsets, z, y.ptr, alpha, x, beta, case["count"], pitch_x, pitch_yz)

    try:
        with torch.cuda.stream(side):
            call()                           # warm-up outside the capture (module load)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call()
        for replay in range(2):
            z.dev.copy_(torch.from_numpy(z.before))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert z.bodies().tobytes() == eager, replay
    finally:
        capi.spgpuSetStream(gpu, None)
    x.assert_unchanged("X")
    y.assert_unchanged("Y")


@pytest.mark.parametrize("letter", M.LETTERS)
def test_degenerate_calls_write_nothing(gpu, letter):
    """rows == 0, count == 0 and hackSize == 0 (dMPitch == 0) write nothing."""
    import torch
    case = _TABLE[letter][f"hdia-all-300x3-h4-aligned-tight-with-y-n2"]
    m = M.matrix_of(case)
    dM, offs, hack_offsets = _dev_matrix(case)
    x, make_zy, pitch_x, pitch_yz = _operands(case)
    z, y = make_zy()
    for rows, hack, count in ((0, 4, 2), (300, 0, 2), (300, 4, 0), (300, 4, -1)):
        mm = dict(m, rows=rows, hack_size=hack, pitch=hack, diags=1)
        for fmt in ("hdia", "dia"):
            _spmm(gpu, dict(case, fmt=fmt), mm, dM, offs, hack_offsets, z, y.ptr, 2.0, x, 0.5, count, pitch_x, pitch_yz)
    torch.cuda.synchronize()
    z.assert_unchanged("Z")


def test_zz_no_case_was_skipped(request):
    """Every case above is mandatory.  This test is the last of the file: of the tests of this file selected for the run, each
    one before it must have been run (a failed one has; a skipped one has not)."""
    mine = [item.nodeid for item in request.session.items
            if item.fspath == request.node.fspath and item.nodeid != request.node.nodeid]
    skipped = [nodeid for nodeid in mine if nodeid not in RAN]
    assert not skipped, skipped
    if not request.config.getoption("keyword") and not any("::" in arg for arg in request.config.args):
        assert len(mine) == len(_IDS) + 2 + 1 + 2, len(mine)
