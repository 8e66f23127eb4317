"""GPU: spgpu?hdiaspmv and spgpu?diaspmv on all seven instantiations of hdiaSpmvKernel their dispatch can choose
(hdia_spmv.hip:231-244), with wideIO on and off, and on the wave-uniform and per-lane branches inside the kernel that no argument
names: wavefronts that leave, dead lanes, hacks without diagonals, stages fetched whole or guarded, the ring of stages turning
twice, lanes of one wavefront with different counts, x as one 16-byte load (at an aligned and at an odd address) or as element
loads (an edge, or fewer columns than a strip has rows), wide and element stores, every mask of a slot.  The constants, the
dispatch and the kernel's control flow restated, the hand-built NaN-poisoned matrices and the case table are in
tests/hdia_launch_shapes.py; tests/test_hdia_launch_shapes.py checks on the CPU that every case takes the branches it is there for.

Every array lies in a buffer with 16 bytes in front and an element and 16 bytes behind, so that a case can pass it one element past
a 16-byte boundary; before it launches, a case computes the offsets of the addresses it is about to pass and asserts that the
restated dispatch returns the (RPL, wideIO) it is there for.  Every call is checked against the long-double sum of the matrix' COO
triplets within exact_ref.TOL, against the oracle's bytes (a row's products are added in ascending stored diagonal whatever the
launch shape), and on the sentinels in front of and behind z."""
import ctypes as C
import zlib

import numpy as np
import pytest

import exact_ref as X
import hdia_launch_shapes as H
import oracle_api as O
from test_gpu_fuzz import _complex_scalars

pytestmark = pytest.mark.gpu
RAN = set()   # node ids of the tests of this file that were run (test_zz_no_case_was_skipped)
SENTINEL = -12345.5

_IDS = [(L, cid) for L in "SDCZ" for cid in H.cases(L)]
_TABLE = {L: H.cases(L) for L in "SDCZ"}


@pytest.fixture(autouse=True)
def _ran(request):
    """A test skipped by a mark or a condition is never set up, so it never gets here; no test of this file skips itself."""
    RAN.add(request.node.nodeid)
    yield


class _Buf:
    """`body` inside one device buffer: WIDE elements (16 bytes) in front, the body `shift` elements (0 or 1) behind them, an
    element and WIDE more behind it; everything that is not body holds `gap`."""

    def __init__(self, body, shift=0, gap=np.nan):
        import torch
        letter = O.LETTER_OF[body.dtype]
        front = H.WIDE[letter] + int(shift)
        host = np.full(front + body.size + 1 + H.WIDE[letter], gap, dtype=body.dtype)
        host[front:front + body.size] = body
        self.front, self.n, self.before = front, body.size, host.copy()
        self.dev = torch.from_numpy(host).to("cuda:0")
        assert self.dev.data_ptr() % 16 == 0

    @property
    def address(self):
        return self.dev.data_ptr() + self.front * self.dev.element_size()

    @property
    def ptr(self):
        return C.c_void_p(self.address)

    def body(self):
        """The body on the host; asserts that nothing around it changed, bit for bit."""
        host = self.dev.cpu().numpy()
        lo, hi = self.front, self.front + self.n
        assert host[:lo].tobytes() == self.before[:lo].tobytes(), "elements in front of the array were written"
        assert host[hi:].tobytes() == self.before[hi:].tobytes(), "elements behind the array were written"
        return host[lo:hi].copy()


_DEV, _REF = {}, {}


def _ints(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to("cuda:0")


def _dev_matrix(case):
    """(dM buffer, offsets, hackOffsets or None) of a case's matrix in HBM; dM one element late where the case says so."""
    key = (H.matrix_key(case), "dM" in case["shift"])
    if key not in _DEV:
        m = H.matrix_of(case)
        _DEV[key] = (_Buf(m["values"], "dM" in case["shift"]), _ints(m["offsets"]),
                     _ints(m["hack_offsets"]) if case["fmt"] == "hdia" else None)
    return _DEV[key]


def _scalars(case):
    return _complex_scalars(zlib.crc32(repr(H.matrix_key(case)).encode()), case["letter"], *case["scalars"])


def _exact(case, alpha, beta):
    """exact_ref.spmv of one (matrix, alpha, beta), computed once and left unchanged."""
    key = (H.matrix_key(case), alpha, beta)
    if key not in _REF:
        rows, cols = case["shape"]
        x, y = H.operands(case["letter"], rows, cols)
        r, c, v = H.matrix_of(case)["coo"]
        _REF[key] = X.spmv(rows, r, c, v, x, y if beta != 0 else None, alpha, beta)
    return _REF[key]


def _call(gpu, case, m, dM, offs, hack_offsets, z, y_ptr, alpha, x, beta):
    from spgpu_amd import capi
    L = case["letter"]
    if case["fmt"] == "hdia":
        capi.hdiaspmv[L](gpu, z.ptr, y_ptr, capi.scalar(L, alpha), dM.ptr, C.c_void_p(offs.data_ptr()), m["hack_size"],
                         C.c_void_p(hack_offsets.data_ptr()), m["rows"], m["cols"], x.ptr, capi.scalar(L, beta))
    else:
        capi.diaspmv[L](gpu, z.ptr, y_ptr, capi.scalar(L, alpha), dM.ptr, C.c_void_p(offs.data_ptr()), m["pitch"], m["rows"],
                        m["cols"], m["diags"], x.ptr, capi.scalar(L, beta))


def _run(gpu, case):
    """One call of `case`, checked: returns z's bytes."""
    import torch
    letter, (rows, cols) = case["letter"], case["shape"]
    m = H.matrix_of(case)
    dM, offs, hack_offsets = _dev_matrix(case)
    alpha, beta = _scalars(case)
    xh, yh = H.operands(letter, rows, cols)
    x = _Buf(xh, "x" in case["shift"])
    mode = case["y_mode"]
    if mode == "z":
        z = _Buf(yh, "z" in case["shift"], gap=SENTINEL)
        y = z
    else:
        z = _Buf(np.full(rows, np.nan, xh.dtype), "z" in case["shift"], gap=SENTINEL)
        y = None if mode == "null" else _Buf(np.full_like(yh, np.nan) if mode == "nan" else yh, "y" in case["shift"])
    off = dict(dM=dM.address % 16, z=z.address % 16, y=y.address % 16 if y is not None else 0, x=x.address % 16)
    assert off == dict(H.offsets_of(letter, case["shift"]), y=off["z"] if mode == "z" else H.offsets_of(letter, case["shift"])["y"])
    assert H.dispatch(letter, case["hp"], off, y is not None) == case["want"], "the arguments of this case select another route"
    assert (beta != 0) == (mode in ("y", "z"))
    _call(gpu, case, m, dM, offs, hack_offsets, z, y.ptr if y is not None else None, alpha, x, beta)
    torch.cuda.synchronize()
    got = z.body()        # checks the sentinels
    assert dM.body().tobytes() == m["values"].tobytes()
    want, scale = _exact(case, alpha, beta)
    X.assert_within(got, want, scale, letter, (case["id"], letter, alpha, beta))
    oracle = (O.hdia_spmv if case["fmt"] == "hdia" else O.dia_spmv)(m, xh, yh if beta != 0 else None, alpha, beta)
    assert got.tobytes() == oracle.tobytes(), (case["id"], letter, "oracle", int(np.flatnonzero(got != oracle)[0]))
    return got.tobytes()


@pytest.mark.parametrize("letter,cid", _IDS, ids=[f"{L}-{cid}" for L, cid in _IDS])
def test_case(gpu, letter, cid):
    """Every row of the case table (hdia_launch_shapes.cases)."""
    _run(gpu, _TABLE[letter][cid])


@pytest.mark.parametrize("prog", ["cycle", "interior", "edge13", "interior8"])
@pytest.mark.parametrize("letter", "SDCZ")
def test_same_bytes_through_every_route(gpu, letter, prog):
    """One matrix, one (alpha, beta), every (RPL, wideIO) the dispatch can return for the letter: the wide kernel with pack stores,
    with element stores (z, then y, off its boundary), the narrow kernel (dM off its boundary), and x off its boundary."""
    stem = f"hdia-{prog}-h32" if prog in ("cycle", "interior") else f"dia-{prog}-alloc"
    routes, first = set(), None
    for kind in ("aligned", "dM-shifted", "z-shifted", "y-shifted", "x-shifted"):
        case = _TABLE[letter][f"{stem}-{kind}"]
        got = _run(gpu, case)
        routes.add(case["want"])
        first = got if first is None else first
        assert got == first, (letter, stem, kind)
    assert routes == ({(1, 1)} if letter == "Z" else {(H.WIDE[letter], 1), (H.WIDE[letter], 0), (1, 1)})


@pytest.mark.parametrize("letter", "SDCZ")
def test_dia_is_hdia_with_one_hack_of_all_rows(gpu, letter):
    """The same arrays through spgpu?diaspmv and through spgpu?hdiaspmv with hackSize = pitch and hackOffsets = {0, diags}: the
    same bytes, at every pitch."""
    import torch
    from spgpu_amd import capi
    for tag in ("alloc", "alloc+32", "rows", "rounded"):
        case = _TABLE[letter][f"dia-edge13-{tag}-aligned"]
        via_dia = _run(gpu, case)
        m = H.matrix_of(case)
        dM, offs, _ = _dev_matrix(case)
        alpha, beta = _scalars(case)
        xh, yh = H.operands(letter, *case["shape"])
        x, y, z = _Buf(xh), _Buf(yh), _Buf(np.full(m["rows"], np.nan, xh.dtype), gap=SENTINEL)
        one = _ints([0, m["diags"]])
        capi.hdiaspmv[letter](gpu, z.ptr, y.ptr, capi.scalar(letter, alpha), dM.ptr, C.c_void_p(offs.data_ptr()), m["pitch"],
                              C.c_void_p(one.data_ptr()), m["rows"], m["cols"], x.ptr, capi.scalar(letter, beta))
        torch.cuda.synchronize()
        assert z.body().tobytes() == via_dia, (letter, tag)


@pytest.mark.parametrize("letter", "SDCZ")
def test_degenerate_calls(gpu, letter):
    """rows == 0 and hackSize == 0 write nothing; DIA without diagonals gives z = beta * y, and zeros for beta == 0."""
    import torch
    from spgpu_amd import capi
    case = _TABLE[letter]["hdia-all-70x70-h4-aligned"]
    m = H.matrix_of(case)
    dM, offs, hack_offsets = _dev_matrix(case)
    xh, yh = H.operands(letter, 70, 70)
    x, y = _Buf(xh), _Buf(yh)
    untouched = np.full(70, SENTINEL, xh.dtype)
    for rows, hack in ((0, 4), (70, 0), (0, 0)):
        z = _Buf(untouched, gap=SENTINEL)
        capi.hdiaspmv[letter](gpu, z.ptr, y.ptr, capi.scalar(letter, 2.0), dM.ptr, C.c_void_p(offs.data_ptr()), hack,
                              C.c_void_p(hack_offsets.data_ptr()), rows, 70, x.ptr, capi.scalar(letter, 0.5))
        capi.diaspmv[letter](gpu, z.ptr, y.ptr, capi.scalar(letter, 2.0), dM.ptr, C.c_void_p(offs.data_ptr()), hack, rows, 70,
                             1, x.ptr, capi.scalar(letter, 0.5))
        torch.cuda.synchronize()
        assert z.body().tobytes() == untouched.tobytes(), (rows, hack)
    for pitch in (H.dia_alloc_pitch(70), 71):
        for beta in _complex_scalars(7, letter, 1.0, 0.5)[1:] + (0.0,):
            z = _Buf(np.full(70, np.nan, xh.dtype), gap=SENTINEL)
            capi.diaspmv[letter](gpu, z.ptr, y.ptr, capi.scalar(letter, 2.0), dM.ptr, C.c_void_p(offs.data_ptr()), pitch, 70, 70,
                                 0, x.ptr, capi.scalar(letter, beta))
            torch.cuda.synchronize()
            got = z.body()
            empty = H.dia_matrix(letter, 70, 70, pitch, [])
            assert got.tobytes() == O.dia_spmv(empty, xh, yh if beta != 0 else None, 2.0, beta).tobytes(), (pitch, beta)
            want, scale = X.spmv(70, [], [], np.zeros(0, xh.dtype), xh, yh, 2.0, beta)
            X.assert_within(got, want, scale, letter, (pitch, beta))
            if beta == 0:
                assert not got.any()


def test_zz_no_case_was_skipped(request):
    """Every case above is mandatory.  This test is the last of the file: of the tests of this file selected for the run, each
    one before it must have been run (a failed one has; a skipped one has not)."""
    mine = [item.nodeid for item in request.session.items
            if item.fspath == request.node.fspath and item.nodeid != request.node.nodeid]
    skipped = [nodeid for nodeid in mine if nodeid not in RAN]
    assert not skipped, skipped
    if not request.config.getoption("keyword") and not any("::" in arg for arg in request.config.args):
        assert len(mine) == len(_IDS) + 4 * 4 + 4 + 4, len(mine)
