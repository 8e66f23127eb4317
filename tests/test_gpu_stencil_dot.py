"""GPU: spgpu?hdiaspmvDotDevice and spgpu?diaspmvDotDevice (include/spgpu/ext/hdia_solver.h, csrc/fused_hdia.hip) on every
instantiation of hdiaSpmvDotKernel their dispatch can choose and on the branches inside the kernel that no argument names.  The
constants, the dispatch and the kernel's control flow restated, the NaN-poisoned matrices and the case table are in
tests/hdia_dot_launch_shapes.py; tests/test_hdia_dot_launch_shapes.py checks on the CPU that every case takes the branches it is
there for.

Every case asserts: z has the bytes spgpu?hdiaspmv / spgpu?diaspmv writes for the same arguments and those of the oracle; *result
has the bytes of spgpu?dotDevice on (w, z) and of spgpu?dot's return value, and agrees with a long-double sum within
rows * eps * sum |w_i z_i|; the integer cases give the integers numpy computes in int64; with beta == 0 y is full of NaN and z is
finite; w == NULL gives the dot with x; the elements around z (a larger buffer filled with a sentinel) are unchanged; z aliased
to y gives the bytes of the out-of-place call.

(The module's name places it behind the GPU modules the suite already had: they run in the order they ran in before it existed.)"""
import ctypes as C

import numpy as np
import pytest

import hdia_dot_launch_shapes as M
import hdia_launch_shapes as H
import oracle_api as O
from test_gpu_hdia_shapes import SENTINEL, _Buf, _ints

pytestmark = pytest.mark.gpu

_IDS = [(L, cid) for L in M.LETTERS for cid in M.cases(L)]
_TABLE = {L: M.cases(L) for L in M.LETTERS}
EPS = {"S": np.finfo(np.float32).eps, "D": np.finfo(np.float64).eps}


def _cell(letter):
    """Four cells of the result type full of NaN; the calls write the second."""
    import torch
    return torch.full((4,), float("nan"), dtype={"S": torch.float32, "D": torch.float64}[letter], device="cuda:0")


def _at(cell, k=1):
    return C.c_void_p(cell.data_ptr() + k * cell.element_size())


def _one(cell, k=1):
    host = cell.cpu().numpy()
    assert np.isnan(host[np.arange(4) != k]).all(), "cells beside the result were written"
    return host[k]


def _matrix_args(case, m, dM, offs, hack_offsets):
    if case["fmt"] == "dia":
        return (dM.ptr, C.c_void_p(offs.data_ptr()), m["pitch"], m["rows"], m["cols"], m["diags"])
    return (dM.ptr, C.c_void_p(offs.data_ptr()), m["hack_size"], C.c_void_p(hack_offsets.data_ptr()), m["rows"], m["cols"])


def _fused(gpu, case, cell, w_ptr, z, y_ptr, alpha, margs, x, beta):
    from spgpu_amd import capi
    L = case["letter"]
    call = capi.diaspmv_dot_device if case["fmt"] == "dia" else capi.hdiaspmv_dot_device
    call[L](gpu, _at(cell), w_ptr, z.ptr, y_ptr, capi.scalar(L, alpha), *margs, x.ptr, capi.scalar(L, beta))


def _plain(gpu, case, z, y_ptr, alpha, margs, x, beta):
    from spgpu_amd import capi
    L = case["letter"]
    call = capi.diaspmv if case["fmt"] == "dia" else capi.hdiaspmv
    call[L](gpu, z.ptr, y_ptr, capi.scalar(L, alpha), *margs, x.ptr, capi.scalar(L, beta))


def _run(gpu, case):
    import torch
    from spgpu_amd import capi
    L, rows, off = case["letter"], case["rows"], case["off"]
    m, xh, wh, yh = M.inputs(case)
    alpha, beta = M.coefficients(case)
    dM = _Buf(m["values"], off["dM"])
    offs = _ints(m["offsets"])
    hack_offsets = None if case["fmt"] == "dia" else _ints(m["hack_offsets"])
    margs = _matrix_args(case, m, dM, offs, hack_offsets)
    x = _Buf(xh, off["x"])
    w = None if wh is None else _Buf(wh, off["w"])
    nan = np.full(rows, np.nan, xh.dtype)
    if case["z_is_y"]:
        z = _Buf(yh, off["z"], gap=SENTINEL)
        y = z
    else:
        z = _Buf(nan, off["z"], gap=SENTINEL)
        y = _Buf(yh if case["beta"] else nan, off["y"])                  # beta == 0: y must not be read
    dot_w = x if w is None else w
    took = M.launch(L, rows, case["hp"], dot_w.address % 16, z.address % 16, dM.address % 16, beta)
    assert took["path"] == case["path"], "the arguments of this case select another path"
    cell = _cell(L)
    _fused(gpu, case, cell, None if w is None else w.ptr, z, y.ptr, alpha, margs, x, beta)
    torch.cuda.synchronize()
    got = z.body()                                                         # checks the sentinels around z
    result = _one(cell)
    assert dM.body().tobytes() == m["values"].tobytes()

    # 1. z: the bytes of the SpMV on the GPU for the same arguments, and of the oracle
    z2 = _Buf(nan, off["z"], gap=SENTINEL)
    y2 = _Buf(yh, off["y"]) if case["z_is_y"] else y
    _plain(gpu, case, z2, y2.ptr, alpha, margs, x, beta)
    torch.cuda.synchronize()
    plain = z2.body()
    assert got.tobytes() == plain.tobytes(), (case["id"], "spmv", int(np.flatnonzero(got != plain)[0]))
    host = m if case["fmt"] == "dia" else dict(m, fmt="hdia")
    oracle = (O.dia_spmv if case["fmt"] == "dia" else O.hdia_spmv)(host, xh, yh if beta != 0 else None, alpha, beta)
    assert got.tobytes() == oracle.tobytes(), (case["id"], "oracle", int(np.flatnonzero(got != oracle)[0]))
    # 5. beta == 0: nothing of the NaN y arrived
    assert np.isfinite(got).all()

    # 2. *result: the bytes of the dot on the stored vectors, device result and host return value
    want = _cell(L)
    capi.dot_device[L](gpu, _at(want), rows, dot_w.ptr, z.ptr)
    returned = capi.dot[L](gpu, rows, dot_w.ptr, z.ptr)
    torch.cuda.synchronize()
    assert np.asarray(result).tobytes() == np.asarray(_one(want)).tobytes(), (case["id"], result, _one(want))
    assert np.asarray(result).tobytes() == np.asarray(returned, dtype=got.dtype).tobytes(), (case["id"], result, returned)

    # 3. and it is a dot product
    wide_w = (xh[:rows] if wh is None else wh).astype(np.longdouble)
    terms = wide_w * got.astype(np.longdouble)
    assert abs(np.longdouble(result) - terms.sum()) <= rows * EPS[L] * np.abs(terms).sum() + 1e-300, (case["id"], result, terms.sum())

    # 4. the integers
    if case["exact"]:
        zi, dot, _ = M.exact(case, m, xh, wh, yh)
        assert np.array_equal(got.astype(np.int64), zi) and np.array_equal(got, zi.astype(got.dtype)), case["id"]
        assert int(result) == dot and float(result) == float(dot), (case["id"], result, dot)

    # 7. z aliased to y: the bytes of the out-of-place call
    if case["z_is_y"]:
        z3, cell3 = _Buf(nan, off["z"], gap=SENTINEL), _cell(L)
        _fused(gpu, case, cell3, None if w is None else w.ptr, z3, y2.ptr, alpha, margs, x, beta)
        torch.cuda.synchronize()
        assert z3.body().tobytes() == got.tobytes() and np.asarray(_one(cell3)).tobytes() == np.asarray(result).tobytes()

    # 6. w == NULL: the dot with x (the path is then chosen from x's address)
    if wh is not None and case["cols"] >= rows and rows <= 200_000:
        z4, cell4, want4 = _Buf(nan, off["z"], gap=SENTINEL), _cell(L), _cell(L)
        _fused(gpu, case, cell4, None, z4, y2.ptr, alpha, margs, x, beta)
        capi.dot_device[L](gpu, _at(want4), rows, x.ptr, z4.ptr)
        torch.cuda.synchronize()
        assert z4.body().tobytes() == got.tobytes()
        assert np.asarray(_one(cell4)).tobytes() == np.asarray(_one(want4)).tobytes()


@pytest.mark.parametrize("letter,cid", [(L, cid) for L, cid in _IDS if _TABLE[L][cid]["rows"] > 0 and _TABLE[L][cid]["hp"] > 0],
                         ids=lambda v: v)
def test_case(gpu, letter, cid):
    """Every row of the case table that launches a first stage."""
    _run(gpu, _TABLE[letter][cid])


@pytest.mark.parametrize("letter", M.LETTERS)
def test_no_rows_and_no_hack_size_write_zero_and_touch_no_vector(gpu, letter):
    """rows <= 0 or hackSize (dMPitch) <= 0: *result = +0 through the dot's second stage, z unchanged."""
    import torch
    from spgpu_amd import capi
    m = H.hdia_matrix(letter, 70, 70, 4, "all")
    dM, offs, hack_offsets = _Buf(m["values"]), _ints(m["offsets"]), _ints(m["hack_offsets"])
    xh, yh = H.operands(letter, 70, 70)
    x, y = _Buf(xh), _Buf(yh)
    untouched = np.full(70, SENTINEL, xh.dtype)
    assert {c["id"] for c in _TABLE[letter].values() if "empty" in c["want"]} == {"rows-0", "hack-0"}
    for rows, hack in ((0, 4), (70, 0), (-3, 4)):
        z, cell, flat = _Buf(untouched, gap=SENTINEL), _cell(letter), _cell(letter)
        capi.hdiaspmv_dot_device[letter](gpu, _at(cell), x.ptr, z.ptr, y.ptr, capi.scalar(letter, 2.0), dM.ptr, C.c_void_p(offs.data_ptr()),
                                         hack, C.c_void_p(hack_offsets.data_ptr()), rows, 70, x.ptr, capi.scalar(letter, 0.5))
        capi.diaspmv_dot_device[letter](gpu, _at(flat), x.ptr, z.ptr, y.ptr, capi.scalar(letter, 2.0), dM.ptr, C.c_void_p(offs.data_ptr()),
                                        hack, rows, 70, 1, x.ptr, capi.scalar(letter, 0.5))
        torch.cuda.synchronize()
        assert z.body().tobytes() == untouched.tobytes(), (rows, hack)
        for got in (_one(cell), _one(flat)):
            assert got == 0 and not np.signbit(got), (rows, hack, got)


@pytest.mark.parametrize("letter", M.LETTERS)
def test_dia_is_hdia_with_one_hack_of_all_rows(gpu, letter):
    """The same arrays through spgpu?diaspmvDotDevice and through spgpu?hdiaspmvDotDevice with hackSize = pitch and
    hackOffsets = {0, diags}: the same bytes."""
    import torch
    from spgpu_amd import capi
    case = _TABLE[letter]["dia-alloc-beta"]
    m, xh, wh, yh = M.inputs(case)
    alpha, beta = M.coefficients(case)
    dM, offs, one = _Buf(m["values"]), _ints(m["offsets"]), _ints([0, m["diags"]])
    x, w, y = _Buf(xh), _Buf(wh), _Buf(yh)
    nan = np.full(m["rows"], np.nan, xh.dtype)
    za, zb, ca, cb = _Buf(nan, gap=SENTINEL), _Buf(nan, gap=SENTINEL), _cell(letter), _cell(letter)
    capi.diaspmv_dot_device[letter](gpu, _at(ca), w.ptr, za.ptr, y.ptr, capi.scalar(letter, alpha), dM.ptr, C.c_void_p(offs.data_ptr()),
                                    m["pitch"], m["rows"], m["cols"], m["diags"], x.ptr, capi.scalar(letter, beta))
    capi.hdiaspmv_dot_device[letter](gpu, _at(cb), w.ptr, zb.ptr, y.ptr, capi.scalar(letter, alpha), dM.ptr, C.c_void_p(offs.data_ptr()),
                                     m["pitch"], C.c_void_p(one.data_ptr()), m["rows"], m["cols"], x.ptr, capi.scalar(letter, beta))
    torch.cuda.synchronize()
    assert za.body().tobytes() == zb.body().tobytes() and np.asarray(_one(ca)).tobytes() == np.asarray(_one(cb)).tobytes()


@pytest.mark.parametrize("letter", M.LETTERS)
def test_a_captured_call_replays_the_eager_bits(gpu, letter):
    """The fused call recorded into a HIP graph on the handle's stream (hipStreamBeginCapture through torch's stream), replayed
    twice with different x: z and *result as the eager call leaves them."""
    import torch
    from spgpu_amd import capi
    from test_gpu_graph_hold import SideStream
    case = _TABLE[letter]["w-null"]
    m, xh, _, yh = M.inputs(case)
    alpha, beta = M.coefficients(case)
    dM, offs, hack_offsets = _Buf(m["values"]), _ints(m["offsets"]), _ints(m["hack_offsets"])
    margs = _matrix_args(case, m, dM, offs, hack_offsets)
    nan = np.full(m["rows"], np.nan, xh.dtype)
    x, y, z, z_eager = _Buf(xh), _Buf(yh), _Buf(nan, gap=SENTINEL), _Buf(nan, gap=SENTINEL)
    cell, cell_eager = _cell(letter), _cell(letter)
    side = SideStream(gpu)
    try:
        side.eager(_fused, gpu, case, cell_eager, None, z_eager, y.ptr, alpha, margs, x, beta)      # code objects loaded before the capture
        graph = side.capture(_fused, gpu, case, cell, None, z, y.ptr, alpha, margs, x, beta)
        for rep in range(2):
            fresh = _Buf(H.values(letter, ("replay", rep), xh.size))
            x.dev.copy_(fresh.dev)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            side.eager(_fused, gpu, case, cell_eager, None, z_eager, y.ptr, alpha, margs, x, beta)
            assert z.body().tobytes() == z_eager.body().tobytes(), rep
            assert np.asarray(_one(cell)).tobytes() == np.asarray(_one(cell_eager)).tobytes(), rep
            assert np.isfinite(_one(cell))
        del graph
    finally:
        side.close()
