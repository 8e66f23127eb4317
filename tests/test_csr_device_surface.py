"""CPU: the CSR -> ELL / HELL construction of include/spgpu/ext/csr_device.h at the drop-in boundary.  The header declares exactly
the three calls, libspgpu.so exports them and spgpu_amd.capi binds them (the check test_capi_surface.py makes for
include/spgpu/*.h, whose count the subdirectory leaves alone); without rows there is nothing to launch, so the no-op cases return
without touching a GPU; and the host helper that makes CSR out of the synthetic COO generators keeps the entry order."""
import ctypes as C
import os

import numpy as np

from spgpu_amd import capi, synth
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "csr_device.h")
NAMES = {"spgpuCsrRowLengthsDevice", "spgpuCsrToEllDevice", "spgpuCsrToHellDevice"}


def test_every_call_of_the_header_is_exported_and_bound():
    with open(HEADER) as f:
        declared = set(DECL.findall(f.read()))
    assert declared == NAMES, sorted(declared)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for name in sorted(declared):
        assert getattr(capi.lib, name) is not None
    assert len(capi.DECLARED["spgpuCsrRowLengthsDevice"][1]) == 6
    assert len(capi.DECLARED["spgpuCsrToEllDevice"][1]) == 13 and len(capi.DECLARED["spgpuCsrToHellDevice"][1]) == 13


def test_the_header_is_a_c_header_of_the_abi():
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src
    assert "spgpuCooConvertWorkBytes(rowsCount, 0)" in src     # what spgpuHellPlanDevice needs of `work` is said there


def test_convert_device_h_points_to_the_header():
    with open(os.path.join(ROOT, "include", "spgpu", "convert_device.h")) as f:
        assert "ext/csr_device.h" in f.read()


def test_the_fills_behind_the_calls_stay_out_of_the_headers():
    """The two fills and the chunk width are reachable for the tests and the A/B tool, but are no part of the declared ABI."""
    assert capi.CSR_FILL_CHUNK >= 1 and capi.CSR_FILL_DEFAULT in (capi.CSR_FILL_PLAIN, capi.CSR_FILL_TRANSPOSE)
    for name in ("spgpuCsrToEllDeviceWith", "spgpuCsrToHellDeviceWith", "spgpuCsrFillChunk", "spgpuCsrDefaultFill"):
        assert name not in capi.DECLARED
        for header in ("convert_device.h", os.path.join("ext", "csr_device.h")):
            with open(os.path.join(ROOT, "include", "spgpu", header)) as f:
                assert name not in f.read()


def test_no_rows_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: rowsCount <= 0 returns first
    for rows in (0, -3):
        longest = C.c_int(-1)
        assert capi.spgpuCsrRowLengthsDevice(C.pointer(h), None, C.byref(longest), rows, None, 0) == capi.SPGPU_SUCCESS
        assert longest.value == 0
        for code in (capi.TYPE_FLOAT, capi.TYPE_COMPLEX_DOUBLE):
            assert capi.spgpuCsrToEllDevice(C.pointer(h), None, None, 0, 0, 0, rows, None, None, None, 0, code, None) == capi.SPGPU_SUCCESS
            assert capi.spgpuCsrToHellDevice(C.pointer(h), None, None, None, 32, 1, rows, None, None, None, 1, code, None) == capi.SPGPU_SUCCESS
            for fill in (capi.CSR_FILL_PLAIN, capi.CSR_FILL_TRANSPOSE):
                assert capi.spgpuCsrToHellDeviceWith(C.pointer(h), None, None, None, 32, 1, rows, None, None, None, 1, code, None, fill,
                                                     0) == capi.SPGPU_SUCCESS


def test_coo_to_csr_keeps_the_encounter_order():
    """synth.coo_to_csr: a stable sort by row -- the k-th CSR entry of a row is its k-th occurrence in the COO order, duplicates kept,
    both bases, empty rows at both ends."""
    rows = np.array([3, 1, 3, 3, 1, 4], np.int32)
    cols = np.array([9, 8, 7, 9, 6, 5], np.int32)
    vals = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    for base in (0, 1):
        row_ptr, c, v = synth.coo_to_csr(6, rows + base, cols + base, vals, base)
        assert row_ptr.dtype == np.int32 and c.dtype == np.int32 and v.dtype == vals.dtype
        assert (row_ptr - base).tolist() == [0, 0, 2, 2, 5, 6, 6]
        assert (c - base).tolist() == [8, 6, 9, 7, 9, 5] and v.tolist() == [2.0, 5.0, 1.0, 3.0, 4.0, 6.0]
    row_ptr, c, v = synth.coo_to_csr(4, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 1)
    assert row_ptr.tolist() == [1, 1, 1, 1, 1] and c.size == 0 and v.size == 0
