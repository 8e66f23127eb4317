"""CPU: the HELL / ELL -> CSR construction of include/spgpu/ext/to_csr_device.h at the drop-in boundary.  The header declares
exactly the five calls, libspgpu.so exports them and spgpu_amd.capi binds them (the check test_capi_surface.py makes for
include/spgpu/*.h, whose count the subdirectory leaves alone); the two fills behind the calls stay out of the headers; the scratch
size is host arithmetic; without rows there is nothing to launch, so the no-op cases return without touching a GPU; and the plain-C
tool is one of the Makefile's TOOLS."""
import ctypes as C
import glob
import os
import re

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "to_csr_device.h")
NAMES = {"spgpuToCsrWorkBytes", "spgpuHellToCsrRowPtrDevice", "spgpuHellToCsrDevice", "spgpuEllToCsrRowPtrDevice", "spgpuEllToCsrDevice"}
HELPERS = ("spgpuHellToCsrDeviceWith", "spgpuEllToCsrDeviceWith", "spgpuToCsrFillChunk", "spgpuToCsrDefaultFill")


def test_every_call_of_the_header_is_exported_and_bound():
    with open(HEADER) as f:
        declared = set(DECL.findall(f.read()))
    assert declared == NAMES, sorted(declared)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for name in sorted(declared):
        assert getattr(capi.lib, name) is not None
    assert len(capi.DECLARED["spgpuToCsrWorkBytes"][1]) == 1
    assert len(capi.DECLARED["spgpuHellToCsrRowPtrDevice"][1]) == 12 and len(capi.DECLARED["spgpuEllToCsrRowPtrDevice"][1]) == 11
    assert len(capi.DECLARED["spgpuHellToCsrDevice"][1]) == 14 and len(capi.DECLARED["spgpuEllToCsrDevice"][1]) == 14


def test_the_header_is_a_c_header_of_the_abi():
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src
    assert src.count("NEW (no counterpart in the reference)") == 4 and "no counterpart in the reference" in src.split("#include")[0]
    for neighbour in ("convert_device.h", os.path.join("ext", "csr_device.h")):
        with open(os.path.join(ROOT, "include", "spgpu", neighbour)) as f:
            assert "ext/to_csr_device.h" in f.read(), neighbour


def test_the_fills_behind_the_calls_stay_out_of_the_headers():
    """The two fills and the chunk width are reachable for the tests and the A/B tool, but are no part of the declared ABI."""
    assert capi.TO_CSR_FILL_CHUNK >= 1 and capi.TO_CSR_FILL_DEFAULT in (capi.TO_CSR_FILL_PLAIN, capi.TO_CSR_FILL_TRANSPOSE)
    exported = exported_symbols()
    headers = glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")) + glob.glob(os.path.join(ROOT, "include", "spgpu", "ext", "*.h"))
    assert HEADER in headers
    for name in HELPERS:
        assert name in exported and name not in capi.DECLARED
        for header in headers:
            with open(header) as f:
                assert name not in f.read(), (name, header)


def test_work_bytes_is_host_arithmetic():
    """No GPU is asked (this test runs without one): 0 without rows, a multiple of 256, never shrinking, and room for the lengths in
    matrix order, the hit counts and the tile totals of the three-launch scan (tiles of 1 024 rows, the grand total behind them)."""
    for rows in (0, -1, -3, -2**31):
        assert capi.spgpuToCsrWorkBytes(rows) == 0
    before = 0
    for rows in (1, 2, 63, 64, 1023, 1024, 1025, 2048, 2049, 10**6, 10**7, 2**31 - 1):
        got = capi.spgpuToCsrWorkBytes(rows)
        assert got % 256 == 0 and got >= before, rows
        before = got
    for rows in (1, 1024, 1025, 10**7):
        tiles = (rows + 1023) // 1024
        assert capi.spgpuToCsrWorkBytes(rows) >= 4 * (2 * rows + tiles + 1), rows


def test_no_rows_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: rowsCount <= 0 returns first
    for rows in (0, -3):
        for call, lead in ((capi.spgpuHellToCsrRowPtrDevice, (32, None)), (capi.spgpuEllToCsrRowPtrDevice, (128,))):
            nnz, longest = C.c_int(-1), C.c_int(-1)
            assert call(C.pointer(h), None, C.byref(nnz), C.byref(longest), 1, *lead, None, None, rows, 0, None) == capi.SPGPU_SUCCESS
            assert nnz.value == 0 and longest.value == 0
        for code in (capi.TYPE_FLOAT, capi.TYPE_COMPLEX_DOUBLE):
            hell = (C.pointer(h), None, None, None, 1, None, None, 32, None, None, None, rows, 0, code)
            ell = (C.pointer(h), None, None, None, 0, None, None, 128, 128, None, None, rows, 1, code)
            assert capi.spgpuHellToCsrDevice(*hell) == capi.SPGPU_SUCCESS and capi.spgpuEllToCsrDevice(*ell) == capi.SPGPU_SUCCESS
            for fill in (capi.TO_CSR_FILL_PLAIN, capi.TO_CSR_FILL_TRANSPOSE):
                assert capi.spgpuHellToCsrDeviceWith(*hell, fill, 0) == capi.SPGPU_SUCCESS
                assert capi.spgpuEllToCsrDeviceWith(*ell, fill, 0) == capi.SPGPU_SUCCESS


def test_the_tool_is_one_of_the_makefiles_tools():
    with open(os.path.join(ROOT, "Makefile")) as f:
        text = f.read()
    tools = re.search(r"^TOOLS\s*:=((?:.*\\\n)*.*)$", text, re.M).group(1)
    assert "tools/to_csr_amd.bin" in tools.split() and os.path.exists(os.path.join(ROOT, "tools", "to_csr_amd.c"))
