"""CPU: the coefficient updates of include/spgpu/ext/update_device.h at the drop-in boundary.  The header declares the calls --
the two value refills, spgpu{S,D,C,Z}hellcsput and spgpuInvertRowOrderDevice -- libspgpu.so exports them and spgpu_amd.capi binds
them with the declared argument counts; the two refills behind the value calls stay out of the headers; without rows or list
entries there is nothing to launch, so the no-op cases return without touching a GPU; an element size that is not 4, 8 or 16 is
refused before a launch; and the plain-C tool is one of the Makefile's TOOLS."""
import ctypes as C
import glob
import os
import re

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "update_device.h")
COUNTS = {"spgpuCsrToHellValuesDevice": 10, "spgpuCsrToEllValuesDevice": 9, "spgpuInvertRowOrderDevice": 4,
          "spgpuShellcsput": 14, "spgpuDhellcsput": 14, "spgpuChellcsput": 14, "spgpuZhellcsput": 14}
HELPERS = ("spgpuCsrToHellValuesDeviceWith", "spgpuCsrToEllValuesDeviceWith")


def test_every_call_of_the_header_is_exported_and_bound():
    with open(HEADER) as f:
        declared = set(DECL.findall(f.read()))
    assert declared == set(COUNTS), sorted(declared)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for name, count in COUNTS.items():
        assert getattr(capi.lib, name) is not None
        assert len(capi.DECLARED[name][1]) == count, name
    for letter in "SDCZ":
        res, args = capi.DECLARED[f"spgpu{letter}hellcsput"]
        assert res is None and args[1] is capi.SCALAR[letter]
        # spgpu?ellcsput's list (alpha, cM, rP, ..., rS, nnz, aI, aJ, aVal, baseIndex) with HELL's storage and rowOf, rows in front of nnz
        ell = capi.DECLARED[f"spgpu{letter}ellcsput"][1]
        assert list(args[:4]) == list(ell[:4]) and list(args[-5:]) == list(ell[-5:])
    for name in ("spgpuCsrToHellValuesDevice", "spgpuCsrToEllValuesDevice", "spgpuInvertRowOrderDevice"):
        assert capi.DECLARED[name][0] is capi.i32


def test_the_header_is_a_c_header_of_the_abi():
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src and "THE CONTRACT" in src
    head = src.split("#include")[0]
    for promise in ("adopted", "Thaw", "csrRowPtr", "ONE of the two values", "never synchronises"):
        assert promise in head, promise
    for neighbour in (os.path.join("ext", "csr_device.h"), "tuning.h"):
        with open(os.path.join(ROOT, "include", "spgpu", neighbour)) as f:
            assert "ext/update_device.h" in f.read(), neighbour


def test_the_refills_behind_the_calls_stay_out_of_the_headers():
    exported = exported_symbols()
    headers = glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")) + glob.glob(os.path.join(ROOT, "include", "spgpu", "ext", "*.h"))
    assert HEADER in headers
    for name in HELPERS:
        assert name in exported and name not in capi.DECLARED
        for header in headers:
            with open(header) as f:
                assert name not in f.read(), (name, header)


def test_nothing_to_do_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: the calls return first
    for rows in (0, -3):
        for code in (capi.TYPE_FLOAT, capi.TYPE_COMPLEX_DOUBLE, 5):
            assert capi.spgpuCsrToHellValuesDevice(C.pointer(h), None, None, 32, rows, None, None, 1, code, None) == capi.SPGPU_SUCCESS
            assert capi.spgpuCsrToEllValuesDevice(C.pointer(h), None, 128, rows, None, None, 0, code, None) == capi.SPGPU_SUCCESS
            for fill in (capi.UPDATE_FILL_PLAIN, capi.UPDATE_FILL_TRANSPOSE, -1):
                assert capi.spgpuCsrToHellValuesDeviceWith(C.pointer(h), None, None, 32, rows, None, None, 1, code, None, fill, 0) == capi.SPGPU_SUCCESS
                assert capi.spgpuCsrToEllValuesDeviceWith(C.pointer(h), None, 128, rows, None, None, 0, code, None, fill, 0) == capi.SPGPU_SUCCESS
        assert capi.spgpuInvertRowOrderDevice(C.pointer(h), None, None, rows) == capi.SPGPU_SUCCESS
    for nnz in (0, -1):
        for letter in "SDCZ":
            assert capi.hellcsput[letter](C.pointer(h), capi.scalar(letter, 1), None, None, 32, None, None, None, 10, nnz, None, None, None,
                                          1) is None


def test_an_element_size_that_is_not_4_8_or_16_is_refused_before_a_launch():
    h = capi.HandleStruct()
    for code in (5, -1):
        assert capi.spgpuSizeOf(code) == 0
        assert capi.spgpuCsrToHellValuesDevice(C.pointer(h), None, None, 32, 10, None, None, 0, code, None) == capi.SPGPU_UNSUPPORTED
        assert capi.spgpuCsrToEllValuesDevice(C.pointer(h), None, 128, 10, None, None, 0, code, None) == capi.SPGPU_UNSUPPORTED
    assert capi.spgpuCsrToHellValuesDevice(C.pointer(h), None, None, 0, 10, None, None, 0, capi.TYPE_DOUBLE, None) == capi.SPGPU_UNSUPPORTED


def test_the_tool_is_one_of_the_makefiles_tools():
    with open(os.path.join(ROOT, "Makefile")) as f:
        text = f.read()
    tools = re.search(r"^TOOLS\s*:=((?:.*\\\n)*.*)$", text, re.M).group(1)
    assert "tools/update_amd.bin" in tools.split() and os.path.exists(os.path.join(ROOT, "tools", "update_amd.c"))
