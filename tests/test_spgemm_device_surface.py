"""CPU: the sparse-product calls of include/spgpu/ext/spgemm_device.h at the drop-in boundary.  The header compiles as plain C99 with
-Wall -Werror and declares the five calls; libspgpu.so exports them and spgpu_amd.capi binds them with the declared argument lists;
the two fills behind the value calls, the default-fill report and the row cap stay out of the headers; the scratch size grows with
the products and with A's rows and is 0 only where the assembly's -- which asks rocPRIM the same kind of question -- is; without
rows or entries there is nothing to launch, so the no-op cases return without touching a GPU; a type the fills cannot multiply is
refused before a launch; the header's text makes the contract's promises; and the plain-C tool is one of the Makefile's TOOLS."""
import ctypes as C
import glob
import os
import re
import subprocess

from spgpu_amd import capi
from test_assemble_device_surface import _declared_arguments
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "spgemm_device.h")
i32, ptr, Handle = capi.i32, capi.ptr, capi.Handle
SIGNATURES = {
    "spgpuCsrSpgemmWorkBytes": (C.c_size_t, [i32, i32, i32]),
    "spgpuCsrSpgemmProductsDevice": (i32, [Handle, C.POINTER(i32), i32, i32, ptr, ptr, ptr, i32, ptr]),
    "spgpuCsrSpgemmPlanDevice": (i32, [Handle, C.POINTER(i32), ptr, i32, i32, i32, ptr, ptr, ptr, ptr, i32, i32, ptr]),
    "spgpuCsrSpgemmDevice": (i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32, ptr]),
    "spgpuCsrSpgemmValuesDevice": (i32, [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32]),
}
HELPERS = ("spgpuCsrSpgemmDeviceWith", "spgpuCsrSpgemmValuesDeviceWith", "spgpuCsrSpgemmDefaultFill", "spgpuCsrSpgemmRowCap")
COUNTS = (-5, 0, 1, 63, 64, 65, 3000, 300000, 5000000)


def test_every_call_of_the_header_is_exported_and_bound_as_declared():
    with open(HEADER) as f:
        src = f.read()
    declared = set(DECL.findall(src))
    assert declared == set(SIGNATURES), sorted(declared)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    for name, (res, args) in SIGNATURES.items():
        assert getattr(capi.lib, name) is not None
        assert capi.DECLARED[name][0] is res, name
        assert list(capi.DECLARED[name][1]) == args, name
        assert _declared_arguments(src, name) == args, name
        body = re.search(r"^(?:spgpuStatus_t|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", src, re.M).group(1)
        for arg in body.split(","):                      # every pointer says where it lives
            assert "*" not in arg or "__device" in arg or "__host" in arg, (name, arg)
    assert src.count("/* NEW") == len(SIGNATURES)


def test_the_header_compiles_as_c99_with_warnings_as_errors(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "spgpu/ext/spgemm_device.h"\n'
                   "int main(void){ spgpuHandle_t h = 0; (void)h; return spgpuCsrSpgemmWorkBytes(0, 0, 0) ? 0 : 1; }\n")
    rocm = "/opt/rocm"
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{ROOT}/include", str(src), "-o",
           str(tmp_path / "abi"), f"-L{os.path.dirname(capi.LIB_PATH)}", "-lspgpu", f"-Wl,-rpath,{os.path.dirname(capi.LIB_PATH)}",
           f"-Wl,-rpath,{rocm}/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    assert subprocess.run([str(tmp_path / "abi")]).returncode == 0


def test_the_header_states_the_contract_and_its_neighbours_point_to_it():
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src and "THE CONTRACT" in src
    head = src.split("#include")[0]
    for promise in ("any order", "more than once", "strictly ascending", "symbolic", "cancel stays", "STORAGE ORDER", "rounded once",
                    "no fused multiply-add", "ar*br - ai*bi", "ar*bi + ai*br", "NOT the hipCfma", "numpy can restate", "starts from +0",
                    "stored as +0.0", "no atomics", "one writer", "SPGPU_UNSUPPORTED", "before a launch", "INT_MAX", "= -1", "clamped",
                    "may be freed", "never reads it", "synchronise", "captured", "trust their index arrays", "all baseIndex"):
        assert promise in head, promise
    for neighbour in ("csr_device.h", "assemble_device.h"):
        with open(os.path.join(ROOT, "include", "spgpu", "ext", neighbour)) as f:
            assert "ext/spgemm_device.h" in f.read(), neighbour


def test_the_fills_behind_the_calls_stay_out_of_the_headers():
    exported = exported_symbols()
    headers = glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")) + glob.glob(os.path.join(ROOT, "include", "spgpu", "ext", "*.h"))
    assert HEADER in headers
    for name in HELPERS:
        assert name in exported and name not in capi.DECLARED
        for header in headers:
            with open(header) as f:
                assert name not in f.read(), (name, header)
    assert capi.SPGEMM_FILL_DEFAULT in (capi.SPGEMM_FILL_PLAIN, capi.SPGEMM_FILL_STAGED)
    # a workgroup of four wavefronts keeps a row each, columns and 16-byte values, in at most 64 KB of static LDS
    assert capi.SPGEMM_ROW_CAP >= 64 and 4 * capi.SPGEMM_ROW_CAP * (4 + 16) <= 64 * 1024
    for header in glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")):   # nothing of the product where test_capi_surface counts
        with open(header) as f:
            assert not [n for n in DECL.findall(f.read()) if "Spgemm" in n], header


def test_work_bytes_grow_with_the_products_and_the_rows_and_vanish_only_where_the_assemblys_do():
    for rows, cols in ((1, 1), (70, 90), (20000, 20000)):
        sizes = [capi.spgpuCsrSpgemmWorkBytes(rows, cols, n) for n in COUNTS]
        twins = [capi.spgpuCooAssembleWorkBytes(rows, cols, n) for n in COUNTS]
        assert [s == 0 for s in sizes] == [t == 0 for t in twins], (sizes, twins)
        assert sizes[0] == sizes[1] > 0                               # no product: the head alone, and no GPU is asked
        assert sizes[1] >= 8 * rows
        alive = [s for s in sizes if s]
        assert alive == sorted(alive), sizes
        for n, size in zip(COUNTS[2:], sizes[2:]):
            assert size == 0 or size >= 20 * n + 4 * rows, (n, size)   # keys twice, entry numbers; the row starts
    assert capi.spgpuCsrSpgemmWorkBytes(1000, 7, 0) == capi.spgpuCsrSpgemmWorkBytes(1000, 7000, 0)
    assert capi.spgpuCsrSpgemmWorkBytes(1000, 7, 0) > capi.spgpuCsrSpgemmWorkBytes(10, 7, 0)
    assert capi.spgpuCsrSpgemmWorkBytes(-4, 7, 0) == capi.spgpuCsrSpgemmWorkBytes(0, 7, 0) > 0


def test_nothing_to_do_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: the calls return first
    count = C.c_int(77)
    for rows in (0, -3):
        assert capi.spgpuCsrSpgemmProductsDevice(C.pointer(h), C.byref(count), rows, 5, None, None, None, 1, None) == capi.SPGPU_SUCCESS
        assert count.value == 0
        count.value = 77
        assert capi.spgpuCsrSpgemmPlanDevice(C.pointer(h), C.byref(count), None, rows, 5, 5, None, None, None, None, 1, 10,
                                             None) == capi.SPGPU_SUCCESS
        assert count.value == 0
        count.value = 77
    for rows, entries in ((0, 5), (-1, 5), (10, 0), (10, -2)):
        for code in (capi.TYPE_FLOAT, capi.TYPE_COMPLEX_DOUBLE, capi.TYPE_INT, 5):
            args = (C.pointer(h), None, None, entries, rows, None, None, None, None, None, None, None, 1, code, None)
            assert capi.spgpuCsrSpgemmDevice(*args) == capi.SPGPU_SUCCESS
            for fill in (capi.SPGEMM_FILL_PLAIN, capi.SPGEMM_FILL_STAGED, -1):
                assert capi.spgpuCsrSpgemmDeviceWith(*args, fill, 0) == capi.SPGPU_SUCCESS
    for rows in (0, -1):
        for code in (capi.TYPE_DOUBLE, capi.TYPE_INT):
            args = (C.pointer(h), None, rows, None, None, None, None, None, None, None, None, 0, code)
            assert capi.spgpuCsrSpgemmValuesDevice(*args) == capi.SPGPU_SUCCESS
            for fill in (capi.SPGEMM_FILL_PLAIN, capi.SPGEMM_FILL_STAGED, -1):
                assert capi.spgpuCsrSpgemmValuesDeviceWith(*args, fill, 0) == capi.SPGPU_SUCCESS


def test_a_type_the_fills_cannot_multiply_is_refused_before_a_launch():
    h = capi.HandleStruct()
    for code in (capi.TYPE_INT, 5, -1):
        values = (C.pointer(h), None, 10, None, None, None, None, None, None, None, None, 0, code)
        full = (C.pointer(h), None, None, 20, 10, None, None, None, None, None, None, None, 0, code, None)
        assert capi.spgpuCsrSpgemmValuesDevice(*values) == capi.SPGPU_UNSUPPORTED
        assert capi.spgpuCsrSpgemmDevice(*full) == capi.SPGPU_UNSUPPORTED
        for fill in (capi.SPGEMM_FILL_PLAIN, capi.SPGEMM_FILL_STAGED):
            assert capi.spgpuCsrSpgemmValuesDeviceWith(*values, fill, 0) == capi.SPGPU_UNSUPPORTED
            assert capi.spgpuCsrSpgemmDeviceWith(*full, fill, 0) == capi.SPGPU_UNSUPPORTED
    ok_type = (C.pointer(h), None, 10, None, None, None, None, None, None, None, None, 0, capi.TYPE_DOUBLE)
    assert capi.spgpuCsrSpgemmValuesDeviceWith(*ok_type, 2, 0) == capi.SPGPU_UNSUPPORTED       # no such fill
    # products to sort and no columns at all, or no scratch: refused before a launch
    count = C.c_int(77)
    assert capi.spgpuCsrSpgemmPlanDevice(C.pointer(h), C.byref(count), None, 5, 5, 0, None, None, None, None, 0, 10, None) == capi.SPGPU_UNSUPPORTED
    assert capi.spgpuCsrSpgemmPlanDevice(C.pointer(h), C.byref(count), None, 5, 5, 5, None, None, None, None, 0, 10, None) == capi.SPGPU_UNSUPPORTED
    assert count.value == 0
    count.value = 77
    assert capi.spgpuCsrSpgemmProductsDevice(C.pointer(h), C.byref(count), 5, 5, None, None, None, 0, None) == capi.SPGPU_UNSUPPORTED
    assert count.value == 0


def test_the_tool_is_one_of_the_makefiles_tools():
    with open(os.path.join(ROOT, "Makefile")) as f:
        text = f.read()
    tools = re.search(r"^TOOLS\s*:=((?:.*\\\n)*.*)$", text, re.M).group(1)
    assert "tools/galerkin_amd.bin" in tools.split() and os.path.exists(os.path.join(ROOT, "tools", "galerkin_amd.c"))
