"""CPU: the sparse-sum calls of include/spgpu/ext/add_device.h at the drop-in boundary.  The header compiles as plain C99 with -Wall
-Werror and declares the five calls; libspgpu.so exports them and spgpu_amd.capi binds them with the declared argument lists; the
fills behind the value calls, the default-fill report, the tile and the row cap stay out of the headers; the scratch size grows with
the rows and is the same without rows as with none; without rows or entries there is nothing to launch, so the no-op cases return
without touching a GPU; a type the fills cannot multiply is refused before a launch; the header's text makes the contract's
promises and its three neighbours point to it; and the plain-C tool is one of the Makefile's TOOLS."""
import ctypes as C
import glob
import os
import re
import subprocess

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "add_device.h")
i32, ptr, Handle = capi.i32, capi.ptr, capi.Handle
_VALUES = [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32]
SIGNATURES = {
    "spgpuCsrAddWorkBytes": (C.c_size_t, [i32]),
    "spgpuCsrAddPlanDevice": (i32, [Handle, C.POINTER(i32), ptr, i32, i32, ptr, ptr, ptr, ptr, i32, ptr]),
    "spgpuCsrAddDevice": (i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32]),
    "spgpuCsrAddValuesDevice": (i32, _VALUES),
    "spgpuCsrAddValuesDeviceScalars": (i32, _VALUES),
}
HELPERS = ("spgpuCsrAddDeviceWith", "spgpuCsrAddValuesDeviceWith", "spgpuCsrAddValuesDeviceScalarsWith", "spgpuCsrAddDefaultFill",
           "spgpuCsrAddTile", "spgpuCsrAddRowCap")
C_TYPE = {"spgpuHandle_t": Handle, "int": i32, "spgpuType_t": i32, "int*": ptr, "void*": ptr}
ROWS = (-5, 0, 1, 63, 64, 65, 1023, 1024, 3000, 300000, 5000000, 2 ** 31 - 1)


def _declared_arguments(src, name):
    """The argument types of `name` as the header declares them, mapped to ctypes: '__host int*' is the host int the Plan returns,
    '__host void*' one element of valuesType on the host -- an address like any other to ctypes."""
    text = re.search(r"^(?:spgpuStatus_t|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", src, re.M).group(1)
    out = []
    for arg in text.split(","):
        words = re.sub(r"/\*.*?\*/", "", arg, flags=re.S).replace("*", "* ").split()
        host = "__host" in words
        words = [w for w in words if w not in ("const", "__device", "__host")]
        kind = "".join(words[:-1])
        out.append(C.POINTER(i32) if host and kind == "int*" else C_TYPE[kind])
    return out


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
    assert src.count("/* NEW (no counterpart in the reference)") == src.count("/* NEW") == len(SIGNATURES)
    # alpha and beta: on the host in the two host forms, on the device in the Scalars form
    scalars = lambda name: re.findall(r"const (__\w+) void\* (?:alpha|beta)", re.search(r"^spgpuStatus_t\s+" + name + r"\s*\(([^;]*)\)\s*;", src, re.M).group(1))
    assert scalars("spgpuCsrAddDevice") == scalars("spgpuCsrAddValuesDevice") == ["__host", "__host"]
    assert scalars("spgpuCsrAddValuesDeviceScalars") == ["__device", "__device"]


def test_the_header_compiles_as_c99_with_warnings_as_errors(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "spgpu/ext/add_device.h"\n'
                   "int main(void){ spgpuHandle_t h = 0; (void)h; return spgpuCsrAddWorkBytes(0) ? 0 : 1; }\n")
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
    for promise in ("strictly ascending", "empty row is fine", "symbolic", "if A or B stores it", "duplicate-free", "cancel stays",
                    "ONE common baseIndex", "ONE element of valuesType", "read them at call time", "(alpha * a) + (beta * b)",
                    "rounded once", "no fused multiply-add", "the product alone and not + 0", "sr*vr - si*vi", "sr*vi + si*vr",
                    "six operations", "componentwise", "NOT the hipCfma", "numpy can restate", "with its own bits", "-0.0 included",
                    "no moved bits are promised", "no atomics", "one writer", "SPGPU_UNSUPPORTED", "before a launch",
                    "must not overlap", "INT_MAX", "64-bit total", "= -1", "clamped", "after its one synchronise", "descends or repeats",
                    "may be freed", "no fill ever reads it", "synchronise", "captured", "trust their index arrays",
                    "read the count on the device", "takes no cColIndices", "nothing launched"):
        assert promise in head, promise
    for neighbour in ("csr_device.h", "assemble_device.h", "spgemm_device.h"):
        with open(os.path.join(ROOT, "include", "spgpu", "ext", neighbour)) as f:
            assert "ext/add_device.h" in f.read(), neighbour


def test_the_fills_behind_the_calls_stay_out_of_the_headers():
    exported = exported_symbols()
    headers = glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")) + glob.glob(os.path.join(ROOT, "include", "spgpu", "ext", "*.h"))
    assert HEADER in headers
    for name in HELPERS:
        assert name in exported and name not in capi.DECLARED
        for header in headers:
            with open(header) as f:
                assert name not in f.read(), (name, header)
    assert capi.ADD_FILL_DEFAULT in (capi.ADD_FILL_PLAIN, capi.ADD_FILL_STAGED)
    # only the last row of a tile can be longer than the tile, so every shorter row must be one the staged fill stages; the column
    # slices of a tile's rows -- A's and B's, at most tile - 1 + cap ints each -- stay within 64 KB of static LDS for every type
    assert capi.ADD_TILE >= 256 and capi.ADD_ROW_CAP >= capi.ADD_TILE
    assert 2 * (capi.ADD_TILE - 1 + capi.ADD_ROW_CAP) * 4 <= 64 * 1024
    for header in glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")):   # nothing of the sum where test_capi_surface counts
        with open(header) as f:
            assert not [n for n in DECL.findall(f.read()) if "CsrAdd" in n], header


def test_work_bytes_grow_with_the_rows_and_are_the_same_without_rows_as_with_none():
    sizes = [capi.spgpuCsrAddWorkBytes(n) for n in ROWS]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] > 0 and sizes[-1] > sizes[1]
    for n, size in zip(ROWS, sizes):
        assert size >= 16 + 4 * ((max(n, 0) + 1 + 1023) // 1024 + 2)          # the count and the flag; a total per 1 024 row counts
    assert sizes[-1] < 16 * 2 ** 20                                            # INT_MAX rows: 8 MB, not a share of the matrix


def test_nothing_to_do_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: the calls return first
    count = C.c_int(77)
    for rows in (0, -3):
        assert capi.spgpuCsrAddPlanDevice(C.pointer(h), C.byref(count), None, rows, 5, None, None, None, None, 1, None) == capi.SPGPU_SUCCESS
        assert count.value == 0
        count.value = 77
    for rows, entries in ((0, 5), (-1, 5), (10, 0), (10, -2)):
        for code in (capi.TYPE_FLOAT, capi.TYPE_COMPLEX_DOUBLE, capi.TYPE_INT, 5):
            args = (C.pointer(h), None, None, entries, rows, None, None, None, None, None, None, None, None, None, 1, code)
            assert capi.spgpuCsrAddDevice(*args) == capi.SPGPU_SUCCESS
            for fill in (capi.ADD_FILL_PLAIN, capi.ADD_FILL_STAGED, -1, 2):
                assert capi.spgpuCsrAddDeviceWith(*args, fill, 0) == capi.SPGPU_SUCCESS
    for rows in (0, -1):
        for code in (capi.TYPE_DOUBLE, capi.TYPE_INT):
            args = (C.pointer(h), None, rows, None, None, None, None, None, None, None, None, None, 0, code)
            assert capi.spgpuCsrAddValuesDevice(*args) == capi.SPGPU_SUCCESS
            assert capi.spgpuCsrAddValuesDeviceScalars(*args) == capi.SPGPU_SUCCESS
            for fill in (capi.ADD_FILL_PLAIN, capi.ADD_FILL_STAGED, -1, 2):
                assert capi.spgpuCsrAddValuesDeviceWith(*args, fill, 0) == capi.SPGPU_SUCCESS
                assert capi.spgpuCsrAddValuesDeviceScalarsWith(*args, fill, 0) == capi.SPGPU_SUCCESS


def test_a_type_the_fills_cannot_multiply_is_refused_before_a_launch():
    h = capi.HandleStruct()
    one = C.c_double(1.0)
    at = C.cast(C.pointer(one), C.c_void_p)
    for code in (capi.TYPE_INT, 5, -1):
        values = (C.pointer(h), None, 10, at, None, None, None, at, None, None, None, None, 0, code)
        full = (C.pointer(h), None, None, 20, 10, at, None, None, None, at, None, None, None, None, 0, code)
        assert capi.spgpuCsrAddValuesDevice(*values) == capi.SPGPU_UNSUPPORTED
        assert capi.spgpuCsrAddValuesDeviceScalars(*values) == capi.SPGPU_UNSUPPORTED
        assert capi.spgpuCsrAddDevice(*full) == capi.SPGPU_UNSUPPORTED
        for fill in (capi.ADD_FILL_PLAIN, capi.ADD_FILL_STAGED):
            assert capi.spgpuCsrAddValuesDeviceWith(*values, fill, 0) == capi.SPGPU_UNSUPPORTED
            assert capi.spgpuCsrAddValuesDeviceScalarsWith(*values, fill, 0) == capi.SPGPU_UNSUPPORTED
            assert capi.spgpuCsrAddDeviceWith(*full, fill, 0) == capi.SPGPU_UNSUPPORTED
    ok_type = (C.pointer(h), None, 10, at, None, None, None, at, None, None, None, None, 0, capi.TYPE_DOUBLE)
    assert capi.spgpuCsrAddValuesDeviceWith(*ok_type, 2, 0) == capi.SPGPU_UNSUPPORTED          # no such fill
    assert capi.spgpuCsrAddValuesDeviceWith(*ok_type, capi.ADD_FILL_PLAIN, 0) == capi.SPGPU_UNSUPPORTED   # no destination
    no_scalar = (C.pointer(h), C.c_void_p(256), 10, None, None, None, None, at, None, None, None, None, 0, capi.TYPE_DOUBLE)
    assert capi.spgpuCsrAddValuesDevice(*no_scalar) == capi.SPGPU_UNSUPPORTED                  # no alpha to read
    # rows to analyse and no scratch, or no row pointer to write: refused before a launch
    count = C.c_int(77)
    assert capi.spgpuCsrAddPlanDevice(C.pointer(h), C.byref(count), C.c_void_p(256), 5, 5, None, None, None, None, 0, None) == capi.SPGPU_UNSUPPORTED
    assert capi.spgpuCsrAddPlanDevice(C.pointer(h), C.byref(count), None, 5, 5, None, None, None, None, 0, C.c_void_p(256)) == capi.SPGPU_UNSUPPORTED
    assert count.value == 0


def test_the_tool_is_one_of_the_makefiles_tools():
    with open(os.path.join(ROOT, "Makefile")) as f:
        text = f.read()
    tools = re.search(r"^TOOLS\s*:=((?:.*\\\n)*.*)$", text, re.M).group(1)
    assert "tools/timestep_amd.bin" in tools.split() and os.path.exists(os.path.join(ROOT, "tools", "timestep_amd.c"))
