"""CPU: the assembly calls of include/spgpu/ext/assemble_device.h at the drop-in boundary.  The header compiles as plain C and
declares the four calls; libspgpu.so exports them and spgpu_amd.capi binds them with the declared argument lists; the two fills
behind the value calls and the staged fill's constants stay out of the headers; the scratch size grows with the list and is 0
only where the transpose's -- which asks rocPRIM the same question -- is; without contributions or matrix entries there is
nothing to launch, so the no-op cases return without touching a GPU; a type the fills cannot add is refused before a launch; and
the plain-C tool is one of the Makefile's TOOLS."""
import ctypes as C
import glob
import os
import re
import subprocess

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "assemble_device.h")
i32, ptr, Handle = capi.i32, capi.ptr, capi.Handle
SIGNATURES = {
    "spgpuCooAssembleWorkBytes": (C.c_size_t, [i32, i32, i32]),
    "spgpuCooAssemblePlanDevice": (i32, [Handle, C.POINTER(i32), ptr, ptr, ptr, i32, i32, i32, ptr, ptr, i32, i32, ptr]),
    "spgpuCooAssembleDevice": (i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, i32, i32, i32, ptr, ptr]),
    "spgpuCooAssembleValuesDevice": (i32, [Handle, ptr, i32, i32, ptr, i32, ptr, ptr]),
}
HELPERS = ("spgpuCooAssembleDeviceWith", "spgpuCooAssembleValuesDeviceWith", "spgpuCooAssembleDefaultFill", "spgpuCooAssembleTile",
           "spgpuCooAssembleChunk")
C_TYPE = {"spgpuHandle_t": Handle, "int": i32, "spgpuType_t": i32, "int*": ptr, "void*": ptr}


def _declared_arguments(src, name):
    """The argument types of `name` as the header declares them, mapped to ctypes ('__host int*' is the one host pointer)."""
    text = re.search(r"^(?:spgpuStatus_t|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", src, re.M).group(1)
    out = []
    for arg in text.split(","):
        words = re.sub(r"/\*.*?\*/", "", arg, flags=re.S).replace("*", "* ").split()
        host = "__host" in words
        words = [w for w in words if w not in ("const", "__device", "__host")]
        kind = "".join(words[:-1])
        out.append(C.POINTER(i32) if host else C_TYPE[kind])
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


def test_the_header_compiles_as_plain_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "spgpu/ext/assemble_device.h"\n'
                   "int main(void){ spgpuHandle_t h = 0; (void)h; return spgpuCooAssembleWorkBytes(0, 0, 0) ? 0 : 1; }\n")
    rocm = "/opt/rocm"
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{ROOT}/include", str(src), "-o",
           str(tmp_path / "abi"), f"-L{os.path.dirname(capi.LIB_PATH)}", "-lspgpu", f"-Wl,-rpath,{os.path.dirname(capi.LIB_PATH)}",
           f"-Wl,-rpath,{rocm}/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    assert subprocess.run([str(tmp_path / "abi")]).returncode == 0


def test_the_header_states_the_contract_and_its_neighbour_points_to_it():
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src and "THE CONTRACT" in src
    head = src.split("#include")[0]
    for promise in ("left to right", "stable", "not from zero", "no atomics", "not written", "SPGPU_UNSUPPORTED", "may be freed",
                    "synchronises"):
        assert promise in head, promise
    with open(os.path.join(ROOT, "include", "spgpu", "convert_device.h")) as f:
        assert "ext/assemble_device.h" in f.read()


def test_the_fills_behind_the_calls_stay_out_of_the_headers():
    exported = exported_symbols()
    headers = glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")) + glob.glob(os.path.join(ROOT, "include", "spgpu", "ext", "*.h"))
    assert HEADER in headers
    for name in HELPERS:
        assert name in exported and name not in capi.DECLARED
        for header in headers:
            with open(header) as f:
                assert name not in f.read(), (name, header)
    assert capi.ASSEMBLE_FILL_DEFAULT in (capi.ASSEMBLE_FILL_PLAIN, capi.ASSEMBLE_FILL_STAGED)
    assert capi.ASSEMBLE_TILE > 0 and capi.ASSEMBLE_CHUNK >= capi.ASSEMBLE_TILE and capi.ASSEMBLE_CHUNK % capi.ASSEMBLE_TILE == 0


def test_work_bytes_grow_with_the_list_and_vanish_only_where_the_transposes_do():
    for rows, cols in ((1, 1), (70, 50), (20000, 20000)):
        sizes = [capi.spgpuCooAssembleWorkBytes(rows, cols, nnz) for nnz in (-5, 0, 1, 63, 64, 65, 3000, 300000, 5000000)]
        twins = [capi.spgpuHellTransposeWorkBytes(rows, cols, nnz) for nnz in (-5, 0, 1, 63, 64, 65, 3000, 300000, 5000000)]
        assert [s == 0 for s in sizes] == [t == 0 for t in twins], (sizes, twins)
        assert sizes[0] == sizes[1] > 0                               # no list: the head alone, and no GPU is asked
        alive = [s for s in sizes if s]
        assert alive == sorted(alive), sizes
        for nnz, size in zip((1, 63, 64, 65, 3000, 300000, 5000000), sizes[2:]):
            assert size == 0 or size >= 24 * nnz + 4 * rows, (nnz, size)   # keys twice, ids, entry numbers; the row starts
    assert capi.spgpuCooAssembleWorkBytes(1000, 7, 100) == capi.spgpuCooAssembleWorkBytes(1000, 7000, 100)
    assert capi.spgpuCooAssembleWorkBytes(1000, 7, 100) > capi.spgpuCooAssembleWorkBytes(10, 7, 100)


def test_nothing_to_do_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: the calls return first
    unique = C.c_int(77)
    for rows in (0, -3):
        assert capi.spgpuCooAssemblePlanDevice(C.pointer(h), C.byref(unique), None, None, None, rows, 5, 10, None, None, 0, 1,
                                               None) == capi.SPGPU_SUCCESS
        assert unique.value == 0
        unique.value = 77
    for nnz, entries in ((0, 5), (-1, 5), (10, 0), (10, -2)):
        for code in (capi.TYPE_FLOAT, capi.TYPE_COMPLEX_DOUBLE, capi.TYPE_INT, 5):
            assert capi.spgpuCooAssembleDevice(C.pointer(h), None, None, entries, nnz, None, None, 0, 1, code, None, None) == capi.SPGPU_SUCCESS
            assert capi.spgpuCooAssembleValuesDevice(C.pointer(h), None, entries, nnz, None, code, None, None) == capi.SPGPU_SUCCESS
            for fill in (capi.ASSEMBLE_FILL_PLAIN, capi.ASSEMBLE_FILL_STAGED, -1):
                assert capi.spgpuCooAssembleDeviceWith(C.pointer(h), None, None, entries, nnz, None, None, 0, 1, code, None, None, fill,
                                                       0) == capi.SPGPU_SUCCESS
                assert capi.spgpuCooAssembleValuesDeviceWith(C.pointer(h), None, entries, nnz, None, code, None, None, fill,
                                                             0) == capi.SPGPU_SUCCESS


def test_a_type_the_fills_cannot_add_is_refused_before_a_launch():
    h = capi.HandleStruct()
    for code in (capi.TYPE_INT, 5, -1):
        assert capi.spgpuCooAssembleValuesDevice(C.pointer(h), None, 10, 20, None, code, None, None) == capi.SPGPU_UNSUPPORTED
        for fill in (capi.ASSEMBLE_FILL_PLAIN, capi.ASSEMBLE_FILL_STAGED):
            assert capi.spgpuCooAssembleValuesDeviceWith(C.pointer(h), None, 10, 20, None, code, None, None, fill, 0) == capi.SPGPU_UNSUPPORTED
    assert capi.spgpuCooAssembleValuesDeviceWith(C.pointer(h), None, 10, 20, None, capi.TYPE_DOUBLE, None, None, 2, 0) == capi.SPGPU_UNSUPPORTED
    # a list with entries and no columns at all, or no scratch: refused before a launch
    unique = C.c_int(77)
    assert capi.spgpuCooAssemblePlanDevice(C.pointer(h), C.byref(unique), None, None, None, 5, 0, 10, None, None, 0, 0,
                                           None) == capi.SPGPU_UNSUPPORTED
    assert capi.spgpuCooAssemblePlanDevice(C.pointer(h), C.byref(unique), None, None, None, 5, 5, 10, None, None, 0, 0,
                                           None) == capi.SPGPU_UNSUPPORTED
    assert unique.value == 0


def test_the_tool_is_one_of_the_makefiles_tools():
    with open(os.path.join(ROOT, "Makefile")) as f:
        text = f.read()
    tools = re.search(r"^TOOLS\s*:=((?:.*\\\n)*.*)$", text, re.M).group(1)
    assert "tools/assemble_amd.bin" in tools.split() and os.path.exists(os.path.join(ROOT, "tools", "assemble_amd.c"))
