"""CPU: the ILU(0) calls of include/spgpu/ext/ilu0_device.h at the drop-in boundary.  The header compiles as plain C99 with -Wall
-Werror and declares the three calls; libspgpu.so exports them and spgpu_amd.capi binds them with the declared argument lists; the
shapes behind the call and the constants of the rules stay out of the headers; the scratch size grows with the rows and is the same
without rows as with none; without rows or levels there is nothing to launch, so the no-op cases return without touching a GPU; a
type the factorisation cannot divide is refused before a launch; the header's text makes the contract's promises and the comments
that sent the user to a vendor ILU point to it."""
import ctypes as C
import glob
import os
import re
import subprocess

from spgpu_amd import capi
from test_add_device_surface import _declared_arguments
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "ilu0_device.h")
i32, ptr, Handle = capi.i32, capi.ptr, capi.Handle
HOST_INT = C.POINTER(i32)
SIGNATURES = {
    "spgpuCsrIlu0WorkBytes": (C.c_size_t, [i32]),
    "spgpuCsrIlu0PlanDevice": (i32, [Handle, HOST_INT, ptr, ptr, HOST_INT, ptr, i32, ptr, ptr, i32, ptr]),
    "spgpuCsrIlu0Device": (i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, HOST_INT, ptr, ptr, ptr, i32, i32]),
}
HELPERS = ("spgpuCsrIlu0DeviceWith", "spgpuCsrIlu0DefaultShape", "spgpuCsrIlu0DefaultSolve", "spgpuCsrIlu0ChainWidth",
           "spgpuCsrIlu0ShapeConstant")
ROWS = (-5, 0, 1, 63, 64, 65, 1023, 1024, 1025, 3000, 300000, 5000000, 2 ** 31 - 1)


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


def test_the_header_compiles_as_c99_with_warnings_as_errors(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "spgpu/ext/ilu0_device.h"\n'
                   "int main(void){ spgpuHandle_t h = 0; (void)h; return spgpuCsrIlu0WorkBytes(0) ? 0 : 1; }\n")
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
    head = re.sub(r"\s*\n \*\s*", " ", src.split("#include")[0])          # the comment as running text
    for promise in ("one square CSR matrix", "baseIndex 0 or 1", "strictly ascending columns", "every row stores its diagonal",
                    "once per pattern", "synchronises the stream", "byte for byte", "SPGPU_TRSV_LOWER, SPGPU_TRSV_DIAG_STORED",
                    "SPGPU_TRSV_LOWER and SPGPU_TRSV_DIAG_UNIT for the L solve", "THE EXTRA SLOT", "levelPtrHost[*levelsCount + 1]",
                    "rowsCount + 2 ints", "without a synchronise", "never the bytes", "diagPos[i]", "0-based position", "may be freed",
                    "*levelsCount = 0", "after its synchronise", "nothing read or written out of bounds",
                    "a column outside [baseIndex, baseIndex + rowsCount)", "does not ascend strictly", "repeats a column",
                    "a missing diagonal", "lu starts as a copy of a", "in ascending k", "lu_ik = lu_ik / lu_kk",
                    "one correctly rounded division", "in ascending j", "lu_ij = lu_ij - (lu_ik * lu_kj)",
                    "the product rounded, then the difference", "no fused multiply-add", "there is no fill",
                    "level(k) < level(i)", "unit L strictly below the diagonal", "U on and above it", "moves its bits", "-0.0 included",
                    "zero pivot is not looked for", "IEEE division decides", "ar*xr - ai*xi", "ar*xi + ai*xr", "six operations",
                    "den = (dr*dr) + (di*di)", "((nr*dr) + (ni*di)) / den", "((ni*dr) - (nr*di)) / den", "NOT safe against overflow",
                    "this restatement is the law", "one writer", "at most once", "no atomics", "on the kernel shape or on the grid",
                    "SPGPU_UNSUPPORTED", "before a launch", "luValues == aValues exactly", "any other overlap is not",
                    "aValues is left untouched", "nothing launched", "before touching the stream", "never synchronises",
                    "allocates nothing", "keeps no state", "at call time", "capture time", "captured", "after aValues changed in place",
                    "waits for another workgroup", "__syncthreads()"):
        assert promise in head, promise
    for neighbour in ("precond.h", "trsv_device.h"):
        with open(os.path.join(ROOT, "include", "spgpu", "ext", neighbour)) as f:
            assert "ext/ilu0_device.h" in f.read(), neighbour
    for document in ("DESIGN.md", "INTEGRATION.md", "README.md", os.path.join("profiles", "README.md")):
        with open(os.path.join(ROOT, document)) as f:
            assert "ilu0" in f.read(), document


def test_the_shapes_behind_the_call_stay_out_of_the_headers():
    exported = exported_symbols()
    headers = glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")) + glob.glob(os.path.join(ROOT, "include", "spgpu", "ext", "*.h"))
    assert HEADER in headers
    for name in HELPERS:
        assert name in exported and name not in capi.DECLARED
        for header in headers:
            with open(header) as f:
                assert name not in f.read(), (name, header)
    for header in headers:
        with open(header) as f:
            assert "ilu0_rules.h" not in f.read(), header
    with open(os.path.join(ROOT, "spgpu_amd", "csrc", "ilu0_rules.h")) as f:
        rules = f.read()
    assert "hip/" not in rules and '#include "trsv_rules.h"' in rules                # plain host C++
    for header in glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")):          # nothing of it where test_capi_surface counts
        with open(header) as f:
            assert not [n for n in DECL.findall(f.read()) if "Ilu0" in n], header
    with open(os.path.join(ROOT, "Makefile")) as f:
        text = f.read()
    assert "fast-math" not in text and "ffast" not in text and "FLAGS_ilu0_device" not in text   # correctly rounded division: hipcc's default


def test_work_bytes_grow_with_the_rows_and_are_the_same_without_rows_as_with_none():
    sizes = [capi.spgpuCsrIlu0WorkBytes(n) for n in ROWS]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] > 0 and sizes[-1] > sizes[1]
    for n, size in zip(ROWS, sizes):
        assert size >= 256 + capi.spgpuCsrTrsvWorkBytes(n)                    # its own words and the Plan of the lower solve
        assert size <= 4096 + 20 * max(n, 0)                                  # and no share of the entries


def test_nothing_to_do_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: the calls return first
    count = C.c_int(77)
    for rows in (0, -3):
        assert capi.spgpuCsrIlu0PlanDevice(C.pointer(h), C.byref(count), None, None, None, None, rows, None, None, 1, None) == capi.SPGPU_SUCCESS
        assert count.value == 0
        count.value = 77
    for rows, levels in ((0, 5), (-1, 5), (10, 0), (10, -2)):
        for code in (capi.TYPE_FLOAT, capi.TYPE_COMPLEX_DOUBLE, capi.TYPE_INT, 5):
            args = (C.pointer(h), None, None, rows, levels, None, None, None, None, None, None, 1, code)
            assert capi.spgpuCsrIlu0Device(*args) == capi.SPGPU_SUCCESS
            for shape in (0, capi.ILU0_SHAPE_THREAD, 8, 3):
                for solve in (capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED, -1, 2):
                    assert capi.spgpuCsrIlu0DeviceWith(*args, shape, solve, 0) == capi.SPGPU_SUCCESS


def test_what_the_factorisation_cannot_do_is_refused_before_a_launch():
    h = capi.HandleStruct()
    level_ptr = (i32 * 3)(0, 10, 70)
    somewhere = C.c_void_p(256)
    call = lambda code, lu=somewhere, a=somewhere, host=level_ptr: (C.pointer(h), lu, a, 10, 1, None, None, host, None, None, None, 0, code)
    for code in (capi.TYPE_INT, 5, -1):
        assert capi.spgpuCsrIlu0Device(*call(code)) == capi.SPGPU_UNSUPPORTED
        for shape in capi.ILU0_SHAPES:
            for solve in (capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED):
                assert capi.spgpuCsrIlu0DeviceWith(*call(code), shape, solve, 0) == capi.SPGPU_UNSUPPORTED
    ok = capi.TYPE_DOUBLE
    assert capi.spgpuCsrIlu0DeviceWith(*call(ok), 0, 2, 0) == capi.SPGPU_UNSUPPORTED                   # no such segmenting
    for shape in (3, 24, 128):
        assert capi.spgpuCsrIlu0DeviceWith(*call(ok), shape, 0, 0) == capi.SPGPU_UNSUPPORTED           # no such group
    assert capi.spgpuCsrIlu0Device(*call(ok, lu=None)) == capi.SPGPU_UNSUPPORTED                       # no destination
    assert capi.spgpuCsrIlu0Device(*call(ok, a=None)) == capi.SPGPU_UNSUPPORTED                        # no matrix
    assert capi.spgpuCsrIlu0Device(*call(ok, host=None)) == capi.SPGPU_UNSUPPORTED                     # no levels to read
    # rows to analyse and no scratch or no output: refused before a launch
    count = C.c_int(77)
    host = (i32 * 7)()
    plan = lambda order=somewhere, lp=somewhere, hp=host, dp=somewhere, work=somewhere: (
        C.pointer(h), C.byref(count), order, lp, hp, dp, 5, None, None, 0, work)
    for bad in (plan(order=None), plan(lp=None), plan(hp=None), plan(dp=None), plan(work=None)):
        count.value = 77
        assert capi.spgpuCsrIlu0PlanDevice(*bad) == capi.SPGPU_UNSUPPORTED
        assert count.value == 0
