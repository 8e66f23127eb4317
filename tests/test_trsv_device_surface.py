"""CPU: the triangular-solve calls of include/spgpu/ext/trsv_device.h at the drop-in boundary.  The header compiles as plain C99 with
-Wall -Werror and declares the three calls; libspgpu.so exports them and spgpu_amd.capi binds them with the declared argument lists;
the solves behind the call, the default-solve report and the chain width stay out of the headers; the scratch size grows with the
rows and is the same without rows as with none; without rows or levels there is nothing to launch, so the no-op cases return without
touching a GPU; a type the solve cannot divide is refused before a launch; the header's text makes the contract's promises and its
three neighbours point to it; and the plain-C tool is one of the Makefile's TOOLS."""
import ctypes as C
import glob
import os
import re
import subprocess

from spgpu_amd import capi
from test_add_device_surface import _declared_arguments
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "trsv_device.h")
i32, ptr, Handle = capi.i32, capi.ptr, capi.Handle
HOST_INT = C.POINTER(i32)
SIGNATURES = {
    "spgpuCsrTrsvWorkBytes": (C.c_size_t, [i32]),
    "spgpuCsrTrsvPlanDevice": (i32, [Handle, HOST_INT, ptr, ptr, HOST_INT, i32, ptr, ptr, i32, i32, i32, ptr]),
    "spgpuCsrTrsvDevice": (i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, HOST_INT, ptr, ptr, ptr, i32, i32, i32, i32]),
}
HELPERS = ("spgpuCsrTrsvDeviceWith", "spgpuCsrTrsvDefaultSolve", "spgpuCsrTrsvChainWidth")
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
    for name, value in (("SPGPU_TRSV_LOWER", capi.TRSV_LOWER), ("SPGPU_TRSV_UPPER", capi.TRSV_UPPER),
                        ("SPGPU_TRSV_DIAG_STORED", capi.TRSV_DIAG_STORED), ("SPGPU_TRSV_DIAG_UNIT", capi.TRSV_DIAG_UNIT)):
        assert re.search(rf"^#define {name} {value}$", src, re.M), name
    assert capi.TRSV_LOWER != capi.TRSV_UPPER and capi.TRSV_DIAG_STORED != capi.TRSV_DIAG_UNIT


def test_the_header_compiles_as_c99_with_warnings_as_errors(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "spgpu/ext/trsv_device.h"\n'
                   "int main(void){ spgpuHandle_t h = 0; (void)h; return spgpuCsrTrsvWorkBytes(0) && SPGPU_TRSV_UPPER && SPGPU_TRSV_DIAG_UNIT ? 0 : 1; }\n")
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
    for promise in ("one square CSR matrix", "holding the whole of A", "baseIndex 0 or 1", "never read as values", "never count as dependencies",
                    "need not ascend", "a stored diagonal is never read", "exactly once", "symbolic", "a stored zero is a dependency",
                    "(level, row index) ascending", "0-based row numbers", "levelPtr[*levelsCount] == rowsCount", "Neither level array is touched beyond",
                    "byte for byte", "acc = b_i", "in storage order", "acc = acc - (a_ij * x_j)", "the product rounded, then the difference",
                    "no fused multiply-add", "one correctly rounded division", "moves b_i's bits", "-0.0 included", "zero pivot is not looked for",
                    "IEEE division decides", "ar*xr - ai*xi", "ar*xi + ai*xr", "six operations", "componentwise",
                    "den = (dr*dr) + (di*di)", "((nr*dr) + (ni*di)) / den", "((ni*dr) - (nr*di)) / den", "NOT safe against overflow",
                    "this restatement is the law", "one writer", "no atomics", "SPGPU_UNSUPPORTED", "before a launch", "x == b exactly",
                    "any other overlap is not", "*levelsCount = 0", "after its synchronise", "clamped", "a missing diagonal",
                    "a diagonal stored twice", "nothing launched", "before touching the stream", "never synchronises", "allocates nothing",
                    "keeps no state", "at call time", "capture time", "captured", "may be freed", "waits for another workgroup",
                    "numpy can restate"):
        assert promise in head, promise
    for neighbour in ("precond.h", "add_device.h", "spgemm_device.h"):
        with open(os.path.join(ROOT, "include", "spgpu", "ext", neighbour)) as f:
            assert "ext/trsv_device.h" in f.read(), neighbour


def test_the_solves_behind_the_call_stay_out_of_the_headers():
    exported = exported_symbols()
    headers = glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")) + glob.glob(os.path.join(ROOT, "include", "spgpu", "ext", "*.h"))
    assert HEADER in headers
    for name in HELPERS:
        assert name in exported and name not in capi.DECLARED
        for header in headers:
            with open(header) as f:
                assert name not in f.read(), (name, header)
    assert capi.TRSV_SOLVE_DEFAULT in (capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED)
    assert capi.TRSV_CHAIN_WIDTH >= 64 and capi.TRSV_CHAIN_WIDTH % 64 == 0            # whole wavefronts of one workgroup
    for header in glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")):          # nothing of the solve where test_capi_surface counts
        with open(header) as f:
            assert not [n for n in DECL.findall(f.read()) if "CsrTrsv" in n], header


def test_work_bytes_grow_with_the_rows_and_are_the_same_without_rows_as_with_none():
    sizes = [capi.spgpuCsrTrsvWorkBytes(n) for n in ROWS]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] > 0 and sizes[-1] > sizes[1]
    for n, size in zip(ROWS, sizes):
        assert size >= 16 + 16 * max(n, 0)                                    # the level and three lists of the rows
        assert size <= 4096 + 20 * max(n, 0)                                  # and no share of the entries


def test_nothing_to_do_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: the calls return first
    count = C.c_int(77)
    for rows in (0, -3):
        for side in (capi.TRSV_LOWER, capi.TRSV_UPPER, 9):
            assert capi.spgpuCsrTrsvPlanDevice(C.pointer(h), C.byref(count), None, None, None, rows, None, None, 1, side, capi.TRSV_DIAG_UNIT,
                                               None) == capi.SPGPU_SUCCESS
            assert count.value == 0
            count.value = 77
    for rows, levels in ((0, 5), (-1, 5), (10, 0), (10, -2)):
        for code in (capi.TYPE_FLOAT, capi.TYPE_COMPLEX_DOUBLE, capi.TYPE_INT, 5):
            args = (C.pointer(h), None, None, rows, levels, None, None, None, None, None, None, 1, capi.TRSV_LOWER, capi.TRSV_DIAG_STORED, code)
            assert capi.spgpuCsrTrsvDevice(*args) == capi.SPGPU_SUCCESS
            for solve in (capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED, -1, 2):
                assert capi.spgpuCsrTrsvDeviceWith(*args, solve, 0) == capi.SPGPU_SUCCESS


def test_what_the_solve_cannot_do_is_refused_before_a_launch():
    h = capi.HandleStruct()
    level_ptr = (i32 * 2)(0, 10)
    somewhere = C.c_void_p(256)
    call = lambda code, side=capi.TRSV_LOWER, diag=capi.TRSV_DIAG_STORED, x=somewhere, b=somewhere, host=level_ptr: (
        C.pointer(h), x, b, 10, 1, None, None, host, None, None, None, 0, side, diag, code)
    for code in (capi.TYPE_INT, 5, -1):
        assert capi.spgpuCsrTrsvDevice(*call(code)) == capi.SPGPU_UNSUPPORTED
        for solve in (capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED):
            assert capi.spgpuCsrTrsvDeviceWith(*call(code), solve, 0) == capi.SPGPU_UNSUPPORTED
    ok = capi.TYPE_DOUBLE
    assert capi.spgpuCsrTrsvDeviceWith(*call(ok), 2, 0) == capi.SPGPU_UNSUPPORTED                      # no such solve
    assert capi.spgpuCsrTrsvDevice(*call(ok, side=2)) == capi.SPGPU_UNSUPPORTED                        # no such side
    assert capi.spgpuCsrTrsvDevice(*call(ok, diag=-1)) == capi.SPGPU_UNSUPPORTED                       # no such diagonal
    assert capi.spgpuCsrTrsvDevice(*call(ok, x=None)) == capi.SPGPU_UNSUPPORTED                        # no destination
    assert capi.spgpuCsrTrsvDevice(*call(ok, b=None)) == capi.SPGPU_UNSUPPORTED                        # no right-hand side
    assert capi.spgpuCsrTrsvDevice(*call(ok, host=None)) == capi.SPGPU_UNSUPPORTED                     # no levels to read
    # rows to analyse and no scratch, no output, or no such triangle: refused before a launch
    count = C.c_int(77)
    host = (i32 * 6)()
    plan = lambda order=somewhere, lp=somewhere, hp=host, side=capi.TRSV_UPPER, diag=capi.TRSV_DIAG_UNIT, work=somewhere: (
        C.pointer(h), C.byref(count), order, lp, hp, 5, None, None, 0, side, diag, work)
    for bad in (plan(order=None), plan(lp=None), plan(hp=None), plan(side=2), plan(diag=2), plan(work=None)):
        count.value = 77
        assert capi.spgpuCsrTrsvPlanDevice(*bad) == capi.SPGPU_UNSUPPORTED
        assert count.value == 0


def test_the_tool_is_one_of_the_makefiles_tools():
    with open(os.path.join(ROOT, "Makefile")) as f:
        text = f.read()
    tools = re.search(r"^TOOLS\s*:=((?:.*\\\n)*.*)$", text, re.M).group(1)
    assert "tools/gs_amd.bin" in tools.split() and os.path.exists(os.path.join(ROOT, "tools", "gs_amd.c"))
    assert "fast-math" not in text and "ffast" not in text and "FLAGS_trsv_device" not in text   # correctly rounded division: hipcc's default
