"""CPU: the calls of include/spgpu/ext/sweep_device.h at the drop-in boundary.  The header compiles as plain C99 with -Wall -Werror and
declares the four calls; libspgpu.so exports them and spgpu_amd.capi binds them with the declared argument lists; the shapes behind
the calls stay out of the headers; without rows there is nothing to launch, so the no-op cases return without touching a GPU; what
the calls cannot do is refused before a launch; the header's text makes the contract's promises and its neighbours point to it."""
import ctypes as C
import glob
import os
import re
import subprocess

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "sweep_device.h")
i32, ptr, Handle = capi.i32, capi.ptr, capi.Handle
HOST_INT = C.POINTER(i32)
SIGNATURES = {
    "spgpuCsrSweepWorkBytes": (C.c_size_t, [i32]),
    "spgpuCsrSweepPlanDevice": (i32, [Handle, HOST_INT, ptr, HOST_INT, i32, i32, ptr, ptr, ptr, ptr, ptr, i32, ptr]),
    "spgpuCsrSweepDevice": (i32, [Handle, ptr, ptr, i32, i32, ptr, HOST_INT, ptr, ptr, ptr, ptr, i32, i32, ptr, i32, i32]),
    "spgpuCsrResidualDevice": (i32, [Handle, ptr, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, i32]),
}
HELPERS = ("spgpuCsrSweepDeviceWith", "spgpuCsrResidualDeviceWith", "spgpuCsrSweepDefaultShape", "spgpuCsrSweepDefaultSolve",
           "spgpuCsrSweepChainWidth", "spgpuCsrSweepChainPasses", "spgpuCsrSweepLaunches")
C_TYPE = {"spgpuHandle_t": Handle, "int": i32, "spgpuType_t": i32, "int*": ptr, "void*": ptr}
DECLARATION = r"^(?:spgpuStatus_t|size_t)\s+%s\s*\(([^;]*)\)\s*;"


def _declared_arguments(src, name):
    """The argument types of `name` as the header declares them, mapped to ctypes; '__host int*' is a host int array."""
    text = re.search(DECLARATION % name, src, re.M).group(1)
    out = []
    for arg in text.split(","):
        words = arg.replace("*", "* ").split()
        host = "__host" in words
        words = [w for w in words if w not in ("const", "__device", "__host")]
        kind = "".join(words[:-1])
        out.append(HOST_INT if host and kind == "int*" else C_TYPE[kind])
    return out


def _argument_names(src, name):
    return [arg.replace("*", " ").split()[-1] for arg in re.search(DECLARATION % name, src, re.M).group(1).split(",")]


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
        for arg in re.search(DECLARATION % name, src, re.M).group(1).split(","):          # every pointer says where it lives
            assert "*" not in arg or "__device" in arg or "__host" in arg, (name, arg)
    assert src.count("/* NEW (no counterpart in the reference)") == src.count("/* NEW") == len(SIGNATURES)
    # the argument order the issue of this feature states
    assert _argument_names(src, "spgpuCsrSweepDevice") == ["handle", "x", "b", "rowsCount", "coloursCount", "order", "colourPtrHost", "diagPos",
                                                          "rowPtr", "colIndices", "values", "baseIndex", "direction", "omega", "valuesType",
                                                          "entriesCount"]
    assert _argument_names(src, "spgpuCsrResidualDevice") == ["handle", "r", "b", "x", "rowsCount", "rowPtr", "colIndices", "values", "baseIndex",
                                                             "valuesType", "entriesCount"]
    assert _argument_names(src, "spgpuCsrSweepPlanDevice") == ["handle", "entriesCount", "diagPos", "colourPtrHost", "rowsCount", "coloursCount",
                                                              "order", "colourPtr", "colourOf", "rowPtr", "colIndices", "baseIndex", "work"]
    assert (capi.SWEEP_FORWARD, capi.SWEEP_BACKWARD, capi.SWEEP_SYMMETRIC) == tuple(
        int(re.search(r"#define SPGPU_SWEEP_%s (\d)" % name, src).group(1)) for name in ("FORWARD", "BACKWARD", "SYMMETRIC"))


def test_the_header_compiles_as_c99_with_warnings_as_errors(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "spgpu/ext/sweep_device.h"\n'
                   "int main(void){ spgpuHandle_t h = 0; (void)h; return spgpuCsrSweepWorkBytes(0) && SPGPU_SWEEP_SYMMETRIC == 2 ? 0 : 1; }\n")
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
    for section in ("Matrix", "Values", "Refusals:", "Degenerate inputs", "State"):
        assert f" {section} " in head, section
    for promise in ("one square CSR matrix", "baseIndex 0 or 1", "need not ascend", "stores its diagonal exactly once", "subtracted twice",
                    "the meaning rIdx has elsewhere", "order[colourPtr[c] .. colourPtr[c + 1])", "the colour of column j is colourOf[j]",
                    "order == NULL", "colourPtr[c] <= k < colourPtr[c + 1]", "by bisection on colourPtr", "colourOf is not read and may be null",
                    "a 0-based entry index whatever baseIndex is", "nothing behind them is touched",
                    "*entriesCount = rowPtr[rowsCount] - baseIndex", "comparable byte for byte", "synchronises the stream once",
                    "not once per colour", "trusts `order`", "256-byte aligned", "may be freed", "with *entriesCount = 0",
                    "nothing read or written out of bounds", "clamped out", "a flag is raised",
                    "a column outside [baseIndex, baseIndex + rowsCount)", "with its diagonal stored twice",
                    "outside [0, coloursCount) when order != NULL", "whose two nodes have the same colour", "free of races",
                    "only in the direction of the stored entries", "UNSYMMETRIC pattern may fail this check", "A + A^T",
                    "spgpu/ext/add_device.h", "visits the colours 0 .. C-1", "the colours C-1 .. 0", "2C colour passes",
                    "the bytes of the two calls in that order", "acc = b_i", "in storage order, except the one at diagPos[i]",
                    "the product rounded, then the difference", "no fused multiply-add", "one correctly rounded division",
                    "omega == NULL (plain Gauss-Seidel): x_i = g", "HOST pointer to one element of the value type", "d = g - x_i",
                    "x_i = x_i + (omega * d)", "a different expression tree", "A zero pivot is not looked for".lower(), "six operations",
                    "do not depend on scheduling", "on the row shape, on the grid, on chaining", "the order of rows inside a colour",
                    "x may not overlap b", "needs no Plan and no colouring", "the diagonal included", "r == b exactly (in place) is allowed",
                    "r may not overlap x", "entriesCount <= 0 with rows to do still computes every r_i", "SPGPU_UNSUPPORTED before a launch",
                    "NOT MEASURED", "those of spgpu/ext/ilu0_device.h", "a colour of more than 256 rows is a launch of its own",
                    "one launch of one workgroup", "a symmetric sweep is two", "before the stream is touched", "an unknown direction",
                    "meant for a matrix that a Plan accepted", "allocates device memory or keeps state", "at call time, which is also capture",
                    "after b, x and values changed in place", "waits for another workgroup", "SPGPU_SWEEP_SYMMETRIC, NULL, SPGPU_TYPE_DOUBLE"):
        assert promise in head, promise
    for neighbour in ("trsv_device.h", "colour_device.h"):
        with open(os.path.join(ROOT, "include", "spgpu", "ext", neighbour)) as f:
            assert "ext/sweep_device.h" in f.read(), neighbour
    with open(os.path.join(ROOT, "include", "spgpu", "ext", "trsv_device.h")) as f:
        trsv = re.sub(r"\s*\n \*\s*", " ", f.read())
    assert "the whole of Gauss-Seidel and SSOR" not in trsv and "zero initial guess" in trsv
    for document in ("DESIGN.md", "INTEGRATION.md", "README.md", os.path.join("profiles", "README.md")):
        with open(os.path.join(ROOT, document)) as f:
            text = f.read()
        assert "sweep_device" in text or "csr_sweep" in text, document
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    assert "3.23" in design
    # the documents say which numbers are measured: the thresholds are ILU(0)'s until profiles/csr_sweep_ab.json moves them
    measured = os.path.exists(os.path.join(ROOT, "profiles", "csr_sweep_ab.json"))
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert measured or ("not measured" in design and "not measured" in readme)


def test_the_shapes_behind_the_calls_stay_out_of_the_headers():
    exported = exported_symbols()
    headers = glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")) + glob.glob(os.path.join(ROOT, "include", "spgpu", "ext", "*.h"))
    assert HEADER in headers
    for name in HELPERS:
        assert name in exported and name not in capi.DECLARED and getattr(capi.lib, name) is not None
        for header in headers:
            with open(header) as f:
                assert name not in f.read(), (name, header)
    for header in headers:
        with open(header) as f:
            assert "sweep_rules.h" not in f.read(), header
    for header in glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")):          # nothing of it where test_capi_surface counts
        with open(header) as f:
            assert not [n for n in DECL.findall(f.read()) if "CsrSweep" in n or "CsrResidual" in n], header
    assert capi.spgpuCsrSweepDeviceWith.argtypes == capi.spgpuCsrSweepDevice.argtypes + [i32, i32, i32]
    assert capi.spgpuCsrResidualDeviceWith.argtypes == capi.spgpuCsrResidualDevice.argtypes + [i32, i32]
    with open(os.path.join(ROOT, "spgpu_amd", "csrc", "sweep_device.hip")) as f:
        device = f.read()
    # no atomics, no library sort or scan, and the shared arithmetic and rules are included, not copied
    assert not re.findall(r"\batomic[A-Z]\w*\s*\(", device) and "rocprim::" not in device
    for used in ('#include "csr_shared.hip.h"', '#include "sweep_rules.h"', "exactSubMul(", "exactDiv(", "exactMulAdd(", "exactMul(", "lowerBound(",
                 "forValueType(", "forEachSweepSegment("):
        assert used in device, used


def test_work_bytes_are_the_same_for_every_number_of_rows():
    sizes = [capi.spgpuCsrSweepWorkBytes(n) for n in (-5, 0, 1, 1000, 5000000, 2 ** 31 - 1)]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] > 0 and all(s % 256 == 0 for s in sizes)


def test_nothing_to_do_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: the calls return first
    entries = C.c_int(77)
    for rows in (0, -3):
        for base in (0, 1):
            assert capi.spgpuCsrSweepPlanDevice(C.pointer(h), C.byref(entries), None, None, rows, 4, None, None, None, None, None, base,
                                                None) == capi.SPGPU_SUCCESS
            assert entries.value == 0
            entries.value = 77
            for code in (capi.TYPE_DOUBLE, capi.TYPE_INT, 9):
                assert capi.spgpuCsrResidualDevice(C.pointer(h), None, None, None, rows, None, None, None, base, code, 0) == capi.SPGPU_SUCCESS
                assert capi.spgpuCsrResidualDeviceWith(C.pointer(h), None, None, None, rows, None, None, None, base, code, 0, 3,
                                                       1) == capi.SPGPU_SUCCESS
    for rows, colours in ((0, 4), (-3, 4), (5, 0), (5, -1)):
        for direction in (0, 1, 2, 9):
            assert capi.spgpuCsrSweepDevice(C.pointer(h), None, None, rows, colours, None, None, None, None, None, None, 0, direction, None,
                                            capi.TYPE_DOUBLE, 0) == capi.SPGPU_SUCCESS
            assert capi.spgpuCsrSweepDeviceWith(C.pointer(h), None, None, rows, colours, None, None, None, None, None, None, 0, direction, None,
                                                capi.TYPE_DOUBLE, 0, 3, 5, 1) == capi.SPGPU_SUCCESS


def test_what_the_calls_cannot_do_is_refused_before_a_launch():
    h = capi.HandleStruct()
    at = C.c_void_p(256)
    host = (C.c_int * 3)(0, 3, 5)
    entries = C.c_int(77)
    def plan(colours=2, host_ptr=host, **missing):
        a = {k: missing.get(k, at) for k in ("diag", "order", "cptr", "cof", "ptr", "col", "work")}
        return (C.pointer(h), C.byref(entries), a["diag"], host_ptr, 5, colours, a["order"], a["cptr"], a["cof"], a["ptr"], a["col"], 0, a["work"])
    for bad in (plan(colours=0), plan(colours=-2), plan(host_ptr=None), plan(diag=None), plan(cptr=None), plan(cof=None), plan(ptr=None),
                plan(col=None), plan(work=None)):
        entries.value = 77
        assert capi.spgpuCsrSweepPlanDevice(*bad) == capi.SPGPU_UNSUPPORTED
        assert entries.value == 0
    def sweep(direction=capi.SWEEP_SYMMETRIC, code=capi.TYPE_DOUBLE, host_ptr=host, **missing):
        a = {k: missing.get(k, at) for k in ("x", "b", "diag", "ptr", "col", "val")}
        return (C.pointer(h), a["x"], a["b"], 5, 2, None, host_ptr, a["diag"], a["ptr"], a["col"], a["val"], 1, direction, None, code, 13)
    for bad in (sweep(direction=3), sweep(direction=-1), sweep(code=capi.TYPE_INT), sweep(code=7), sweep(host_ptr=None), sweep(x=None),
                sweep(b=None), sweep(diag=None), sweep(ptr=None), sweep(col=None), sweep(val=None), sweep(host_ptr=(C.c_int * 3)(0, 3, 6)),
                sweep(host_ptr=(C.c_int * 3)(0, 6, 5)), sweep(host_ptr=(C.c_int * 3)(1, 3, 5))):
        assert capi.spgpuCsrSweepDevice(*bad) == capi.SPGPU_UNSUPPORTED
    for run in ((3, 0, 0), (24, 1, 0), (128, 0, 0), (1, 2, 0)):
        assert capi.spgpuCsrSweepDeviceWith(*sweep(), *run) == capi.SPGPU_UNSUPPORTED
    def residual(code=capi.TYPE_DOUBLE, **missing):
        a = {k: missing.get(k, at) for k in ("r", "b", "x", "ptr", "col", "val")}
        return (C.pointer(h), a["r"], a["b"], a["x"], 5, a["ptr"], a["col"], a["val"], 0, code, 13)
    for bad in (residual(code=capi.TYPE_INT), residual(code=9), residual(r=None), residual(b=None), residual(x=None), residual(ptr=None),
                residual(col=None), residual(val=None)):
        assert capi.spgpuCsrResidualDevice(*bad) == capi.SPGPU_UNSUPPORTED
    for shape in (3, 24, 128):
        assert capi.spgpuCsrResidualDeviceWith(*residual(), shape, 0) == capi.SPGPU_UNSUPPORTED
