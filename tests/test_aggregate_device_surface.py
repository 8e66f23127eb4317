"""CPU: the aggregation calls of include/spgpu/ext/aggregate_device.h at the drop-in boundary.  The header compiles as plain C99 with
-Wall -Werror and declares the four calls; libspgpu.so exports them and spgpu_amd.capi binds them with the declared argument lists;
the shapes behind the calls stay out of the headers; the scratch size grows with the rows, is the same without rows as with none and
takes no share of the entries; without rows there is nothing to launch, so the no-op cases return without touching a GPU; what the
calls cannot do is refused before a launch; the header's text makes the contract's promises and the products' headers point to it."""
import ctypes as C
import glob
import os
import re
import subprocess

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "aggregate_device.h")
i32, ptr, Handle = capi.i32, capi.ptr, capi.Handle
HOST_INT = C.POINTER(i32)
SIGNATURES = {
    "spgpuCsrAggregateWorkBytes": (C.c_size_t, [i32]),
    "spgpuCsrStrengthDevice": (i32, [Handle, ptr, ptr, i32, ptr, ptr, ptr, i32, C.c_double, i32]),
    "spgpuCsrAggregateDevice": (i32, [Handle, HOST_INT, HOST_INT, ptr, ptr, i32, ptr, ptr, ptr, i32, ptr]),
    "spgpuCsrTentativeDevice": (i32, [Handle, ptr, ptr, ptr, i32, ptr, ptr, i32, i32]),
}
HELPERS = ("spgpuCsrAggregateDeviceWith", "spgpuCsrStrengthDeviceWith", "spgpuCsrAggregateDefaultShape")
C_TYPE = {"spgpuHandle_t": Handle, "int": i32, "spgpuType_t": i32, "double": C.c_double, "int*": ptr, "void*": ptr, "unsignedchar*": ptr}
ROWS = (-5, 0, 1, 63, 64, 65, 1023, 1024, 1025, 3000, 300000, 5000000, 2 ** 31 - 1)


def _declared_arguments(src, name):
    """The argument types of `name` as the header declares them, mapped to ctypes; '__host int*' is a host int the call returns."""
    text = re.search(r"^(?:spgpuStatus_t|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", src, re.M).group(1)
    out = []
    for arg in text.split(","):
        words = arg.replace("*", "* ").split()
        host = "__host" in words
        words = [w for w in words if w not in ("const", "__device", "__host")]
        kind = "".join(words[:-1])
        out.append(HOST_INT if host and kind == "int*" else C_TYPE[kind])
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


def test_the_header_compiles_as_c99_with_warnings_as_errors(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "spgpu/ext/aggregate_device.h"\n'
                   "int main(void){ spgpuHandle_t h = 0; (void)h; return spgpuCsrAggregateWorkBytes(0) ? 0 : 1; }\n")
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
    for promise in ("one square CSR matrix", "baseIndex 0 or 1", "columns need not ascend", "may lack its diagonal",
                    "the first stored (i, i)", "+0 if there is none", "real types only", "SPGPU_UNSUPPORTED before a launch",
                    "diagAbs[i] = d_i", "every operation is rounded separately", "t = (T)(theta*theta)", "in double on the host",
                    "lhs = a_ij*a_ij", "rhs = (t*d_i)*d_j", "(j != i) && lhs >= rhs", "a NaN on either side gives 0",
                    "theta = 0", "a stored zero included", "d_j is not read", "takes no scratch", "keeps no state", "captured",
                    "after the values changed in place", "one writer", "a repeated call gives the same bytes",
                    "strong == NULL", "every stored j != i", "hash(i) = lowbias32(i) >> 1", "0x7FEB352D", "0x846CA68B",
                    "(state, hash(i), i)", "OUT = 0 < UNDECIDED = 1 < ROOT = 2", "one 64-bit word", "All nodes start UNDECIDED",
                    "from buffer to buffer", "t1[i] = max(t0[i]", "t2[i] = max(t1[i]", "t2[i] == t0[i] becomes ROOT", "it becomes OUT",
                    "until no node is undecided", "always decides", "*roundsCount receives the number of rounds",
                    "by ascending row", "one exclusive scan", "two joining passes", "reading only the previous pass's array",
                    "the smallest such aggregate number", "every node is assigned after pass 2", "i -> j -> r",
                    "empty S(i) is a root", "a singleton", "0-based whatever baseIndex is", "a < *aggregatesCount",
                    "nothing beyond it is touched", "structurally symmetric", "the unique MIS-2", "descending tuple order",
                    "the rounds are the definition", "on the kernel shape or on the grid", "no floating-point atomics",
                    "about once per round", "about 32 bytes per row", "no share of the entries", "256-byte aligned", "may be freed",
                    "*aggregatesCount = 0 and *roundsCount = 0", "after the synchronise", "nothing read or written out of bounds",
                    "clamped out", "a flag is raised", "tRowPtr[i] = i + baseIndex", "aggregateOf[i] + baseIndex",
                    "the bits of candidate[i]", "candidate == NULL", "one ascending column per row", "spgpuCsrSpgemm*",
                    "spgpuCsrAdd*", "nothing launched", "waits for another workgroup"):
        assert promise in head, promise
    for neighbour in ("spgemm_device.h", "add_device.h"):
        with open(os.path.join(ROOT, "include", "spgpu", "ext", neighbour)) as f:
            assert "ext/aggregate_device.h" in f.read(), neighbour
    for document in ("DESIGN.md", "INTEGRATION.md", "README.md", os.path.join("profiles", "README.md")):
        with open(os.path.join(ROOT, document)) as f:
            assert "aggregate" in f.read(), document
    if not os.path.exists(os.path.join(ROOT, "profiles", "csr_aggregate_ab.json")):
        with open(os.path.join(ROOT, "README.md")) as f:
            assert "not yet timed on an MI355X" in f.read()


def test_the_shapes_behind_the_calls_stay_out_of_the_headers():
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
            assert "aggregate_rules.h" not in f.read(), header
    for header in glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")):          # nothing of it where test_capi_surface counts
        with open(header) as f:
            assert not [n for n in DECL.findall(f.read()) if "Aggregate" in n or "Strength" in n or "Tentative" in n], header
    with open(os.path.join(ROOT, "spgpu_amd", "csrc", "aggregate_device.hip")) as f:
        device = f.read()
    assert re.findall(r"\batomic[A-Z]\w*\s*\(", device) == ["atomicAdd("]            # the integer count of the undecided, nothing else
    assert "atomicAdd(&misc[0], left)" in device and "rocprim::" not in device       # the scratch is a function of the rows alone


def test_work_bytes_grow_with_the_rows_and_take_no_share_of_the_entries():
    sizes = [capi.spgpuCsrAggregateWorkBytes(n) for n in ROWS]
    assert sizes == sorted(sizes) and sizes[0] == sizes[1] > 0 and sizes[-1] > sizes[1]
    for n, size in zip(ROWS, sizes):
        assert size % 256 == 0
        assert 32 * max(n, 0) <= size <= 8192 + 33 * max(n, 0)                # about 32 bytes per row


def test_nothing_to_do_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: the calls return first
    count, rounds = C.c_int(77), C.c_int(77)
    for rows in (0, -3):
        for base in (0, 1):
            assert capi.spgpuCsrAggregateDevice(C.pointer(h), C.byref(count), C.byref(rounds), None, None, rows, None, None, None, base,
                                                None) == capi.SPGPU_SUCCESS
            assert count.value == 0 and rounds.value == 0
            count.value = rounds.value = 77
            for shape in (0, 1, 8, 3):
                assert capi.spgpuCsrAggregateDeviceWith(C.pointer(h), C.byref(count), C.byref(rounds), None, None, rows, None, None, None, base,
                                                        None, shape, 0) == capi.SPGPU_SUCCESS
                assert count.value == 0 and rounds.value == 0
                count.value = rounds.value = 77
            for code in (capi.TYPE_FLOAT, capi.TYPE_DOUBLE, capi.TYPE_COMPLEX_DOUBLE, capi.TYPE_INT, 5):
                assert capi.spgpuCsrStrengthDevice(C.pointer(h), None, None, rows, None, None, None, base, 0.25, code) == capi.SPGPU_SUCCESS
                assert capi.spgpuCsrTentativeDevice(C.pointer(h), None, None, None, rows, None, None, base, code) == capi.SPGPU_SUCCESS


def test_what_the_calls_cannot_do_is_refused_before_a_launch():
    h = capi.HandleStruct()
    somewhere = C.c_void_p(256)
    # strength: real types only, and both outputs
    strength = lambda code, strong=somewhere, diag=somewhere: (C.pointer(h), strong, diag, 10, somewhere, somewhere, somewhere, 0, 0.25, code)
    for code in (capi.TYPE_INT, capi.TYPE_COMPLEX_FLOAT, capi.TYPE_COMPLEX_DOUBLE, 5, -1):
        assert capi.spgpuCsrStrengthDevice(*strength(code)) == capi.SPGPU_UNSUPPORTED
        for shape in (1, 8, 32, 64):
            assert capi.spgpuCsrStrengthDeviceWith(*strength(code), shape, 0) == capi.SPGPU_UNSUPPORTED
    for code in (capi.TYPE_FLOAT, capi.TYPE_DOUBLE):
        assert capi.spgpuCsrStrengthDevice(*strength(code, strong=None)) == capi.SPGPU_UNSUPPORTED
        assert capi.spgpuCsrStrengthDevice(*strength(code, diag=None)) == capi.SPGPU_UNSUPPORTED
        for shape in (3, 24, 128):
            assert capi.spgpuCsrStrengthDeviceWith(*strength(code), shape, 0) == capi.SPGPU_UNSUPPORTED       # no such group
    # the tentative prolongator: the four value types, and every output
    tentative = lambda code, a=somewhere, b=somewhere, c=somewhere, of=somewhere: (C.pointer(h), a, b, c, 10, of, None, 1, code)
    for code in (capi.TYPE_INT, 5, -1):
        assert capi.spgpuCsrTentativeDevice(*tentative(code)) == capi.SPGPU_UNSUPPORTED
    for bad in (tentative(capi.TYPE_DOUBLE, a=None), tentative(capi.TYPE_FLOAT, b=None), tentative(capi.TYPE_COMPLEX_FLOAT, c=None),
                tentative(capi.TYPE_COMPLEX_DOUBLE, of=None)):
        assert capi.spgpuCsrTentativeDevice(*bad) == capi.SPGPU_UNSUPPORTED
    # the aggregation: rows to do and no scratch or no output
    count, rounds = C.c_int(77), C.c_int(77)
    aggregate = lambda of=somewhere, size=somewhere, row_ptr=somewhere, work=somewhere: (
        C.pointer(h), C.byref(count), C.byref(rounds), of, size, 5, row_ptr, somewhere, None, 0, work)
    for bad in (aggregate(of=None), aggregate(size=None), aggregate(row_ptr=None), aggregate(work=None)):
        count.value = rounds.value = 77
        assert capi.spgpuCsrAggregateDevice(*bad) == capi.SPGPU_UNSUPPORTED
        assert count.value == 0 and rounds.value == 0
    for shape in (3, 24, 128):
        count.value = rounds.value = 77
        assert capi.spgpuCsrAggregateDeviceWith(*aggregate(), shape, 0) == capi.SPGPU_UNSUPPORTED             # no such group
        assert count.value == 0 and rounds.value == 0
