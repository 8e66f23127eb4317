"""CPU: the multicolour-ordering calls of include/spgpu/ext/colour_device.h at the drop-in boundary.  The header compiles as plain C99
with -Wall -Werror and declares the five calls; libspgpu.so exports them and spgpu_amd.capi binds them with the declared argument
lists; the shapes behind the calls stay out of the headers; the scratch sizes grow with the rows, are the same without rows as with
none and take no share of the entries; without rows there is nothing to launch, so the no-op cases return without touching a GPU;
what the calls cannot do is refused before a launch; the header's text makes the contract's promises and the Plans' headers point to
it."""
import ctypes as C
import glob
import os
import re
import subprocess

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "colour_device.h")
i32, ptr, Handle = capi.i32, capi.ptr, capi.Handle
HOST_INT = C.POINTER(i32)
SIGNATURES = {
    "spgpuCsrColourWorkBytes": (C.c_size_t, [i32]),
    "spgpuCsrColourDevice": (i32, [Handle, HOST_INT, HOST_INT, ptr, i32, ptr, ptr, i32, ptr]),
    "spgpuCsrColourOrderDevice": (i32, [Handle, ptr, ptr, ptr, i32, i32, ptr, ptr]),
    "spgpuCsrPermuteWorkBytes": (C.c_size_t, [i32]),
    "spgpuCsrPermuteDevice": (i32, [Handle, ptr, ptr, ptr, i32, ptr, ptr, ptr, ptr, ptr, i32, i32, ptr]),
}
HELPERS = ("spgpuCsrColourDeviceWith", "spgpuCsrPermuteDeviceWith", "spgpuCsrColourDefaultShape")
C_TYPE = {"spgpuHandle_t": Handle, "int": i32, "spgpuType_t": i32, "int*": ptr, "void*": ptr}
ROWS = (-5, 0, 1, 63, 64, 65, 1023, 1024, 1025, 3000, 300000, 5000000, 2 ** 31 - 1)
DECLARATION = r"^(?:spgpuStatus_t|size_t)\s+%s\s*\(([^;]*)\)\s*;"


def _declared_arguments(src, name):
    """The argument types of `name` as the header declares them, mapped to ctypes; '__host int*' is a host int the call returns."""
    text = re.search(DECLARATION % name, src, re.M).group(1)
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
        for arg in re.search(DECLARATION % name, src, re.M).group(1).split(","):          # every pointer says where it lives
            assert "*" not in arg or "__device" in arg or "__host" in arg, (name, arg)
    assert src.count("/* NEW (no counterpart in the reference)") == src.count("/* NEW") == len(SIGNATURES)


def test_the_header_compiles_as_c99_with_warnings_as_errors(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "spgpu/ext/colour_device.h"\n'
                   "int main(void){ spgpuHandle_t h = 0; (void)h; return spgpuCsrColourWorkBytes(0) && spgpuCsrPermuteWorkBytes(0) ? 0 : 1; }\n")
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
    for promise in ("one square CSR matrix", "baseIndex 0 or 1", "columns need not ascend", "may be stored twice", "may lack its diagonal",
                    "a row may be empty", "the columns j != i of the stored entries", "(hash(i), i)", "hash(i) = lowbias32(i) >> 1",
                    "0x7FEB352D", "0x846CA68B", "with colour -1", "from buffer to buffer", "has c0[j] >= 0 or has a smaller tuple",
                    "the smallest c >= 0 that is not c0[j]", "Every other node keeps c0[i]", "until no node is uncoloured",
                    "is always ready", "at most rowsCount rounds", "*roundsCount receives the number of rounds",
                    "*coloursCount receives 1 + the largest colour", "0-based whatever baseIndex is", "structurally symmetric",
                    "a proper colouring", "descending tuple order", "never ready in the same round", "neighbours with larger tuples",
                    "the rounds are the definition", "costs levels afterwards, never a wrong solve",
                    "on the kernel shape or on the grid", "a repeated call gives the same bytes", "The only atomics are integer",
                    "no floating-point atomics", "about once per round", "cannot be captured", "256-byte aligned",
                    "no share of the entries", "may be freed", "*coloursCount = 0 and *roundsCount = 0",
                    "after the first round's synchronise", "nothing read or written out of bounds", "clamped out", "a flag is raised",
                    "by (colour, row) ascending", "inverse[order[k]] = k", "the number of rows of colours < c",
                    "nothing behind them is touched", "one stable split per bit of coloursCount - 1", "returns no host data",
                    "can be captured", "may share the colouring's", "row k of B is row order[k] of A",
                    "inverse[j - baseIndex] + baseIndex", "the exclusive scan of the gathered row lengths", "in ascending new column",
                    "in A's storage order", "strictly ascending", "quadratic in the row length", "4-, 8- or 16-byte words",
                    "-0.0 and NaN payloads survive", "SPGPU_UNSUPPORTED before a launch", "every output byte has one writer",
                    "after aValues changed in place", "B may not overlap A", "trusts order / inverse", "nothing launched",
                    "waits for another workgroup", "spgpuDgath(h, bp, rows, order, 0, b)", "spgpuDgath(h, x, rows, inverse, 0, xp)",
                    "A poor colouring costs levels, not answers"):
        assert promise in head, promise
    for neighbour in ("trsv_device.h", "ilu0_device.h"):
        with open(os.path.join(ROOT, "include", "spgpu", "ext", neighbour)) as f:
            assert "ext/colour_device.h" in f.read(), neighbour
    for document in ("DESIGN.md", "INTEGRATION.md", "README.md", os.path.join("profiles", "README.md")):
        with open(os.path.join(ROOT, document)) as f:
            text = f.read()
        assert "colour_device" in text or "csr_colour" in text, document
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "3.22" in f.read()


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
            assert "colour_rules.h" not in f.read(), header
    for header in glob.glob(os.path.join(ROOT, "include", "spgpu", "*.h")):          # nothing of it where test_capi_surface counts
        with open(header) as f:
            assert not [n for n in DECL.findall(f.read()) if "CsrColour" in n or "CsrPermute" in n], header
    with open(os.path.join(ROOT, "spgpu_amd", "csrc", "colour_device.hip")) as f:
        device = f.read()
    # the integer count of the uncoloured and the integer running maximum, nothing else; the scratch is a function of the rows alone
    assert re.findall(r"\batomic[A-Z]\w*\s*\(", device) == ["atomicAdd(", "atomicMax("]
    assert "atomicAdd(&misc[0], left)" in device and "atomicMax(&misc[2], top)" in device and "rocprim::" not in device


def test_work_bytes_grow_with_the_rows_and_take_no_share_of_the_entries():
    for size_of, per_row in ((capi.spgpuCsrColourWorkBytes, 16), (capi.spgpuCsrPermuteWorkBytes, 8)):
        sizes = [size_of(n) for n in ROWS]
        assert sizes == sorted(sizes) and sizes[0] == sizes[1] > 0 and sizes[-1] > sizes[1]
        for n, size in zip(ROWS, sizes):
            assert size % 256 == 0
            assert per_row * max(n, 0) <= size <= 8192 + (per_row + 1) * max(n, 0), (n, size)


def test_nothing_to_do_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: the calls return first
    colours, rounds = C.c_int(77), C.c_int(77)
    for rows in (0, -3):
        for base in (0, 1):
            assert capi.spgpuCsrColourDevice(C.pointer(h), C.byref(colours), C.byref(rounds), None, rows, None, None, base,
                                             None) == capi.SPGPU_SUCCESS
            assert colours.value == 0 and rounds.value == 0
            colours.value = rounds.value = 77
            for shape in (0, 1, 8, 3):
                assert capi.spgpuCsrColourDeviceWith(C.pointer(h), C.byref(colours), C.byref(rounds), None, rows, None, None, base, None,
                                                     shape, 0) == capi.SPGPU_SUCCESS
                assert colours.value == 0 and rounds.value == 0
                colours.value = rounds.value = 77
            for count in (0, 1, 5):
                assert capi.spgpuCsrColourOrderDevice(C.pointer(h), None, None, None, rows, count, None, None) == capi.SPGPU_SUCCESS
            for code in (capi.TYPE_FLOAT, capi.TYPE_DOUBLE, capi.TYPE_COMPLEX_DOUBLE, capi.TYPE_INT, 5):
                assert capi.spgpuCsrPermuteDevice(C.pointer(h), None, None, None, rows, None, None, None, None, None, base, code,
                                                  None) == capi.SPGPU_SUCCESS
                assert capi.spgpuCsrPermuteDeviceWith(C.pointer(h), None, None, None, rows, None, None, None, None, None, base, code,
                                                      None, 8, 1) == capi.SPGPU_SUCCESS


def test_what_the_calls_cannot_do_is_refused_before_a_launch():
    h = capi.HandleStruct()
    at = C.c_void_p(256)
    # the colouring: rows to do and no output, no matrix array or no scratch
    colours, rounds = C.c_int(77), C.c_int(77)
    colour = lambda of=at, row_ptr=at, cols=at, work=at: (C.pointer(h), C.byref(colours), C.byref(rounds), of, 5, row_ptr, cols, 0, work)
    for bad in (colour(of=None), colour(row_ptr=None), colour(cols=None), colour(work=None)):
        colours.value = rounds.value = 77
        assert capi.spgpuCsrColourDevice(*bad) == capi.SPGPU_UNSUPPORTED
        assert colours.value == 0 and rounds.value == 0
    for shape in (3, 24, 128):
        colours.value = rounds.value = 77
        assert capi.spgpuCsrColourDeviceWith(*colour(), shape, 0) == capi.SPGPU_UNSUPPORTED               # no such group
        assert colours.value == 0 and rounds.value == 0
    # the order: every array, and a count of colours that no colouring of these rows returns
    order = lambda a=at, b=at, c=at, count=3, of=at, work=at: (C.pointer(h), a, b, c, 5, count, of, work)
    for bad in (order(a=None), order(b=None), order(c=None), order(of=None), order(work=None), order(count=0), order(count=-1),
                order(count=6)):
        assert capi.spgpuCsrColourOrderDevice(*bad) == capi.SPGPU_UNSUPPORTED
    # the permutation: the four value types, every array, the known shapes
    def permute(code=capi.TYPE_DOUBLE, **missing):
        names = ("b_ptr", "b_cols", "b_vals", "order", "inverse", "a_ptr", "a_cols", "a_vals", "work")
        assert set(missing) <= set(names)
        a = {name: missing.get(name, at) for name in names}
        return (C.pointer(h), a["b_ptr"], a["b_cols"], a["b_vals"], 5, a["order"], a["inverse"], a["a_ptr"], a["a_cols"], a["a_vals"], 1,
                code, a["work"])
    for code in (capi.TYPE_INT, 5, -1):
        assert capi.spgpuCsrPermuteDevice(*permute(code)) == capi.SPGPU_UNSUPPORTED
        for shape in (1, 8, 32, 64):
            assert capi.spgpuCsrPermuteDeviceWith(*permute(code), shape, 0) == capi.SPGPU_UNSUPPORTED
    for code in (capi.TYPE_FLOAT, capi.TYPE_DOUBLE, capi.TYPE_COMPLEX_FLOAT, capi.TYPE_COMPLEX_DOUBLE):
        for name in ("b_ptr", "b_cols", "b_vals", "order", "inverse", "a_ptr", "a_cols", "a_vals", "work"):
            assert capi.spgpuCsrPermuteDevice(*permute(code, **{name: None})) == capi.SPGPU_UNSUPPORTED, name
        for shape in (3, 24, 128):
            assert capi.spgpuCsrPermuteDeviceWith(*permute(code), shape, 0) == capi.SPGPU_UNSUPPORTED         # no such group
