"""CPU: the HDIA / DIA SpMM of include/spgpu/ext/hdia_spmm.h at the drop-in boundary.  The header declares exactly the four calls,
libspgpu.so exports them and spgpu_amd.capi binds them with the SpMV's argument list followed by count, pitchX, pitchYZ; the header
is a C header of the ABI; without a handle's stream to launch on, the no-op cases return without touching a GPU."""
import ctypes as C
import os
import subprocess

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "hdia_spmm.h")
NAMES = {"spgpuShdiaspmmMv", "spgpuDhdiaspmmMv", "spgpuSdiaspmmMv", "spgpuDdiaspmmMv"}


def test_every_call_of_the_header_is_exported_and_bound():
    with open(HEADER) as f:
        declared = set(DECL.findall(f.read()))
    assert declared == NAMES, sorted(declared)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for name in sorted(declared):
        assert getattr(capi.lib, name) is not None
    assert set(capi.hdiaspmm_mv) == {"S", "D"} and set(capi.diaspmm_mv) == {"S", "D"}


def test_the_argument_lists_are_the_spmv_s_and_three_ints():
    """spgpu?hdiaspmv and spgpu?diaspmv take 12 arguments each (hdia.h, dia.h); count, pitchX and pitchYZ follow: 15."""
    for letter in "SD":
        for mm, mv in ((f"spgpu{letter}hdiaspmmMv", f"spgpu{letter}hdiaspmv"), (f"spgpu{letter}diaspmmMv", f"spgpu{letter}diaspmv")):
            (res, args), (res_mv, args_mv) = capi.DECLARED[mm], capi.DECLARED[mv]
            assert res is None and res_mv is None
            assert list(args) == list(args_mv) + [C.c_int] * 3 and len(args) == 15, mm


def test_the_header_is_a_c_header_of_the_abi(tmp_path):
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src
    assert "pitchX" in src and "pitchYZ" in src
    prog = tmp_path / "abi.c"
    prog.write_text('#include "spgpu/hdia.h"\n#include "spgpu/dia.h"\n#include "spgpu/ext/hdia_spmm.h"\n'
                    "int main(void){ void (*f)(spgpuHandle_t, double*, const double*, double, const double*, const int*, int, const int*,"
                    " int, int, const double*, double, int, int, int) = spgpuDhdiaspmmMv;\n"
                    " void (*g)(spgpuHandle_t, float*, const float*, float, const float*, const int*, int, int, int, int, const float*,"
                    " float, int, int, int) = spgpuSdiaspmmMv; return f == 0 || g == 0; }\n")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include", "-c", str(prog),
           "-o", str(tmp_path / "abi.o")]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_hdia_h_and_dia_h_point_to_the_header():
    for name in ("hdia.h", "dia.h"):
        with open(os.path.join(ROOT, "include", "spgpu", name)) as f:
            assert "ext/hdia_spmm.h" in f.read(), name


def test_no_rows_no_vectors_or_no_hack_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: rows <= 0, count <= 0 and hackSize <= 0 return first
    for letter in "SD":
        one, zero = capi.scalar(letter, 1), capi.scalar(letter, 0)
        for hack, rows, count in ((32, 0, 8), (32, 64, 0), (0, 64, 8), (32, -1, 8), (32, 64, -3), (-2, 64, 8), (32, 0, 1), (0, 64, 1)):
            capi.hdiaspmm_mv[letter](C.pointer(h), None, None, one, None, None, hack, None, rows, 64, None, zero, count, 64, 64)
            capi.diaspmm_mv[letter](C.pointer(h), None, None, one, None, None, hack, rows, 64, 3, None, zero, count, 64, 64)
