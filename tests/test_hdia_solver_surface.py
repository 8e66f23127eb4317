"""CPU: the fused SpMV + dot calls for HDIA and DIA matrices (include/spgpu/ext/hdia_solver.h) at the drop-in boundary.  The header
declares exactly the four calls, libspgpu.so exports them and spgpu_amd.capi binds them with [result, w] followed by the argument
list of the matching SpMV; the header is a C header of the ABI; the headers of include/spgpu/*.h declare what they declared.  (The
calls write *result = 0 through the dot's second stage even without rows: there is no call here that runs without a GPU.)"""
import os
import subprocess

from spgpu_amd import capi
from test_capi_surface import DECL, declared_functions, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "hdia_solver.h")
CALLS = {"hdiaspmvDotDevice": ("hdiaspmv_dot_device", "hdiaspmv"), "diaspmvDotDevice": ("diaspmv_dot_device", "diaspmv")}
NAMES = {f"spgpu{letter}{call}" for letter in "SD" for call in CALLS}


def test_every_call_of_the_header_is_exported_and_bound():
    with open(HEADER) as f:
        declared = set(DECL.findall(f.read()))
    assert len(NAMES) == 4 and declared == NAMES, sorted(declared ^ NAMES)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for call, (table, _) in CALLS.items():
        assert set(getattr(capi, table)) == {"S", "D"}, table
        for letter in "SD":
            assert getattr(capi.lib, f"spgpu{letter}{call}") is not None
            assert capi.DECLARED[f"spgpu{letter}{call}"][0] is None


def test_the_argument_lists_are_result_and_w_then_those_of_the_spmv():
    for letter in "SD":
        for call, (_, spmv) in CALLS.items():
            args, plain = capi.DECLARED[f"spgpu{letter}{call}"][1], capi.DECLARED[f"spgpu{letter}{spmv}"][1]
            assert list(args) == [plain[0], capi.ptr, capi.ptr] + list(plain[1:]), call


def test_the_header_is_a_c_header_of_the_abi(tmp_path):
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src
    prog = tmp_path / "abi.c"
    prog.write_text('#include "spgpu/ext/hdia_solver.h"\n'
                    "int main(void){ void (*f)(spgpuHandle_t, double*, const double*, double*, const double*, double, const double*,"
                    " const int*, int, const int*, int, int, const double*, double) = spgpuDhdiaspmvDotDevice;\n"
                    " void (*g)(spgpuHandle_t, float*, const float*, float*, const float*, float, const float*, const int*, int, int, int,"
                    " int, const float*, float) = spgpuSdiaspmvDotDevice;\n"
                    " void (*s)(spgpuHandle_t, float*, const float*, float*, const float*, float, const float*, const int*, int,"
                    " const int*, int, int, const float*, float) = spgpuShdiaspmvDotDevice;\n"
                    " void (*d)(spgpuHandle_t, double*, const double*, double*, const double*, double, const double*, const int*, int, int,"
                    " int, int, const double*, double) = spgpuDdiaspmvDotDevice;\n"
                    " return f == 0 || g == 0 || s == 0 || d == 0; }\n")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include", "-c", str(prog),
           "-o", str(tmp_path / "abi.o")]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_hdia_h_dia_h_and_device_scalars_h_point_to_the_header():
    for name in ("hdia.h", "dia.h", "device_scalars.h"):
        with open(os.path.join(ROOT, "include", "spgpu", name)) as f:
            assert "ext/hdia_solver.h" in f.read(), name


def test_the_headers_of_the_reference_surface_declare_what_they_declared():
    assert len(declared_functions()) == 199
    assert not NAMES & declared_functions()
