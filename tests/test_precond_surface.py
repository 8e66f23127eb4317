"""CPU: the Jacobi preconditioning calls (include/spgpu/ext/precond.h) at the drop-in boundary.  The header declares exactly the
fourteen calls, libspgpu.so exports them and spgpu_amd.capi binds them; the header is a C header of the ABI; the m-forms take the
single-vector argument lists followed by count and pitch; without rows or vectors the calls return without touching a GPU."""
import ctypes as C
import os
import subprocess

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "precond.h")
TABLES = {"hellDiag": "hell_diag", "ellDiag": "ell_diag", "hdiaDiag": "hdia_diag", "axyDotDevice": "axy_dot_device",
          "axpbyPairAxyDotDevice": "axpby_pair_axy_dot_device", "maxyDotDevice": "maxy_dot_device",
          "maxpbyPairAxyDotDevice": "maxpby_pair_axy_dot_device"}
NAMES = {f"spgpu{letter}{call}" for letter in "SD" for call in TABLES}


def test_every_call_of_the_header_is_exported_and_bound():
    with open(HEADER) as f:
        declared = set(DECL.findall(f.read()))
    assert len(NAMES) == 14 and declared == NAMES, sorted(declared ^ NAMES)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for name in sorted(declared):
        assert getattr(capi.lib, name) is not None
    for call, table in TABLES.items():
        assert set(getattr(capi, table)) == {"S", "D"}, table
        for letter in "SD":
            assert capi.DECLARED[f"spgpu{letter}{call}"][0] is None


def test_the_m_forms_take_the_single_vector_lists_and_the_layout():
    for letter in "SD":
        for call in ("axyDotDevice", "axpbyPairAxyDotDevice"):
            args, single = capi.DECLARED[f"spgpu{letter}m{call}"][1], capi.DECLARED[f"spgpu{letter}{call}"][1]
            assert list(args) == list(single) + [C.c_int] * 2, call
        # the pair call is spgpu?axpbyPairDotDevice with w and d in front of the coefficient
        pair, plain = capi.DECLARED[f"spgpu{letter}axpbyPairAxyDotDevice"][1], capi.DECLARED[f"spgpu{letter}axpbyPairDotDevice"][1]
        assert list(pair) == list(plain[:-2]) + [capi.ptr, capi.ptr] + list(plain[-2:])


def test_the_matrix_arguments_lead_as_in_the_matching_spmv():
    """(handle, d, <the spmv's arguments from cM / dM up to the one before x, without rIdx and avgNnzPerRow>, [baseIndex,] invert)."""
    for letter in "SD":
        hell, ell, hdia = (capi.DECLARED[f"spgpu{letter}{f}spmv"][1] for f in ("hell", "ell", "hdia"))
        # hellspmv: handle z y alpha | cM rP hackSize hackOffsets rS | rIdx avgNnz | rows | x beta baseIndex
        assert list(capi.DECLARED[f"spgpu{letter}hellDiag"][1]) == [capi.Handle, capi.ptr] + list(hell[4:9]) + [hell[11], hell[14], capi.i32]
        # ellspmv: handle z y alpha | cM rP cMPitch rPPitch rS | rIdx avgNnz | maxNnz rows | x beta baseIndex
        assert list(capi.DECLARED[f"spgpu{letter}ellDiag"][1]) == [capi.Handle, capi.ptr] + list(ell[4:9]) + list(ell[11:13]) + [ell[15], capi.i32]
        # hdiaspmv: handle z y alpha | dM offsets hackSize hackOffsets rows cols | x beta
        assert list(capi.DECLARED[f"spgpu{letter}hdiaDiag"][1]) == [capi.Handle, capi.ptr] + list(hdia[4:10]) + [capi.i32]


def test_the_header_is_a_c_header_of_the_abi(tmp_path):
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src
    prog = tmp_path / "abi.c"
    prog.write_text('#include "spgpu/ext/precond.h"\n'
                    "int main(void){\n"
                    " void (*a)(spgpuHandle_t, double*, const double*, const int*, int, const int*, const int*, int, int, int) = spgpuDhellDiag;\n"
                    " void (*b)(spgpuHandle_t, float*, const float*, const int*, int, int, const int*, int, int, int, int) = spgpuSellDiag;\n"
                    " void (*c)(spgpuHandle_t, double*, const double*, const int*, int, const int*, int, int, int) = spgpuDhdiaDiag;\n"
                    " void (*d)(spgpuHandle_t, float*, int, float*, const float*, const float*) = spgpuSaxyDotDevice;\n"
                    " void (*e)(spgpuHandle_t, double*, int, double*, const double*, const double*, double*, const double*, const double*,"
                    " double*, const double*, const double*, const double*) = spgpuDaxpbyPairAxyDotDevice;\n"
                    " void (*f)(spgpuHandle_t, double*, int, double*, const double*, const double*, int, int) = spgpuDmaxyDotDevice;\n"
                    " void (*g)(spgpuHandle_t, float*, int, float*, const float*, const float*, float*, const float*, const float*,"
                    " float*, const float*, const float*, const float*, int, int) = spgpuSmaxpbyPairAxyDotDevice;\n"
                    " return a == 0 || b == 0 || c == 0 || d == 0 || e == 0 || f == 0 || g == 0; }\n")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include", "-c", str(prog),
           "-o", str(tmp_path / "abi.o")]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_the_device_scalar_headers_point_to_the_header():
    for name in (("device_scalars.h",), ("ext", "device_scalars_mv.h")):
        with open(os.path.join(ROOT, "include", "spgpu", *name)) as f:
            assert "ext/precond.h" in f.read(), name


def test_no_rows_and_no_vectors_are_no_ops_without_a_gpu():
    h = C.pointer(capi.HandleStruct())   # never launched on: rows <= 0, hackSize <= 0 and count <= 0 return first
    for letter in "SD":
        for rows in (0, -1, -70):
            for invert in (0, 1):
                capi.hell_diag[letter](h, None, None, None, 32, None, None, rows, 0, invert)
                capi.ell_diag[letter](h, None, None, None, 128, 128, None, 5, rows, 1, invert)
                capi.hdia_diag[letter](h, None, None, None, 32, None, rows, 70, invert)
        for hack in (0, -32):
            capi.hell_diag[letter](h, None, None, None, hack, None, None, 70, 0, 1)
            capi.hdia_diag[letter](h, None, None, None, hack, None, 70, 70, 1)
        for count in (0, -1, -1025):
            for n in (0, 5):
                capi.maxy_dot_device[letter](h, None, n, None, None, None, count, 8)
                capi.maxpby_pair_axy_dot_device[letter](h, None, n, None, None, None, None, None, None, None, None, None, None, count, 8)
