"""CPU: the device-scalar Level-1 calls on pitch multivectors (include/spgpu/ext/device_scalars_mv.h) at the drop-in boundary.  The
header declares exactly the twelve calls, libspgpu.so exports them and spgpu_amd.capi binds them with the single-vector argument
lists followed by count and pitch; the header is a C header of the ABI; without vectors the calls return without touching a GPU."""
import ctypes as C
import os
import subprocess

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "device_scalars_mv.h")
CALLS = ("mdotDevice", "mnrm2Device", "mdivDevice", "maxpbyDevice", "maxpbyQuotDevice", "maxpbyPairDotDevice")
NAMES = {f"spgpu{letter}{call}" for letter in "SD" for call in CALLS}
TABLES = {"mdotDevice": "mdot_device", "mnrm2Device": "mnrm2_device", "mdivDevice": "mdiv_device", "maxpbyDevice": "maxpby_device",
          "maxpbyQuotDevice": "maxpby_quot_device", "maxpbyPairDotDevice": "maxpby_pair_dot_device"}


def test_every_call_of_the_header_is_exported_and_bound():
    with open(HEADER) as f:
        declared = set(DECL.findall(f.read()))
    assert len(NAMES) == 12 and declared == NAMES, sorted(declared ^ NAMES)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for name in sorted(declared):
        assert getattr(capi.lib, name) is not None
    for call, table in TABLES.items():
        assert set(getattr(capi, table)) == {"S", "D"}, table
        for letter in "SD":
            assert getattr(capi, table)[letter] is getattr(capi, table)[letter] and capi.DECLARED[f"spgpu{letter}{call}"][0] is None


def test_the_argument_lists_are_the_single_vector_ones_and_the_layout():
    """count and pitch follow the argument list of the single-vector call (device_scalars.h); the division has no vector: count alone."""
    for letter in "SD":
        for call, extra in (("dotDevice", 2), ("nrm2Device", 2), ("divDevice", 1), ("axpbyDevice", 2), ("axpbyQuotDevice", 2),
                            ("axpbyPairDotDevice", 2)):
            args, single = capi.DECLARED[f"spgpu{letter}m{call}"][1], capi.DECLARED[f"spgpu{letter}{call}"][1]
            assert list(args) == list(single) + [C.c_int] * extra, call


def test_the_header_is_a_c_header_of_the_abi(tmp_path):
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src
    prog = tmp_path / "abi.c"
    prog.write_text('#include "spgpu/ext/device_scalars_mv.h"\n'
                    "int main(void){ void (*f)(spgpuHandle_t, double*, int, const double*, const double*, const double*, const double*,"
                    " const double*, int, const double*, int, int) = spgpuDmaxpbyQuotDevice;\n"
                    " void (*g)(spgpuHandle_t, float*, int, float*, const float*, const float*, float*, const float*, const float*,"
                    " const float*, const float*, int, int) = spgpuSmaxpbyPairDotDevice;\n"
                    " void (*d)(spgpuHandle_t, double*, int, const double*, const double*, int, int) = spgpuDmdotDevice;\n"
                    " return f == 0 || g == 0 || d == 0; }\n")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include", "-c", str(prog),
           "-o", str(tmp_path / "abi.o")]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_device_scalars_h_and_vector_h_point_to_the_header():
    for name in ("device_scalars.h", "vector.h"):
        with open(os.path.join(ROOT, "include", "spgpu", name)) as f:
            assert "ext/device_scalars_mv.h" in f.read(), name


def test_no_vectors_is_a_no_op_without_a_gpu():
    h = C.pointer(capi.HandleStruct())   # never launched on: count <= 0 returns first
    for letter in "SD":
        for count in (0, -1, -1025):
            for n in (0, 5):
                capi.mdot_device[letter](h, None, n, None, None, count, 8)
                capi.mnrm2_device[letter](h, None, n, None, count, 8)
                capi.maxpby_device[letter](h, None, n, None, None, None, None, count, 8)
                capi.maxpby_quot_device[letter](h, None, n, None, None, None, None, None, 1, None, count, 8)
                capi.maxpby_pair_dot_device[letter](h, None, n, None, None, None, None, None, None, None, None, count, 8)
            capi.mdiv_device[letter](h, None, None, None, 1, count)
