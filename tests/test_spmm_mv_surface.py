"""CPU: the pitch-layout SpMM of include/spgpu/ext/spmm_mv.h at the drop-in boundary.  The header declares exactly the two
calls, libspgpu.so exports them and spgpu_amd.capi binds them with spgpu?hellspmm's argument list (the check
test_capi_surface.py makes for include/spgpu/*.h, whose count the subdirectory leaves alone); without a handle's stream to
launch on, the no-op cases return without touching a GPU."""
import ctypes as C
import os

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "spmm_mv.h")


def test_every_call_of_the_header_is_exported_and_bound():
    with open(HEADER) as f:
        declared = set(DECL.findall(f.read()))
    assert declared == {"spgpuShellspmmMv", "spgpuDhellspmmMv"}, sorted(declared)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for name in sorted(declared):
        assert getattr(capi.lib, name) is not None
    assert set(capi.hellspmm_mv) == {"S", "D"}


def test_the_header_is_a_c_header_of_the_abi():
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src
    assert "pitchX" in src and "pitchYZ" in src


def test_the_argument_list_is_hellspmm_s():
    for letter in "SD":
        mv, inter = capi.DECLARED[f"spgpu{letter}hellspmmMv"], capi.DECLARED[f"spgpu{letter}hellspmm"]
        assert mv == inter and len(mv[1]) == 18


def test_spmm_h_points_to_the_header():
    with open(os.path.join(ROOT, "include", "spgpu", "spmm.h")) as f:
        assert "ext/spmm_mv.h" in f.read()


def test_no_rows_or_no_vectors_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: rows <= 0 and count <= 0 return first
    for letter in "SD":
        capi.hellspmm_mv[letter](C.pointer(h), None, None, capi.scalar(letter, 1), None, None, 32, None, None, None, 0, 0, None,
                                 capi.scalar(letter, 0), 0, 16, 0, 0)
        capi.hellspmm_mv[letter](C.pointer(h), None, None, capi.scalar(letter, 1), None, None, 32, None, None, None, 0, 64, None,
                                 capi.scalar(letter, 0), 0, 0, 64, 64)
