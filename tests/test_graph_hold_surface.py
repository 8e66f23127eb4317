"""CPU: the holds of include/spgpu/ext/graph.h at the drop-in boundary.  Every call the header declares is exported by
libspgpu.so and bound in spgpu_amd.capi (the check test_capi_surface.py makes for include/spgpu/*.h, whose count the
subdirectory leaves alone); NULL arguments are refused without a GPU; SPGPU_IN_USE is a status of its own."""
import os

from spgpu_amd import capi
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "graph.h")


def test_every_call_of_the_graph_header_is_exported_and_bound():
    with open(HEADER) as f:
        declared = set(DECL.findall(f.read()))
    assert declared == {"spgpuSpmvHold", "spgpuSpmvRelease", "spgpuSpmvHolds"}, sorted(declared)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for name in sorted(declared):
        assert getattr(capi.lib, name) is not None


def test_the_header_is_a_c_header_of_the_abi():
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src
    assert "#define SPGPU_IN_USE 4" in src


def test_null_arguments_are_refused_without_a_gpu():
    assert capi.spgpuSpmvHold(None, None) == capi.SPGPU_UNSPECIFIED
    assert capi.spgpuSpmvRelease(None, None) == capi.SPGPU_UNSPECIFIED
    assert capi.spgpuSpmvHolds(None, None) == 0


def test_in_use_is_a_status_of_its_own():
    assert capi.SPGPU_IN_USE == 4
    assert capi.SPGPU_IN_USE not in (capi.SPGPU_SUCCESS, capi.SPGPU_UNSUPPORTED, capi.SPGPU_UNSPECIFIED, capi.SPGPU_OUTOFMEMORY)
