"""CPU: the device-side transpose of include/spgpu/ext/transpose_device.h at the drop-in boundary.  The header declares exactly
the five calls, libspgpu.so exports them and spgpu_amd.capi binds them with the declared argument counts (the check
test_capi_surface.py makes for include/spgpu/*.h, whose count the subdirectory leaves alone); without rows or columns there is
nothing to launch, so the no-op cases return without touching a GPU; and the host helper that lists A^T in the contract's order
from HELL or ELL arrays is pinned on a small example."""
import ctypes as C
import os

import numpy as np

from spgpu_amd import capi, formats
from test_capi_surface import DECL, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgpu", "ext", "transpose_device.h")
ARGS = {"spgpuHellTransposeWorkBytes": 3, "spgpuHellTransposeLengthsDevice": 14, "spgpuHellTransposeDevice": 19,
        "spgpuEllTransposeLengthsDevice": 13, "spgpuEllTransposeDevice": 19}


def _declaration(src, name):
    """The text between the parentheses of the declaration of `name`."""
    start = src.index(name + "(", src.index('extern "C"')) + len(name) + 1
    return src[start:src.index(");", start)]


def test_every_call_of_the_header_is_exported_and_bound():
    with open(HEADER) as f:
        src = f.read()
    declared = set(DECL.findall(src))
    assert declared == set(ARGS), sorted(declared)
    exported = exported_symbols()
    assert declared <= exported, sorted(declared - exported)
    assert declared <= set(capi.DECLARED), sorted(declared - set(capi.DECLARED))
    for name, count in ARGS.items():
        assert getattr(capi.lib, name) is not None
        assert len(capi.DECLARED[name][1]) == count, name
        assert _declaration(src, name).count(",") + 1 == count, name        # the binding has the header's argument count
    assert capi.DECLARED["spgpuHellTransposeWorkBytes"][0] is C.c_size_t


def test_the_header_is_a_c_header_of_the_abi():
    with open(HEADER) as f:
        src = f.read()
    assert '#include "../core.h"' in src and 'extern "C"' in src
    assert src.isascii()
    for word in ("entry order", "byte for byte", "duplicates are kept", "never read", "spgpuHellPlanDevice", "bytes per source slot"):
        assert word in src, word


def test_convert_device_h_points_to_the_header():
    with open(os.path.join(ROOT, "include", "spgpu", "convert_device.h")) as f:
        assert "ext/transpose_device.h" in f.read()


def test_no_rows_or_no_columns_is_a_no_op_without_a_gpu():
    h = capi.HandleStruct()   # never launched on: rowsCount <= 0 or columnsCount <= 0 returns first
    for rows, cols in ((0, 5), (5, 0), (-3, 5), (5, -3), (0, 0), (-3, -3)):
        longest, nnz = C.c_int(-1), C.c_int(-1)
        assert capi.spgpuHellTransposeLengthsDevice(C.pointer(h), None, C.byref(longest), C.byref(nnz), None, 32, None, None, None,
                                                    rows, cols, 0, 0, None) == capi.SPGPU_SUCCESS
        assert (longest.value, nnz.value) == (0, 0)
        longest, nnz = C.c_int(-1), C.c_int(-1)
        assert capi.spgpuEllTransposeLengthsDevice(C.pointer(h), None, C.byref(longest), C.byref(nnz), None, 32, None, None, rows,
                                                   cols, 1, 0, None) == capi.SPGPU_SUCCESS
        assert (longest.value, nnz.value) == (0, 0)
        for code in (capi.TYPE_FLOAT, capi.TYPE_DOUBLE, capi.TYPE_COMPLEX_DOUBLE, 5, -1):
            assert capi.spgpuHellTransposeDevice(C.pointer(h), None, None, None, 32, 1, None, None, 32, None, None, None, rows, cols,
                                                 0, 0, code, None, None) == capi.SPGPU_SUCCESS
            assert capi.spgpuEllTransposeDevice(C.pointer(h), None, None, None, 32, 0, None, None, 32, 32, None, None, rows, cols, 1,
                                                0, code, None, None) == capi.SPGPU_SUCCESS


def test_an_element_size_other_than_4_8_16_is_refused_before_anything_is_launched():
    h = capi.HandleStruct()
    for code in (5, -1):
        assert capi.spgpuSizeOf(code) == 0
        assert capi.spgpuHellTransposeDevice(C.pointer(h), None, None, None, 32, 0, None, None, 32, None, None, None, 4, 4, 0, 128, code,
                                             None, None) == capi.SPGPU_UNSUPPORTED
        assert capi.spgpuEllTransposeDevice(C.pointer(h), None, None, None, 32, 0, None, None, 32, 32, None, None, 4, 4, 0, 128, code,
                                            None, None) == capi.SPGPU_UNSUPPORTED


def _example(base):
    """Five storage rows, four columns, six entries: rows 0 and 4 empty, (storage row 2, column 2) stored twice."""
    rows = np.array([1, 1, 2, 2, 3, 3], np.int32) + base
    cols = np.array([2, 0, 2, 2, 0, 3], np.int32) + base
    vals = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    ell = formats.coo_to_ell(5, rows, cols, vals, coo_base=base, ell_base=base)
    return ell, formats.ell_to_hell(ell, 2)      # hacks of two rows: three of them, the last one row only and empty


def test_the_transposed_listing_is_in_the_contracts_order():
    """formats.hell_transposed_coo / ell_transposed_coo: by column, then by ascending matrix row i (= rIdx[r]), then by slot; the
    duplicate stays, in slot order; both bases; the padding is poisoned and never looked at."""
    r_idx = np.array([0, 3, 1, 2, 4], np.int32)
    for base in (0, 1):
        ell, hell = _example(base)
        assert hell["hack_offsets"].tolist() == [0, 4, 8] and hell["row_lengths"].tolist() == [0, 2, 2, 2, 0]
        r, k = np.array([1, 1, 2, 2, 3, 3]), np.array([0, 1, 0, 1, 0, 1])
        for mat, listing, slots in ((hell, formats.hell_transposed_coo, hell["hack_offsets"][r // 2] + r % 2 + k * 2),
                                    (ell, formats.ell_transposed_coo, r + k * ell["pitch"])):
            mat = dict(mat, indices=mat["indices"].copy(), values=mat["values"].copy())
            stored = np.zeros(mat["indices"].size, bool)
            stored[slots] = True
            mat["indices"][~stored] = 1 << 30
            mat["values"][~stored] = np.nan
            t_rows, t_cols, t_vals = listing(mat)
            assert t_rows.dtype == np.int32 and t_cols.dtype == np.int32 and t_vals.dtype == np.float64
            assert t_rows.tolist() == [0, 0, 2, 2, 2, 3] and t_cols.tolist() == [1, 3, 1, 2, 2, 3]
            assert t_vals.tolist() == [2.0, 5.0, 1.0, 3.0, 4.0, 6.0]
            t_rows, t_cols, t_vals = listing(mat, r_idx)
            assert t_rows.tolist() == [0, 0, 2, 2, 2, 3] and t_cols.tolist() == [2, 3, 1, 1, 3, 2]
            assert t_vals.tolist() == [5.0, 2.0, 3.0, 4.0, 1.0, 6.0]
    empty = formats.ell_to_hell(formats.coo_to_ell(3, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)), 32)
    t_rows, t_cols, t_vals = formats.hell_transposed_coo(empty)
    assert t_rows.size == 0 and t_cols.size == 0 and t_vals.size == 0 and t_vals.dtype == np.float32
