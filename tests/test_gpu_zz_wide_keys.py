"""GPU: COO assembly, SpGEMM and the HELL transpose on matrices whose 64-bit sort keys reach beyond bit 31.

The three analyses build one composite key per entry -- (row << colBits) | column in assemble_device.hip and spgemm_device.hip,
(column << rowBits) | row in transpose_device.hip --, sort it with rocPRIM over rowBits + colBits bits and take it apart again with
shifts and masks.  The cases are those of tests/test_wide_keys_restated.py, which shows on the CPU that each of them sets a key bit
at or above bit 32 (up to bit 39) and that the restatements the helpers compare with are right there; here they run through the
helpers of the three device test files unchanged: guard bytes, poisoned outputs, both fills on every grid cap, byte for byte.  A
shift done in 32 bits, a mask of type unsigned, an end bit clamped to 32 or an (int) cast in front of a shift merges or misorders
entries of these matrices, and of no other in the suite.

Two cases also drive the three-launch scan of convert_scan.hip.h, of which every translation unit has its own device code, past
256 tiles (262 144 elements), where scanTotalsKernel loops with a carry: spgemm_device.hip's on the row counts and on the products
of the many-rows product, transpose_device.hip's on the 2^20 source rows of the second transpose of the round trip.  No array of a
matrix's column count is allocated on either side: the widest matrices have 2^31 - 1 columns."""
import numpy as np
import pytest

import test_wide_keys_restated as K
from test_gpu_transpose_device import _check, _poisoned, _transpose
from test_gpu_zz_assemble_device import _assemble
from test_gpu_zz_assemble_device import _plan as _assembly_plan
from test_gpu_zz_spgemm_device import _device, _multiply, _products
from test_gpu_zz_spgemm_device import _plan as _spgemm_plan

pytestmark = pytest.mark.gpu


def _integer_values(count, letter, seed):
    return K.integer_values(np.random.default_rng(seed), count, letter)


# ---- 1. assembly, narrow rows x widest columns: 7 + 31 = 38 bits -------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SZ")
def test_assembly_of_narrow_rows_and_widest_columns(gpu, letter):
    """70 x (2^31 - 1): with base 1 the largest index is INT_MAX.  Entries that differ only in bits 16 .. 30 of the column, or only
    in the top row bit, must stay apart; their duplicates must be added."""
    case = K.assembly_narrow_rows_widest_columns()
    vals = _integer_values(2000, letter, 1)
    for coo_base, csr_base in K.BASE_PAIRS:
        want = _assemble(gpu, 70, K.W, case["rows"], case["cols"], vals, letter, coo_base, csr_base)
        assert np.diff(want[2]).max() > 1 and int(want[3].max()) == K.W - 1 + csr_base


# ---- 2. assembly, both halves wide: 19 + 21 = 40 bits ------------------------------------------------------------------------------
def test_assembly_with_both_halves_wide(gpu):
    case = K.assembly_both_halves_wide()
    want = _assemble(gpu, case["n_rows"], case["n_cols"], case["rows"], case["cols"], _integer_values(5000, "D", 2), "D", 1, 0)
    lengths = np.diff(want[0])
    assert lengths[0] > 0 and lengths[2 ** 18] > 0 and int(want[3].max()) == 2 ** 20 and int(want[3].min()) == 0


# ---- 3. assembly, widths around a power of two: 32, 33, 33 and 34 bits ----------------------------------------------------------------
@pytest.mark.parametrize("n_rows,n_cols", K.POWER_OF_TWO_SHAPES)
def test_assembly_around_a_power_of_two(gpu, n_rows, n_cols):
    case = K.assembly_around_a_power_of_two(n_rows, n_cols)
    want = _assemble(gpu, n_rows, n_cols, case["rows"], case["cols"], _integer_values(1000, "D", 3), "D", 0, 1)
    assert want[0][n_rows] - want[0][n_rows - 1] >= 2 and int(want[3][-1]) == n_cols           # (rows - 1, 0) and (rows - 1, cols - 1)


# ---- 4. assembly refusals at width ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["column at base + columnsCount", "row at base + rowsCount"])
def test_assembly_refusals_at_width(gpu, kind):
    """columnsCount = 2^31 - 2, so that base + columnsCount is an int: SPGPU_UNSUPPORTED, the guards intact (_plan), and the handle
    assembles the valid wide list next."""
    from spgpu_amd import capi
    for base in (0, 1):
        case = K.refused_assembly_list(base)
        rows, cols = case["rows"] + base, case["cols"] + base
        if kind == "row at base + rowsCount":
            rows[1234] = base + 70
        else:
            cols[1234] = base + case["n_cols"]
            assert cols[1234] <= 2 ** 31 - 1
        st, unique, *_ = _assembly_plan(gpu, 70, case["n_cols"], rows, cols, base, base)
        assert st == capi.SPGPU_UNSUPPORTED and unique == 0, (kind, base)
        _assemble(gpu, 70, case["n_cols"], case["rows"], case["cols"], _integer_values(2000, "D", 4), "D", base, base)


# ---- 5. SpGEMM, widest B: 7 + 31 = 38 bits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("base", [0, 1])
def test_spgemm_with_the_widest_b(gpu, letter, base):
    case = K.spgemm_widest_b(letter, base)
    products, c_ptr, c_cols, _ = _multiply(gpu, case["a"], case["b"], K.W, letter, base, caps=(0, 1))
    lengths = np.diff(c_ptr)
    assert lengths[0] == lengths[5] == lengths[33] == lengths[69] == 0 and products > c_cols.size
    assert int(c_cols.max()) == K.W - 1 + base and lengths[case["last"]] > 0


# ---- 6. SpGEMM, many rows: 19 + 21 = 40 bits, both scans past 256 tiles ------------------------------------------------------------------
def test_spgemm_with_many_rows_and_scans_that_carry(gpu):
    case = K.spgemm_many_rows()
    n_rows = case["a"][0].size - 1
    products, c_ptr, c_cols, _ = _multiply(gpu, case["a"], case["b"], case["n_b_cols"], "D", 0, caps=(0, 3))
    assert n_rows + 1 > K.SCAN_CARRY and products > K.SCAN_CARRY          # the carry loop of this file's scanTotalsKernel, twice
    assert c_ptr[n_rows] > c_ptr[n_rows - 1] and int(c_cols[-1]) == 2 ** 20 and (np.diff(c_ptr) == 0).sum() > 200000


# ---- 7. SpGEMM refusals at width ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("kind", ["column at base + bColumnsCount", "row descends in its high bits", "row repeats a column above 2^16"])
def test_spgemm_refusals_at_width(gpu, kind, base):
    from spgpu_amd import capi
    (case, k), n_b_cols = K.refused_spgemm_pair(base), K.W - 1
    a, b = case["a"], K.bad_rows_of_b(case["b"], k, base, n_b_cols)[kind]
    d_a, d_b = _device(a), _device(b)
    st, products = _products(gpu, a, d_a, d_b, 50, base)
    assert st == capi.SPGPU_SUCCESS and products > 0                       # the products do not read B's columns
    st, entries, _, _ = _spgemm_plan(gpu, a, d_a, d_b, 50, n_b_cols, base, products)      # guards checked in _plan
    assert st == capi.SPGPU_UNSUPPORTED and entries == 0, kind
    _multiply(gpu, a, case["b"], n_b_cols, "D", base)                      # the handle works on, at the same width


# ---- 8. SpGEMM chain: wide columns read as aColIndices -------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
def test_spgemm_chain_through_wide_columns(gpu, base):
    case = K.spgemm_chain(base)
    _, ab_ptr, ab_cols, ab_vals = _multiply(gpu, case["a"], case["b"], case["n_mid"], "D", base, caps=(0, 1))
    assert int(ab_cols.max()) == 2 ** 20 + base
    _, c_ptr, c_cols, _ = _multiply(gpu, (ab_ptr, ab_cols, ab_vals), case["c"], 90, "D", base, caps=(0, 1))
    assert c_cols.size > 70 and (np.diff(c_ptr) > 0).sum() > 40


# ---- 9. transpose, both halves wide: 18 + 21 = 39 bits ---------------------------------------------------------------------------------
TRANSPOSE_RUNS = [("D", t_hack, t_base) for t_hack in (32, 24) for t_base in (0, 1)] + [("S", 32, 0)]


@pytest.mark.parametrize("with_order", [False, True])
@pytest.mark.parametrize("letter,t_hack,t_base", TRANSPOSE_RUNS)
def test_transpose_with_both_halves_wide(gpu, letter, t_hack, t_base, with_order):
    """(2^17 + 1) x 2^20 with duplicates.  Without rIdx the sort starts at bit rowBits = 18; with rIdx, shuffled and mapping the
    last storage row to matrix row 0, at bit 0."""
    hell, _, r_idx, _, case = K.transpose_source(letter, with_order=with_order)
    got, _, (t_rows, t_cols, _) = _check(gpu, _poisoned(hell), case["n_cols"], t_hack, t_base, r_idx=r_idx)
    assert got["row_lengths"][0] > 0 and got["row_lengths"][2 ** 20 - 1] > 0 and got["nnz"] > 150000
    assert int(t_cols.max()) == 2 ** 17 and ((np.diff(t_rows) == 0) & (np.diff(t_cols) == 0)).sum() > 100


# ---- 10. transpose twice at that shape ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hack,base", [(32, 0), (24, 1)])
def test_transposing_twice_at_that_shape_gives_the_source_back(gpu, hack, base):
    """Rows column-sorted, no duplicates, no rIdx.  The second transpose has 2^20 source rows: the scan of their lengths in
    transpose_device.hip runs past 256 tiles."""
    clean, ell, _, (r, _, _), case = K.transpose_source("D", duplicates=False, hack_size=hack, base=base)
    n_rows, n_cols = case["n_rows"], case["n_cols"]
    assert n_cols > K.SCAN_CARRY
    once = _transpose(gpu, _poisoned(clean), n_cols, hack, base)
    middle = dict(letter="D", rows=n_cols, hack_size=hack, base=base, row_lengths=once["row_lengths"], hack_offsets=once["hack_offsets"],
                  indices=once["indices"], values=once["values"])
    twice = _transpose(gpu, _poisoned(middle), n_rows, hack, base)
    assert twice["row_lengths"].tobytes() == np.ascontiguousarray(clean["row_lengths"][:n_rows], np.int32).tobytes()
    assert twice["hack_offsets"].tobytes() == clean["hack_offsets"].tobytes()
    assert twice["indices"].tobytes() == clean["indices"].tobytes() and twice["values"].tobytes() == clean["values"].tobytes()
    assert (twice["longest"], twice["nnz"], twice["height"]) == (ell["max_row"], r.size, clean["height"])
