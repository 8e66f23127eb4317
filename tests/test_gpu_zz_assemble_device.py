"""GPU: assembly of a COO list with duplicates into CSR (include/spgpu/ext/assemble_device.h).

Every output array -- csrRowPtr, perm, segPtr, csrColIndices, csrValues -- lies between 64 guard bytes, is poisoned as a whole with
one byte pattern and must afterwards equal numpy's restatement of the contract (formats.coo_assemble) BYTE FOR BYTE: the row
pointers, the permutation, the first uniqueCount + 1 elements of segPtr (the rest still the poison), the columns and the sums.  The
fills run through the public calls and through each of the two fills behind them (one thread per matrix entry; a workgroup per
ASSEMBLE_TILE entries staging ASSEMBLE_CHUNK positions of perm per trip through LDS), pattern + values and values only: all must
give the same bytes (_assemble).  The lists are the smallest at which each branch of the plan and of the staged fill can go wrong."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
from test_gpu_csr_device import _hell_plan, _p, _row_lengths, _upload, _zeros
from test_gpu_to_csr_device import PATTERN, _Guarded, _device_hell_of_csr, _expect, _to_csr
from test_gpu_update_device import _bits

pytestmark = pytest.mark.gpu

BASES = ((0, 0), (1, 1), (0, 1), (1, 0))          # (cooBaseIndex, csrBaseIndex)


def _values(rng, count, letter):
    dtype = np.dtype(X.DTYPE_OF[letter])
    real = X.REAL_OF[letter]
    if dtype.kind == "c":
        return rng.standard_normal(2 * count).astype(real).view(dtype)
    return rng.standard_normal(count).astype(real)


def _plan(gpu, n_rows, n_cols, rows, cols, coo_base, csr_base):
    """spgpuCooAssemblePlanDevice on a list given in `coo_base`: (status, uniqueCount, row_ptr, perm, seg_ptr as _Guarded, the device
    list).  The scratch is overwritten when the call has returned: the plan arrays are self-contained."""
    import torch
    from spgpu_amd import capi, formats
    nnz = len(rows)
    d_rows = formats.to_device(np.ascontiguousarray(rows, np.int32)) if nnz else None
    d_cols = formats.to_device(np.ascontiguousarray(cols, np.int32)) if nnz else None
    row_ptr, perm, seg_ptr = _Guarded((n_rows + 1) * 4), _Guarded(nnz * 4), _Guarded((nnz + 1) * 4)
    work = torch.empty(capi.spgpuCooAssembleWorkBytes(n_rows, n_cols, nnz), dtype=torch.uint8, device="cuda:0")
    unique = C.c_int(-1)
    torch.cuda.synchronize()
    st = capi.spgpuCooAssemblePlanDevice(gpu, C.byref(unique), row_ptr.ptr(), perm.ptr(), seg_ptr.ptr(), n_rows, n_cols, nnz, _p(d_rows),
                                         _p(d_cols), coo_base, csr_base, _p(work))
    work.fill_(0xFF)
    torch.cuda.synchronize()
    assert row_ptr.guards_intact() and perm.guards_intact() and seg_ptr.guards_intact()
    return st, unique.value, row_ptr, perm, seg_ptr, (d_rows, d_cols)


def _fills(gpu, unique, nnz, d_cols, vals_at, coo_base, csr_base, letter, perm, seg_ptr, max_blocks=0):
    """Every way to the columns and sums: {(fill or None, 'full' or 'values'): (cols bytes or None, vals bytes)}, guards checked."""
    import torch
    from spgpu_amd import capi
    code, size = capi.TYPE_CODE[letter], np.dtype(X.DTYPE_OF[letter]).itemsize
    out = {}
    for fill in (None, capi.ASSEMBLE_FILL_PLAIN, capi.ASSEMBLE_FILL_STAGED):
        for what in ("full", "values"):
            cols, vals = _Guarded(unique * 4), _Guarded(unique * size)
            torch.cuda.synchronize()
            if what == "full":
                args = (gpu, cols.ptr(), vals.ptr(), unique, nnz, _p(d_cols), C.c_void_p(vals_at), coo_base, csr_base, code, perm.ptr(),
                        seg_ptr.ptr())
                st = capi.spgpuCooAssembleDevice(*args) if fill is None else capi.spgpuCooAssembleDeviceWith(*args, fill, max_blocks)
            else:
                args = (gpu, vals.ptr(), unique, nnz, C.c_void_p(vals_at), code, perm.ptr(), seg_ptr.ptr())
                st = capi.spgpuCooAssembleValuesDevice(*args) if fill is None else capi.spgpuCooAssembleValuesDeviceWith(*args, fill, max_blocks)
            assert st == capi.SPGPU_SUCCESS, (fill, what)
            torch.cuda.synchronize()
            assert cols.guards_intact() and vals.guards_intact() and perm.guards_intact() and seg_ptr.guards_intact(), (fill, what)
            if what == "values":
                assert cols.untouched(), fill
            out[(fill, what)] = (cols.numpy(np.uint8).tobytes() if what == "full" else None, vals.numpy(np.uint8).tobytes())
    return out


def _assemble(gpu, n_rows, n_cols, rows, cols, vals, letter, coo_base=0, csr_base=0, max_blocks=0):
    """Plan and fills on a 0-based list (moved to coo_base here), every array against formats.coo_assemble.  Returns the restated
    arrays (row_ptr, perm, seg_ptr, cols, vals)."""
    from spgpu_amd import capi, formats
    rows, cols = np.asarray(rows, np.int64) + coo_base, np.asarray(cols, np.int64) + coo_base
    vals = np.ascontiguousarray(vals)
    assert vals.dtype == np.dtype(X.DTYPE_OF[letter])
    nnz = rows.size
    want = formats.coo_assemble(n_rows, n_cols, rows, cols, vals, coo_base, csr_base)
    w_ptr, w_perm, w_seg, w_cols, w_vals = want
    st, unique, row_ptr, perm, seg_ptr, (d_rows, d_cols) = _plan(gpu, n_rows, n_cols, rows, cols, coo_base, csr_base)
    case = (letter, n_rows, n_cols, nnz, coo_base, csr_base)
    assert st == capi.SPGPU_SUCCESS and unique == w_cols.size, case
    assert row_ptr.numpy(np.int32).tobytes() == w_ptr.tobytes(), case
    assert perm.numpy(np.int32).tobytes() == w_perm.tobytes(), case
    got_seg = seg_ptr.numpy(np.uint8)
    assert got_seg[:4 * (unique + 1)].tobytes() == w_seg.tobytes(), case
    assert (got_seg[4 * (unique + 1):] == PATTERN).all(), case          # beyond uniqueCount: not written
    vals_buf, vals_at = _upload(vals.view(np.uint8))
    results = _fills(gpu, unique, nnz, d_cols, vals_at, coo_base, csr_base, letter, perm, seg_ptr, max_blocks)
    for (fill, what), (got_cols, got_vals) in results.items():
        if got_cols is not None:
            assert got_cols == w_cols.tobytes(), (case, fill, what)
        assert got_vals == w_vals.tobytes(), (case, fill, what)
    del vals_buf
    return want


def _shuffled_list(rng, n_rows, n_cols, nnz, skip_rows=()):
    """`nnz` contributions at random places of the matrix, 0-based; no contribution in `skip_rows`."""
    allowed = np.setdiff1d(np.arange(n_rows), skip_rows)
    return allowed[rng.integers(0, allowed.size, nnz)], rng.integers(0, n_cols, nnz)


def _list_of_lengths(rng, lengths, n_cols):
    """A shuffled 0-based list whose matrix entry u (in the contract's numbering) has lengths[u] contributions: entry u is
    (u // n_cols, u % n_cols).  Returns (n_rows, rows, cols)."""
    lengths = np.asarray(lengths, np.int64)
    entry = np.repeat(np.arange(lengths.size), lengths)
    entry = entry[rng.permutation(entry.size)]
    return int((lengths.size + n_cols - 1) // n_cols), entry // n_cols, entry % n_cols


# ---- 1. every type x both bases on either side, heavy duplication, empty rows ------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
def test_duplicated_lists_give_numpys_arrays(gpu, letter):
    """70 x 50, 3 000 shuffled contributions (almost every entry listed, most of them more than once; the plan's scan is past its
    first tile of 1 024), with every row named and with rows 0, 7 and 69 -- first, middle, last -- never named."""
    rng = np.random.default_rng(ord(letter))
    for skip in ((), (0, 7, 69)):
        rows, cols = _shuffled_list(rng, 70, 50, 3000, skip)
        assert not np.isin(rows, skip).any()
        vals = _values(rng, 3000, letter)
        for coo_base, csr_base in BASES:
            row_ptr, _, seg_ptr, _, _ = _assemble(gpu, 70, 50, rows, cols, vals, letter, coo_base, csr_base)
            assert np.diff(seg_ptr).max() > 1 and seg_ptr.size - 1 < 3000
            for r in skip:
                assert row_ptr[r] == row_ptr[r + 1]


# ---- 2. every entry listed once: the straight gather; values move as bits -------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
def test_single_contributions_are_moved_as_bits(gpu, letter):
    """unique == nnz = 1 000 (three whole tiles and a part), so every tile takes the straight-gather branch of the staged fill; the
    values are random bits with quiet and signalling NaNs that carry payloads and -0.0 planted."""
    from spgpu_amd import capi
    rng = np.random.default_rng(10 + ord(letter))
    dtype = np.dtype(X.DTYPE_OF[letter])
    assert 1000 > 3 * capi.ASSEMBLE_TILE
    once = rng.permutation(40 * 30)[:1000]
    vals = _bits(rng, 1000, dtype.itemsize).copy().reshape(-1).view(dtype)
    want = _assemble(gpu, 40, 30, once // 30, once % 30, vals, letter, 1, 0)
    assert np.diff(want[2]).max() == 1
    assert want[4].tobytes() == vals[want[1]].tobytes()                     # the restatement itself moved bits
    assert np.isnan(vals.view(X.REAL_OF[letter])[:8]).any()


@pytest.mark.parametrize("letter", "SDCZ")
def test_single_contributions_among_sums_are_moved_as_bits(gpu, letter):
    """Tiles that are NOT straight gathers: NaNs with payloads and -0.0 planted only in entries with a single contribution (how a NaN
    payload goes through an addition is not part of the contract), sums all around them."""
    rng = np.random.default_rng(20 + ord(letter))
    dtype = np.dtype(X.DTYPE_OF[letter])
    lengths = rng.integers(1, 5, 700)
    lengths[::3] = 1
    n_rows, rows, cols = _list_of_lengths(rng, lengths, 37)
    vals = _values(rng, rows.size, letter)
    entry = rows * 37 + cols
    single = np.flatnonzero(lengths[entry] == 1)
    planted = _bits(rng, single.size, dtype.itemsize).copy().reshape(-1).view(dtype)
    vals[single] = planted
    assert np.isnan(vals.view(X.REAL_OF[letter])).sum() >= 2
    want = _assemble(gpu, n_rows, 37, rows, cols, vals, letter)
    assert want[4][lengths == 1].tobytes() == vals[want[1][want[2][:-1][lengths == 1]]].tobytes()


# ---- 3. one entry listed 5 000 times: a segment longer than any chunk and any tile -----------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
def test_an_entry_listed_5000_times_among_1000_others(gpu, letter):
    from spgpu_amd import capi
    rng = np.random.default_rng(30 + ord(letter))
    assert 5000 > 4 * capi.ASSEMBLE_CHUNK and 5000 > capi.ASSEMBLE_TILE
    rows, cols = _shuffled_list(rng, 60, 60, 1000)
    rows, cols = np.concatenate((rows, np.full(5000, 31))), np.concatenate((cols, np.full(5000, 17)))
    order = rng.permutation(6000)
    want = _assemble(gpu, 60, 60, rows[order], cols[order], _values(rng, 6000, letter), letter, 1, 1)
    assert np.diff(want[2]).max() >= 5000


# ---- 4. tile edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unique", [255, 256, 257, 1025])
def test_tile_edges(gpu, unique):
    """uniqueCount one below, at and one above a tile of the staged fill, and four tiles plus one entry; 1 to 4 contributions each; on
    the whole grid and on a grid of one and of three workgroups (the grid stride of both fills)."""
    from spgpu_amd import capi
    assert capi.ASSEMBLE_TILE == 256
    rng = np.random.default_rng(unique)
    lengths = rng.integers(1, 5, unique)
    lengths[-1] = 3                                                        # the lone entry of the last tile is a sum
    n_rows, rows, cols = _list_of_lengths(rng, lengths, 41)
    for letter in "SZ":
        vals = _values(rng, rows.size, letter)
        for cap in (0, 1, 3):
            want = _assemble(gpu, n_rows, 41, rows, cols, vals, letter, max_blocks=cap)
            assert want[3].size == unique


# ---- 5. segments that straddle the staged fill's chunk boundaries ---------------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
def test_segments_straddle_chunk_boundaries(gpu, letter):
    """The staged fill cuts the range of perm that belongs to a tile of ASSEMBLE_TILE entries into chunks of ASSEMBLE_CHUNK positions
    counted from the TILE'S first position.  In tile 0 a segment crosses the first boundary, one ends exactly on the second (the
    next starts there), one contains the third and the fourth (two whole trips with the running sum carried); the tile's last
    segment ends away from a multiple of the chunk, so tile 1's boundaries are not tile 0's, and a segment crosses tile 1's first."""
    from spgpu_amd import capi
    tile, chunk = capi.ASSEMBLE_TILE, capi.ASSEMBLE_CHUNK
    rng = np.random.default_rng(40 + ord(letter))
    lengths = np.ones(2 * tile + 5, np.int64)
    lengths[0] = chunk - 3
    lengths[1] = 7                                   # positions chunk - 3 .. chunk + 4: crosses boundary 1
    lengths[2] = chunk - 4                           # ends on boundary 2
    lengths[3] = 1                                   # starts on boundary 2
    lengths[4] = 2 * chunk + 5                       # contains boundaries 3 and 4
    lengths[5:tile] = rng.integers(1, 4, tile - 5)
    first_of_tile_1 = int(lengths[:tile].sum())
    lengths[tile] = chunk - 2                        # tile 1: positions first .. first + chunk - 2
    lengths[tile + 1] = 5                            # crosses tile 1's boundary 1
    lengths[tile + 2:] = rng.integers(1, 4, tile + 3)
    n_rows, rows, cols = _list_of_lengths(rng, lengths, 29)
    want = _assemble(gpu, n_rows, 29, rows, cols, _values(rng, rows.size, letter), letter)
    seg = want[2].astype(np.int64)
    assert np.array_equal(np.diff(seg), lengths)
    assert first_of_tile_1 % chunk != 0 and seg[tile] == first_of_tile_1
    inside = lambda u, b: seg[u] < b < seg[u + 1]
    assert inside(1, chunk) and seg[3] == 2 * chunk and inside(4, 3 * chunk) and inside(4, 4 * chunk)
    assert inside(tile + 1, first_of_tile_1 + chunk) and not any(inside(tile + 1, k * chunk) for k in range(1, 8))


# ---- 6. degenerate shapes ---------------------------------------------------------------------------------------------
def test_an_empty_list_one_row_one_column(gpu):
    import torch
    from spgpu_amd import capi
    rng = np.random.default_rng(6)
    none = np.zeros(0, np.int64)
    for coo_base, csr_base in BASES:
        st, unique, row_ptr, perm, seg_ptr, _ = _plan(gpu, 9, 4, none, none, coo_base, csr_base)
        assert st == capi.SPGPU_SUCCESS and unique == 0
        assert row_ptr.numpy(np.int32).tobytes() == np.full(10, csr_base, np.int32).tobytes()
        assert seg_ptr.numpy(np.int32).tolist() == [0] and perm.untouched()
        cols, vals = _Guarded(64), _Guarded(64)
        assert capi.spgpuCooAssembleDevice(gpu, cols.ptr(), vals.ptr(), 0, 0, None, None, coo_base, csr_base, capi.TYPE_DOUBLE, perm.ptr(),
                                           seg_ptr.ptr()) == capi.SPGPU_SUCCESS
        assert capi.spgpuCooAssembleValuesDevice(gpu, vals.ptr(), 0, 0, None, capi.TYPE_DOUBLE, perm.ptr(), seg_ptr.ptr()) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        assert cols.untouched() and vals.untouched()
    for letter in "SDCZ":
        for coo_base, csr_base in BASES:
            cols = rng.integers(0, 300, 900)
            _assemble(gpu, 1, 300, np.zeros(900, np.int64), cols, _values(rng, 900, letter), letter, coo_base, csr_base)   # rowsCount == 1
            rows = rng.integers(0, 300, 900)
            rows[rows == 299] = 5                                                                                       # the last row empty
            _assemble(gpu, 300, 1, rows, np.zeros(900, np.int64), _values(rng, 900, letter), letter, coo_base, csr_base)   # columnsCount == 1
        _assemble(gpu, 1, 1, np.zeros(7, np.int64), np.zeros(7, np.int64), _values(rng, 7, letter), letter, 1, 0)          # a key of no bits
        _assemble(gpu, 1, 1, np.zeros(1, np.int64), np.zeros(1, np.int64), _values(rng, 1, letter), letter)


# ---- 7. every kernel of the plan on more than one workgroup, the scan on more than one tile -----------------------------------
def test_300k_contributions_over_20k_rows(gpu):
    rng = np.random.default_rng(7)
    n, entries, nnz = 20000, 110000, 300000
    pairs = np.unique(rng.integers(0, n * n, entries))
    pick = pairs[rng.integers(0, pairs.size, nnz)]
    want = _assemble(gpu, n, n, pick // n, pick % n, _values(rng, nnz, "D"), "D", 1, 0)
    assert 1024 * 64 < want[3].size <= entries and (np.diff(want[0]) == 0).any()


# ---- 8. entries outside the matrix -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["row below the base", "row at base + rowsCount", "column at base + columnsCount"])
def test_an_entry_outside_the_matrix_is_refused(gpu, kind):
    """One bad entry among 2 000 good ones: SPGPU_UNSUPPORTED, the guards intact (_plan), and the handle assembles a valid list next."""
    from spgpu_amd import capi
    rng = np.random.default_rng(8)
    rows, cols = _shuffled_list(rng, 70, 50, 2000)
    for base in (0, 1):
        r, c = rows + base, cols + base
        if kind == "row below the base":
            r[1234] = base - 1
        elif kind == "row at base + rowsCount":
            r[1234] = base + 70
        else:
            c[1234] = base + 50
        st, unique, *_ = _plan(gpu, 70, 50, r, c, base, base)
        assert st == capi.SPGPU_UNSUPPORTED and unique == 0, (kind, base)
        _assemble(gpu, 70, 50, rows, cols, _values(rng, 2000, "D"), "D", base, base)


# ---- 9. determinism ---------------------------------------------------------------------------------------------------
def test_the_values_call_gives_the_same_bytes_every_time(gpu):
    import torch
    from spgpu_amd import capi
    rng = np.random.default_rng(9)
    rows, cols = _shuffled_list(rng, 500, 400, 60000)
    vals = _values(rng, 60000, "D")
    st, unique, row_ptr, perm, seg_ptr, _ = _plan(gpu, 500, 400, rows, cols, 0, 0)
    assert st == capi.SPGPU_SUCCESS
    vals_buf, vals_at = _upload(vals)
    seen = set()
    for _ in range(3):
        out = _Guarded(unique * 8)
        assert capi.spgpuCooAssembleValuesDevice(gpu, out.ptr(), unique, 60000, C.c_void_p(vals_at), capi.TYPE_DOUBLE, perm.ptr(),
                                                 seg_ptr.ptr()) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        seen.add(out.buf.cpu().numpy().tobytes())
    assert len(seen) == 1


# ---- 10. the assembled CSR is a CSR the other calls take --------------------------------------------------------------------
def test_round_trip_through_hell(gpu):
    """The assembled arrays through spgpuCsrToHellDevice and back through spgpuHellToCsrRowPtrDevice / spgpuHellToCsrDevice."""
    rng = np.random.default_rng(10)
    rows, cols = _shuffled_list(rng, 333, 200, 9000, skip_rows=(0, 100, 332))
    base = 1
    row_ptr, _, _, out_cols, out_vals = _assemble(gpu, 333, 200, rows, cols, _values(rng, 9000, "D"), "D", 0, base)
    src, _ = _device_hell_of_csr(gpu, 333, row_ptr, out_cols, out_vals, base, 32, None)
    _expect(_to_csr(gpu, src, base), row_ptr, out_cols, out_vals, int(np.diff(row_ptr).max()))


def _device_assembled_hell(gpu, n_rows, n_cols, rows, cols, vals, letter, base, hs=32):
    """Plan, fill, spgpuCsrRowLengthsDevice, spgpuHellPlanDevice, spgpuCsrToHellDevice, all on device arrays (0-based list in, `base`
    everywhere): a dict of the tensors."""
    import torch
    from spgpu_amd import capi, formats
    dtype = np.dtype(X.DTYPE_OF[letter])
    st, unique, row_ptr, perm, seg_ptr, (d_rows, d_cols) = _plan(gpu, n_rows, n_cols, rows + base, cols + base, base, base)
    assert st == capi.SPGPU_SUCCESS
    d_vals = formats.to_device(vals)
    csr_cols, csr_vals = _zeros(unique, np.int32), _zeros(unique, dtype)
    assert capi.spgpuCooAssembleDevice(gpu, _p(csr_cols), _p(csr_vals), unique, rows.size, _p(d_cols), _p(d_vals), base, base,
                                       capi.TYPE_CODE[letter], perm.ptr(), seg_ptr.ptr()) == capi.SPGPU_SUCCESS
    d_ptr = torch.from_numpy(row_ptr.numpy(np.int32).copy()).to("cuda:0")
    st, longest, rs = _row_lengths(gpu, n_rows, d_ptr, base)
    assert st == capi.SPGPU_SUCCESS
    height, ho = _hell_plan(gpu, n_rows, hs, rs)
    cm, rp = _zeros(hs * height, dtype), _zeros(hs * height, np.int32)
    assert capi.spgpuCsrToHellDevice(gpu, _p(cm), _p(rp), _p(ho), hs, base, n_rows, _p(d_ptr), _p(csr_cols), _p(csr_vals), base,
                                     capi.TYPE_CODE[letter], None) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    return dict(cM=cm, rP=rp, ho=ho, rS=rs, ptr=d_ptr, cols=csr_cols, vals=csr_vals, unique=unique, perm=perm, seg=seg_ptr, coo_rows=d_rows,
                coo_cols=d_cols, coo_vals=d_vals, slots=hs * height, longest=longest)


def _hellspmv(gpu, letter, z, mat, hs, n_rows, x, base):
    from spgpu_amd import capi
    capi.hellspmv[letter](gpu, _p(z), _p(z), capi.scalar(letter, 1), _p(mat["cM"]), _p(mat["rP"]), hs, _p(mat["ho"]), _p(mat["rS"]), None, 0,
                          n_rows, _p(x), capi.scalar(letter, 0), base)


@pytest.mark.parametrize("letter", "SDCZ")
def test_the_product_is_that_of_the_list_with_duplicates_kept(gpu, letter):
    """Integer contributions of magnitude <= 64, at most 16 per entry, and an integer x of magnitude <= 8: every sum and every
    product is exact even in fp32 (a row's products, complex ones included, add up to less than 60 * 16 * 64 * 8 * 2 < 2^24), so spgpu?hellspmv on the
    assembled matrix and on the spgpuCooToHellDevice matrix of the same list -- every duplicate a slot -- give equal z."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(50 + ord(letter))
    n_rows, n_cols, base, hs = 150, 60, 1, 32
    lengths = rng.integers(0, 17, n_rows * n_cols)
    lengths[rng.random(lengths.size) < 0.6] = 0                      # 40 % of the entries listed: rows of about 24 entries
    lengths[:n_cols] = 0                                             # row 0 empty
    _, rows, cols = _list_of_lengths(rng, lengths, n_cols)
    dtype, real = np.dtype(X.DTYPE_OF[letter]), X.REAL_OF[letter]
    parts = 2 if dtype.kind == "c" else 1
    vals = rng.integers(-64, 65, parts * rows.size).astype(real).view(dtype)
    x = rng.integers(-8, 9, parts * n_cols).astype(real).view(dtype)
    asm = _device_assembled_hell(gpu, n_rows, n_cols, rows, cols, vals, letter, base, hs)
    assert asm["unique"] == int((lengths > 0).sum()) and lengths.max() == 16
    # the same list with every duplicate kept
    nnz = rows.size
    work = torch.empty(capi.spgpuCooConvertWorkBytes(n_rows, nnz), dtype=torch.uint8, device="cuda:0")
    rs = torch.zeros(n_rows, dtype=torch.int32, device="cuda:0")
    longest = C.c_int(-1)
    assert capi.spgpuCooRowLengthsDevice(gpu, _p(rs), C.byref(longest), n_rows, nnz, _p(asm["coo_rows"]), base, _p(work)) == capi.SPGPU_SUCCESS
    ho = torch.zeros((n_rows + hs - 1) // hs, dtype=torch.int32, device="cuda:0")
    height = C.c_int(-1)
    assert capi.spgpuHellPlanDevice(gpu, C.byref(height), _p(ho), hs, n_rows, _p(rs), _p(work)) == capi.SPGPU_SUCCESS
    kept = dict(cM=_zeros(hs * height.value, dtype), rP=_zeros(hs * height.value, np.int32), ho=ho, rS=rs)
    assert capi.spgpuCooToHellDevice(gpu, _p(kept["cM"]), _p(kept["rP"]), _p(ho), hs, base, n_rows, nnz, _p(asm["coo_rows"]), _p(asm["coo_cols"]),
                                     _p(asm["coo_vals"]), base, capi.TYPE_CODE[letter], _p(rs), _p(work)) == capi.SPGPU_SUCCESS
    assert longest.value > asm["longest"] and hs * height.value > asm["slots"]
    d_x = formats.to_device(x)
    z_asm, z_kept = _zeros(n_rows, dtype), _zeros(n_rows, dtype)
    _hellspmv(gpu, letter, z_asm, asm, hs, n_rows, d_x, base)
    _hellspmv(gpu, letter, z_kept, kept, hs, n_rows, d_x, base)
    torch.cuda.synchronize()
    got = z_asm.cpu().numpy()
    assert np.array_equal(got, z_kept.cpu().numpy())
    want, scale = X.spmv(n_rows, rows, cols, vals, x, None, 1, 0)
    assert np.array_equal(got, want.astype(dtype)) and np.abs(want).max() < 2 ** 24 and np.abs(got).max() > 0
    X.assert_within(got, want, scale, letter, "assembled")


# ---- 11. sorted rows take the partial update -------------------------------------------------------------------------------
def test_hellcsput_finds_a_chosen_entry_in_every_row(gpu):
    """After assembly and spgpuCsrToHellDevice the columns of every row ascend, so spgpuDhellcsput's bisection finds them: one chosen
    entry of every non-empty row is overwritten, and the matrix read back as CSR (spgpuHellToCsrDevice) is numpy's."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(11)
    n_rows, n_cols, base, hs = 200, 90, 1, 32
    rows, cols = _shuffled_list(rng, n_rows, n_cols, 5000, skip_rows=(0, 50))
    vals = _values(rng, 5000, "D")
    row_ptr, _, _, out_cols, out_vals = formats.coo_assemble(n_rows, n_cols, rows + base, cols + base, vals, base, base)
    asm = _device_assembled_hell(gpu, n_rows, n_cols, rows, cols, vals, "D", base, hs)
    lengths = np.diff(row_ptr)
    live = np.flatnonzero(lengths > 0)
    assert live.size == n_rows - 2
    chosen = row_ptr[live] - base + rng.integers(0, lengths[live])          # one entry of every non-empty row: first, last, any
    chosen[0], chosen[1] = row_ptr[live[0]] - base, row_ptr[live[1] + 1] - base - 1
    new = rng.standard_normal(live.size)
    order = rng.permutation(live.size)
    a_i, a_j, a_v = (live + base).astype(np.int32)[order], out_cols[chosen][order], new[order]
    d_ai, d_aj, d_av = formats.to_device(a_i), formats.to_device(a_j), formats.to_device(a_v)
    capi.hellcsput["D"](gpu, capi.scalar("D", 1), _p(asm["cM"]), _p(asm["rP"]), hs, _p(asm["ho"]), _p(asm["rS"]), None, n_rows, live.size,
                        _p(d_ai), _p(d_aj), _p(d_av), base)
    torch.cuda.synchronize()
    want_vals = out_vals.copy()
    want_vals[chosen] = new
    assert want_vals.tobytes() != out_vals.tobytes()
    src = dict(kind="hell", dtype=np.dtype(np.float64), rows=n_rows, base=base, hack_size=hs, slots=asm["slots"], cM=asm["cM"], rP=asm["rP"],
               hack_offsets=asm["ho"], rS=asm["rS"])
    _expect(_to_csr(gpu, src, base), row_ptr, out_cols, want_vals, int(lengths.max()))


# ---- 12. the step in a captured graph ----------------------------------------------------------------------------------------
def test_assemble_refill_spmv_replays_from_a_captured_graph(gpu):
    """spgpuCooAssembleValuesDevice -> spgpuCsrToHellValuesDevice -> spgpuDhellspmv as one linear chain on the handle's stream,
    replayed twice with cooValues rewritten in place in between: each replay gives the bits of the eager calls on the same values."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(12)
    n_rows, n_cols, base, hs, nnz = 512, 300, 0, 32, 12000
    rows, cols = _shuffled_list(rng, n_rows, n_cols, nnz)
    v1, v2, v3 = (_values(rng, nnz, "D") for _ in range(3))
    asm = _device_assembled_hell(gpu, n_rows, n_cols, rows, cols, v1, "D", base, hs)
    d_x = formats.to_device(rng.standard_normal(n_cols))
    d_z = torch.zeros(n_rows, dtype=torch.float64, device="cuda:0")

    def chain():
        assert capi.spgpuCooAssembleValuesDevice(gpu, _p(asm["vals"]), asm["unique"], nnz, _p(asm["coo_vals"]), capi.TYPE_DOUBLE, asm["perm"].ptr(),
                                                 asm["seg"].ptr()) == capi.SPGPU_SUCCESS
        assert capi.spgpuCsrToHellValuesDevice(gpu, _p(asm["cM"]), _p(asm["ho"]), hs, n_rows, _p(asm["ptr"]), _p(asm["vals"]), base,
                                               capi.TYPE_DOUBLE, None) == capi.SPGPU_SUCCESS
        _hellspmv(gpu, "D", d_z, asm, hs, n_rows, d_x, base)

    eager = []
    for values in (v2, v3):
        asm["coo_vals"].copy_(formats.to_device(values))
        torch.cuda.synchronize()
        chain()
        torch.cuda.synchronize()
        eager.append((d_z.cpu().numpy().tobytes(), asm["vals"].cpu().numpy().tobytes()))
        assert eager[-1][1] == formats.coo_assemble(n_rows, n_cols, rows, cols, values)[4].tobytes()
    assert eager[0][0] != eager[1][0]
    side = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            chain()
        for values, want in zip((v2, v3), eager):
            asm["coo_vals"].copy_(formats.to_device(values))
            asm["vals"].fill_(float("nan"))
            asm["cM"].fill_(float("nan"))
            d_z.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert (d_z.cpu().numpy().tobytes(), asm["vals"].cpu().numpy().tobytes()) == want
    finally:
        capi.spgpuSetStream(gpu, None)
