"""GPU: the device-side COO converters of include/spgpu/convert_device.h (COO -> ELL / HELL / HDIA / DIA) between guards, on the
listings of tests/coo_convert_cases.py, each of which sits on one threshold of those converters (profiles/coo_convert_coverage.md
lists them; tests/test_coo_convert_restated.py shows on the CPU that every case reaches its threshold).

Every device output -- rowLengths, the ELL values and indices, hackOffsets, the HELL values and indices, the HDIA values and
offsets, the DIA values and offsets -- and both scratch areas lie between 64 guard bytes of 0xA5 (_Guarded of
tests/test_gpu_to_csr_device.py); `work` and `scratch` have exactly the size the library's own byte-count call reports, 256-byte
aligned as hipMalloc would leave them.  The guards are checked after every call.

The values and index arrays are not zeroed but filled with a second pattern (0x3C): the contract is "destination arrays zeroed by
the caller", so the converters write the occupied slots and nothing else.  Which slots are occupied, and by which COO entry, comes
from the restatement in tests/test_coo_convert_restated.py (a dict of Python-int pairs, compared there with the host converters);
the device array must equal the pattern with those entries in place, byte for byte.  One case per family also runs with zeroed
arrays and compares whole arrays with the host converters'.  No comparison has a tolerance."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import coo_convert_cases as K
import test_coo_convert_restated as R
from test_gpu_to_csr_device import PATTERN, _Guarded

pytestmark = pytest.mark.gpu

FILL = 0x3C                      # what the destination arrays hold before a converter runs
AREA_OFFSET = 192                # _Guarded's 64 guard bytes + 192: `work` and `scratch` start on a 256-byte boundary


def _sync():
    import torch
    torch.cuda.synchronize()


def _out(nbytes, fill=FILL):
    """A guarded device output of `nbytes`, every byte `fill`."""
    g = _Guarded(nbytes)
    if nbytes:
        g.buf[g.first:g.first + nbytes] = fill
    return g


def _area(nbytes):
    """`work` or `scratch`: exactly `nbytes`, between guards, 256-byte aligned; its content is the guard pattern."""
    assert nbytes > 0
    g = _Guarded(nbytes, AREA_OFFSET)
    assert g.at % 256 == 0
    return g


def _intact(*guarded):
    _sync()
    for i, g in enumerate(guarded):
        assert g.guards_intact(), i


def _device(case):
    from spgpu_amd import formats
    some = lambda a: formats.to_device(a if a.size else np.zeros(1, a.dtype))
    return some(case.rows), some(case.cols), some(case.vals)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _code(case):
    from spgpu_amd import capi, formats
    return capi.TYPE_CODE[formats.LETTER_OF[np.dtype(case.vals.dtype)]]


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


@contextlib.contextmanager
def _side_stream(gpu):
    """The handle on a stream of its own, the default stream idle; the handle is put back whatever happens."""
    import torch
    from spgpu_amd import capi
    side = torch.cuda.Stream()
    _sync()
    capi.spgpuSetStream(gpu, C.c_void_p(side.cuda_stream))
    try:
        assert capi.spgpuGetStream(gpu) == side.cuda_stream
        yield side
    finally:
        _sync()
        capi.spgpuSetStream(gpu, None)


# ---- ELL / HELL ------------------------------------------------------------------------------------------------------------------
def _row_lengths(gpu, case, work, rows=None):
    """spgpuCooRowLengthsDevice on `work` (made here when None) -> (status, longest row, guarded rowLengths, work, device COO)."""
    from spgpu_amd import capi, formats
    n, nnz = case.n_rows, int(case.rows.size)
    work = work or _area(capi.spgpuCooConvertWorkBytes(n, nnz))
    assert work.nbytes == capi.spgpuCooConvertWorkBytes(n, nnz)
    coo = _device(case if rows is None else K.with_entries(case, rows=rows))
    rs = _out(n * 4)
    longest = C.c_int(-1)
    _sync()
    st = capi.spgpuCooRowLengthsDevice(gpu, rs.ptr(), C.byref(longest), n, nnz, _p(coo[0]), case.coo_base, work.ptr())
    _intact(rs, work)
    return st, longest.value, rs, work, coo


def _ell_and_hell(gpu, case, out_base, hack_sizes, pitches=(0, 0), fill=FILL, work=None):
    """The four calls on guarded arrays filled with `fill`; every array against the restatement.  `pitches`: what is added to
    computeEllAllocPitch(rows) for the values and for the indices.  Returns (work, ell arrays, {hack size: hell arrays})."""
    from spgpu_amd import capi
    n, nnz, size = case.n_rows, int(case.rows.size), case.vals.dtype.itemsize
    pitch = capi.computeEllAllocPitch(n)
    book = R.ell_by_the_book(case, out_base, pitch + pitches[0], pitch + pitches[1])
    vp, ip = book["values_pitch"], book["indices_pitch"]
    assert min(vp, ip) >= n and (vp, ip) == (pitch + pitches[0], pitch + pitches[1])
    st, longest, rs, work, (dr, dc, dv) = _row_lengths(gpu, case, work)
    assert st == capi.SPGPU_SUCCESS and longest == book["max_row"]
    if n:
        _same(rs.numpy(np.int32), book["row_lengths"], "rowLengths")
    else:
        assert rs.untouched()
    ell_v, ell_i = _out(longest * vp * size, fill), _out(longest * ip * 4, fill)
    _sync()
    assert capi.spgpuCooToEllDevice(gpu, ell_v.ptr(), ell_i.ptr(), vp, ip, out_base, n, nnz, _p(dr), _p(dc), _p(dv), case.coo_base,
                                    _code(case), rs.ptr(), work.ptr()) == capi.SPGPU_SUCCESS
    _intact(ell_v, ell_i, rs, work)
    ell = dict(max_row=longest, row_lengths=rs.numpy(np.int32), values=ell_v.numpy(case.vals.dtype), indices=ell_i.numpy(np.int32))
    _same(ell["values"], R.filled(longest * vp, case.vals.dtype, book["value_slots"], case.vals, fill), "ELL values")
    _same(ell["indices"], R.filled(longest * ip, np.int32, book["index_slots"], book["stored"], fill), "ELL indices")
    hells = {}
    for hs in hack_sizes:
        want = R.hell_by_the_book(book, hs)
        hacks = (n + hs - 1) // hs
        ho = _out(hacks * 4)
        height = C.c_int(-1)
        _sync()
        assert capi.spgpuHellPlanDevice(gpu, C.byref(height), ho.ptr(), hs, n, rs.ptr(), work.ptr()) == capi.SPGPU_SUCCESS
        _intact(ho, rs, work)
        assert height.value == want["height"], hs
        _same(ho.numpy(np.int32), want["hack_offsets"], ("hackOffsets", hs))
        slots = hs * height.value
        hell_v, hell_i = _out(slots * size, fill), _out(slots * 4, fill)
        _sync()
        assert capi.spgpuCooToHellDevice(gpu, hell_v.ptr(), hell_i.ptr(), ho.ptr(), hs, out_base, n, nnz, _p(dr), _p(dc), _p(dv),
                                         case.coo_base, _code(case), rs.ptr(), work.ptr()) == capi.SPGPU_SUCCESS
        _intact(hell_v, hell_i, ho, rs, work)
        hells[hs] = dict(height=height.value, hack_offsets=ho.numpy(np.int32), values=hell_v.numpy(case.vals.dtype),
                         indices=hell_i.numpy(np.int32))
        _same(hells[hs]["values"], R.filled(slots, case.vals.dtype, want["slots"], case.vals, fill), ("HELL values", hs))
        _same(hells[hs]["indices"], R.filled(slots, np.int32, want["slots"], book["stored"], fill), ("HELL indices", hs))
    return work, ell, hells


def _whole_ell_and_hell_against_the_host(gpu, case, out_base, hack_sizes, pitches):
    """Zeroed destinations: whole arrays against formats.coo_to_ell (once per pitch) and formats.ell_to_hell."""
    from spgpu_amd import capi, formats
    _, ell, hells = _ell_and_hell(gpu, case, out_base, hack_sizes, pitches, fill=0)
    pitch = capi.computeEllAllocPitch(case.n_rows)
    host = [formats.coo_to_ell(case.n_rows, case.rows, case.cols, case.vals, coo_base=case.coo_base, ell_base=out_base, pitch=pitch + p)
            for p in pitches]
    assert ell["max_row"] == host[0]["max_row"]
    _same(ell["row_lengths"], host[0]["row_lengths"], "rowLengths")
    _same(ell["values"], host[0]["values"], "ELL values")
    _same(ell["indices"], host[1]["indices"], "ELL indices")
    for hs in hack_sizes:
        host_hell = formats.ell_to_hell(host[0], hs)
        assert hells[hs]["height"] == host_hell["height"]
        for name in ("hack_offsets", "values", "indices"):
            _same(hells[hs][name], host_hell[name], (name, hs))


@pytest.mark.parametrize("letter", "SDCZ")
def test_ell_and_hell_with_every_pair_of_bases_and_two_pitches(gpu, letter):
    """1. cooBase and the output base differ in two of the four pairs; the values' and the indices' pitch differ always: one is
    computeEllAllocPitch(rows), the other 32 or 64 more.  Hack sizes 32 and 96 (one hack, deeper than the matrix)."""
    for at, (coo_base, out_base) in enumerate(K.BASE_PAIRS):
        case = K.ell_base_pairs(letter, coo_base)
        pitches = ((0, 32), (64, 0))[at % 2]
        _ell_and_hell(gpu, case, out_base, case.info["hack_sizes"], pitches)
    _whole_ell_and_hell_against_the_host(gpu, K.ell_base_pairs(letter, 0), 1, (32, 96), (0, 32))


@pytest.mark.parametrize("n_rows", K.ROW_COUNTS)
def test_ell_row_counts_around_powers_of_two_and_refusals_on_one_work_area(gpu, n_rows):
    """2. The row sort takes the smallest number of bits that holds the key `rows` (= outside the matrix).  A good run, a row index
    at base + rows, one at base - 1 -- SPGPU_UNSUPPORTED, guards intact (_row_lengths) --, then the good run again, all on one
    `work`."""
    from spgpu_amd import capi
    for coo_base in (0, 1):
        case = K.ell_row_counts(n_rows, coo_base)
        work, first, _ = _ell_and_hell(gpu, case, 1 - coo_base, (32,))
        for bad in ("row_too_high", "row_too_low"):
            st, _, _, _, _ = _row_lengths(gpu, case, work, rows=case.info[bad])
            assert st == capi.SPGPU_UNSUPPORTED, (bad, coo_base)
        _, again, _ = _ell_and_hell(gpu, case, 1 - coo_base, (32,), work=work)
        assert all(np.asarray(first[k]).tobytes() == np.asarray(again[k]).tobytes() for k in first)


@pytest.mark.parametrize("coo_base", [0, 1])
def test_ell_and_hell_with_column_indices_up_to_int_max(gpu, coo_base):
    """3. 70 x (2^31 - 1): cooCols - cooBase + outBase with the largest column an int holds, on either side."""
    case = K.ell_wide_columns(coo_base)
    for out_base in (0, 1):
        _, ell, _ = _ell_and_hell(gpu, case, out_base, case.info["hack_sizes"], (32, 0))
        stored = ell["indices"][ell["indices"] != np.full(1, FILL, np.uint8).repeat(4).view(np.int32)[0]]
        assert int(stored.max()) == 2 ** 31 - 2 + out_base and int(stored.min()) == out_base


@pytest.mark.parametrize("hacks", K.HELL_PLAN_HACKS)
def test_hell_plan_at_the_tile_edge(gpu, hacks):
    """4. 1, 1 023, 1 024 and 1 025 hack depths to scan: one tile, one tile less one, a full tile, two tiles."""
    case = K.hell_plan_hacks(hacks)
    _ell_and_hell(gpu, case, 1 - case.coo_base, (case.info["hack_size"],))


def test_hell_plan_scan_that_carries(gpu):
    """4. 262 147 hacks of two rows: 257 tiles, so scanTotalsKernel of convert_device.hip goes round twice and carries."""
    case = K.hell_plan_carry()
    assert case.info["scan_tiles"] > K.CARRY_TILES
    _ell_and_hell(gpu, case, 0, (case.info["hack_size"],))


@pytest.mark.parametrize("kind", ["no entries", "no rows", "one entry"])
def test_ell_and_hell_degenerate(gpu, kind):
    """5. With no entries rowLengths and hackOffsets are zeros and nothing else is written; with no rows nothing at all is."""
    case = K.ell_degenerate(kind)
    work, ell, hells = _ell_and_hell(gpu, case, 0, (32,))
    assert ell["max_row"] == (kind == "one entry") and hells[32]["height"] == (kind == "one entry")
    if kind == "no rows":
        assert work.untouched()


def test_ell_and_hell_on_a_side_stream(gpu):
    """14. The same bytes with the handle on a stream of its own."""
    case = K.ell_base_pairs("Z", 1)
    _, ell, hells = _ell_and_hell(gpu, case, 0, (32,), (0, 32))
    with _side_stream(gpu):
        _, side_ell, side_hells = _ell_and_hell(gpu, case, 0, (32,), (0, 32))
    assert all(np.asarray(ell[k]).tobytes() == np.asarray(side_ell[k]).tobytes() for k in ell)
    assert all(np.asarray(hells[32][k]).tobytes() == np.asarray(side_hells[32][k]).tobytes() for k in hells[32])


def test_hell_plan_without_a_hack_size_or_rows_writes_nothing(gpu):
    """13. spgpuHellPlanDevice with hackSize <= 0 or no rows: height 0, SPGPU_SUCCESS as its first lines say, nothing written."""
    from spgpu_amd import capi, formats
    rs = formats.to_device(np.ones(70, np.int32))
    for hack_size, n_rows in ((0, 70), (-32, 70), (32, 0), (32, -5)):
        work, ho, height = _area(capi.spgpuCooConvertWorkBytes(70, 0)), _out(3 * 4), C.c_int(-1)
        _sync()
        assert capi.spgpuHellPlanDevice(gpu, C.byref(height), ho.ptr(), hack_size, n_rows, _p(rs), work.ptr()) == capi.SPGPU_SUCCESS
        _sync()
        assert height.value == 0 and work.untouched() and ho.guards_intact() and (ho.numpy(np.uint8) == FILL).all()


# ---- HDIA ------------------------------------------------------------------------------------------------------------------------
def _hdia(gpu, case, hack_size=None, fill=FILL, work=None, refused=False):
    """spgpuCooHdiaPlanDevice and spgpuCooToHdiaDevice on guarded arrays, against the restatement.  With `refused` the plan must
    return SPGPU_UNSUPPORTED with height 0.  Returns (work, arrays or None)."""
    from spgpu_amd import capi
    hs = hack_size or case.info["hack_size"]
    n, nnz, size = case.n_rows, int(case.rows.size), case.vals.dtype.itemsize
    work = work or _area(capi.spgpuCooHdiaPlanWorkBytes(n, nnz))
    assert work.nbytes == capi.spgpuCooHdiaPlanWorkBytes(n, nnz)
    dr, dc, dv = _device(case)
    hacks = capi.getHdiaHacksCount(hs, n)
    ho = _out((hacks + 1) * 4)
    height = C.c_int(-1)
    _sync()
    st = capi.spgpuCooHdiaPlanDevice(gpu, C.byref(height), ho.ptr(), hs, n, case.n_cols, nnz, _p(dr), _p(dc), case.coo_base, work.ptr())
    _intact(ho, work)
    if refused:
        assert st == capi.SPGPU_UNSUPPORTED and height.value == 0
        return work, None
    want = R.hdia_by_the_book(case, R.book(case), hs)
    assert st == capi.SPGPU_SUCCESS and height.value == want["height"]
    _same(ho.numpy(np.int32), want["hack_offsets"], "hackOffsets")
    slots = hs * height.value
    values, offsets = _out(slots * size, fill), _out(height.value * 4)
    scratch = _area(capi.spgpuCooToHdiaScratchBytes(hs, height.value))
    _sync()
    assert capi.spgpuCooToHdiaDevice(gpu, values.ptr(), offsets.ptr(), ho.ptr(), hs, n, case.n_cols, nnz, _p(dr), _p(dc), _p(dv),
                                     case.coo_base, _code(case), height.value, work.ptr(), scratch.ptr()) == capi.SPGPU_SUCCESS
    _intact(values, offsets, scratch, ho, work)
    got = dict(height=height.value, hack_offsets=ho.numpy(np.int32), offsets=offsets.numpy(np.int32), values=values.numpy(case.vals.dtype))
    _same(got["offsets"], want["offsets"], "hdiaOffsets")
    _same(got["values"], R.filled(slots, case.vals.dtype, want["slots"], case.vals[want["owners"]], fill), "hdiaValues")
    return work, got


def _whole_hdia_against_the_host(gpu, case):
    from spgpu_amd import formats
    _, got = _hdia(gpu, case, fill=0)
    host = formats.coo_to_hdia(case.n_rows, case.n_cols, case.rows, case.cols, case.vals, case.info["hack_size"], coo_base=case.coo_base)
    assert got["height"] == host["height"]
    for name in ("hack_offsets", "offsets", "values"):
        _same(got[name], host[name], name)


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("hack_size", K.HDIA_HACK_SIZES)
def test_hdia_hack_sizes_and_row_counts(gpu, letter, hack_size):
    """6. 1, hackSize - 1, hackSize, hackSize + 1 and 3 * hackSize + 5 rows, wider than tall and taller than wide, both bases: the
    extreme offsets, a hack with no diagonal between two that have some, a hack with one diagonal, a last hack of five rows."""
    for n_rows in K.hdia_row_counts(hack_size):
        for coo_base, wide in ((0, True), (1, False), (1, True), (0, False)):
            _hdia(gpu, K.hdia_shape(hack_size, n_rows, letter, coo_base, wide))
    _whole_hdia_against_the_host(gpu, K.hdia_shape(hack_size, 3 * hack_size + 5, letter, 1, True))


def test_hdia_single_entry(gpu):
    for coo_base in (0, 1):
        _, got = _hdia(gpu, K.hdia_single_entry(coo_base))
        assert got["hack_offsets"].tolist() == [0, 0, 1, 1] and got["offsets"].tolist() == [-37]


@pytest.mark.parametrize("coo_base", [0, 1])
@pytest.mark.parametrize("hack_size", K.HDIA_WIDE_HACK_SIZES)
def test_hdia_keys_whose_low_word_passes_2_to_31(gpu, hack_size, coo_base):
    """7. 70 x (2^31 - 1): column - row % hackSize + hackSize passes INT_MAX for the last hackSize columns; the key must order
    and come apart again as if it had not."""
    for letter in "DS":
        _, got = _hdia(gpu, K.hdia_wide(hack_size, coo_base, letter))
        assert int(got["offsets"].max()) == 2 ** 31 - 2


def test_hdia_slot_with_100k_writers(gpu):
    """8. The entry with the largest COO position is stored, in this order and in the opposite one."""
    case = K.hdia_contention()
    r, c = case.info["slot"]
    stored = []
    for listing in (case, K.reversed_listing(case)):
        _, got = _hdia(gpu, listing)
        want = R.hdia_by_the_book(listing, R.book(listing), 32)
        at = int(want["slots"][list(R.book(listing)).index((r, c))])
        stored.append(got["values"][at])
    assert stored[0] != stored[1]
    _whole_hdia_against_the_host(gpu, case)


@pytest.mark.parametrize("coo_base", [0, 1])
def test_hdia_refusals_and_then_a_good_matrix_on_one_work_area(gpu, coo_base):
    """9. An entry outside the matrix by row or by column, above or below: SPGPU_UNSUPPORTED and height 0; the same `work` then
    serves the good listing."""
    case = K.hdia_refused(coo_base)
    work, first = _hdia(gpu, case)
    for kind in K.OUTSIDE:
        _hdia(gpu, K.spoilt(case, kind), work=work, refused=True)
        _, again = _hdia(gpu, case, work=work)
        assert all(np.asarray(first[k]).tobytes() == np.asarray(again[k]).tobytes() for k in first), kind


def test_hdia_on_a_side_stream(gpu):
    case = K.hdia_shape(32, 101, "C", 1, True)
    _, got = _hdia(gpu, case)
    with _side_stream(gpu):
        _, side = _hdia(gpu, case)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(side[k]).tobytes() for k in got)


# ---- DIA -------------------------------------------------------------------------------------------------------------------------
def _dia(gpu, case, extra_pitch=0, fill=FILL, work=None, refused=False):
    """spgpuCooDiaPlanDevice and spgpuCooToDiaDevice on guarded arrays with valuesPitch = computeDiaAllocPitch(rows) +
    extra_pitch, against the restatement.  Returns (work, arrays or None)."""
    from spgpu_amd import capi
    n, nnz, size = case.n_rows, int(case.rows.size), case.vals.dtype.itemsize
    work = work or _area(capi.spgpuCooDiaWorkBytes(n, case.n_cols))
    assert work.nbytes == capi.spgpuCooDiaWorkBytes(n, case.n_cols)
    dr, dc, dv = _device(case)
    count = C.c_int(-1)
    _sync()
    st = capi.spgpuCooDiaPlanDevice(gpu, C.byref(count), n, case.n_cols, nnz, _p(dr), _p(dc), case.coo_base, work.ptr())
    _intact(work)
    if refused:
        assert st == capi.SPGPU_UNSUPPORTED and count.value == 0
        return work, None
    pitch = capi.computeDiaAllocPitch(n) + extra_pitch
    want = R.dia_by_the_book(case, R.book(case), pitch)
    assert st == capi.SPGPU_SUCCESS and count.value == want["diags"]
    values, offsets = _out(pitch * count.value * size, fill), _out(count.value * 4)
    scratch = _area(capi.spgpuCooToDiaScratchBytes(pitch, count.value))
    _sync()
    assert capi.spgpuCooToDiaDevice(gpu, values.ptr(), offsets.ptr(), pitch, count.value, n, case.n_cols, nnz, _p(dr), _p(dc), _p(dv),
                                    case.coo_base, _code(case), work.ptr(), scratch.ptr()) == capi.SPGPU_SUCCESS
    _intact(values, offsets, scratch, work)
    got = dict(diags=count.value, offsets=offsets.numpy(np.int32), values=values.numpy(case.vals.dtype))
    _same(got["offsets"], want["offsets"], "offsets")
    _same(got["values"], R.filled(pitch * count.value, case.vals.dtype, want["slots"], case.vals[want["owners"]], fill), "values")
    return work, got


def _whole_dia_against_the_host(gpu, case):
    from spgpu_amd import formats
    _, got = _dia(gpu, case, fill=0)
    host = formats.coo_to_dia(case.n_rows, case.n_cols, case.rows, case.cols, case.vals, coo_base=case.coo_base)
    assert got["diags"] == host["diags"]
    _same(got["offsets"], host["offsets"], "offsets")
    _same(got["values"], host["values"], "values")


@pytest.mark.parametrize("span", K.DIA_SPANS)
def test_dia_spans_at_the_tile_edge(gpu, span):
    """10. and 12. rows + cols - 1 = 1 023 .. 1 026 flags to scan; S, D, C and Z, both bases; valuesPitch equal to
    computeDiaAllocPitch(rows) and 32 and 7 greater."""
    for at, letter in enumerate("SDCZ"):
        for coo_base in (0, 1):
            _dia(gpu, K.dia_span(span, coo_base, letter), extra_pitch=(0, 32, 7)[(at + coo_base) % 3])
    _whole_dia_against_the_host(gpu, K.dia_span(span, 1, "Z"))


def test_dia_scan_that_carries(gpu):
    """10. 270 000 flags: 264 tiles, diagonals at the first and the last flag and either side of flag 262 144, where the second
    round of scanTotalsKernel starts."""
    case = K.dia_carry()
    assert case.info["scan_tiles"] > K.CARRY_TILES
    _, got = _dia(gpu, case)
    assert got["diags"] == 8 and set(case.info["astride"]) <= set(got["offsets"].tolist())


def test_dia_slot_with_50k_writers(gpu):
    """11. As for HDIA: the last entry in COO order is stored, whichever end of the list that is."""
    case = K.dia_contention()
    r, c = case.info["slot"]
    stored = []
    for listing in (case, K.reversed_listing(case)):
        _, got = _dia(gpu, listing, extra_pitch=32)
        want = R.dia_by_the_book(listing, R.book(listing), 320 + 32)
        stored.append(got["values"][int(want["slots"][list(R.book(listing)).index((r, c))])])
    assert stored[0] != stored[1]
    _whole_dia_against_the_host(gpu, case)


@pytest.mark.parametrize("coo_base", [0, 1])
def test_dia_refusals_and_then_a_good_matrix_on_one_work_area(gpu, coo_base):
    """12. An entry outside the matrix: SPGPU_UNSUPPORTED from the plan, then the good listing on the same `work`; and a
    valuesPitch below the row count: SPGPU_UNSUPPORTED from the fill, nothing written."""
    from spgpu_amd import capi
    case = K.dia_refused(coo_base)
    work, first = _dia(gpu, case)
    for kind in K.OUTSIDE:
        _dia(gpu, K.spoilt(case, kind), work=work, refused=True)
        _, again = _dia(gpu, case, work=work)
        assert all(np.asarray(first[k]).tobytes() == np.asarray(again[k]).tobytes() for k in first), kind
    dr, dc, dv = _device(case)
    n, nnz, diags = case.n_rows, int(case.rows.size), first["diags"]
    values, offsets, scratch = _out(n * diags * 8), _out(diags * 4), _area(capi.spgpuCooToDiaScratchBytes(n, diags))
    _sync()
    assert capi.spgpuCooToDiaDevice(gpu, values.ptr(), offsets.ptr(), n - 1, diags, n, case.n_cols, nnz, _p(dr), _p(dc), _p(dv), coo_base,
                                    _code(case), work.ptr(), scratch.ptr()) == capi.SPGPU_UNSUPPORTED
    _sync()
    assert scratch.untouched() and all(g.guards_intact() and (g.numpy(np.uint8) == FILL).all() for g in (values, offsets))


def test_dia_on_a_side_stream(gpu):
    case = K.dia_span(1025, 0, "S")
    _, got = _dia(gpu, case, extra_pitch=32)
    with _side_stream(gpu):
        _, side = _dia(gpu, case, extra_pitch=32)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(side[k]).tobytes() for k in got)


# ---- 13. the argument refusals of the HDIA and DIA entry points -------------------------------------------------------------------
def _nothing_written(outputs, areas):
    _sync()
    assert all(a.untouched() for a in areas) and all(o.guards_intact() and (o.numpy(np.uint8) == FILL).all() for o in outputs)


def test_hdia_entry_points_refuse_bad_arguments_and_write_nothing(gpu):
    """What the first lines of spgpuCooHdiaPlanDevice and spgpuCooToHdiaDevice refuse: a null handle, height, hackOffsets, work or
    scratch, hackSize <= 0, negative counts.  SPGPU_UNSUPPORTED; outputs, work and scratch keep their bytes."""
    from spgpu_amd import capi
    case = K.hdia_refused(0)
    n, m, nnz, hs = case.n_rows, case.n_cols, int(case.rows.size), 32
    dr, dc, dv = _device(case)
    work, ho = _area(capi.spgpuCooHdiaPlanWorkBytes(n, nnz)), _out((capi.getHdiaHacksCount(hs, n) + 1) * 4)
    height = C.c_int(-1)
    good = dict(handle=gpu, height=C.byref(height), ho=ho.ptr(), hs=hs, n=n, nnz=nnz, work=work.ptr())
    for bad in (dict(handle=None), dict(height=None), dict(ho=None), dict(work=None), dict(hs=0), dict(hs=-32), dict(n=-1), dict(nnz=-1)):
        a = dict(good, **bad)
        _sync()
        st = capi.spgpuCooHdiaPlanDevice(a["handle"], a["height"], a["ho"], a["hs"], a["n"], m, a["nnz"], _p(dr), _p(dc), 0, a["work"])
        assert st == capi.SPGPU_UNSUPPORTED and height.value == -1, bad
        _nothing_written((ho,), (work,))
    values, offsets, scratch = _out(hs * 10 * 8), _out(10 * 4), _area(capi.spgpuCooToHdiaScratchBytes(hs, 10))
    good = dict(handle=gpu, hs=hs, n=n, nnz=nnz, height=10, work=work.ptr(), scratch=scratch.ptr())
    for bad in (dict(handle=None), dict(work=None), dict(scratch=None), dict(hs=0), dict(hs=-32), dict(n=-1), dict(nnz=-1), dict(height=-1)):
        a = dict(good, **bad)
        _sync()
        st = capi.spgpuCooToHdiaDevice(a["handle"], values.ptr(), offsets.ptr(), ho.ptr(), a["hs"], a["n"], m, a["nnz"], _p(dr), _p(dc),
                                       _p(dv), 0, _code(case), a["height"], a["work"], a["scratch"])
        assert st == capi.SPGPU_UNSUPPORTED, bad
        _nothing_written((values, offsets, ho), (work, scratch))
    _hdia(gpu, case, work=work)                                # the handle and the area serve a good call afterwards


def test_dia_entry_points_refuse_bad_arguments_and_write_nothing(gpu):
    """What the first lines of spgpuCooDiaPlanDevice and spgpuCooToDiaDevice refuse: a null handle, count, work or scratch, negative
    counts, valuesPitch < rowsCount.  SPGPU_UNSUPPORTED; outputs, work and scratch keep their bytes."""
    from spgpu_amd import capi
    case = K.dia_refused(0)
    n, m, nnz = case.n_rows, case.n_cols, int(case.rows.size)
    dr, dc, dv = _device(case)
    work = _area(capi.spgpuCooDiaWorkBytes(n, m))
    count = C.c_int(-1)
    good = dict(handle=gpu, count=C.byref(count), n=n, m=m, nnz=nnz, work=work.ptr())
    for bad in (dict(handle=None), dict(count=None), dict(work=None), dict(n=-1), dict(m=-1), dict(nnz=-1)):
        a = dict(good, **bad)
        _sync()
        st = capi.spgpuCooDiaPlanDevice(a["handle"], a["count"], a["n"], a["m"], a["nnz"], _p(dr), _p(dc), 0, a["work"])
        assert st == capi.SPGPU_UNSUPPORTED and count.value == -1, bad
        _nothing_written((), (work,))
    pitch = capi.computeDiaAllocPitch(n)
    values, offsets, scratch = _out(pitch * 4 * 8), _out(4 * 4), _area(capi.spgpuCooToDiaScratchBytes(pitch, 4))
    good = dict(handle=gpu, pitch=pitch, diags=4, nnz=nnz, work=work.ptr(), scratch=scratch.ptr())
    for bad in (dict(handle=None), dict(work=None), dict(scratch=None), dict(pitch=n - 1), dict(diags=-1), dict(nnz=-1)):
        a = dict(good, **bad)
        _sync()
        st = capi.spgpuCooToDiaDevice(a["handle"], values.ptr(), offsets.ptr(), a["pitch"], a["diags"], n, m, a["nnz"], _p(dr), _p(dc),
                                      _p(dv), 0, _code(case), a["work"], a["scratch"])
        assert st == capi.SPGPU_UNSUPPORTED, bad
        _nothing_written((values, offsets), (work, scratch))
    _dia(gpu, case, work=work)
