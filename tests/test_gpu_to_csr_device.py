"""GPU: device-side HELL / ELL -> CSR construction (include/spgpu/ext/to_csr_device.h): the bytes of the CSR arrays -- exact and
independent of any library -- for every value type, both index bases on either side, hack sizes that are and are not multiples of
32, rows of any length, a row order through rIdx, values as bit patterns, padding that is never read, and the refusals of the
row-pointer call.

Every small conversion runs THREE times -- the public call and each fill through the unexported spgpu{Hell,Ell}ToCsrDeviceWith --
and the three results must be the same bytes.  Every destination array lies between 64 guard bytes of a fixed pattern on both
sides, and the guards must be intact afterwards (_to_csr)."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as O
from test_gpu_csr_device import _hell_plan, _p, _row_lengths, _to_hell, _zeros

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0xA5


class _Guarded:
    """`nbytes` of HBM at `offset` bytes behind a 16-byte boundary, between GUARD bytes of PATTERN (the bytes in front of the array up
    to the allocation's start, `offset` included, belong to the front guard)."""

    def __init__(self, nbytes, offset=0):
        import torch
        self.first, self.nbytes = GUARD + offset, nbytes
        self.buf = torch.full((self.first + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        self.at = self.buf.data_ptr() + self.first

    def ptr(self):
        return C.c_void_p(self.at)

    def guards_intact(self):
        return bool((self.buf[:self.first] == PATTERN).all()) and bool((self.buf[self.first + self.nbytes:] == PATTERN).all())

    def untouched(self):
        return bool((self.buf == PATTERN).all())

    def numpy(self, dtype):
        return self.buf[self.first:self.first + self.nbytes].cpu().numpy().view(dtype)


def _hell_source(hell, dtype=None):
    """A dict of ell_to_hell (host arrays) -> the source in HBM."""
    from spgpu_amd import formats
    return dict(kind="hell", dtype=np.dtype(dtype or hell["values"].dtype), rows=hell["rows"], base=hell["base"],
                hack_size=hell["hack_size"], slots=int(hell["indices"].size), cM=formats.to_device(_some(hell["values"])),
                rP=formats.to_device(_some(hell["indices"])), hack_offsets=formats.to_device(_some(hell["hack_offsets"])),
                rS=formats.to_device(_some(hell["row_lengths"])))


def _some(a):
    return a if a.size else np.zeros(1, a.dtype)


def _repitch(a, depth, old, new):
    out = np.zeros(depth * new, a.dtype)
    out.reshape(depth, new)[:, :old] = a.reshape(depth, old)
    return out


def _ell_source(ell, values_pitch, indices_pitch):
    """A dict of coo_to_ell (host arrays) -> the source in HBM with a pitch each for the values and the indices."""
    from spgpu_amd import formats
    depth = ell["max_row"]
    return dict(kind="ell", dtype=np.dtype(ell["values"].dtype), rows=ell["rows"], base=ell["base"], slots=indices_pitch * depth,
                values_pitch=values_pitch, indices_pitch=indices_pitch,
                cM=formats.to_device(_some(_repitch(ell["values"], depth, ell["pitch"], values_pitch))),
                rP=formats.to_device(_some(_repitch(ell["indices"], depth, ell["pitch"], indices_pitch))),
                rS=formats.to_device(_some(ell["row_lengths"])))


def _row_ptr_call(gpu, src, csr_base, d_ridx, row_ptr, nnz, longest, work, slots=None):
    from spgpu_amd import capi
    slots = src["slots"] if slots is None else slots
    if src["kind"] == "hell":
        return capi.spgpuHellToCsrRowPtrDevice(gpu, row_ptr.ptr(), C.byref(nnz), C.byref(longest), csr_base, src["hack_size"],
                                               _p(src["hack_offsets"]), _p(src["rS"]), _p(d_ridx), src["rows"], slots, _p(work))
    return capi.spgpuEllToCsrRowPtrDevice(gpu, row_ptr.ptr(), C.byref(nnz), C.byref(longest), csr_base, src["indices_pitch"],
                                          _p(src["rS"]), _p(d_ridx), src["rows"], slots, _p(work))


def _fill_call(gpu, src, which, cols, vals, row_ptr, csr_base, d_ridx, max_blocks=0):
    """which None: the public call; else the fill of that number through the unexported entry point."""
    from spgpu_amd import capi, formats
    code = capi.TYPE_CODE[formats.LETTER_OF[src["dtype"]]]
    if src["kind"] == "hell":
        args = (gpu, cols.ptr(), vals.ptr(), row_ptr.ptr(), csr_base, _p(src["cM"]), _p(src["rP"]), src["hack_size"],
                _p(src["hack_offsets"]), _p(src["rS"]), _p(d_ridx), src["rows"], src["base"], code)
        return capi.spgpuHellToCsrDevice(*args) if which is None else capi.spgpuHellToCsrDeviceWith(*args, which, max_blocks)
    args = (gpu, cols.ptr(), vals.ptr(), row_ptr.ptr(), csr_base, _p(src["cM"]), _p(src["rP"]), src["values_pitch"], src["indices_pitch"],
            _p(src["rS"]), _p(d_ridx), src["rows"], src["base"], code)
    return capi.spgpuEllToCsrDevice(*args) if which is None else capi.spgpuEllToCsrDeviceWith(*args, which, max_blocks)


def _to_csr(gpu, src, csr_base, r_idx=None, misalign=False, runs=None):
    """The row-pointer call, then the fill once per entry of `runs` ((which, maxBlocks); default: the public call and each fill): all
    runs must give the same bytes and leave every guard intact.  Returns (nnz, longest, row_ptr, cols, vals) as numpy arrays."""
    import torch
    from spgpu_amd import capi, formats
    runs = runs or ((None, 0), (capi.TO_CSR_FILL_PLAIN, 0), (capi.TO_CSR_FILL_TRANSPOSE, 0))
    n, size = src["rows"], src["dtype"].itemsize
    d_ridx = r_idx if r_idx is None or isinstance(r_idx, torch.Tensor) else formats.to_device(np.ascontiguousarray(r_idx, np.int32))
    work = torch.empty(capi.spgpuToCsrWorkBytes(n), dtype=torch.uint8, device="cuda:0")
    row_ptr = _Guarded((n + 1) * 4)
    nnz, longest = C.c_int(-1), C.c_int(-1)
    torch.cuda.synchronize()
    assert _row_ptr_call(gpu, src, csr_base, d_ridx, row_ptr, nnz, longest, work) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    assert row_ptr.guards_intact()
    del work                                                # free again when the row-pointer call has returned
    results = []
    for which, max_blocks in runs:
        cols = _Guarded(nnz.value * 4, 4 if misalign else 0)
        vals = _Guarded(nnz.value * size, min(size, 8) if misalign else 0)
        torch.cuda.synchronize()
        assert _fill_call(gpu, src, which, cols, vals, row_ptr, csr_base, d_ridx, max_blocks) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        assert cols.guards_intact() and vals.guards_intact() and row_ptr.guards_intact(), (which, max_blocks)
        results.append((cols.numpy(np.int32), vals.numpy(src["dtype"])))
    for (which, max_blocks), (c, v) in zip(runs[1:], results[1:]):
        assert c.tobytes() == results[0][0].tobytes() and v.tobytes() == results[0][1].tobytes(), (which, max_blocks)
    return nnz.value, longest.value, row_ptr.numpy(np.int32), results[0][0], results[0][1]


def _expect(got, want_ptr, want_cols, want_vals, longest):
    nnz, got_longest, ptr, cols, vals = got
    assert nnz == want_cols.size and got_longest == longest
    assert ptr.tobytes() == np.ascontiguousarray(want_ptr, np.int32).tobytes()
    assert cols.tobytes() == np.ascontiguousarray(want_cols, np.int32).tobytes()
    assert vals.dtype == want_vals.dtype and vals.tobytes() == np.ascontiguousarray(want_vals).tobytes()


def _csr_of(n, r, c, v, src_base, csr_base):
    """synth.coo_to_csr of the listing, the row pointers and columns moved to csr_base."""
    from spgpu_amd import synth
    ptr, cols, vals = synth.coo_to_csr(n, r, c, v, src_base)
    return (ptr - src_base + csr_base).astype(np.int32), (cols - src_base + csr_base).astype(np.int32), vals


def _pitches(ell):
    return ell["pitch"] + 64, ell["pitch"] + 32             # values, indices: different, and both greater than the row count


# ---- 1. random matrices ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
def test_random_matrices_give_the_csr_of_the_listing(gpu, letter):
    """About 1 000 rows of 0 .. 70 entries with duplicates, shuffled COO: HELL from the host converters at five hack sizes (partial
    last groups, hacks that are no multiple of 32) and ELL with two pitches, both bases on both sides."""
    from spgpu_amd import formats, synth
    rng = np.random.default_rng(300 + ord(letter))
    n = 1003
    lengths = rng.integers(0, 71, n)
    for src_base, csr_base in ((0, 0), (0, 1), (1, 0), (1, 1)):
        _, _, r, c, v = synth.random_rows_coo(n, 50, lengths, seed=40 + src_base, letter=letter, base=src_base, shuffle=True)
        want = _csr_of(n, r, c, v, src_base, csr_base)
        ell = formats.coo_to_ell(n, r, c, v, coo_base=src_base, ell_base=src_base)
        for hs in (32, 64, 8, 24, 40):
            _expect(_to_csr(gpu, _hell_source(formats.ell_to_hell(ell, hs)), csr_base), *want, int(lengths.max()))
        vp, ip = _pitches(ell)
        assert vp != ip and min(vp, ip) > n
        _expect(_to_csr(gpu, _ell_source(ell, vp, ip), csr_base), *want, int(lengths.max()))


# ---- 2. chunk and group edges ---------------------------------------------------------------------------------------
def _edge_lengths():
    lengths = np.zeros(100, np.int64)
    lengths[:11] = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49)     # one group: K-1, K, K+1 around one, two and three chunks
    lengths[12:32] = np.arange(20) % 6
    # rows 32 .. 63: a whole group empty;  rows 64 .. 95: one row of 300 among empty rows;  rows 96 .. 99: a partial last group
    lengths[70] = 300
    lengths[97] = 2
    return lengths


@pytest.mark.parametrize("letter", "SDCZ")
def test_chunk_and_group_edges_and_unaligned_destinations(gpu, letter):
    """The chunk width K is read from the library, so a new K fails the assertion here instead of leaving its edges untested.  The
    destination cols / vals start one element (8 bytes for the 16-byte type) behind a 16-byte boundary."""
    from spgpu_amd import capi, formats, synth
    K = capi.TO_CSR_FILL_CHUNK
    lengths = _edge_lengths()
    assert {0, 1, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 3 * K - 1, 3 * K, 3 * K + 1} <= set(lengths[:32].tolist())
    assert not lengths[32:64].any() and sorted(lengths[64:96].tolist())[-2:] == [0, 300]
    n = lengths.size
    _, _, r, c, v = synth.random_rows_coo(n, 500, lengths, seed=9, letter=letter, base=1)
    ell = formats.coo_to_ell(n, r, c, v, coo_base=1, ell_base=1)
    for hs in (32, 64):
        _expect(_to_csr(gpu, _hell_source(formats.ell_to_hell(ell, hs)), 0, misalign=True), *_csr_of(n, r, c, v, 1, 0), 300)
    _expect(_to_csr(gpu, _ell_source(ell, *_pitches(ell)), 1, misalign=True), *_csr_of(n, r, c, v, 1, 1), 300)
    rng = np.random.default_rng(8)
    for rows in (1, 31, 32, 33, 63, 64, 65):
        few = rng.integers(0, 40, rows)
        few[-1] = 37                                            # the last row of the matrix is not empty
        _, _, r, c, v = synth.random_rows_coo(rows, 90, few, seed=rows, letter=letter)
        ell = formats.coo_to_ell(rows, r, c, v)
        _expect(_to_csr(gpu, _hell_source(formats.ell_to_hell(ell, 32)), 1, misalign=True), *_csr_of(rows, r, c, v, 0, 1), int(few.max()))
        _expect(_to_csr(gpu, _ell_source(ell, *_pitches(ell)), 0, misalign=True), *_csr_of(rows, r, c, v, 0, 0), int(few.max()))


# ---- 3. bits, not numbers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SDZ")
def test_values_are_moved_as_bits(gpu, letter):
    """Random 32-, 64- and 128-bit patterns viewed as the type, with patterns of the type's OWN width planted (32-bit words for S,
    64-bit words for D and for both halves of Z): quiet and signalling NaNs with payloads of either sign, -0.0, +0.0, the smallest
    and the largest denormal of either sign, both infinities.  Each class is asserted present before the run; every CSR value is
    its slot's bytes."""
    from spgpu_amd import formats, synth
    rng = np.random.default_rng(900 + ord(letter))
    dtype = np.dtype(O.NP_DTYPE[letter])
    n = 150
    lengths = rng.integers(0, 40, n)
    lengths[0] = 12
    nnz = int(lengths.sum())
    words = rng.integers(0, 1 << 32, size=nnz * dtype.itemsize // 4, dtype=np.uint64).astype(np.uint32)
    if letter == "S":
        planted = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8ABCDE, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x007FFFFF,
                            0x80000001, 0x7F800000, 0xFF800000], np.uint32)
        words[:planted.size] = planted
        real = words.view(np.float32)
        tiny = np.finfo(np.float32).tiny
    else:
        planted = np.array([0x7FF8DEADBEEF0001, 0xFFF8000000012345, 0x7FF0000000000001, 0xFFF0000000000001, 0x8000000000000000,
                            0x0000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x000FFFFFFFFFFFFF, 0x8000000000000001,
                            0x7FF0000000000000, 0xFFF0000000000000], np.uint64)
        words.view(np.uint64)[:planted.size] = planted        # for Z: real and imaginary parts of the first six entries
        real = words.view(np.float64)
        tiny = np.finfo(np.float64).tiny
    head = real[:planted.size]
    with np.errstate(invalid="ignore"):
        assert int(np.isnan(head).sum()) == 4 and np.signbit(head[np.isnan(head)]).tolist() == [False, True, False, True]
        assert int(np.isposinf(head).sum()) == 1 and int(np.isneginf(head).sum()) == 1
        assert ((head == 0) & np.signbit(head)).sum() == 1 and ((head == 0) & ~np.signbit(head)).sum() == 1       # -0.0 and +0.0
        denormal = (head != 0) & (np.abs(head) < tiny)
        assert int(denormal.sum()) == 4 and int(np.signbit(head[denormal]).sum()) == 2
    assert head.view(planted.dtype).tolist() == planted.tolist()
    v = words.view(dtype)
    r = np.repeat(np.arange(n), lengths).astype(np.int32)
    c = rng.integers(0, 500, nnz).astype(np.int32)
    want = _csr_of(n, r, c, v, 0, 0)
    assert want[2].tobytes() == v.tobytes()                 # row-major listing: the CSR values are the listing's bytes
    ell = formats.coo_to_ell(n, r, c, v)
    hell = formats.ell_to_hell(ell, 32)
    k = np.arange(nnz) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    slot = hell["hack_offsets"].astype(np.int64)[r // 32] + r % 32 + k * 32
    assert hell["values"].view(np.uint8).reshape(-1, dtype.itemsize)[slot].tobytes() == v.tobytes()   # the source holds the bits
    _expect(_to_csr(gpu, _hell_source(hell), 0), *want, int(lengths.max()))
    _expect(_to_csr(gpu, _ell_source(ell, *_pitches(ell)), 0), *want, int(lengths.max()))


# ---- 4. padding is never read -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "DZ")
def test_padding_is_never_read(gpu, letter):
    """The same matrix with zeroed padding and with padding that would show: values a NaN pattern, indices 0x7fffffff or -5 (either
    would leave the column range; the index arithmetic on them would show in the output)."""
    from spgpu_amd import formats, synth
    rng = np.random.default_rng(12)
    n, hs = 200, 32
    lengths = rng.integers(0, 50, n)
    _, _, r, c, v = synth.random_rows_coo(n, 300, lengths, seed=4, letter=letter, base=1)
    want = _csr_of(n, r, c, v, 1, 0)
    ell = formats.coo_to_ell(n, r, c, v, coo_base=1, ell_base=1)
    hell = formats.ell_to_hell(ell, hs)
    rows = np.arange(n)
    depth = np.arange(int(hell["indices"].size) // hs + 1)
    stored_hell = np.zeros(hell["indices"].size, bool)
    stored_ell = np.zeros(ell["indices"].size, bool)
    for i in rows[lengths > 0]:
        stored_hell[int(hell["hack_offsets"][i // hs]) + i % hs + depth[:lengths[i]] * hs] = True
        stored_ell[i + depth[:lengths[i]] * ell["pitch"]] = True
    assert int(stored_hell.sum()) == int(lengths.sum()) == int(stored_ell.sum()) and not stored_hell.all()
    clean = _to_csr(gpu, _hell_source(hell), 0)
    _expect(clean, *want, int(lengths.max()))
    nan = np.frombuffer(np.array([0x7FF8DEADBEEF0001] * 2, np.uint64).tobytes(), dtype=v.dtype)[0]
    for poison in (0x7FFFFFFF, -5):
        dirty = dict(hell, values=hell["values"].copy(), indices=hell["indices"].copy())
        dirty["values"][~stored_hell], dirty["indices"][~stored_hell] = nan, poison
        got = _to_csr(gpu, _hell_source(dirty), 0)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, clean))
        dirty = dict(ell, values=ell["values"].copy(), indices=ell["indices"].copy())
        dirty["values"][~stored_ell], dirty["indices"][~stored_ell] = nan, poison
        src = _ell_source(dirty, *_pitches(ell))            # the columns the wider pitches add stay zero: beyond every row
        got = _to_csr(gpu, src, 0)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, clean))


# ---- 5. round trips on the device -------------------------------------------------------------------------------------
def _device_hell_of_csr(gpu, n, row_ptr, cols, vals, base, hs, d_ridx):
    """spgpuCsrRowLengthsDevice -> spgpuHellPlanDevice -> spgpuCsrToHellDevice on host CSR arrays: the HELL source in HBM."""
    import torch
    from spgpu_amd import capi, formats
    letter = formats.LETTER_OF[np.dtype(vals.dtype)]
    d_ptr, d_cols, d_vals = formats.to_device(row_ptr), formats.to_device(_some(cols)), formats.to_device(_some(vals))
    st, longest, rs = _row_lengths(gpu, n, d_ptr, base)
    assert st == capi.SPGPU_SUCCESS
    dest = rs if d_ridx is None else rs[d_ridx.long()].contiguous()     # plumbing: the lengths in storage order
    height, ho = _hell_plan(gpu, n, hs, dest)
    slots = hs * height
    hv, hi = _zeros(slots, vals.dtype), _zeros(slots, np.int32)
    torch.cuda.synchronize()
    assert _to_hell(gpu, None, hv, hi, ho, hs, base, n, d_ptr, d_cols.data_ptr(), d_vals.data_ptr(), base, capi.TYPE_CODE[letter],
                    d_ridx) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    return dict(kind="hell", dtype=np.dtype(vals.dtype), rows=n, base=base, hack_size=hs, slots=slots, cM=hv, rP=hi, hack_offsets=ho,
                rS=dest), rs


@pytest.mark.parametrize("order", ["as the rows come", "aligned order", "random permutation"])
def test_csr_to_hell_and_back_gives_the_callers_csr(gpu, order):
    import torch
    from spgpu_amd import capi, formats, synth
    n, base = 3001, 1
    lengths = synth.power_law_lengths(n, 9.0, 700, seed=21)
    lengths[::17] = 0
    _, _, r, c, v = synth.random_rows_coo(n, 4000, lengths, seed=22, letter="D", base=base)
    row_ptr, cols, vals = synth.coo_to_csr(n, r, c, v, base)
    d_ridx = None
    if order == "aligned order":
        st, _, rs = _row_lengths(gpu, n, formats.to_device(row_ptr), base)
        assert st == capi.SPGPU_SUCCESS
        order_work = torch.empty(capi.spgpuOellOrderWorkBytes(n), dtype=torch.uint8, device="cuda:0")
        d_ridx = torch.empty(n, dtype=torch.int32, device="cuda:0")
        sorted_lengths = torch.empty(n, dtype=torch.int32, device="cuda:0")
        assert capi.spgpuOellOrderAlignedDevice(gpu, _p(d_ridx), _p(sorted_lengths), _p(rs), n, 2048, 256, _p(order_work)) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        assert sorted(d_ridx.cpu().numpy().tolist()) == list(range(n))
    elif order == "random permutation":
        d_ridx = formats.to_device(np.random.default_rng(3).permutation(n).astype(np.int32))
    src, _ = _device_hell_of_csr(gpu, n, row_ptr, cols, vals, base, 32, d_ridx)
    _expect(_to_csr(gpu, src, base, r_idx=d_ridx), row_ptr, cols, vals, int(lengths.max()))


def test_hell_to_csr_and_back_gives_every_stored_slot(gpu):
    from spgpu_amd import formats, synth
    rng = np.random.default_rng(77)
    n, hs = 777, 24
    lengths = rng.integers(0, 60, n)
    _, _, r, c, v = synth.random_rows_coo(n, 900, lengths, seed=6, letter="C", shuffle=True)
    hell = formats.ell_to_hell(formats.coo_to_ell(n, r, c, v), hs)              # padding zeroed
    nnz, longest, row_ptr, cols, vals = _to_csr(gpu, _hell_source(hell), 0)
    back, rs = _device_hell_of_csr(gpu, n, row_ptr, cols, vals, 0, hs, None)
    assert rs.cpu().numpy()[:n].tobytes() == hell["row_lengths"].tobytes()
    assert back["slots"] == hell["indices"].size
    assert back["hack_offsets"].cpu().numpy()[:hell["hack_offsets"].size].tobytes() == hell["hack_offsets"].tobytes()
    assert back["rP"].cpu().numpy()[:back["slots"]].tobytes() == hell["indices"].tobytes()
    assert back["cM"].cpu().numpy()[:back["slots"]].tobytes() == hell["values"].tobytes()


# ---- 6. grid stride ---------------------------------------------------------------------------------------------------
def test_capped_grids_give_the_same_bytes(gpu):
    from spgpu_amd import capi, formats, synth
    rng = np.random.default_rng(61)
    n = 5000
    lengths = rng.integers(0, 41, n)
    _, _, r, c, v = synth.random_rows_coo(n, 7000, lengths, seed=62, letter="D")
    want = _csr_of(n, r, c, v, 0, 1)
    ell = formats.coo_to_ell(n, r, c, v)
    runs = ((None, 0),) + tuple((fill, cap) for fill in (capi.TO_CSR_FILL_PLAIN, capi.TO_CSR_FILL_TRANSPOSE) for cap in (0, 1, 3))
    _expect(_to_csr(gpu, _hell_source(formats.ell_to_hell(ell, 32)), 1, runs=runs), *want, int(lengths.max()))
    _expect(_to_csr(gpu, _ell_source(ell, *_pitches(ell)), 1, runs=runs), *want, int(lengths.max()))


# ---- 7. CSC through the transpose -------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "DC")
def test_csc_through_the_transpose(gpu, letter):
    """spgpuHellTransposeDevice, then these calls: the CSR arrays of A^T are the CSC arrays of A -- here by a stable sort of A's CSR
    entries by column."""
    from spgpu_amd import formats, synth
    rng = np.random.default_rng(70)
    n_rows, n_cols, base = 900, 650, 1
    lengths = rng.integers(0, 30, n_rows)
    _, _, r, c, v = synth.random_rows_coo(n_rows, n_cols, lengths, seed=71, letter=letter, base=base, shuffle=True)
    row_ptr, cols, vals = synth.coo_to_csr(n_rows, r, c, v, base)
    row_of = np.repeat(np.arange(n_rows), np.diff(row_ptr))
    by_col = np.argsort(cols, kind="stable")
    csc_ptr = np.zeros(n_cols + 1, np.int64)
    np.cumsum(np.bincount(cols - base, minlength=n_cols), out=csc_ptr[1:])
    src = _hell_source(formats.ell_to_hell(formats.coo_to_ell(n_rows, r, c, v, coo_base=base, ell_base=base), 32))
    t = formats.hell_transpose_device(gpu, src["cM"], src["rP"], src["hack_offsets"], src["rS"], None, n_rows, n_cols, 32, base,
                                      src["slots"], letter, t_hack_size=32, t_base=base)
    t_src = dict(kind="hell", dtype=src["dtype"], rows=n_cols, base=base, hack_size=32, slots=t["slots"], cM=t["cM"], rP=t["rP"],
                 hack_offsets=t["hack_offsets"], rS=t["rS"])
    _expect(_to_csr(gpu, t_src, base), (csc_ptr + base).astype(np.int32), (row_of[by_col] + base).astype(np.int32), vals[by_col],
            int(np.bincount(cols - base, minlength=n_cols).max()))


# ---- 8. one size with many workgroups -----------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "DS")
def test_300k_banded_rows_give_back_the_csr(gpu, letter):
    """300 000 rows x 32, banded: 9 375 row groups -- more workgroups than the chip holds at once.  The CSR arrays that
    spgpuCsrToHellDevice was given come back."""
    import torch
    from spgpu_amd import capi, formats, synth
    n, L = 300_000, 32
    _, cols_t, vals_t = synth.ragged_coo_on_device(np.full(n, L), n, "band", 0, letter, seed=3)
    d_ptr = torch.arange(0, (n + 1) * L, L, dtype=torch.int32, device="cuda:0")
    st, longest, rs = _row_lengths(gpu, n, d_ptr, 0)
    assert st == capi.SPGPU_SUCCESS and longest == L
    height, ho = _hell_plan(gpu, n, 32, rs)
    slots = 32 * height
    dtype = np.dtype(O.NP_DTYPE[letter])
    hv, hi = _zeros(slots, dtype), _zeros(slots, np.int32)
    torch.cuda.synchronize()
    assert _to_hell(gpu, None, hv, hi, ho, 32, 0, n, d_ptr, cols_t.data_ptr(), vals_t.data_ptr(), 0, capi.TYPE_CODE[letter],
                    None) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    src = dict(kind="hell", dtype=dtype, rows=n, base=0, hack_size=32, slots=slots, cM=hv, rP=hi, hack_offsets=ho, rS=rs)
    _expect(_to_csr(gpu, src, 0), d_ptr.cpu().numpy(), cols_t.cpu().numpy(), vals_t.cpu().numpy(), L)


# ---- 9. bad input -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hell", "ell"])
def test_bad_input_is_refused_and_nothing_else_is_written(gpu, kind):
    """The four refusals of the row-pointer call.  After each: SPGPU_UNSUPPORTED, both scalars 0, the guards around csrRowPtr intact
    and cols / vals -- never handed to a fill, as a caller would not after a refusal -- still their fill pattern."""
    import torch
    from spgpu_amd import capi, formats, synth
    rng = np.random.default_rng(91)
    n = 130
    lengths = rng.integers(1, 20, n)
    lengths[5] = 25                                            # the longest row: its last slot is the deepest of its hack
    _, _, r, c, v = synth.random_rows_coo(n, 200, lengths, seed=92, letter="D")
    ell = formats.coo_to_ell(n, r, c, v)
    good = _hell_source(formats.ell_to_hell(ell, 32)) if kind == "hell" else _ell_source(ell, *_pitches(ell))
    identity = np.arange(n, dtype=np.int32)
    _expect(_to_csr(gpu, good, 0, r_idx=identity), *_csr_of(n, r, c, v, 0, 0), 25)      # the source itself is accepted

    def spoil(what):
        rs, r_idx, slots = lengths.astype(np.int32), identity.copy(), good["slots"]
        if what == "negative rS":
            rs[17] = -1
        elif what == "rS beyond slots":
            rs[n - 1] = 10**6                                   # (10^6 - 1) steps of at least 32 slots: beyond any `slots` here
        elif what == "rS one slot too deep":
            # one slab column fewer than the source has: the longest row of the last hack (ELL: of the matrix) ends in it
            slots = good["slots"] - (32 if kind == "hell" else good["indices_pitch"])
        elif what == "rIdx out of range":
            r_idx[40] = n
        elif what == "rIdx negative":
            r_idx[0] = -1
        elif what == "rIdx repeated":
            r_idx[99] = r_idx[3]
        return rs, r_idx, slots

    for what in ("negative rS", "rS beyond slots", "rS one slot too deep", "rIdx out of range", "rIdx negative", "rIdx repeated"):
        rs, r_idx, slots = spoil(what)
        src = dict(good, rS=formats.to_device(rs))
        # a spoilt rS is refused with the (identity) row order and without one; a spoilt rIdx needs the order
        orders = (formats.to_device(r_idx), None) if "rS" in what else (formats.to_device(r_idx),)
        for d_ridx in orders:
            work = torch.empty(capi.spgpuToCsrWorkBytes(n), dtype=torch.uint8, device="cuda:0")
            row_ptr, cols, vals = _Guarded((n + 1) * 4), _Guarded(int(lengths.sum()) * 4), _Guarded(int(lengths.sum()) * 8)
            nnz, longest = C.c_int(-1), C.c_int(-1)
            torch.cuda.synchronize()
            st = _row_ptr_call(gpu, src, 1, d_ridx, row_ptr, nnz, longest, work, slots=slots)
            torch.cuda.synchronize()
            assert st == capi.SPGPU_UNSUPPORTED and nnz.value == 0 and longest.value == 0, (what, d_ridx is None)
            assert row_ptr.guards_intact() and cols.untouched() and vals.untouched(), (what, d_ridx is None)
    # the same source is still accepted afterwards, and without a row order
    _expect(_to_csr(gpu, good, 1), *_csr_of(n, r, c, v, 0, 1), 25)
    # an element size that is not 4, 8 or 16 (no such type code): refused before anything is launched
    row_ptr = _Guarded((n + 1) * 4)
    for code in (5, -1):
        assert capi.spgpuSizeOf(code) == 0
        if kind == "hell":
            st = capi.spgpuHellToCsrDevice(gpu, None, None, row_ptr.ptr(), 0, None, None, 32, _p(good["hack_offsets"]), _p(good["rS"]), None,
                                           n, 0, code)
        else:
            st = capi.spgpuEllToCsrDevice(gpu, None, None, row_ptr.ptr(), 0, None, None, good["values_pitch"], good["indices_pitch"],
                                          _p(good["rS"]), None, n, 0, code)
        assert st == capi.SPGPU_UNSUPPORTED
