"""GPU: new coefficients for a stored HELL / ELL matrix (include/spgpu/ext/update_device.h).

The value refill is held to the full fill of include/spgpu/ext/csr_device.h byte for byte: every value buffer lies between 64
guard bytes, is poisoned as a whole with one byte pattern, is built from values V1 by the full fill and refilled from V2 -- by the
public call and by each of the two refills behind it -- and must then equal (a) numpy's restatement of the contract and (b) the
full fill from V2 into an equally poisoned buffer, guards and padding included; rP must not change.  spgpu?hellcsput is held to
numpy's restatement of spgpu?ellcsput's contract on HELL storage and, in one case, to spgpu?ellcsput itself.  A frozen matrix
takes new values with no Thaw, and refill -> SpMV replays from a captured graph."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
from test_gpu_csr_device import _p, _upload
from test_gpu_to_csr_device import PATTERN, _Guarded

pytestmark = pytest.mark.gpu

CODE_OF_SIZE = {4: 1, 8: 2, 16: 4}        # TYPE_FLOAT, TYPE_DOUBLE, TYPE_COMPLEX_DOUBLE: only the element size matters to the refill
# (csrBaseIndex, csrValues one element behind a 16-byte boundary, cM one element (at most 8 bytes) behind one, ELL pitch odd):
# an aligned cM with hackSize % 32 == 0 (ELL: a pitch that is a multiple of 16 bytes) takes the 16-byte stores, the others the
# element stores
VARIANTS = ((0, False, False, False), (1, True, False, True), (1, False, True, False), (0, True, True, True))


def _bits(rng, count, size, plant=True):
    """`count` elements of `size` bytes as rows of bytes: random bits, with (plant) NaNs that carry payloads (quiet and signalling, both
    signs) and -0.0 planted in the element type's own word width (both halves of the 16-byte type)."""
    words = rng.integers(0, 1 << 32, size=max(count, 1) * size // 4, dtype=np.uint64).astype(np.uint32)
    if not plant:
        return words.view(np.uint8).reshape(-1, size)[:count]
    if size == 4:
        planted = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000], np.uint32)
        words[:min(planted.size, words.size)] = planted[:words.size]
    else:
        planted = np.array([0x7FF8DEADBEEF0001, 0xFFF8000000012345, 0x7FF0000000000001, 0x8000000000000000], np.uint64)
        wide = words.view(np.uint64)
        wide[:min(planted.size, wide.size)] = planted[:wide.size]
    return words.view(np.uint8).reshape(-1, size)[:count]


def _lengths(kind, rows, rng):
    if kind == "uniform":
        return np.full(rows, 3, np.int64)
    if kind == "empty":
        return np.zeros(rows, np.int64)
    lengths = rng.integers(1, 9, rows)
    lengths[::3] = 0                                           # empty rows ...
    lengths[rows // 2] = 257                                   # ... and one row of 257 entries: 17 chunks of 16 slab columns
    return lengths


def _order(kind, gpu, rows, lengths, rng):
    """rIdx as numpy (None: no order).  'oell': from spgpuOellOrderDevice on the lengths; 'bad': a permutation with one entry out of
    range."""
    import torch
    from spgpu_amd import capi, formats
    if kind == "none":
        return None
    if kind == "reversed":
        return np.arange(rows, dtype=np.int32)[::-1].copy()
    if kind == "bad":
        r_idx = rng.permutation(rows).astype(np.int32)
        r_idx[rows // 2] = rows if rows % 2 else -1
        return r_idx
    src = formats.to_device(lengths.astype(np.int32))
    d_ridx = torch.full((rows,), -9, dtype=torch.int32, device="cuda:0")
    dst = torch.empty(rows, dtype=torch.int32, device="cuda:0")
    work = torch.empty(max(capi.spgpuOellOrderWorkBytes(rows), 16), dtype=torch.uint8, device="cuda:0")
    assert capi.spgpuOellOrderDevice(gpu, _p(d_ridx), _p(dst), _p(src), rows, 0, 0, _p(work)) == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    r_idx = d_ridx.cpu().numpy()
    assert sorted(r_idx.tolist()) == list(range(rows))
    return r_idx


def _layout(rows, hack_size, dest_lengths):
    """hackOffsets (as computeHellAllocSize / spgpuHellPlanDevice give them) and the slot count, in numpy."""
    hacks = (rows + hack_size - 1) // hack_size
    padded = np.zeros(hacks * hack_size, np.int64)
    padded[:rows] = dest_lengths
    depth = padded.reshape(hacks, hack_size).max(axis=1)
    offsets = np.concatenate(([0], np.cumsum(depth * hack_size)))
    return offsets[:hacks].astype(np.int32), int(offsets[hacks])


def _expected(guarded_bytes, first, size, first_slot, stride, dest_lengths, dest_start, values):
    """numpy's statement of the contract: the whole guarded buffer -- PATTERN everywhere but slot k of destination row i (at
    first_slot[i] + k * stride), which holds entry dest_start[i] + k of `values`."""
    out = np.full(guarded_bytes, PATTERN, np.uint8)
    total = int(dest_lengths.sum())
    if total:
        row = np.repeat(np.arange(dest_lengths.size), dest_lengths)
        k = np.arange(total) - np.repeat(np.cumsum(dest_lengths) - dest_lengths, dest_lengths)
        slot = first_slot[row] + k * stride
        assert np.unique(slot).size == total
        byte = (first + slot * size)[:, None] + np.arange(size)[None, :]
        out[byte] = values[dest_start[row] + k]
    return out


@pytest.mark.parametrize("hack_size", [32, 64, 5])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 97, 300])
def test_refill_writes_the_bytes_of_the_full_fill_and_nothing_else(gpu, rows, hack_size):
    """Row lengths x row order x element size x (base, alignments): HELL at this hackSize, and -- once per row count -- ELL."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(1000 * rows + hack_size)
    for kind in ("uniform", "ragged", "empty"):
        lengths = _lengths(kind, rows, rng)
        nnz = int(lengths.sum())
        for order in ("none", "oell", "reversed", "bad"):
            r_idx = _order(order, gpu, rows, lengths, rng)
            source = np.arange(rows) if r_idx is None else r_idx.astype(np.int64)
            valid = (source >= 0) & (source < rows)
            dest_lengths = np.where(valid, lengths[np.clip(source, 0, rows - 1)], 0)
            starts = np.cumsum(lengths) - lengths
            dest_start = np.where(valid, starts[np.clip(source, 0, rows - 1)], 0)
            assert (order == "bad") == (not valid.all())
            d_ridx = None if r_idx is None else formats.to_device(r_idx)
            cols = rng.integers(0, 1000, max(nnz, 1)).astype(np.int32)
            for size in (4, 8, 16):
                v1, v2 = _bits(rng, nnz, size, plant=False), _bits(rng, nnz, size)
                for base, csr_off, cm_off, odd_pitch in VARIANTS:
                    d_ptr = formats.to_device((np.concatenate(([0], np.cumsum(lengths))) + base).astype(np.int32))
                    cols_buf, cols_at = _upload(cols + base)
                    off = min(size, 8) if csr_off else 0
                    v1_buf, v1_at = _upload(v1, off)
                    v2_buf, v2_at = _upload(v2, off)
                    assert (v2_at % 16 == off) and v2_at % min(size, 8) == 0
                    cm_shift = min(size, 8) if cm_off else 0
                    targets = []
                    offsets, slots = _layout(rows, hack_size, dest_lengths)
                    first_slot = offsets.astype(np.int64)[np.arange(rows) // hack_size] + np.arange(rows) % hack_size
                    targets.append(("hell", slots, first_slot, hack_size, formats.to_device(offsets)))
                    if hack_size == 32:
                        pitch = rows + 1 + rows % 2 if odd_pitch else (rows + 31) // 32 * 32
                        assert pitch % 2 == (1 if odd_pitch else 0) and pitch >= rows
                        targets.append(("ell", pitch * int(dest_lengths.max()), np.arange(rows, dtype=np.int64), pitch, None))
                    for fmt, slots, first_slot, stride, d_offsets in targets:
                        case = (fmt, kind, order, size, base, csr_off, cm_off, odd_pitch)

                        def full_fill(values_at):
                            cm, rp = _Guarded(slots * size, cm_shift), _Guarded(slots * 4)
                            if fmt == "hell":
                                st = capi.spgpuCsrToHellDevice(gpu, cm.ptr(), rp.ptr(), _p(d_offsets), hack_size, base, rows, _p(d_ptr),
                                                               C.c_void_p(cols_at), C.c_void_p(values_at), base, CODE_OF_SIZE[size], _p(d_ridx))
                            else:
                                st = capi.spgpuCsrToEllDevice(gpu, cm.ptr(), rp.ptr(), stride, stride, base, rows, _p(d_ptr),
                                                              C.c_void_p(cols_at), C.c_void_p(values_at), base, CODE_OF_SIZE[size], _p(d_ridx))
                            assert st == capi.SPGPU_SUCCESS, case
                            return cm, rp

                        built, rp = full_fill(v1_at)                   # steps 1 and 2: poisoned, then built from V1
                        reference, _ = full_fill(v2_at)                # the parent's call on V2, into an equally poisoned buffer
                        torch.cuda.synchronize()
                        rp_before = rp.buf.clone()
                        want = _expected(built.buf.numel(), built.first, size, first_slot, stride, dest_lengths, dest_start, v2)
                        for fill in (None, capi.UPDATE_FILL_PLAIN, capi.UPDATE_FILL_TRANSPOSE):
                            cm = _Guarded(slots * size, cm_shift)
                            cm.buf.copy_(built.buf)
                            if fmt == "hell":
                                args = (gpu, cm.ptr(), _p(d_offsets), hack_size, rows, _p(d_ptr), C.c_void_p(v2_at), base, CODE_OF_SIZE[size],
                                        _p(d_ridx))
                                st = capi.spgpuCsrToHellValuesDevice(*args) if fill is None else capi.spgpuCsrToHellValuesDeviceWith(*args, fill, 0)
                            else:
                                args = (gpu, cm.ptr(), stride, rows, _p(d_ptr), C.c_void_p(v2_at), base, CODE_OF_SIZE[size], _p(d_ridx))
                                st = capi.spgpuCsrToEllValuesDevice(*args) if fill is None else capi.spgpuCsrToEllValuesDeviceWith(*args, fill, 0)
                            assert st == capi.SPGPU_SUCCESS, (case, fill)
                            torch.cuda.synchronize()
                            assert torch.equal(cm.buf, reference.buf), (case, fill)        # the full fill's bytes, guards and padding included
                            assert torch.equal(rp.buf, rp_before), (case, fill)            # rP byte for byte
                            if fill is None:
                                got = cm.buf.cpu().numpy()
                                assert got.tobytes() == want.tobytes(), case               # live slots V2's bits, every other byte the poison
                        if nnz and valid.any() and dest_lengths.sum():
                            assert not torch.equal(built.buf, reference.buf), case         # V1 and V2 differ: the refill had work to do
                    del cols_buf, v1_buf, v2_buf


def test_refill_with_a_capped_grid_strides_over_the_groups(gpu):
    """3 000 rows on a grid of one and of three workgroups (the grid stride of both refills), ragged, in the aligned order."""
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(5)
    rows, hs, size = 3000, 32, 8
    lengths = rng.integers(0, 40, rows)
    r_idx = rng.permutation(rows).astype(np.int32)
    dest_lengths = lengths[r_idx]
    dest_start = (np.cumsum(lengths) - lengths)[r_idx]
    nnz = int(lengths.sum())
    offsets, slots = _layout(rows, hs, dest_lengths)
    first_slot = offsets.astype(np.int64)[np.arange(rows) // hs] + np.arange(rows) % hs
    v2 = _bits(rng, nnz, size)
    d_ptr = formats.to_device(np.concatenate(([0], np.cumsum(lengths))).astype(np.int32))
    d_vals, d_off, d_ridx = formats.to_device(v2.reshape(-1).view(np.uint64)), formats.to_device(offsets), formats.to_device(r_idx)
    want = None
    for fill in (capi.UPDATE_FILL_PLAIN, capi.UPDATE_FILL_TRANSPOSE):
        for cap in (0, 1, 3):
            cm = _Guarded(slots * size)
            assert capi.spgpuCsrToHellValuesDeviceWith(gpu, cm.ptr(), _p(d_off), hs, rows, _p(d_ptr), _p(d_vals), 0, capi.TYPE_DOUBLE,
                                                       _p(d_ridx), fill, cap) == capi.SPGPU_SUCCESS
            torch.cuda.synchronize()
            if want is None:
                want = _expected(cm.buf.numel(), cm.first, size, first_slot, hs, dest_lengths, dest_start, v2)
            assert cm.buf.cpu().numpy().tobytes() == want.tobytes(), (fill, cap)


# ---- csput ------------------------------------------------------------------------------------------------------------
def _csput_matrix(rng, rows, cols, base):
    """Row lengths 0, 1, 2, 3 and 64 in turn; columns ascending within each row (in `base`)."""
    lengths = np.array([0, 1, 2, 3, 64])[np.arange(rows) % 5]
    columns = [np.sort(rng.choice(cols, n, replace=False)).astype(np.int32) + base for n in lengths]
    return lengths, columns


def _csput_list(rng, lengths, columns, rows, cols, base, blocked_row):
    """(aI, aJ, hits): a shuffled list without duplicate targets that names the first and the last slot of every row that has one,
    a few slots inside the long rows, columns that are not stored (also in an empty row), rows below the base, a row beyond the
    matrix, and -- all slots of matrix row `blocked_row`, whose rowOf entry the caller has put out of range (None: no such row).
    hits[i] is the slot index k that entry i must overwrite, or -1 when it must be ignored."""
    a_i, a_j, hits = [], [], []
    for i in range(rows):
        n = int(lengths[i])
        ks = sorted({0, n - 1} | ({5, 31, 32, 62} if n == 64 else set())) if n else []
        if i == blocked_row:
            ks = list(range(n))
        for k in ks:
            a_i.append(i + base), a_j.append(int(columns[i][k])), hits.append(-1 if i == blocked_row else k)
        stored = set(columns[i].tolist())
        missing = next(c for c in range(base, base + cols) if c not in stored)
        a_i.append(i + base), a_j.append(missing), hits.append(-1)
    for below in (base - 1, base - 5):
        a_i.append(below), a_j.append(int(columns[1][0])), hits.append(-1)
    a_i.append(rows + 3 + base), a_j.append(base), hits.append(-1)
    shuffle = rng.permutation(len(a_i))
    return np.array(a_i, np.int32)[shuffle], np.array(a_j, np.int32)[shuffle], np.array(hits)[shuffle]


@pytest.mark.parametrize("ordered", [False, True], ids=["natural", "rowOf"])
@pytest.mark.parametrize("hack_size", [32, 5])
@pytest.mark.parametrize("letter", "SDCZ")
def test_hellcsput_overwrites_what_numpy_overwrites(gpu, letter, hack_size, ordered):
    import torch
    from spgpu_amd import capi, formats
    rng = np.random.default_rng(ord(letter) * 100 + hack_size + ordered)
    rows, cols, base = 70, 200, 1
    dtype = np.dtype(X.DTYPE_OF[letter])
    size = dtype.itemsize
    lengths, columns = _csput_matrix(rng, rows, cols, base)
    # storage row r holds matrix row r_idx[r]; row_of is its inverse, built on the device and checked against numpy
    r_idx = rng.permutation(rows).astype(np.int32) if ordered else np.arange(rows, dtype=np.int32)
    row_of = np.empty(rows, np.int32)
    row_of[r_idx] = np.arange(rows, dtype=np.int32)
    blocked = None
    d_row_of = None
    if ordered:
        spoilt = r_idx.copy()
        spoilt[7], spoilt[8] = rows, -1                                       # skipped: their rowOf entries keep the fill value
        d_row_of = torch.full((rows,), -77, dtype=torch.int32, device="cuda:0")
        assert capi.spgpuInvertRowOrderDevice(gpu, _p(d_row_of), _p(formats.to_device(spoilt)), rows) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        want_inverse = row_of.copy()
        want_inverse[r_idx[7]], want_inverse[r_idx[8]] = -77, -77
        assert d_row_of.cpu().numpy().tobytes() == want_inverse.tobytes()
        assert capi.spgpuInvertRowOrderDevice(gpu, _p(d_row_of), _p(formats.to_device(r_idx)), rows) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        assert d_row_of.cpu().numpy().tobytes() == row_of.tobytes()
        blocked = next(int(m) for m in r_idx if lengths[m] == 64)              # a long matrix row whose rowOf entry goes out of range
        d_row_of[blocked] = rows + 5
    storage_lengths = lengths[r_idx]
    offsets, slots = _layout(rows, hack_size, storage_lengths)
    first_slot = offsets.astype(np.int64)[np.arange(rows) // hack_size] + np.arange(rows) % hack_size
    # the stored arrays in numpy: padding of cM and rP is the poison
    cm_host = np.full(slots * size, PATTERN, np.uint8).view(dtype)
    rp_host = np.full(slots * 4, PATTERN, np.uint8).view(np.int32)
    real = np.float32 if size in (4, 8) and letter in "SC" else np.float64
    for r in range(rows):
        m, n = int(r_idx[r]), int(storage_lengths[r])
        at = first_slot[r] + np.arange(n) * hack_size
        rp_host[at] = columns[m]
        cm_host[at] = (rng.standard_normal(2 * n).astype(real).view(dtype) if letter in "CZ" else rng.standard_normal(n).astype(real))[:n]
    a_i, a_j, hits = _csput_list(rng, lengths, columns, rows, cols, base, blocked)
    a_val = (rng.standard_normal(2 * a_i.size).astype(real).view(dtype) if letter in "CZ" else rng.standard_normal(a_i.size).astype(real))
    assert (hits >= 0).sum() >= 2 * (lengths > 1).sum() and (hits < 0).sum() > rows
    want = cm_host.copy()
    for i in np.flatnonzero(hits >= 0):
        want[first_slot[row_of[a_i[i] - base]] + hits[i] * hack_size] = a_val[i]
    assert want.tobytes() != cm_host.tobytes()
    cm, rp = _Guarded(slots * size), _Guarded(slots * 4)
    cm.buf[cm.first:cm.first + cm.nbytes] = torch.from_numpy(cm_host.view(np.uint8).copy()).to("cuda:0")
    rp.buf[rp.first:rp.first + rp.nbytes] = torch.from_numpy(rp_host.view(np.uint8).copy()).to("cuda:0")
    rp_before = rp.buf.clone()
    d_off, d_rs = formats.to_device(offsets), formats.to_device(storage_lengths.astype(np.int32))
    d_ai, d_aj, d_av = formats.to_device(a_i), formats.to_device(a_j), formats.to_device(a_val)
    torch.cuda.synchronize()
    capi.hellcsput[letter](gpu, capi.scalar(letter, 3.5), cm.ptr(), rp.ptr(), hack_size, _p(d_off), _p(d_rs), _p(d_row_of), rows, a_i.size,
                           _p(d_ai), _p(d_aj), _p(d_av), base)              # alpha 3.5: accepted and not applied
    torch.cuda.synchronize()
    assert cm.guards_intact() and torch.equal(rp.buf, rp_before)
    assert cm.numpy(dtype).tobytes() == want.tobytes()

    if letter == "D" and hack_size == 32 and not ordered:
        # the same matrix held as ELL, the same list without the row beyond the matrix (spgpu?ellcsput does not check it)
        keep = a_i - base < rows
        pitch = 96
        depth = int(lengths.max())
        ell_cm, ell_rp = np.zeros(pitch * depth, dtype), np.zeros(pitch * depth, np.int32)
        for r in range(rows):
            at = r + np.arange(int(lengths[r])) * pitch
            ell_rp[at] = columns[r]
            ell_cm[at] = cm_host[first_slot[r] + np.arange(int(lengths[r])) * hack_size]
        d_cm, d_rp = formats.to_device(ell_cm), formats.to_device(ell_rp)
        d_ai, d_aj, d_av = formats.to_device(a_i[keep]), formats.to_device(a_j[keep]), formats.to_device(a_val[keep])
        capi.ellcsput["D"](gpu, capi.scalar("D", 3.5), _p(d_cm), _p(d_rp), pitch, pitch, _p(d_rs), int(keep.sum()), _p(d_ai), _p(d_aj),
                           _p(d_av), base)
        torch.cuda.synchronize()
        ell_after = d_cm.cpu().numpy()
        for r in range(rows):
            k = np.arange(int(lengths[r]))
            assert ell_after[r + k * pitch].tobytes() == want[first_slot[r] + k * hack_size].tobytes(), r


# ---- a frozen matrix takes new values with no Thaw; refill -> SpMV in a captured graph ----------------------------------------
def _banded(rows, width, base):
    """CSR of a banded matrix, `width` ascending columns per row; three sets of values."""
    rng = np.random.default_rng(77)
    row_ptr = (np.arange(rows + 1) * width + base).astype(np.int32)
    cols = (np.arange(rows)[:, None] + np.arange(width)[None, :]).reshape(-1).astype(np.int32) + base
    return row_ptr, cols, [rng.standard_normal(rows * width) for _ in range(3)]


def _build_hell(gpu, rows, hs, base, d_ptr, d_cols, d_vals):
    import torch
    from spgpu_amd import capi, formats
    lengths = np.diff(d_ptr.cpu().numpy())
    offsets, slots = _layout(rows, hs, lengths)
    mat = dict(cM=torch.zeros(slots, dtype=torch.float64, device="cuda:0"), rP=torch.zeros(slots, dtype=torch.int32, device="cuda:0"),
               ho=formats.to_device(offsets), rS=formats.to_device(lengths.astype(np.int32)))
    assert all(mat[k].data_ptr() % 16 == 0 for k in mat)
    assert capi.spgpuCsrToHellDevice(gpu, _p(mat["cM"]), _p(mat["rP"]), _p(mat["ho"]), hs, base, rows, _p(d_ptr), _p(d_cols), _p(d_vals), base,
                                     capi.TYPE_DOUBLE, None) == capi.SPGPU_SUCCESS
    return mat


def _spmv(gpu, mat, hs, rows, dx, dy, dz, base):
    from spgpu_amd import capi
    capi.hellspmv["D"](gpu, _p(dz), _p(dy), capi.scalar("D", 1.25), _p(mat["cM"]), _p(mat["rP"]), hs, _p(mat["ho"]), _p(mat["rS"]), None, 0, rows,
                       _p(dx), capi.scalar("D", -0.5), base)


def test_a_frozen_matrix_takes_new_values_with_no_thaw(gpu):
    import torch
    from spgpu_amd import capi, formats
    rows, width, hs, base = 512, 8, 32, 1
    row_ptr, cols, (v1, v2, v3) = _banded(rows, width, base)
    d_ptr, d_cols = formats.to_device(row_ptr), formats.to_device(cols)
    d_v1, d_v2 = formats.to_device(v1), formats.to_device(v2)
    rng = np.random.default_rng(78)
    x, y = rng.standard_normal(rows + width), rng.standard_normal(rows)
    dx, dy = formats.to_device(x), formats.to_device(y)
    frozen = _build_hell(gpu, rows, hs, base, d_ptr, d_cols, d_v1)
    twin = _build_hell(gpu, rows, hs, base, d_ptr, d_cols, d_v2)            # never frozen; holds the new values from the start
    torch.cuda.synchronize()
    assert capi.spgpuHellSpmvFreeze(gpu, capi.TYPE_DOUBLE, _p(frozen["cM"]), _p(frozen["rP"]), hs, _p(frozen["ho"]), _p(frozen["rS"]), None, rows,
                                    base) == capi.SPGPU_SUCCESS
    try:
        coo_rows = np.repeat(np.arange(rows), width) + base
        # a list for spgpuDhellcsput: every other entry, back to front
        picked = np.arange(rows * width)[::2][::-1].copy()
        a_i, a_j, a_v = coo_rows[picked].astype(np.int32), cols[picked], v3[picked]
        after_list = v2.copy()
        after_list[picked] = a_v
        d_ai, d_aj, d_av = formats.to_device(a_i), formats.to_device(a_j), formats.to_device(a_v)
        for stage, values in (("refill", v2), ("csput", after_list)):
            for mat in (frozen, twin):
                if stage == "refill" and mat is frozen:
                    assert capi.spgpuCsrToHellValuesDevice(gpu, _p(mat["cM"]), _p(mat["ho"]), hs, rows, _p(d_ptr), _p(d_v2), base, capi.TYPE_DOUBLE,
                                                           None) == capi.SPGPU_SUCCESS
                if stage == "csput":
                    capi.hellcsput["D"](gpu, capi.scalar("D", 1.0), _p(mat["cM"]), _p(mat["rP"]), hs, _p(mat["ho"]), _p(mat["rS"]), None, rows,
                                        a_i.size, _p(d_ai), _p(d_aj), _p(d_av), base)
            uses = capi.plan_counts(gpu)[0]
            z_frozen, z_twin = torch.full((rows,), float("nan"), dtype=torch.float64, device="cuda:0"), torch.zeros(rows, dtype=torch.float64, device="cuda:0")
            _spmv(gpu, frozen, hs, rows, dx, dy, z_frozen, base)            # no Thaw in between
            assert capi.plan_counts(gpu)[0] == uses + 1, stage              # it ran from the frozen record
            _spmv(gpu, twin, hs, rows, dx, dy, z_twin, base)
            torch.cuda.synchronize()
            assert torch.equal(frozen["cM"], twin["cM"]), stage
            got = z_frozen.cpu().numpy()
            assert got.tobytes() == z_twin.cpu().numpy().tobytes(), stage
            want, scale = X.spmv(rows, coo_rows, cols, values, x, y, 1.25, -0.5, base=base)
            X.assert_within(got, want, scale, "D", stage)
    finally:
        assert capi.spgpuSpmvThaw(gpu, _p(frozen["rP"])) == capi.SPGPU_SUCCESS


def test_refill_then_spmv_replays_from_a_captured_graph(gpu):
    """refill -> spgpuDhellspmv as one linear chain on the handle's stream, replayed twice with csrValues rewritten in between: each
    replay gives the bits of the eager pair of calls on the same values."""
    import torch
    from spgpu_amd import capi, formats
    rows, width, hs, base = 512, 8, 32, 0
    row_ptr, cols, (v1, v2, v3) = _banded(rows, width, base)
    d_ptr, d_cols = formats.to_device(row_ptr), formats.to_device(cols)
    d_vals = formats.to_device(v1)
    rng = np.random.default_rng(79)
    dx, dy = formats.to_device(rng.standard_normal(rows + width)), formats.to_device(rng.standard_normal(rows))
    mat = _build_hell(gpu, rows, hs, base, d_ptr, d_cols, d_vals)
    dz = torch.zeros(rows, dtype=torch.float64, device="cuda:0")

    def chain():
        assert capi.spgpuCsrToHellValuesDevice(gpu, _p(mat["cM"]), _p(mat["ho"]), hs, rows, _p(d_ptr), _p(d_vals), base, capi.TYPE_DOUBLE,
                                               None) == capi.SPGPU_SUCCESS
        _spmv(gpu, mat, hs, rows, dx, dy, dz, base)

    eager = []
    for values in (v2, v3):
        d_vals.copy_(formats.to_device(values))
        torch.cuda.synchronize()
        chain()
        torch.cuda.synchronize()
        eager.append(dz.cpu().numpy().tobytes())
    assert eager[0] != eager[1]
    side = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            chain()
        for values, want in zip((v2, v3), eager):
            d_vals.copy_(formats.to_device(values))
            mat["cM"].fill_(float("nan"))
            dz.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert dz.cpu().numpy().tobytes() == want
    finally:
        capi.spgpuSetStream(gpu, None)
